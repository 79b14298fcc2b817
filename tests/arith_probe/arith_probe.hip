// arith_probe.hip — TEST INFRASTRUCTURE: the arithmetic forms of hc_arith.h and the butterflies and radix-16 rounds of hc_kernels.h, one call each per element, so that
// tests/arith_cases.py can feed them the operands at which their stated lazy-reduction bounds are tight and compare every result with Python's integers. Never linked into
// libhconv.so. Two builds of this one source (tests/arith_probe/Makefile): hipcc for gfx950 (the code the product runs) and g++ -DHC_EMU against tests/kernel_emu (the host twin).
//
// One kernel per operation, one thread per element (rounds: one thread per 16-element tile). Every array is n items of a fixed width in 8-byte words; 32-bit values and doubles
// travel in 8-byte words (the low word, the bit pattern). The modulus and its constants are kernel arguments: uniform, as hc_q wants them.
#ifdef HC_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "hc_kernels.h"

#define AP_MAXARR 8
struct ApArgs {
    u64 p[8];                       // per operation: p[0] = q, then what the operation's comment says
    const u64 *in[AP_MAXARR];
    u64 *out[AP_MAXARR];
    u64 n;
};
struct ApTw { const u64 *p; __device__ __forceinline__ HcTw operator()(int slot) const { HcTw t; t.w = p[2 * slot]; t.ws = p[2 * slot + 1]; return t; } };
struct ApTw32 { const u64 *p; __device__ __forceinline__ HcTw32 operator()(int slot) const { HcTw t; t.w = p[2 * slot]; t.ws = p[2 * slot + 1]; return hc_tw32(t); } };

#define AP_KERNEL(name) __global__ void ap_k_##name(ApArgs a)
#define AP_INDEX() const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; if (i >= a.n) return
#define AP_TW(k, l) HcTw{a.in[k][i], a.in[l][i]}

AP_KERNEL(mulhi_lo2) { AP_INDEX(); a.out[0][i] = hc_mulhi_lo2(a.in[0][i], a.in[1][i]); }
AP_KERNEL(mulhi) { AP_INDEX(); a.out[0][i] = hc_mulhi(a.in[0][i], a.in[1][i]); }
AP_KERNEL(shoup_companion) { AP_INDEX(); a.out[0][i] = hc_shoup_companion(a.in[0][i], a.p[0]); }
AP_KERNEL(shoup4) { AP_INDEX(); const HcQ Q = hc_q(a.p[0]); a.out[0][i] = hc_shoup4(a.in[0][i], a.in[1][i], a.in[2][i], Q); }
AP_KERNEL(mul_shoup_lazy) { AP_INDEX(); a.out[0][i] = hc_mul_shoup_lazy(a.in[0][i], a.in[1][i], a.in[2][i], a.p[0]); }
AP_KERNEL(mul_shoup) { AP_INDEX(); a.out[0][i] = hc_mul_shoup(a.in[0][i], a.in[1][i], a.in[2][i], a.p[0]); }
AP_KERNEL(fold) { AP_INDEX(); a.out[0][i] = hc_fold(a.in[0][i], a.p[1]); }                                                         // p[1] = 2^64 - b
AP_KERNEL(canon4) { AP_INDEX(); const HcQ Q = hc_q(a.p[0]); a.out[0][i] = hc_canon4(a.in[0][i], Q); }
AP_KERNEL(canon8) { AP_INDEX(); const HcQ Q = hc_q(a.p[0]); a.out[0][i] = hc_canon8(a.in[0][i], Q); }
AP_KERNEL(reduce64) { AP_INDEX(); const HcQ Q = hc_q(a.p[0]); a.out[0][i] = hc_reduce64(a.in[0][i], a.p[1], Q); }                  // p[1] = mu
AP_KERNEL(addmod) { AP_INDEX(); a.out[0][i] = hc_addmod(a.in[0][i], a.in[1][i], a.p[0]); a.out[1][i] = hc_submod(a.in[0][i], a.in[1][i], a.p[0]); }
AP_KERNEL(mont) { AP_INDEX(); a.out[0][i] = hc_mont(a.in[0][i], a.in[1][i], a.p[0], a.p[1]); }                                     // p[1] = q^-1 mod 2^64
AP_KERNEL(mont_lazy) { AP_INDEX(); a.out[0][i] = hc_mont_lazy(a.in[0][i], a.in[1][i], a.p[0], a.p[1]); }
AP_KERNEL(mont_redc) { AP_INDEX(); a.out[0][i] = hc_mont_redc(((u128)a.in[1][i] << 64) | a.in[0][i], a.p[0], a.p[1]); }            // T = in[1] * 2^64 + in[0]

// fp64: p[0] = the bit pattern of (double)q, p[1] = that of 1.0 / (double)q
AP_KERNEL(f64_mulmod) { AP_INDEX(); a.out[0][i] = hc_d2u(hc_f64_mulmod(hc_u2d(a.in[0][i]), hc_u2d(a.in[1][i]), hc_u2d(a.in[2][i]), hc_u2d(a.p[0]))); }
AP_KERNEL(f64_reduce) { AP_INDEX(); a.out[0][i] = hc_d2u(hc_f64_reduce(hc_u2d(a.in[0][i]), hc_u2d(a.p[0]), hc_u2d(a.p[1]))); }
AP_KERNEL(f64_from_u) { AP_INDEX(); const double d = hc_f64_from_u(a.in[0][i]); a.out[0][i] = hc_d2u(d); a.out[1][i] = hc_f64_to_u_plus(d, a.in[1][i]); }
AP_KERNEL(f64_to_u_plus) { AP_INDEX(); a.out[0][i] = hc_f64_to_u_plus(hc_u2d(a.in[0][i]), a.in[1][i]); }

// 32-bit canonical; the twiddle is narrowed from the 64-bit pair the way the tables are (hc_tw32)
AP_KERNEL(mul32) { AP_INDEX(); a.out[0][i] = hc_mul32((u32)a.in[0][i], hc_tw32(AP_TW(1, 2)), (u32)a.p[0]); }
AP_KERNEL(add32) { AP_INDEX(); a.out[0][i] = hc_add32((u32)a.in[0][i], (u32)a.in[1][i], (u32)a.p[0]); a.out[1][i] = hc_sub32((u32)a.in[0][i], (u32)a.in[1][i], (u32)a.p[0]); }
AP_KERNEL(csub32) { AP_INDEX(); a.out[0][i] = hc_csub32((u32)a.in[0][i], (u32)a.p[0]); }

// butterflies: in = x, y, w, w' (pairs: x0, y0, x1, y1, w, w'), out = x, y (x0, y0, x1, y1)
template <int FM> __device__ __forceinline__ void ap_fwd(const ApArgs &a, u64 i) {
    const HcQ Q = hc_q(a.p[0]);
    u64 x = a.in[0][i], y = a.in[1][i];
    HcLazy<FM>{Q}.fwd(x, y, AP_TW(2, 3));
    a.out[0][i] = x; a.out[1][i] = y;
}
template <int FM, bool INV> __device__ __forceinline__ void ap_pair(const ApArgs &a, u64 i) {
    const HcQ Q = hc_q(a.p[0]);
    u64 x0 = a.in[0][i], y0 = a.in[1][i], x1 = a.in[2][i], y1 = a.in[3][i];
    if (INV) HcLazy<FM>{Q}.inv(0, x0, y0, x1, y1, AP_TW(4, 5));
    else HcLazy<FM>{Q}.fwd(x0, y0, x1, y1, AP_TW(4, 5));
    a.out[0][i] = x0; a.out[1][i] = y0; a.out[2][i] = x1; a.out[3][i] = y1;
}
AP_KERNEL(lazy_fwd_free) { AP_INDEX(); ap_fwd<HC_FM_FREE>(a, i); }
AP_KERNEL(lazy_fwd_alt) { AP_INDEX(); ap_fwd<HC_FM_ALT>(a, i); }
AP_KERNEL(lazy_fwd2_free) { AP_INDEX(); ap_pair<HC_FM_FREE, false>(a, i); }
AP_KERNEL(lazy_fwd2_alt) { AP_INDEX(); ap_pair<HC_FM_ALT, false>(a, i); }
AP_KERNEL(lazy_inv2) { AP_INDEX(); ap_pair<HC_FM_ALT, true>(a, i); }
AP_KERNEL(canon32_fwd) {
    AP_INDEX();
    u32 x = (u32)a.in[0][i], y = (u32)a.in[1][i];
    HcCanon32{(u32)a.p[0]}.fwd(x, y, hc_tw32(AP_TW(2, 3)));
    a.out[0][i] = x; a.out[1][i] = y;
}

// rounds, one thread per tile. in[0]: 16 values per tile; in[1]: the twiddle pairs of the tile, 16 slots of (w, w') per round (slot 15 unused);
// inverse rounds: in[2] = (ninv, ninv', w_last, w_last') per tile
// four forward rounds = the 16 stages of a whole transform. out[0]: the lazy outputs, out[1]: hc_fwd_canon of them (p[1] = mu)
template <int FM> __device__ __forceinline__ void ap_ct4(const ApArgs &a, u64 i) {
    const HcQ Q = hc_q(a.p[0]);
    u64 e[16];
    for (int k = 0; k < 16; k++) e[k] = a.in[0][i * 16 + k];
    for (int r = 0; r < 4; r++) hc_ct_round(HcLazy<FM>{Q}, ApTw{a.in[1] + (i * 4 + r) * 32}, e);
    for (int k = 0; k < 16; k++) { a.out[0][i * 16 + k] = e[k]; a.out[1][i * 16 + k] = hc_fwd_canon<FM>(e[k], Q, a.p[1]); }
}
AP_KERNEL(ct_round4_free) { AP_INDEX(); ap_ct4<HC_FM_FREE>(a, i); }
AP_KERNEL(ct_round4_alt) { AP_INDEX(); ap_ct4<HC_FM_ALT>(a, i); }
template <bool LAST> __device__ __forceinline__ void ap_gs64(const ApArgs &a, u64 i) {
    const HcQ Q = hc_q(a.p[0]);
    u64 e[16];
    for (int k = 0; k < 16; k++) e[k] = a.in[0][i * 16 + k];
    const u64 *x = a.in[2] + i * 4;
    hc_gs_round<LAST>(HcLazy<HC_FM_ALT>{Q}, ApTw{a.in[1] + i * 32}, e, HcTw{x[0], x[1]}, HcTw{x[2], x[3]});
    for (int k = 0; k < 16; k++) a.out[0][i * 16 + k] = e[k];
}
AP_KERNEL(gs_round) { AP_INDEX(); ap_gs64<false>(a, i); }
AP_KERNEL(gs_round_last) { AP_INDEX(); ap_gs64<true>(a, i); }
template <bool LAST> __device__ __forceinline__ void ap_gs32(const ApArgs &a, u64 i) {
    u32 e[16];
    for (int k = 0; k < 16; k++) e[k] = (u32)a.in[0][i * 16 + k];
    const u64 *x = a.in[2] + i * 4;
    hc_gs_round<LAST>(HcCanon32{(u32)a.p[0]}, ApTw32{a.in[1] + i * 32}, e, hc_tw32(HcTw{x[0], x[1]}), hc_tw32(HcTw{x[2], x[3]}));
    for (int k = 0; k < 16; k++) a.out[0][i * 16 + k] = e[k];
}
AP_KERNEL(gs_round32) { AP_INDEX(); ap_gs32<false>(a, i); }
AP_KERNEL(gs_round32_last) { AP_INDEX(); ap_gs32<true>(a, i); }
// fp64: values and twiddles {w, w / q} are bit patterns of doubles; p[0], p[1] = q and 1 / q as doubles
template <bool LAST> __device__ __forceinline__ void ap_gsf(const ApArgs &a, u64 i) {
    double e[16];
    for (int k = 0; k < 16; k++) e[k] = hc_u2d(a.in[0][i * 16 + k]);
    const u64 *x = a.in[2] + i * 4;
    hc_gs_round_f64<LAST>(e, ApTw{a.in[1] + i * 32}, HcF64Mod{hc_u2d(a.p[0]), hc_u2d(a.p[1])}, HcTw{x[0], x[1]}, HcTw{x[2], x[3]});
    for (int k = 0; k < 16; k++) a.out[0][i * 16 + k] = hc_d2u(e[k]);
}
AP_KERNEL(gs_round_f64) { AP_INDEX(); ap_gsf<false>(a, i); }
AP_KERNEL(gs_round_f64_last) { AP_INDEX(); ap_gsf<true>(a, i); }

// ---- the one entry point
typedef void (*ApKernel)(ApArgs);
#define AP_ENTRY(name) {#name, ap_k_##name}
static const struct { const char *name; ApKernel k; } ap_table[] = {
    AP_ENTRY(mulhi_lo2), AP_ENTRY(mulhi), AP_ENTRY(shoup_companion), AP_ENTRY(shoup4), AP_ENTRY(mul_shoup_lazy), AP_ENTRY(mul_shoup), AP_ENTRY(fold), AP_ENTRY(canon4),
    AP_ENTRY(canon8), AP_ENTRY(reduce64), AP_ENTRY(addmod), AP_ENTRY(mont), AP_ENTRY(mont_lazy), AP_ENTRY(mont_redc), AP_ENTRY(f64_mulmod), AP_ENTRY(f64_reduce),
    AP_ENTRY(f64_from_u), AP_ENTRY(f64_to_u_plus), AP_ENTRY(mul32), AP_ENTRY(add32), AP_ENTRY(csub32), AP_ENTRY(lazy_fwd_free), AP_ENTRY(lazy_fwd_alt),
    AP_ENTRY(lazy_fwd2_free), AP_ENTRY(lazy_fwd2_alt), AP_ENTRY(lazy_inv2), AP_ENTRY(canon32_fwd), AP_ENTRY(ct_round4_free), AP_ENTRY(ct_round4_alt), AP_ENTRY(gs_round),
    AP_ENTRY(gs_round_last), AP_ENTRY(gs_round32), AP_ENTRY(gs_round32_last), AP_ENTRY(gs_round_f64), AP_ENTRY(gs_round_f64_last),
};

// Runs operation `op` on n items. params: 8 words. in[k] / out[k]: HOST arrays of n * in_w[k] / n * out_w[k] words. Returns 0, a HIP error code, or -1 (unknown operation, bad counts).
extern "C" int arith_probe_run(const char *op, const uint64_t *params, uint64_t n, int nin, const uint64_t *const *in, const uint64_t *in_w, int nout, uint64_t *const *out,
                               const uint64_t *out_w) {
    ApKernel k = nullptr;
    for (const auto &e : ap_table) if (strcmp(e.name, op) == 0) k = e.k;
    if (k == nullptr || nin < 0 || nin > AP_MAXARR || nout < 1 || nout > AP_MAXARR || n == 0 || n > (1u << 24)) return -1;
    ApArgs a; memset(&a, 0, sizeof a);
    memcpy(a.p, params, sizeof a.p);
    a.n = n;
    void *din[AP_MAXARR] = {}, *dout[AP_MAXARR] = {};
    hipError_t err = hipSuccess;
    for (int j = 0; j < nin && err == hipSuccess; j++) {
        err = hipMalloc(&din[j], n * in_w[j] * sizeof(u64));
        if (err == hipSuccess) err = hipMemcpy(din[j], in[j], n * in_w[j] * sizeof(u64), hipMemcpyHostToDevice);
        a.in[j] = (const u64 *)din[j];
    }
    for (int j = 0; j < nout && err == hipSuccess; j++) {
        err = hipMalloc(&dout[j], n * out_w[j] * sizeof(u64));
        a.out[j] = (u64 *)dout[j];
    }
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)0, a);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    for (int j = 0; j < nout && err == hipSuccess; j++) err = hipMemcpy(out[j], dout[j], n * out_w[j] * sizeof(u64), hipMemcpyDeviceToHost);
    for (int j = 0; j < AP_MAXARR; j++) { if (din[j]) (void)hipFree(din[j]); if (dout[j]) (void)hipFree(dout[j]); }
    return (int)err;
}
extern "C" int arith_probe_ops(char *buf, int len) {          // the operation names, comma separated: the table of tests/arith_cases.py must cover exactly these
    int o = 0;
    for (const auto &e : ap_table) { const int l = (int)strlen(e.name); if (o + l + 2 > len) return -1; memcpy(buf + o, e.name, (size_t)l); o += l; buf[o++] = ','; }
    buf[o ? o - 1 : 0] = 0;
    return 0;
}
