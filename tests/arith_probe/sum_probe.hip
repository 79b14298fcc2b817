// sum_probe.hip — TEST INFRASTRUCTURE beside arith_probe.hip: the key switch's inner products (hc_k_ks_mac_all, hc_k_ks_mac_multi of hc_kernels.h, included unchanged) launched
// DIRECTLY, so that tests/lazy_sum_cases.py can plant the operands no caller of libhconv.so chooses - the foreign digits, which are outputs of the basis extension, and key words
// that are extreme AFTER hc_k_pack32_rows - and hold the lazy sums to their stated bounds (PER = 6 products in 128 bits, PER = 4 in 64 bits) at every digit count where a group
// closes. Never linked into libhconv.so. Two builds of this one source (tests/arith_probe/Makefile): hipcc for gfx950 with the product's flags, and g++ -DHC_EMU against
// tests/kernel_emu.
//
// One C entry per kernel family. Each takes HOST arrays (staged into device buffers here, as arith_probe_run does), the HcMod table as the kernels read it (7 words per modulus),
// the shape and the flags, checks every extent the kernel will index against the word counts it was given, and launches the product's kernel with the grid its header comment
// states: (64, nt, image groups) / (64, nt). Returns 0, a HIP error code, or -1 (a template instance the host's dispatch cannot pick, or a buffer too small for the shape).
#ifdef HC_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "hc_kernels.h"

static_assert(sizeof(HcMod) == 7 * sizeof(u64), "tests/lazy_sum_cases.py builds the HcMod table as 7 words per modulus");
static_assert(sizeof(HcTw) == 2 * sizeof(u64), "HcMacPrep::pinv comes as (w, w') pairs");

#define SP_N ((size_t)65536)
struct SpBuf {                    // a device copy of a host array (null stays null)
    void *d = nullptr; size_t bytes = 0;
    hipError_t up(const void *h, size_t b) {
        if (h == nullptr) return hipSuccess;
        bytes = b;
        hipError_t e = hipMalloc(&d, b);
        return e == hipSuccess ? hipMemcpy(d, h, b, hipMemcpyHostToDevice) : e;
    }
    hipError_t down(void *h) const { return hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost); }
    ~SpBuf() { if (d) (void)hipFree(d); }
};
static hipError_t sp_finish() { hipError_t e = hipGetLastError(); return e == hipSuccess ? hipDeviceSynchronize() : e; }
static bool sp_shape_ok(int nmods, int nl, int nq, int nt, int alpha, int beta, int n) {
    return nl >= 1 && nt >= nl && alpha >= 1 && beta >= 1 && beta <= 64 && n >= 1 && n <= 64 && nq >= nl && nq + (nt - nl) <= nmods && nt <= 64;
}

// hc_k_ks_mac_all<NB>: evk [beta][2][nt][N]; cx: n images cx_is words apart, nl rows each; digits: n images dg_is apart, [beta][nt][N] each; acc: n images acc_is apart, [2][nt][N]
// each (in: the fill the test chose, out: the result). pinv: nt (w, w') pairs or null (HcMacPrep off); add: n images add_is apart, components add_zs apart, nl rows, or null.
extern "C" int sum_probe_mac_all(int NB, const uint64_t *mods, int nmods, int nl, int nq, int nt, int alpha, int beta, int n, const uint64_t *evk, uint64_t evk_words, const uint64_t *cx,
                                 uint64_t cx_is, uint64_t cx_words, const uint64_t *digits, uint64_t dg_is, uint64_t dg_words, uint64_t *acc, uint64_t acc_is, uint64_t acc_words,
                                 const uint64_t *pinv, const uint64_t *add, uint64_t add_zs, uint64_t add_is, uint64_t add_words, int pk) {
    if (!sp_shape_ok(nmods, nl, nq, nt, alpha, beta, n) || !mods || !evk || !cx || !digits || !acc) return -1;
    if (evk_words < (size_t)beta * 2 * nt * SP_N || cx_words < (size_t)(n - 1) * cx_is + (size_t)nl * SP_N || dg_words < (size_t)(n - 1) * dg_is + (size_t)beta * nt * SP_N ||
        acc_words < (size_t)(n - 1) * acc_is + (size_t)2 * nt * SP_N) return -1;
    if (add != nullptr && (pinv == nullptr || add_words < (size_t)(n - 1) * add_is + add_zs + (size_t)nl * SP_N)) return -1;
    SpBuf dm, dk, dx, dd, da, dp, dadd;
    hipError_t e = dm.up(mods, (size_t)nmods * sizeof(HcMod));
    if (e == hipSuccess) e = dk.up(evk, evk_words * 8);
    if (e == hipSuccess) e = dx.up(cx, cx_words * 8);
    if (e == hipSuccess) e = dd.up(digits, dg_words * 8);
    if (e == hipSuccess) e = da.up(acc, acc_words * 8);
    if (e == hipSuccess) e = dp.up(pinv, (size_t)nt * sizeof(HcTw));
    if (e == hipSuccess) e = dadd.up(add, add_words * 8);
    if (e != hipSuccess) return (int)e;
    HcMacPrep PR; memset(&PR, 0, sizeof PR);
    PR.pinv = (const HcTw *)dp.d; PR.add = (const u64 *)dadd.d; PR.add_zs = add_zs; PR.add_is = add_is;
#define SP_MAC_ALL(NN) hipLaunchKernelGGL(hc_k_ks_mac_all<NN>, dim3(64, (unsigned)nt, (unsigned)((n + NN - 1) / NN)), dim3(HC_TPB), 0, (hipStream_t)0, (const u64 *)dk.d, (const u64 *)dx.d, (size_t)cx_is, \
                                          (const u64 *)dd.d, (size_t)dg_is, (u64 *)da.d, (size_t)acc_is, (const HcMod *)dm.d, nl, nq, nt, alpha, beta, n, PR, pk)
    switch (NB) {                 // what HC_MAC_ALL (hconv.hip) can pick
        case 1: SP_MAC_ALL(1); break;
        case 2: SP_MAC_ALL(2); break;
        case 4: SP_MAC_ALL(4); break;
        case 8: SP_MAC_ALL(8); break;
        default: return -1;
    }
#undef SP_MAC_ALL
    e = sp_finish();
    if (e == hipSuccess) e = da.down(acc);
    return (int)e;
}

// hc_k_ks_mac_multi<R, NB, FIN, LAZY>: keys: nrot switching keys key_rs words apart, [beta][2][nt][N] each; cx, digits as above; out: nrot x n results [2][nt][N], rotations out_rs
// and images out_is words apart - the plain accumulators (fin = 0) or HcRotFin's outputs (fin = 1: stored permuted by ginv[r], pc0 - n images pc0_is apart, nl rows, or null -
// added to the Q rows of component 0). One image group: n <= NB, as the host launches it.
template <int R, int NB>
static void sp_mac_multi_launch(int fin, int lazy, const HcKeyPtrs &K, int nrot, const u64 *cx, size_t cx_is, const u64 *digits, size_t dg_is, u64 *acc, size_t acc_rs, size_t acc_is, const HcMod *mods,
                                int nl, int nq, int nt, int alpha, int beta, int n, int pk, const HcRotFin &F) {
    const dim3 grid(64, (unsigned)nt), block(HC_TPB);
#define SP_MACM(FF, LL) hipLaunchKernelGGL((hc_k_ks_mac_multi<R, NB, FF, LL>), grid, block, 0, (hipStream_t)0, K, nrot, cx, cx_is, digits, dg_is, acc, acc_rs, acc_is, mods, nl, nq, nt, alpha, beta, n, pk, F)
    if (fin) { if (lazy) SP_MACM(true, true); else SP_MACM(true, false); }
    else { if (lazy) SP_MACM(false, true); else SP_MACM(false, false); }
#undef SP_MACM
}
extern "C" int sum_probe_mac_multi(int R, int NB, int fin, int lazy, const uint64_t *mods, int nmods, int nl, int nq, int nt, int alpha, int beta, int n, int nrot, const uint64_t *keys,
                                   uint64_t key_rs, uint64_t key_words, const uint64_t *cx, uint64_t cx_is, uint64_t cx_words, const uint64_t *digits, uint64_t dg_is, uint64_t dg_words,
                                   uint64_t *out, uint64_t out_rs, uint64_t out_is, uint64_t out_words, const uint32_t *ginv, const uint64_t *pc0, uint64_t pc0_is, uint64_t pc0_words, int pk) {
    if (!sp_shape_ok(nmods, nl, nq, nt, alpha, beta, n) || !mods || !keys || !cx || !digits || !out || nrot < 1 || nrot > R || n > NB) return -1;
    if (key_words < (size_t)(nrot - 1) * key_rs + (size_t)beta * 2 * nt * SP_N || cx_words < (size_t)(n - 1) * cx_is + (size_t)nl * SP_N ||
        dg_words < (size_t)(n - 1) * dg_is + (size_t)beta * nt * SP_N || out_words < (size_t)(nrot - 1) * out_rs + (size_t)(n - 1) * out_is + (size_t)2 * nt * SP_N) return -1;
    if (fin && !ginv) return -1;
    if (pc0 != nullptr && (!fin || pc0_words < (size_t)(n - 1) * pc0_is + (size_t)nl * SP_N)) return -1;
    SpBuf dm, dk, dx, dd, dout, dpc;
    hipError_t e = dm.up(mods, (size_t)nmods * sizeof(HcMod));
    if (e == hipSuccess) e = dk.up(keys, key_words * 8);
    if (e == hipSuccess) e = dx.up(cx, cx_words * 8);
    if (e == hipSuccess) e = dd.up(digits, dg_words * 8);
    if (e == hipSuccess) e = dout.up(out, out_words * 8);
    if (e == hipSuccess) e = dpc.up(pc0, pc0_words * 8);
    if (e != hipSuccess) return (int)e;
    HcKeyPtrs K; memset(&K, 0, sizeof K);
    HcRotFin F; memset(&F, 0, sizeof F);
    for (int r = 0; r < nrot; r++) {
        K.k[r] = (const u64 *)dk.d + (size_t)r * key_rs;
        if (fin) { if (!(ginv[r] & 1) || ginv[r] > 0x1FFFFu) return -1; F.out[r] = (u64 *)dout.d + (size_t)r * out_rs; F.ginv[r] = ginv[r]; }
    }
    if (fin) { F.pc0 = (const u64 *)dpc.d; F.pc0_is = pc0_is; F.out_is = out_is; }
#define SP_GO(RR, NN) sp_mac_multi_launch<RR, NN>(fin, lazy, K, nrot, (const u64 *)dx.d, (size_t)cx_is, (const u64 *)dd.d, (size_t)dg_is, (u64 *)dout.d, (size_t)out_rs, (size_t)out_is, (const HcMod *)dm.d, \
                                                  nl, nq, nt, alpha, beta, n, pk, F)
    if (R == 2 && NB == 8) SP_GO(2, 8);            // what HC_MAC_MULTI (hconv.hip) can pick
    else if (R == 4 && NB == 4) SP_GO(4, 4);
    else if (R == 8 && NB == 2) SP_GO(8, 2);
    else if (R == 8 && NB == 1) SP_GO(8, 1);
    else return -1;
#undef SP_GO
    e = sp_finish();
    if (e == hipSuccess) e = dout.down(out);
    return (int)e;
}
