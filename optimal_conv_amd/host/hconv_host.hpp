// hconv_host.hpp — C++ host side above the C ABI (include/hconv.h), mirroring the reference's operator interface
// for the `conv` path with the same names, argument meaning and error behaviour (errors are fatal, like Go's panic).
//
// The reference's host code is Go; no Go toolchain exists in this image or on the GPU box,
// so per the build contract the host side is C++. Mapping (reference -> here):
//   main.go:22-42   type context              -> struct Context
//   main.go:44-462  newContext("Conv")        -> newContext()
//   conv.go:241-261 gen_idxNlogs              -> inside newContext (idx on the device, Galois keys 2^(i+1)+1)
//   main.go:1007    prep_Input                -> prep_Input
//   conv.go:184     reshape_ker               -> reshape_ker
//   conv.go:206     encode_ker_final          -> encode_ker_final
//   conv.go:487     prep_Ker                  -> prep_Ker      (EncodeCoeffs on the host, ToNTT on the GPU)
//   conv.go:522     conv_then_pack            -> conv_then_pack (fused: hc_conv_then_pack; or op-by-op through
//   conv.go:266     pack_ctxts                -> pack_ctxts      GpuEvaluator with HCONV_OPWISE=1)
//   eval.go:224     evalConv_BN               -> evalConv_BN
//   main.go:1057    post_process              -> post_process
//   main.go:971     readTxt                   -> readTxt
//   main.go:694     printDebugCfsPlain        -> printDebugCfsPlain
//   test.go:15      testConv_in               -> testConv_in
// ckks.Evaluator methods the path calls -> class GpuEvaluator {MulNew, SetScale, SubNew, Add, RotateGal}.
// Keys/encryption/decryption are harness-only (the reference draws them from crypto-random; nothing to match):
// implemented here on the host with every NTT done on the GPU through the ABI.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "../../include/hconv.h"
#include "../../include/hconv_test_hooks.h"      // --test-mode replays only (HCONV_RESNET_REPLAY)
#include "hconv_prng.hpp"

namespace hconv {

typedef unsigned __int128 u128;
static const int LOGN = 16;
static const int N = 1 << LOGN;

// ckks.DefaultBootstrapParams[6] of the fork, level order; only Q[0], Q[1] carry the conv path
extern const std::vector<uint64_t> PARAMS6_Q;
extern const std::vector<uint64_t> PARAMS7_Q;      // ckks.DefaultBootstrapParams[7]: the baseline's chain (main.go:54)
extern const std::vector<uint64_t> PARAMS6_P;      // bootstrapping key-switch primes (logQP print only)
static const uint64_t PACK_P = 0x1fffffffffe00001ull;   // main.go:449

[[noreturn]] void panic(const std::string &msg);        // Go's panic(): message to stderr, exit status 2
// a failing library call is a panic with the call's text and the context's last error
#define HC(c, call) do { int rc_ = (call); if (rc_) panic(std::string(#call) + ": " + hc_last_error(c)); } while (0)
inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a * b) % q); }
inline uint64_t addmod(uint64_t a, uint64_t b, uint64_t q) { uint64_t r = a + b; return r >= q ? r - q : r; }
inline uint64_t submod(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a + q - b; }
inline uint64_t to_mont(uint64_t a, uint64_t q) { return (uint64_t)((((u128)a) << 64) % q); }
// the timers of the console lines: Go's time.Duration.String() shape ("57.154502ms", "3.40439908s"), and seconds as a number
inline std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
inline std::string dur_ns(double ns) {
    char b[64];
    if (ns < 1e3) snprintf(b, sizeof b, "%.0fns", ns);
    else if (ns < 1e6) snprintf(b, sizeof b, "%.6gµs", ns / 1e3);
    else if (ns < 1e9) snprintf(b, sizeof b, "%.9gms", ns / 1e6);
    else snprintf(b, sizeof b, "%.9gs", ns / 1e9);
    return b;
}
inline std::string dur(std::chrono::steady_clock::time_point t0) { return dur_ns((double)std::chrono::duration_cast<std::chrono::nanoseconds>(now() - t0).count()); }
inline double secs(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(now() - t0).count(); }
// eval.go:433: the out_scale of a convolution that a bootstrapping chain follows
inline double chain_out_scale(double pow) { return exp2(round(log2((double)PARAMS6_Q[0]) - (pow + 8))); }
// The library reads no configuration from the environment (include/hconv.h); this CLI does, and hands it over as options right after every hc_ctx_create:
// HCONV_ASYNC_ALLOC (0 / 1 / 2), HCONV_SMALL32, HCONV_ROT_FUSE, HCONV_PACK32 (A/B switches; same residues in every setting). pack32_default: the value a context takes
// when HCONV_PACK32 is unset (-1: the library's own default)
void applyEnvOptions(hc_ctx *hc, int pack32_default = -1);
// Test-only overrides (HCONV_SEED: deterministic keys; HCONV_CHAIN_REPLAY: planted keys and input) take effect only when the CLI was
// started with --test-mode as its first argument; set in the environment WITHOUT that flag they end the process (an inherited variable
// must never turn a deployment into key-less or predictable computation).
bool &testMode();
const char *testOnlyEnv(const char *name);              // getenv(name) under --test-mode; nullptr when unset; panic when set without the flag
// HCONV_RESNET_REPLAY=<seed> (test mode): the secret key, every switching key and the input's encryption randomness are the counter-based splitmix64 draws of the
// test oracle's harness generators (or_gen_sk / or_gen_galois_key_l0 / or_gen_swk / or_encrypt, restated in hconv_host.cpp): the `resnet` run then
// computes, bit for bit, the network tests/golden/gen_resnet_digests.py ran on the oracle, and prints a `replay digest layer i` line per layer (tests/test_gpu_z_cli.py)
uint64_t resnetReplaySeed();                            // 0: off
namespace replay {                                      // the oracle harness' generators (splitmix64, Box-Muller sigma 3.2 bound 6 sigma)
uint64_t sm64(uint64_t seed, uint64_t i);
void fill_seeded(uint64_t seed, uint64_t q, uint64_t *out);
void gauss(uint64_t seed, std::vector<int64_t> &e);
std::vector<int64_t> gen_sk(uint64_t seed, int h);
}

// Device-resident ciphertext / plaintext (ckks.Ciphertext{Value []*ring.Poly; Scale}, ckks.Plaintext)
struct Ciphertext {
    uint64_t *d = nullptr;   // device [2][level+1][N]
    int level = 0;
    double Scale = 0;
};
struct Plaintext {
    uint64_t *d = nullptr;   // device [level+1][N], NTT domain
    int level = 0;
    double Scale = 0;
};

struct Boot;                                   // hconv_relu.cpp: bootstrapper + leveled evaluator (cont.btp, cont.evaluator of main.go:464-507)
struct BootCiphertext { uint64_t *d = nullptr; int level = 0; double Scale = 0; };   // device [2][level+1][N]

struct Context {
    int logN = LOGN, Nn = N, ECD_LV = 1;       // main.go:46
    Boot *btp = nullptr;                      // only when newContext(..., boot = true)
    hc_ctx *hc = nullptr;                     // pack_evaluator + evaluator (both run on the same device context)
    std::vector<hc_ctx *> shards;             // HCONV_GPUS=G > 1: shards[0] = hc, shards[g] = a context on device g (mod the device count)
                                              // with the same Galois keys: ONE convolution runs i mod G over them (`conv 7 3`)
    std::vector<int64_t> sk;                  // sparse ternary secret, h = 192 (main.go:410)
    std::vector<uint64_t> sk_ntt[3];          // NTT rows mod Q0, Q1, P (host)
    double scale = (double)(1 << 30);
    int num_rotations = 0;
    Seed256 seed;                             // key of this context's generators (hconv_prng.hpp)
    ChaChaRng g;                              // this context's own generator: secret key, Galois keys, encryption randomness
    uint64_t replay_encryptions = 0;          // HCONV_RESNET_REPLAY: encryptions so far (the i-th takes the oracle harness' seed 5 + 1000 i)
    uint64_t *d_sk = nullptr;                 // device [3][N]: NTT(s) mod Q0, Q1, P, the sk_ntt operand of hc_encrypt_sk / hc_decrypt_decode_coeffs (uploaded once)
    uint32_t enc_seed8[8] = {0};              // key of the device encryptor's draws: eight draws of g at context creation
    uint64_t enc_stream = 0;                  // hc_encrypt_sk's stream id: one per call, never reused
    std::map<int, std::vector<std::vector<int>>> ext_idx;   // kind "Resnet_crop_fast": ext_idx[step][ul], the keep masks of the "inside" layers (main.go:123-136);
                                              // kind "Resnet_crop_packed": the entries packedMaskKey(step) and packedStrideMaskKey(step) instead
};

// rot_util.go:226-267 gen_keep_vec_stride: gen_keep_vec (ul = 0 upper, 1 lower half of the full-slot bootstrapping) that keeps only the outputs at
// stride `step` on the in_wid grid: kp_wid x kp_wid of them, from position init = 0 (raw_in_wid_odd) or step - 1, slot order bit-reversed over logN - 1 bits.
// Header-only so that a test can build it without a device.
inline std::vector<int> gen_keep_vec_stride(int vec_size, int in_wid, int kp_wid, int step, int ul, bool raw_in_wid_odd) {
    int logN = 0; for (; (1 << logN) < 2 * vec_size; logN++) {}
    std::vector<int> idx((size_t)vec_size, 0);
    const int batch = 2 * vec_size / (in_wid * in_wid);
    const int init = raw_in_wid_odd ? 0 : step - 1;
    auto rev = [&](int x) { uint32_t v = (uint32_t)x, r = 0; for (int k = 0; k < logN - 1; k++) r |= ((v >> k) & 1u) << (logN - 2 - k); return (size_t)r; };
    if (ul == 0) {
        for (int i = 0; i < kp_wid; i++) if (init + i * step < in_wid / 2)
            for (int j = 0; j < kp_wid; j++) for (int b = 0; b < batch; b++) idx[rev(in_wid * batch * (init + i * step) + batch * (j * step + init) + b)] = 1;
    } else if (ul == 1) {
        for (int i = 0; i < kp_wid; i++) if (init + i * step >= in_wid / 2)
            for (int j = 0; j < kp_wid; j++) for (int b = 0; b < batch; b++) idx[rev(in_wid * batch * (init + i * step - in_wid / 2) + batch * (j * step + init) + b)] = 1;
    } else panic("ul not 0 nor 1");
    return idx;
}

// rot_util.go:141-174 gen_keep_vec: the 0/1 mask of keep_ctxt on full slots, for the upper (ul = 0) or lower (ul = 1) half of the in_wid x in_wid grid: the
// kp_wid x kp_wid corner, every channel slot, slot order bit-reversed over logN - 1 bits. Header-only, like gen_keep_vec_stride.
inline std::vector<int> gen_keep_vec(int vec_size, int in_wid, int kp_wid, int ul) {
    int logN = 0; for (; (1 << logN) < 2 * vec_size; logN++) {}
    std::vector<int> idx((size_t)vec_size, 0); const int batch = 2 * vec_size / (in_wid * in_wid);
    if (kp_wid < in_wid / 2) panic("keep width too small. less than in_wid/2");
    if (ul != 0 && ul != 1) panic("ul not 0 nor 1");
    const int rows = ul == 0 ? in_wid / 2 : kp_wid - in_wid / 2;
    for (int i = 0; i < rows; i++) for (int j = 0; j < kp_wid; j++) for (int b = 0; b < batch; b++) {
        uint32_t v = (uint32_t)(in_wid * batch * i + batch * j + b), r = 0; for (int k = 0; k < logN - 1; k++) r |= ((v >> k) & 1u) << (logN - 2 - k);
        idx[r] = 1;
    }
    return idx;
}
// rot_util.go:428-492 gen_comprs_full (its padding = false branch, the one the reference runs): rotation -> 0/1 mask of ext_ctxt for the full-packing stride layer (kind
// "StrConv"). Half ul (0 upper, 1 lower) of a full-slot ciphertext on the in_wid grid goes through sum over (rot, mask) of Rotate(ct (.) mask, rot): the stride-2 positions
// (odd row and column below kp_wid) land on the in_wid/2 grid with four times the channel slots, in quarter pos (0..3) of that channel axis (DESIGN.md "Full-packing stride
// layer"). 2 * (in_wid/4) rotations, the same set for both halves. Header-only, like the masks above.
inline std::map<int, std::vector<int>> gen_comprs_full(int vec_size, int in_wid, int kp_wid, int pos, int ul) {
    if (kp_wid < in_wid / 2) panic("keep width too small. less than in_wid/2");
    if (in_wid % 4 != 0) panic("input wid not divisible by 4");
    if (pos < 0 || pos > 3) panic("pos not in 0..3");
    if (ul != 0 && ul != 1) panic("ul not 0 nor 1");
    const int batch = 2 * vec_size / (in_wid * in_wid), min_wid = in_wid / 4;
    int log_in_wid = 0; for (; (1 << log_in_wid) < in_wid; log_in_wid++) {}
    auto rev = [](int x, int bits) { int r = 0; for (int k = 0; k < bits; k++) r |= ((x >> k) & 1) << (bits - 1 - k); return r; };
    const int rpos = rev(pos, 2);
    std::map<int, std::vector<int>> r_idx;
    for (int j = 0; j < 2 * min_wid; j++) {                                                   // the kind of move depends on j
        std::vector<int> tmp((size_t)vec_size, 0);
        if (rev(in_wid / 2 + j, log_in_wid) < kp_wid)
            for (int b = 0; b < batch; b++) for (int i = 0; i < min_wid; i++)
                if (ul == 0 || rev(3 * min_wid + i, log_in_wid - 1) < kp_wid - in_wid / 2) tmp[(size_t)(2 * min_wid * in_wid * b + 2 * min_wid * j + i + in_wid * min_wid + min_wid)] = 1;
        r_idx[j * min_wid - 2 * rpos * min_wid * min_wid + min_wid + in_wid * min_wid] = tmp;
    }
    return r_idx;
}
// rot_util.go:179-218: one mask for the packed (low | high) ciphertext of sparse bootstrapping, period 2 n_s
inline std::vector<int> gen_keep_vec_sparse(int vec_size, int in_wid, int kp_wid, int log_sparse) {
    int logN = 0; for (; (1 << logN) < 2 * vec_size; logN++) {}
    std::vector<int> idx((size_t)vec_size, 0); const int batch = 2 * vec_size / (in_wid * in_wid), sparsity = 1 << log_sparse;
    if (sparsity == 1) panic("We do not support full packing in gen_keep_vec_sparse");
    if (kp_wid < in_wid / 2) panic("keep width too small. less than in_wid/2");
    auto rev = [&](int x) { uint32_t v = (uint32_t)x, r = 0; for (int k = 0; k < logN - 1; k++) r |= ((v >> k) & 1u) << (logN - 2 - k); return (int)r; };
    for (int i = 0; i < in_wid / 2; i++) for (int j = 0; j < kp_wid; j++) for (int b = 0; b < batch / sparsity; b++) idx[(size_t)rev(in_wid * batch * i + batch * j + b * sparsity)] = 1;
    for (int i = 0; i < kp_wid - in_wid / 2; i++) for (int j = 0; j < kp_wid; j++) for (int b = 0; b < batch / sparsity; b++) idx[(size_t)(rev(in_wid * batch * i + batch * j + b * sparsity) + vec_size / sparsity)] = 1;
    const int post_slot = 2 * vec_size / sparsity;
    for (int i = 0; i < post_slot; i++) for (int j = 1; j < sparsity / 2; j++) idx[(size_t)(i + post_slot * j)] = idx[(size_t)i];
    return idx;
}

// ---- the packed layout of `resnet_packed` (not a reference layout; DESIGN.md "The packed layout"). Header-only, like the masks above, so that a test can build it without a device.
// Block b = 0, 1, 2 of the full-slot network holds its C = 16, 32, 64 channels norm = 4, 2, 1 slots apart on the cells of the lattice of step s = 1, 2, 4. An IMAGE SLOT of block b
// is (g, py, px), g < norm, py, px < s: channel c at channel slot norm*c + g, activation cell (i, j) at grid cell (py + s*i, px + s*j). norm * s^2 = 4, 8, 16 images per ciphertext.
static const int PACKED_GROUP = 16;                                            // images of a group: one ciphertext of block 2, two of block 1, four of block 0
struct PackedSlot { int ct, g, py, px; };
// THE slot assignment: where image m (0..15) of a group lives in block blk. Block 0 takes images 4q..4q+3 into ciphertext q at g = m mod 4 (the input merge sum_g X^g ct_g). A stride
// layer sends (ciphertext q, channel offset g) of its input block, norm_out = norm_in / 2, to result r = 2q + (g / norm_out): channel offset g mod norm_out, output ciphertext r / 4,
// moved by s_in * (t / 2, t mod 2) cells, t = r mod 4. The three cases below are that rule applied once and twice to block 0's assignment.
inline PackedSlot packed_slot(int blk, int m) {
    if (m < 0 || m >= PACKED_GROUP) panic("packed_slot: image index outside the group");
    if (blk == 0) return {m / 4, m % 4, 0, 0};
    if (blk == 1) return {m / 8, m % 2, (m / 4) % 2, (m / 2) % 2};
    if (blk == 2) return {0, 0, (m / 4) % 2 + 2 * (m / 8), (m / 2) % 2 + 2 * (m % 2)};
    panic("packed_slot: block not in 0..2");
}
// ext_idx keys of a "Resnet_crop_packed" context (the "Resnet_crop_fast" kind's are the steps 1, 2, 4 themselves): the mask of block `step`'s layers, all step^2 phases; and the mask
// of the stride layer that enters it, the (step/2)^2 phases its images reach by themselves
inline int packedMaskKey(int step) { return 100 + step; }
inline int packedStrideMaskKey(int step) { return 200 + step; }
// keep mask (ul = 0 upper, 1 lower half; gen_keep_vec_stride's slot order) of the cells (py + step*i, px + step*j), py, px < n_phase, i, j < kp_wid, every channel slot
inline std::vector<int> gen_keep_vec_packed(int vec_size, int in_wid, int kp_wid, int step, int n_phase, int ul) {
    int logN = 0; for (; (1 << logN) < 2 * vec_size; logN++) {}
    if (ul != 0 && ul != 1) panic("ul not 0 nor 1");
    if (n_phase < 1 || n_phase > step || (kp_wid - 1) * step + n_phase > in_wid) panic("gen_keep_vec_packed: phases outside the lattice, or cells outside the grid");
    std::vector<int> idx((size_t)vec_size, 0);
    const int batch = 2 * vec_size / (in_wid * in_wid);
    auto rev = [&](int x) { uint32_t v = (uint32_t)x, r = 0; for (int k = 0; k < logN - 1; k++) r |= ((v >> k) & 1u) << (logN - 2 - k); return (size_t)r; };
    auto live = [&](int x) { return x % step < n_phase && x / step < kp_wid; };
    for (int row = ul * in_wid / 2; row < (ul + 1) * in_wid / 2; row++) if (live(row))
        for (int col = 0; col < in_wid; col++) if (live(col))
            for (int b = 0; b < batch; b++) idx[rev(in_wid * batch * (row - ul * in_wid / 2) + batch * col + b)] = 1;
    return idx;
}
// The block-diagonal kernel over all `slots` channel slots that the packed layers hand to hc_prep_ker_ex2 at norm 1 (dilation stays the library's): ker is HWIO (ker_size, cin,
// cout); for the channel offsets g = g_lo .. g_lo + g_cnt - 1, input slot norm_in*c + g feeds output slot norm_out*o + (g mod norm_out) and nothing else. A layer inside a block:
// norm_in = norm_out = norm, g_lo = 0, g_cnt = norm. Half h of a stride layer: norm_in = 2 norm_out, g_lo = h * norm_out, g_cnt = norm_out.
inline std::vector<double> packed_expand_ker(const std::vector<double> &ker, int ker_size, int cin, int cout, int norm_in, int norm_out, int g_lo, int g_cnt, int slots = 64) {
    if ((int)ker.size() != ker_size * cin * cout) panic("packed_expand_ker: input size inconsistent");
    if (g_lo < 0 || g_cnt < 1 || g_lo + g_cnt > norm_in || norm_in * cin > slots || norm_out * cout > slots) panic("packed_expand_ker: channel slots exceeded");
    std::vector<double> out((size_t)ker_size * slots * slots, 0.0);
    for (int t = 0; t < ker_size; t++) for (int c = 0; c < cin; c++) for (int o = 0; o < cout; o++) for (int g = g_lo; g < g_lo + g_cnt; g++)
        out[((size_t)t * slots + (size_t)(norm_in * c + g)) * slots + (size_t)(norm_out * o + g % norm_out)] = ker[((size_t)t * cin + c) * cout + o];
    return out;
}
// bn_a / bn_b of the same layers: channel o's value on the slots norm_out*o + g, g < norm_out
inline std::vector<double> packed_expand_bn(const std::vector<double> &v, int norm_out) {
    std::vector<double> out(v.size() * (size_t)norm_out);
    for (size_t o = 0; o < v.size(); o++) for (int g = 0; g < norm_out; g++) out[o * (size_t)norm_out + (size_t)g] = v[o];
    return out;
}

// ---- harness / reference-shaped API ----
Context *newContext(int logN, int ker_wid, const std::vector<int> &in_wids, const std::vector<int> &kp_wids, bool boot, const std::string &kind);
void freeContext(Context *);
std::vector<double> readTxt(const std::string &name_file, int size);
std::vector<double> prep_Input(const std::vector<double> &input, int raw_in_wid, int in_wid, int Nn, int norm, bool trans, bool printResult);
std::vector<std::vector<double>> reshape_ker(const std::vector<double> &ker_in, int k_sz, int out_batch, bool trans);
std::vector<double> encode_ker_final(const std::vector<std::vector<double>> &ker_in, int pos, int i, int in_wid, int in_batch, int ker_wid);
std::vector<double> post_process(const std::vector<double> &in_cfs, int raw_in_wid, int in_wid);
void printDebugCfsPlain(const std::vector<double> &valuesTest, const std::vector<double> &valuesWant);
void set_Variables(int batch, int raw_in_wid, int in_wid, int ker_wid, const std::string &kind, int *kp_wid, int *out_batch, int *logN, bool *trans);

// encoder / encryptor / decryptor (ckks.Encoder.EncodeCoeffs, Encryptor.EncryptNew, Decryptor.Decrypt + DecodeCoeffs)
std::vector<uint64_t> EncodeCoeffs(const std::vector<double> &coeffs, int level, double scale);   // host rows, coefficient domain
Ciphertext EncryptNew(Context *cont, const std::vector<uint64_t> &pt_rows, int level, double scale);
std::vector<double> DecryptDecodeCoeffs(Context *cont, const Ciphertext &ct);
// HCONV_DEVICE_ENCRYPT: 1 = hc_encode_coeffs + hc_encrypt_sk / hc_decrypt_decode_coeffs, 0 or unset = the host encryptor and decryptor (every
// existing run keeps the stream it has; the default waits for the measurement profiles/LEDGER.md asks for). Under HCONV_RESNET_REPLAY / HCONV_CHAIN_REPLAY* the draws are always the host's.
bool deviceEncrypt();
// HCONV_DEVICE_ENCODE: 1 = the bootstrappers' DFT diagonals and slot masks are encoded by hc_encode_slots_ex from uploaded VALUE vectors (all diagonals of a matrix in a few
// calls), 0 = by hconv_encoder.hpp on the host, a diagonal at a time. The same words either way: no replay, digest or seeded stream depends on the switch.
bool deviceEncode();
// EncodeCoeffs + EncryptNew of n inputs: ONE hc_encode_coeffs and ONE hc_encrypt_sk call on the device path, n EncryptNew calls otherwise
std::vector<Ciphertext> EncryptCoeffsBatch(Context *cont, const std::vector<const std::vector<double> *> &inputs, int level, double scale);
// Decrypt + DecodeCoeffs of n level-0 ciphertexts: ONE hc_decrypt_decode_coeffs call on the device path
std::vector<std::vector<double>> DecryptDecodeCoeffsBatch(Context *cont, const std::vector<Ciphertext> &cts);
void freeCt(Context *cont, Ciphertext &ct);

// kernel plaintexts: handle to the B device-resident plaintexts
struct KerPlain { hc_ker *h = nullptr; int max_bat = 0; double Scale = 0; std::vector<hc_ker *> shard_h; };   // shard_h[g]: the same plaintexts on device g
KerPlain prep_Ker(Context *cont, const std::vector<double> &ker_in, const std::vector<double> &BN_a, int in_wid, int ker_wid,
                  int real_ib, int real_ob, int norm, int ECD_LV, int pos, bool trans, int dilation = 1, int ib_stride = 1, int ob_stride = 1);   // dilation / ib_stride: hc_prep_ker_ex2; ob_stride: output channel o's plaintext on row norm*ob_stride*o (moved on the host)

Ciphertext conv_then_pack(Context *cont, const Ciphertext &ctxt_in, const KerPlain &pl_ker, int max_ob, int norm, int ECD_LV,
                          double out_scale, const Plaintext *pl_bn_b);
Ciphertext evalConv_BN(Context *cont, const Ciphertext &ct_input, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                       const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale, bool trans,
                       int dilation = 1, int ib_stride = 1, int ob_stride = 1);
void testConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, bool boot);
// The marshalling of ONE hc_conv_then_pack_batch call. groups: the images of a launch set, each with one input ciphertext per entry of kers (ciphertext j of every group goes
// with kers[j]); all inputs share level and scale (checked). bias (or nullptr): added once per group. Returns one fresh level-0 ciphertext per group at the scale the library
// reports. The call is queued, not waited for, and nothing is printed: the callers sync and print their own timing lines.
std::vector<Ciphertext> conv_then_pack_batch(Context *cont, const std::vector<std::vector<Ciphertext>> &groups, const std::vector<const hc_ker *> &kers, double ker_scale, const Plaintext *bias,
                                             int max_batch, int out_norm, double out_scale);
// `transconv` (not a reference command): kind "TransConv" through prep_Input / prep_Ker with trans = true and the same conv_then_pack, Ours only.
// boot (`transconvReLU`): the layer evalTransConv_BNRelu_batch; sparse: its log_sparse = 2 form
void testTransConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, bool boot = false, bool sparse = false);
// evalConv_BN for a layer with more input channels than one ciphertext holds (not a reference routine): ker_in is HWIO with real_ib = m * ib input channels, ciphertext j
// holds the channels j*ib .. (j+1)*ib - 1 and its plaintexts are prep_Ker of that channel slice with the same bn_a. ONE convolution: the m products are summed at level 1
// (hc_conv_then_pack_batch's members with one ct_out), then one SetScale, one pack tree, one bias add. _batch: the images of a batch, each with its m ciphertexts (<= 16 in all)
Ciphertext evalConv_BN_multi(Context *cont, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                             const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale);
std::vector<Ciphertext> evalConv_BN_multi_batch(Context *cont, const std::vector<std::vector<Ciphertext>> &groups, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale);
// `multiconv` (not a reference command): `conv`'s layer with n_in * in_batch input channels in n_in input ciphertexts, Ours only
// boot (`multiconvReLU`): the layer evalConv_BNRelu_multi_batch
void testMultiConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, int n_in, bool boot = false);
// The hand-over of a layer: hc_sync of the convolution context (the bootstrapper's context runs on another stream), then evalConv_BNRelu_tail_batch on the convolution results'
// device blocks (keep_idx, mask_key, pack_pos: that function's). ct_conv stays the caller's; the results stay with the bootstrapper (bootDecryptDecodeCoeffs / freeBootCt).
std::vector<BootCiphertext> conv_tail(Context *cont, const std::vector<Ciphertext> &ct_conv, const std::string &kind, int log_sparse, double alpha, double pow, int in_wid, int kp_wid,
                                      const std::vector<std::vector<int>> *keep_idx = nullptr, const std::string &mask_key = "", int pack_pos = 0);
// Layers of the new convolution forms (not reference routines): the convolution at chain_out_scale(pow), then conv_tail.
// ct_conv_out != nullptr: the convolution results are handed to the caller (who frees them) instead of being freed here.
// Transposed (a context of kind "TransConv" / "TransConv_sparse" with boot): kp_wid = 2 * raw_in_wid. sparse = false: kind "TransConv", the "Conv" tail on full slots, the
// real_ob = real_ib / 4 output channels at slots o. sparse = true: kind "TransConv_sparse" at log_sparse = 2: the kernel plaintexts with ob_stride = 4 and the pack tree's
// norm = 4 put output channel o at slot 4*o - the layout of the sparse ResNet's first block - and ONE packed ciphertext goes through the sparse bootstrapper.
std::vector<BootCiphertext> evalTransConv_BNRelu_batch(Context *cont, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                       const std::vector<double> &bn_b, double alpha, double pow, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob,
                                                       bool sparse, std::vector<Ciphertext> *ct_conv_out = nullptr);
// Multi-input (a context of kind "Conv" with boot): evalConv_BN_multi_batch, then the "Conv" tail over the groups' results (groups.size() within the bootstrapper's image batch)
std::vector<BootCiphertext> evalConv_BNRelu_multi_batch(Context *cont, const std::vector<std::vector<Ciphertext>> &groups, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                        const std::vector<double> &bn_b, double alpha, double pow, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob);
// ---- convReLU chain (hconv_relu.cpp; eval.go:272-607 for kind "Conv") ----
Boot *newBoot(const std::vector<int64_t> &sk, const Seed256 &seed, int device, const std::vector<int> &log_sparse_sets, int image_batch = 1);   // one "bootstrapper" per log_sparse; image_batch: images per launch set of the tail (HCONV_IMAGE_BATCH)
void freeBoot(Boot *);
void bootPrepareCompress(Boot *B, int in_wid, int kp_wid, int log_sparse);   // rotation keys of a stride layer's ext_double_ctxt
void bootPrepareCompressFull(Boot *B, int in_wid, int kp_wid, int pos);      // rotation keys of the full-packing stride layer's ext_ctxt (gen_comprs_full, both halves), main.go:378-402
// everything after evalConv_BN: Scale *= 2^pow, BootstrappConv_CtoS, evalReLU + MulByPow2, keep_ctxt, BootstrappConv_StoC
BootCiphertext evalConv_BNRelu_tail(Boot *B, const std::string &kind, int log_sparse, const uint64_t *ct_conv_dev, double ct_scale, double alpha, double pow, int in_wid, int kp_wid);
// the same tail for the images of a batch (same layer, same weights) as ONE set of launches; at most the image_batch the bootstrapper was built with
// kinds "TransConv" (the "Conv" tail; kp_wid = 2 * raw_in_wid) and "TransConv_sparse" (the "Conv_sparse" tail, log_sparse = 2 only): a stride-2 transposed layer's output.
// kinds "Conv_inside" / "StrConv_inside" (the "Conv" tail on full slots) keep with keep_idx[ul] (Context::ext_idx[step]) instead of gen_keep_vec; mask_key names them in the mask cache
// kind "StrConv" (eval.go:303, 507-520: the full-packing stride layer): instead of a keep mask each half goes through ext_ctxt with gen_comprs_full(N/2, in_wid, kp_wid, pack_pos, ul),
// as ONE hoisted linear transform; the result lives on the in_wid/2 grid, quarter pack_pos of its channel slots (DESIGN.md "Full-packing stride layer")
std::vector<BootCiphertext> evalConv_BNRelu_tail_batch(Boot *B, const std::string &kind, int log_sparse, const std::vector<const uint64_t *> &ct_conv_dev, double ct_scale, double alpha, double pow, int in_wid, int kp_wid,
                                                       const std::vector<std::vector<int>> *keep_idx = nullptr, const std::string &mask_key = "", int pack_pos = 0);
std::vector<double> bootDecryptDecodeCoeffs(Boot *B, const BootCiphertext &ct);
void freeBootCt(Boot *B, BootCiphertext &ct);
void bootStats(Boot *B, long *keys, long *keyswitches);
std::vector<int> bootSets(Boot *B);              // log_sparse of every bootstrapper built so far (0: the full-slot one)
void bootEncodeStats(Boot *B, long *diagonals, long *masks, bool *device);   // plaintexts encoded since the bootstrapper was built, and where (deviceEncode)
// ---- the baseline's bootstrapping + ReLU (test_BL.go:113-168) on parameter set [7]: cont.btp.Bootstrapp (the stock full-slot
// bootstrapper), imaginary packing / unpacking, evalReLU + MulByPow2 + SetScale on both halves
Boot *newBootBL(const std::vector<int64_t> &sk, const Seed256 &seed, int device);
// ct_res0/1: level-1 results of the two baseline convolutions, device [2][2][N] over (Q0, Q1 of set [7]) at `scale`; out0/1 likewise at level 1
void blBootReLU(Boot *B, const uint64_t *ct_res0, const uint64_t *ct_res1, double scale, double alpha, double pow, uint64_t *out0, uint64_t *out1, double *out_scale);
// eval.go:272-607 for kinds "Conv", "Conv_sparse", "StrConv_sparse" (hconv_resnet.cpp); returns a level-1, scale-2^30 ciphertext
// evalConv_BN / evalConv_BNRelu_new for the images of a batch: kernel plaintexts prepared once, hc_conv_then_pack_batch, the tail as one launch set
std::vector<Ciphertext> evalConv_BN_batch(Context *cont, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                          const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale, bool trans,
                                          int dilation = 1, int ib_stride = 1, int ob_stride = 1);
// step (kinds "Conv_inside" / "StrConv_inside" of a "Resnet_crop_fast" context): the stride of the layer's OUTPUT on the in_wid grid; the kernel is dilated by step
// (StrConv_inside: step / 2). ib_stride: input channel c of ker_in is channel ib_stride*c of the kernel (test.go:484-492), real_ib counts ker_in's channels.
std::vector<Ciphertext> evalConv_BNRelu_new_batch(Context *cont, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                  const std::vector<double> &bn_b, double alpha, double pow, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob,
                                                  int norm, int log_sparse, const std::string &kind, int step = 1, int ib_stride = 1, int pack_pos = 0);   // pack_pos: kind "StrConv" (kp_wid = the kept width on the INPUT grid)
int imageBatch();                                // HCONV_IMAGE_BATCH (1..8; default 1): images that go through a layer as one launch set
Ciphertext evalConv_BNRelu_new(Context *cont, const Ciphertext &ct_input, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                               const std::vector<double> &bn_b, double alpha, double pow, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob,
                               int norm, int log_sparse, const std::string &kind);
// test.go:76-370 — `resnet ker depth 1 n false`
void testResNet_crop_sparse(int st, int end, int ker_wid, int depth, bool debug);
// test.go:372-636 — `resnet_fast ker depth 1 n false` (not a reference command; the reference's main.go:622 alternative to the line above): full slots on the 32-wide grid,
// stride layers keep their outputs in place (gen_keep_vec_stride), later layers use dilated kernels; one full-slot bootstrapper
void testResNet_crop_fast_in(int st, int end, int ker_wid, int depth, bool debug);
// `resnet_packed ker depth 1 n false` (not a reference command): resnet_fast's network, files and results with up to 16 images per ciphertext (packed_slot above); ker 3 and 7
void testResNet_crop_packed(int st, int end, int ker_wid, int depth);
// sum_g X^g cts[g] into cts[0] (HC_LV_MONOMIAL, one pass per further ciphertext), the others freed: resnet_fast's inputs, channel b at slot 4b, become one block-0 ciphertext of
// cts.size() <= 4 images, image g at the channel slots 4b + g. Same level and scale throughout.
Ciphertext mergePackedInputs(Context *cont, std::vector<Ciphertext> &cts);
// `strconvReLU ker i_batch n [pos]` (not a reference command): the full-packing stride layer alone - kind "StrConv" at pack_pos = pos on testConv_in's shapes, Ours only
void testStrConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, int pos);
// test.go:1209-1400 — `imagenet ker n [c1]`: the ImageNet tail (3 layers of c1 channels on the 16-grid, the stride layer to 2 c1 on the 8-grid, 3 layers, reduce-mean + FC to 1000 classes)
void testImagenet_final_fast_in(int st, int end, int ker_wid, int c1 = 256);
// test_BL.go:16 — the slot-packed baseline the reference runs first (hconv_bl.cpp); boot = true adds Bootstrapp + ReLU (test_BL.go:113-168)
void testConv_BL_in(int real_batch, int in_wid, int ker_wid, int total_test_num, bool boot);

// ckks.Evaluator subset used by conv.go, one C-ABI call per limb row
class GpuEvaluator {
public:
    explicit GpuEvaluator(Context *c) : cont(c) {}
    Ciphertext MulNew(const Ciphertext &ct, const Plaintext &pt);            // conv.go:527, 288
    void SetScale(Ciphertext &ct, double scale);                             // conv.go:528
    Ciphertext SubNew(const Ciphertext &a, const Ciphertext &b);             // conv.go:289
    void Add(const Ciphertext &a, const Ciphertext &b, Ciphertext &out);     // conv.go:290, 292
    void AddPlain(const Ciphertext &a, const Plaintext &b, Ciphertext &out); // eval.go:258
    void RotateGal(const Ciphertext &ct, uint64_t galEl, Ciphertext &out);   // conv.go:291
private:
    Context *cont;
    Ciphertext alloc(int level, double scale);
};

}  // namespace hconv
