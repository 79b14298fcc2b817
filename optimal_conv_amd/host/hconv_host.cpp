// hconv_host.cpp — see hconv_host.hpp for the reference mapping. Everything that touches residues of a ciphertext
// on the conv path runs on the GPU through the C ABI; the host does float index shuffling, sampling and printing.
#include "hconv_host.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <functional>
#include <random>
#include <sstream>

namespace hconv {

const std::vector<uint64_t> PARAMS6_Q = {
    0x80000000080001ull, 0x1ffffffea0001ull,                                                          // residual (levels 0-1)
    0x1000000000b00001ull, 0x1000000000ce0001ull,                                                     // StC
    0x3ffffe80001ull,                                                                                 // 42-bit
    0x3ffc0001ull, 0x40080001ull, 0x3fac0001ull, 0x40720001ull, 0x3f820001ull, 0x3f760001ull, 0x40980001ull,
    0x3f5a0001ull, 0x3f540001ull, 0x40b00001ull, 0x40c20001ull,                                       // 11 x ~30-bit
    0x80000000440001ull, 0x7fffffffba0001ull, 0x80000000500001ull, 0x7fffffffaa0001ull, 0x800000005e0001ull,
    0x7fffffff7e0001ull, 0x7fffffff380001ull, 0x80000000ca0001ull,                                    // sine
    0x200000000e0001ull, 0x20000000140001ull, 0x20000000280001ull, 0x1fffffffd80001ull};              // CtS
// ckks.DefaultBootstrapParams[7] (the baseline's set, main.go:54): residual group = levels 0-13, StC 14-15, sine, CtS
const std::vector<uint64_t> PARAMS7_Q = {
    0x80000000080001ull, 0x10000000006e0001ull,
    0x3ffc0001ull, 0x40080001ull, 0x3fac0001ull, 0x40720001ull, 0x3f820001ull, 0x3f760001ull, 0x40980001ull,
    0x3f5a0001ull, 0x3f540001ull, 0x40b00001ull, 0x40c20001ull,                                       // 11 x ~30-bit (levels 2-12)
    0xffffffffffc0001ull,                                                                             // level 13
    0x1000000000b00001ull, 0x1000000000ce0001ull,                                                     // StC
    0x80000000440001ull, 0x7fffffffba0001ull, 0x80000000500001ull, 0x7fffffffaa0001ull, 0x800000005e0001ull,
    0x7fffffff7e0001ull, 0x7fffffff380001ull, 0x80000000ca0001ull,                                    // sine
    0x200000000e0001ull, 0x20000000140001ull, 0x20000000280001ull, 0x1fffffffd80001ull};              // CtS
const std::vector<uint64_t> PARAMS6_P = {0x1fffffffffe00001ull, 0x1fffffffffc80001ull, 0x1fffffffffb40001ull,
                                         0x1fffffffff500001ull, 0x1fffffffff420001ull};

void panic(const std::string &msg) {
    fprintf(stderr, "panic: %s\n", msg.c_str());
    exit(2);
}
bool &testMode() { static bool on = false; return on; }
const char *testOnlyEnv(const char *name) {
    const char *v = getenv(name);
    if (!v || !*v) return nullptr;
    if (!testMode()) panic(std::string(name) + " is set but the CLI was not started with --test-mode: refusing to run with test-only key / input overrides");
    return v;
}
static const uint64_t MODQ[3] = {0x80000000080001ull, 0x1ffffffea0001ull, PACK_P};   // Q0, Q1, P (ABI indices 0,1,2)

// ---------------------------------------------------------------- device helpers
static uint64_t *dev_rows(Context *c, size_t rows) { void *p = nullptr; HC(c->hc, hc_malloc(c->hc, rows * N * sizeof(uint64_t), &p)); return (uint64_t *)p; }
static uint64_t *dev_upload(Context *c, const std::vector<uint64_t> &h) { uint64_t *d = dev_rows(c, h.size() / N); HC(c->hc, hc_upload(c->hc, d, h.data(), h.size() * 8)); return d; }
static std::vector<uint64_t> dev_download(Context *c, const uint64_t *d, size_t rows) { std::vector<uint64_t> h(rows * N); HC(c->hc, hc_download(c->hc, h.data(), d, h.size() * 8)); return h; }
// NTT of host rows (all rows mod the same modulus) on the GPU
static std::vector<uint64_t> gpu_ntt(Context *c, int mod, const std::vector<uint64_t> &rows, bool inverse = false) {
    uint64_t *d = dev_upload(c, rows); int cnt = (int)(rows.size() / N);
    HC(c->hc, inverse ? hc_intt(c->hc, mod, d, d, cnt) : hc_ntt(c->hc, mod, d, d, cnt));
    std::vector<uint64_t> out = dev_download(c, d, (size_t)cnt);
    HC(c->hc, hc_free(c->hc, d));
    return out;
}

// ---------------------------------------------------------------- test mode: the oracle harness' deterministic generators (HCONV_RESNET_REPLAY)
uint64_t resnetReplaySeed() { static const uint64_t v = testOnlyEnv("HCONV_RESNET_REPLAY") ? strtoull(testOnlyEnv("HCONV_RESNET_REPLAY"), nullptr, 0) : 0; return v; }
namespace replay {
uint64_t sm64(uint64_t seed, uint64_t i) { uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
void fill_seeded(uint64_t seed, uint64_t q, uint64_t *out) { for (int j = 0; j < N; j++) out[j] = sm64(seed, (uint64_t)j) % q; }
void gauss(uint64_t seed, std::vector<int64_t> &e) {
    e.resize(N);
    for (int j = 0; j < N; j++) for (uint64_t k = 0;; k++) {
        const double u1 = ((double)(sm64(seed, (uint64_t)j * 64 + 2 * k) >> 11) + 1.0) / 9007199254740993.0, u2 = (double)(sm64(seed, (uint64_t)j * 64 + 2 * k + 1) >> 11) / 9007199254740992.0;
        const double g = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2) * 3.2;
        if (fabs(g) <= 19.2) { e[(size_t)j] = (int64_t)llround(g); break; }
    }
}
std::vector<int64_t> gen_sk(uint64_t seed, int h) {
    std::vector<int64_t> sk((size_t)N, 0); uint64_t ctr = 0; int placed = 0;
    while (placed < h) { const uint64_t r = sm64(seed, ctr++); const int pos = (int)(r % (uint64_t)N); if (!sk[(size_t)pos]) { sk[(size_t)pos] = (r >> 40) & 1 ? 1 : -1; placed++; } }
    return sk;
}
}  // namespace replay

// ---------------------------------------------------------------- sampling (harness only)
static ChaChaRng &rng(Context *c) { return c->g; }      // one generator per context (image threads own their contexts)
static std::vector<uint64_t> uniform_row(Context *c, uint64_t q) {
    std::vector<uint64_t> r(N); std::uniform_int_distribution<uint64_t> d(0, q - 1); auto &g = rng(c);
    for (auto &x : r) x = d(g);
    return r;
}
static std::vector<int64_t> gaussian(Context *c) {   // sigma = 3.2 (rlwe.DefaultSigma, main.go:421), bound 6 sigma
    std::vector<int64_t> e(N); std::normal_distribution<double> d(0.0, 3.2); auto &g = rng(c);
    for (auto &x : e) { double v; do { v = d(g); } while (fabs(v) > 19.2); x = (int64_t)llround(v); }
    return e;
}
static std::vector<uint64_t> signed_row(const std::vector<int64_t> &v, uint64_t q) {
    std::vector<uint64_t> r(N);
    for (int j = 0; j < N; j++) r[j] = v[j] >= 0 ? (uint64_t)v[j] % q : q - ((uint64_t)(-v[j]) % q);
    return r;
}

// rlwe.GenRotationKeys for one Galois element, restricted to what level-0 key switching reads (digit 0; limbs Q0, P):
// b = -a*sigma_{g^-1}(s) + e + P*s, stored NTT + Montgomery (SURVEY.md 8(a)-R last rows)
static void gen_and_load_galois_key(Context *c, uint64_t galEl) {
    const uint64_t twoN = 2ull * N; uint64_t ginv = 1, b = galEl % twoN;
    for (uint64_t e = twoN - 1; e; e >>= 1, b = (b * b) % twoN) if (e & 1) ginv = (ginv * b) % twoN;
    std::vector<int64_t> sko(N, 0);
    for (int i = 0; i < N; i++) { uint64_t t = ((uint64_t)i * ginv) % twoN; if (t < (uint64_t)N) sko[t] = c->sk[i]; else sko[t - N] = -c->sk[i]; }
    const uint64_t rs = resnetReplaySeed(); int jj = 0; while ((1ull << jj) + 1 < galEl) jj++;       // replay: or_gen_galois_key_l0(sk, 2^j + 1, seed 100 + j) of the oracle network
    std::vector<int64_t> e; if (rs) replay::gauss((100 + (uint64_t)jj) ^ 0xE44E44ull, e); else e = gaussian(c);
    std::vector<uint64_t> rows[4];   // b_q, a_q, b_p, a_p
    const int mods[2] = {0, 2};
    for (int w = 0; w < 2; w++) {
        const int mod = mods[w]; const uint64_t q = MODQ[mod];
        std::vector<uint64_t> a; if (rs) { a.resize(N); replay::fill_seeded(100 + (uint64_t)jj + 0x1000 + (uint64_t)w, q, a.data()); } else a = uniform_row(c, q);
        std::vector<uint64_t> both = signed_row(sko, q), en = signed_row(e, q);
        both.insert(both.end(), en.begin(), en.end());
        both = gpu_ntt(c, mod, both);
        const uint64_t *so = both.data(), *ent = both.data() + N; const std::vector<uint64_t> &si = c->sk_ntt[mod];
        const uint64_t pmod = w == 0 ? PACK_P % q : 0;
        std::vector<uint64_t> bb(N);
        for (int j = 0; j < N; j++) {
            uint64_t v = submod(ent[j], mulmod(a[j], so[j], q), q);
            v = addmod(v, mulmod(pmod, si[j], q), q);
            bb[j] = to_mont(v, q); a[j] = to_mont(a[j], q);
        }
        rows[2 * w] = bb; rows[2 * w + 1] = a;
    }
    HC(c->hc, hc_evk_load(c->hc, galEl, rows[0].data(), rows[1].data(), rows[2].data(), rows[3].data()));
    for (size_t g = 1; g < c->shards.size(); g++) HC(c->shards[g], hc_evk_load(c->shards[g], galEl, rows[0].data(), rows[1].data(), rows[2].data(), rows[3].data()));
    if (galEl - 1 < 32) {       // 2^j+1 with j < 5 leaves the 4096-coefficient tile of the fused kernels: RotateGal takes the general key switch
        std::vector<uint64_t> g; for (int r : {0, 2, 1, 3}) g.insert(g.end(), rows[r].begin(), rows[r].end());     // [digit 0][b | a][Q0, P][N]
        HC(c->hc, hc_swk_load(c->hc, galEl, 0, g.data()));
    }
}

// ---------------------------------------------------------------- newContext (main.go:44-462, kind "Conv")
void applyEnvOptions(hc_ctx *hc, int pack32_default) {
    auto opt = [&](const char *env, const char *name, long dflt) {
        const char *v = getenv(env);
        const long val = (v && *v) ? atol(v) : dflt;
        if (val < 0) return;
        if (hc_set_option(hc, name, val)) panic(std::string("hc_set_option(") + name + "): " + hc_last_error(hc));
    };
    opt("HCONV_ASYNC_ALLOC", "async_alloc", -1);      // first: the allocation mode can only change while the context owns nothing but its tables
    opt("HCONV_SMALL32", "small32", -1);
    opt("HCONV_ROT_FUSE", "rot_fuse", -1);
    opt("HCONV_SMALL_MM_WGS", "small_mm_wgs", -1);    // A/B: 16-row workgroups per pass up to which the batched inverse transforms run on quarter tiles (0: never)
    opt("HCONV_PACK32", "pack32", pack32_default);
}

Context *newContext(int logN, int ker_wid, const std::vector<int> &in_wids, const std::vector<int> &kp_wids, bool boot, const std::string &kind) {
    (void)ker_wid;
    const bool stride_full = kind == "StrConv" || kind == "Imagenet_final_fast";      // the kinds whose stride layer is ext_ctxt with gen_comprs_full (main.go:378-402); "StrConv": that layer alone (not a reference kind)
    if (stride_full && !boot) panic("Wrong kinds! (" + kind + " is a bootstrapping context)");
    if (kind != "Conv" && kind != "Resnet_crop_sparse" && kind != "Resnet_crop_fast" && kind != "Resnet_crop_packed" && kind != "TransConv" && !(kind == "TransConv_sparse" && boot) && !stride_full) panic("Wrong kinds!");       // main.go:404 (the kinds the built command lines use; "TransConv_sparse": TransConv with the log_sparse = 2 bootstrapper)
    Context *c = new Context();
    double logqp = 0; for (uint64_t q : PARAMS6_Q) logqp += log2((double)q); for (uint64_t p : PARAMS6_P) logqp += log2((double)p);
    printf("CKKS parameters: logN = %d, logSlots = %d, h = %d, logQP = %d, levels = %d, scale= 2^%f, sigma = %f \n",
           LOGN, LOGN - 1, 192, (int)llround(logqp), (int)PARAMS6_Q.size(), log2(c->scale), 3.2);       // main.go:85-86
    if ((1 << logN) != N) { printf("Set Boot logN to %d\n", logN); panic("Boot N != N"); }           // main.go:87-90
    c->seed = seedFromEnvironment(); c->g.reseed(c->seed, 0x436f6e76);      // 256 bits from getrandom(2) unless HCONV_SEED asks for deterministic keys
    int dev = getenv("HCONV_DEVICE") ? atoi(getenv("HCONV_DEVICE")) : 0;
    uint64_t q[2] = {MODQ[0], MODQ[1]}, p[1] = {PACK_P};
    if (hc_ctx_create(&c->hc, LOGN, q, 2, p, 1, dev)) panic(std::string("hc_ctx_create: ") + hc_last_error(nullptr));
    applyEnvOptions(c->hc);
    c->shards.push_back(c->hc);
    if (const char *ng = getenv("HCONV_GPUS")) {       // one convolution over G devices (contexts share devices when the box has fewer)
        const int G = atoi(ng); int ndev = 1; hc_device_count(&ndev);
        if (G < 1 || G > 16 || (G & (G - 1))) panic("HCONV_GPUS must be a power of two in 1..16");
        for (int g = 1; g < G; g++) { hc_ctx *h = nullptr; if (hc_ctx_create(&h, LOGN, q, 2, p, 1, (dev + g) % ndev)) panic(std::string("hc_ctx_create: ") + hc_last_error(nullptr)); applyEnvOptions(h); c->shards.push_back(h); }
        if (G > 1) printf("Sharding every convolution over %d device contexts (%d device%s visible)\n", G, ndev, ndev == 1 ? "" : "s");
    }
    // kgen.GenKeyPairSparse(h = 192) (main.go:410)
    c->sk.assign(N, 0);
    if (resnetReplaySeed()) c->sk = replay::gen_sk(resnetReplaySeed(), 192);       // the oracle network's key: Ckks(seed).sk = or_gen_sk(seed, 192)
    else { auto &g = rng(c); int placed = 0; while (placed < 192) { uint64_t r = g(); int pos = (int)(r % N); if (!c->sk[pos]) { c->sk[pos] = (r >> 40) & 1 ? 1 : -1; placed++; } } }
    for (int m = 0; m < 3; m++) c->sk_ntt[m] = gpu_ntt(c, m, signed_row(c->sk, MODQ[m]));
    if (deviceEncrypt()) {      // the secret key on the device once, and the key of the encryptor's draws (the host stream is left as it is when the device path is off)
        c->d_sk = dev_rows(c, 3);
        for (int m = 0; m < 3; m++) HC(c->hc, hc_upload(c->hc, c->d_sk + (size_t)m * N, c->sk_ntt[m].data(), (size_t)N * 8));
        for (uint32_t &w : c->enc_seed8) w = (uint32_t)rng(c)();
        printf("Encryption and decryption on the device (hc_encrypt_sk / hc_decrypt_decode_coeffs)\n");
    }
    printf("Num Rotations:  %d\n", c->num_rotations);                                                  // main.go:412
    // gen_idxNlogs (conv.go:241-261): idx[i] = NTT(X^(2^i)) on the device; Galois keys for 2^(i+1)+1, i < logN
    for (hc_ctx *h : c->shards) HC(h, hc_idx_load(h, nullptr));
    for (int i = 0; i < LOGN; i++) gen_and_load_galois_key(c, (1ull << (i + 1)) + 1);
    if (boot) {                                                                                        // main.go:464-507
        printf("Generating bootstrapping keys...\n");
        auto start = now();
        // DFT matrices and every switching key, same secret key. "Conv" and "Resnet_crop_fast": one full-slot bootstrapper; the sparse resnet kind: the
        // four sparse ones its layers use (btp2..btp5 of main.go:480-500; log_sparse 1..4)
        const bool full = kind == "Conv" || kind == "Resnet_crop_fast" || kind == "Resnet_crop_packed" || kind == "TransConv" || stride_full;
        if (kind == "TransConv_sparse") c->btp = newBoot(c->sk, c->seed, dev, std::vector<int>{2}, imageBatch());      // a quarter of the channel slots live: btp3's slot set alone
        else c->btp = full ? newBoot(c->sk, c->seed, dev, {0}, imageBatch()) : newBoot(c->sk, c->seed, dev, std::vector<int>{2, 1, 3, 4}, imageBatch());
        if (kind == "Resnet_crop_sparse") { bootPrepareCompress(c->btp, in_wids[0], kp_wids[1], 1); bootPrepareCompress(c->btp, in_wids[1], kp_wids[2], 2); }   // main.go:163-215
        // the rotation keys of the stride layer's table, generated with the bootstrapper's own: "StrConv" one (in_wid, kp_wid) at every pos, "Imagenet_final_fast" the first
        // width's at the kept width 2 * kp_wids[1] of the next block, pos 0 and 1 (main.go:390-401)
        if (kind == "StrConv") for (int pos = 0; pos < 4; pos++) bootPrepareCompressFull(c->btp, in_wids[0], kp_wids[0], pos);
        if (kind == "Imagenet_final_fast") for (int pos = 0; pos < 2; pos++) bootPrepareCompressFull(c->btp, in_wids[0], 2 * kp_wids[1], pos);
        printf("Done in %s \n", dur(start).c_str());
    }
    if (kind == "Imagenet_final_fast") {                                                               // main.go:380-384: ext_idx[in_wid][ul] = gen_keep_vec per width
        for (size_t i = 0; i < in_wids.size(); i++) { c->ext_idx[in_wids[i]].resize(2); for (int ul = 0; ul < 2; ul++) c->ext_idx[in_wids[i]][(size_t)ul] = gen_keep_vec(N / 2, in_wids[i], kp_wids[i], ul); }
    }
    if (kind == "Resnet_crop_fast") {                                                                  // main.go:123-136: masks only, no rotation keys
        for (size_t i = 0; i < in_wids.size(); i++) {
            const int step = 1 << i;
            c->ext_idx[step].resize(2);
            for (int ul = 0; ul < 2; ul++) c->ext_idx[step][(size_t)ul] = gen_keep_vec_stride(N / 2, in_wids[0], kp_wids[i], step, ul, kp_wids[i] % 2 != 0);
        }
    }
    if (kind == "Resnet_crop_packed") {                                                                // not a reference kind: the packed layout's masks (hconv_host.hpp), entries of their own
        for (size_t i = 0; i < in_wids.size(); i++) {
            const int step = 1 << i;
            for (int ul = 0; ul < 2; ul++) {
                c->ext_idx[packedMaskKey(step)].push_back(gen_keep_vec_packed(N / 2, in_wids[0], kp_wids[i], step, step, ul));
                if (i) c->ext_idx[packedStrideMaskKey(step)].push_back(gen_keep_vec_packed(N / 2, in_wids[0], kp_wids[i], step, step / 2, ul));
            }
        }
    }
    return c;
}
void freeContext(Context *c) { if (!c) return; freeBoot(c->btp); for (size_t g = 1; g < c->shards.size(); g++) hc_ctx_destroy(c->shards[g]); hc_ctx_destroy(c->hc); delete c; }

// ---------------------------------------------------------------- text I/O and float layout
std::vector<double> readTxt(const std::string &name_file, int size) {      // main.go:971-990
    std::ifstream f(name_file);
    if (!f) panic("open " + name_file + ": no such file or directory");
    std::vector<double> input; std::string w;
    while (f >> w) input.push_back(strtod(w.c_str(), nullptr));
    if (size != 0 && (int)input.size() != size) panic("input size inconsistent!");
    return input;
}
std::vector<double> prep_Input(const std::vector<double> &input, int raw_in_wid, int in_wid, int Nn, int norm, bool trans, bool) {   // main.go:1007-1042
    std::vector<double> out((size_t)Nn, 0.0); int batch = Nn / (in_wid * in_wid), k = 0;
    if (trans) {            // main.go:1011-1021: the raw image on the odd grid points (2i+1, 2j+1) of the in_wid x in_wid frame
        for (int i = 0; i < in_wid / 2; i++) for (int j = 0; j < in_wid / 2; j++) for (int b = 0; b < batch / norm; b++)
            if (i < raw_in_wid && j < raw_in_wid) out[(size_t)((2 * i + 1) * in_wid * batch + (2 * j + 1) * batch + b * norm)] = input[(size_t)k++];
        return out;
    }
    for (int i = 0; i < in_wid; i++) for (int j = 0; j < in_wid; j++) for (int b = 0; b < batch / norm; b++)
        if (i < raw_in_wid && j < raw_in_wid) out[(size_t)(i * in_wid * batch + j * batch + b * norm)] = input[(size_t)k++];
    return out;
}
std::vector<std::vector<double>> reshape_ker(const std::vector<double> &ker_in, int k_sz, int out_batch, bool trans) {   // conv.go:184-202
    int in_batch = (int)ker_in.size() / (k_sz * out_batch);
    std::vector<std::vector<double>> ker_out((size_t)out_batch, std::vector<double>((size_t)(k_sz * in_batch)));
    for (int i = 0; i < out_batch; i++) for (int j = 0; j < in_batch; j++) for (int k = 0; k < k_sz; k++)
        if (trans) ker_out[(size_t)i][(size_t)(j * k_sz + (k_sz - k - 1))] = ker_in[(size_t)(j + i * in_batch + k * out_batch * in_batch)];   // conv.go:192
        else ker_out[(size_t)i][(size_t)(j * k_sz + k)] = ker_in[(size_t)(i + j * out_batch + k * out_batch * in_batch)];
    return ker_out;
}
std::vector<double> encode_ker_final(const std::vector<std::vector<double>> &ker_in, int pos, int i, int in_wid, int in_batch, int ker_wid) {   // conv.go:206-237
    int vec_size = in_wid * in_wid * in_batch, k_sz = ker_wid * ker_wid, bias = pos * ker_wid * ker_wid * in_batch;
    std::vector<double> output((size_t)vec_size, 0.0);
    for (int j = 0; j < in_batch; j++) for (int k = 0; k < k_sz; k++)
        output[(size_t)((in_wid * (k / ker_wid) + k % ker_wid) * in_batch + j)] = ker_in[(size_t)i][(size_t)((in_batch - 1 - j) * k_sz + (k_sz - 1 - k) + bias)];
    int adj = (in_batch - 1) + in_batch * (in_wid + 1) * (ker_wid - 1) / 2;
    std::vector<double> tmp((size_t)adj);
    for (int t = 0; t < adj; t++) { tmp[(size_t)t] = output[(size_t)(vec_size - adj + t)]; output[(size_t)(vec_size - adj + t)] = -output[(size_t)t]; }
    for (int t = 0; t < vec_size - 2 * adj; t++) output[(size_t)t] = output[(size_t)(t + adj)];
    for (int t = 0; t < adj; t++) output[(size_t)(t + vec_size - 2 * adj)] = tmp[(size_t)t];
    return output;
}
std::vector<double> post_process(const std::vector<double> &in_cfs, int raw_in_wid, int in_wid) {     // main.go:1057-1070
    int batch = (int)in_cfs.size() / (in_wid * in_wid);
    std::vector<double> out((size_t)(raw_in_wid * raw_in_wid * batch));
    for (int i = 0; i < raw_in_wid; i++) for (int j = 0; j < raw_in_wid; j++) for (int b = 0; b < batch; b++)
        out[(size_t)(i * raw_in_wid * batch + batch * j + b)] = in_cfs[(size_t)(i * in_wid * batch + batch * j + b)];
    return out;
}
void set_Variables(int batch, int raw_in_wid, int in_wid, int ker_wid, const std::string &kind, int *kp_wid, int *out_batch, int *logN, bool *trans) {   // eval.go:13-54
    int Nn = batch * in_wid * in_wid; *logN = 0; while ((1 << *logN) < Nn) (*logN)++;
    int max_kp_wid = in_wid - ((ker_wid - 1) / 2);
    if (kind == "Conv") {
        *trans = false; *kp_wid = raw_in_wid; *out_batch = batch;
        if (*kp_wid > max_kp_wid) { printf("max raw_in_wid:  %d\n", max_kp_wid); panic("too large raw_in_wid."); }
    } else if (kind == "TransConv") {                                                              // eval.go:41-48
        *trans = true; *kp_wid = 2 * raw_in_wid; *out_batch = batch / 4;
        if (*kp_wid > max_kp_wid) { printf("max raw_in_wid:  %d\n", max_kp_wid / 2); panic("too large raw_in_wid."); }
    } else panic("Wrong kinds!");
}
void printDebugCfsPlain(const std::vector<double> &valuesTest, const std::vector<double> &valuesWant) {   // main.go:694-717
    printf("ValuesTest:"); for (int i = 0; i < 10; i++) printf("%6.10f, ", valuesTest[(size_t)i]); printf("... \n");
    printf("ValuesWant:"); for (int i = 0; i < 10; i++) printf("%6.10f, ", valuesWant[(size_t)i]); printf("... \n");
    std::vector<double> d(valuesWant.size());
    for (size_t i = 0; i < d.size(); i++) d[i] = fabs(valuesWant[i] - valuesTest[i]);
    double mn = *std::min_element(d.begin(), d.end()), mx = *std::max_element(d.begin(), d.end()), mean = 0;
    for (double x : d) mean += x; mean /= (double)d.size();
    std::vector<double> s = d; std::sort(s.begin(), s.end()); double med = s[s.size() / 2];
    auto lg = [](double x) { return log2(1.0 / x); };
    printf("MIN Prec : (%.2f, +Inf) Log2 \nMAX Prec : (%.2f, +Inf) Log2 \nAVG Prec : (%.2f, +Inf) Log2 \nMED Prec : (%.2f, +Inf) Log2 \n", lg(mx), lg(mn), lg(mean), lg(med));
    printf("Err stdF :  -Inf Log2 \nErr stdT :  -Inf Log2 \n\n\n");
}

// ---------------------------------------------------------------- encoder / encryptor / decryptor
// ckks EncodeCoeffs -> scaleUpVecExact: x = uint64(|v|*scale + 0.5) (plain f64), mod q, q - r if v < 0
std::vector<uint64_t> EncodeCoeffs(const std::vector<double> &coeffs, int level, double scale) {
    if ((int)coeffs.size() > N) panic("cannot EncodeCoeffs: too many coefficients");
    std::vector<uint64_t> out((size_t)(level + 1) * N, 0);
    for (size_t i = 0; i < coeffs.size(); i++) {
        const double val = coeffs[i]; const bool neg = val < 0; const double x = neg ? -scale * val : scale * val;
        if (x > 1.8446744073709552e+19) panic("EncodeCoeffs: |value*scale| beyond 2^64 is outside the conv path");
        const uint64_t xi = (uint64_t)(x + 0.5);
        for (int l = 0; l <= level; l++) { uint64_t r = xi % MODQ[l]; out[(size_t)l * N + i] = neg ? MODQ[l] - r : r; }
    }
    return out;
}
bool deviceEncrypt() {
    static const bool v = [] {
        bool replay = resnetReplaySeed() != 0;
        for (const char *n : {"HCONV_CHAIN_REPLAY", "HCONV_CHAIN_REPLAY_BL"}) if (testOnlyEnv(n)) replay = true;
        if (replay) return false;                                             // every committed digest depends on the oracle harness' host draws
        if (const char *e = getenv("HCONV_DEVICE_ENCRYPT")) return atoi(e) != 0;
        return false;                                                         // unset: the host path, until the device path is measured against it (profiles/LEDGER.md)
    }();
    return v;
}
bool deviceEncode() {
    static const bool v = [] {
        if (const char *e = getenv("HCONV_DEVICE_ENCODE")) return atoi(e) != 0;
        return true;                                                          // unset: the device path (set-up times against the host path: profiles/LEDGER.md)
    }();
    return v;
}
std::vector<Ciphertext> EncryptCoeffsBatch(Context *c, const std::vector<const std::vector<double> *> &inputs, int level, double scale) {
    std::vector<Ciphertext> out; const int n = (int)inputs.size();
    if (!deviceEncrypt()) { for (const auto *in : inputs) out.push_back(EncryptNew(c, EncodeCoeffs(*in, level, scale), level, scale)); return out; }
    size_t nvals = 0; for (const auto *in : inputs) nvals = std::max(nvals, in->size());
    if ((int)nvals > N) panic("cannot EncodeCoeffs: too many coefficients");
    std::vector<double> vals((size_t)n * nvals, 0.0);
    for (int z = 0; z < n; z++) std::copy(inputs[(size_t)z]->begin(), inputs[(size_t)z]->end(), vals.begin() + (size_t)z * nvals);
    void *dv = nullptr; HC(c->hc, hc_malloc(c->hc, std::max<size_t>(8, vals.size() * 8), &dv));
    HC(c->hc, hc_upload(c->hc, dv, vals.data(), vals.size() * 8));
    uint64_t *pt = dev_rows(c, (size_t)n * (level + 1));
    HC(c->hc, hc_encode_coeffs(c->hc, (const double *)dv, n, (int)nvals, level, scale, 0, pt));       // HC_ERR_UNSUPPORTED where EncodeCoeffs panics (|value * scale| beyond 2^64)
    std::vector<uint64_t *> ptrs;
    for (int z = 0; z < n; z++) { Ciphertext r; r.d = dev_rows(c, (size_t)2 * (level + 1)); r.level = level; r.Scale = scale; out.push_back(r); ptrs.push_back(r.d); }
    HC(c->hc, hc_encrypt_sk(c->hc, n, level, pt, c->d_sk, c->enc_seed8, c->enc_stream++, ptrs.data()));
    HC(c->hc, hc_free(c->hc, dv)); HC(c->hc, hc_free(c->hc, pt));
    return out;
}
std::vector<std::vector<double>> DecryptDecodeCoeffsBatch(Context *c, const std::vector<Ciphertext> &cts) {
    std::vector<std::vector<double>> out; const int n = (int)cts.size();
    if (!deviceEncrypt()) { for (const Ciphertext &ct : cts) out.push_back(DecryptDecodeCoeffs(c, ct)); return out; }
    std::vector<const uint64_t *> ptrs;
    for (const Ciphertext &ct : cts) { if (ct.level != 0 || ct.Scale != cts[0].Scale) panic("DecryptDecodeCoeffs: level 0 and one scale expected on the conv path"); ptrs.push_back(ct.d); }
    void *dv = nullptr; HC(c->hc, hc_malloc(c->hc, (size_t)n * N * 8, &dv));
    HC(c->hc, hc_decrypt_decode_coeffs(c->hc, n, 0, ptrs.data(), c->d_sk, cts[0].Scale, (double *)dv));
    std::vector<double> all((size_t)n * N); HC(c->hc, hc_download(c->hc, all.data(), dv, all.size() * 8)); HC(c->hc, hc_free(c->hc, dv));
    for (int z = 0; z < n; z++) out.emplace_back(all.begin() + (size_t)z * N, all.begin() + (size_t)(z + 1) * N);
    return out;
}
Ciphertext EncryptNew(Context *c, const std::vector<uint64_t> &pt_rows, int level, double scale) {    // sk-encryption: c0 = -c1*s + e + m
    if (deviceEncrypt()) {                                                    // the same plaintext rows through hc_encrypt_sk (one image)
        uint64_t *pt = dev_upload(c, pt_rows); Ciphertext r; r.d = dev_rows(c, (size_t)2 * (level + 1)); r.level = level; r.Scale = scale;
        HC(c->hc, hc_encrypt_sk(c->hc, 1, level, pt, c->d_sk, c->enc_seed8, c->enc_stream++, &r.d));
        HC(c->hc, hc_free(c->hc, pt));
        return r;
    }
    const uint64_t rs = resnetReplaySeed() ? 5 + 1000 * c->replay_encryptions++ : 0;          // replay: or_encrypt(seed 5) for the first image, as resnet_layer_digests encrypts it
    std::vector<int64_t> e; if (rs) replay::gauss(rs ^ 0xABCDEFull, e); else e = gaussian(c);
    std::vector<uint64_t> ct((size_t)2 * (level + 1) * N);
    for (int l = 0; l <= level; l++) {
        const uint64_t q = MODQ[l];
        std::vector<uint64_t> c1, t = signed_row(e, q);
        if (rs) { c1.resize(N); replay::fill_seeded(rs + 0x2000 + (uint64_t)l, q, c1.data()); } else c1 = uniform_row(c, q);
        for (int j = 0; j < N; j++) t[(size_t)j] = addmod(t[(size_t)j], pt_rows[(size_t)l * N + (size_t)j] % q, q);
        t = gpu_ntt(c, l, t);
        for (int j = 0; j < N; j++) {
            ct[(size_t)l * N + (size_t)j] = submod(t[(size_t)j], mulmod(c1[(size_t)j], c->sk_ntt[l][(size_t)j], q), q);
            ct[(size_t)(level + 1 + l) * N + (size_t)j] = c1[(size_t)j];
        }
    }
    Ciphertext r; r.d = dev_upload(c, ct); r.level = level; r.Scale = scale;
    return r;
}
// Decrypt + DecodeCoeffs of a level-1 ciphertext (what a layer hands on: its scale is whatever the chain's last Rescale left, so the value is reconstructed over q0 q1, as
// bootDecryptDecodeCoeffs does it on the bootstrapper's context)
static std::vector<double> decryptDecodeCoeffsLevel1(Context *c, const Ciphertext &ct) {
    std::vector<uint64_t> sk2((size_t)2 * N);
    for (int l = 0; l < 2; l++) std::copy(c->sk_ntt[l].begin(), c->sk_ntt[l].end(), sk2.begin() + (size_t)l * N);
    uint64_t *d_sk2 = dev_upload(c, sk2), *t = dev_rows(c, 2);
    HC(c->hc, hc_lv_mul_plain(c->hc, 1, ct.d + (size_t)2 * N, d_sk2, t)); HC(c->hc, hc_lv_add(c->hc, 1, ct.d, t, t)); HC(c->hc, hc_lv_intt(c->hc, 1, t, t));
    const std::vector<uint64_t> m = dev_download(c, t, 2);
    HC(c->hc, hc_free(c->hc, t)); HC(c->hc, hc_free(c->hc, d_sk2));
    const uint64_t q0 = MODQ[0], q1 = MODQ[1]; uint64_t inv = 1; { uint64_t b = q0 % q1, e = q1 - 2; while (e) { if (e & 1) inv = mulmod(inv, b, q1); b = mulmod(b, b, q1); e >>= 1; } }
    const u128 QQ = (u128)q0 * q1; std::vector<double> cf((size_t)N);
    for (int j = 0; j < N; j++) {
        const uint64_t a0 = m[(size_t)j], a1 = m[(size_t)N + (size_t)j], d = (a1 % q1 + q1 - a0 % q1) % q1;
        const u128 x = (u128)a0 + (u128)q0 * mulmod(d, inv, q1);
        cf[(size_t)j] = x > QQ / 2 ? -(double)(QQ - x) / ct.Scale : (double)x / ct.Scale;
    }
    return cf;
}
std::vector<double> DecryptDecodeCoeffs(Context *c, const Ciphertext &ct) {       // Decrypt + DecodeCoeffs at level 0 (test.go:59-60); level 1: a layer's output, on the host path
    if (ct.level == 1) return decryptDecodeCoeffsLevel1(c, ct);
    if (ct.level != 0) panic("DecryptDecodeCoeffs: level 0 expected on the conv path");
    if (deviceEncrypt()) return DecryptDecodeCoeffsBatch(c, {ct})[0];
    std::vector<uint64_t> h = dev_download(c, ct.d, 2), m(N);
    const uint64_t q = MODQ[0];
    for (int j = 0; j < N; j++) m[(size_t)j] = addmod(h[(size_t)j], mulmod(h[(size_t)N + (size_t)j], c->sk_ntt[0][(size_t)j], q), q);
    m = gpu_ntt(c, 0, m, true);
    std::vector<double> out(N);
    for (int j = 0; j < N; j++) { uint64_t v = m[(size_t)j]; out[(size_t)j] = (v > q / 2 ? -(double)(q - v) : (double)v) / ct.Scale; }
    return out;
}
void freeCt(Context *c, Ciphertext &ct) { if (ct.d) HC(c->hc, hc_free(c->hc, ct.d)); ct.d = nullptr; }
Ciphertext mergePackedInputs(Context *c, std::vector<Ciphertext> &cts) {
    if (cts.empty() || cts.size() > 4) panic("mergePackedInputs: 1..4 ciphertexts");
    Ciphertext acc = cts[0];
    const size_t poly = (size_t)(acc.level + 1) * N;
    for (size_t g = 1; g < cts.size(); g++) {
        if (cts[g].level != acc.level || cts[g].Scale != acc.Scale) panic("mergePackedInputs: the ciphertexts share level and scale");
        const uint64_t e[2] = {(uint64_t)g, 0};                                 // acc + X^g cts[g]: the channel slot is the innermost coefficient index
        HC(c->hc, hc_lv_op2(c->hc, HC_LV_MONOMIAL, acc.level, acc.d, acc.d + poly, cts[g].d, cts[g].d + poly, acc.d, acc.d + poly, e));
        freeCt(c, cts[g]);
    }
    cts.clear();
    return acc;
}

// ---------------------------------------------------------------- prep_Ker (conv.go:487-518)
KerPlain prep_Ker(Context *c, const std::vector<double> &ker_in, const std::vector<double> &BN_a, int in_wid, int ker_wid,
                  int real_ib, int real_ob, int norm, int ECD_LV, int pos, bool trans, int dilation, int ib_stride, int ob_stride) {
    // The whole of conv.go:487-518 runs on the device (hc_prep_ker / hc_prep_ker_ex: reshape_ker, BN scale, max_bat embedding,
    // encode_ker_final, EncodeCoeffs rounding, ToNTT); reshape_ker/encode_ker_final above remain as the host-side
    // statement of the layout (used by tests and by anyone who wants to inspect a kernel plaintext).
    if (pos != 0 || ECD_LV != 1) panic("prep_Ker: only the conv path's (pos=0, ECD_LV=1) form is built");
    KerPlain k; k.max_bat = N / (in_wid * in_wid); k.Scale = c->scale;
    if (ob_stride < 1 || (long)norm * ob_stride * real_ob > k.max_bat) panic("prep_Ker: norm*ob_stride*real_ob exceeds max_bat");
    auto prep = [&](hc_ctx *h, hc_ker **out) {
        // the "inside" layers' dilated / channel-spread kernels (eval.go:418-431, test.go:484-492) from the undilated weights
        if (dilation != 1 || ib_stride != 1) HC(h, hc_prep_ker_ex2(h, ker_in.data(), (int)ker_in.size(), BN_a.data(), in_wid, ker_wid, real_ib, real_ob, norm, c->scale, trans ? 1 : 0, dilation, ib_stride, out));
        else if (trans) HC(h, hc_prep_ker_ex(h, ker_in.data(), (int)ker_in.size(), BN_a.data(), in_wid, ker_wid, real_ib, real_ob, norm, c->scale, 1, out));
        else HC(h, hc_prep_ker(h, ker_in.data(), (int)ker_in.size(), BN_a.data(), in_wid, ker_wid, real_ib, real_ob, norm, c->scale, out));
        if (ob_stride == 1) return;
        // Output channels ob_stride slots apart (a transposed layer in front of a sparse bootstrapper): plaintext norm*o moves to row norm*ob_stride*o. A row is one
        // plaintext, so no word changes. The library has no call that places the rows (one would be a new entry point of the C ABI), so the move goes through the host:
        // hc_ker_download, the rows re-ordered, hc_ker_load - 2 max_bat rows each way, once per layer, in the set-up the reference spends seconds on.
        const size_t row = (size_t)2 * N;
        std::vector<uint64_t> src((size_t)k.max_bat * row), dst((size_t)k.max_bat * row, 0);
        HC(h, hc_ker_download(h, *out, src.data()));
        for (int o = 0; o < real_ob; o++) std::copy(src.begin() + (size_t)norm * o * row, src.begin() + ((size_t)norm * o + 1) * row, dst.begin() + (size_t)norm * ob_stride * o * row);
        hc_ker_free(h, *out); *out = nullptr;
        HC(h, hc_ker_load(h, dst.data(), k.max_bat, out));
    };
    prep(c->hc, &k.h);
    k.shard_h.push_back(k.h);
    for (size_t g = 1; g < c->shards.size(); g++) { hc_ker *h = nullptr; prep(c->shards[g], &h); k.shard_h.push_back(h); }
    return k;
}

// ---------------------------------------------------------------- GpuEvaluator
Ciphertext GpuEvaluator::alloc(int level, double scale) { Ciphertext r; r.d = dev_rows(cont, (size_t)2 * (level + 1)); r.level = level; r.Scale = scale; return r; }
Ciphertext GpuEvaluator::MulNew(const Ciphertext &ct, const Plaintext &pt) {
    const int level = std::min(ct.level, pt.level);
    Ciphertext r = alloc(level, ct.Scale * pt.Scale);
    for (int p = 0; p < 2; p++) for (int l = 0; l <= level; l++)
        HC(cont->hc, hc_mul(cont->hc, l, ct.d + ((size_t)p * (ct.level + 1) + l) * N, pt.d + (size_t)l * N, r.d + ((size_t)p * (level + 1) + l) * N, 1));
    return r;
}
void GpuEvaluator::SetScale(Ciphertext &ct, double scale) {       // MultByConst(scale/ct.Scale) ; Rescale ; ct.Scale = scale
    const double constant = scale / ct.Scale; double smul = 1;
    for (int p = 0; p < 2; p++) for (int l = 0; l <= ct.level; l++) {
        uint64_t k = hc_const_for(constant, (double)MODQ[ct.level], MODQ[l], &smul);
        uint64_t *row = ct.d + ((size_t)p * (ct.level + 1) + l) * N;
        HC(cont->hc, hc_mul_const(cont->hc, l, row, k, row, 1));
    }
    double sc = ct.Scale * smul; int drops = 0;
    while (ct.level - drops > 0 && sc / (double)MODQ[ct.level - drops] >= scale / 2) { sc /= (double)MODQ[ct.level - drops]; drops++; }
    if (ct.level == 1 && drops == 1) {
        Ciphertext r = alloc(0, scale);
        for (int p = 0; p < 2; p++) HC(cont->hc, hc_div_round_last(cont->hc, 1, ct.d + (size_t)p * 2 * N, r.d + (size_t)p * N));
        HC(cont->hc, hc_free(cont->hc, ct.d));
        ct = r;
    } else if (drops != 0) panic("SetScale: only the level 1 -> 0 rescale of the conv path is built");
    ct.Scale = scale;
}
Ciphertext GpuEvaluator::SubNew(const Ciphertext &a, const Ciphertext &b) {
    if (a.level != b.level) panic("SubNew: level mismatch");
    Ciphertext r = alloc(a.level, a.Scale);
    HC(cont->hc, hc_sub(cont->hc, 0, a.d, b.d, r.d, 2 * (a.level + 1)));    // level 0 on this path: both rows mod Q0
    if (a.level != 0) panic("SubNew: level 0 expected on the pack path");
    return r;
}
void GpuEvaluator::Add(const Ciphertext &a, const Ciphertext &b, Ciphertext &out) {
    if (a.level != 0 || b.level != 0) panic("Add: level 0 expected on the pack path");
    if (!out.d) out = alloc(0, a.Scale);
    HC(cont->hc, hc_add(cont->hc, 0, a.d, b.d, out.d, 2)); out.Scale = a.Scale; out.level = 0;
}
void GpuEvaluator::AddPlain(const Ciphertext &a, const Plaintext &b, Ciphertext &out) {
    if (!out.d) out = alloc(0, a.Scale);
    HC(cont->hc, hc_add(cont->hc, 0, a.d, b.d, out.d, 1));
    if (out.d != a.d) HC(cont->hc, hc_copy(cont->hc, out.d + N, a.d + N, (size_t)N * 8));
    out.Scale = a.Scale; out.level = 0;
}
void GpuEvaluator::RotateGal(const Ciphertext &ct, uint64_t galEl, Ciphertext &out) {
    if (ct.level != 0) panic("RotateGal: level 0 expected on the pack path");
    if (!out.d) out = alloc(0, ct.Scale);
    if (galEl - 1 < 32) {       // evaluator.permuteNTT from the general primitives
        uint64_t *d = dev_rows(cont, 2);
        HC(cont->hc, hc_keyswitch(cont->hc, galEl, 0, ct.d + N, d, d + N));
        HC(cont->hc, hc_add(cont->hc, 0, d, ct.d, d, 1));
        HC(cont->hc, hc_permute(cont->hc, galEl, d, out.d, 1));
        HC(cont->hc, hc_permute(cont->hc, galEl, d + N, out.d + N, 1));
        HC(cont->hc, hc_free(cont->hc, d));
    } else HC(cont->hc, hc_rotate_gal_l0(cont->hc, galEl, ct.d, ct.d + N, out.d, out.d + N));
    out.Scale = ct.Scale; out.level = 0;
}

static void dbg_digest(Context *c, const char *what, const uint64_t *d, size_t rows) {      // HCONV_DBG_STAGES: FNV-1a of device rows, on stderr
    if (!getenv("HCONV_DBG_STAGES")) return;
    std::vector<uint64_t> h = dev_download(c, d, rows); uint64_t f = 1469598103934665603ull;
    for (uint64_t w : h) for (int b = 0; b < 8; b++) { f ^= (w >> (8 * b)) & 0xff; f *= 1099511628211ull; }
    fprintf(stderr, "[stage] %-28s %016llx\n", what, (unsigned long long)f);
}
// ---------------------------------------------------------------- conv_then_pack / evalConv_BN
// pack_ctxts (conv.go:266-300), statement by statement, on the ckks.Evaluator subset (GpuEvaluator = one C-ABI call per
// limb row). This is the path a cgo gpuEvaluator takes when conv.go is left untouched.
static Ciphertext pack_ctxts(Context *c, GpuEvaluator &pack_eval, std::vector<Ciphertext> &ctxts_in, int max_cnum, int real_cnum, const std::vector<Plaintext> &idx) {
    int step = max_cnum / 2;
    const int norm = max_cnum / real_cnum;
    std::vector<Ciphertext> &ctxts = ctxts_in;                       // CopyNew is not needed: the inputs are ours
    for (int i = 0; i < max_cnum; i++) if (i % norm == 0) ctxts[(size_t)i].Scale *= (double)real_cnum;   // conv.go:274
    int logStep = 0;
    for (int i = step; i > 1; i /= 2) logStep++;
    int j = c->logN - logStep;
    while (step >= norm && step >= 1) {
        for (int i = 0; i < step; i += norm) {
            Ciphertext tmp1 = pack_eval.MulNew(ctxts[(size_t)(i + step)], idx[(size_t)logStep]);   // conv.go:288
            Ciphertext tmp2 = pack_eval.SubNew(ctxts[(size_t)i], tmp1);                               // conv.go:289
            pack_eval.Add(ctxts[(size_t)i], tmp1, tmp1);                                              // conv.go:290
            pack_eval.RotateGal(tmp2, (1ull << j) + 1, tmp2);                                         // conv.go:291
            pack_eval.Add(tmp1, tmp2, ctxts[(size_t)i]);                                              // conv.go:292
            freeCt(c, tmp1); freeCt(c, tmp2);
        }
        step /= 2; logStep--; j++;
    }
    return ctxts[0];
}
// conv_then_pack (conv.go:522-546) op by op on the evaluator interface (HCONV_OPWISE=1): must give the same bits
// as the fused kernels.
static Ciphertext conv_then_pack_opwise(Context *c, const Ciphertext &ctxt_in, const KerPlain &pl_ker, int max_ob, int norm, double out_scale) {
    GpuEvaluator pack_evaluator(c);
    auto start = now();
    std::vector<uint64_t> flat((size_t)max_ob * 2 * N);
    HC(c->hc, hc_ker_download(c->hc, pl_ker.h, flat.data()));        // pl_ker[i] as Lattigo holds them (plain NTT rows)
    uint64_t *dker = dev_upload(c, flat);
    std::vector<Ciphertext> ctxt_out((size_t)max_ob);
    for (int i = 0; i < max_ob; i++) if (i % norm == 0) {
        Plaintext pt; pt.d = dker + (size_t)i * 2 * N; pt.level = 1; pt.Scale = pl_ker.Scale;
        ctxt_out[(size_t)i] = pack_evaluator.MulNew(ctxt_in, pt);                                     // conv.go:527
        pack_evaluator.SetScale(ctxt_out[(size_t)i], out_scale / (double)(max_ob / norm));            // conv.go:528
    }
    HC(c->hc, hc_sync(c->hc));
    auto mt = now();
    printf("\t mult time:  %s\n", dur(start).c_str());
    // plain_idx (conv.go:248-253) as device plaintexts
    std::vector<uint64_t> xs((size_t)LOGN * N, 0);
    for (int s = 0; s < LOGN; s++) xs[(size_t)s * N + ((size_t)1 << s)] = 1;
    uint64_t *didx = dev_upload(c, xs);
    HC(c->hc, hc_ntt(c->hc, 0, didx, didx, LOGN));
    std::vector<Plaintext> idx((size_t)LOGN);
    for (int s = 0; s < LOGN; s++) { idx[(size_t)s].d = didx + (size_t)s * N; idx[(size_t)s].level = 0; idx[(size_t)s].Scale = 1.0; }
    Ciphertext res = pack_ctxts(c, pack_evaluator, ctxt_out, max_ob, max_ob / norm, idx);
    HC(c->hc, hc_sync(c->hc));
    printf("\t Pack time:  %s\n", dur(mt).c_str());
    for (int i = 1; i < max_ob; i++) if (ctxt_out[(size_t)i].d) freeCt(c, ctxt_out[(size_t)i]);
    HC(c->hc, hc_free(c->hc, dker)); HC(c->hc, hc_free(c->hc, didx));
    if (out_scale != res.Scale || 0 != res.level) panic("LV or scale after conv then pack, inconsistent");   // conv.go:541-543
    return res;
}

Ciphertext conv_then_pack(Context *c, const Ciphertext &ctxt_in, const KerPlain &pl_ker, int max_ob, int norm, int ECD_LV, double out_scale, const Plaintext *pl_bn_b) {
    (void)ECD_LV;
    if (getenv("HCONV_OPWISE")) return conv_then_pack_opwise(c, ctxt_in, pl_ker, max_ob, norm, out_scale);
    auto start = now();
    Ciphertext r; r.d = dev_rows(c, 2); r.level = 0;
    const int G = (int)c->shards.size();
    if (G > 1 && norm == 1 && max_ob % G == 0 && (int)pl_ker.shard_h.size() == G) {
        // ONE convolution over G devices: replicas of the input by peer copies, then hc_conv_then_pack_sharded (channels i mod G per
        // device, one collection of G x 1 MiB partials on device 0, last log2 G levels there). The two phases overlap across devices,
        // so "mult time" here is the time to queue the work and "Pack time" the time until the result is complete.
        std::vector<uint64_t *> rep((size_t)G); std::vector<const uint64_t *> ins((size_t)G);
        rep[0] = nullptr; ins[0] = ctxt_in.d;
        for (int g = 1; g < G; g++) { void *p = nullptr; HC(c->shards[(size_t)g], hc_malloc(c->shards[(size_t)g], (size_t)4 * N * 8, &p)); rep[(size_t)g] = (uint64_t *)p; ins[(size_t)g] = rep[(size_t)g];
                                      HC(c->shards[(size_t)g], hc_copy_peer(c->shards[(size_t)g], p, c->hc, ctxt_in.d, (size_t)4 * N * 8)); }
        double sc = 0;
        HC(c->hc, hc_conv_then_pack_sharded(c->shards.data(), G, ins.data(), ctxt_in.Scale, pl_ker.shard_h.data(), pl_ker.Scale, max_ob, out_scale, nullptr, r.d, &sc));
        printf("\t mult time:  %s\n", dur(start).c_str());
        auto mt = now();
        HC(c->hc, hc_sync(c->hc));
        printf("\t Pack time:  %s\n", dur(mt).c_str());
        dbg_digest(c, "pack result", r.d, 2);
        for (int g = 1; g < G; g++) { HC(c->shards[(size_t)g], hc_sync(c->shards[(size_t)g])); HC(c->shards[(size_t)g], hc_free(c->shards[(size_t)g], rep[(size_t)g])); }
        r.Scale = sc;
        if (out_scale != r.Scale || 0 != r.level) panic("LV or scale after conv then pack, inconsistent");   // conv.go:541-543
        return r;
    }
    // The reference prints "mult time" and "Pack time" separately (conv.go:533,535); run the two phases through
    // the same fused kernels, synchronising in between only to print the split.
    uint64_t *cts = dev_rows(c, (size_t)max_ob * 2);
    HC(c->hc, hc_conv_mult_phase(c->hc, ctxt_in.d, ctxt_in.Scale, pl_ker.h, pl_ker.Scale, max_ob, norm, out_scale, cts));
    HC(c->hc, hc_sync(c->hc));
    dbg_digest(c, "ct_in", ctxt_in.d, 4); dbg_digest(c, "mult slot 0", cts, 2); dbg_digest(c, "mult slot last", cts + (size_t)(max_ob - 1) * 2 * N, 2); dbg_digest(c, "mult all", cts, (size_t)max_ob * 2);
    auto mt = now();
    printf("\t mult time:  %s\n", dur(start).c_str());
    HC(c->hc, hc_pack_ctxts(c->hc, cts, max_ob, max_ob / norm));
    HC(c->hc, hc_sync(c->hc));
    printf("\t Pack time:  %s\n", dur(mt).c_str());
    dbg_digest(c, "pack result", cts, 2);
    HC(c->hc, hc_copy(c->hc, r.d, cts, (size_t)2 * N * 8));     // keep the pack result (slot 0), drop the workspace
    HC(c->hc, hc_free(c->hc, cts));
    r.Scale = (out_scale / (double)(max_ob / norm)) * (double)(max_ob / norm);            // conv.go:528 then conv.go:274
    if (out_scale != r.Scale || 0 != r.level) panic("LV or scale after conv then pack, inconsistent");   // conv.go:541-543
    (void)pl_bn_b;
    return r;
}
// eval.go:233-243: the bias plaintext of a layer - bn_b[i] on coefficient out_norm*i of every cell of the in_wid grid, encoded at out_scale, level 0, NTT domain
static Plaintext prep_bias(Context *c, const std::vector<double> &bn_b, int in_wid, int out_norm, double out_scale) {
    const int max_batch = N / (in_wid * in_wid);
    std::vector<double> b_coeffs((size_t)N, 0.0);
    for (size_t i = 0; i < bn_b.size(); i++) for (int j = 0; j < in_wid * in_wid; j++) b_coeffs[(size_t)(out_norm * (int)i + j * max_batch)] = bn_b[i];   // eval.go:233-238
    Plaintext pl; pl.level = 0; pl.Scale = out_scale;
    pl.d = dev_upload(c, EncodeCoeffs(b_coeffs, 0, out_scale));
    HC(c->hc, hc_ntt(c->hc, 0, pl.d, pl.d, 1));                                                                        // eval.go:242-243
    HC(c->hc, hc_sync(c->hc));
    return pl;
}
static void free_ker(Context *c, KerPlain &k) { hc_ker_free(c->hc, k.h); for (size_t g = 1; g < k.shard_h.size(); g++) hc_ker_free(c->shards[g], k.shard_h[g]); }

Ciphertext evalConv_BN(Context *c, const Ciphertext &ct_input, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                       const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale, bool trans, int dilation, int ib_stride, int ob_stride) {
    const int max_batch = N / (in_wid * in_wid), out_norm = norm * ob_stride;      // out_norm: the rows out_norm*o hold the output channels; the pack tree and the bias step by it
    auto start = now();
    KerPlain pl_ker = prep_Ker(c, ker_in, bn_a, in_wid, ker_wid, real_ib, real_ob, norm, c->ECD_LV, 0, trans, dilation, ib_stride, ob_stride);      // eval.go:231
    Plaintext pl_bn_b = prep_bias(c, bn_b, in_wid, out_norm, out_scale);
    printf("Plaintext (kernel) preparation, Done in %s \n", dur(start).c_str());                                      // eval.go:244
    start = now();
    dbg_digest(c, "bias plaintext", pl_bn_b.d, 1);
    Ciphertext ct_res = conv_then_pack(c, ct_input, pl_ker, max_batch, out_norm, c->ECD_LV, out_scale, &pl_bn_b);          // eval.go:251
    if (pl_bn_b.Scale != ct_res.Scale || ct_res.level != 0) {                                                          // eval.go:252-257
        printf("plain scale:  %g\nctxt scale:  %g\nctxt lv:  %d\n", pl_bn_b.Scale, ct_res.Scale, ct_res.level);
        panic("LV or scale after conv then pack, inconsistent");
    }
    HC(c->hc, hc_add(c->hc, 0, ct_res.d, pl_bn_b.d, ct_res.d, 1));                                                     // eval.go:258
    HC(c->hc, hc_sync(c->hc));
    printf("Conv (with BN) Done in %s \n", dur(start).c_str());                                                       // eval.go:260
    free_ker(c, pl_ker);
    HC(c->hc, hc_free(c->hc, pl_bn_b.d));
    return ct_res;
}

// HCONV_IMAGE_BATCH (not a reference feature): the reference pushes images through a layer one after another (test.go:128); here up to 8 go through it as
// one set of launches - hc_conv_then_pack_batch for the convolution, hc_set_batch for the bootstrapping chain - with weights, masks, matrices and keys read once
int imageBatch() {
    const char *e = getenv("HCONV_IMAGE_BATCH"); const int n = e ? atoi(e) : 1;
    if (n < 1 || n > 8) panic("HCONV_IMAGE_BATCH must be 1..8");
    return n;
}
std::vector<Ciphertext> conv_then_pack_batch(Context *c, const std::vector<std::vector<Ciphertext>> &groups, const std::vector<const hc_ker *> &kers, double ker_scale, const Plaintext *bias,
                                             int max_batch, int out_norm, double out_scale) {
    const int G = (int)groups.size(), m = (int)kers.size(), n = G * m;
    if (G < 1 || m < 1 || n > 16) panic("conv_then_pack_batch: 1..16 input ciphertexts in all (groups x ciphertexts per group)");
    std::vector<Ciphertext> res((size_t)G); std::vector<const uint64_t *> ins((size_t)n), bs((size_t)n, nullptr); std::vector<const hc_ker *> ks((size_t)n); std::vector<uint64_t *> outs((size_t)n);
    for (int g = 0; g < G; g++) {
        if ((int)groups[(size_t)g].size() != m) panic("conv_then_pack_batch: every group has one input ciphertext per kernel handle");
        res[(size_t)g].d = dev_rows(c, 2); res[(size_t)g].level = 0;
        for (int j = 0; j < m; j++) {
            const Ciphertext &ct = groups[(size_t)g][(size_t)j], &first = groups[0][0]; const size_t z = (size_t)g * m + j;
            if (ct.Scale != first.Scale || ct.level != first.level) panic("conv_then_pack_batch: the input ciphertexts share level and scale");
            ins[z] = ct.d; ks[z] = kers[(size_t)j]; outs[z] = res[(size_t)g].d;
        }
        if (bias) bs[(size_t)g * m] = bias->d;                              // the group's bias is its first member's entry
    }
    double sc = 0;
    if (hc_conv_then_pack_batch(c->hc, n, ins.data(), groups[0][0].Scale, ks.data(), ker_scale, max_batch, out_norm, out_scale, bias ? bs.data() : nullptr, outs.data(), &sc)) panic(std::string("hc_conv_then_pack_batch: ") + hc_last_error(c->hc));   // conv.go:541-543's panic included
    for (Ciphertext &r : res) r.Scale = sc;
    return res;
}
// eval.go:224-263 for the images of a batch: prep_Ker and the bias plaintext once (they depend on the layer only), conv_then_pack + the bias add of all images as ONE launch set
std::vector<Ciphertext> evalConv_BN_batch(Context *c, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                          const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale, bool trans,
                                          int dilation, int ib_stride, int ob_stride) {
    const int n = (int)ct_inputs.size();
    if (n == 1 || getenv("HCONV_OPWISE") || c->shards.size() > 1) {      // one image (the reference's own flow, with its two timers), or modes that exist per image only
        std::vector<Ciphertext> r; for (const Ciphertext &ct : ct_inputs) r.push_back(evalConv_BN(c, ct, ker_in, bn_a, bn_b, in_wid, ker_wid, real_ib, real_ob, norm, out_scale, trans, dilation, ib_stride, ob_stride));
        return r;
    }
    if (n < 1 || n > 16) panic("evalConv_BN_batch: 1..16 images");
    const int max_batch = N / (in_wid * in_wid), out_norm = norm * ob_stride;      // out_norm: the rows out_norm*o hold the output channels; the pack tree and the bias step by it
    auto start = now();
    KerPlain pl_ker = prep_Ker(c, ker_in, bn_a, in_wid, ker_wid, real_ib, real_ob, norm, c->ECD_LV, 0, trans, dilation, ib_stride, ob_stride);      // eval.go:231
    Plaintext pl_bn_b = prep_bias(c, bn_b, in_wid, out_norm, out_scale);
    printf("Plaintext (kernel) preparation, Done in %s \n", dur(start).c_str());                                      // eval.go:244
    start = now();
    std::vector<std::vector<Ciphertext>> groups; for (const Ciphertext &ct : ct_inputs) groups.push_back({ct});         // one input ciphertext per image
    std::vector<Ciphertext> res = conv_then_pack_batch(c, groups, {pl_ker.h}, pl_ker.Scale, &pl_bn_b, max_batch, out_norm, out_scale);
    HC(c->hc, hc_sync(c->hc));
    printf("Conv (with BN) Done in %s  (%d images)\n", dur(start).c_str(), n);                                       // eval.go:260
    free_ker(c, pl_ker);
    HC(c->hc, hc_free(c->hc, pl_bn_b.d));
    return res;
}

// evalConv_BN for a layer whose real_ib = m * ib input channels fill m input ciphertexts (not a reference routine: the reference's networks split the output side only,
// test.go:1499-1541, because with its evaluator an input split costs m pack trees). ker_in is HWIO over all real_ib channels; ciphertext j of a group holds the channels
// j*ib .. (j+1)*ib - 1, and its plaintexts are prep_Ker of that channel slice with the same bn_a. hc_conv_then_pack_batch's grouping rule (members with one ct_out) sums the
// m products at level 1, ahead of the one SetScale, and runs ONE pack tree and ONE bias add per group. groups: the images of a batch, each its m input ciphertexts.
std::vector<Ciphertext> evalConv_BN_multi_batch(Context *c, const std::vector<std::vector<Ciphertext>> &groups, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale) {
    const int G = (int)groups.size(), m = G ? (int)groups[0].size() : 0, n = G * m;
    if (G < 1 || m < 1 || n > 16) panic("evalConv_BN_multi: 1..16 input ciphertexts in all (images x ciphertexts per image)");
    if (real_ib % m) panic("evalConv_BN_multi: the input channels do not divide into the input ciphertexts");
    const int ib = real_ib / m, k_sz = ker_wid * ker_wid;
    if ((int)ker_in.size() != k_sz * real_ib * real_ob) panic("evalConv_BN_multi: kernel size inconsistent");
    const int max_batch = N / (in_wid * in_wid);
    auto start = now();
    std::vector<KerPlain> pl_ker((size_t)m); std::vector<const hc_ker *> kers;
    std::vector<double> slice((size_t)k_sz * ib * real_ob);
    for (int j = 0; j < m; j++) {
        for (int t = 0; t < k_sz; t++) for (int ch = 0; ch < ib; ch++) for (int o = 0; o < real_ob; o++)
            slice[(size_t)o + (size_t)ch * real_ob + (size_t)t * real_ob * ib] = ker_in[(size_t)o + (size_t)(j * ib + ch) * real_ob + (size_t)t * real_ob * real_ib];
        pl_ker[(size_t)j] = prep_Ker(c, slice, bn_a, in_wid, ker_wid, ib, real_ob, norm, c->ECD_LV, 0, false);
        kers.push_back(pl_ker[(size_t)j].h);
    }
    Plaintext pl_bn_b = prep_bias(c, bn_b, in_wid, norm, out_scale);
    printf("Plaintext (kernel) preparation, Done in %s \n", dur(start).c_str());                                      // eval.go:244
    start = now();
    std::vector<Ciphertext> res = conv_then_pack_batch(c, groups, kers, pl_ker[0].Scale, &pl_bn_b, max_batch, norm, out_scale);
    // one launch set does both of conv_then_pack's phases: "mult time" is the time to queue it, "Pack time" the time until the results are complete
    printf("\t mult time:  %s\n", dur(start).c_str());
    auto mt = now();
    HC(c->hc, hc_sync(c->hc));
    printf("\t Pack time:  %s\n", dur(mt).c_str());
    if (G > 1) printf("Conv (with BN) Done in %s  (%d images)\n", dur(start).c_str(), G);
    else printf("Conv (with BN) Done in %s \n", dur(start).c_str());                                                  // eval.go:260
    for (KerPlain &k : pl_ker) free_ker(c, k);
    HC(c->hc, hc_free(c->hc, pl_bn_b.d));
    return res;
}
Ciphertext evalConv_BN_multi(Context *c, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                             const std::vector<double> &bn_b, int in_wid, int ker_wid, int real_ib, int real_ob, int norm, double out_scale) {
    return evalConv_BN_multi_batch(c, {ct_inputs}, ker_in, bn_a, bn_b, in_wid, ker_wid, real_ib, real_ob, norm, out_scale)[0];
}

// ---------------------------------------------------------------- layers of the transposed and the multi-input convolution (not reference routines)
// The hand-over from the convolution context to the bootstrapper's (its own stream), then the tail: everything queued on the convolution context - the stride layers end on a
// product and an addition that nothing has waited for - must be complete before the other stream reads ct_conv
std::vector<BootCiphertext> conv_tail(Context *c, const std::vector<Ciphertext> &ct_conv, const std::string &kind, int log_sparse, double alpha, double pow_, int in_wid, int kp_wid,
                                      const std::vector<std::vector<int>> *keep_idx, const std::string &mask_key, int pack_pos) {
    HC(c->hc, hc_sync(c->hc));
    std::vector<const uint64_t *> conv_d; for (const Ciphertext &ct : ct_conv) conv_d.push_back(ct.d);
    return evalConv_BNRelu_tail_batch(c->btp, kind, log_sparse, conv_d, ct_conv[0].Scale, alpha, pow_, in_wid, kp_wid, keep_idx, mask_key, pack_pos);
}
static void free_cts(Context *c, std::vector<Ciphertext> &cts) { for (Ciphertext &ct : cts) freeCt(c, ct); }
static void free_boot_cts(Context *c, std::vector<BootCiphertext> &cts) { for (BootCiphertext &ct : cts) freeBootCt(c->btp, ct); }
// What evalConv_BNRelu_new is for kind "Conv": the convolution at chain_out_scale, conv_tail. The transposed layer's sparse form asks prep_Ker for ob_stride = 4: with norm = 1
// on the input side (the B input channels fill the slots) the B/4 output channels land on rows 4*o, the pack tree runs with norm = 4 over those rows and the bias sits at
// slots 4*o: every coefficient of the result is on a multiple of 4, which is what the log_sparse = 2 bootstrapper packs into one ciphertext.
std::vector<BootCiphertext> evalTransConv_BNRelu_batch(Context *c, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                       const std::vector<double> &bn_b, double alpha, double pow_, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob,
                                                       bool sparse, std::vector<Ciphertext> *ct_conv_out) {
    if (!c->btp) panic("evalTransConv_BNRelu needs a context built with boot = true");
    if (sparse && 4 * real_ob > N / (in_wid * in_wid)) panic("evalTransConv_BNRelu: the sparse form puts output channel o at slot 4*o");
    std::vector<Ciphertext> ct_conv = evalConv_BN_batch(c, ct_inputs, ker_in, bn_a, bn_b, in_wid, ker_wid, real_ib, real_ob, 1, chain_out_scale(pow_), true, 1, 1, sparse ? 4 : 1);
    std::vector<BootCiphertext> r = conv_tail(c, ct_conv, sparse ? "TransConv_sparse" : "TransConv", sparse ? 2 : 0, alpha, pow_, in_wid, kp_wid);
    if (ct_conv_out) *ct_conv_out = ct_conv; else free_cts(c, ct_conv);
    return r;
}
std::vector<BootCiphertext> evalConv_BNRelu_multi_batch(Context *c, const std::vector<std::vector<Ciphertext>> &groups, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                        const std::vector<double> &bn_b, double alpha, double pow_, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob) {
    if (!c->btp) panic("evalConv_BNRelu_multi needs a context built with boot = true");
    std::vector<Ciphertext> ct_conv = evalConv_BN_multi_batch(c, groups, ker_in, bn_a, bn_b, in_wid, ker_wid, real_ib, real_ob, 1, chain_out_scale(pow_));
    std::vector<BootCiphertext> r = conv_tail(c, ct_conv, "Conv", 0, alpha, pow_, in_wid, kp_wid);
    free_cts(c, ct_conv);
    return r;
}

// ---------------------------------------------------------------- what the layer drivers share
// HCONV_BOOT_STATS lines of the layer commands; sets: also which bootstrappers (slot sets) the context built (testConv_in prints the first two lines only)
static void print_boot_stats(Context *cont, bool sets = true) {
    if (!getenv("HCONV_BOOT_STATS")) return;
    long nk, nks; bootStats(cont->btp, &nk, &nks);
    printf("boot stats: %ld switching keys generated, %ld key switches\n", nk, nks);
    long nd, nm; bool dev; bootEncodeStats(cont->btp, &nd, &nm, &dev); printf("boot stats: %ld diagonals and %ld masks encoded on the %s\n", nd, nm, dev ? "device" : "host");
    if (!sets) return;
    printf("boot stats: bootstrapper sets (log_sparse):"); for (int ls : bootSets(cont->btp)) printf(" %d", ls); printf("\n");
}
static void print_ct_digest(Context *cont, const Ciphertext &ct) {      // FNV-1a over a level-0 ciphertext: lets tests compare code paths bit for bit
    std::vector<uint64_t> h = dev_download(cont, ct.d, 2); uint64_t f = 1469598103934665603ull;
    for (uint64_t w : h) for (int b = 0; b < 8; b++) { f ^= (w >> (8 * b)) & 0xff; f *= 1099511628211ull; }
    printf("ciphertext digest: %016llx\n", (unsigned long long)f);
}
static void print_shapes(Context *cont, int raw_in_wid, int ker_wid, int in_ch, int out_ch) {
    printf("vec size: log2 =  %d\n", cont->logN);
    printf("raw input width:  %d\n", raw_in_wid);
    printf("kernel width:  %d\n", ker_wid);
    printf("num raw batches in & out:  %d ,  %d\n", in_ch, out_ch);
}
// One test case: test_conv_data/test_<stem>_{in,ker,bna,bnb}_<iter>.csv read at the given sizes, and ..._{out,reluout}_<iter>.csv, the expected output of the command without / with the chain
struct TestCase {
    std::string pre, suf;
    std::vector<double> raw_input, ker_in, bn_a, bn_b;
    std::vector<double> expected(bool relu, int size) const { return readTxt(pre + (relu ? "reluout" : "out") + suf, size); }
};
static TestCase read_case(const std::string &stem, int test_iter, int in_size, int ker_size, int out_ch) {
    printf("%d -th iter...start\n", test_iter + 1);
    TestCase t; t.pre = "test_conv_data/test_" + stem + "_"; t.suf = "_" + std::to_string(test_iter) + ".csv";
    t.raw_input = readTxt(t.pre + "in" + t.suf, in_size); t.ker_in = readTxt(t.pre + "ker" + t.suf, ker_size);
    t.bn_a = readTxt(t.pre + "bna" + t.suf, out_ch); t.bn_b = readTxt(t.pre + "bnb" + t.suf, out_ch);
    return t;
}
static std::string case_stem(const char *layer, int ker_wid, int in_batch) { return layer + std::to_string(ker_wid) + "_batch_" + std::to_string(in_batch); }
// ONE EncryptCoeffsBatch call (one launch set on the device path) at the context's level and scale, and its console line
static std::vector<Ciphertext> encrypt_inputs(Context *cont, const std::vector<const std::vector<double> *> &inputs) {
    auto start = now();
    std::vector<Ciphertext> enc = EncryptCoeffsBatch(cont, inputs, cont->ECD_LV, cont->scale);
    printf("Encryption done in %s \n", dur(start).c_str());
    return enc;
}
// cells_of(z, &outside): the driver's output cells of image z, decoded; outside: the stride layer's largest coefficient outside them (the other drivers leave it alone)
typedef std::function<std::vector<double>(int, double *)> CellsOf;
// images 1 .. nimg - 1 of a batch against image 0 and the expected output: independent encryptions of one input decrypt to the same values up to the scheme's noise
static void print_batch_agreement(const std::vector<double> &test_out, const std::vector<double> &real_out, int nimg, const CellsOf &cells_of, bool with_outside = false) {
    for (int z = 1; z < nimg; z++) {
        double oz = 0; const std::vector<double> cz = cells_of(z, &oz);
        double mx = 0, mr = 0; for (size_t i = 0; i < cz.size(); i++) { mx = std::max(mx, fabs(cz[i] - test_out[i])); mr = std::max(mr, fabs(cz[i] - real_out[i])); }
        printf("image %d of the batch: max |difference| to image 0 = %.3g, to the expected output = %.3g", z, mx, mr);
        if (with_outside) printf(", outside the kept cells = %.3g", oz);
        printf("\n");
    }
}
// the report of a test case: image 0 against the expected output (printDebugCfsPlain), then the batch's agreement. decrypt_start: when the decryption began
static void report_case(std::chrono::steady_clock::time_point decrypt_start, const TestCase &tc, bool relu, int out_size, int nimg, const CellsOf &cells_of) {
    double unused = 0; const std::vector<double> test_out = cells_of(0, &unused);
    printf("Decryption Done in %s \n", dur(decrypt_start).c_str());
    const std::vector<double> real_out = tc.expected(relu, out_size);
    printDebugCfsPlain(test_out, real_out);
    print_batch_agreement(test_out, real_out, nimg, cells_of);
}

// ---------------------------------------------------------------- testMultiConv_in (not a reference routine: testConv_in's shape for n_in input ciphertexts)
// n_in * in_batch input channels on the raw width in_wid - ker_wid/2, in_batch output channels: the layer testConv_in runs, with n_in times the input channels. Ours only.
// HCONV_IMAGE_BATCH = g: g independent encryptions of the image as g groups of one call (g * n_in <= 16).
void testMultiConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, int n_in, bool boot) {
    const std::string kind = "Conv";
    const int raw_in_wid = in_wid - ker_wid / 2, norm = 1, m = n_in, px = raw_in_wid * raw_in_wid;
    const int nimg = imageBatch();
    if (nimg * m > 16) panic("multiconv: HCONV_IMAGE_BATCH x n_in must be <= 16 (the members of one hc_conv_then_pack_batch call)");
    int kp_wid, out_batch, logN; bool trans;
    set_Variables(in_batch, raw_in_wid, in_wid, ker_wid, kind, &kp_wid, &out_batch, &logN, &trans);
    Context *cont = newContext(logN, ker_wid, {in_wid}, {kp_wid}, boot, kind);
    print_shapes(cont, raw_in_wid, ker_wid, m * in_batch, out_batch);
    printf("num input ciphertexts:  %d\n", m);
    for (int test_iter = 0; test_iter < total_test_num; test_iter++) {
        const TestCase tc = read_case(case_stem("multiconv", ker_wid, in_batch) + "_in" + std::to_string(m), test_iter, px * m * in_batch, m * in_batch * out_batch * ker_wid * ker_wid, out_batch);
        std::vector<std::vector<double>> input((size_t)m);
        for (int j = 0; j < m; j++) {                                                                  // ciphertext j: the channels j*in_batch .. (j+1)*in_batch - 1
            std::vector<double> part((size_t)px * in_batch);
            for (int p = 0; p < px; p++) for (int ch = 0; ch < in_batch; ch++) part[(size_t)p * in_batch + ch] = tc.raw_input[(size_t)p * m * in_batch + (size_t)j * in_batch + ch];
            input[(size_t)j] = prep_Input(part, raw_in_wid, in_wid, cont->Nn, norm, trans, false);
        }
        std::vector<const std::vector<double> *> ptrs; for (int g = 0; g < nimg; g++) for (int j = 0; j < m; j++) ptrs.push_back(&input[(size_t)j]);
        std::vector<Ciphertext> enc = encrypt_inputs(cont, ptrs);
        std::vector<std::vector<Ciphertext>> groups((size_t)nimg);
        for (int g = 0; g < nimg; g++) groups[(size_t)g].assign(enc.begin() + (size_t)g * m, enc.begin() + (size_t)(g + 1) * m);
        if (boot) {                                                                                    // `multiconvReLU`: testConv_in's boot branch over the groups
            const double pow_ = 4.0, alpha = 0.0;                                                      // test.go:22
            auto layer = now();
            std::vector<BootCiphertext> ct_res = evalConv_BNRelu_multi_batch(cont, groups, tc.ker_in, tc.bn_a, tc.bn_b, alpha, pow_, in_wid, kp_wid, ker_wid, m * in_batch, out_batch);
            if (nimg > 1) printf("Convolution + Bootstrapping + ReLU of %d ciphertexts done in %s \n", nimg, dur(layer).c_str());
            report_case(now(), tc, true, px * out_batch, nimg, [&](int z, double *) { return post_process(bootDecryptDecodeCoeffs(cont->btp, ct_res[(size_t)z]), raw_in_wid, in_wid); });
            print_boot_stats(cont);
            free_cts(cont, enc); free_boot_cts(cont, ct_res);
            continue;
        }
        std::vector<Ciphertext> ct_result = evalConv_BN_multi_batch(cont, groups, tc.ker_in, tc.bn_a, tc.bn_b, in_wid, ker_wid, m * in_batch, out_batch, norm, (double)(1 << 30));
        if (getenv("HCONV_PRINT_DIGEST")) print_ct_digest(cont, ct_result[0]);      // lets tests compare code paths bit for bit
        auto start = now();
        const std::vector<std::vector<double>> dec = DecryptDecodeCoeffsBatch(cont, ct_result);
        report_case(start, tc, false, px * out_batch, nimg, [&](int z, double *) { return post_process(dec[(size_t)z], raw_in_wid, in_wid); });
        free_cts(cont, enc); free_cts(cont, ct_result);
    }
    freeContext(cont);
}

// ---------------------------------------------------------------- testConv_in (test.go:15-74)
void testConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, bool boot) {
    const std::string kind = "Conv";
    const int raw_in_batch = in_batch, raw_in_wid = in_wid - ker_wid / 2, norm = in_batch / raw_in_batch;
    int kp_wid, out_batch, logN; bool trans;
    set_Variables(in_batch, raw_in_wid, in_wid, ker_wid, kind, &kp_wid, &out_batch, &logN, &trans);
    const int raw_out_batch = out_batch / norm, out_size = raw_in_wid * raw_in_wid * raw_in_batch;
    Context *cont = newContext(logN, ker_wid, {in_wid}, {kp_wid}, boot, kind);
    print_shapes(cont, raw_in_wid, ker_wid, raw_in_batch, raw_out_batch);
    // HCONV_IMAGE_BATCH = n > 1 with the bootstrapping chain (not a reference feature): n independent encryptions of the input go through the layer as ONE set of launches
    const int nimg = boot ? imageBatch() : 1;
    for (int test_iter = 0; test_iter < total_test_num; test_iter++) {
        const TestCase tc = read_case(case_stem("conv", ker_wid, in_batch), test_iter, raw_in_wid * raw_in_wid * raw_in_batch, raw_in_batch * raw_out_batch * ker_wid * ker_wid, raw_out_batch);
        const std::vector<double> input = prep_Input(tc.raw_input, raw_in_wid, in_wid, cont->Nn, norm, trans, false);
        std::vector<Ciphertext> enc = encrypt_inputs(cont, std::vector<const std::vector<double> *>((size_t)nimg, &input));
        if (boot) {                                                                                    // test.go:52-53, eval.go:272-607
            const double pow_ = 4.0, alpha = 0.0;                                                      // test.go:22
            std::vector<Ciphertext> ct_conv = evalConv_BN_batch(cont, enc, tc.ker_in, tc.bn_a, tc.bn_b, in_wid, ker_wid, raw_in_batch, raw_out_batch, norm, chain_out_scale(pow_), trans);
            auto layer = now();
            std::vector<BootCiphertext> ct_res = conv_tail(cont, ct_conv, "Conv", 0, alpha, pow_, in_wid, kp_wid);
            if (nimg > 1) printf("Bootstrapping + ReLU of %d ciphertexts done in %s \n", nimg, dur(layer).c_str());
            report_case(now(), tc, true, out_size, nimg, [&](int z, double *) { return post_process(bootDecryptDecodeCoeffs(cont->btp, ct_res[(size_t)z]), raw_in_wid, in_wid); });
            print_boot_stats(cont, false);
            free_cts(cont, enc); free_cts(cont, ct_conv); free_boot_cts(cont, ct_res);
            continue;
        }
        Ciphertext ct_result = evalConv_BN(cont, enc[0], tc.ker_in, tc.bn_a, tc.bn_b, in_wid, ker_wid, raw_in_batch, raw_out_batch, norm, (double)(1 << 30), trans);
        if (getenv("HCONV_PRINT_DIGEST")) print_ct_digest(cont, ct_result);      // lets tests compare code paths bit for bit
        report_case(now(), tc, false, out_size, 1, [&](int, double *) { return post_process(DecryptDecodeCoeffs(cont, ct_result), raw_in_wid, in_wid); });
        free_cts(cont, enc); freeCt(cont, ct_result);
    }
    freeContext(cont);
}

// ---------------------------------------------------------------- testStrConv_in (not a reference routine: testConv_in's boot branch for kind "StrConv")
// The full-packing stride layer alone: B channels on the raw width kp_wid = 2 (in_wid/2 - ker_wid/2) (set_Variables' keep width of the NEXT block, doubled), the
// convolution at the chain's out_scale, the "StrConv" tail at pack_pos = pos. The result lives on the in_wid/2 grid with 4 B channel slots: the stride-2 outputs
// (odd row and column) of channel c at slot c + B pos. test_strconv{k}_batch_{B}_reluout_{t}.csv holds them as (kp_wid/2, kp_wid/2, B); every other coefficient of the
// result is expected to be zero, and the largest one is printed.
void testStrConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, int pos) {
    if (in_wid % 4 != 0) panic("input wid not divisible by 4");
    const int kp_wid = 2 * (in_wid / 2 - ker_wid / 2), raw_in_wid = kp_wid, out_wid = in_wid / 2, raw_out_wid = kp_wid / 2, out_slots = 4 * in_batch, norm = 1;
    Context *cont = newContext(LOGN, ker_wid, {in_wid}, {kp_wid}, true, "StrConv");
    print_shapes(cont, raw_in_wid, ker_wid, in_batch, in_batch);
    printf("stride layer: keep width  %d , pack position  %d , output width  %d , output slots  %d\n", kp_wid, pos, raw_out_wid, out_slots);
    const int nimg = imageBatch();
    // the kept cells: (y', x', c + B pos) of the out_wid grid, y', x' < raw_out_wid; everything else is outside
    auto kept_of = [&](const std::vector<double> &cf, double *outside) {
        std::vector<double> kept((size_t)raw_out_wid * raw_out_wid * in_batch); double mx = 0;
        for (int y = 0; y < out_wid; y++) for (int x = 0; x < out_wid; x++) for (int s = 0; s < out_slots; s++) {
            const double v = cf[(size_t)(y * out_wid + x) * out_slots + s];
            if (y < raw_out_wid && x < raw_out_wid && s / in_batch == pos) kept[(size_t)(y * raw_out_wid + x) * in_batch + (size_t)(s % in_batch)] = v; else mx = std::max(mx, fabs(v));
        }
        *outside = mx; return kept; };
    for (int test_iter = 0; test_iter < total_test_num; test_iter++) {
        const TestCase tc = read_case(case_stem("strconv", ker_wid, in_batch), test_iter, raw_in_wid * raw_in_wid * in_batch, in_batch * in_batch * ker_wid * ker_wid, in_batch);
        const std::vector<double> input = prep_Input(tc.raw_input, raw_in_wid, in_wid, cont->Nn, norm, false, false);
        std::vector<Ciphertext> enc = encrypt_inputs(cont, std::vector<const std::vector<double> *>((size_t)nimg, &input));
        const double pow_ = 4.0, alpha = 0.0;                                                          // test.go:22
        std::vector<Ciphertext> ct_conv = evalConv_BN_batch(cont, enc, tc.ker_in, tc.bn_a, tc.bn_b, in_wid, ker_wid, in_batch, in_batch, norm, chain_out_scale(pow_), false);
        auto layer = now();
        std::vector<BootCiphertext> ct_res = conv_tail(cont, ct_conv, "StrConv", 0, alpha, pow_, in_wid, kp_wid, nullptr, "", pos);
        if (nimg > 1) printf("Bootstrapping + ReLU of %d ciphertexts done in %s \n", nimg, dur(layer).c_str());
        auto start = now();
        std::vector<double> cfs = bootDecryptDecodeCoeffs(cont->btp, ct_res[0]);
        printf("Decryption Done in %s \n", dur(start).c_str());
        if (const char *dump = testOnlyEnv("HCONV_STRCONV_DUMP")) {                                     // test mode: the N decoded coefficients of image 0, raw doubles, for a check outside this driver
            FILE *f = fopen(dump, "wb"); if (!f || fwrite(cfs.data(), sizeof(double), cfs.size(), f) != cfs.size()) panic(std::string("HCONV_STRCONV_DUMP: cannot write ") + dump); fclose(f);
        }
        double outside = 0;
        std::vector<double> test_out = kept_of(cfs, &outside);
        std::vector<double> real_out = tc.expected(true, raw_out_wid * raw_out_wid * in_batch);
        printDebugCfsPlain(test_out, real_out);
        double err = 0; for (size_t i = 0; i < real_out.size(); i++) err = std::max(err, fabs(test_out[i] - real_out[i]));
        printf("stride layer: max |error| on the kept cells = %.6g, max |coefficient| outside them = %.6g\n", err, outside);
        print_batch_agreement(test_out, real_out, nimg, [&](int z, double *oz) { return kept_of(bootDecryptDecodeCoeffs(cont->btp, ct_res[(size_t)z]), oz); }, true);
        print_boot_stats(cont);
        free_cts(cont, enc); free_cts(cont, ct_conv); free_boot_cts(cont, ct_res);
    }
    freeContext(cont);
}

// ---------------------------------------------------------------- testTransConv_in (not a reference routine: testConv_in's shape for kind "TransConv")
// The reference builds the transposed convolution's operators (set_Variables "TransConv", prep_Input / reshape_ker / prep_Ker with trans) but no
// command runs them. Here: raw_in_wid = in_wid/2 - ker_wid/2, real_ib = in_batch, real_ob = in_batch/4, norm = 1; the result is TF's
// conv2d_transpose(strides = 2, padding = 'SAME') on the 2*raw_in_wid grid in the first real_ob channels. Ours only.
void testTransConv_in(int in_batch, int in_wid, int ker_wid, int total_test_num, bool boot, bool sparse) {
    const std::string kind = "TransConv";
    const int raw_in_batch = in_batch, raw_in_wid = in_wid / 2 - ker_wid / 2, norm = 1;
    int kp_wid, out_batch, logN; bool trans;
    set_Variables(in_batch, raw_in_wid, in_wid, ker_wid, kind, &kp_wid, &out_batch, &logN, &trans);
    const int raw_out_batch = out_batch / norm, out_wid = kp_wid, out_size = out_wid * out_wid * raw_out_batch;
    if (sparse && !boot) panic("testTransConv_in: the sparse form is a form of the bootstrapping chain");
    Context *cont = newContext(logN, ker_wid, {in_wid}, {kp_wid}, boot, sparse ? "TransConv_sparse" : kind);
    print_shapes(cont, raw_in_wid, ker_wid, raw_in_batch, raw_out_batch);
    if (sparse) printf("layer kind:  TransConv_sparse  log_sparse 2  (output channel o at slot 4*o)\n");
    const int nimg = imageBatch();
    const int ch_step = sparse ? 4 : 1;                                  // the slots between two output channels
    // test mode, `transconv` only: the convolution at out_scale 2^e instead of 2^30, so that its digest can be set against the layer command's convolution
    const char *ose = boot ? nullptr : testOnlyEnv("HCONV_TRANSCONV_OUT_SCALE_LOG2");
    if (ose && (atoi(ose) < 20 || atoi(ose) > 50)) panic("HCONV_TRANSCONV_OUT_SCALE_LOG2 must be 20..50 (the chain's convolutions run at 2^43, `transconv` at 2^30)");
    const double conv_out_scale = ose ? exp2((double)atoi(ose)) : (double)(1 << 30);
    // the result's first raw_out_batch channels on the out_wid x out_wid grid, [(i*out_wid + j)*raw_out_batch + o]
    auto out_channels = [&](const std::vector<double> &cfs) {
        std::vector<double> all = post_process(cfs, out_wid, in_wid), out((size_t)out_wid * out_wid * raw_out_batch);
        for (int p = 0; p < out_wid * out_wid; p++) for (int o = 0; o < raw_out_batch; o++) out[(size_t)p * raw_out_batch + o] = all[(size_t)p * in_batch + (size_t)ch_step * o];
        return out;
    };
    for (int test_iter = 0; test_iter < total_test_num; test_iter++) {
        const TestCase tc = read_case(case_stem("transconv", ker_wid, in_batch), test_iter, raw_in_wid * raw_in_wid * raw_in_batch, raw_in_batch * raw_out_batch * ker_wid * ker_wid, raw_out_batch);
        const std::vector<double> input = prep_Input(tc.raw_input, raw_in_wid, in_wid, cont->Nn, norm, trans, false);
        // HCONV_IMAGE_BATCH = n > 1: n independent encryptions of the input through ONE set of launches (evalConv_BN_batch)
        std::vector<Ciphertext> ins = encrypt_inputs(cont, std::vector<const std::vector<double> *>((size_t)nimg, &input));
        if (boot) {                                                                                    // `transconvReLU`: testConv_in's boot branch for the transposed layer
            const double pow_ = 4.0, alpha = 0.0;                                                      // test.go:22
            auto layer = now();
            std::vector<Ciphertext> ct_conv;
            std::vector<BootCiphertext> ct_res = evalTransConv_BNRelu_batch(cont, ins, tc.ker_in, tc.bn_a, tc.bn_b, alpha, pow_, in_wid, kp_wid, ker_wid, raw_in_batch, raw_out_batch, sparse, &ct_conv);
            if (nimg > 1) printf("Convolution + Bootstrapping + ReLU of %d ciphertexts done in %s \n", nimg, dur(layer).c_str());
            if (getenv("HCONV_PRINT_DIGEST")) { printf("convolution out_scale: 2^%d\n", (int)lround(log2(ct_conv[0].Scale))); print_ct_digest(cont, ct_conv[0]); }
            report_case(now(), tc, true, out_size, nimg, [&](int z, double *) { return out_channels(bootDecryptDecodeCoeffs(cont->btp, ct_res[(size_t)z])); });
            print_boot_stats(cont);
            free_cts(cont, ins); free_cts(cont, ct_conv); free_boot_cts(cont, ct_res);
            continue;
        }
        std::vector<Ciphertext> ct_result = evalConv_BN_batch(cont, ins, tc.ker_in, tc.bn_a, tc.bn_b, in_wid, ker_wid, raw_in_batch, raw_out_batch, norm, conv_out_scale, trans);
        if (getenv("HCONV_PRINT_DIGEST")) print_ct_digest(cont, ct_result[0]);      // lets tests compare code paths bit for bit
        auto start = now();
        const std::vector<std::vector<double>> dec = DecryptDecodeCoeffsBatch(cont, ct_result);
        report_case(start, tc, false, out_size, nimg, [&](int z, double *) { return out_channels(dec[(size_t)z]); });
        free_cts(cont, ins); free_cts(cont, ct_result);
    }
    freeContext(cont);
}

}  // namespace hconv
