// hconv_resnet.cpp — `resnet <ker> <depth> 1 <n> false` (scope row 8f-3): the reference's encrypted ResNet inference
// (test.go:76-370 testResNet_crop_sparse) on the MI355X engine, and the layer operator it is built from
// (eval.go:272-607 evalConv_BNRelu_new for kinds "Conv_sparse" / "StrConv_sparse").
//
// Reference mapping (file:line -> here):
//   main.go:609-621   CLI `resnet ker depth wide_case test_num cf100` (wide_case 1)        -> conv_main.cpp -> testResNet_crop_sparse
//   test.go:76-370    testResNet_crop_sparse: 7+1+5+1+5 conv-BN-ReLU layers (depth 20), reduce-mean + FC as one convolution,
//                     file formats Resnet_weights/.../w{i}-{conv,a,b}.csv, final-fckernel.csv, final-fcbias.csv,
//                     Resnet_plain_data/.../test_image_{i}.csv, Resnet_enc_results/.../class_result_ker{k}_{i}.csv -> same
//   eval.go:335-392   StrConv_sparse front end: two convolutions on the even / odd output channels at norm/2, X^(norm/4)
//                     shift, add, offset monomial                                                -> evalConv_BNRelu_new
//   eval.go:437-565   bootstrapping (sparse slots), evalReLU, keep_ctxt / ext_double_ctxt, StoC   -> hconv_relu.cpp
//   main.go:920-939   prt_mat_one_norm                                                            -> prt_mat_one_norm
//   test.go:372-636   testResNet_crop_fast_in (`resnet_fast`, not a reference command: main.go:622's alternative driver): every layer on the 32-wide
//                     grid at full slots; kinds "Conv_inside" / "StrConv_inside" (eval.go:295-302, 418-431: dilated kernels through hc_prep_ker_ex2,
//                     the stride layers' input channels spread to ib_stride 2 on the device instead of test.go:484-492's host copy)  -> testResNet_crop
// Weights and images are not shipped with the reference (README.md:23); tests/golden/gen_resnet_csv.py writes synthetic
// ones in the same file layout together with the plain float model's class scores.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <fstream>
#include <mutex>
#include <thread>

#include "hconv_host.hpp"
#include "hconv_sha256.hpp"

namespace hconv {

// conv_tail for the convolution results of one launch set (freed here), and its outputs as blocks of the convolution context
static std::vector<Ciphertext> tail_of_conv(Context *cont, const std::string &kind, int log_sparse, std::vector<Ciphertext> &ct_conv, double alpha, double pow_, int in_wid, int kp_wid,
                                            const std::vector<std::vector<int>> *keep_idx, const std::string &mask_key, int pack_pos = 0) {
    const int nimg = (int)ct_conv.size();
    std::vector<BootCiphertext> r = conv_tail(cont, ct_conv, kind, log_sparse, alpha, pow_, in_wid, kp_wid, keep_idx, mask_key, pack_pos);
    for (Ciphertext &c : ct_conv) freeCt(cont, c);
    // [2][2][N] over (Q0, Q1): what the next convolution reads. The result blocks belong to the bootstrapper's context and go back to it; the layer's outputs are
    // blocks of the convolution context (a block released into a context that did not allocate it would leave the owner's block table pointing at memory it no longer
    // owns - the lifetime bug hc_free's stream synchronisation used to hide). The tail has synchronised its stream, so the copies see the finished results.
    std::vector<Ciphertext> outs((size_t)nimg);
    for (int z = 0; z < nimg; z++) {
        Ciphertext &out = outs[(size_t)z]; out.level = r[(size_t)z].level; out.Scale = r[(size_t)z].Scale;
        const size_t bytes = (size_t)2 * (out.level + 1) * N * 8;
        { void *v = nullptr; HC(cont->hc, hc_malloc(cont->hc, bytes, &v)); out.d = (uint64_t *)v; }
        HC(cont->hc, hc_copy(cont->hc, out.d, r[(size_t)z].d, bytes));
    }
    HC(cont->hc, hc_sync(cont->hc));
    for (BootCiphertext &b : r) freeBootCt(cont->btp, b);
    return outs;
}

// eval.go:272-607 for the kinds the conv / convReLU / resnet command lines reach, for the images of a batch (ct_inputs.size() <= HCONV_IMAGE_BATCH): every image
// sees the operations of the reference's per-image flow, but a launch covers all of them (hc_conv_then_pack_batch; hc_set_batch inside the tail)
std::vector<Ciphertext> evalConv_BNRelu_new_batch(Context *cont, const std::vector<Ciphertext> &ct_inputs, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                                                  const std::vector<double> &bn_b, double alpha, double pow_, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob,
                                                  int norm, int log_sparse, const std::string &kind, int step, int ib_stride, int pack_pos) {
    if (!cont->btp) panic("evalConv_BNRelu_new needs a context built with boot = true");
    const bool inside = kind == "Conv_inside" || kind == "StrConv_inside";
    if (ib_stride != 1 && !inside) panic("evalConv_BNRelu_new: ib_stride is for the inside kinds only");
    const int nimg = (int)ct_inputs.size();
    const double out_scale = chain_out_scale(pow_);
    std::vector<Ciphertext> ct_conv;
    if (kind == "StrConv_sparse") {                                                                       // eval.go:335-392 (modify_ker, !full)
        std::vector<double> a0((size_t)real_ob / 2), a1((size_t)real_ob / 2), b0((size_t)real_ob / 2), b1((size_t)real_ob / 2);
        for (int i = 0; i < real_ob / 2; i++) { a0[(size_t)i] = bn_a[(size_t)(2 * i)]; a1[(size_t)i] = bn_a[(size_t)(2 * i + 1)]; b0[(size_t)i] = bn_b[(size_t)(2 * i)]; b1[(size_t)i] = bn_b[(size_t)(2 * i + 1)]; }
        std::vector<double> k0(ker_in.size() / 2), k1(ker_in.size() / 2);
        for (int k = 0; k < ker_wid * ker_wid; k++) for (int i = 0; i < real_ib; i++) for (int j = 0; j < real_ob / 2; j++) {
            k0[(size_t)(k * real_ib * real_ob / 2 + (i * real_ob / 2 + j))] = ker_in[(size_t)(k * real_ib * real_ob + (i * real_ob + 2 * j))];
            k1[(size_t)(k * real_ib * real_ob / 2 + (i * real_ob / 2 + j))] = ker_in[(size_t)(k * real_ib * real_ob + (i * real_ob + 2 * j + 1))];
        }
        std::vector<Ciphertext> r1 = evalConv_BN_batch(cont, ct_inputs, k0, a0, b0, in_wid, ker_wid, real_ib, real_ob / 2, norm / 2, out_scale, false);
        std::vector<Ciphertext> r2 = evalConv_BN_batch(cont, ct_inputs, k1, a1, b1, in_wid, ker_wid, real_ib, real_ob / 2, norm / 2, out_scale, false);
        const int max_batch = N / (in_wid * in_wid);
        // MulNew(r2, EncodeCoeffs(X^(norm/4))) (eval.go:361-367), AddNew (369) and, for these widths, MulNew by -X^(N - max_batch (in_wid + 1)) (eval.go:377-387; -X^s is
        // X^(N + s)) as ONE pass per image at level 0: HC_LV_MONOMIAL forms the transformed monomials in the kernel
        const uint64_t e[2] = {(uint64_t)(norm / 4), (in_wid - ker_wid / 2) % 2 == 0 ? (uint64_t)(2 * N - max_batch * (in_wid + 1)) : 0};
        for (int z = 0; z < nimg; z++) {
            uint64_t *a = r1[(size_t)z].d, *b = r2[(size_t)z].d;
            HC(cont->hc, hc_lv_op2(cont->hc, HC_LV_MONOMIAL, 0, a, a + N, b, b + N, a, a + N, e));
            freeCt(cont, r2[(size_t)z]);
        }
        ct_conv = r1;
    } else if (kind == "Conv_sparse" || kind == "Conv" || kind == "StrConv") {                            // "StrConv": the stride is the tail's (eval.go:303, 515-519)
        ct_conv = evalConv_BN_batch(cont, ct_inputs, ker_in, bn_a, bn_b, in_wid, ker_wid, real_ib, real_ob, norm, out_scale, false);             // eval.go:433
    } else if (inside) {                                                                                  // eval.go:295-302, 418-431
        if (kind == "StrConv_inside" && step % 2 != 0) panic("step can not be divided by 2 (for strided conv)");
        const int in_step = kind == "StrConv_inside" ? step / 2 : step;
        ct_conv = evalConv_BN_batch(cont, ct_inputs, ker_in, bn_a, bn_b, in_wid, ker_wid, real_ib, real_ob, norm, out_scale, false, in_step, ib_stride);
    } else panic("No kind!");
    const std::vector<std::vector<int>> *keep_idx = nullptr;
    if (inside) {                                                                                         // eval.go:526-528: keep_ctxt(ext_idx[step][ul])
        auto it = cont->ext_idx.find(step);
        if (it == cont->ext_idx.end()) panic("evalConv_BNRelu_new: no ext_idx for step " + std::to_string(step) + " (the inside kinds need a Resnet_crop_fast context)");
        keep_idx = &it->second;
    }
    return tail_of_conv(cont, kind, log_sparse, ct_conv, alpha, pow_, in_wid, kp_wid, keep_idx, "step" + std::to_string(step), pack_pos);
}
Ciphertext evalConv_BNRelu_new(Context *cont, const Ciphertext &ct_input, const std::vector<double> &ker_in, const std::vector<double> &bn_a,
                               const std::vector<double> &bn_b, double alpha, double pow_, int in_wid, int kp_wid, int ker_wid, int real_ib, int real_ob,
                               int norm, int log_sparse, const std::string &kind) {
    return evalConv_BNRelu_new_batch(cont, {ct_input}, ker_in, bn_a, bn_b, alpha, pow_, in_wid, kp_wid, ker_wid, real_ib, real_ob, norm, log_sparse, kind, 1, 1, 0)[0];
}

// main.go:920-939
static std::vector<double> prt_mat_one_norm(const std::vector<double> &vec, int batch, int norm, int sj, int sk) {
    const int mat_size = (int)vec.size() / batch; std::vector<double> out;
    int j = 1, k = 1;
    for (size_t i = 0; i < vec.size(); i += (size_t)batch) {
        if (j == sj && k == sk) {
            out.assign((size_t)(batch / norm), 0.0);
            for (size_t idx = 0; idx < out.size(); idx++) out[idx] = vec[i + (size_t)norm * idx];
            for (double v : out) printf("%.10f ", v);
            printf("\n");
        }
        k++;
        if (k * k > mat_size) { k = 1; j++; }
    }
    return out;
}
// main.go:992-1005
static void writeTxt(const std::string &name, const std::vector<double> &v) {
    std::ofstream f(name, std::ios::trunc);
    if (!f) { fprintf(stderr, "failed creating file: %s\n", name.c_str()); exit(1); }
    char buf[64];
    for (double d : v) { snprintf(buf, sizeof buf, "%.17g\n", d); f << buf; }
}

// ---------------------------------------------------------------- what `resnet`, `resnet_fast` and `resnet_packed` share: the CIFAR-10 network's files, schedule and head
static const int PK_W = 32, PK_SLOTS = 64;                  // the first block's grid and its channel slots (`resnet_fast` and `resnet_packed` stay on it throughout)
static const int RESNET_BATCH[3] = {16, 32, 64};            // the channels of block 1, 2, 3 (test.go:107)
struct ResnetFiles {                                        // test.go:84-105: the directories of (ker_wid, depth), and the layers per block of that depth
    std::string ker_name, weight_dir, out_dir, img_dir;
    int num_blcs[3];
    ResnetFiles(int ker_wid, int depth) : ker_name("ker" + std::to_string(ker_wid)) {
        const std::string tag = "crop_" + ker_name + "_d" + std::to_string(depth) + "_wid1/";
        weight_dir = "Resnet_weights/weights_" + tag; out_dir = "Resnet_enc_results/results_" + tag; img_dir = "Resnet_plain_data/" + tag;
        if (depth == 20) { num_blcs[0] = 7; num_blcs[1] = 5; num_blcs[2] = 5; } else if (depth == 14) { num_blcs[0] = 5; num_blcs[1] = 3; num_blcs[2] = 3; }
        else if (depth == 8) { num_blcs[0] = 3; num_blcs[1] = 1; num_blcs[2] = 1; } else panic("wrong depth (not in 8, 14, 20)!");
    }
    void make_out_dir() const { mkdir("Resnet_enc_results", 0755); mkdir(out_dir.c_str(), 0755); }
    std::vector<double> W(int i, const char *what, int size) const { return readTxt(weight_dir + "w" + std::to_string(i) + "-" + what + ".csv", size); }
    void write_scores(int image, const std::vector<double> &scores) const { writeTxt(out_dir + "class_result_" + ker_name + "_" + std::to_string(image) + ".csv", scores); }
};
// test.go:141-150: test image `iter`, sparse packed - its raw x raw corner on the 32-wide grid, channel b at slot 4b of the 64
static std::vector<double> resnet_input(const ResnetFiles &files, int iter, int ker_wid, int raw) {
    printf("Running  %d -th iter... ker size:  %d\n", iter, ker_wid);
    const std::vector<double> image = readTxt(files.img_dir + "test_image_" + std::to_string(iter) + ".csv", PK_W * PK_W * 3);
    std::vector<double> input((size_t)N, 0.0); int k = 0;
    for (int i = 0; i < PK_W; i++) for (int j = 0; j < PK_W; j++) for (int b = 0; b < 3; b++) {
        if (i < raw && j < raw) input[(size_t)(i * PK_W * PK_SLOTS + j * PK_SLOTS + b * 4)] = image[(size_t)k];
        k++;
    }
    return input;
}
// test.go:160-277: the layers in the reference's order - block 1, the stride layer into block 2, block 2, the stride layer into block 3, block 3 - with its console lines and
// the five stage times. inside(w, cin, blk, pow) runs the layer of the weight files w<w>-*.csv, cin input channels, inside block blk; strided(w, blk, pow) the layer that
// enters blk. pow is init_pow for the first layer, final_pow for the last and mid_pow between (test.go:160, 173, 262).
template <class Inside, class Strided>
static void resnet_schedule(const int num_blcs[3], double init_pow, double mid_pow, double final_pow, const Inside &inside, const Strided &strided, double timings[6]) {
    auto start = now();
    double pow_ = init_pow;                                                                              // ResNet Block 1
    for (int i = 1; i <= num_blcs[0]; i++) {
        inside(i - 1, i == 1 ? 3 : RESNET_BATCH[0], 0, pow_);
        pow_ = mid_pow;
        printf("Block1, Layer  %d done!\n", i);
    }
    printf("Block1 done.\n"); timings[0] = secs(start); start = now();
    strided(num_blcs[0], 1, pow_);                                                                       // test.go:200 / 480-495
    printf("Block1 to 2 done!\n"); timings[1] = secs(start); start = now();
    for (int i = 1; i <= num_blcs[1]; i++) {                                                             // ResNet Block 2
        inside(num_blcs[0] + i, RESNET_BATCH[1], 1, pow_);
        printf("Block2, Layer  %d done!\n", i);
    }
    printf("Block2 done.\n"); timings[2] = secs(start); start = now();
    strided(num_blcs[0] + num_blcs[1] + 1, 2, pow_);                                                     // test.go:225 / 513-529
    printf("Block2 to 3 done!\n"); timings[3] = secs(start); start = now();
    for (int i = 1; i <= num_blcs[2]; i++) {                                                             // ResNet Block 3
        if (i == num_blcs[2]) pow_ = final_pow;
        inside(num_blcs[0] + num_blcs[1] + i + 1, RESNET_BATCH[2], 2, pow_);
        printf("Block3, Layer  %d done!\n", i);
    }
    printf("Block3 done.\n"); timings[4] = secs(start);
}
// test.go:279-334: reduce-mean + FC as ONE convolution - final-fckernel.csv (64 x fc_out) on every one of the kernel's taps, bn_a = 1 / raw^2 (the mean over the last block's
// raw x raw cells), bn_b = final-fcbias.csv
struct FcHead { std::vector<double> ker, bn_a, bn_b; };
static FcHead resnet_fc_head(const ResnetFiles &files, int taps, int fc_out, int raw) {
    const std::vector<double> fc = readTxt(files.weight_dir + "final-fckernel.csv", RESNET_BATCH[2] * fc_out);
    FcHead h; h.bn_b = readTxt(files.weight_dir + "final-fcbias.csv", fc_out);
    h.ker.resize((size_t)taps * fc.size());
    for (size_t i = 0; i < fc.size(); i++) for (int b = 0; b < taps; b++) h.ker[i + (size_t)b * fc.size()] = fc[i];
    h.bn_a.assign((size_t)fc_out, 1.0 / (double)(raw * raw));
    return h;
}
static void print_stage_times(const double t[6]) {
    printf("Blc1:  %g  sec\nBlc1->2:  %g  sec\nBlc2:  %g  sec\nBlc2->3:  %g  sec\nBlc3:  %g  sec\nFinal (reduce_mean & FC):  %g  sec\n", t[0], t[1], t[2], t[3], t[4], t[5]);
}

// test.go:76-370: `resnet ker depth 1 n false` (BASELINE config 5). The wide drivers (wide_case 2 / 3: testResNet_crop_sparse_wide, test.go:638-912) and the CIFAR-100 head
// (cf100: two final convolutions, test.go:287-315) are SURVEY section 2 row 14 - out of scope - and were removed from this host in round 6 (they lived here in rounds 1-5).
// fast = true: test.go:372-636 testResNet_crop_fast_in, the same network, files and console lines; every layer runs on the 32-wide grid at full slots (log_sparse 0),
// norm 4 / 2 / 1, outputs at stride step 1 / 2 / 4 kept in place (ext_idx[step]), the stride layers' weights read with their input channels at ib_stride 2.
static void testResNet_crop(int st, int end, int ker_wid, int depth, bool fast) {
    if (const char *fi = testOnlyEnv("HCONV_RESNET_FIRST_IMAGE")) st = atoi(fi);      // test mode: images st .. end - 1 (one image of a batch run alone, for the batch == single digest test)
    const ResnetFiles files(ker_wid, depth);
    const int fc_out = 10; const double init_pow = 6.0, mid_pow = 6.0, final_pow = 6.0;                  // test.go:84-89 (cifar10)
    const int *real_batch = RESNET_BATCH, norm_sparse[3] = {4, 8, 16}, log_sparse_sparse[3] = {2, 3, 4};      // test.go:107-112
    const int norm_fast[3] = {4, 2, 1}, log_sparse_fast[3] = {0, 0, 0}, steps[3] = {1, 2, 4};                 // test.go:409-411
    const int *norm = fast ? norm_fast : norm_sparse, *log_sparse = fast ? log_sparse_fast : log_sparse_sparse;
    const int logN = 16; const double alpha = 0.0;
    const std::vector<int> in_wids = {32, 16, 8}, raw_in_wids = {32 - ker_wid / 2, 16 - ker_wid / 2, 8 - ker_wid / 2};
    const int ker_size = ker_wid * ker_wid;
    int max_batch[3]; for (int i = 0; i < 3; i++) max_batch[i] = (1 << logN) / (in_wids[(size_t)i] * in_wids[(size_t)i]);
    files.make_out_dir();
    const char *kind_name = fast ? "Resnet_crop_fast" : "Resnet_crop_sparse";
    // one conv-BN-ReLU layer whose output belongs to block blk (strided: the layer that enters it). Sparse: on block blk's grid (a stride layer on the previous one's, its
    // sparse bootstrapper one slot set below: test.go:200, 225). Fast: on the 32-wide grid, the output at stride steps[blk], dilated kernels, a stride layer's input channels at 2c.
    auto layer = [&](Context *cont, const std::vector<Ciphertext> &in, int w, int ib, int ob, int blk, bool strided, double pow_) {
        const std::vector<double> ker = files.W(w, "conv", ib * ob * ker_size), a = files.W(w, "a", ob), b = files.W(w, "b", ob);
        if (fast) return evalConv_BNRelu_new_batch(cont, in, ker, a, b, alpha, pow_, in_wids[0], raw_in_wids[(size_t)blk], ker_wid, ib, ob, norm[blk], 0,
                                                   strided ? "StrConv_inside" : "Conv_inside", steps[blk], strided ? 2 : 1);
        const int gb = strided ? blk - 1 : blk;
        return evalConv_BNRelu_new_batch(cont, in, ker, a, b, alpha, pow_, in_wids[(size_t)gb], raw_in_wids[(size_t)blk], ker_wid, ib, ob, norm[blk],
                                         strided ? log_sparse[gb] - 1 : log_sparse[blk], strided ? "StrConv_sparse" : "Conv_sparse");
    };

    // HCONV_IMAGE_THREADS=K (not a reference feature): K host threads, each with its own context (keys, bootstrappers, stream),
    // classify disjoint shares of the images at the same time. A layer's launches are mostly far below one wave of workgroups, so the
    // images of several streams overlap on the CUs (separate PROCESSES time-slice the device instead: tools/resnet_throughput.py).
    // Measured on MI355X, ResNet-20, 24 images, HCONV_ASYNC_ALLOC=1: 1 thread 4 704 images/hour, 2 threads 5 982, 3 threads 5 553,
    // 4 threads 5 340 (each image is ~60 000 kernel launches; the threads share the runtime's launch path).
    const int nbatch = imageBatch();
    const int n_threads = std::max(1, std::min(getenv("HCONV_IMAGE_THREADS") ? atoi(getenv("HCONV_IMAGE_THREADS")) : 1, (end - st + nbatch - 1) / nbatch));
    if (n_threads > 1) setenv("HCONV_ASYNC_ALLOC", "1", 0);      // several contexts in one process: cached allocations on non-blocking streams, or every hipFree stalls all of them
    std::mutex mu; std::condition_variable cv; int ready = 0; std::chrono::steady_clock::time_point t_go;
    auto run_images = [&](int tix) {
    Context *cont;
    { std::lock_guard<std::mutex> g(mu); cont = newContext(logN, ker_wid, in_wids, raw_in_wids, true, kind_name); }      // one at a time: key generation prints and allocates
    { std::unique_lock<std::mutex> g(mu); if (++ready == n_threads) { t_go = now(); cv.notify_all(); } else cv.wait(g, [&] { return ready == n_threads; }); }
    // images go through the network in groups of HCONV_IMAGE_BATCH (every layer's launches cover the whole group); thread tix takes groups tix, tix + n_threads, ...
    for (int g0 = st + tix * nbatch; g0 < end; g0 += n_threads * nbatch) {
        const int nimg = std::min(nbatch, end - g0);
        std::vector<Ciphertext> ct_layer;
        auto enc_start = now();
        for (int iter = g0; iter < g0 + nimg; iter++) {
            const std::vector<double> input = resnet_input(files, iter, ker_wid, raw_in_wids[0]);
            if (resnetReplaySeed()) cont->replay_encryptions = iter;     // test mode: the encryption randomness of an image depends on its index only, not on which images ran before it in this process
            ct_layer.push_back(EncryptNew(cont, EncodeCoeffs(input, cont->ECD_LV, cont->scale), cont->ECD_LV, cont->scale));
        }
        printf("vec size:  %d\n", N); printf("input width:  [%d %d %d]\n", raw_in_wids[0], raw_in_wids[1], raw_in_wids[2]);
        printf("kernel width:  %d\n", ker_wid); printf("num batches:  [%d %d %d]\n", real_batch[0], real_batch[1], real_batch[2]);
        printf("Encryption done in %s \n", dur(enc_start).c_str());
        double timings[6]; auto begin_start = now();
        int layer_no = 0;
        auto step = [&](std::vector<Ciphertext> next) {
            for (Ciphertext &c : ct_layer) freeCt(cont, c);
            ct_layer = std::move(next);
            if (resnetReplaySeed()) for (size_t z = 0; z < ct_layer.size(); z++) {      // test mode: SHA-256 of the ciphertext the layer hands on ([2][level+1][N], as tests/parity_cases.py sha_ct)
                std::vector<uint64_t> rows((size_t)2 * (ct_layer[z].level + 1) * N); HC(cont->hc, hc_download(cont->hc, rows.data(), ct_layer[z].d, rows.size() * 8));
                Sha256 h; h.update(rows.data(), rows.size() * 8);
                printf("replay digest layer %d image %d level %d scale %.17g %s\n", layer_no, g0 + (int)z, ct_layer[z].level, ct_layer[z].Scale, h.hex().c_str());
            }
            layer_no++;
        };
        resnet_schedule(files.num_blcs, init_pow, mid_pow, final_pow,
                        [&](int w, int cin, int blk, double pow_) { step(layer(cont, ct_layer, w, cin, real_batch[blk], blk, false, pow_)); },
                        [&](int w, int blk, double pow_) { step(layer(cont, ct_layer, w, real_batch[blk - 1], real_batch[blk], blk, true, pow_)); }, timings);
        auto start = now();

        const int fb = fast ? 0 : 2;                                                                     // the grid the FC convolution runs on (fast: test.go:555-600)
        int ker_inf_wid = raw_in_wids[(size_t)fb]; if (ker_inf_wid % 2 == 0) ker_inf_wid++;             // test.go:279-334: reduce_mean + FC
        const FcHead head = resnet_fc_head(files, ker_inf_wid * ker_inf_wid, fc_out, raw_in_wids[2]);
        std::vector<Ciphertext> ct_result = evalConv_BN_batch(cont, ct_layer, head.ker, head.bn_a, head.bn_b, in_wids[(size_t)fb], ker_inf_wid, real_batch[2], fc_out, norm[2], (double)(1 << 30), false);
        printf("Final FC done.\n"); timings[5] = secs(start); start = now();
        printf("\n===============  DECRYPTION  ===============\n\n");
        for (int z = 0; z < nimg; z++) {
            std::vector<double> res_tmp = DecryptDecodeCoeffs(cont, ct_result[(size_t)z]);
            printf("Decryption Done in %s \n", dur(start).c_str());
            std::vector<double> res_out = prt_mat_one_norm(res_tmp, max_batch[fb], norm[2], ker_inf_wid / 2 + 1, ker_inf_wid / 2 + 1);
            res_out.resize((size_t)fc_out);
            printf("\n result:  ["); for (double v : res_out) printf("%.10f ", v);
            printf("]\n");
            files.write_scores(g0 + z, res_out);
            freeCt(cont, ct_layer[(size_t)z]); freeCt(cont, ct_result[(size_t)z]);
        }
        print_stage_times(timings);
        printf("Total done in %s %s\n", dur(begin_start).c_str(), nimg > 1 ? ("(" + std::to_string(nimg) + " images)").c_str() : "");
    }
    { std::lock_guard<std::mutex> g(mu); freeContext(cont); }
    };
    if (n_threads == 1) { run_images(0); return; }
    std::vector<std::thread> th; for (int t = 0; t < n_threads; t++) th.emplace_back(run_images, t);
    for (auto &t : th) t.join();
    // all contexts were ready at t_go; context release is included in the figure below (a few hipFree), image work dominates
    printf("All %d images done in %s  (%d image threads)\n", end - st, dur(t_go).c_str(), n_threads);
}
void testResNet_crop_sparse(int st, int end, int ker_wid, int depth, bool debug) { (void)debug; testResNet_crop(st, end, ker_wid, depth, false); }
void testResNet_crop_fast_in(int st, int end, int ker_wid, int depth, bool debug) { (void)debug; testResNet_crop(st, end, ker_wid, depth, true); }

// ---------------------------------------------------------------- `imagenet ker n [c1]`: test.go:1209-1400 testImagenet_final_fast_in, the reference's ImageNet tail
// Full packing throughout: three c1 -> c1 layers on the 16-grid (kind "Conv"), the stride-2 layer to 2 c1 channels on the 8-grid as two "StrConv" calls on the halves of the
// output channels at pack_pos 0 and 1 and one addition, three 2 c1 -> 2 c1 layers, and the reduce-mean + FC head as one 7 x 7 convolution to 1000 classes whose plaintexts
// come from hc_prep_ker_fc (the FC matrix is uploaded once, not once per tap). File names, the weight numbering (a layer's conv file is w<i>, its BN files w<i+1>: test.go:1293-1296),
// widths, the pow schedule and the console lines are the reference's. c1 = 256 is the reference's network; a smaller c1 (not a reference feature) reads files of c1 / 2 c1
// channels and zero-embeds them into the same 256 / 1024 channel slots, block-2 channel h c1 + j at slot 256 h + j - where the stride layer puts it. Same launches either way.
void testImagenet_final_fast_in(int st, int end, int ker_wid, int c1) {
    const std::string ker_name = "ker" + std::to_string(ker_wid), weight_dir = "weight_imgnet_" + ker_name + "_h5/", img_dir = ker_name + "_data/", out_dir = ker_name + "_enc_result/";
    const int logN = 16, num_blc1 = 3, num_blc2 = 3, full_b1 = 256, full_b2 = 512, fin_out_batch = 1000;
    const std::vector<int> raw_in_wids = {14, 7}, in_wids = {16, 8};
    std::vector<int> kp_wids;
    if (ker_wid == 3) kp_wids = {14, 7}; else if (ker_wid == 5) kp_wids = {14, 6}; else panic("strange ker name!");
    if (c1 < 1 || c1 > full_b1) panic("imagenet: c1 not in 1..256");
    const int real_batch[2] = {c1, 2 * c1}, ker_size = ker_wid * ker_wid, norm = 1;
    Context *cont = newContext(logN, ker_wid, in_wids, kp_wids, true, "Imagenet_final_fast");
    const int max_batch[2] = {N / (in_wids[0] * in_wids[0]), N / (in_wids[1] * in_wids[1])};
    const double alpha = 0.0, init_pow = 6.0, mid_pow = 5.0, final_pow = 6.0;
    mkdir(out_dir.c_str(), 0755);
    auto W = [&](int i, const char *what, int size) { return readTxt(weight_dir + "w" + std::to_string(i) + "-" + what + ".csv", size); };
    auto slot2 = [&](int ch) { return full_b1 * (ch / c1) + ch % c1; };                                    // block-2 channel -> channel slot
    const int nbatch = imageBatch();
    for (int g0 = st; g0 < end; g0 += nbatch) {
        const int nimg = std::min(nbatch, end - g0);
        int weight_num = 10;
        std::vector<std::vector<double>> inputs((size_t)nimg, std::vector<double>((size_t)N, 0.0));
        for (int z = 0; z < nimg; z++) {
            printf("Start  %d -th iter..\n", g0 + z);
            const std::vector<double> raw_input = readTxt(img_dir + "test_image_" + std::to_string(g0 + z) + ".csv", raw_in_wids[0] * raw_in_wids[0] * real_batch[0]);
            for (int i = 0; i < raw_in_wids[0]; i++) for (int j = 0; j < raw_in_wids[0]; j++) for (int b = 0; b < real_batch[0]; b++)
                inputs[(size_t)z][(size_t)(i * in_wids[0] * max_batch[0] + j * max_batch[0] + b)] = raw_input[(size_t)(i * raw_in_wids[0] * real_batch[0] + j * real_batch[0] + b)];
        }
        printf("vec size:  %d\n", N); printf("input width:  [%d %d]\n", raw_in_wids[0], raw_in_wids[1]);
        printf("kernel width:  %d\n", ker_wid); printf("num batches:  [%d %d]\n", real_batch[0], real_batch[1]);
        auto start = now();
        std::vector<const std::vector<double> *> ptrs; for (auto &v : inputs) ptrs.push_back(&v);
        std::vector<Ciphertext> ct_layer = EncryptCoeffsBatch(cont, ptrs, cont->ECD_LV, cont->scale);
        printf("Encryption done in %s \n", dur(start).c_str());
        double timings[4]; auto begin_start = now(); start = now();
        auto step = [&](std::vector<Ciphertext> next) { for (Ciphertext &c : ct_layer) freeCt(cont, c); ct_layer = std::move(next); };

        double pow_ = init_pow;                                                                          // Block 1
        for (int i = 1; i <= num_blc1; i++) {
            const std::vector<double> ker = W(weight_num, "conv", real_batch[0] * real_batch[0] * ker_size); weight_num++;
            const std::vector<double> a = W(weight_num, "a", real_batch[0]), b = W(weight_num, "b", real_batch[0]);
            if (i == num_blc1) pow_ = mid_pow;
            step(evalConv_BNRelu_new_batch(cont, ct_layer, ker, a, b, alpha, pow_, in_wids[0], kp_wids[0], ker_wid, real_batch[0], real_batch[0], norm, 0, "Conv"));
            printf("Block1, Layer  %d done!\n", i);
        }
        printf("Block1 done!\n"); timings[0] = secs(start); start = now();
        {                                                                                                // block 1 to 2: the halves of the output channels at pack_pos 0 and 1
            const std::vector<double> ker = W(weight_num, "conv", real_batch[0] * real_batch[1] * ker_size); weight_num++;
            const std::vector<double> a = W(weight_num, "a", real_batch[1]), b = W(weight_num, "b", real_batch[1]);
            std::vector<Ciphertext> half[2];
            for (int h = 0; h < 2; h++) {
                std::vector<double> kh(ker.size() / 2), ah((size_t)c1), bh((size_t)c1);
                for (int k = 0; k < ker_size; k++) for (int i = 0; i < c1; i++) for (int j = 0; j < c1; j++) kh[(size_t)(k * c1 * c1 + i * c1 + j)] = ker[(size_t)(k * c1 * 2 * c1 + i * 2 * c1 + h * c1 + j)];
                for (int j = 0; j < c1; j++) { ah[(size_t)j] = a[(size_t)(h * c1 + j)]; bh[(size_t)j] = b[(size_t)(h * c1 + j)]; }
                half[h] = evalConv_BNRelu_new_batch(cont, ct_layer, kh, ah, bh, alpha, pow_, in_wids[0], 2 * kp_wids[1], ker_wid, c1, c1, norm, 0, "StrConv", 1, 1, h);
            }
            for (int z = 0; z < nimg; z++) {                                                             // AddNew (test.go:1336)
                Ciphertext &x = half[0][(size_t)z], &y = half[1][(size_t)z];
                if (x.level != y.level || x.Scale != y.Scale) panic("imagenet: the halves of the stride layer differ in level or scale");
                const size_t poly = (size_t)(x.level + 1) * N;
                HC(cont->hc, hc_lv_op2(cont->hc, HC_LV_ADD, x.level, x.d, x.d + poly, y.d, y.d + poly, x.d, x.d + poly, nullptr));
                freeCt(cont, y);
            }
            step(half[0]);
        }
        printf("Block1 to 2 done!\n"); timings[1] = secs(start); start = now();
        for (int i = 1; i <= num_blc2; i++) {                                                            // Block 2, on all 512 channel slots of the layout
            const std::vector<double> ker = W(weight_num, "conv", real_batch[1] * real_batch[1] * ker_size); weight_num++;
            const std::vector<double> a = W(weight_num, "a", real_batch[1]), b = W(weight_num, "b", real_batch[1]);
            std::vector<double> kf((size_t)ker_size * full_b2 * full_b2, 0.0), af((size_t)full_b2, 0.0), bf((size_t)full_b2, 0.0);
            for (int k = 0; k < ker_size; k++) for (int ci = 0; ci < real_batch[1]; ci++) for (int co = 0; co < real_batch[1]; co++)
                kf[((size_t)k * full_b2 + (size_t)slot2(ci)) * full_b2 + (size_t)slot2(co)] = ker[((size_t)k * real_batch[1] + ci) * real_batch[1] + co];
            for (int co = 0; co < real_batch[1]; co++) { af[(size_t)slot2(co)] = a[(size_t)co]; bf[(size_t)slot2(co)] = b[(size_t)co]; }
            if (i == num_blc2) pow_ = final_pow;
            step(evalConv_BNRelu_new_batch(cont, ct_layer, kf, af, bf, alpha, pow_, in_wids[1], kp_wids[1], ker_wid, full_b2, full_b2, norm, 0, "Conv"));
            printf("Block2, Layer  %d done!\n", i);
        }
        printf("Block2 done!\n"); timings[2] = secs(start); start = now();
        std::vector<Ciphertext> ct_result((size_t)nimg);                                                 // RMFC (test.go:1359-1384): bn_a = the mean's factor, no bias
        {
            const std::vector<double> fc = readTxt(weight_dir + "fc.csv", real_batch[1] * fin_out_batch);
            std::vector<double> fcf((size_t)full_b2 * fin_out_batch, 0.0);
            for (int ci = 0; ci < real_batch[1]; ci++) std::copy(fc.begin() + (long)ci * fin_out_batch, fc.begin() + (long)(ci + 1) * fin_out_batch, fcf.begin() + (long)slot2(ci) * fin_out_batch);
            const std::vector<double> bn_af((size_t)fin_out_batch, ker_wid == 3 ? 1.0 / (7 * 7) : 1.0 / (6 * 6));
            const double out_scale = (double)(1 << 30);
            auto t0 = now();
            KerPlain pl_ker; pl_ker.max_bat = max_batch[1]; pl_ker.Scale = cont->scale;
            HC(cont->hc, hc_prep_ker_fc(cont->hc, fcf.data(), bn_af.data(), in_wids[1], 7, full_b2, fin_out_batch, norm, cont->scale, 1, &pl_ker.h));
            HC(cont->hc, hc_sync(cont->hc));
            printf("Plaintext (kernel) preparation, Done in %s \n", dur(t0).c_str());
            t0 = now();
            if (nimg == 1) ct_result[0] = conv_then_pack(cont, ct_layer[0], pl_ker, max_batch[1], norm, cont->ECD_LV, out_scale, nullptr);
            else {
                std::vector<std::vector<Ciphertext>> groups; for (const Ciphertext &c : ct_layer) groups.push_back({c});
                ct_result = conv_then_pack_batch(cont, groups, {pl_ker.h}, pl_ker.Scale, nullptr, max_batch[1], norm, out_scale);
                HC(cont->hc, hc_sync(cont->hc));
            }
            if (nimg > 1) printf("Conv (with BN) Done in %s  (%d images)\n", dur(t0).c_str(), nimg); else printf("Conv (with BN) Done in %s \n", dur(t0).c_str());
            hc_ker_free(cont->hc, pl_ker.h);
        }
        timings[3] = secs(start);
        for (int z = 0; z < nimg; z++) {
            start = now();
            std::vector<double> res_tmp = DecryptDecodeCoeffs(cont, ct_result[(size_t)z]);
            printf("Decryption done in %s \n", dur(start).c_str());
            std::vector<double> final_result = prt_mat_one_norm(res_tmp, max_batch[1], 1, 4, 4);        // cell (3, 3) of the 8-grid: the centre of the 7 x 7 window
            final_result.resize((size_t)fin_out_batch);
            writeTxt(out_dir + "enc_result_" + std::to_string(g0 + z) + ".csv", final_result);
            freeCt(cont, ct_layer[(size_t)z]); freeCt(cont, ct_result[(size_t)z]);
        }
        printf("Blc1:  %g  sec\nBlc1->2:  %g  sec\nBlc2:  %g  sec\nFinal (reduce_mean & FC):  %g  sec\n", timings[0], timings[1], timings[2], timings[3]);
        printf("Total done in %s \n", dur(begin_start).c_str());                                       // test.go:1398
        if (nimg > 1) printf("(%d images of one launch set)\n", nimg);
    }
    freeContext(cont);
}

// ---------------------------------------------------------------- `resnet_packed` (not a reference command): the network of `resnet_fast` with every coefficient in use
// The layout, the slot assignment (packed_slot) and the expanded kernels are stated in hconv_host.hpp; DESIGN.md "The packed layout" says why the stride layers merge after the mask.
// Every convolution is 64 slots to 64 slots at norm 1: the block-diagonal expansion of the layer's weights through hc_prep_ker_ex2, dilated by the input lattice's step.
// the tails of convolution results (freed here) in launch sets of HCONV_IMAGE_BATCH, kept with the context's ext_idx[mask_id]
static std::vector<Ciphertext> packed_tails(Context *cont, std::vector<Ciphertext> &ct_conv, const char *kind, double alpha, double pow_, int kp_wid, int mask_id, const std::string &mask_key) {
    auto it = cont->ext_idx.find(mask_id);
    if (it == cont->ext_idx.end()) panic("resnet_packed: no ext_idx entry " + std::to_string(mask_id) + " (a Resnet_crop_packed context holds the packed masks)");
    std::vector<Ciphertext> outs; const size_t nb = (size_t)imageBatch();
    for (size_t i0 = 0; i0 < ct_conv.size(); i0 += nb) {
        std::vector<Ciphertext> set(ct_conv.begin() + (long)i0, ct_conv.begin() + (long)std::min(ct_conv.size(), i0 + nb));
        for (const Ciphertext &c : tail_of_conv(cont, kind, 0, set, alpha, pow_, PK_W, kp_wid, &it->second, mask_key)) outs.push_back(c);
    }
    ct_conv.clear();
    return outs;
}
// a layer inside block blk (norm, step s, keep width raw): ONE kernel preparation and one convolution call for the group's ciphertexts, then their tails with the all-phases mask
static std::vector<Ciphertext> packed_layer(Context *cont, const std::vector<Ciphertext> &in, const std::vector<double> &ker, const std::vector<double> &a, const std::vector<double> &b,
                                            double alpha, double pow_, int ker_wid, int cin, int cout, int norm, int s, int raw) {
    std::vector<Ciphertext> ct_conv = evalConv_BN_batch(cont, in, packed_expand_ker(ker, ker_wid * ker_wid, cin, cout, norm, norm, 0, norm, PK_SLOTS), packed_expand_bn(a, norm), packed_expand_bn(b, norm),
                                                        PK_W, ker_wid, PK_SLOTS, PK_SLOTS, 1, chain_out_scale(pow_), false, s, 1);
    return packed_tails(cont, ct_conv, "Conv_inside", alpha, pow_, raw, packedMaskKey(s), "packed" + std::to_string(s));
}
// the stride layer that enters the block of (norm, step s, keep width raw) from the block of (2 norm, s / 2). Result r = 2q + h is input ciphertext q convolved with the kernel of
// half h of its channel offsets, through a tail of its own whose mask keeps the (s/2)^2 phases those images reach by themselves; only then do results 4o .. 4o + 3 meet in output
// ciphertext o, result 4o + t moved by (s/2) * (t / 2, t mod 2) cells. (Merging BEFORE the tails - two inputs into one convolution - fails: a stride layer's convolution is computed
// at every cell of the input lattice, and the three quarters of its outputs that the mask drops would land on the cells of the images merged in.)
static std::vector<Ciphertext> packed_stride_layer(Context *cont, const std::vector<Ciphertext> &in, const std::vector<double> &ker, const std::vector<double> &a, const std::vector<double> &b,
                                                   double alpha, double pow_, int ker_wid, int cin, int cout, int norm, int s, int raw) {
    const size_t nin = in.size();
    std::vector<Ciphertext> ct_conv(2 * nin);
    for (int h = 0; h < 2; h++) {
        std::vector<Ciphertext> r = evalConv_BN_batch(cont, in, packed_expand_ker(ker, ker_wid * ker_wid, cin, cout, 2 * norm, norm, h * norm, norm, PK_SLOTS), packed_expand_bn(a, norm), packed_expand_bn(b, norm),
                                                      PK_W, ker_wid, PK_SLOTS, PK_SLOTS, 1, chain_out_scale(pow_), false, s / 2, 1);
        for (size_t q = 0; q < nin; q++) ct_conv[2 * q + (size_t)h] = r[q];
    }
    std::vector<Ciphertext> res = packed_tails(cont, ct_conv, "StrConv_inside", alpha, pow_, raw, packedStrideMaskKey(s), "packedstride" + std::to_string(s));
    std::vector<Ciphertext> outs;
    for (size_t r = 0; r < res.size(); r++) {
        const int t = (int)(r % 4);
        if (t == 0) { outs.push_back(res[r]); continue; }
        Ciphertext &acc = outs.back(); const size_t poly = (size_t)(acc.level + 1) * N;
        if (res[r].level != acc.level || res[r].Scale != acc.Scale) panic("resnet_packed: the results of a stride layer share level and scale");
        // whole cells: (dy, dx) is the exponent (32 dy + dx) * 64; the live cells end at row and column (s/2 - 1) + s (raw - 1) + s/2 < 32, so none wraps past the ring's end
        const uint64_t e[2] = {(uint64_t)((PK_W * (s / 2) * (t / 2) + (s / 2) * (t % 2)) * PK_SLOTS), 0};
        HC(cont->hc, hc_lv_op2(cont->hc, HC_LV_MONOMIAL, acc.level, acc.d, acc.d + poly, res[r].d, res[r].d + poly, acc.d, acc.d + poly, e));
        freeCt(cont, res[r]);
    }
    HC(cont->hc, hc_sync(cont->hc));
    return outs;
}
// HCONV_PACKED_DUMP_LAYERS (test mode): every image slot of a ciphertext the layer hands on, unpacked to its raw x raw x C activation (an observer: the ciphertext is only read)
static void packed_dump(Context *cont, const std::vector<Ciphertext> &cts, int blk, int layer_no, int g0, int nimg, int raw, int C, const std::string &out_dir) {
    const int norm = 4 >> blk, s = 1 << blk;
    for (size_t z = 0; z < cts.size(); z++) {
        const std::vector<double> cf = DecryptDecodeCoeffs(cont, cts[z]);          // level 1, the chain's own scale: reconstructed over q0 q1
        for (int m = 0; m < nimg; m++) {
            const PackedSlot p = packed_slot(blk, m);
            if (p.ct != (int)z) continue;
            std::vector<double> act((size_t)raw * raw * C);
            for (int i = 0; i < raw; i++) for (int j = 0; j < raw; j++) for (int c = 0; c < C; c++)
                act[((size_t)i * raw + j) * C + c] = cf[((size_t)(p.py + s * i) * PK_W + (size_t)(p.px + s * j)) * PK_SLOTS + (size_t)(norm * c + p.g)];
            writeTxt(out_dir + "packed_act_L" + std::to_string(layer_no) + "_" + std::to_string(g0 + m) + ".csv", act);
        }
    }
}
void testResNet_crop_packed(int st, int end, int ker_wid, int depth) {
    if (ker_wid != 3 && ker_wid != 7) panic("resnet_packed: kernel width 3 or 7 (the even keep widths of 5 put init at step - 1)");
    const ResnetFiles files(ker_wid, depth);
    const int fc_out = 10; const double init_pow = 6.0, mid_pow = 6.0, final_pow = 6.0, alpha = 0.0;     // resnet_fast's (test.go:84-89)
    const int *real_batch = RESNET_BATCH, norm[3] = {4, 2, 1}, steps[3] = {1, 2, 4};
    const std::vector<int> in_wids = {32, 16, 8}, raw = {32 - ker_wid / 2, 16 - ker_wid / 2, 8 - ker_wid / 2};
    const int ker_size = ker_wid * ker_wid;
    std::vector<int> dump_layers;
    if (const char *dl = testOnlyEnv("HCONV_PACKED_DUMP_LAYERS")) for (const char *p = dl; *p;) {
        char *e; const long v = strtol(p, &e, 10);
        if (e == p || (*e && *e != ',')) panic("HCONV_PACKED_DUMP_LAYERS: a comma list of layer numbers");
        dump_layers.push_back((int)v); p = *e ? e + 1 : e;
    }
    files.make_out_dir();
    Context *cont = newContext(LOGN, ker_wid, in_wids, raw, true, "Resnet_crop_packed");
    auto run_start = now();
    for (int g0 = st; g0 < end; g0 += PACKED_GROUP) {
        const int nimg = std::min(PACKED_GROUP, end - g0);
        std::vector<Ciphertext> ct_layer;
        auto enc_start = now();
        for (int q0 = 0; q0 < nimg; q0 += 4) {                                                          // block 0: images 4q .. 4q + 3 of the group into ciphertext q
            std::vector<Ciphertext> four;
            for (int m = q0; m < std::min(nimg, q0 + 4); m++) {
                const std::vector<double> input = resnet_input(files, g0 + m, ker_wid, raw[0]);                   // as resnet_fast encodes it
                four.push_back(EncryptNew(cont, EncodeCoeffs(input, cont->ECD_LV, cont->scale), cont->ECD_LV, cont->scale));
            }
            ct_layer.push_back(mergePackedInputs(cont, four));
        }
        HC(cont->hc, hc_sync(cont->hc));
        printf("Encryption done in %s  (%d images in %zu ciphertexts)\n", dur(enc_start).c_str(), nimg, ct_layer.size());
        double timings[6]; auto begin_start = now();
        int layer_no = 0;
        auto step = [&](std::vector<Ciphertext> next, int blk) {
            for (Ciphertext &c : ct_layer) freeCt(cont, c);
            ct_layer = std::move(next);
            if (std::find(dump_layers.begin(), dump_layers.end(), layer_no) != dump_layers.end()) packed_dump(cont, ct_layer, blk, layer_no, g0, nimg, raw[(size_t)blk], real_batch[blk], files.out_dir);
            layer_no++;
        };
        resnet_schedule(files.num_blcs, init_pow, mid_pow, final_pow,
                        [&](int w, int cin, int blk, double pow_) {
                            step(packed_layer(cont, ct_layer, files.W(w, "conv", cin * real_batch[blk] * ker_size), files.W(w, "a", real_batch[blk]), files.W(w, "b", real_batch[blk]), alpha, pow_, ker_wid,
                                              cin, real_batch[blk], norm[blk], steps[blk], raw[(size_t)blk]), blk); },
                        [&](int w, int blk, double pow_) {
                            step(packed_stride_layer(cont, ct_layer, files.W(w, "conv", real_batch[blk - 1] * real_batch[blk] * ker_size), files.W(w, "a", real_batch[blk]), files.W(w, "b", real_batch[blk]), alpha, pow_,
                                                     ker_wid, real_batch[blk - 1], real_batch[blk], norm[blk], steps[blk], raw[(size_t)blk]), blk); }, timings);
        auto start = now();

        // reduce-mean and FC as ONE convolution at norm 1: raw[2] x raw[2] taps of the FC weights over raw[2]^2, dilated by 4, so that a tap set reads the cells of ONE phase
        // (resnet_fast's undilated 31-wide kernel would sum across the phases). The image at phase (py, px) has its scores at cell (kd/2 + py, kd/2 + px).
        const int kd = steps[2] * (raw[2] - 1) + 1;
        const FcHead head = resnet_fc_head(files, raw[2] * raw[2], fc_out, raw[2]);
        std::vector<Ciphertext> ct_result = evalConv_BN_batch(cont, ct_layer, head.ker, head.bn_a, head.bn_b, PK_W, raw[2], real_batch[2], fc_out, 1, (double)(1 << 30), false, steps[2], 1);
        printf("Final FC done.\n"); timings[5] = secs(start); start = now();
        printf("\n===============  DECRYPTION  ===============\n\n");
        const std::vector<double> res_tmp = DecryptDecodeCoeffs(cont, ct_result[0]);
        printf("Decryption Done in %s \n", dur(start).c_str());
        for (int m = 0; m < nimg; m++) {
            const PackedSlot p = packed_slot(2, m);
            std::vector<double> res_out((size_t)fc_out);
            for (int o = 0; o < fc_out; o++) res_out[(size_t)o] = res_tmp[((size_t)(kd / 2 + p.py) * PK_W + (size_t)(kd / 2 + p.px)) * PK_SLOTS + (size_t)o];
            printf("\n result %d:  [", g0 + m); for (double v : res_out) printf("%.10f ", v);
            printf("]\n");
            files.write_scores(g0 + m, res_out);
        }
        for (Ciphertext &c : ct_layer) freeCt(cont, c);
        for (Ciphertext &c : ct_result) freeCt(cont, c);
        print_stage_times(timings);
        printf("Total done in %s (%d images)\n", dur(begin_start).c_str(), nimg);
    }
    printf("All %d images done in %s  (first encryption to last result)\n", end - st, dur(run_start).c_str());
    freeContext(cont);
}

}  // namespace hconv
