// conv_main.cpp — the reference's CLI surface (main.go:578-645) over the MI355X engine:
//     conv <ker_wid 3|5|7> <i_batch 0..3> <num_tests <= 10>
// prints the same line shapes as the reference's `conv` run (SURVEY.md 8(a)-S "CLI output contract").
// It runs the slot-packed "Base Line" (hconv_bl.cpp, scope row 8f-2) and then "Ours" (hconv_host.cpp), as main.go:639-643 does.
// `convReLU k i n` runs both with their bootstrapping chains (hconv_relu.cpp, scope row 8f-1: the baseline's stock Bootstrapp over
// parameter set [7] and Ours' CtoS / StoC over set [6]); `resnet ker depth 1 n false` runs the encrypted ResNet inference (hconv_resnet.cpp, scope row 8f-3).
// `transconv <ker_wid 3|5|7> <i_batch 0..3> <num_tests <= 10>` (not a reference command; the reference builds TransConv's operators but runs
// none of them): stride-2 transposed convolution, Ours only (the reference's baseline side of it is unfinished), on
// test_conv_data/test_transconv{k}_batch_{B}_{in,ker,bna,bnb,out}_{t}.csv with raw width widths[i]/2 - k/2, B in and B/4 out channels.
// `multiconv <ker_wid 3|5|7> <i_batch 0..3> <num_tests <= 10> <n_in 1..16>` (not a reference command): `conv`'s layer with n_in * B input channels held in n_in input
// ciphertexts and B output channels, as ONE convolution (the products summed at level 1, one pack tree), Ours only, on
// test_conv_data/test_multiconv{k}_batch_{B}_in{n_in}_{in,ker,bna,bnb,out}_{t}.csv (tests/golden/gen_multiconv_csv.py). HCONV_IMAGE_BATCH = g: g images, g * n_in <= 16.
// `transconvReLU <ker_wid 3|5|7> <i_batch 0..3> <num_tests <= 10> [sparse]` and `multiconvReLU <ker_wid 3|5|7> <i_batch 0..3> <num_tests <= 10> <n_in 1..16>` (not reference
// commands; Ours only): `transconv` / `multiconv` as LAYERS - the convolution at out_scale 2^(round(log2 Q0) - 12), then convReLU's bootstrapping chain (CtoS, ReLU, keep mask, StoC),
// checked against ..._reluout_{t}.csv = max(out, 0) (tests/golden/gen_transconv_relu_csv.py, gen_multiconv_relu_csv.py). They print convReLU's Ours-column lines. `sparse`: the
// transposed layer's B/4 output channels at slots 4*o and the log_sparse = 2 bootstrapper on one packed ciphertext (kind "TransConv_sparse") instead of the full-slot one on two.
// Argument checks are those of `transconv` / `multiconv`; HCONV_IMAGE_BATCH, HCONV_DEVICE_ENCRYPT, HCONV_DEBUG_LAYERS and HCONV_BOOT_STATS apply as for convReLU.
// `resnet_fast <ker_wid> <depth> 1 <test_num> false` (not a reference command: the reference reaches testResNet_crop_fast_in, test.go:372-636, only by swapping
// main.go:620-622): the same network as `resnet` on full slots, one bootstrapper (hconv_resnet.cpp). Same arguments; wide_case != 1 and cf100 are refused like `resnet`'s.
// `resnet_packed <ker_wid 3|7> <depth> 1 <test_num> false` (not a reference command): resnet_fast's network, weight, image and result files with 4 / 8 / 16 images per ciphertext
// of block 1 / 2 / 3 (hconv_host.hpp packed_slot; DESIGN.md "The packed layout"), in groups of up to 16 images. Refused: wide_case != 1, cf100, ker_wid 5, the replay switches and
// HCONV_DEBUG_LAYERS. HCONV_PACKED_DUMP_LAYERS=<layers> (test mode) writes every image's activation after the listed layers to packed_act_L<layer>_<image>.csv.
// `strconvReLU <ker_wid 3|5|7> <i_batch 0..3> <num_tests <= 10> [pos 0..3]` (not a reference command; Ours only): the full-packing stride layer alone - the convolution at the chain's
// out_scale, then the bootstrapping chain of kind "StrConv" (eval.go:303, 507-520: ext_ctxt with gen_comprs_full after the ReLU) at pack position pos - on
// test_conv_data/test_strconv{k}_batch_{B}_{in,ker,bna,bnb,reluout}_{t}.csv (tests/golden/gen_strconv_relu_csv.py): raw width kp_wid = 2 (widths[i]/2 - k/2), reluout = the ReLU of the
// stride-2 outputs, (kp_wid/2, kp_wid/2, B). Widths divisible by 4. It prints convReLU's Ours-column lines and the largest coefficient outside the kept cells.
// `imagenet <ker_wid 3|5> <test_num> [c1 1..256]` (test.go:1209-1400 testImagenet_final_fast_in, which the reference reaches by editing main.go:570-575): the ImageNet tail on
// weight_imgnet_ker{k}_h5/, ker{k}_data/test_image_{i}.csv -> ker{k}_enc_result/enc_result_{i}.csv. c1 (default 256; not a reference argument): the real channel count of block 1
// (block 2 has 2 c1) of the files (tests/golden/gen_imagenet_csv.py). HCONV_IMAGE_BATCH, HCONV_SEED (test mode), HCONV_PROFILE and HCONV_DEBUG_LAYERS as for resnet_fast; the replay switches are refused.
// HCONV_SKIP_BL=1 skips the baseline half (not a reference feature; for timing "Ours" alone).
// `conv --test-mode <args>` honours the test-only overrides HCONV_SEED / HCONV_CHAIN_REPLAY; without the flag they are fatal when set.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>
#include <string>

#include "hconv_host.hpp"

// `<name> <ker_wid> <depth> <wide_case> <test_num> <cf100>` of the three resnet commands (main.go:609-621's argument handling), refused before any device work
struct ResnetArgs { int depth, test_num; };
static ResnetArgs resnet_args(const std::string &name, int argc, char **argv) {
    if (argc < 7) hconv::panic("runtime error: index out of range (usage: " + name + " <ker_wid> <depth> <wide_case> <test_num> <cf100>)");
    const int depth = atoi(argv[3]), wide_case = atoi(argv[4]), test_num = atoi(argv[5]);
    const bool cf100 = std::string(argv[6]) == "true" || std::string(argv[6]) == "1";
    if (wide_case < 1 || wide_case > 3) hconv::panic("Wrong wide case!");                                  // main.go:628
    // BASELINE config 5 is `resnet 3 20 1 n false`; the wide networks and the CIFAR-100 head are outside the scope table and not built
    if (wide_case != 1 || cf100) hconv::panic(name + ": wide_case 2 / 3 and cf100 = true are out of scope in this build (SURVEY.md section 2, row 14)");
    return {depth, test_num};
}
static void check_depth(int depth) { if (!(depth == 8 || depth == 14 || depth == 20)) hconv::panic("wrong depth (not in 8, 14, 20)!"); }   // test.go:397-405
// a command that cannot honour these switches refuses them when they are set (to anything but 0)
static void refuse_env(const std::string &name, std::initializer_list<const char *> vars, const char *why) {
    for (const char *v : vars) if (getenv(v) && *getenv(v) && std::string(getenv(v)) != "0") hconv::panic(name + ": " + v + " " + why);
}
static const std::initializer_list<const char *> REPLAYS = {"HCONV_RESNET_REPLAY", "HCONV_CHAIN_REPLAY", "HCONV_CHAIN_REPLAY_BL"};
static const char *const PINNED = "replays a pinned run of another command and is not available here";
// main.go:583-585's bounds of the layer commands, and the index Go would panic on
static void check_layer_args(int num_tests, int i_batch) {
    if (num_tests > 10 || i_batch > 3) hconv::panic("Too many tests (>10) or too many batch index (>3)");
    if (i_batch < 0) hconv::panic("runtime error: index out of range");
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "--test-mode") {      // not a reference feature: enables HCONV_SEED / HCONV_CHAIN_REPLAY (hconv_host.hpp)
        hconv::testMode() = true; argv[1] = argv[0]; argv++; argc--;
        fprintf(stderr, "hconv: --test-mode: test-only overrides from the environment are honoured\n");
    }
    const int batchs[5] = {4, 16, 64, 256, 1024}, widths[5] = {128, 64, 32, 16, 8};   // main.go:578-579
    if (argc > 1 && std::string(argv[1]) == "imagenet") {                  // imagenet <ker_wid> <test_num> [c1]: test.go:1209's (st = 0, end, ker) with the arguments in this CLI's order
        if (argc < 4 || argc > 5) hconv::panic("runtime error: index out of range (usage: imagenet <ker_wid 3|5> <test_num> [c1 1..256])");
        const int ker = atoi(argv[2]), test_num = atoi(argv[3]), c1 = argc > 4 ? atoi(argv[4]) : 256;
        if (!(ker == 3 || ker == 5)) hconv::panic("strange ker name!");                                    // test.go:1236
        if (test_num < 1) hconv::panic("imagenet: test_num must be at least 1");
        if (c1 < 1 || c1 > 256) hconv::panic("imagenet: c1 not in 1..256");
        refuse_env("imagenet", REPLAYS, PINNED);
        setenv("HCONV_ASYNC_ALLOC", "1", 0);                                                               // a chain command (see below)
        hconv::testImagenet_final_fast_in(0, test_num, ker, c1);
        return 0;
    }
    if (argc < 5) hconv::panic("runtime error: index out of range (usage: conv|convReLU|transconv <ker_wid> <i_batch> <num_tests>)");
    const std::string test_name = argv[1];
    // The bootstrapping chains allocate and free a few buffers per evaluator operation, and hipFree drains the device every time: the chain commands run on cached
    // allocations (hconv.hip hcx_malloc) unless HCONV_ASYNC_ALLOC=0 says otherwise - ResNet-20 at 8 images per launch set 2.12 -> 2.02 s per set (profiles/round4_cached_alloc_ab.txt)
    if (test_name == "convReLU" || test_name == "resnet" || test_name == "resnet_fast" || test_name == "resnet_packed" || test_name == "transconvReLU" || test_name == "multiconvReLU" || test_name == "strconvReLU") setenv("HCONV_ASYNC_ALLOC", "1", 0);
    const int ker_wid = atoi(argv[2]), i_batch = atoi(argv[3]), num_tests = atoi(argv[4]);
    if (!(ker_wid == 3 || ker_wid == 5 || ker_wid == 7)) hconv::panic("Wrong kernel wid (not in 3,5,7)");
    if (test_name == "resnet" || test_name == "resnet_fast") {             // main.go:609-621: resnet ker depth wide_case test_num cf100; resnet_fast: not a reference command (see the top of this file)
        const ResnetArgs a = resnet_args(test_name, argc, argv);
        check_depth(a.depth);
        if (test_name == "resnet") hconv::testResNet_crop_sparse(0, a.test_num, ker_wid, a.depth, false);
        else hconv::testResNet_crop_fast_in(0, a.test_num, ker_wid, a.depth, false);
        return 0;
    }
    if (test_name == "resnet_packed") {                                  // not a reference command (see the top of this file); resnet_fast's arguments
        const ResnetArgs a = resnet_args(test_name, argc, argv);
        if (ker_wid == 5) hconv::panic("resnet_packed: kernel width 5 is not packed: its even keep widths 30, 14, 6 put the first kept position at step - 1, not 0 "
                                       "(and that network differs from the plain model anyway); use 3 or 7");
        check_depth(a.depth);
        // the replays' and the per-stage report's shadows know one image per ciphertext
        refuse_env(test_name, {"HCONV_RESNET_REPLAY", "HCONV_CHAIN_REPLAY", "HCONV_CHAIN_REPLAY_BL", "HCONV_DEBUG_LAYERS"}, "follows one image per ciphertext and is not available here");
        hconv::testOnlyEnv("HCONV_PACKED_DUMP_LAYERS");                    // fatal without --test-mode, before any device work
        hconv::testResNet_crop_packed(0, a.test_num, ker_wid, a.depth);
        return 0;
    }
    if (test_name != "conv" && test_name != "convReLU" && test_name != "transconv" && test_name != "transconvReLU" && test_name != "strconvReLU" && test_name != "multiconv" && test_name != "multiconvReLU")
        hconv::panic("wrong test type");
    const bool relu = test_name == "convReLU" || test_name == "transconvReLU" || test_name == "multiconvReLU";
    auto banner = [&](const char *line) { printf("%s\n", line); printf("Ker:  %d batches:  %d widths:  %d\n", ker_wid, batchs[i_batch], widths[i_batch]); };
    if (test_name == "transconv" || test_name == "transconvReLU") {        // not reference commands (see the top of this file)
        check_layer_args(num_tests, i_batch);
        bool sparse = false;
        if (relu && argc > 5) { if (std::string(argv[5]) != "sparse") hconv::panic("transconvReLU: the optional fourth argument is `sparse`"); sparse = true; }
        banner(relu ? "Transposed convolution followed by ReLU (& Bootstrapping) test start!" : "Transposed convolution test start! (No Bootstrapping)");
        printf("Ours start.\n");
        hconv::testTransConv_in(batchs[i_batch], widths[i_batch], ker_wid, num_tests, relu, sparse);
    } else if (test_name == "strconvReLU") {                                // not a reference command (see the top of this file)
        if (argc > 6) hconv::panic("strconvReLU: at most one optional argument, the pack position");
        check_layer_args(num_tests, i_batch);
        const int pos = argc > 5 ? atoi(argv[5]) : 0;
        if (pos < 0 || pos > 3 || (argc > 5 && (argv[5][0] < '0' || argv[5][0] > '3' || argv[5][1]))) hconv::panic("strconvReLU: the pack position is 0..3");
        if (widths[i_batch] % 4 != 0) hconv::panic("input wid not divisible by 4");
        refuse_env(test_name, REPLAYS, PINNED);
        banner("Stride-2 convolution followed by ReLU (& Bootstrapping) on full packing test start!");
        printf("Ours start.\n");
        hconv::testStrConv_in(batchs[i_batch], widths[i_batch], ker_wid, num_tests, pos);
    } else if (test_name == "multiconv" || test_name == "multiconvReLU") {   // not reference commands (see the top of this file)
        if (argc < 6) hconv::panic(std::string("runtime error: index out of range (usage: ") + test_name + " <ker_wid> <i_batch> <num_tests> <n_in>)");
        check_layer_args(num_tests, i_batch);
        const int n_in = atoi(argv[5]);
        if (n_in < 1 || n_in > 16) hconv::panic("Wrong number of input ciphertexts (not in 1..16)");
        banner(relu ? "Multi-input convolution followed by ReLU (& Bootstrapping) test start!" : "Multi-input convolution test start! (No Bootstrapping)");
        printf("Ours start.\n");
        hconv::testMultiConv_in(batchs[i_batch], widths[i_batch], ker_wid, num_tests, n_in, relu);
    } else {                                                                // conv, convReLU: the baseline, then Ours (main.go:639-643)
        check_layer_args(num_tests, i_batch);
        banner(relu ? "Convolution followed by ReLU (& Bootstrapping) test start!" : "Convolution test start! (No Bootstrapping)");
        printf("Base Line start.\n");
        if (getenv("HCONV_SKIP_BL") && atoi(getenv("HCONV_SKIP_BL"))) printf("(HCONV_SKIP_BL set: baseline skipped)\n");
        else hconv::testConv_BL_in(batchs[i_batch], widths[i_batch], ker_wid, num_tests, relu);
        printf("Ours start.\n");
        hconv::testConv_in(batchs[i_batch], widths[i_batch], ker_wid, num_tests, relu);
    }
    return 0;
}
