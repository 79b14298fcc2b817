"""`resnet_packed` without a GPU: (1) the packed layout on the grid model - block-diagonal dilated kernels, all-phase masks, the stride layers' split / mask / merge, the
dilated FC - computes the plain strided network for every image of a group, exactly on integer data; (2) the host's packed masks, slot assignment and expanded kernels
(header-only in hconv_host.hpp, through a small stand-alone tool) equal the model's; (3) the command's refusals.

Exactness of (1): weights in {-1, 0, 1}, bn_a in {1, 2}, small integer biases and images. Every value is an integer, and the test checks that the largest activation
stays below 2^50, so every sum of the model and of the plain network is exact in float64 in whatever order it is taken."""
import os
import subprocess

import numpy as np
import pytest

import golden.gen_resnet_packed_images as pgen
import oracle_resnet as rn
import resnet_fast_ref as F
import resnet_packed_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def net_layers(depth=8):
    """(strided, block of the output, cin, cout) in driver order"""
    blocks = {8: (3, 1, 1), 20: (7, 5, 5)}[depth]
    out, cin = [], 3
    for blk, c in enumerate((16, 32, 64)):
        if blk:
            out.append((True, blk, cin, c))
            cin = c
        for _ in range(blocks[blk]):
            out.append((False, blk, cin, c))
            cin = c
    return out


def integer_net(k, seed):
    rng = np.random.default_rng(seed)
    layers = [(strided, blk, rng.integers(-1, 2, size=(k, k, cin, cout)).astype(np.float64), rng.integers(1, 3, size=cout).astype(np.float64),
               rng.integers(-2, 3, size=cout).astype(np.float64)) for strided, blk, cin, cout in net_layers()]
    return layers, rng.integers(-2, 3, size=(64, 10)).astype(np.float64), rng.integers(-2, 3, size=10).astype(np.float64)


def plain_network(layers, image, k):
    """conv 'same', * a + b, ReLU; a stride layer keeps the even positions (odd keep widths: k = 3, 7)"""
    x, acts = image, []
    for strided, blk, w, a, b in layers:
        y = rn.plain_conv_same(x, w) * a + b
        if strided:
            r = F.RAW(k)[blk]
            y = y[0:2 * r:2, 0:2 * r:2]
        x = np.maximum(y, 0)
        acts.append(x)
    return acts


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("n_images", [16, 5])
def test_packed_grid_model_is_the_plain_network(k, n_images):
    """after every one of the 7 layers every ciphertext equals the plain activations of its images placed in their slots - every cell and slot, the empty ones of a partial
    group excepted (they carry ReLU(bias), and nothing reads them) - and the FC readings are mean(activation) @ fc_w + fc_b"""
    layers, fc_w, fc_b = integer_net(k, 10 + k)
    rng = np.random.default_rng(k)
    r0 = F.RAW(k)[0]
    images = [rng.integers(-3, 4, size=(r0, r0, 3)).astype(np.float64) for _ in range(n_images)]
    plain = [plain_network(layers, im, k) for im in images]
    assert max(np.abs(a).max() for acts in plain for a in acts) < 2.0 ** 50
    handed, scores, tails = P.network(layers, fc_w, fc_b, images)
    assert tails == {16: 27, 5: 3 * 2 + 4 + 1 + 2 + 1}[n_images]
    for li, (cts, blk) in enumerate(handed):
        want = P.place([acts[li] for acts in plain], blk)
        assert len(cts) == len(want) == P.n_cts(blk, n_images)
        if n_images == 16:
            for q, (g, w_) in enumerate(zip(cts, want)):
                assert np.array_equal(g, w_), f"k={k} layer {li} ciphertext {q}"
        for m in range(n_images):
            r, C = plain[m][li].shape[0], plain[m][li].shape[2]
            assert np.array_equal(P.unplace(cts[P.slot_of(blk, m)[0]], blk, m, r, C), plain[m][li]), f"k={k} layer {li} image {m}"
    for m in range(n_images):
        np.testing.assert_allclose(scores[m], plain[m][-1].mean(axis=(0, 1)) @ fc_w + fc_b, rtol=1e-12, atol=0)
    a = np.stack([acts[-1] for acts in plain])
    assert all(np.abs(a[i] - a[j]).max() > 0 for i in range(n_images) for j in range(i)), "the images differ, so a swap of two slots would show"


def test_slot_assignment_fills_every_slot_once_and_follows_the_stride_rule():
    """slot_of is a bijection onto each block's image slots, and block b + 1's slot is block b's under the stride layer's rule: result r = 2q + g // norm_out,
    channel offset g % norm_out, output ciphertext r // 4, moved by s_in * (t // 2, t % 2), t = r % 4"""
    for blk in range(3):
        slots = {P.slot_of(blk, m) for m in range(16)}
        assert slots == {(q, g, py, px) for q in range(16 // P.CAP[blk]) for g in range(P.NORM[blk]) for py in range(P.STEPS[blk]) for px in range(P.STEPS[blk])}
    for blk in (1, 2):
        for m in range(16):
            q, g, py, px = P.slot_of(blk - 1, m)
            r = 2 * q + g // P.NORM[blk]
            t, s_in = r % 4, P.STEPS[blk - 1]
            assert P.slot_of(blk, m) == (r // 4, g % P.NORM[blk], py + s_in * (t // 2), px + s_in * (t % 2))


def test_plain_activations_tell_the_images_apart():
    """the GPU test's condition d_own < d_other / 4 needs d_other, the smallest mean |difference| between two images' plain activations, well above the chain's error at
    the dumped layers 3, 5 and 6. That error is the polynomial ReLU's on the range 64: up to about 0.05 near zero, in absolute terms. gen_resnet_csv's own images give
    d_other 0.046 / 0.015 / 0.0072 there, so the GPU test draws gen_resnet_packed_images's: every pre-activation inside the range, and d_other above 0.1, twice that error"""
    net = rn.Net(16, ker_wid=3, depth=8, seed=0)
    res = [pgen.plain(net, im) for im in pgen.images(16, net.raw[0])]
    assert max(r[2] for r in res) < pgen.RANGE
    for li in (3, 5, 6):
        d, mean = pgen.d_other([r[0] for r in res], li)
        print(f"layer {li}: smallest mean |difference| between two images {min(d):.4f}, mean activation {mean:.4f}")
        assert min(d) > 0.1, (li, min(d))
    small = [pgen.plain(net, im)[0] for im in pgen.images(16, net.raw[0], 1.0)]
    assert max(min(pgen.d_other(small, li)[0]) for li in (3, 5, 6)) < 0.05  # why not amplitude 1


TOOL_SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hconv_host.hpp"
namespace hconv { [[noreturn]] void panic(const std::string &m) { fprintf(stderr, "panic: %s\n", m.c_str()); exit(2); } }
using namespace hconv;
// mask <vec_size> <in_wid> <kp_wid> <step> <n_phase> <ul> | slot <blk> | ker <k> <cin> <cout> <norm_in> <norm_out> <g_lo> <g_cnt> | bn <n> <norm_out>
int main(int c, char **v) {
    if (c < 2) return 1;
    if (!strcmp(v[1], "mask")) { auto m = gen_keep_vec_packed(atoi(v[2]), atoi(v[3]), atoi(v[4]), atoi(v[5]), atoi(v[6]), atoi(v[7])); for (size_t i = 0; i < m.size(); i++) if (m[i]) printf("%zu\n", i); }
    else if (!strcmp(v[1], "slot")) { for (int m = 0; m < PACKED_GROUP; m++) { PackedSlot p = packed_slot(atoi(v[2]), m); printf("%d %d %d %d\n", p.ct, p.g, p.py, p.px); } }
    else if (!strcmp(v[1], "keys")) printf("%d %d %d %d %d\n", packedMaskKey(1), packedMaskKey(2), packedMaskKey(4), packedStrideMaskKey(2), packedStrideMaskKey(4));
    else if (!strcmp(v[1], "ker")) {      // weights 1, 2, 3, ... in HWIO order
        const int k = atoi(v[2]), cin = atoi(v[3]), cout = atoi(v[4]);
        std::vector<double> w((size_t)k * k * cin * cout); for (size_t i = 0; i < w.size(); i++) w[i] = (double)(i + 1);
        auto e = packed_expand_ker(w, k * k, cin, cout, atoi(v[5]), atoi(v[6]), atoi(v[7]), atoi(v[8]));
        printf("%zu\n", e.size()); for (size_t i = 0; i < e.size(); i++) if (e[i] != 0) printf("%zu %.0f\n", i, e[i]);
    } else if (!strcmp(v[1], "bn")) {
        std::vector<double> a((size_t)atoi(v[2])); for (size_t i = 0; i < a.size(); i++) a[i] = (double)(i + 1);
        for (double x : packed_expand_bn(a, atoi(v[3]))) printf("%.0f\n", x);
    } else return 1;
    return 0;
}
'''


@pytest.fixture(scope="module")
def packed_tool(tmp_path_factory):
    """the host's packed-layout helpers (header-only in hconv_host.hpp) compiled into a tiny printer"""
    d = tmp_path_factory.mktemp("packedtool")
    src = d / "packed.cpp"
    src.write_text(TOOL_SRC)
    exe = d / "packed"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "optimal_conv_amd", "host"), "-o", str(exe), str(src)])

    def run(*args, check=True):
        return subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=check)
    return run


@pytest.mark.parametrize("k", [3, 7])
def test_host_packed_masks_equal_the_model(packed_tool, k):
    """gen_keep_vec_packed at the arguments a Resnet_crop_packed context uses == the model's cell masks in the keep vector's slot order; the block-1 mask is resnet_fast's"""
    for blk, r in enumerate(F.RAW(k)):
        s = 1 << blk
        for stride_in in ((False, True) if blk else (False,)):
            for ul in (0, 1):
                got = np.array([int(t) for t in packed_tool("mask", 1 << 15, 32, r, s, s // 2 if stride_in else s, ul).stdout.split()], dtype=np.int64)
                want = np.nonzero(P.keep_vec(P.keep_cells(k, blk, stride_in), ul))[0]
                assert got.size and np.array_equal(got, want), (k, blk, stride_in, ul)
                if blk == 0:
                    assert np.array_equal(want, np.nonzero(F.gen_keep_vec_stride(1 << 15, 32, r, 1, ul, True))[0])
    assert P.keep_cells(k, 1).sum() == 4 * F.RAW(k)[1] ** 2 and P.keep_cells(k, 2, True).sum() == 4 * F.RAW(k)[2] ** 2
    assert packed_tool("keys").stdout.split() == ["101", "102", "104", "202", "204"]          # none of resnet_fast's ext_idx keys 1, 2, 4
    bad = packed_tool("mask", 1 << 15, 32, 31, 1, 1, 2, check=False)
    assert bad.returncode == 2 and "ul not 0 nor 1" in bad.stderr
    assert packed_tool("mask", 1 << 15, 32, 17, 2, 2, 0, check=False).returncode == 2         # cells past the grid


def test_host_slot_assignment_equals_the_model(packed_tool):
    for blk in range(3):
        got = [tuple(int(t) for t in line.split()) for line in packed_tool("slot", blk).stdout.splitlines()]
        assert got == [P.slot_of(blk, m) for m in range(16)], blk
    assert packed_tool("slot", 3, check=False).returncode == 2


@pytest.mark.parametrize("shape", [(3, 3, 16, 4, 4, 0, 4), (3, 32, 32, 2, 2, 0, 2), (7, 64, 64, 1, 1, 0, 1),                      # inside layers of blocks 1, 2, 3 (the first reads 3 channels)
                                   (3, 16, 32, 4, 2, 0, 2), (3, 16, 32, 4, 2, 2, 2), (3, 32, 64, 2, 1, 0, 1), (3, 32, 64, 2, 1, 1, 1)])      # both halves of both stride layers
def test_host_expanded_kernels_equal_the_model(packed_tool, shape):
    k, cin, cout, norm_in, norm_out, g_lo, g_cnt = shape
    lines = packed_tool("ker", *shape).stdout.split("\n")
    got = np.zeros(int(lines[0]))
    for ln in lines[1:]:
        if ln:
            i, v = ln.split()
            got[int(i)] = float(v)
    w = (np.arange(k * k * cin * cout, dtype=np.float64) + 1).reshape(k, k, cin, cout)
    want = P.expand_ker(w, norm_in, norm_out, g_lo, g_cnt)
    assert got.size == want.size and np.array_equal(got.reshape(want.shape), want)
    assert np.count_nonzero(want) == w.size * g_cnt
    got_bn = np.array([float(t) for t in packed_tool("bn", cout, norm_out).stdout.split()])
    assert np.array_equal(got_bn, np.repeat(np.arange(cout) + 1.0, norm_out))


def test_host_expanded_kernel_refusals(packed_tool):
    assert packed_tool("ker", 3, 16, 32, 4, 2, 3, 2, check=False).returncode == 2             # channel offsets past norm_in
    assert packed_tool("ker", 3, 32, 32, 4, 2, 0, 2, check=False).returncode == 2             # norm_in * cin > 64


@pytest.mark.parametrize("argv,env,msg", [(["resnet_packed", "5", "8", "1", "1", "false"], {}, "kernel width 5 is not packed"),
                                          (["resnet_packed", "3", "8", "2", "1", "false"], {}, "out of scope"),
                                          (["resnet_packed", "3", "8", "1", "1", "true"], {}, "out of scope"),
                                          (["resnet_packed", "3", "9", "1", "1", "false"], {}, "panic: wrong depth (not in 8, 14, 20)!"),
                                          (["resnet_packed", "3", "8", "1", "1"], {}, "runtime error: index out of range"),
                                          (["resnet_packed", "3", "8", "1", "1", "false"], {"HCONV_PACKED_DUMP_LAYERS": "3"}, "HCONV_PACKED_DUMP_LAYERS"),
                                          (["resnet_packed", "3", "8", "1", "1", "false"], {"HCONV_DEBUG_LAYERS": "1"}, "HCONV_DEBUG_LAYERS follows one image per ciphertext"),
                                          (["--test-mode", "resnet_packed", "3", "8", "1", "1", "false"], {"HCONV_RESNET_REPLAY": "7"}, "HCONV_RESNET_REPLAY follows one image per ciphertext")])
def test_resnet_packed_cli_refusals(tmp_path, argv, env, msg):
    """bad arguments and switches end the command like a Go panic (status 2) before it touches a device"""
    cli = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")
    if not os.path.exists(cli):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([cli] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60, env=dict(os.environ, **env))
    assert r.returncode == 2 and msg in r.stderr, (argv, r.returncode, r.stderr[-300:])
    assert "CKKS parameters" not in r.stdout
