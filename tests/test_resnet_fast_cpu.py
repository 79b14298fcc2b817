"""`resnet_fast` (the reference's testResNet_crop_fast_in, test.go:372-636) without a GPU: (a) the "inside" formulation - dilated kernels on the
32-wide grid, the kd offsets, the stride masks of gen_keep_vec_stride, the stride layers' input channels at 2c - computes a plain strided
network layer by layer, exactly on integer data (torch conv2d); (b) the host's gen_keep_vec_stride equals rot_util.go:226-267 restated;
(c) hc_prep_ker_ex2 on the emulated kernel library equals hc_prep_ker_ex on the host-expanded kernel bit for bit; (d) the command's refusals.

Phase: a stride layer keeps positions init + i*step (init = 0 for an odd keep width, step - 1 for an even one). For k = 3 and 7 every keep
width is odd and the fast network is the plain model tests/oracle_resnet.py holds the sparse driver to (even positions). For k = 5 (widths
30, 14, 6) it keeps the ODD positions of each stride layer's output, a different network: the tests compare it to its own plain model."""
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import oracle_resnet as rn
import resnet_fast_ref as F
import transconv_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")


def plain_layer(x, w, a, b, strided, r_next):
    """conv 'same' (torch) * a + b, ReLU; a stride layer keeps phase 0 (odd next width) or 1 (even) at stride 2"""
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]
    wt = torch.from_numpy(np.ascontiguousarray(w.transpose(3, 2, 0, 1)))
    y = Fn.conv2d(xt, wt, padding=w.shape[0] // 2)[0].permute(1, 2, 0).numpy() * a + b
    if strided:
        ph = 0 if r_next % 2 else 1
        y = y[ph:ph + 2 * r_next:2, ph:ph + 2 * r_next:2]
    return np.maximum(y, 0)


def net_layers(k, depth=8):
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


def test_grid_model_is_the_reference_ring_product():
    """the grid model (a tap moves the input by whole cells, negacyclic sign past the end) == the reference's own formulas (prep_Input, prep_Ker,
    encode_ker_final, the negacyclic product, the packing tree: transconv_ref.conv_plain) on a small ring, dilated kernel, data up to every edge"""
    W, B, N = 16, 4, 1024
    rng = np.random.default_rng(3)
    for k, dil in ((3, 1), (3, 2), (3, 4), (5, 2)):
        ker = rng.integers(-3, 4, size=(k, k, B, B)).astype(np.float64)
        kexp = F.expand_ker(ker, dil)
        x = rng.integers(-3, 4, size=(W, W, B)).astype(np.float64)
        want = R.conv_plain(x, kexp.reshape(-1), np.ones(B), W, kexp.shape[0], B, B, N, trans=False)
        np.testing.assert_array_equal(F.grid_conv(x, kexp, 1), want)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_inside_layers_are_the_plain_strided_network(k):
    """every layer of the fast network, given the plain network's activation in its layout, returns the plain layer's output in its layout -
    every cell and slot, masked ones included - exactly, on integer data"""
    rng = np.random.default_rng(k)
    raw = F.RAW(k)
    for strided, blk, cin, cout in net_layers(k):
        bin_ = blk - 1 if strided else blk
        x = rng.integers(-3, 4, size=(raw[bin_], raw[bin_], cin)).astype(np.float64)
        if cin != 3:
            x = np.maximum(x, 0)                                            # a ReLU output
        w = rng.integers(-2, 3, size=(k, k, cin, cout)).astype(np.float64)
        a = rng.integers(1, 3, size=cout).astype(np.float64)
        b = rng.integers(-2, 3, size=cout).astype(np.float64)
        got = F.inside_layer(F.place(x, k, bin_), k, strided, blk, w, a, b)
        want = plain_layer(x, w, a, b, strided, raw[blk])
        assert want.shape == (raw[blk], raw[blk], cout)
        np.testing.assert_array_equal(got, F.place(want, k, blk), err_msg=f"k={k} layer strided={strided} block={blk}")
    fc_w = rng.integers(-2, 3, size=(64, 10)).astype(np.float64)
    fc_b = rng.integers(-2, 3, size=10).astype(np.float64)
    x = np.maximum(rng.integers(-3, 4, size=(raw[2], raw[2], 64)), 0).astype(np.float64)
    np.testing.assert_allclose(F.inside_fc(F.place(x, k, 2), k, fc_w, fc_b), x.mean(axis=(0, 1)) @ fc_w + fc_b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_inside_network_against_the_sparse_drivers_plain_model(k):
    """the whole depth-8 network on gen_resnet_csv's weights and image: for k = 3, 7 the fast network IS oracle_resnet.Net's plain model (the
    scores resnet_fast is checked against on the GPU); for k = 5 it is not (odd phase), and equals the odd-phase plain network instead"""
    net = rn.Net(16, ker_wid=k, depth=8, seed=0)
    layers = [(kind.startswith("Str"), blk + 1 if kind.startswith("Str") else blk, w, a, b) for kind, blk, w, a, b in net.layers]
    _, got = F.inside_network(layers, net.fc_w, net.fc_b, net.image)
    _, want = net.plain()
    x = net.image
    for strided, blk, w, a, b in layers:
        x = plain_layer(x, w, a, b, strided, F.RAW(k)[blk])
    own = x.mean(axis=(0, 1)) @ net.fc_w + net.fc_b
    np.testing.assert_allclose(got, own, rtol=0, atol=1e-12)
    if k == 5:
        assert np.max(np.abs(got - want)) > 1e-4
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.fixture(scope="module")
def mask_tool(tmp_path_factory):
    """the host's gen_keep_vec_stride (header-only in hconv_host.hpp) compiled into a tiny printer"""
    d = tmp_path_factory.mktemp("keepmask")
    src = d / "keep.cpp"
    src.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "hconv_host.hpp"\n'
                   'namespace hconv { [[noreturn]] void panic(const std::string &m) { fprintf(stderr, "panic: %s\\n", m.c_str()); exit(2); } }\n'
                   'int main(int c, char **v) { (void)c; auto m = hconv::gen_keep_vec_stride(atoi(v[1]), atoi(v[2]), atoi(v[3]), atoi(v[4]), atoi(v[5]), atoi(v[6]) != 0);\n'
                   '  for (size_t i = 0; i < m.size(); i++) if (m[i]) printf("%zu\\n", i); return 0; }\n')
    exe = d / "keep"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "optimal_conv_amd", "host"), "-o", str(exe), str(src)])
    return str(exe)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_host_keep_masks_equal_the_restatement(mask_tool, k):
    """ext_idx[step][ul] of a Resnet_crop_fast context (main.go:123-136: gen_keep_vec_stride(N/2, 32, raw_in_wids[i], 2^i, ul, raw odd)) for every
    (step, ul, parity) the driver uses == the numpy restatement of rot_util.go:226-267"""
    for i, r in enumerate(F.RAW(k)):
        for ul in (0, 1):
            out = subprocess.run([mask_tool, str(1 << 15), "32", str(r), str(1 << i), str(ul), str(r % 2)], capture_output=True, text=True, check=True).stdout
            got = np.array([int(t) for t in out.split()], dtype=np.int64)
            want = np.nonzero(F.gen_keep_vec_stride(1 << 15, 32, r, 1 << i, ul, r % 2 == 1))[0]
            assert got.size and np.array_equal(got, want), (k, i, ul)
    r = subprocess.run([mask_tool, str(1 << 15), "32", "31", "1", "2", "1"], capture_output=True, text=True)
    assert r.returncode == 2 and "ul not 0 nor 1" in r.stderr


@pytest.fixture(scope="module")
def emu():
    from optimal_conv_amd import Context
    from oracle_lib import Oracle, P0, Q0, Q1
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx = Context([Q0, Q1], [P0], lib_path=EMU_LIB)
    yield ctx, Oracle()
    ctx.close()


@pytest.mark.parametrize("shape", F.DRIVER_SHAPES)
def test_prep_ker_ex2_emulated(emu, shape):
    F.case_prep_ker_ex2(emu[0], *shape)


def test_prep_ker_fc_k31_emulated(emu):
    F.case_fc_k31(*emu)


def test_prep_ker_ex2_identity_is_prep_ker_ex(emu):
    """dilation = ib_stride = 1 is hc_prep_ker_ex, trans = 0 and trans = 1"""
    import ctypes as C
    ctx = emu[0]
    rng = np.random.default_rng(9)
    ker = rng.uniform(-1, 1, (3, 3, 16, 16)).reshape(-1)
    bna = rng.uniform(0.5, 1.5, 16)
    f64p = C.POINTER(C.c_double)
    for trans in (0, 1):
        hs = []
        for fn, extra in ((ctx.L.hc_prep_ker_ex, ()), (ctx.L.hc_prep_ker_ex2, (1, 1))):
            h = C.c_void_p()
            assert fn(ctx.h, ker.ctypes.data_as(f64p), ker.size, bna.ctypes.data_as(f64p), 32, 3, 16, 16, 4, 2.0 ** 30, trans, *extra, C.byref(h)) == 0
            hs.append(h)
        assert np.array_equal(ctx.ker_download(hs[0], 64), ctx.ker_download(hs[1], 64)), trans
        for h in hs:
            ctx.ker_free(h)


def test_prep_ker_ex2_refusals(emu):
    """HC_ERR_ARG: trans with dilation / ib_stride != 1, values < 1, norm*real_ib*ib_stride > max_bat, a dilated width past 2*adj <= N"""
    import ctypes as C
    ctx = emu[0]
    f64p = C.POINTER(C.c_double)

    def call(k, real_ib, real_ob, norm, trans, dil, ibs, in_wid=32):
        ker = np.zeros(k * k * real_ib * real_ob) + 0.5
        bna = np.ones(real_ob)
        h = C.c_void_p()
        rc = ctx.L.hc_prep_ker_ex2(ctx.h, ker.ctypes.data_as(f64p), ker.size, bna.ctypes.data_as(f64p), in_wid, k, real_ib, real_ob, norm, 2.0 ** 30, trans, dil, ibs, C.byref(h))
        if rc == 0:
            ctx.ker_free(h)
        return rc
    assert call(3, 16, 16, 1, 0, 2, 2) == 0
    for args in ((3, 16, 16, 1, 1, 2, 1), (3, 16, 16, 1, 1, 1, 2), (3, 16, 16, 1, 0, 0, 1), (3, 16, 16, 1, 0, 1, 0), (3, 16, 16, 1, 0, -1, 1),
                 (3, 16, 16, 4, 0, 1, 2), (3, 32, 32, 2, 0, 1, 2), (3, 16, 16, 1, 0, 16, 1), (2, 16, 16, 1, 0, 31, 1)):
        assert call(*args) != 0, args
    assert call(3, 32, 64, 1, 0, 1, 2) == 0                                 # norm*real_ib*ib_stride == max_bat passes
    assert call(7, 16, 16, 1, 0, 4, 1) == 0                                 # 25 wide (k = 7 in block 3)
    from optimal_conv_amd import HconvError
    with pytest.raises(HconvError, match="input size inconsistent"):
        ctx.prep_ker(np.zeros(3 * 3 * 16 * 16), np.ones(16), 32, 5, 16, 16, dilation=2)


def test_version_and_symbol():
    from optimal_conv_amd import SYMBOLS, abi
    assert "hc_prep_ker_ex2" in SYMBOLS
    if not os.path.exists(abi.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert abi.load().hc_version() >= 4


@pytest.mark.parametrize("argv,msg", [(["resnet_fast", "3", "20", "2", "1", "false"], "out of scope"),
                                      (["resnet_fast", "3", "20", "3", "1", "false"], "out of scope"),
                                      (["resnet_fast", "3", "20", "1", "1", "true"], "out of scope"),
                                      (["resnet_fast", "3", "20", "4", "1", "false"], "panic: Wrong wide case!"),
                                      (["resnet_fast", "3", "9", "1", "1", "false"], "panic: wrong depth (not in 8, 14, 20)!"),
                                      (["resnet_fast", "4", "20", "1", "1", "false"], "panic: Wrong kernel wid (not in 3,5,7)"),
                                      (["resnet_fast", "3", "20", "1", "1"], "runtime error: index out of range")])
def test_resnet_fast_cli_refusals(tmp_path, argv, msg):
    """bad arguments end the command like a Go panic (status 2) before it touches a device"""
    cli = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")
    if not os.path.exists(cli):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([cli] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr, (argv, r.returncode, r.stderr[-300:])
    assert "CKKS parameters" not in r.stdout
