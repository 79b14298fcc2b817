"""Stride-2 transposed convolution (kind "TransConv") without a GPU: (a) the reference's formulas (prep_Input / reshape_ker / prep_Ker
with trans = true, encode_ker_final, the negacyclic product and the packing tree) compute TF's conv2d_transpose(strides=2, padding='SAME');
(b) hc_prep_ker_ex on the emulated kernel library gives those plaintexts bit for bit; (c) the `transconv` command's argument errors."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden.gen_conv_csv as gen_conv
import golden.gen_transconv_csv as gen
import transconv_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
EMU_CLI = os.path.join(EMU_DIR, "_build", "conv_emu")


def torch_transconv(x, ker):
    """x (raw, raw, ib), ker HWOI (k, k, ob, ib) -> (2raw, 2raw, ob)"""
    raw, k = x.shape[0], ker.shape[0]
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]
    w = torch.from_numpy(np.ascontiguousarray(ker)).permute(3, 2, 0, 1)
    return F.conv_transpose2d(xt, w, stride=2, padding=(k - 3) // 2)[0, :, :2 * raw, :2 * raw].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("B,W", [(4, 16), (16, 16)])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_reference_formulas_are_conv_transpose2d(k, B, W):
    """on a ring of degree N = B*W^2 and integer data the packed result equals conv_transpose2d exactly; the same shadow gives
    conv2d 'same' for kind Conv, so it reads the coefficients the packing tree collects"""
    N, ob = B * W * W, B // 4
    rng = np.random.default_rng(100 * k + B)
    raw = W // 2 - k // 2
    x = rng.integers(-3, 4, size=(raw, raw, B)).astype(np.float64)
    ker = rng.integers(-3, 4, size=(k, k, ob, B)).astype(np.float64)
    a = rng.integers(1, 4, size=ob).astype(np.float64)
    got = R.conv_plain(x, ker, a, W, k, B, ob, N, trans=True)
    assert got.shape == (2 * raw, 2 * raw, ob)
    np.testing.assert_array_equal(got, torch_transconv(x, ker) * a)
    raw = W - k // 2
    x = rng.integers(-3, 4, size=(raw, raw, B)).astype(np.float64)
    ker = rng.integers(-3, 4, size=(k, k, B, B)).astype(np.float64)
    np.testing.assert_array_equal(R.conv_plain(x, ker, np.ones(B), W, k, B, B, N, trans=False), gen_conv.plain_conv(x, ker, np.ones(B), np.zeros(B)))


def test_fixture_model_is_the_restatement():
    """gen_transconv_csv's plain model (torch, BN a / b) and the restatement agree on the CLI's layout at a small shape"""
    B, W, k = 4, 16, 5
    raw, ob = W // 2 - k // 2, B // 4
    rng = np.random.default_rng(7)
    x = rng.integers(-3, 4, size=(raw, raw, B)).astype(np.float64)
    ker = rng.integers(-3, 4, size=(k, k, ob, B)).astype(np.float64)
    a, b = np.array([2.0]), np.array([0.25])
    np.testing.assert_array_equal(gen.plain_transconv(x, ker, a, b), R.conv_plain(x, ker, a, W, k, B, ob, B * W * W, trans=True) + b)


@pytest.fixture(scope="module")
def emu():
    from optimal_conv_amd import Context
    from oracle_lib import Oracle, P0, Q0, Q1
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx = Context([Q0, Q1], [P0], lib_path=EMU_LIB)
    yield ctx, Oracle()
    ctx.close()


@pytest.mark.parametrize("k,i_batch", [(3, 0), (5, 1), (7, 2)])
def test_prep_ker_ex_emulated(emu, k, i_batch):
    R.case_prep_ker_trans(*emu, k, i_batch)


def test_prep_ker_ex_refuses_bad_trans(emu):
    from optimal_conv_amd import HconvError
    ctx = emu[0]
    import ctypes as C
    B, W, raw, x, ker, bna, bnb = gen.make_case(3, 0, 0)
    flat = np.ascontiguousarray(ker.reshape(-1))
    f64p = C.POINTER(C.c_double)
    h = C.c_void_p()
    assert ctx.L.hc_prep_ker_ex(ctx.h, flat.ctypes.data_as(f64p), flat.size, np.ascontiguousarray(bna).ctypes.data_as(f64p), W, 3, B, B // 4, 1,
                                2.0 ** 30, 2, C.byref(h)) != 0
    with pytest.raises(HconvError, match="input size inconsistent"):
        ctx.prep_ker(ker.reshape(-1), bna, W, 3, B, B, trans=True)


def test_version_and_symbol():
    from optimal_conv_amd import SYMBOLS, abi
    assert "hc_prep_ker_ex" in SYMBOLS
    if not os.path.exists(abi.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert abi.load().hc_version() >= 3


@pytest.mark.parametrize("argv,msg", [(["transconv", "4", "0", "1"], "Wrong kernel wid (not in 3,5,7)"),
                                      (["transconv", "3", "4", "1"], "Too many tests (>10) or too many batch index (>3)"),
                                      (["transconv", "3", "0", "11"], "Too many tests (>10) or too many batch index (>3)"),
                                      (["transconv", "3", "-1", "1"], "runtime error: index out of range"),
                                      (["transconv", "3", "0"], "runtime error: index out of range")])
def test_transconv_cli_argument_panics(tmp_path, argv, msg):
    """bad arguments end the command like a Go panic (status 2) before it touches a device"""
    cli = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")
    if not os.path.exists(cli):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([cli] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and f"panic: {msg}" in r.stderr, (argv, r.returncode, r.stderr[-300:])
    assert "Ours start." not in r.stdout


def test_transconv_3_0_1_emulated(tmp_path):
    """the whole host path (set_Variables "TransConv", prep_Input / prep_Ker with trans, evalConv_BN, post_process) on the emulated kernel
    library: `transconv 3 0 1` decrypts to the torch model"""
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_CLI])
    gen.write_case(str(tmp_path / "test_conv_data"), 3, 0, 0)
    out = subprocess.run([EMU_CLI, "--test-mode", "transconv", "3", "0", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=1200,
                         env=dict(os.environ, HCONV_SEED="12345"))
    assert out.returncode == 0, out.stderr[-2000:]
    txt = out.stdout
    for pat in (r"^Transposed convolution test start! \(No Bootstrapping\)$", r"^Ker:  3 batches:  4 widths:  128$", r"^Ours start\.$",
                r"^raw input width:  63$", r"^num raw batches in & out:  4 ,  1$", r"^Plaintext \(kernel\) preparation, Done in \S+ $",
                r"^\t mult time:  \S+$", r"^\t Pack time:  \S+$", r"^Conv \(with BN\) Done in \S+ $", r"^Decryption Done in \S+ $"):
        assert re.search(pat, txt, re.M), f"missing line {pat!r} in:\n{txt}"
    assert "Base Line start." not in txt
    med = float(re.search(r"^MED Prec : \(([-0-9.]+), \+Inf\) Log2", txt, re.M).group(1))
    assert med >= 22.0, txt


@pytest.mark.parametrize("n", [1, 3])
def test_conv_then_pack_on_trans_plaintexts_emulated(emu, n):
    R.case_conv_trans(*emu, 3, 0, n)
