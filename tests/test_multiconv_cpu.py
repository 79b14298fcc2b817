"""The convolution with several input ciphertexts (hc_conv_then_pack_batch's members with one ct_out) without a GPU: (1) the yardstick tests/multiconv_ref.py is itself
pinned to the oracle's fused calls; (2) the grouped kernels hc_k_a1g / hc_k_a3g and the host's grouping rule on the emulated kernel library, word for word against the
yardstick; (3) the plain model: summing the per-ciphertext products ahead of ONE packing tree is the m*B-channel convolution, exactly; (4) the `multiconv` command."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden.gen_conv_csv as gen_conv
import golden.gen_multiconv_csv as gen
import multiconv_cases as mc
import multiconv_ref as MR
import parity_cases as pc
import transconv_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
EMU_CLI = os.path.join(EMU_DIR, "_build", "conv_emu")
S30 = 2.0 ** 30


class _NoDevice:
    """parity_cases.load_tree_keys without a device: only the oracle's key array is wanted"""
    def evk_load(self, gal, evk4):
        pass


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


# ---- 1. the yardstick is itself pinned
def test_yardstick_loopA_is_mul_setscale_at_one_input(oracle):
    O = oracle
    ct, ker = pc.planted_conv_inputs(0x111, 2, O)
    cst, _ = MR.setscale_consts(O, S30, S30, 2, 1, S30)
    for i in range(2):
        pc.eq(MR.loopA_sum(O, [ct], [ker[i]], cst), O.mul_setscale(ct, ker[i], cst), f"loopA_sum at m = 1, channel {i}")


@pytest.mark.parametrize("max_ob,norm", [(4, 1), (4, 2), (1, 1)])
def test_yardstick_is_conv_then_pack_at_one_input(oracle, max_ob, norm):
    O = oracle
    seed = 0x222 + max_ob + norm
    ct, ker = pc.planted_conv_inputs(seed, max_ob, O)
    evk_all = pc.load_tree_keys(_NoDevice(), seed, max_ob, norm, O)
    bias = pc.rows(seed + 5, pc.conv_moduli(O)[0])[0]
    want, sc = O.conv_then_pack(ct, S30, ker, S30, O.idx_plaintexts(), evk_all, max_ob, norm, S30, bias)
    assert sc == S30
    pc.eq(MR.multi_conv(O, [ct], [ker], evk_all, max_ob, norm, bias), want, f"pack_tree(loopA_sum) B={max_ob} norm={norm}")


# ---- 2. the emulated library
@pytest.fixture(scope="module")
def emu(oracle):
    from optimal_conv_amd import Context
    from oracle_lib import P0, Q0, Q1
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx = Context([Q0, Q1], [P0], lib_path=EMU_LIB)
    yield ctx, oracle
    ctx.close()


@pytest.mark.parametrize("m,G,max_ob,norm,chunk", mc.GROUP_TABLE, ids=[mc.group_id(t) for t in mc.GROUP_TABLE])
def test_groups_emulated(emu, m, G, max_ob, norm, chunk):
    mc.case_groups(*emu, m, G, max_ob, norm, chunk)


def test_multi_binding_emulated(emu):
    mc.case_multi_binding(*emu)


def test_refusals_emulated(emu):
    mc.case_refusals(*emu)


def test_distinct_outputs_are_the_batch_of_before_emulated(emu):
    mc.case_distinct_outputs_unchanged(*emu)


def test_integer_body_of_a1g_emulated():
    """Q1 just above 2^49: hc_k_a1g<0> (canonical running sum) and hc_k_a2<FREE, 0>, at an even and an odd m"""
    from optimal_conv_amd import Context
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    mc.case_branch(lambda Q, P: Context(Q, P, lib_path=EMU_LIB), pc.CONV_TRIPLES[0], "edge", ms=(2, 5))


# ---- 3. the plain shadow
@pytest.mark.parametrize("k,B,W,m", [(3, 4, 16, 2), (5, 4, 16, 3), (3, 16, 16, 4)])
def test_sum_over_ciphertext_slices_is_the_wide_convolution(k, B, W, m):
    """on a ring of degree N = B*W^2 and integer data: ciphertext j holds the channels j*B .. (j+1)*B - 1, its plaintexts are prep_Ker of that channel slice; the products
    summed slot by slot ahead of ONE packing tree give gen_conv_csv.plain_conv on the m*B-channel input exactly"""
    N, raw = B * W * W, W - k // 2
    rng = np.random.default_rng(1000 * k + 10 * B + m)
    x = rng.integers(-3, 4, size=(raw, raw, m * B)).astype(np.float64)
    ker = rng.integers(-3, 4, size=(k, k, m * B, B)).astype(np.float64)
    a = rng.integers(1, 4, size=B).astype(np.float64)
    prods = np.zeros((B, N), dtype=np.int64)
    for j in range(m):
        xs, ks = x[:, :, j * B:(j + 1) * B], np.ascontiguousarray(ker[:, :, j * B:(j + 1) * B, :])
        inp = np.rint(R.prep_input(xs, raw, W, N)).astype(np.int64)
        kc = np.rint(R.prep_ker_coeffs(ks.reshape(-1), a, W, k, B, B, N)).astype(np.int64)
        for i in range(B):
            prods[i] += R.negacyclic_mul(inp, kc[i])
    packed = R.pack_ctxts(list(prods), B)
    assert not np.any(packed % B)
    got = R.post_process(packed // B, raw, W)
    np.testing.assert_array_equal(got, gen_conv.plain_conv(x, ker, a, np.zeros(B)))


def test_fixture_model_and_layout():
    """gen_multiconv_csv: the m*B-channel shapes the command reads, and plain_conv as the model"""
    B, W, raw, x, ker, a, b = gen.make_case(3, 0, 0, 2)
    assert (B, W, raw) == (4, 128, 127) and x.shape == (127, 127, 8) and ker.shape == (3, 3, 8, 4) and a.shape == b.shape == (4,)


# ---- 4. the command
@pytest.mark.parametrize("argv,msg", [(["multiconv", "4", "0", "1", "2"], "Wrong kernel wid (not in 3,5,7)"),
                                      (["multiconv", "3", "4", "1", "2"], "Too many tests (>10) or too many batch index (>3)"),
                                      (["multiconv", "3", "0", "11", "2"], "Too many tests (>10) or too many batch index (>3)"),
                                      (["multiconv", "3", "-1", "1", "2"], "runtime error: index out of range"),
                                      (["multiconv", "3", "0", "1"], "runtime error: index out of range"),
                                      (["multiconv", "3", "0", "1", "0"], "Wrong number of input ciphertexts (not in 1..16)"),
                                      (["multiconv", "3", "0", "1", "17"], "Wrong number of input ciphertexts (not in 1..16)")])
def test_multiconv_cli_argument_panics(tmp_path, argv, msg):
    """bad arguments end the command like a Go panic (status 2) before it touches a device"""
    cli = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")
    if not os.path.exists(cli):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([cli] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and f"panic: {msg}" in r.stderr, (argv, r.returncode, r.stderr[-300:])
    assert "Ours start." not in r.stdout


def test_multiconv_cli_refuses_an_image_batch_past_16_members(tmp_path):
    cli = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")
    if not os.path.exists(cli):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([cli, "multiconv", "3", "0", "1", "5"], cwd=tmp_path, capture_output=True, text=True, timeout=60, env=dict(os.environ, HCONV_IMAGE_BATCH="4"))
    assert r.returncode == 2 and "HCONV_IMAGE_BATCH x n_in must be <= 16" in r.stderr, (r.returncode, r.stderr[-300:])
    assert "vec size" not in r.stdout


def test_multiconv_3_0_two_inputs_emulated(tmp_path):
    """the whole host path (evalConv_BN_multi: channel slices of the input and of the kernel, the grouped call, one bias add) on the emulated kernel library: `multiconv 3 0 1 2`
    decrypts to plain_conv on the 8-channel input. Floor: tests/test_gpu_z_cli.py holds `conv 3 0` to MED 23.0 bits; two independent ciphertext noises add, so
    -0.5*log2(2) = -0.5, and 0.5 bit of margin for the seed: 22.0."""
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_CLI])
    gen.write_case(str(tmp_path / "test_conv_data"), 3, 0, 0, 2)
    out = subprocess.run([EMU_CLI, "--test-mode", "multiconv", "3", "0", "1", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=1200,
                         env=dict(os.environ, HCONV_SEED="12345"))
    assert out.returncode == 0, out.stderr[-2000:]
    txt = out.stdout
    for pat in (r"^Multi-input convolution test start! \(No Bootstrapping\)$", r"^Ker:  3 batches:  4 widths:  128$", r"^Ours start\.$", r"^vec size: log2 =  16$",
                r"^raw input width:  127$", r"^kernel width:  3$", r"^num raw batches in & out:  8 ,  4$", r"^num input ciphertexts:  2$",
                r"^Plaintext \(kernel\) preparation, Done in \S+ $", r"^\t mult time:  \S+$", r"^\t Pack time:  \S+$", r"^Conv \(with BN\) Done in \S+ $",
                r"^Decryption Done in \S+ $"):
        assert re.search(pat, txt, re.M), f"missing line {pat!r} in:\n{txt}"
    assert "Base Line start." not in txt
    med = float(re.search(r"^MED Prec : \(([-0-9.]+), \+Inf\) Log2", txt, re.M).group(1))
    print("multiconv 3 0 1 2 (emulated): MED Prec", med)
    assert med >= 22.0, txt
