"""The leaf level's product with its idx plaintext is taken out of the pack tree (hc_kernels.h above hc_k_b1x; hconv.hip hc_ker_fold): the x-role channels' kernel plaintexts
are multiplied by the level's monomial once per handle, loop A run on that copy writes I*x, and the leaf level runs on hc_k_b1x / hc_k_b5x, which neither load idx nor form
the product. The claim is word-for-word equality with the unfolded computation, so every case below is compared with the oracle (which knows nothing of the fold), on the
fibre emulator, under the product's moduli (HC_FM_FREE) and pc.CONV_TRIPLES[1] (Q0 above 2^57: HC_FM_ALT), with small_levels = 0 and launches of three nodes, so that every
level runs on the 256-thread kernels and a level's last launch is a short one. FOLD is the profile name of the kernel that makes the copy: it tells whether a call folded."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import multiconv_cases as MC
import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import P0, Q0, Q1

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")

PRODUCT = (Q0, Q1, P0, (True, True, False))
TRIPLES = [PRODUCT, pc.CONV_TRIPLES[1]]
assert PRODUCT[0] < 1 << 57 <= pc.CONV_TRIPLES[1][0]             # one triple on each arithmetic form of hc_k_b5x
N = pc.N
S30 = 2.0 ** 30
FOLD = "ker_fold_monomial"


@pytest.fixture(params=TRIPLES, ids=pc.conv_triple_id)
def env(request):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx, O = pc._triple_env(lambda Q, P: Context(Q, P, lib_path=EMU_LIB), request.param)
    ctx.set_option("small_levels", 0)
    ctx.set_option("profile", 1)
    ctx.profile_reset()
    yield ctx, O
    ctx.close()


def folds(ctx):
    return ctx.profile().get(FOLD, (0.0, 0))[1]


def conv_on_handle(ctx, O, hk, ct_in, ker, evk_all, idx, max_ob, norm=1, bias=None):
    """hc_conv_then_pack on an existing handle == the oracle on the first max_ob plaintexts it was loaded with"""
    cin, out = ctx.buf(ct_in), ctx.buf(nwords=2 * N)
    b = ctx.buf(bias) if bias is not None else None
    sc = ctx.conv_then_pack_dev(cin, S30, hk, S30, max_ob, norm, S30, b, out)
    got = out.download((2, N))
    want, wsc = O.conv_then_pack(ct_in, S30, ker[:max_ob], S30, idx, evk_all, max_ob, norm, S30, bias)
    assert sc == wsc == S30
    pc.eq(got, want, f"conv_then_pack on a handle, B={max_ob} norm={norm}")
    for x in (cin, out, b):
        if x is not None:
            x.free()


@pytest.mark.parametrize("max_ob", [4, 8])
def test_one_convolution(env, max_ob):
    """four channels: the leaf level and the root; eight: a level between them that runs on the unfolded kernels"""
    ctx, O = env
    pc.case_conv(ctx, O, max_ob, chunk=3)
    assert folds(ctx) == 1


def test_sparse_packing(env):
    """norm = 2: every second channel is live, the folded array holds channels 4 and 6 one after the other"""
    ctx, O = env
    pc.case_conv(ctx, O, 8, chunk=3, norm=2)
    assert folds(ctx) == 1


def test_batch_of_three_twice(env):
    """three members, each its own handle, in one launch set and one at a time (which reuses the member's folded array): 3 folds per run"""
    ctx, O = env
    for run in (1, 2):
        pc.case_conv_batch(ctx, O, 4, 3, chunk=3, oracle_members=(0, 1, 2))
        assert folds(ctx) == 3 * run


def test_one_handle_at_two_shapes(env):
    """max_ob = 8, then 4, then 8 again on one handle: the folded array is remade for each shape (another half of the channels, another monomial), and kept between calls of one"""
    ctx, O = env
    seed = 0x1EAF
    ct_in, ker = pc.planted_conv_inputs(seed, 8, O)
    evk_all = pc.load_tree_keys(ctx, seed, 8, 1, O)             # the keys of max_ob = 4 are the upper two of these
    ctx.idx_load(None)
    ctx.set_option("chunk_nodes", 3)
    idx = O.idx_plaintexts()
    bias = pc.rows(seed + 5, pc.conv_moduli(O)[0])[0]
    hk = ctx.ker_load(ker)
    for n, max_ob in enumerate((8, 4, 8, 8), 1):
        conv_on_handle(ctx, O, hk, ct_in, ker, evk_all, idx, max_ob, bias=bias)
        assert folds(ctx) == min(n, 3)
    ctx.ker_free(hk)


def test_handle_keeps_its_plaintexts(env):
    """after a folded convolution hc_ker_download returns what was loaded and hc_conv_mult_phase multiplies by the unfolded plaintexts"""
    ctx, O = env
    seed, max_ob = 0x2EAF, 4
    ct_in, ker = pc.planted_conv_inputs(seed, max_ob, O)
    evk_all = pc.load_tree_keys(ctx, seed, max_ob, 1, O)
    ctx.idx_load(None)
    ctx.set_option("chunk_nodes", 3)
    hk = ctx.ker_load(ker)
    conv_on_handle(ctx, O, hk, ct_in, ker, evk_all, O.idx_plaintexts(), max_ob)
    assert folds(ctx) == 1
    pc.eq(ctx.ker_download(hk, max_ob), ker, "ker_download after a folded convolution")
    cin, out = ctx.buf(ct_in), ctx.buf(nwords=max_ob * 2 * N)
    ctx._ck(ctx.L.hc_conv_mult_phase(ctx.h, cin.ptr, C.c_double(S30), hk, C.c_double(S30), max_ob, 1, C.c_double(S30), out.ptr))
    cst = [O.const_for(S30 / max_ob / 2.0 ** 60, 1, l)[0] for l in range(2)]
    want = np.stack([O.mul_setscale(ct_in, ker[i], cst) for i in range(max_ob)])
    pc.eq(out.download((max_ob, 2, N)), want, "conv_mult_phase after a folded convolution")
    cin.free(); out.free(); ctx.ker_free(hk)


def test_host_table_equal_to_the_derived_one_folds(env):
    ctx, O = env
    seed, max_ob = 0x3EAF, 4
    ct_in, ker = pc.planted_conv_inputs(seed, max_ob, O)
    evk_all = pc.load_tree_keys(ctx, seed, max_ob, 1, O)
    idx = O.idx_plaintexts()
    ctx.idx_load(idx)
    ctx.set_option("chunk_nodes", 3)
    hk = ctx.ker_load(ker)
    conv_on_handle(ctx, O, hk, ct_in, ker, evk_all, idx, max_ob)
    assert folds(ctx) == 1
    ctx.ker_free(hk)


def test_another_idx_table_is_not_folded(env):
    """the leaf level's row replaced by random residues: no monomial, so no fold - the oracle's result for that table, from today's launches. Loaded over a handle that already
    holds a folded array for the derived table, which must not be used."""
    ctx, O = env
    seed, max_ob = 0x4EAF, 4
    ct_in, ker = pc.planted_conv_inputs(seed, max_ob, O)
    evk_all = pc.load_tree_keys(ctx, seed, max_ob, 1, O)
    ctx.set_option("chunk_nodes", 3)
    hk = ctx.ker_load(ker)
    ctx.idx_load(None)
    conv_on_handle(ctx, O, hk, ct_in, ker, evk_all, O.idx_plaintexts(), max_ob)
    assert folds(ctx) == 1
    idx = O.idx_plaintexts().copy()
    idx[1] = pc.rows(seed + 9, pc.conv_moduli(O)[0])[0]           # step = 2: the leaf level multiplies by idx[1]
    ctx.idx_load(idx)
    conv_on_handle(ctx, O, hk, ct_in, ker, evk_all, idx, max_ob)
    assert folds(ctx) == 1
    ctx.idx_load(None)                                           # and back: the array made for the first table is not taken for this one
    conv_on_handle(ctx, O, hk, ct_in, ker, evk_all, O.idx_plaintexts(), max_ob)
    assert folds(ctx) == 2
    ctx.ker_free(hk)


def test_small_level_kernels_are_not_folded(env):
    """small_levels = 16: both levels of four channels run on the S kernels, which multiply by idx themselves"""
    ctx, O = env
    ctx.set_option("small_levels", 16)
    pc.case_conv(ctx, O, 4, chunk=3)
    assert folds(ctx) == 0


def test_two_input_ciphertexts(env):
    """a grouped call, m = 2: both members' handles are folded and the grouped a1 / a3 sum the folded products"""
    ctx, O = env
    MC.case_groups(ctx, O, 2, 1, 4, 1, chunk=3)
    assert folds(ctx) == 2
