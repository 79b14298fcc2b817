"""The fixed-operand streams of the convolution's kernels (hc_kernels.h), in the fibre emulator against the oracle, bit for bit. hc_k_a2, hc_k_b2 and hc_k_b4 take the colsB
round's twiddles of both their transforms from a wave-local LDS image (HcTwC) instead of one global load per slot: small_levels = 0 keeps every tree level on b1 .. b4 and b5m, so
every instantiation of the three runs at every level. Three modulus triples: the product's own (a1p / a2 in fp64, the FREE forms), one with Q1 >= 2^49 (integer a1p / a2) and one
with Q0 >= 2^57 (the ALT forms). A batch of three ciphertexts with their own inputs and kernel plaintexts - one all q - 1, one all 0 - is compared member by member with the same
convolution run alone and with the oracle: a wrong stride of loop A's fixed operand c' ([z][2 polys][2 limbs][N]) between batch members shows there. hc_mont_lazy - the product
on 8-byte Montgomery operands that hc_k_b5m uses, measured for c' in hc_k_a1p / hc_k_a3p and for idx in hc_k_b1 and not kept there (profiles/operand_streams_ab.txt) - is checked
against exact integers at the operand extremes under Q0 and Q1 of each triple."""
import os
import subprocess

import numpy as np
import pytest

import arith_cases as ac
import parity_cases as pc
from oracle_lib import P0, Q0, Q1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
N = pc.N

BENCH_TRIPLE = (Q0, Q1, P0, (True, True, False))        # hc_k_a1p<1>, hc_k_a2<FREE, 1>, the FREE forms of a3p / b4 / b5m
INT_A1_TRIPLE = pc.CONV_TRIPLES[0]                      # Q1 >= 2^49: hc_k_a1p<0>, hc_k_a2<FREE, 0>
ALT_TRIPLE = pc.CONV_TRIPLES[1]                         # Q0 >= 2^57: hc_k_a2<ALT, 1>, the ALT forms of a3p / b4 / b5m
TRIPLES = [BENCH_TRIPLE, INT_A1_TRIPLE, ALT_TRIPLE]
assert INT_A1_TRIPLE[1] >= 1 << 49 and ALT_TRIPLE[0] >= 1 << 57


def case_batch_of_three(make_ctx, triple, max_ob=4, seed=0x0B57):
    """three ciphertexts through ONE launch set (4 channels, launches of 3 nodes per ciphertext, small_levels = 0): member 0 uniform residues with a bias, member 1 every input and
    kernel residue q - 1, member 2 all 0. Each member == the same convolution alone == the oracle."""
    ctx, O = pc._triple_env(make_ctx, triple)
    q0, q1 = triple[0], triple[1]
    try:
        ctx.set_option("small_levels", 0)
        ctx.set_option("chunk_nodes", 9)
        evk_all = pc.load_tree_keys(ctx, seed, max_ob, 1, O)
        ctx.idx_load(None)
        ins, kers = [], []
        ct_in, ker = pc.planted_conv_inputs(seed, max_ob, O)
        ins.append(ct_in); kers.append(ker)
        for fill in (lambda q: q - 1, lambda q: 0):
            ct_in, ker = np.empty((2, 2, N), dtype=np.uint64), np.empty((max_ob, 2, N), dtype=np.uint64)
            ct_in[:, 0], ct_in[:, 1], ker[:, 0], ker[:, 1] = fill(q0), fill(q1), fill(q0), fill(q1)
            ins.append(ct_in); kers.append(ker)
        biases = [pc.rows(seed + 5, q0)[0], None, None]
        hk = [ctx.ker_load(k) for k in kers]
        bin_ = [ctx.buf(x) for x in ins]
        bb = [ctx.buf(b) if b is not None else None for b in biases]
        bout = [ctx.buf(nwords=2 * N) for _ in range(3)]
        ctx.conv_then_pack_batch_dev(bin_, 2.0 ** 30, hk, 2.0 ** 30, max_ob, 1, 2.0 ** 30, bb, bout)
        got = [b.download((2, N)) for b in bout]
        one = ctx.buf(nwords=2 * N)
        idx = O.idx_plaintexts()
        for z in range(3):
            ctx.conv_then_pack_dev(bin_[z], 2.0 ** 30, hk[z], 2.0 ** 30, max_ob, 1, 2.0 ** 30, bb[z], one)
            pc.eq(got[z], one.download((2, N)), f"batch member {z} vs the same convolution alone")
            want, _ = O.conv_then_pack(ins[z], 2.0 ** 30, kers[z], 2.0 ** 30, idx, evk_all, max_ob, 1, 2.0 ** 30, biases[z])
            pc.eq(got[z], want, f"batch member {z} vs the oracle")
        assert got[0].any() and not np.array_equal(got[0], got[1])
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def emu():
    from optimal_conv_amd import Context
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    return lambda Q, P: Context(Q, P, lib_path=EMU_LIB)


@pytest.mark.parametrize("triple", TRIPLES, ids=pc.conv_triple_id)
def test_conv_on_the_big_level_kernels(emu, triple):
    pc.case_conv_triple(emu, triple, 0, "random")


@pytest.mark.parametrize("triple", TRIPLES, ids=pc.conv_triple_id)
def test_batch_of_three_with_extreme_members(emu, triple):
    case_batch_of_three(emu, triple)


@pytest.fixture(scope="module")
def probe():
    return ac.Probe(ac.build_host_twin())


@pytest.mark.parametrize("q", sorted({t[i] for t in TRIPLES for i in (0, 1)}), ids=lambda q: f"q{q:x}")
def test_mont_lazy_is_exact_at_the_operand_extremes(probe, q):
    """hc_mont_lazy(x, w 2^64 mod q) for x in {0, 1, q - 1, 2^64 - 1}, w in {0, 1, q - 1}: the very integer
    hi + q - mulhi(lo * qinv, q) of m = x * wm, congruent to x w, in [1, 2q - 1]"""
    M64 = ac.M64
    qinv = pow(q, -1, 1 << 64)
    xs, ws = [0, 1, q - 1, M64], [0, 1, q - 1]
    x, w = ac.cols([(a, b) for a in xs for b in ws])
    wm = [(v << 64) % q for v in w]
    got = probe.run("mont_lazy", [q, qinv], [x, wm])[0]
    for xi, wi, mi, r in zip(x, w, wm, got):
        m = xi * mi
        assert r == (m >> 64) + q - ((((m & M64) * qinv) & M64) * q >> 64), (hex(xi), hex(wi), hex(r))
        assert r % q == xi * wi % q and 0 < r < 2 * q, (hex(xi), hex(wi), hex(r))
