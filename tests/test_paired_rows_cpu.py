"""The rows kernels that run two transforms in lock step behind one twiddle load (hc_k_a1p, hc_k_a3p: both polynomials of a channel; hc_k_b3p: both key components of a
node) under the CPU emulator, against the oracle word for word. What test_emu_parity.py does not force: the 256-thread kernels of the big tree levels (small_levels = 0) with
launches of 1 and 3 nodes next to even ones, alone and in a batch of three ciphertexts, and the kernels' other arithmetic forms - the integer inverse pass of a1 (Q1 above 2^49)
and the folding forward pass of a3 / b5m (Q0 at or above 2^57), which no parity case of the default moduli (Q0 ~ 2^55, Q1 ~ 2^49) reaches."""
import os
import subprocess

import pytest

import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import Oracle, P0, Q0, Q1

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")

Q60 = pc.Q1_BL                      # 2^60 + ...: as Q0 it takes HC_FM_ALT (74 q >= 2^64), as Q1 the integer inverse pass (4 q >= 2^51)
assert Q60 >= 1 << 57 and Q60 > 1 << 49 and Q1 < 1 << 49 and Q0 < 1 << 57 and Q60 < P0


@pytest.fixture(scope="module")
def env():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx = Context([Q0, Q1], [P0], lib_path=EMU_LIB)
    ctx.set_option("small_levels", 0)
    yield ctx, Oracle()
    ctx.close()


@pytest.mark.parametrize("max_ob,chunk", [(8, 1), (8, 3), (16, 1), (16, 3)])
def test_big_level_kernels_with_odd_and_even_launches(env, max_ob, chunk):
    """chunk_nodes 1 and 3: loop A launches of 1 and 3 channels (2 and 6 jobs: one and three pairs), tree launches of 1, 2 and 3 nodes"""
    pc.case_conv(*env, max_ob, chunk=chunk)


@pytest.mark.parametrize("max_ob,chunk", [(8, 3), (8, 9), (16, 3)])
def test_big_level_kernels_in_a_batch_of_three(env, max_ob, chunk):
    """three ciphertexts per launch set: chunk 3 = one channel / one node of each per launch, chunk 9 = three (a pair never takes its partner from the next ciphertext)"""
    pc.case_conv_batch(*env, max_ob, 3, chunk=chunk)


@pytest.mark.parametrize("q0,q1", [(Q0, Q60), (Q60, Q1), (Q60, Q0)], ids=["integer-a1", "alt-a3-b5m", "alt-and-integer-a1"])
@pytest.mark.parametrize("small", [0, 16])
def test_other_modulus_sizes(q0, q1, small):
    """Q1 above 2^49: hc_k_a1p<0> (hc_rows_inv on two tiles); Q0 at or above 2^57: HC_FM_ALT in hc_k_a3p and hc_k_b5m. The parity case draws its inputs below the moduli of the oracle it is handed."""
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx = Context([q0, q1], [P0], lib_path=EMU_LIB)
    ctx.set_option("small_levels", small)
    try:
        pc.case_conv(ctx, Oracle(q=(q0, q1), p=(P0,)), 4, chunk=3)
    finally:
        ctx.close()


@pytest.mark.parametrize("inputs", ["random", "edge"])
@pytest.mark.parametrize("small", [0, 16])
@pytest.mark.parametrize("triple", pc.CONV_TRIPLES, ids=pc.conv_triple_id)
def test_conv_under_every_modulus_size_class(triple, small, inputs):
    """the six (Q0, Q1, P) of pc.CONV_TRIPLES: every branch the host takes on a modulus' size, a special prime below 2^57 and below Q0 included, on random and on edge rows"""
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    pc.case_conv_triple(lambda Q, P: Context(Q, P, lib_path=EMU_LIB), triple, small, inputs)


@pytest.mark.parametrize("triple", pc.CONV_TRIPLES, ids=pc.conv_triple_id)
def test_keyswitch_under_every_modulus_size_class(triple):
    pc.case_keyswitch_triple(lambda Q, P: Context(Q, P, lib_path=EMU_LIB), triple)


@pytest.mark.parametrize("triple", pc.CONV_TRIPLES_BATCH, ids=pc.conv_triple_id)
def test_conv_batch_under_other_modulus_sizes(triple):
    pc.case_conv_batch_triple(lambda Q, P: Context(Q, P, lib_path=EMU_LIB), triple)


def test_tile_local_galois_levels_still_read_b1s_t2c1(env):
    """the 1 024-channel sparse tree (Galois elements 2^7 + 1, 2^8 + 1): hc_k_b1 writes tmpT for the two-job hc_k_b5, with hc_k_b3p between them"""
    pc.case_keyswitch(*env, gals=(129, 257))
    pc.case_conv(*env, 1024, norm=16, out_scale=2.0 ** 41)
