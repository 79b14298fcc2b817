"""hc_k_b5m runs both of its rows-forward transforms and its epilogue through ONE 32 KiB LDS tile (hc_kernels.h): the two register tiles are exchanged in turn, and in the
epilogue polynomial 0 of row batch b goes through tile rows b .. b + 3 while polynomial 1 goes through the rows eight further on, with no barrier beyond the one per batch.
The fibre emulator runs every fibre of a workgroup up to its next barrier before any goes on, so a tile row that is written again without a barrier after its last read holds
the wrong words deterministically here - on the device the same mistake is a race. Checked word for word against the oracle on the smallest tree that sends every level
through b1 .. b4 and hc_k_b5m on all 16 tiles (four channels, small_levels = 0, launches of three nodes; tests/test_gpu_twiddle_stage.py), a batch of three ciphertexts, under
the product's moduli (HC_FM_FREE) and under pc.CONV_TRIPLES[1] (Q0 above 2^57: HC_FM_ALT). Each tree level has its own Galois element, so every in-row permutation the tree uses
reads the aliased rows; the bias lands on the root node."""
import os
import subprocess

import pytest

import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import P0, Q0, Q1

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")

PRODUCT = (Q0, Q1, P0, (True, True, False))
TRIPLES = [PRODUCT, pc.CONV_TRIPLES[1]]
assert PRODUCT[0] < 1 << 57 <= pc.CONV_TRIPLES[1][0]             # one triple on each arithmetic form of hc_k_b5m


@pytest.fixture(params=TRIPLES, ids=pc.conv_triple_id)
def env(request):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx, O = pc._triple_env(lambda Q, P: Context(Q, P, lib_path=EMU_LIB), request.param)
    ctx.set_option("small_levels", 0)
    yield ctx, O
    ctx.close()


def test_batch_of_three_against_the_oracle_and_one_at_a_time(env):
    """hc_conv_then_pack_batch on three ciphertexts (a bias on members 0 and 2) == the oracle for every member, and == hc_conv_then_pack on the three one at a time"""
    pc.case_conv_batch(*env, 4, 3, chunk=3, oracle_members=(0, 1, 2))


def test_one_convolution_with_a_bias(env):
    """one convolution of four channels with the bias on the root node == the oracle"""
    pc.case_conv(*env, 4, chunk=3)
