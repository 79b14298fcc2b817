"""The rows kernels that fetch the A group of their twiddles through an LDS image (HcTwL in hc_kernels.h: hc_k_a1p, hc_k_a3p, hc_k_b1, hc_k_b3p, hc_k_b5m), on the device.
The image has a fixed index map, so a wrong map fails every conv parity test there is. What those cannot show is a missing or misplaced row-local sync around the image, or around
its reuse of the exchange tile: that is a race, intermittent, and invisible to the CPU emulator (which runs a block's threads one after the other). So the same small convolution
runs five times on one context and every repetition is compared word for word with the oracle - under the product's moduli and under the triple that flips every arithmetic
branch (hc_k_a1p<0>, the HC_FM_ALT forms of a3p / b5m, the HC_FM_FREE form of b3p). Four channels is the smallest tree that runs every one of these kernels on all 16 tiles, with
a batch and a launch boundary (chunk) inside a level. One context per test, closed before the next."""
import pytest

import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import P0, Q0, Q1

pytestmark = pytest.mark.gpu

GPU = lambda Q, P: Context(Q, P)
PRODUCT = (Q0, Q1, P0, (True, True, False))
TRIPLES = [PRODUCT, pc.CONV_TRIPLES[5]]
REPEATS = 5


@pytest.fixture(params=TRIPLES, ids=pc.conv_triple_id)
def env(request):
    ctx, O = pc._triple_env(GPU, request.param)
    yield ctx, O
    ctx.close()


def test_conv_batch_repeated(env):
    """a batch of three through b1 .. b4 and b5m (small_levels = 0), launches of nine jobs; each repetition == three separate calls == the oracle"""
    ctx, O = env
    ctx.set_option("small_levels", 0)
    for _ in range(REPEATS):
        pc.case_conv_batch(ctx, O, 4, 3, chunk=9)


def test_conv_default_levels(env):
    """one convolution at the default small_levels (the top of the tree on the sb* kernels, loop A on a1p / a3p), launches of three jobs"""
    pc.case_conv(*env, 4, chunk=3)


def test_keyswitch_level0(env):
    """the level-0 key switch: b1 .. b4 and the two-job hc_k_b5, whose b1 stores t2.c1"""
    pc.case_keyswitch(*env)
