"""hc_k_b5m on one LDS tile (hc_kernels.h), on the device: the two register tiles exchanged in turn, the epilogue's two polynomials through disjoint row sets of the same tile
with one barrier per row batch. tests/test_b5m_one_tile_cpu.py shows in the emulator that no row is reused without a barrier between; what only the device can show is three
workgroups of the kernel resident on a CU (HC_B5M_WAVES) and the order in which real wavefronts reach the barriers. The same batch of three ciphertexts (four channels,
small_levels = 0, launches of three nodes, a bias on the root) runs twice in a row on one context - the second time on warm pools - under the product's moduli (HC_FM_FREE) and
under pc.CONV_TRIPLES[1] (HC_FM_ALT), every member compared word for word with the oracle and with the same ciphertext run alone. One context per test, closed before the next."""
import pytest

import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import P0, Q0, Q1

pytestmark = pytest.mark.gpu

PRODUCT = (Q0, Q1, P0, (True, True, False))
TRIPLES = [PRODUCT, pc.CONV_TRIPLES[1]]
REPEATS = 2


@pytest.fixture(params=TRIPLES, ids=pc.conv_triple_id)
def env(request):
    ctx, O = pc._triple_env(lambda Q, P: Context(Q, P), request.param)
    yield ctx, O
    ctx.close()


def test_batch_of_three_twice(env):
    ctx, O = env
    ctx.set_option("small_levels", 0)
    for _ in range(REPEATS):
        pc.case_conv_batch(ctx, O, 4, 3, chunk=3, oracle_members=(0, 1, 2))
