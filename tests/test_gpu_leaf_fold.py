"""The leaf level through folded kernel plaintexts (hc_kernels.h above hc_k_b1x; hconv.hip hc_ker_fold), on the device: tests/test_leaf_fold_cpu.py shows the arithmetic word
for word in the emulator; what only the device can show is hc_k_b1x at five and hc_k_b5x at four workgroups per CU, real wavefronts at hc_k_b5x's one barrier per row batch, and
loop A's launches for the x-role channels reading the folded array while the tree's reads of the other channels are still queued. Four and eight channels and the sparse packing
(norm = 2), small_levels = 0 and launches of three nodes, under the product's moduli (HC_FM_FREE) and pc.CONV_TRIPLES[1] (HC_FM_ALT), each compared word for word with the
oracle and each seen to have folded (the profile entry of the kernel that makes the folded array). One context per test, closed before the next."""
import pytest

import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import P0, Q0, Q1

pytestmark = pytest.mark.gpu

PRODUCT = (Q0, Q1, P0, (True, True, False))
TRIPLES = [PRODUCT, pc.CONV_TRIPLES[1]]
FOLD = "ker_fold_monomial"


@pytest.fixture(params=TRIPLES, ids=pc.conv_triple_id)
def env(request):
    ctx, O = pc._triple_env(lambda Q, P: Context(Q, P), request.param)
    ctx.set_option("small_levels", 0)
    ctx.set_option("profile", 1)
    ctx.profile_reset()
    yield ctx, O
    ctx.close()


@pytest.mark.parametrize("max_ob", [4, 8])
def test_one_convolution(env, max_ob):
    ctx, O = env
    pc.case_conv(ctx, O, max_ob, chunk=3)
    assert ctx.profile().get(FOLD, (0.0, 0))[1] == 1


def test_sparse_packing(env):
    ctx, O = env
    pc.case_conv(ctx, O, 8, chunk=3, norm=2)
    assert ctx.profile().get(FOLD, (0.0, 0))[1] == 1
