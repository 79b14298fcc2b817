"""hc_lv_op2(HC_LV_MONOMIAL) on the GPU against the CPU oracle and against the sequences it replaces in the hosts (run through the same library). The cases are in
tests/monomial_cases.py (shared with the CPU emulator's run of the same kernel). N = 2^16 is fixed: levels <= 3 and <= 3 images."""
import pytest

import monomial_cases as mc
from optimal_conv_amd import Context
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

GPU = (lambda Q, P: Context(Q, P)), (lambda Q, P: Oracle(q=Q, p=P))


@pytest.mark.parametrize("chain,level,pack32,expect32", mc.SETTINGS)
def test_values_equal_the_oracle(chain, level, pack32, expect32):
    """every exponent class (+1, -1, both sides of the table split, the far end), alone and in pairs, random operands and a = b = q - 1, every word of every limb"""
    mc.case_values(*GPU, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


@pytest.mark.parametrize("chain,level,pack32,expect32", [(mc.CONV_CHAIN, 1, 1, False), (mc.BOOT_SMALL, 3, 2, True)])
def test_image_batch_equals_single_calls(chain, level, pack32, expect32):
    mc.case_batch(*GPU, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


@pytest.mark.parametrize("chain,level,pack32,expect32", [(mc.CONV_CHAIN, 1, 1, False), (mc.BOOT_SMALL, 3, 2, True)])
def test_output_may_be_an_operand(chain, level, pack32, expect32):
    mc.case_aliasing(*GPU, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


@pytest.mark.parametrize("chain,level,pack32,expect32", [(mc.BOOT_CHAIN, 3, 2, False), (mc.BOOT_SMALL, 3, 2, True)])
def test_chain_sequences_are_bit_equal(chain, level, pack32, expect32):
    mc.case_former_chain(*GPU, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


def test_stride_front_end_is_bit_equal():
    mc.case_former_stride(*GPU)


def test_refusals_leave_the_context_usable():
    mc.case_refusals(*GPU)


def test_operation_leaves_a_held_decomposition_and_the_arena_alone():
    """three images, pack32 = 2, three special primes, level 4: the environment of tests/test_gpu_a_abi_contract.py"""
    import abi_contract_cases as ab
    from test_gpu_a_abi_contract import LEVEL, make_ctx, mo
    E = ab.part_a_env(make_ctx(2)(*ab.chain(LEVEL, 3)), LEVEL, 3)
    try:
        mc.case_held_decomposition_survives(E, make_oracle=mo)
    finally:
        E.close(); E.ctx.close()
