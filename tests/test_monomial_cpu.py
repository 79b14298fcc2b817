"""No GPU needed: hc_lv_op2(HC_LV_MONOMIAL) on the CPU fiber emulator (tests/kernel_emu: the product's kernel sources compiled as they are) gives the oracle's words at
full N - the cases of tests/monomial_cases.py, the ones tests/test_gpu_monomial.py runs on the device - and the interface came without a new symbol or version."""
import os
import re
import subprocess

import pytest

import monomial_cases as mc
from optimal_conv_amd import Context
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    return (lambda Q, P: Context(Q, P, lib_path=EMU_LIB)), (lambda Q, P: Oracle(q=Q, p=P))


def test_the_operation_is_an_enum_value_and_a_binding_not_a_symbol():
    import optimal_conv_amd
    text = open(os.path.join(ROOT, "include", "hconv.h")).read()
    assert re.search(r"enum \{[^}]*\bHC_LV_MONOMIAL = 10\b[^}]*\};\s*int hc_lv_op2\(", text), "HC_LV_MONOMIAL = 10 belongs to the enum of hc_lv_op2"
    assert optimal_conv_amd.HC_LV_MONOMIAL == 10 and callable(getattr(Context, "lv_monomial", None))
    assert not [s for s in optimal_conv_amd.SYMBOLS if "monomial" in s], "the operation enters through hc_lv_op2: no entry point of its own"


@pytest.mark.parametrize("chain,level,pack32,expect32", mc.SETTINGS)
def test_emulated_values_equal_the_oracle(emu, chain, level, pack32, expect32):
    mc.case_values(*emu, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


@pytest.mark.parametrize("chain,level,pack32,expect32", [(mc.CONV_CHAIN, 1, 1, False), (mc.BOOT_SMALL, 3, 2, True)])
def test_emulated_image_batch_equals_single_calls(emu, chain, level, pack32, expect32):
    mc.case_batch(*emu, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


@pytest.mark.parametrize("chain,level,pack32,expect32", [(mc.CONV_CHAIN, 1, 1, False), (mc.BOOT_SMALL, 3, 2, True)])
def test_emulated_output_may_be_an_operand(emu, chain, level, pack32, expect32):
    mc.case_aliasing(*emu, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


@pytest.mark.parametrize("chain,level,pack32,expect32", [(mc.BOOT_CHAIN, 3, 2, False), (mc.BOOT_SMALL, 3, 2, True)])
def test_emulated_chain_sequences_are_bit_equal(emu, chain, level, pack32, expect32):
    mc.case_former_chain(*emu, chain[0], chain[1], level, pack32=pack32, expect32=expect32)


def test_emulated_stride_front_end_is_bit_equal(emu):
    mc.case_former_stride(*emu)


def test_emulated_refusals_leave_the_context_usable(emu):
    mc.case_refusals(*emu)


def test_emulated_operation_leaves_a_held_decomposition_and_the_arena_alone(emu):
    """three images, pack32 = 2, three special primes, level 4: the environment of tests/test_emu_abi_contract.py"""
    import abi_contract_cases as ab
    from test_emu_abi_contract import LEVEL, make_ctx
    from test_emu_chain_edges import mo
    E = ab.part_a_env(make_ctx(2)(*ab.chain(LEVEL, 3)), LEVEL, 3)
    try:
        mc.case_held_decomposition_survives(E, make_oracle=mo)
    finally:
        E.close(); E.ctx.close()
