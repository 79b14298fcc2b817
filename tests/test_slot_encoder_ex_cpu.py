"""No GPU needed: hc_encode_slots_ex is declared in include/hconv.h, typed in the abi.py table with the header's arity and exported by the cross-compiled libhconv.so
(hc_version() stays 5: the header says the entry point is detected by symbol); and its kernels, compiled for the CPU fiber emulator (tests/kernel_emu), give the oracle's
words at full N: the cases of tests/slot_encoder_cases.py, the ones tests/test_gpu_slot_encoder_ex.py runs on the device."""
import os
import re
import subprocess

import pytest

import slot_encoder_cases as sc
from optimal_conv_amd import Context
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
NAME = "hc_encode_slots_ex"
SIGNATURE = "int hc_encode_slots_ex(hc_ctx *ctx, double *values, int count, int log_slots, int level, int with_p, double scale, int to_ntt, uint64_t *out);"


def header_text():
    return open(os.path.join(ROOT, "include", "hconv.h")).read()


def test_symbol_is_declared_typed_and_exported():
    from optimal_conv_amd import SYMBOLS, abi
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S))
    assert SIGNATURE in text, f"{NAME} is not declared in include/hconv.h as issued"
    assert NAME in SYMBOLS, f"{NAME} is missing from the abi.py table"
    assert len(SYMBOLS[NAME][1]) == len(SIGNATURE.split(",")), f"{NAME}: the abi.py table and the header disagree on the number of arguments"
    if not os.path.exists(abi.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(abi.load(), NAME), f"libhconv.so does not export {NAME}"


def test_version_stays_5_and_the_header_says_detect_by_symbol():
    from optimal_conv_amd import abi
    m = re.search(r"int hc_version\(void\);\s*/\*(.*?)\*/", header_text(), flags=re.S)
    assert m and re.search(r"hc_encode_slots_ex\b.*\bby symbol", m.group(1), flags=re.S), "the header's hc_version comment does not say how hc_encode_slots_ex is detected"
    assert abi.load().hc_version() == 5


def test_context_method_exists():
    assert callable(getattr(Context, "encode_slots_ex", None)), "Context.encode_slots_ex"


# ---- the kernels on the CPU emulator (the emulated library is the product's sources compiled as they are)
@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    return (lambda Q, P: Context(Q, P, lib_path=EMU_LIB)), (lambda Q, P: Oracle(q=Q, p=P))


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_emulated_encoder_equals_the_oracle(emu, c):
    sc.case(*emu, *c)


def test_emulated_encoder_refusals_leave_the_context_usable(emu):
    sc.case_refusals(*emu)
