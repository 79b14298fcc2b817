"""No GPU needed: hc_decode_slots and hc_decrypt_decode_slots are declared in include/hconv.h, typed in the abi.py table with the header's arity and exported by the
cross-compiled libhconv.so (hc_version() stays 5: the header says the entry points are detected by symbol); and their kernels, compiled for the CPU fiber emulator
(tests/kernel_emu), give the oracle's words at full N: the cases of tests/slot_decoder_cases.py, the ones tests/test_gpu_slot_decoder.py runs on the device."""
import os
import re
import subprocess

import pytest

import slot_decoder_cases as sd
from optimal_conv_amd import Context
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
SIGNATURES = {
    "hc_decode_slots": "int hc_decode_slots(hc_ctx *ctx, const double *coeffs, int count, int log_slots, double *values_out);",
    "hc_decrypt_decode_slots": "int hc_decrypt_decode_slots(hc_ctx *ctx, int count, int level, const uint64_t *const *ct, const uint64_t *sk_ntt, double scale, int log_slots, double *values_out);",
}


def header_text():
    return open(os.path.join(ROOT, "include", "hconv.h")).read()


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_symbol_is_declared_typed_and_exported(name):
    from optimal_conv_amd import SYMBOLS, abi
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S))
    assert SIGNATURES[name] in text, f"{name} is not declared in include/hconv.h as issued"
    assert name in SYMBOLS, f"{name} is missing from the abi.py table"
    assert len(SYMBOLS[name][1]) == len(SIGNATURES[name].split(",")), f"{name}: the abi.py table and the header disagree on the number of arguments"
    if not os.path.exists(abi.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(abi.load(), name), f"libhconv.so does not export {name}"


def test_version_stays_5_and_the_header_says_detect_by_symbol():
    from optimal_conv_amd import abi
    m = re.search(r"int hc_version\(void\);\s*/\*(.*?)\*/", header_text(), flags=re.S)
    assert m and re.search(r"hc_decode_slots\b.*\bhc_decrypt_decode_slots\b.*\bby symbol", m.group(1), flags=re.S), "the header's hc_version comment does not say how the decoder is detected"
    assert re.search(r"hc_encode_slots_ex\b.*\bby symbol", m.group(1), flags=re.S), "the header's wording about hc_encode_slots_ex is gone"
    assert hasattr(abi.load(), "hc_decode_slots") and abi.load().hc_version() == 5


def test_context_methods_exist():
    for name in ("decode_slots", "decrypt_decode_slots"):
        assert callable(getattr(Context, name, None)), f"Context.{name}"


# ---- the kernels on the CPU emulator (the emulated library is the product's sources compiled as they are)
@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    env = sd.Env((lambda Q, P: Context(Q, P, lib_path=EMU_LIB)), (lambda Q, P: Oracle(q=Q, p=P)))
    yield env
    env.close()


@pytest.mark.parametrize("count", sd.COUNTS)
@pytest.mark.parametrize("log_slots", sd.LOG_SLOTS)
def test_emulated_decoder_equals_the_oracle(emu, log_slots, count):
    sd.case_decode(emu, log_slots, count)


@pytest.mark.parametrize("log_slots", [15, 12])
@pytest.mark.parametrize("level", [0, 1])
def test_emulated_decrypt_decode_slots_is_the_two_calls_composed(emu, level, log_slots):
    sd.case_decrypt_composed(emu, level, log_slots)


def test_emulated_decrypt_decode_slots_equals_the_level_1_oracle(emu):
    sd.case_decrypt_l1_oracle(emu)


@pytest.mark.parametrize("log_slots", [0, 8, 12, 15])
def test_emulated_round_trip_through_the_encoder(emu, log_slots):
    sd.case_round_trip(emu, log_slots)


def test_emulated_refusals_leave_the_context_usable(emu):
    sd.case_refusals(emu)
