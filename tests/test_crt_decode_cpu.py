"""No GPU needed: hc_decode_coeffs / hc_decrypt_decode_lv are declared in include/hconv.h, typed in the abi.py table with the header's arity and exported by the
cross-compiled libhconv.so (hc_version() stays 5: they are detected by symbol); Python's float(int), the expected value of every case, is correctly rounded; and the kernels
themselves, compiled for the CPU fiber emulator (tests/kernel_emu), give those doubles at full N: the cases of tests/crt_decode_cases.py, the ones
tests/test_gpu_crt_decode.py runs on the device."""
import fractions
import os
import random
import re
import subprocess

import numpy as np
import pytest

import crt_decode_cases as cd
from optimal_conv_amd import Context
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
NEW = ("hc_decode_coeffs", "hc_decrypt_decode_lv")


def header_text():
    return open(os.path.join(ROOT, "include", "hconv.h")).read()


@pytest.mark.parametrize("name", NEW)
def test_symbol_is_declared_typed_and_exported(name):
    from optimal_conv_amd import SYMBOLS, abi
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/hconv.h"
    assert name in SYMBOLS, f"{name} is missing from the abi.py table"
    assert len(SYMBOLS[name][1]) == len([a for a in m.group(1).split(",") if a.strip()]), f"{name}: the abi.py table and the header disagree on the number of arguments"
    if not os.path.exists(abi.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(abi.load(), name), f"libhconv.so does not export {name}"


def test_declared_signatures_are_the_issued_ones_and_the_version_stays_5():
    from optimal_conv_amd import abi
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S))
    for sig in ("int hc_decode_coeffs(hc_ctx *ctx, const uint64_t *pt, int count, int level, int from_ntt, double scale, double *out);",
                "int hc_decrypt_decode_lv(hc_ctx *ctx, int count, int level, const uint64_t *const *c0, const uint64_t *const *c1, const uint64_t *sk_ntt, double scale, int log_slots, double *out);"):
        assert sig in text, sig
    m = re.search(r"int hc_version\(void\);\s*/\*(.*?)\*/", header_text(), flags=re.S)
    assert m and "hc_decode_coeffs and hc_decrypt_decode_lv: detect them by symbol" in m.group(1), "the header must say the new entry points are detected by symbol"
    assert abi.load().hc_version() == 5
    for name in ("decode_coeffs", "decrypt_decode_lv"):
        assert callable(getattr(Context, name, None)), f"Context.{name}"


def test_python_float_of_int_is_correctly_rounded():
    """the reference of every case: float(int) must be the nearest double, ties to even, at every width the cases use - checked in exact rationals against both neighbours"""
    rnd = random.Random(5)
    vals = [2 ** 80 + 2 ** 27, 2 ** 80 + 2 ** 27 + 1, 2 ** 80 + 3 * 2 ** 27, 2 ** 1024 - 2 ** 970 - 1, 2 ** 64 - 1, 2 ** 53 + 1]
    vals += [rnd.randrange(1 << rnd.randrange(54, 1024)) for _ in range(2000)]
    for t in vals:
        f = float(t)
        with np.errstate(over="ignore"):
            lo, hi = np.nextafter(f, 0.0), np.nextafter(f, np.inf)
        err = abs(fractions.Fraction(f) - t)
        for nb in (lo, hi):
            if np.isfinite(nb):
                e2 = abs(fractions.Fraction(float(nb)) - t)
                assert err < e2 or (err == e2 and int(np.float64(f).view(np.uint64)) % 2 == 0), t
    with pytest.raises(OverflowError):
        float(2 ** 1024 - 2 ** 970)


# ---- the kernels on the CPU emulator (the emulated library is the product's sources compiled as they are)
@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    return (lambda Q, P: Context(Q, P, lib_path=EMU_LIB)), (lambda Q, P: Oracle(q=Q, p=P))


@pytest.mark.parametrize("chain,level,count,pack32,expect32", [(cd.CHAIN5, 2, 3, 1, False), (cd.CHAIN5, 4, 1, 1, False), (cd.CHAIN16, 15, 1, 1, False), (cd.CHAIN16, 15, 3, 2, True),
                                                               (cd.CHAIN28, 27, 1, 1, False)])
def test_emulated_decoder_equals_exact_integers(emu, chain, level, count, pack32, expect32):
    cd.case_planted(*emu, chain, level, count, pack32=pack32, expect32=expect32)


def test_emulated_levels_0_and_1_keep_the_bits_of_the_two_limb_decoder(emu):
    cd.case_low_levels(*emu)


@pytest.mark.parametrize("chain,level,pack32", [(cd.CHAIN5, 4, 1), (cd.CHAIN16, 15, 2)])
def test_emulated_decryptor_equals_decode_of_c0_plus_c1_s(emu, chain, level, pack32):
    cd.case_decrypt_relation(*emu, chain, level, pack32=pack32)


def test_emulated_decryptor_equals_exact_integers_on_an_oracle_encryption(emu):
    cd.case_decrypt_l4(*emu)


def test_emulated_refusals_leave_the_context_usable(emu):
    cd.case_refusals(*emu)
