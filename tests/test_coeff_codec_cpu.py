"""No GPU needed: hc_encode_coeffs / hc_encrypt_sk / hc_decrypt_decode_coeffs are declared in include/hconv.h, typed in the abi.py table with the header's arity and
exported by the cross-compiled libhconv.so (hc_version() = 5); and the kernels themselves, compiled for the CPU fiber emulator (tests/kernel_emu), give the oracle's
words at full N: the encoder cases and the decryptor cases of tests/coeff_codec_cases.py, the ones tests/test_gpu_coeff_codec.py runs on the device."""
import os
import re
import subprocess

import pytest

import coeff_codec_cases as cc
from optimal_conv_amd import Context
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
NEW = ("hc_encode_coeffs", "hc_encrypt_sk", "hc_decrypt_decode_coeffs")


def header_text():
    return open(os.path.join(ROOT, "include", "hconv.h")).read()


def declared_arity(name):
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/hconv.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", NEW)
def test_symbol_is_declared_typed_and_exported(name):
    from optimal_conv_amd import SYMBOLS, abi
    assert name in SYMBOLS, f"{name} is missing from the abi.py table"
    assert len(SYMBOLS[name][1]) == declared_arity(name), f"{name}: the abi.py table and the header disagree on the number of arguments"
    if not os.path.exists(abi.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(abi.load(), name), f"libhconv.so does not export {name}"


def test_declared_signatures_are_the_issued_ones():
    text = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S))
    for sig in ("int hc_encode_coeffs(hc_ctx *ctx, const double *values, int count, int nvals, int level, double scale, int to_ntt, uint64_t *out);",
                "int hc_encrypt_sk(hc_ctx *ctx, int count, int level, const uint64_t *pt, const uint64_t *sk_ntt, const uint32_t *seed8, uint64_t stream_id, uint64_t *const *ct_out);",
                "int hc_decrypt_decode_coeffs(hc_ctx *ctx, int count, int level, const uint64_t *const *ct, const uint64_t *sk_ntt, double scale, double *out);"):
        assert sig in text, sig


def test_version_5_is_stated_in_the_header_and_returned():
    from optimal_conv_amd import abi
    m = re.search(r"int hc_version\(void\);\s*/\*(.*?)\*/", header_text(), flags=re.S)
    assert m and re.search(r"\b5: hc_encode_coeffs, hc_encrypt_sk, hc_decrypt_decode_coeffs", m.group(1)), "the header's hc_version comment does not state version 5"
    assert abi.load().hc_version() == 5


def test_context_methods_exist():
    for name in ("encode_coeffs", "encrypt_sk", "decrypt_decode_coeffs"):
        assert callable(getattr(Context, name, None)), f"Context.{name}"


# ---- the kernels on the CPU emulator (no existing file under tests/kernel_emu is touched: the emulated library is the product's sources compiled as they are)
@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    return (lambda Q, P: Context(Q, P, lib_path=EMU_LIB)), (lambda Q, P: Oracle(q=Q, p=P))


@pytest.mark.parametrize("chain,level,pack32,expect32", [(cc.CONV_CHAIN, 0, 1, False), (cc.CONV_CHAIN, 1, 1, False), (cc.BOOT_CHAIN, 3, 1, False), (cc.BOOT_CHAIN, 3, 2, False),
                                                         (cc.BOOT_SMALL, 3, 2, True)])
def test_emulated_encoder_equals_the_oracle(emu, chain, level, pack32, expect32):
    cc.case_encoder(*emu, chain[0], chain[1], level, cc.SCALE if level < 3 else cc.SCALE * 1.25 + 3, pack32=pack32, expect32=expect32)


def test_emulated_encoder_refuses_what_the_big_float_branch_would_take(emu):
    cc.case_refusals(*emu)


def test_emulated_decryptor_equals_the_oracle_at_level_0(emu):
    cc.case_decrypt_l0(*emu)


def test_emulated_decryptor_equals_the_oracle_at_level_1(emu, monkeypatch):
    cc.case_decrypt_l1(*emu, monkeypatch)
