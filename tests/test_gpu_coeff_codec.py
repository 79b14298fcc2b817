"""hc_encode_coeffs (product: ckks.Encoder.EncodeCoeffs + ToNTT on the device), hc_encrypt_sk and hc_decrypt_decode_coeffs (harness only) on the GPU against the CPU
oracle. The cases are in tests/coeff_codec_cases.py (shared with the CPU emulator's run of the same kernels). N = 2^16 is fixed: every case is one to three vectors at
levels 0 to 3."""
import pytest

import coeff_codec_cases as cc
from optimal_conv_amd import Context
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

GPU = (lambda Q, P: Context(Q, P)), (lambda Q, P: Oracle(q=Q, p=P))


@pytest.mark.parametrize("chain,level,pack32,expect32", [(cc.CONV_CHAIN, 0, 1, False), (cc.CONV_CHAIN, 1, 1, False), (cc.BOOT_CHAIN, 3, 1, False), (cc.BOOT_CHAIN, 3, 2, False),
                                                         (cc.BOOT_SMALL, 3, 1, False), (cc.BOOT_SMALL, 3, 2, True)])
def test_encoder_equals_the_oracle(chain, level, pack32, expect32):
    """word for word, the non-canonical q_l of a negative value that rounds to 0 included; count = 3, nvals in {0, 1, N - 1, N}, to_ntt 0 / 1. Level 3 of the bootstrapping
    chain has no limb below 2^31, so a second chain puts two of its ~30-bit limbs at levels 2 and 3: under pack32 = 2 those rows are 4-byte words (hc_row_is32)."""
    cc.case_encoder(*GPU, chain[0], chain[1], level, cc.SCALE if level < 3 else cc.SCALE * 1.25 + 3, pack32=pack32, expect32=expect32)


def test_encoder_refusals_leave_the_context_usable():
    cc.case_refusals(*GPU)


def test_encryption_relation_and_round_trip():
    """c0 + c1 s - m is one integer polynomial per image under both limbs, |e| <= 19, with the sampler's variance; streams are reproducible and distinct; and
    decrypt(encrypt(encode(v))) * scale - round(v * scale) is that e exactly, at levels 1 and 0"""
    cc.case_encrypt_relation(*GPU)


def test_decryptor_equals_the_oracle_at_level_0():
    cc.case_decrypt_l0(*GPU)


def test_decryptor_equals_the_oracle_at_level_1(monkeypatch):
    """the CRT magnitude's conversion is correctly rounded: ties at the 53-bit boundary, sticky bits, the 64-bit word boundary, both sides of Q/2"""
    cc.case_decrypt_l1(*GPU, monkeypatch)
