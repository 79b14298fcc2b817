"""hc_decode_coeffs (product: ckks.Encoder.DecodeCoeffs at any level on the device) and hc_decrypt_decode_lv (harness only) on the GPU against exact integer arithmetic in
Python. The cases are in tests/crt_decode_cases.py (shared with the CPU emulator's run of the same kernels). N = 2^16 is fixed: every case is one or three plaintexts, at
the levels where the kernel takes another path (2, 4, 15 with and without 4-byte rows, 27)."""
import pytest

import crt_decode_cases as cd
from optimal_conv_amd import Context
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

GPU = (lambda Q, P: Context(Q, P)), (lambda Q, P: Oracle(q=Q, p=P))


@pytest.mark.parametrize("chain,level,count,pack32,expect32", [(cd.CHAIN5, 2, 1, 1, False), (cd.CHAIN5, 2, 3, 1, False), (cd.CHAIN5, 4, 1, 1, False), (cd.CHAIN5, 4, 3, 1, False),
                                                               (cd.CHAIN16, 15, 1, 1, False), (cd.CHAIN16, 15, 3, 1, False), (cd.CHAIN16, 15, 1, 2, True), (cd.CHAIN16, 15, 3, 2, True),
                                                               (cd.CHAIN28, 27, 1, 1, False), (cd.CHAIN28, 27, 3, 1, False)])
def test_decoder_equals_exact_integers(chain, level, count, pack32, expect32):
    """planted residues, both signs: 0, 1, Q/2 and Q/2 - 1, the 53-bit ties and their sticky bits, every 64-bit word boundary of the magnitude, q0 q1 / 2 + 1 and random
    values of full width (a two-limb shortcut gets them wrong), at level 27 the largest finite double and the first infinity; a scale that is no power of two; NTT-domain
    input == coefficient-domain input"""
    cd.case_planted(*GPU, chain, level, count, pack32=pack32, expect32=expect32)


def test_levels_0_and_1_keep_the_bits_of_the_two_limb_decoder():
    cd.case_low_levels(*GPU)


@pytest.mark.parametrize("chain,level,pack32", [(cd.CHAIN5, 4, 1), (cd.CHAIN16, 15, 1), (cd.CHAIN16, 15, 2), (cd.CHAIN28, 27, 1)])
def test_decryptor_equals_decode_of_c0_plus_c1_s(chain, level, pack32):
    """c0 + c1 s formed with hc_lv_mul / hc_lv_add; log_slots 12 and 15 == hc_decode_slots of the coefficients (below the levels whose magnitudes overflow)"""
    cd.case_decrypt_relation(*GPU, chain, level, pack32=pack32)


def test_decryptor_equals_exact_integers_on_an_oracle_encryption():
    cd.case_decrypt_l4(*GPU)


def test_refusals_leave_the_context_usable():
    cd.case_refusals(*GPU)
