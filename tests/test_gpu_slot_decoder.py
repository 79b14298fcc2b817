"""hc_decode_slots / hc_decrypt_decode_slots (ckks.Encoder.Decode's float half, full and sparse slots; Decrypt + Decode at level 0 or 1) on the GPU: the cases of
tests/slot_decoder_cases.py against tests/oracle_bl.py (shared with the CPU emulator's run of the same kernels), doubles compared as 64-bit words. N = 2^16 is fixed: a
case is one to six vectors, or two ciphertexts of one or two limbs."""
import pytest

import slot_decoder_cases as sd
from optimal_conv_amd import Context
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    env = sd.Env((lambda Q, P: Context(Q, P)), (lambda Q, P: Oracle(q=Q, p=P)))
    yield env
    env.close()


@pytest.mark.parametrize("count", sd.COUNTS)
@pytest.mark.parametrize("log_slots", sd.LOG_SLOTS)
def test_decoder_equals_the_oracle(gpu, log_slots, count):
    """four kinds of input (mixed exponents, zeros, 1.0 at coefficient 0, 1.0 at coefficient N/2); garbage on every coefficient off the gap grid"""
    sd.case_decode(gpu, log_slots, count)


@pytest.mark.parametrize("log_slots", [15, 12])
@pytest.mark.parametrize("level", [0, 1])
def test_decrypt_decode_slots_is_the_two_calls_composed(gpu, level, log_slots):
    sd.case_decrypt_composed(gpu, level, log_slots)


def test_decrypt_decode_slots_equals_the_level_1_oracle(gpu):
    sd.case_decrypt_l1_oracle(gpu)


@pytest.mark.parametrize("log_slots", [0, 8, 12, 15])
def test_round_trip_through_the_encoder(gpu, log_slots):
    sd.case_round_trip(gpu, log_slots)


def test_refusals_leave_the_context_usable(gpu):
    sd.case_refusals(gpu)
