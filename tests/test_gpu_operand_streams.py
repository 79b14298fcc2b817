"""tests/test_operand_streams_cpu.py's batch of three ciphertexts (4 channels, small_levels = 0, own inputs and kernel plaintexts, one member all q - 1 and one all 0) on the device
against the oracle, under the product's own moduli and under the triple that takes the ALT forms: the cols kernels hc_k_a2, hc_k_b2, hc_k_b4 with their colsB twiddles through
wave-local LDS images, and loop A's fixed operand c' with its [z][2][2][N] layout across batch members."""
import pytest

import parity_cases as pc
from optimal_conv_amd import Context
from test_operand_streams_cpu import ALT_TRIPLE, BENCH_TRIPLE, case_batch_of_three

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("triple", [BENCH_TRIPLE, ALT_TRIPLE], ids=pc.conv_triple_id)
def test_batch_of_three_with_extreme_members(triple):
    case_batch_of_three(lambda Q, P: Context(Q, P), triple)
