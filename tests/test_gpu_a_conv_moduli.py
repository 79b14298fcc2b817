"""The conv path on the device under every modulus-size class (parity_cases.CONV_TRIPLES). Every other GPU conv test runs the product's own moduli - Q0 ~ 2^55, Q1 just below 2^49,
P ~ 2^61 - and with them one side of each branch the host takes on a modulus' size: these six triples execute the other kernel instantiations (hc_k_a1p<0>, hc_k_a2<*, 0>,
hc_k_a2<HC_FM_ALT, *>, the HC_FM_ALT forms of a3p / b4 / b5 / b5m / sb4 / sb5, the HC_FM_FREE forms of b2 / b3p / sb2 / sb3) against the oracle, bit for bit, on uniform and on
edge rows. One context per test, closed before the next."""
import pytest

import parity_cases as pc
from optimal_conv_amd import Context

pytestmark = pytest.mark.gpu

GPU = lambda Q, P: Context(Q, P)


@pytest.mark.parametrize("inputs", ["random", "edge"])
@pytest.mark.parametrize("small", [0, 16])
@pytest.mark.parametrize("triple", pc.CONV_TRIPLES, ids=pc.conv_triple_id)
def test_conv(triple, small, inputs):
    pc.case_conv_triple(GPU, triple, small, inputs)


@pytest.mark.parametrize("triple", pc.CONV_TRIPLES, ids=pc.conv_triple_id)
def test_keyswitch(triple):
    """rotate_gal_l0 / keyswitch_l0 for two Galois elements"""
    pc.case_keyswitch_triple(GPU, triple)


@pytest.mark.parametrize("triple", pc.CONV_TRIPLES_BATCH, ids=pc.conv_triple_id)
def test_conv_batch_of_three(triple):
    pc.case_conv_batch_triple(GPU, triple)
