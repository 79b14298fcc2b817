"""Every entry of tests/arith_cases.py through the DEVICE probe (tests/arith_probe/arith_probe.hip compiled by hipcc for gfx950 with the product's flags; build() makes it): the
bounds and congruences of csrc/hc_arith.h and of the butterfly policies of csrc/hc_kernels.h as the gfx950 code computes them - the short high product, the multiply-add chain
behind hc_opaque_uniform, the uncontracted fp64 sequence - at the operands where they are tight, against Python's integers. A few thousand elements and one or two launches per
operation and modulus."""
import os

import pytest

import arith_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(ac.DEVICE_LIB), f"{ac.DEVICE_LIB} is missing: __graft_entry__.build() makes it"
    return ac.Probe(ac.DEVICE_LIB)


@pytest.mark.parametrize("case", ac.PARAMS, ids=ac.case_id)
def test_form_at_its_bounds_on_the_device(probe, case):
    name, q = case
    ac.CASES[name][0](probe.run, q)


def test_every_kernel_of_the_probe_is_in_the_table(probe):
    """after the cases above: nothing in the probe goes unasked (module-scoped probe, so this counts their launches)"""
    seen = set()

    def spy(op, *a, **k):
        seen.add(op)
        return probe.run(op, *a, **k)
    for name, (fn, moduli) in ac.CASES.items():
        fn(spy, moduli[0])
    assert seen == set(probe.ops())
