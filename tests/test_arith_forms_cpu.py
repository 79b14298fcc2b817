"""Every entry of tests/arith_cases.py through the HOST twin of the arithmetic probe (tests/arith_probe/arith_probe.hip compiled by g++ against tests/kernel_emu): the bounds and
congruences that csrc/hc_arith.h and the butterfly policies of csrc/hc_kernels.h state, at the operands where they are tight, against Python's integers. This says that the
ARITHMETIC is right; what hipcc makes of it for gfx950 is tests/test_gpu_a_arith_forms.py's question. The last tests feed the checkers wrong answers: a checker that accepts
everything fails them."""
import os
import re

import pytest

import arith_cases as ac


@pytest.fixture(scope="module")
def probe():
    return ac.Probe(ac.build_host_twin())


@pytest.mark.parametrize("case", ac.PARAMS, ids=ac.case_id)
def test_form_at_its_bounds(probe, case):
    name, q = case
    ac.CASES[name][0](probe.run, q)


def test_the_table_covers_every_kernel_of_the_probe(probe):
    seen = set()

    def spy(op, *a, **k):
        seen.add(op)
        return probe.run(op, *a, **k)
    for name, (fn, moduli) in ac.CASES.items():
        fn(spy, moduli[-1])
    assert seen == set(probe.ops())


def test_the_makefile_states_the_products_flags():
    """build() passes HIP_FLAGS to the probe's Makefile; a bare `make` must compile the device probe the same way"""
    import __graft_entry__ as ge
    mk = open(os.path.join(ac.PROBE_DIR, "Makefile")).read()
    assert re.search(r"^HIP_FLAGS \?= (.*)$", mk, re.M).group(1).split() == ge.HIP_FLAGS


# ---- the checkers against wrong answers
def corrupted(run, change, only=None):
    """the probe's run with output 0 of every launch (of operation `only`) altered at three places by change(r, params)"""
    def bad(op, params, ins, **k):
        outs = run(op, params, ins, **k)
        if only is None or op == only:
            for j in (0, len(outs[0]) // 2, len(outs[0]) - 1):
                outs[0][j] = change(outs[0][j], params) & ac.M64
        return outs
    return bad


@pytest.mark.parametrize("case", ac.PARAMS, ids=ac.case_id)
def test_checker_rejects_a_result_off_by_one(probe, case):
    """r + 1 (an fp64 result: one ulp up): every case must notice. hc_mulhi_lo2 may be short by up to 2, so there the wrong answer is r + 3"""
    name, q = case
    with pytest.raises(AssertionError):
        ac.CASES[name][0](corrupted(probe.run, lambda r, p: r + (3 if name == "mulhi_lo2" else 1)), q)


# operation -> the multiple of q its results must stay below (the fp64 forms: in magnitude)
BOUNDS = {"shoup4": 4, "mul_shoup_lazy": 2, "mul_shoup": 1, "mont_lazy": 2, "canon4": 1, "canon8": 1, "reduce64": 1, "mont": 1, "mont_redc": 1, "lazy_fwd_alt": 8, "lazy_fwd2_alt": 8,
          "lazy_inv2": 4, "ct_round4_free": 70, "ct_round4_alt": 8, "gs_round": 4, "gs_round_last": 4, "mul32": 1, "gs_round32": 1}
CASE_OF = {"mul_shoup_lazy": "mul_shoup", "canon4": "canon", "canon8": "canon", "lazy_fwd2_alt": "lazy_fwd_alt", "lazy_inv2": "lazy_inv", "gs_round_last": "gs_round"}


@pytest.mark.parametrize("op", sorted(BOUNDS))
def test_checker_rejects_a_congruent_result_outside_the_bound(probe, op):
    """r + k q, the smallest that leaves [0, bound): still congruent, so only the bound check can refuse it"""
    name = CASE_OF.get(op, op)
    q = max(m for m in ac.CASES[name][1] if (BOUNDS[op] + 1) * m <= ac.M64)        # the wrong answer must fit 64 bits
    b = BOUNDS[op] * q
    with pytest.raises(AssertionError):
        ac.CASES[name][0](corrupted(probe.run, lambda r, p: r + q * -((r - b) // q), only=op), q)


@pytest.mark.parametrize("op,name", [("f64_mulmod", "f64_mulmod"), ("f64_reduce", "f64_reduce"), ("gs_round_f64", "gs_round_f64"), ("gs_round_f64_last", "gs_round_f64")])
def test_checker_rejects_an_fp64_result_moved_by_q(probe, op, name):
    """r +- q away from zero: an exact integer, still congruent, outside |r| < q (hc_f64_reduce: outside q/2 + 1)"""
    q = ac.MF64[-1]

    def move(bits, p):
        r = ac.u2d([bits])[0]
        return ac.d2u([r + q if r >= 0 else r - q])[0]
    with pytest.raises(AssertionError):
        ac.CASES[name][0](corrupted(probe.run, move, only=op), q)


def test_checker_rejects_one_ulp_at_the_largest_fp64_product(probe):
    """hc_f64_mulmod at |x| = 2^51 - 1, w = q - 1: one ulp down is no integer any more or breaks the congruence"""
    q = ac.MF64[-1]
    with pytest.raises(AssertionError):
        ac.case_f64_mulmod(corrupted(probe.run, lambda r, p: r - 1, only="f64_mulmod"), q)
