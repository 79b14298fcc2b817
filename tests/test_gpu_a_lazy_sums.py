"""The cases of tests/test_lazy_sums_cpu.py on a real MI355X: the lazy sums of hc_qp_mul_sum*, hc_lv_lincomb2 and hc_lv_mul_sum through libhconv.so, and hc_k_ks_mac_all and
hc_k_ks_mac_multi launched directly by the device build of tests/arith_probe/sum_probe.hip (hipcc, the product's flags; build() makes it), at the term counts where a reduction
group closes and with the operands planted so that every group reaches count (q - 1)^2. The emulator shows that the sources' periods and phases are right; only this file shows
what gfx950 computes with them - the 128-bit adds, the multiply-add chain into a 64-bit sum, the unrolled accumulator arrays. Exact equality with Python's integers."""
import os

import pytest

import lazy_sum_cases as lz
from oracle_lib import P0, Q0, Q1

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(lz.DEVICE_LIB), f"{lz.DEVICE_LIB} is missing: __graft_entry__.build() makes it"
    return lz.SumProbe(lz.DEVICE_LIB)


@pytest.fixture(scope="module", params=[1, 2], ids=["pack32=1", "pack32=2"])
def leveled(request):
    from optimal_conv_amd import Context, abi
    assert os.path.exists(abi.DEFAULT_LIB), "libhconv.so missing: run __graft_entry__.build() (no CPU fallback exists)"
    ctx = Context(lz.CTX_Q, lz.CTX_P)
    ctx.set_option("pack32", request.param)
    assert ctx.row32() == [False, False, False, request.param == 2, request.param == 2]
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = {"qp": lz.QpSums, "lin": lz.LinComb}[kind](ctx)
        return made[kind]
    yield get
    for m in made.values():
        m.free()
    ctx.close()


@pytest.mark.parametrize("case", lz.MAC_ALL_PARAMS, ids=lz.mac_all_id)
def test_ks_mac_all(probe, case):
    triple, rowsel, beta, NB, n = case
    lz.case_mac_all(probe, triple, rowsel, beta, NB, n)


@pytest.mark.parametrize("case", lz.MAC_ALL_PREP_PARAMS, ids=lz.mac_all_id)
def test_ks_mac_all_with_prep(probe, case):
    triple, rowsel, beta, NB, n, prep = case
    lz.case_mac_all(probe, triple, rowsel, beta, NB, n, prep=prep)


@pytest.mark.parametrize("case", lz.MAC_MULTI_PARAMS, ids=lz.mac_multi_id)
def test_ks_mac_multi(probe, case):
    triple, rowsel, beta, shape = case
    lz.case_mac_multi(probe, triple, rowsel, beta, shape)


@pytest.mark.parametrize("case", lz.MAC_MULTI_FORCED, ids=lz.mac_multi_id)
def test_ks_mac_multi_lazy_forced_either_way(probe, case):
    triple, rowsel, beta, shape, lazy = case
    lz.case_mac_multi(probe, triple, rowsel, beta, shape, lazy=bool(lazy))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nterms", lz.QP_COUNTS)
def test_qp_mul_sum(leveled, nterms, accumulate):
    leveled("qp").run(nterms, [list(range(nterms))], [accumulate])


@pytest.mark.parametrize("case", lz.QP_G_PARAMS, ids=lambda p: f"G{p[0]}-terms{p[1]}-{p[2]}")
def test_qp_mul_sum_giant_steps(leveled, case):
    G, nterms, variant = case
    leveled("qp").run(nterms, lz.qp_plan(G, nterms, variant), [(h + (variant == "edges")) % 2 for h in range(G)])


@pytest.mark.parametrize("case", lz.QP_BATCH_PARAMS, ids=lambda p: f"G{p[0]}-terms{p[1]}")
def test_qp_mul_sum_giant_steps_on_three_images(leveled, case):
    G, nterms = case
    leveled("qp").run(nterms, lz.qp_plan(G, nterms, "edges" if nterms != 8 else "nullgroup"), [h % 2 for h in range(G)], n=3)


@pytest.mark.parametrize("case", lz.LIN_PARAMS, ids=lambda p: f"terms{p[0]}-{p[1]}-" + ("addc" if p[2] else "noaddc"))
def test_lv_lincomb2(leveled, case):
    nterms, consts, addc = case
    leveled("lin").run(nterms, consts, addc)


def test_lv_lincomb2_into_its_first_term(leveled):
    leveled("lin").run(8, "max", True, alias=True)
    leveled("lin").run(8, "max", True)


@pytest.fixture(scope="module")
def conv_ctx():
    from optimal_conv_amd import Context
    ctx = Context([Q0, Q1], [P0])
    yield ctx
    ctx.close()


@pytest.mark.parametrize("ntaps", [1, 2, 63, 64])
def test_lv_mul_sum(conv_ctx, ntaps):
    lz.case_lv_mul_sum(conv_ctx, ntaps)
