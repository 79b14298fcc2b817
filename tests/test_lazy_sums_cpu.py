"""The lazy sums of the inner products at their term counts and extremes (tests/lazy_sum_cases.py) on the EMULATOR builds: hc_qp_mul_sum*, hc_lv_lincomb2 and hc_lv_mul_sum
through the C ABI of libhconv_emu.so, hc_k_ks_mac_all and hc_k_ks_mac_multi launched directly by the host twin of tests/arith_probe/sum_probe.hip. This says that the reduction
periods and phase boundaries of the sources are right at the operands where their bounds are tight; what hipcc makes of them for gfx950 is tests/test_gpu_a_lazy_sums.py's
question. The last tests feed the checkers wrong answers - r + 1, and what a kernel with an overlong reduction period would return - so a checker that accepts everything fails."""
import subprocess

import numpy as np
import pytest

import lazy_sum_cases as lz
from optimal_conv_amd import Context
from oracle_lib import P0, Q0, Q1
from test_emu_parity import EMU_DIR, EMU_LIB


@pytest.fixture(scope="module")
def probe():
    return lz.SumProbe(lz.build_host_twin())


@pytest.fixture(scope="module")
def emulator():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    return EMU_LIB


@pytest.fixture(scope="module", params=[1, 2], ids=["pack32=1", "pack32=2"])
def leveled(request, emulator):
    """the context of section 2 under one pack32 setting, with the operands of the diagonal sums and of the linear combination built once"""
    ctx = Context(lz.CTX_Q, lz.CTX_P, lib_path=emulator)
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


# ---- section 3: the key switch's inner products
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


def test_the_probe_refuses_what_the_host_cannot_launch(probe):
    """an (R, NB) or NB outside the host's dispatch, more images than one group of hc_k_ks_mac_multi holds, a buffer smaller than the shape: -1 before any launch"""
    one = np.zeros(1, dtype=np.uint64)
    assert probe.L.sum_probe_mac_all(3, one.ctypes.data, 3, 2, 2, 3, 1, 1, 1, *([one.ctypes.data, 1] + [one.ctypes.data, 1, 1] * 3), None, None, 0, 0, 0, 0) == -1
    assert probe.L.sum_probe_mac_all(1, one.ctypes.data, 3, 2, 2, 3, 1, 1, 1, *([one.ctypes.data, 1] + [one.ctypes.data, 1, 1] * 3), None, None, 0, 0, 0, 0) == -1
    assert probe.L.sum_probe_mac_multi(4, 2, 0, 0, one.ctypes.data, 3, 2, 2, 3, 1, 1, 1, 1, *([one.ctypes.data, 1, 1] * 3 + [one.ctypes.data, 1, 1, 1]), None, None, 0, 0, 0) == -1
    assert probe.L.sum_probe_mac_multi(8, 1, 0, 0, one.ctypes.data, 3, 2, 2, 3, 1, 1, 2, 1, *([one.ctypes.data, 1, 1] * 3 + [one.ctypes.data, 1, 1, 1]), None, None, 0, 0, 0) == -1


# ---- section 2: the sums behind the C ABI
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
    leveled("lin").run(8, "max", True)              # and the operands are as they were


@pytest.fixture(scope="module")
def conv_ctx(emulator):
    ctx = Context([Q0, Q1], [P0], lib_path=emulator)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("ntaps", [1, 2, 63, 64])
def test_lv_mul_sum(conv_ctx, ntaps):
    lz.case_lv_mul_sum(conv_ctx, ntaps)


# ---- the checkers against wrong answers
def plus_one(where):
    def tamper(a):
        a[where] += np.uint64(1)
    return tamper


def test_checkers_reject_a_result_off_by_one(probe, leveled, conv_ctx):
    with pytest.raises(AssertionError, match="residues differ"):
        lz.case_mac_all(probe, "top32", (1, 0), 5, 2, 2, tamper=plus_one((1, 3 + 2, lz.N - 1)))                 # image 1, component 1, the P limb, the last coefficient
    with pytest.raises(AssertionError, match="residues differ"):
        lz.case_mac_multi(probe, "bits20", (0, 0), 7, (4, 4, 3, 4, 1, 1), tamper=plus_one((2, 3, 0, 0)))        # rotation 2, image 3, component 0, limb 0
    with pytest.raises(AssertionError, match="residues differ"):
        leveled("qp").run(8, [list(range(8))], [1], tamper=plus_one((0, 5 * lz.N + 77)))                           # image 0, component 0, the special prime's row
    with pytest.raises(AssertionError, match="residues differ"):
        leveled("lin").run(8, "max", True, tamper=plus_one((2, 1535)))
    with pytest.raises(AssertionError, match="residues differ"):
        lz.case_lv_mul_sum(conv_ctx, 2, tamper=plus_one((1, 4096)))


@pytest.mark.parametrize("triple", list(lz.TRIPLES))
def test_the_planted_columns_expose_an_overlong_period(triple):
    """what a kernel would return whose 64-bit sum took five products (the sum modulo 2^64 first) or whose 128-bit sum took nine or thirteen (past q 2^64, where hc_mont_redc's
    difference leaves (-q, q)) differs from the reference in the planted columns; the kernels' own periods and the provably safe ones (8 on 8-byte rows below 2^61) do not"""
    assert lz.case_mac_all(None, triple, (1, 0), 5, 1, 1, model=5) == (triple == "top32")          # PER = 5 on the 4-byte limb: overflows at the top of the class, not at 20 bits
    assert not lz.case_mac_all(None, triple, (1, 0), 5, 1, 1, model=4)
    assert not lz.case_mac_all(None, triple, (0, 0), 5, 1, 1, model=5)           # 8-byte rows throughout: five products are within the bound
    assert lz.case_mac_all(None, triple, (0, 0), 9, 1, 1, model=9)               # PER = 9 on the limb below 2^61
    assert not lz.case_mac_all(None, triple, (0, 0), 9, 1, 1, model=8)
    assert not lz.case_mac_all(None, triple, (0, 0), 13, 1, 1, model=6)


def test_check_rejects_the_overlong_sums_of_the_diagonal_and_linear_kernels():
    """a period of 10 in the diagonal sums, and a ninth term in the linear combination's single group, on the special prime just below 2^61. Both kernels join the reduced sum to
    a canonical word by hc_addmod - ONE conditional subtraction - which also repairs an hc_mont_redc result in [q, 2q) when that word is 0: what exposes the overlong sum is an
    accumulator (an addend) of q - 1, as the cases plant it"""
    q = lz.P_CHAIN[0]
    X, Y = lz.pattern(q, 13, 0xBAD)
    rinv = pow(lz.R64, -1, q)
    want = (q - 1 + sum(X[t] * Y[t] for t in range(13)) * rinv) % q
    lz.check(lz.row(lz.lazy_model(X, Y, q, 7, start=q - 1)), want, "period 7")
    lz.check(lz.row(lz.lazy_model(X, Y, q, 8, start=q - 1)), want, "period 8: safe below 2^61")
    for per, n in ((10, 13), (9, 9)):
        want = (q - 1 + sum(X[t] * Y[t] for t in range(n)) * rinv) % q
        with pytest.raises(AssertionError, match="classes"):
            lz.check(lz.row(lz.lazy_model(X[:n], Y[:n], q, per, start=q - 1)), want, f"period {per}")
