"""tests/abi_contract_cases.py on the fibre emulator: a held decomposition under every intruder of the table (the plain hoisted key switch and the fused baby steps as
consumers; one image, pack32 = 2, alpha 3), the settled lists also on three images and with every consumer, the placements and the permitted aliasings of the pair entry
points, all inside the arena whose every word outside a call's documented footprint is checked. tests/test_gpu_a_abi_contract.py runs the full product on the device.
The emulator shows what the host code and the kernels' indexing do; a 4 GiB distance is within its reach too (untouched pages of the arena's middle are never mapped)."""
import subprocess

import pytest

import abi_contract_cases as ab
from test_emu_chain_edges import maker, mo
from test_emu_parity import EMU_DIR, EMU_LIB

LEVEL = 4


@pytest.fixture(scope="module", autouse=True)
def emulator():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])


def make_ctx(pack32):
    def mk(Q, P, async_alloc=0):
        from optimal_conv_amd import Context
        if async_alloc:                                   # only right after hc_ctx_create
            ctx = Context(Q, P, lib_path=EMU_LIB)
            ctx.set_option("async_alloc", async_alloc); ctx.set_option("pack32", pack32)
        else:
            ctx = maker(pack32)(Q, P)
        ctx.wgs0 = 0                                      # the emulated library's small_mm_wgs
        return ctx
    return mk


@pytest.fixture(scope="module")
def envs():
    """Part A environments by (alpha, pack32, n): a context, its keys, its arena; made at first use, closed with the module"""
    made = {}

    def get(alpha, pack32, n):
        if (alpha, pack32, n) not in made:
            made[(alpha, pack32, n)] = ab.part_a_env(make_ctx(pack32)(*ab.chain(LEVEL, alpha)), LEVEL, n)
        return made[(alpha, pack32, n)]
    yield get
    for E in made.values():
        E.close(); E.ctx.close()


def test_every_entry_point_is_an_intruder_or_excluded_with_a_reason():
    ab.check_table_is_complete()
    one_less = {k: v for k, v in ab.INTRUDERS.items() if v[0] != "hc_lv_mod_raise"}
    with pytest.raises(AssertionError, match="hc_lv_mod_raise"):
        ab.check_table_is_complete(one_less)


@pytest.mark.parametrize("consumer", ["hoisted", "rotate_many"])
def test_held_decomposition_under_every_intruder(envs, consumer):
    """Cost, accepted: the whole table, about a minute per consumer"""
    ab.case_held_decomposition(envs(3, 2, 1), consumer, make_oracle=mo)


@pytest.mark.parametrize("consumer", ["hoisted", "rotate_many"])
def test_settled_outcomes_on_three_images(envs, consumer):
    ab.case_held_decomposition(envs(3, 2, 3), consumer, sorted(ab.MUST_SURVIVE | ab.MUST_REFUSE))


@pytest.mark.parametrize("consumer", ["rotate", "qp", "qp_rotate", "qp_rotate_acc"])
def test_settled_outcomes_with_the_other_consumers(envs, consumer):
    ab.case_held_decomposition(envs(3, 2, 1), consumer, sorted(ab.MUST_SURVIVE | ab.MUST_REFUSE))


def test_settled_outcomes_with_three_digits(envs):
    """alpha = 2: beta = 3, hc_k_ks_mac_multi's lazy instantiation"""
    ab.case_held_decomposition(envs(2, 1, 1), "rotate_many", sorted(ab.MUST_SURVIVE | ab.MUST_REFUSE))


def test_another_pointer_or_another_level_is_refused(envs):
    ab.case_wrong_pointer_or_level(envs(3, 2, 1))


def test_scratch_that_grows_or_changes_layout_under_a_held_decomposition():
    ab.case_scratch_growth(make_ctx(2), LEVEL, 3)


def test_freed_and_recycled_polynomial_is_not_taken_for_the_held_one():
    ab.case_freed_and_recycled(make_ctx(2), LEVEL, 3)


@pytest.fixture(scope="module")
def placed():
    made = {}

    def get(n, far):
        if (n, far) not in made:
            ctx = make_ctx(2)(*ab.chain(LEVEL, 3))
            made[(n, far)] = ab.far_env(ctx, LEVEL, n) if far else (ab.part_b_env(ctx, LEVEL, n), 0)
        return made[(n, far)]
    yield get
    for E, dist in made.values():
        E.close(); E.ctx.close()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", ab.PLACEMENT_OPS)
def test_placement_of_the_two_polynomials(placed, name, n):
    E, _ = placed(n, False)
    ab.case_placement(E, name)


@pytest.mark.parametrize("name", ab.PLACEMENT_OPS)
def test_polynomials_more_than_4_gib_apart(placed, name):
    E, dist = placed(3, True)
    assert dist > 1 << 32, f"the arena of the far layout could only be {dist} bytes long"
    ab.case_placement(E, name, layouts=("far",))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name,alias", ab.ALIASED, ids=[f"{a}-{'+'.join(f'{x}={y}' for x, y in m.items())}" for a, m in ab.ALIASED])
def test_permitted_aliasing(placed, name, alias, n):
    E, _ = placed(n, False)
    ab.case_aliased(E, name, alias)


def test_keyswitch_rotate_refuses_outputs_on_inputs(placed):
    ab.case_keyswitch_rotate_refuses_aliasing(placed(3, False)[0])


def test_rotate_gal_l0_in_place():
    ab.case_rotate_gal_l0_in_place(make_ctx(1))
