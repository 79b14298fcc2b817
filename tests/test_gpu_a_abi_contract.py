"""tests/abi_contract_cases.py on libhconv.so and a real MI355X: the full product of Part A - every intruder of the table between hc_keyswitch_decompose and every hoisted
consumer, on both chains (alpha 3: two digits; alpha 2: three, hc_k_ks_mac_multi's lazy form), pack32 1 and 2, one image and three -, the placements of Part B with the two
polynomials of a pair in descending, mixed and more-than-4-GiB-apart order, and the aliased forms the header permits; every call inside an arena whose words outside the
call's documented footprint are compared with a host shadow (Part C). Exact equality with the same entry point in its plain form, which tests/test_gpu_a_parity.py and
tests/test_gpu_a_chain_edges.py hold to the oracle; the plain hoisted key switch is held to the oracle here as well."""
import os

import pytest

import abi_contract_cases as ab
from oracle_lib import Oracle
from test_emu_chain_edges import maker

pytestmark = pytest.mark.gpu
LEVEL = 4
_oracles = {}


def mo(Q, P):
    key = (tuple(Q), tuple(P))
    if key not in _oracles:
        _oracles[key] = Oracle(q=Q, p=P)
    return _oracles[key]


def make_ctx(pack32):
    def mk(Q, P, async_alloc=0):
        from optimal_conv_amd import Context, abi
        assert os.path.exists(abi.DEFAULT_LIB), "libhconv.so missing: run __graft_entry__.build() (no CPU fallback exists)"
        if async_alloc:                                   # only right after hc_ctx_create
            ctx = Context(Q, P)
            ctx.set_option("async_alloc", async_alloc); ctx.set_option("pack32", pack32)
        else:
            ctx = maker(pack32, lib_path=None)(Q, P)
        ctx.wgs0 = 1024                                   # the library's small_mm_wgs
        return ctx
    return mk


@pytest.fixture(scope="module")
def envs():
    """Part A environments by (alpha, pack32, n) - a context, its keys, its arena -, one alive at a time: the tests are ordered so that each is made once"""
    made = {}

    def get(alpha, pack32, n):
        if (alpha, pack32, n) not in made:
            for E in made.values():
                E.close(); E.ctx.close()
            made.clear()
            made[(alpha, pack32, n)] = ab.part_a_env(make_ctx(pack32)(*ab.chain(LEVEL, alpha)), LEVEL, n)
        return made[(alpha, pack32, n)]
    yield get
    for E in made.values():
        E.close(); E.ctx.close()


def test_every_entry_point_is_an_intruder_or_excluded_with_a_reason():
    ab.check_table_is_complete()


@pytest.mark.parametrize("part", range(ab.INTRUDER_PARTS))
@pytest.mark.parametrize("consumer", list(ab.CONSUMERS))
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("alpha", [3, 2])
def test_held_decomposition_under_every_intruder(envs, alpha, pack32, n, consumer, part):
    """the table in INTRUDER_PARTS interleaved parts: a case is about thirty sequences, each ending in one download and comparison of the whole arena"""
    ab.case_held_decomposition(envs(alpha, pack32, n), consumer, ab.intruder_part(part), make_oracle=mo)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("alpha", [3, 2])
def test_another_pointer_or_another_level_is_refused(envs, alpha, pack32, n):
    ab.case_wrong_pointer_or_level(envs(alpha, pack32, n))


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("alpha", [3, 2])
def test_scratch_that_grows_or_changes_layout_under_a_held_decomposition(alpha, pack32):
    ab.case_scratch_growth(make_ctx(pack32), LEVEL, alpha)


@pytest.mark.parametrize("pack32", [1, 2])
def test_freed_and_recycled_polynomial_is_not_taken_for_the_held_one(pack32):
    ab.case_freed_and_recycled(make_ctx(pack32), LEVEL, 3)


@pytest.fixture(scope="module")
def placed():
    """Part B environments by (alpha, pack32, n, far), one alive at a time"""
    made = {}

    def get(alpha, pack32, n, far=False):
        key = (alpha, pack32, n, far)
        if key not in made:
            for E, dist in made.values():
                E.close(); E.ctx.close()
            made.clear()
            ctx = make_ctx(pack32)(*ab.chain(LEVEL, alpha))
            made[key] = ab.far_env(ctx, LEVEL, n) if far else (ab.part_b_env(ctx, LEVEL, n), 0)
        return made[key]
    yield get
    for E, dist in made.values():
        E.close(); E.ctx.close()


@pytest.mark.parametrize("name", ab.PLACEMENT_OPS)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("alpha", [3, 2])
def test_placement_of_the_two_polynomials(placed, alpha, pack32, n, name):
    ab.case_placement(placed(alpha, pack32, n)[0], name)


@pytest.mark.parametrize("name", ab.PLACEMENT_OPS)
@pytest.mark.parametrize("n", [1, 3])
def test_polynomials_more_than_4_gib_apart(placed, n, name):
    E, dist = placed(3, 2, n, far=True)
    print(f"far layout: {dist} bytes between the windows")
    assert dist > 1 << 32, f"the arena of the far layout could only be {dist} bytes long on this device"
    ab.case_placement(E, name, layouts=("far",))


@pytest.mark.parametrize("name,alias", ab.ALIASED, ids=[f"{a}-{'+'.join(f'{x}={y}' for x, y in m.items())}" for a, m in ab.ALIASED])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("pack32", [1, 2])
def test_permitted_aliasing(placed, pack32, n, name, alias):
    ab.case_aliased(placed(3, pack32, n)[0], name, alias)


def test_keyswitch_rotate_refuses_outputs_on_inputs(placed):
    ab.case_keyswitch_rotate_refuses_aliasing(placed(3, 2, 3)[0])


def test_rotate_gal_l0_in_place():
    ab.case_rotate_gal_l0_in_place(make_ctx(1))
