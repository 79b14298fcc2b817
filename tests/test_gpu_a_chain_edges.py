"""The cases of tests/test_emu_chain_edges.py on libhconv.so and a real MI355X: the leveled entry points on chains whose limb 0 or 1 is below 2^31, whose moduli sit at the
top of the 32-bit class, just above it, at 20 bits and either side of 2^32, 2^49, 2^57 and 2^58, under every setting of pack32, small32 and small_mm_wgs; rows of extreme
residues; inputs planted on Rescale's rounding point and on the edges of the basis extension's overflow count. The emulator shows that the sources index and exchange
correctly; only this file shows what gfx950 computes with them. Exact equality with the oracle, which runs beside the device."""
import os

import pytest

import parity_cases as pc
from oracle_lib import Oracle
from test_emu_chain_edges import ALL_CHAINS, ALPHA5, ROUNDING_LEVELS, key_switch_shapes, maker

pytestmark = pytest.mark.gpu


class _Kept:
    """a context the cases may close: it stays open, back at one image per call, for the next test with the same chain and options"""

    def __init__(self, ctx):
        self.__dict__["_ctx"] = ctx

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def close(self):
        self._ctx.set_batch(1)


@pytest.fixture(scope="module")
def contexts():
    """make_ctx(pack32, small32, wgs) -> the cases' make_ctx(Q, P): one context per (whole chain, options), shared by the tests that use it, and one oracle per chain.
    At most KEEP contexts are alive: the least recently used one is closed (tables, workspaces and keys freed) when another is made - the six (chain, pack32) pairs that
    the tests after the first share, and a few of the first test's, each of which is used once. A context over a part of a chain (the key switch at level 1) is not kept:
    the case that made it closes it."""
    from optimal_conv_amd import abi
    assert os.path.exists(abi.DEFAULT_LIB), "libhconv.so missing: run __graft_entry__.build() (no CPU fallback exists)"
    KEEP = 8
    made, oracles = {}, {}
    whole = {(tuple(Q), tuple(P)) for Q, P in list(pc.CHAINS.values()) + [ALPHA5]}

    def make_ctx(pack32=1, small32=1, wgs=None):
        fresh = maker(pack32, small32, wgs, lib_path=None)

        def mk(Q, P):
            if (tuple(Q), tuple(P)) not in whole:
                return fresh(Q, P)
            key = (tuple(Q), tuple(P), pack32, small32, wgs)
            ctx = made.pop(key) if key in made else fresh(Q, P)
            made[key] = ctx                              # most recently used last
            while len(made) > KEEP:
                made.pop(next(iter(made))).close()
            return _Kept(ctx)
        return mk

    def make_oracle(Q, P):
        key = (tuple(Q), tuple(P))
        if key not in oracles:
            oracles[key] = Oracle(q=Q, p=P)
        return oracles[key]
    yield make_ctx, make_oracle
    for ctx in made.values():
        ctx.close()


@pytest.mark.parametrize("wgs", [0, 1 << 30], ids=["tiles16", "quarter"])
@pytest.mark.parametrize("small32", [0, 1])
@pytest.mark.parametrize("pack32", [0, 1, 2])
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_leveled_entry_points_and_key_switch(contexts, name, pack32, small32, wgs):
    make_ctx, mo = contexts
    chain, mk = pc.CHAINS[name], make_ctx(pack32, small32, wgs)
    pc.case_leveled_rows(mk, mo, chain=chain)
    if chain[1]:
        pc.case_keyswitch_general(mk, mo, shapes=key_switch_shapes(chain), chain=chain)


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("name", ["small01", "edges", "edges2"])
def test_hoisted_and_qp_entry_points(contexts, name, pack32):
    make_ctx, mo = contexts
    chain, mk = pc.CHAINS[name], make_ctx(pack32)
    pc.case_keyswitch_hoisted(mk, mo, chain=chain)
    pc.case_keyswitch_qp_mod_down(mk, mo, chain=chain)


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("name", ["small01", "edges", "edges2"])
def test_batched_entry_points(contexts, name, pack32):
    make_ctx, mo = contexts
    chain = pc.CHAINS[name]
    pc.case_batched_leveled(make_ctx(pack32), n=3, level=len(chain[0]) - 1, alpha=len(chain[1]), make_oracle=mo, chain=chain)


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("name", ["small01", "edges", "edges2"])
def test_rescale_at_the_rounding_point(contexts, name, pack32):
    make_ctx, mo = contexts
    pc.case_rescale_rounding_point(make_ctx(pack32), mo, pc.CHAINS[name], ROUNDING_LEVELS[name])


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("chain", [pc.CHAIN_SMALL01, pc.CHAIN_EDGES, pc.CHAIN_EDGES2, ALPHA5], ids=["small01", "edges", "edges2", "alpha5"])
def test_basis_extension_at_the_edges_of_the_overflow_count(contexts, chain, pack32):
    make_ctx, mo = contexts
    pc.case_basis_ext_edges(make_ctx(pack32), mo, chain)


@pytest.mark.parametrize("pack32", [0, 1, 2])
@pytest.mark.parametrize("name", ["edges", "edges2", "allsmall"])
def test_rows_of_extreme_residues(contexts, name, pack32):
    make_ctx, mo = contexts
    chain, mk = pc.CHAINS[name], make_ctx(pack32)
    pc.case_leveled_rows(mk, mo, chain=chain, rows="edge")
    pc.case_keyswitch_general(mk, mo, shapes=key_switch_shapes(chain), chain=chain, rows="edge")
    pc.case_keyswitch_qp_mod_down(mk, mo, chain=chain, rows="edge")
