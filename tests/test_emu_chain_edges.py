"""The leveled entry points on chains the product does not build (tests/parity_cases.py, CHAINS): limbs 0 and 1 below 2^31, moduli at the top of the 32-bit class and just
above it, a 20-bit modulus, moduli either side of 2^32, 2^49, 2^57 and 2^58, a small special prime, a context of one modulus - under every setting of the options that choose
a row width or a transform body (pack32, small32, small_mm_wgs), with uniform rows, with rows of extreme residues, and with inputs planted on Rescale's rounding point and on
the edges of the basis extension's overflow count. The kernel sources run under the fibre emulator (tests/test_emu_parity.py says what that does and does not show);
tests/test_gpu_a_chain_edges.py runs the same cases on the device. Everything is exact equality with the oracle."""
import subprocess

import pytest

import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import Oracle
from test_emu_parity import EMU_DIR, EMU_LIB

ALL_CHAINS = ["small01", "small0", "allsmall", "edges", "edges2", "sizes", "one"]
mo = lambda Q, P: Oracle(q=Q, p=P)


@pytest.fixture(scope="module", autouse=True)
def emulator():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])


def maker(pack32=1, small32=1, wgs=None, lib_path=EMU_LIB):
    """make_ctx of the parity cases under the given options; every context it makes is also held to the table above hc_pk: HcMod::row32 of each of its limbs"""
    def mk(Q, P):
        ctx = Context(Q, P, **({"lib_path": lib_path} if lib_path else {}))
        ctx.set_option("pack32", pack32); ctx.set_option("small32", small32)
        if wgs is not None:
            ctx.set_option("small_mm_wgs", wgs)
        assert ctx.row32() == pc.expected_row32((Q, P), pack32), f"row32 of Q={[hex(q) for q in Q]} under pack32={pack32}"
        assert [bool(ctx.L.hc_row_is32(ctx.h, len(Q) + j)) for j in range(len(P))] == [pack32 == 2 and p < 1 << 31 and len(Q) + j >= 2 for j, p in enumerate(P)]
        return ctx
    return mk


def key_switch_shapes(chain):
    """(level, alpha) of case_keyswitch_general on a chain: its top level, and level 1 - limbs 0 and 1 alone, as one digit or two"""
    Q, P = chain
    return ((len(Q) - 1, len(P)), (1, len(P)))


@pytest.mark.parametrize("wgs", [0, 1 << 30], ids=["tiles16", "quarter"])
@pytest.mark.parametrize("small32", [0, 1])
@pytest.mark.parametrize("pack32", [0, 1, 2])
@pytest.mark.parametrize("name", ALL_CHAINS)
def test_leveled_entry_points_and_key_switch(name, pack32, small32, wgs):
    """every leveled entry point row by row, and the key switch at the top level and at level 1, on each chain under each setting. The chains whose limb 0 or 1 is below 2^31
    are the ones on which the batched transforms once read 4-byte rows where hc_row32 says 8-byte rows (pack32 = 2).
    Cost, accepted: 84 cases of 3 to 8 s on the emulator, about 7 minutes. The full product is kept on purpose, also where an option should change nothing (small32 on `sizes`,
    which has no modulus below 2^31): that an option changes nothing there is a property of the host's dispatch that only running it shows."""
    chain, mk = pc.CHAINS[name], maker(pack32, small32, wgs)
    pc.case_leveled_rows(mk, mo, chain=chain)
    if chain[1]:
        pc.case_keyswitch_general(mk, mo, shapes=key_switch_shapes(chain), chain=chain)
    else:
        ctx = mk(*chain)            # hc_ctx_create accepts a chain without special primes; there is no key switch to run on it
        assert ctx.row32() == [pack32 == 2]
        ctx.close()


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("name", ["small01", "edges", "edges2"])
def test_hoisted_and_qp_entry_points(name, pack32):
    chain, mk = pc.CHAINS[name], maker(pack32)
    pc.case_keyswitch_hoisted(mk, mo, chain=chain)
    pc.case_keyswitch_qp_mod_down(mk, mo, chain=chain)


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("name", ["small01", "edges"])
def test_batched_entry_points(name, pack32):
    """three images per launch: row widths that differ per limb (pack32 = 2), image strides and small limbs 0 and 1 together"""
    chain = pc.CHAINS[name]
    pc.case_batched_leveled(maker(pack32), n=3, level=len(chain[0]) - 1, alpha=len(chain[1]), make_oracle=mo, chain=chain)


# Rescale with a small last limb and with a large one: the top level and one below it whose last limb is of the other class; level 1 is hc_div_round_last_n's branch of its
# own, which reads limbs 0 and 1 as 8-byte rows - on small01 they are below 2^31
ROUNDING_LEVELS = {"small01": (3, 2, 1), "edges": (5, 3), "edges2": (5, 1)}


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("name", ["small01", "edges", "edges2"])
def test_rescale_at_the_rounding_point(name, pack32):
    pc.case_rescale_rounding_point(maker(pack32), mo, pc.CHAINS[name], ROUNDING_LEVELS[name])


ALPHA5 = (pc.Q_MIX, pc.P_CHAIN)       # digits of five limbs and of two: v = 0 .. 4


@pytest.mark.parametrize("pack32", [1, 2])
@pytest.mark.parametrize("chain", [pc.CHAIN_SMALL01, pc.CHAIN_EDGES, pc.CHAIN_EDGES2, ALPHA5], ids=["small01", "edges", "edges2", "alpha5"])
def test_basis_extension_at_the_edges_of_the_overflow_count(chain, pack32):
    pc.case_basis_ext_edges(maker(pack32), mo, chain)


@pytest.mark.parametrize("pack32", [0, 1, 2])
@pytest.mark.parametrize("name", ["edges", "edges2", "allsmall"])
def test_rows_of_extreme_residues(name, pack32):
    """every operand row, key rows included, all 0, all q-1, alternating or one of edge_rows(q): what the lazy sums of the inner products, the 4-byte seam and Rescale see at most"""
    chain, mk = pc.CHAINS[name], maker(pack32)
    pc.case_leveled_rows(mk, mo, chain=chain, rows="edge")
    pc.case_keyswitch_general(mk, mo, shapes=key_switch_shapes(chain), chain=chain, rows="edge")
    pc.case_keyswitch_qp_mod_down(mk, mo, chain=chain, rows="edge")
