"""hc_prep_ker_fc under the held-decomposition contract of tests/abi_contract_cases.py: its row in the INTRUDERS table, and the sequence decompose; hc_prep_ker_fc; consumer
with every hoisted consumer, on the fibre emulator and on the device.

The row is placed from here, when this module is imported. pytest imports every test module of a run before it runs the first test, so in any run that collects this file
next to tests/test_emu_abi_contract.py / tests/test_gpu_a_abi_contract.py their completeness check sees the entry point placed. Those two files run ALONE report
hc_prep_ker_fc as unplaced: run them with this file (or the whole directory). The row belongs beside `prep_ker_ex2` in the table itself; a change that edits that file
should move it there and delete the three lines below."""
import subprocess

import numpy as np
import pytest

import abi_contract_cases as ab
from test_emu_parity import EMU_DIR, EMU_LIB

LEVEL = 4


def _prep_ker_fc(E):
    k = E.ctx.prep_ker_fc(np.linspace(-1, 1, 4 * 4), np.ones(4), 16, 3, 4, 4)
    E.ctx.ker_free(k)


ab.INTRUDERS.setdefault("prep_ker_fc", ("hc_prep_ker_fc", _prep_ker_fc))


def test_the_row_is_placed_and_the_table_complete():
    assert ab.INTRUDERS["prep_ker_fc"][0] == "hc_prep_ker_fc" and "hc_prep_ker_fc" in ab.declared_entry_points()
    ab.check_table_is_complete()
    without = {k: v for k, v in ab.INTRUDERS.items() if k != "prep_ker_fc"}
    with pytest.raises(AssertionError, match="hc_prep_ker_fc"):
        ab.check_table_is_complete(without)


def _run(E):
    """the same rule as for hc_prep_ker / _ex / _ex2 (their rows run in the table's own tests): whatever the consumer answers, HC_OK comes with the right words
    (sequence() compares them) and a refusal is HC_ERR_STATE with untouched outputs; and the new call answers as its siblings do"""
    for consumer in ab.CONSUMERS:
        got = ab.case_held_decomposition(E, consumer, ["prep_ker_fc", "prep_ker_ex2", "prep_ker"])
        assert set(got.values()) <= {ab.HC_OK, ab.HC_ERR_STATE}, (consumer, got)
        assert got["prep_ker_fc"] == got["prep_ker_ex2"] == got["prep_ker"], (consumer, got)


def test_held_decomposition_with_hc_prep_ker_fc_between_emulated():
    from test_emu_abi_contract import make_ctx
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    E = ab.part_a_env(make_ctx(2)(*ab.chain(LEVEL, 3)), LEVEL, 1)
    try:
        _run(E)
    finally:
        E.close(); E.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
def test_held_decomposition_with_hc_prep_ker_fc_between_on_device(n):
    from test_gpu_a_abi_contract import make_ctx
    E = ab.part_a_env(make_ctx(2)(*ab.chain(LEVEL, 3)), LEVEL, n)
    try:
        _run(E)
    finally:
        E.close(); E.ctx.close()
