"""hc_k_a1p<1> / hc_k_a1g<1> with the fp64 product on 8-byte c' operands (hc_f64_mulmod_q; hc_k_ctc_pairs' dense limb-1 array), on the device, word for word against the oracle:
the batch of three and the grouped convolutions of tests/test_a1_fp64_product_cpu.py at max_ob = 4, hc_div_round_last on the same rows, and one convolution at max_ob = 2 whose
limb-1 rows hold every pair of operand extremes (k_1, c') at known coefficients - c' is reached through the input residue c' * cst^-1 mod Q1, cst being MultByConst's integer."""
import itertools

import numpy as np
import pytest

import multiconv_ref as MR
import parity_cases as pc
from optimal_conv_amd import Context
from oracle_lib import Q1
from test_a1_fp64_product_cpu import case_div_round_last_extremes, case_grouped_extremes, extremes
from test_operand_streams_cpu import BENCH_TRIPLE, INT_A1_TRIPLE, case_batch_of_three

pytestmark = pytest.mark.gpu
N = pc.N
S30 = 2.0 ** 30


def device(Q, P):
    return Context(Q, P)


def test_batch_of_three_fp64_product():
    case_batch_of_three(device, BENCH_TRIPLE, max_ob=4)


def test_batch_of_three_integer_path():
    case_batch_of_three(device, INT_A1_TRIPLE, max_ob=4)


@pytest.mark.parametrize("m", [2, 3])
def test_grouped_members_fp64_product(m):
    case_grouped_extremes(device, BENCH_TRIPLE, m)


def test_div_round_last_fp64_product():
    case_div_round_last_extremes(device, BENCH_TRIPLE)


def test_every_extreme_pair_planted_in_limb_1():
    """max_ob = 2. Coefficient 100 b + 10 i + j of both channels' k_1 is E[i]; there c'_0 = E[j] and c'_1 = E[(i + j) % 10], for b = 0 (the first tile's first rows) and at the
    end of the last tile; everything else is uniform."""
    max_ob, seed = 2, 0xA1E
    ctx, O = pc._triple_env(device, BENCH_TRIPLE)
    try:
        E = extremes(Q1)
        assert len(E) == 10
        cst1 = MR.setscale_consts(O, S30, S30, max_ob, 1, S30)[0][1] % Q1
        inv = pow(cst1, -1, Q1)
        ct_in, ker = pc.planted_conv_inputs(seed, max_ob, O)
        for base in (0, N - 100):
            for i, j in itertools.product(range(10), repeat=2):
                at = base + 10 * i + j
                ker[:, 1, at] = E[i]
                for p, c in ((0, E[j]), (1, E[(i + j) % 10])):
                    ct_in[p, 1, at] = c * inv % Q1
                    assert int(ct_in[p, 1, at]) * cst1 % Q1 == c
        evk_all = pc.load_tree_keys(ctx, seed, max_ob, 1, O)
        ctx.idx_load(None)
        ctx.set_option("small_levels", 0)
        bias = pc.rows(seed + 5, BENCH_TRIPLE[0])[0]
        got, sc = ctx.conv_then_pack(ct_in, S30, ker, S30, max_ob, 1, S30, bias)
        want, wsc = O.conv_then_pack(ct_in, S30, ker, S30, O.idx_plaintexts(), evk_all, max_ob, 1, S30, bias)
        assert sc == wsc == S30
        pc.eq(got, want, "conv_then_pack with the extreme pairs of (k_1, c') planted")
    finally:
        ctx.close()
