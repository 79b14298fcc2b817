"""hc_k_a1p<1> / hc_k_a1g<1> form a_1 = k_1 * c' mod Q1 in fp64 from ONE double of c' per coefficient (hc_f64_mulmod_q in hc_arith.h; hc_k_ctc_pairs writes limb 1 of c' as a
dense array of doubles when Q1 < 2^49). Without a GPU:
(1) the product function, compiled for the host as the arithmetic probes are, against exact Python integers: congruence, the magnitude bound its comment states,
    (1/2 + q 2^-51) q, and the exactness of every intermediate (h + l = k c' with l representable and |l| <= 2^44; h - kq q representable; the sum representable), at the operand
    extremes in all pairs and on seeded random pairs, with c' canonical and centred, under Q1 - the largest modulus below 2^49 that tests/parity_cases.py offers - and a 42-bit one;
(2) in the fibre emulator, word for word against the oracle: the batch of three of tests/test_operand_streams_cpu.py (members uniform / all q - 1 / all 0, max_ob = 4,
    small_levels = 0) under the product's triple and under the Q1 >= 2^49 triple (the integer path), grouped convolutions of m = 2 and m = 3 such members (hc_k_a1g<1>), and
    hc_div_round_last (c' = ct_in x 1) on the same three kinds of rows."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import multiconv_cases as mc
import multiconv_ref as MR
import parity_cases as pc
from oracle_lib import Q1
from test_operand_streams_cpu import BENCH_TRIPLE, EMU_DIR, EMU_LIB, INT_A1_TRIPLE, case_batch_of_three

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tests", "arith_probe")
PROBE_LIB = os.path.join(PROBE_DIR, "_build", "liba1_product_probe.so")
N = pc.N

Q1_OFFERED = max(t[1] for t in pc.CONV_TRIPLES if t[1] < 1 << 49)          # the largest Q1 below 2^49 among parity_cases' conv triples: the product's own
Q_42 = 0x3FFFFE80001                                                       # parity_cases.Q_MIX: an accepted modulus well below the limit
assert Q_42 in pc.Q_MIX and Q_42 < 1 << 42
PRODUCT_MODULI = sorted({Q1, Q1_OFFERED, Q_42})


@pytest.fixture(scope="module")
def product():
    os.makedirs(os.path.dirname(PROBE_LIB), exist_ok=True)
    src = os.path.join(PROBE_DIR, "a1_product_probe.cpp")
    hdr = os.path.join(ROOT, "optimal_conv_amd", "csrc", "hc_arith.h")
    if not os.path.exists(PROBE_LIB) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(PROBE_LIB):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.dirname(hdr), "-shared", "-o", PROBE_LIB, src])
    L = C.CDLL(PROBE_LIB)
    L.a1_product_probe.restype = None
    L.a1_product_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]

    def run(ks, ws, q):
        k, w = np.array(ks, dtype=np.uint64), np.array(ws, dtype=np.float64)
        out = np.zeros(len(ks), dtype=np.float64)
        L.a1_product_probe(k.ctypes.data, w.ctypes.data, out.ctypes.data, len(ks), q)
        return out.tolist()
    return run


def exact(v):
    """the integer v is a double"""
    return abs(v) < 1 << 53 or int(float(v)) == v


def check_product(run, q, pairs):
    """every step of hc_f64_mulmod_q in exact integers beside the probe's result"""
    fq, qinv = float(q), 1.0 / float(q)
    bound = q // 2 + (q * q >> 51) + 1                                     # (1/2 + q 2^-51) q, rounded up
    got = run([k for k, _ in pairs], [float(w) for _, w in pairs], q)
    worst = 0
    for (k, w), r in zip(pairs, got):
        assert 0 <= k < q and abs(w) < q
        P = k * w
        h = float(k) * float(w)                                            # one rounding, as the kernel's v_mul_f64
        l = P - int(h)
        assert int(float(l)) == l and abs(l) <= 1 << 44, (hex(k), w, l)    # fma(x, w, -h) is exact
        kq = round(h * qinv)                                               # rint: ties to even, as Python's round
        t = int(h) - kq * q
        assert exact(t) and abs(t) < 1 << 53, (hex(k), w, t)               # fma(-kq, q, h) is exact
        want = t + l
        assert want == P - kq * q and exact(want) and abs(want) < 1 << 53
        assert r == float(want) and int(r) == want, (hex(k), w, r, want)
        assert (int(r) - P) % q == 0, (hex(k), w, r)
        assert abs(int(r)) <= bound, (hex(k), w, r, bound)
        worst = max(worst, abs(int(r)))
    return worst / fq


def extremes(q):
    xs = [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, 1 << 48, (1 << 48) - 1, (1 << 48) + 1]
    return list(dict.fromkeys(x for x in xs if 0 <= x < q))


@pytest.mark.parametrize("q", PRODUCT_MODULI, ids=lambda q: f"q{q:x}")
@pytest.mark.parametrize("centred", [False, True], ids=["canonical", "centred"])
def test_product_is_exact_and_inside_its_bound(product, q, centred):
    rng = random.Random(0xA1F64 ^ q)
    pairs = list(itertools.product(extremes(q), repeat=2)) + [(rng.randrange(q), rng.randrange(q)) for _ in range(100000)]
    if centred:
        pairs = [(k, w - q if w > q // 2 else w) for k, w in pairs]
    worst = check_product(product, q, pairs)
    print(f"q = {q:#x} {'centred' if centred else 'canonical'}: {len(pairs)} pairs, max |r| / q = {worst:.4f} (bound {0.5 + q / 2.0 ** 51:.4f})")


# ---- the kernels in the fibre emulator
@pytest.fixture(scope="module")
def emu():
    from optimal_conv_amd import Context
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    return lambda Q, P: Context(Q, P, lib_path=EMU_LIB)


def test_batch_of_three_fp64_product(emu):
    case_batch_of_three(emu, BENCH_TRIPLE, max_ob=4)


def test_batch_of_three_integer_path(emu):
    case_batch_of_three(emu, INT_A1_TRIPLE, max_ob=4)


def extreme_members(seed, m, max_ob, O):
    """m members of one grouped convolution: uniform residues, then all q - 1, then all 0"""
    q0, q1, _ = pc.conv_moduli(O)
    ins, kers = [], []
    for j, fill in enumerate([None, lambda q: q - 1, lambda q: 0][:m]):
        if fill is None:
            ct_in, ker = pc.planted_conv_inputs(seed + 17 * j, max_ob, O)
        else:
            ct_in, ker = np.empty((2, 2, N), dtype=np.uint64), np.empty((max_ob, 2, N), dtype=np.uint64)
            ct_in[:, 0], ct_in[:, 1], ker[:, 0], ker[:, 1] = fill(q0), fill(q1), fill(q0), fill(q1)
        ins.append(ct_in); kers.append(ker)
    return ins, kers


def case_grouped_extremes(make_ctx, triple, m, max_ob=4, seed=0xA16):
    """one convolution of m input ciphertexts sharing a ct_out (hc_k_a1g / hc_k_a3g), small_levels = 0, launches of 3 nodes: == the yardstick of tests/multiconv_ref.py"""
    ctx, O = pc._triple_env(make_ctx, triple)
    try:
        ctx.set_option("small_levels", 0)
        ctx.set_option("chunk_nodes", 3)
        evk_all = pc.load_tree_keys(ctx, seed, max_ob, 1, O)
        ctx.idx_load(None)
        ins, kers = extreme_members(seed, m, max_ob, O)
        bias = pc.rows(seed + 5, triple[0])[0]
        got = mc.run_groups(ctx, [ins], [kers], [bias], max_ob, 1)[0][0]
        pc.eq(got, MR.multi_conv(O, ins, kers, evk_all, max_ob, 1, bias), f"grouped convolution of m = {m} members (uniform / all q - 1 / all 0)")
        assert got.any()
    finally:
        ctx.close()


@pytest.mark.parametrize("m", [2, 3])
def test_grouped_members_fp64_product(emu, m):
    case_grouped_extremes(emu, BENCH_TRIPLE, m)


def case_div_round_last_extremes(make_ctx, triple, seed=0xA1D):
    """hc_div_round_last at level 1 runs loop A with constants of one and a kernel plaintext of ones: c' is the input's limb 1 itself"""
    ctx, O = pc._triple_env(make_ctx, triple)
    q0, q1 = triple[0], triple[1]
    try:
        for name, limb1 in (("uniform", pc.rows(seed, q1)[0]), ("all q - 1", np.full(N, q1 - 1, dtype=np.uint64)), ("all 0", np.zeros(N, dtype=np.uint64))):
            x = np.stack([pc.rows(seed + 1, q0)[0], limb1])
            pc.eq(ctx.div_round_last(1, x), O.div_round_last(1, x), f"div_round_last, limb 1 {name}")
    finally:
        ctx.close()


def test_div_round_last_fp64_product(emu):
    case_div_round_last_extremes(emu, BENCH_TRIPLE)
