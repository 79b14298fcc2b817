"""The arithmetic forms of csrc/hc_arith.h and the butterflies and radix-16 rounds of csrc/hc_kernels.h AT THEIR STATED BOUNDS, shared by the host twin
(tests/test_arith_forms_cpu.py) and the device probe (tests/test_gpu_a_arith_forms.py). Both are builds of tests/arith_probe/arith_probe.hip, which calls each form once per
element; this module holds the operand vectors and the checkers. Every check is exact: Python integers (for the fp64 forms: the integer values of the doubles).

A case is a function case(run, q): it builds its vectors for the modulus q, calls run(op, params, ins, ...) - one launch of the probe's kernel `op` - and asserts on what comes
back. The vectors are the extremes of each form's stated input domain (and the values outside it that its comment says are still handled, "ANY 64-bit x"), where a lazy bound
that is wrong by less than a factor of two shows; uniform residues sit near half of every bound. CASES maps a name to (case, moduli)."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np

from oracle_lib import Q0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tests", "arith_probe")
DEVICE_LIB = os.path.join(PROBE_DIR, "_build", "libarith_probe.so")
HOST_LIB = os.path.join(PROBE_DIR, "_build", "libarith_probe_emu.so")
M64 = (1 << 64) - 1

# 20 bits; either side of 2^31 (the 32-bit form's limit); Q1 just below 2^49 (the fp64 form's limit); Q0; either side of 2^57 (HC_FM_FREE's limit: the largest prime it takes, the
# smallest it does not); 60 bits; the 61-bit special prime (8q = 2^64 - 2^24 + 8: no headroom at all)
MODULI = [0xC0001, 0x7FFE0001, 0x80140001, 0x1FFFFFFEA0001, Q0, 0x1FFFFFFFFFC0001, 0x2000000003A0001, 0x10000000006E0001, 0x1FFFFFFFFFE00001]
M32 = [q for q in MODULI if q < 1 << 31]                    # HC_SMALL_Q
MF64 = [q for q in MODULI if q < 1 << 49]                   # hc_f64_ok
MFREE = [q for q in MODULI if q < 1 << 57]                  # hc_fm_free
MALT = [q for q in MODULI if q >= 1 << 31]                  # HC_FM_ALT holds for every modulus; the kernels take it at or above 2^57, and the smaller ones cost nothing here
assert all(74 * q <= M64 for q in MFREE) and all(8 * q <= M64 for q in MODULI) and 0x1FFFFFFFFFC0001 in MFREE and 0x2000000003A0001 not in MFREE


class Probe:
    """ctypes binding of one build of arith_probe.hip"""

    def __init__(self, lib_path):
        self.L = C.CDLL(lib_path)
        self.L.arith_probe_run.restype = C.c_int
        self.L.arith_probe_run.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.launches = 0

    def ops(self):
        buf = C.create_string_buffer(4096)
        assert self.L.arith_probe_ops(buf, len(buf)) == 0
        return buf.value.decode().split(",")

    def run(self, op, params, ins, out_w=(1,), in_w=None):
        """one launch: ins are lists of integers below 2^64 (n items of in_w[k] words each); returns the outputs as lists of Python integers"""
        in_w = [1] * len(ins) if in_w is None else list(in_w)
        n = len(ins[0]) // in_w[0]
        arr = [np.array(x, dtype=np.uint64) for x in ins]
        for a, w in zip(arr, in_w):
            assert a.ndim == 1 and a.size == n * w, (op, a.shape, n, w)          # the probe trusts these sizes
        outs = [np.zeros(n * w, dtype=np.uint64) for w in out_w]
        p = np.array(list(params) + [0] * (8 - len(params)), dtype=np.uint64)
        pin = (C.c_void_p * len(arr))(*[a.ctypes.data for a in arr])
        pout = (C.c_void_p * len(outs))(*[a.ctypes.data for a in outs])
        win = (C.c_uint64 * len(arr))(*in_w)
        wout = (C.c_uint64 * len(outs))(*out_w)
        rc = self.L.arith_probe_run(op.encode(), p.ctypes.data, n, len(arr), pin, win, len(outs), pout, wout)
        assert rc == 0, f"arith_probe_run({op}) returned {rc}"
        self.launches += 1
        return [o.tolist() for o in outs]


def build_host_twin():
    subprocess.check_call(["make", "-s", "-C", PROBE_DIR, HOST_LIB])
    return HOST_LIB


# ---------------------------------------------------------------- vectors
def _uniq(xs, limit=M64):
    return list(dict.fromkeys(x for x in xs if 0 <= x <= limit))


def xs_any(q, rng, nrand=12):
    """a 64-bit x: 0, 1, q-+1, k q -+ 1 at the lazy bounds the kernels state (2q, 4q, 6q, 8q, 70q, 74q), 2^32 -+ 1, 2^63 -+ 1, 2^64 - 1, random"""
    xs = [0, 1, q - 1, q, q + 1]
    for k in (2, 4, 6, 8, 70, 74):
        xs += [k * q - 1, k * q, k * q + 1]
    xs += [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64 - 1, M64]
    xs += [rng.getrandbits(64) for _ in range(nrand)] + [rng.randrange(q) for _ in range(nrand // 2)]
    return _uniq(xs)


def ws_fixed(q, rng, nrand=5):
    """a fixed operand w in [0, q): 0, 1, 2, q-1, q-2, (q-+1)/2, random"""
    return _uniq([0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2] + [rng.randrange(q) for _ in range(nrand)], q - 1)


def below(b, q, rng, nrand=10):
    """x in [0, b) for a bound b = k q: both ends, every multiple of q inside and its neighbours, random"""
    xs = [0, 1, b - 2, b - 1]
    for m in range(q, b, q):
        xs += [m - 1, m, m + 1]
    return _uniq(xs + [rng.randrange(b) for _ in range(nrand)], b - 1)


def companion(w, q):
    return (w << 64) // q


def cols(tuples):
    return [list(c) for c in zip(*tuples)]


def d2u(values):
    return np.array(values, dtype=np.float64).view(np.uint64).tolist()


def u2d(words):
    return np.array(words, dtype=np.uint64).view(np.float64).tolist()


def f64_int(bits, what):
    """the exact integer a double holds"""
    d = u2d([bits])[0]
    assert d == d and abs(d) != float("inf") and d.is_integer(), f"{what}: {d!r} is no integer"
    return int(d)


def signed(xs):
    """every magnitude with both signs"""
    return list(dict.fromkeys(list(xs) + [-x for x in xs if x > 0]))


# ---------------------------------------------------------------- the forms of hc_arith.h
def case_mulhi_lo2(run, q):
    """floor(x p / 2^64) - result is 0, 1 or 2; hc_mulhi is exact. p: the Shoup companions and the Barrett constant the kernels hand it, and the extremes"""
    rng = random.Random(q)
    ps = _uniq([companion(w, q) for w in ws_fixed(q, rng)] + [M64 // q, 0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, M64] + [rng.getrandbits(64) for _ in range(4)])
    x, p = cols(itertools.product(xs_any(q, rng), ps))
    for xi, pi, r, e in zip(x, p, run("mulhi_lo2", [q], [x, p])[0], run("mulhi", [q], [x, p])[0]):
        assert (xi * pi >> 64) - r in (0, 1, 2), (hex(xi), hex(pi), hex(r))
        assert e == xi * pi >> 64, (hex(xi), hex(pi), hex(e))


def _shoup_vectors(q):
    rng = random.Random(q + 1)
    x, w = cols(itertools.product(xs_any(q, rng), ws_fixed(q, rng)))
    return x, w, [companion(v, q) for v in w]


def case_shoup4(run, q):
    """congruent to x w and below 4q for ANY 64-bit x; the companions come from hc_shoup_companion itself"""
    x, w, wp = _shoup_vectors(q)
    assert run("shoup_companion", [q], [w])[0] == wp
    for xi, wi, r in zip(x, w, run("shoup4", [q], [x, w, wp])[0]):
        assert r % q == xi * wi % q, (hex(xi), hex(wi), hex(r))
        assert r < 4 * q, (hex(xi), hex(wi), hex(r))


def case_mul_shoup(run, q):
    """hc_mul_shoup_lazy: below 2q for any 64-bit x; hc_mul_shoup: canonical"""
    x, w, wp = _shoup_vectors(q)
    for xi, wi, r, c in zip(x, w, run("mul_shoup_lazy", [q], [x, w, wp])[0], run("mul_shoup", [q], [x, w, wp])[0]):
        assert r % q == xi * wi % q and r < 2 * q, (hex(xi), hex(wi), hex(r))
        assert c == xi * wi % q, (hex(xi), hex(wi), hex(c))


def case_fold(run, q):
    """x mod b on [0, 2b) for b = q, 2q, 4q (what the kernels fold by) and b = 2^63 (the largest b the comment allows: x up to 2^64 - 1)"""
    rng = random.Random(q + 2)
    for b in (q, 2 * q, 4 * q, 1 << 63):
        x = below(2 * b, b, rng)
        for xi, r in zip(x, run("fold", [q, (1 << 64) - b], [x])[0]):
            assert r == xi % b, (hex(b), hex(xi), hex(r))


def case_canon(run, q):
    """hc_canon4 on [0, 4q), hc_canon8 on [0, 8q): x mod q"""
    rng = random.Random(q + 3)
    for op, k in (("canon4", 4), ("canon8", 8)):
        x = below(k * q, q, rng)
        for xi, r in zip(x, run(op, [q], [x])[0]):
            assert r == xi % q, (op, hex(xi), hex(r))


def case_reduce64(run, q):
    """x mod q for any 64-bit x; hc_addmod / hc_submod on residues"""
    rng = random.Random(q + 4)
    x = xs_any(q, rng, nrand=200)
    for xi, r in zip(x, run("reduce64", [q, M64 // q], [x])[0]):
        assert r == xi % q, (hex(xi), hex(r))
    a, b = cols(itertools.product(ws_fixed(q, rng), repeat=2))
    s, d = run("addmod", [q], [a, b], out_w=(1, 1))
    for ai, bi, si, di in zip(a, b, s, d):
        assert si == (ai + bi) % q and di == (ai - bi) % q, (hex(ai), hex(bi), hex(si), hex(di))


def case_mont(run, q):
    """a b 2^-64 mod q, canonical, for a b < q 2^64: a residue times ANY 64-bit b"""
    rng = random.Random(q + 5)
    rinv = pow(1 << 64, -1, q)
    a, b = cols(itertools.product(ws_fixed(q, rng), xs_any(q, rng)))
    for ai, bi, r in zip(a, b, run("mont", [q, pow(q, -1, 1 << 64)], [a, b])[0]):
        assert ai * bi < q << 64
        assert r == ai * bi * rinv % q, (hex(ai), hex(bi), hex(r))


def mont_lazy_vectors(q):
    """the vectors of tests/test_mont_operand_cpu.py::test_mont_lazy_against_big_integers"""
    rng = random.Random(q)
    xs = [0, 1, q - 1, q, q + 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1, (1 << 32) - 1, 1 << 32]
    for k in (2, 4, 6, 8, 72, 81, 83):
        xs += [v for v in (k * q - 1, k * q, k * q + 1) if v <= M64]
    xs += [rng.getrandbits(64) for _ in range(200)]
    ws = [q - 1, q - 2, 1, 0, 2, (q - 1) // 2, (q + 1) // 2] + [rng.randrange(q) for _ in range(40)]
    return xs, ws


def case_mont_lazy(run, q):
    """congruent to x w and in [1, 2q - 1] for any 64-bit x, w held as w 2^64 mod q; the operand is built as hc_k_pointwise<HC_PW_TO_MONT> builds it: hc_mont(w, 2^128 mod q)"""
    xs, ws = mont_lazy_vectors(q)
    qinv = pow(q, -1, 1 << 64)
    wm = run("mont", [q, qinv], [ws, [pow(2, 128, q)] * len(ws)])[0]
    assert wm == [(w << 64) % q for w in ws]
    x, w = cols(itertools.product(xs, ws))
    for xi, wi, r in zip(x, w, run("mont_lazy", [q, qinv], [x, [(v << 64) % q for v in w]])[0]):
        assert r % q == xi * wi % q, (hex(xi), hex(wi), hex(r))
        assert 0 < r < 2 * q, (hex(xi), hex(wi), hex(r))


def case_mont_redc(run, q):
    """T 2^-64 mod q, canonical, for sums T of 1 to 7 products of residues and for every T up to just below q 2^64"""
    rng = random.Random(q + 6)
    rinv = pow(1 << 64, -1, q)
    ts = [0, 1, M64, 1 << 64, (1 << 64) + 1, (q << 64) - 1, (q << 64) - 2, (q - 1) << 64, ((q - 1) << 64) + 1, (q << 64) - (1 << 63)]
    for k in range(1, 8):
        ts.append(k * (q - 1) * (q - 1))
        ts += [sum(rng.randrange(q) * rng.randrange(q) for _ in range(k)) for _ in range(20)]
        ts.append(sum((q - 1) * rng.randrange(q) for _ in range(k)))
    ts += [rng.randrange(q << 64) for _ in range(100)]
    assert all(t < q << 64 for t in ts)
    for t, r in zip(ts, run("mont_redc", [q, pow(q, -1, 1 << 64)], [[t & M64 for t in ts], [t >> 64 for t in ts]])[0]):
        assert r == t * rinv % q, (hex(t), hex(r))


# ---------------------------------------------------------------- fp64 (q < 2^49)
def f64_params(q):
    return d2u([float(q), 1.0 / float(q)])


def case_f64_mulmod(run, q):
    """an exact integer congruent to x w with |r| < q, for |x| up to 2^51 - 1 and w in [0, q); the companion w / q is one correctly rounded division, as hc_build_tables makes it"""
    assert q < 1 << 49
    rng = random.Random(q + 7)
    mags = _uniq([0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q + 1, 4 * q - 1, 4 * q, 4 * q + 1, (1 << 50) - 1, 1 << 50, (1 << 50) + 1, (1 << 51) - 2, (1 << 51) - 1]
                 + [rng.randrange(1 << 51) for _ in range(12)] + [rng.randrange(4 * q) for _ in range(12)], (1 << 51) - 1)
    x, w = cols(itertools.product(signed(mags), ws_fixed(q, rng, nrand=8)))
    out = run("f64_mulmod", f64_params(q), [d2u([float(v) for v in x]), d2u([float(v) for v in w]), d2u([float(v) / float(q) for v in w])])[0]
    for xi, wi, bits in zip(x, w, out):
        r = f64_int(bits, (xi, wi))
        assert (r - xi * wi) % q == 0, (xi, wi, r)
        assert abs(r) < q, (xi, wi, r)


def case_f64_reduce(run, q):
    """an exact integer congruent to u with |r| <= q/2 + 1, for |u| < 2^53"""
    rng = random.Random(q + 8)
    mags = _uniq([0, 1, q // 2, q // 2 + 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 3 * q // 2, 3 * q // 2 + 1, 4 * q - 1, 4 * q, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, (1 << 53) - 2, (1 << 53) - 1]
                 + [(2 * k + 1) * q // 2 + d for k in (1, 5, 1000) for d in (0, 1)] + [rng.randrange(1 << 53) for _ in range(100)] + [rng.randrange(4 * q) for _ in range(100)], (1 << 53) - 1)
    u = signed(mags)
    for ui, bits in zip(u, run("f64_reduce", f64_params(q), [d2u([float(v) for v in u])])[0]):
        r = f64_int(bits, ui)
        assert (r - ui) % q == 0, (ui, r)
        assert 2 * abs(r) <= q + 2, (ui, r)


def case_f64_convert(run, q):
    """hc_f64_from_u is exact for x < 2^52; hc_f64_to_u_plus(v, base) = v + base modulo 2^64 for integers |v| < 2^51, negative ones and base = 2^64 - 1 included; the round trip"""
    rng = random.Random(q + 9)
    bases = [0, 1, q - 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1, 0x0008000000000000, 0x0007FFFFFFFFFFFF, rng.getrandbits(64), rng.getrandbits(64)]
    xs = _uniq([0, 1, q - 1, q, (1 << 32) - 1, 1 << 32, (1 << 51) - 1, 1 << 51, (1 << 52) - 1] + [rng.randrange(1 << 52) for _ in range(30)])
    x, base = cols(itertools.product(xs, bases))
    dbl, back = run("f64_from_u", [q], [x, base], out_w=(1, 1))
    for xi, bi, d, r in zip(x, base, dbl, back):
        assert f64_int(d, xi) == xi, (xi, d)
        assert xi >= 1 << 51 or r == (xi + bi) & M64, (xi, hex(bi), hex(r))
    vs = signed(_uniq([0, 1, q - 1, q, 4 * q - 1, (1 << 50), (1 << 51) - 1] + [rng.randrange(1 << 51) for _ in range(30)], (1 << 51) - 1))
    v, base = cols(itertools.product(vs, bases))
    for vi, bi, r in zip(v, base, run("f64_to_u_plus", [q], [d2u([float(t) for t in v]), base])[0]):
        assert r == (vi + bi) & M64, (vi, hex(bi), hex(r))


# ---------------------------------------------------------------- 32-bit canonical (q < 2^31)
def case_mul32(run, q):
    """canonical x w for ANY y < 2^32; the 8-byte twiddle is narrowed from the 64-bit pair by hc_tw32"""
    assert q < 1 << 31
    rng = random.Random(q + 10)
    ys = _uniq([0, 1, q - 1, q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1] + [rng.getrandbits(32) for _ in range(60)], (1 << 32) - 1)
    y, w = cols(itertools.product(ys, ws_fixed(q, rng, nrand=8)))
    for yi, wi, r in zip(y, w, run("mul32", [q], [y, w, [companion(v, q) for v in w]])[0]):
        assert r == yi * wi % q, (hex(yi), hex(wi), hex(r))


def case_addsub32(run, q):
    """hc_add32 / hc_sub32 on residues, hc_csub32 on [0, 2q): canonical"""
    rng = random.Random(q + 11)
    a, b = cols(itertools.product(ws_fixed(q, rng, nrand=20), repeat=2))
    s, d = run("add32", [q], [a, b], out_w=(1, 1))
    for ai, bi, si, di in zip(a, b, s, d):
        assert si == (ai + bi) % q and di == (ai - bi) % q, (hex(ai), hex(bi), hex(si), hex(di))
    x = below(2 * q, q, rng, nrand=100)
    for xi, r in zip(x, run("csub32", [q], [x])[0]):
        assert r == xi % q, (hex(xi), hex(r))


# ---------------------------------------------------------------- butterflies, one call each
def _xyw(X, q, rng):
    """(X, Y, w): X from the mode's list, Y ANY 64-bit value (hc_shoup4 takes it), w fixed operands"""
    return list(itertools.product(X, xs_any(q, rng, nrand=6), ws_fixed(q, rng, nrand=3)))


def _check_fwd(q, X, Y, w, x2, y2, bound):
    assert x2 % q == (X + w * Y) % q and y2 % q == (X - w * Y) % q, (hex(X), hex(Y), hex(w), hex(x2), hex(y2))
    assert x2 < bound and y2 < bound, (hex(X), hex(Y), hex(w), hex(x2), hex(y2), hex(bound))


def case_lazy_fwd_free(run, q):
    """HcLazy<HC_FM_FREE>::fwd: (X + wY, X - wY), each stage adding at most 4q to the bound - up to X = 66q - 1, the input of a transform's last stage, whose outputs are the 70q
    that HC_FREE_OFF = 72 and the 74q < 2^64 condition rest on; one tile and the pair form"""
    assert 74 * q <= M64
    rng = random.Random(q + 12)
    t = _xyw(_uniq([0, q - 1, 6 * q - 1, 62 * q - 1, 66 * q - 2, 66 * q - 1] + [rng.randrange(66 * q) for _ in range(3)]), q, rng)
    X, Y, w = cols(t)
    wp = [companion(v, q) for v in w]
    x2, y2 = run("lazy_fwd_free", [q], [X, Y, w, wp], out_w=(1, 1))
    X1, Y1 = X[::-1], Y[::-1]
    p = run("lazy_fwd2_free", [q], [X, Y, X1, Y1, w, wp], out_w=(1, 1, 1, 1))
    for i, (Xi, Yi, wi) in enumerate(t):
        _check_fwd(q, Xi, Yi, wi, x2[i], y2[i], Xi + 1 + 4 * q)
        assert x2[i] < 70 * q and y2[i] < 70 * q
        assert (p[0][i], p[1][i]) == (x2[i], y2[i]), "the pair form's first tile differs from the one-tile form"
        _check_fwd(q, X1[i], Y1[i], wi, p[2][i], p[3][i], X1[i] + 1 + 4 * q)


def case_lazy_fwd_alt(run, q):
    """HcLazy<HC_FM_ALT>::fwd: inputs below 8q stay below 8q (X folded by 4q first); one tile and the pair form"""
    assert 8 * q <= M64
    rng = random.Random(q + 13)
    t = _xyw(_uniq([0, q - 1, 4 * q - 1, 4 * q, 4 * q + 1, 8 * q - 2, 8 * q - 1] + [rng.randrange(8 * q) for _ in range(3)]), q, rng)
    X, Y, w = cols(t)
    wp = [companion(v, q) for v in w]
    x2, y2 = run("lazy_fwd_alt", [q], [X, Y, w, wp], out_w=(1, 1))
    X1, Y1 = X[::-1], Y[::-1]
    p = run("lazy_fwd2_alt", [q], [X, Y, X1, Y1, w, wp], out_w=(1, 1, 1, 1))
    for i, (Xi, Yi, wi) in enumerate(t):
        _check_fwd(q, Xi, Yi, wi, x2[i], y2[i], 8 * q)
        assert (p[0][i], p[1][i]) == (x2[i], y2[i]), "the pair form's first tile differs from the one-tile form"
        _check_fwd(q, X1[i], Y1[i], wi, p[2][i], p[3][i], 8 * q)


def case_lazy_inv(run, q):
    """HcLazy::inv (the pair form): (X + Y, w (X - Y)) with everything in [0, 4q), in and out"""
    rng = random.Random(q + 14)
    v = below(4 * q, q, rng, nrand=4)
    t = list(itertools.product(v, v, ws_fixed(q, rng, nrand=2)))
    X, Y, w = cols(t)
    wp = [companion(u, q) for u in w]
    X1, Y1 = Y[::-1], X[::-1]
    p = run("lazy_inv2", [q], [X, Y, X1, Y1, w, wp], out_w=(1, 1, 1, 1))
    for i, (Xi, Yi, wi) in enumerate(t):
        for a, b, s, d in ((Xi, Yi, p[0][i], p[1][i]), (X1[i], Y1[i], p[2][i], p[3][i])):
            assert s % q == (a + b) % q and d % q == wi * (a - b) % q, (hex(a), hex(b), hex(wi), hex(s), hex(d))
            assert s < 4 * q and d < 4 * q, (hex(a), hex(b), hex(wi), hex(s), hex(d))


def case_canon32_fwd(run, q):
    """HcCanon32::fwd: canonical in, canonical out"""
    rng = random.Random(q + 15)
    v = ws_fixed(q, rng, nrand=4)
    t = list(itertools.product(v, v, v))
    X, Y, w = cols(t)
    x2, y2 = run("canon32_fwd", [q], [X, Y, w, [companion(u, q) for u in w]], out_w=(1, 1))
    for (Xi, Yi, wi), a, b in zip(t, x2, y2):
        assert a == (Xi + wi * Yi) % q and b == (Xi - wi * Yi) % q, (hex(Xi), hex(Yi), hex(wi), hex(a), hex(b))


# ---------------------------------------------------------------- rounds: the plain networks, and tiles that start at the top of the stated input bound
def ct_network(e, tw, q):
    """hc_ct_round's butterfly network on canonical residues; tw[slot]"""
    e = [v % q for v in e]
    for s in range(4):
        half = 8 >> s
        for g in range(1 << s):
            w = tw[(1 << s) - 1 + g]
            for k in range(half):
                a = g * 2 * half + k
                b = a + half
                e[a], e[b] = (e[a] + w * e[b]) % q, (e[a] - w * e[b]) % q
    return e


def gs_network(e, tw, q, last=None):
    """hc_gs_round's; last = (ninv, w_last) for the round that also scales by N^-1"""
    e = [v % q for v in e]
    for s in range(4):
        dist = 1 << s
        for g in range(8 >> s):
            w = tw[(8 >> s) - 1 + g]
            if last is not None and s == 3:
                w = last[1]
            for k in range(dist):
                a = g * 2 * dist + k
                b = a + dist
                u, d = e[a] + e[b], e[a] - e[b]
                e[a] = (u * last[0] if last is not None and s == 3 else u) % q
                e[b] = d * w % q
    return e


def _tiles(lo, hi, q, rng):
    """16-element tiles over [lo, hi]: all at the top, all at the bottom, the alternating extremes in both phases and by halves, +-(q - 1), random"""
    t = [[hi] * 16, [lo] * 16, [hi, lo] * 8, [lo, hi] * 8, [hi] * 8 + [lo] * 8, [lo] * 8 + [hi] * 8, [q - 1] * 16, [q - 1, max(lo, 1 - q)] * 8, [max(lo, 1 - q), q - 1] * 8]
    return t + [[rng.randint(lo, hi) for _ in range(16)] for _ in range(3)] + [[rng.choice((lo, hi, hi - 1, q - 1)) for _ in range(16)] for _ in range(3)]


def _twiddles(q, rng, rounds=1):
    """per tile: q - 1 everywhere, 1 everywhere, random (each with its true companion)"""
    n = 16 * rounds
    return [[q - 1] * n, [1] * n, [rng.randrange(q) for _ in range(n)], [rng.choice((q - 1, q - 2, 1, (q + 1) // 2)) for _ in range(n)]]


def _flat_tw(tw, conv):
    return [v for w in tw for v in conv(w)]


def _case_ct_round4(run, q, op, in_top, out_bound):
    rng = random.Random(q + 16)
    cases = list(itertools.product(_tiles(0, in_top, q, rng), _twiddles(q, rng, rounds=4)))
    e = [v for tile, _ in cases for v in tile]
    tw = [v for _, t in cases for v in _flat_tw(t, lambda w: (w, companion(w, q)))]
    lazy, canon = run(op, [q, M64 // q], [e, tw], out_w=(16, 16), in_w=(16, 128))
    for i, (tile, t) in enumerate(cases):
        want = tile
        for r in range(4):
            want = ct_network(want, t[16 * r:16 * r + 16], q)
        got = lazy[16 * i:16 * i + 16]
        assert [v % q for v in got] == want, (op, hex(q), i, "residues")
        assert max(got) < out_bound, (op, hex(q), i, hex(max(got)), hex(out_bound))
        assert canon[16 * i:16 * i + 16] == want, (op, hex(q), i, "hc_fwd_canon")


def case_ct_round4_free(run, q):
    """hc_ct_round<HcLazy<HC_FM_FREE>> four times = the 16 stages of a transform: inputs up to 6q - 1 give outputs below 70q, congruent to the plain network; hc_fwd_canon<FREE>
    (hc_reduce64) of them is canonical"""
    assert 74 * q <= M64
    _case_ct_round4(run, q, "ct_round4_free", 6 * q - 1, 70 * q)


def case_ct_round4_alt(run, q):
    """the same under HC_FM_ALT: inputs up to 8q - 1 stay below 8q; hc_fwd_canon<ALT> (hc_canon8) is canonical"""
    _case_ct_round4(run, q, "ct_round4_alt", 8 * q - 1, 8 * q)


def _gs_inputs(q, lo, hi, conv, seed):
    rng = random.Random(q + seed)
    cases = list(itertools.product(_tiles(lo, hi, q, rng), _twiddles(q, rng)))
    lasts = [(rng.choice((q - 1, 1, rng.randrange(q))), rng.choice((q - 1, 1, rng.randrange(q)))) for _ in cases]
    tw = [v for _, t in cases for v in _flat_tw(t, conv)]
    extra = [v for l in lasts for w in l for v in conv(w)]
    return cases, lasts, tw, extra


def case_gs_round(run, q):
    """hc_gs_round, 64-bit lazy, one round, plain and LAST: [0, 4q) in, [0, 4q) out, congruent to the plain network"""
    cases, lasts, tw, extra = _gs_inputs(q, 0, 4 * q - 1, lambda w: (w, companion(w, q)), 17)
    e = [v for tile, _ in cases for v in tile]
    for op in ("gs_round", "gs_round_last"):
        got = run(op, [q], [e, tw, extra], out_w=(16,), in_w=(16, 32, 4))[0]
        for i, (tile, t) in enumerate(cases):
            want = gs_network(tile, t, q, lasts[i] if op == "gs_round_last" else None)
            assert [v % q for v in got[16 * i:16 * i + 16]] == want, (op, hex(q), i)
            assert max(got[16 * i:16 * i + 16]) < 4 * q, (op, hex(q), i)


def case_gs_round32(run, q):
    """hc_gs_round(HcCanon32), one round, plain and LAST: canonical in and out"""
    cases, lasts, tw, extra = _gs_inputs(q, 0, q - 1, lambda w: (w, companion(w, q)), 18)
    e = [v for tile, _ in cases for v in tile]
    for op in ("gs_round32", "gs_round32_last"):
        got = run(op, [q], [e, tw, extra], out_w=(16,), in_w=(16, 32, 4))[0]
        for i, (tile, t) in enumerate(cases):
            assert got[16 * i:16 * i + 16] == gs_network(tile, t, q, lasts[i] if op == "gs_round32_last" else None), (op, hex(q), i)


def case_gs_round_f64(run, q):
    """hc_gs_round_f64<false / true>, one round on tiles of +-(q - 1): exact integers below q in magnitude, congruent to the plain network; the pairs {w, w / q} as
    hc_build_tables converts them"""
    def conv(w):
        return d2u([float(w), float(w) / float(q)])
    cases, lasts, tw, extra = _gs_inputs(q, 1 - q, q - 1, conv, 19)
    e = d2u([float(v) for tile, _ in cases for v in tile])
    for op in ("gs_round_f64", "gs_round_f64_last"):
        got = run(op, f64_params(q), [e, tw, extra], out_w=(16,), in_w=(16, 32, 4))[0]
        for i, (tile, t) in enumerate(cases):
            vals = [f64_int(b, (op, i)) for b in got[16 * i:16 * i + 16]]
            assert [v % q for v in vals] == gs_network(tile, t, q, lasts[i] if op == "gs_round_f64_last" else None), (op, hex(q), i)
            assert max(abs(v) for v in vals) < q, (op, hex(q), i)


CASES = {
    "mulhi_lo2": (case_mulhi_lo2, MODULI), "shoup4": (case_shoup4, MODULI), "mul_shoup": (case_mul_shoup, MODULI), "fold": (case_fold, MODULI), "canon": (case_canon, MODULI),
    "reduce64": (case_reduce64, MODULI), "mont": (case_mont, MODULI), "mont_lazy": (case_mont_lazy, MODULI), "mont_redc": (case_mont_redc, MODULI),
    "f64_mulmod": (case_f64_mulmod, MF64), "f64_reduce": (case_f64_reduce, MF64), "f64_convert": (case_f64_convert, MF64[-1:]),
    "mul32": (case_mul32, M32), "addsub32": (case_addsub32, M32),
    "lazy_fwd_free": (case_lazy_fwd_free, MFREE), "lazy_fwd_alt": (case_lazy_fwd_alt, MODULI), "lazy_inv": (case_lazy_inv, MODULI), "canon32_fwd": (case_canon32_fwd, M32),
    "ct_round4_free": (case_ct_round4_free, MFREE), "ct_round4_alt": (case_ct_round4_alt, MALT),
    "gs_round": (case_gs_round, MODULI), "gs_round32": (case_gs_round32, M32), "gs_round_f64": (case_gs_round_f64, MF64),
}
PARAMS = [(name, q) for name, (_, moduli) in CASES.items() for q in moduli]


def case_id(p):
    return f"{p[0]}-q{p[1].bit_length()}-{p[1]:x}"
