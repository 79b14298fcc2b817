"""The inner products' LAZY SUMS at their term counts and extremes, shared by tests/test_lazy_sums_cpu.py (the emulator builds) and tests/test_gpu_a_lazy_sums.py (the device).

Since round 6 every sum of products on the bootstrapping chain adds its terms as plain integers and reduces once per group; four bounds of csrc/hc_kernels.h carry that:
    hc_k_ks_mac_all / _multi, 8-byte rows   128-bit sums, PER = 6 products per reduction   6 q^2 < q 2^64
    the same on 4-byte rows                  64-bit sums, PER = 4                           4 (2^31 - 1)^2 < 2^64 - 5 overflow
    hc_k_qp_mul_sum, hc_k_qp_mul_sum_g       128-bit sums, 7 products                       7 q^2 < q 2^64
    hc_k_lv_lincomb<NT>, NT <= 8             128-bit sums, all at once                      8 q^2 < q 2^64: tight below 2^61
With uniform residues a product averages q^2 / 4 and a period one or two too long still gives the right residues. Here the operands are PLANTED: the pattern is chosen per
coefficient and is the SAME in every term, so that a group's sum reaches count (q - 1)^2, and what is planted is the pre-image of the value the kernel multiplies by after its own
conversions (a stored key word that packs to q - 1, a plaintext that MForm turns into q - 1, a constant whose Montgomery form is q - 1). Every case asserts on its own inputs, with
Python integers, that the maximum is reached in every (limb, component) and every reduction group it checks, before it looks at a result. Every comparison is exact.

A row holds N coefficients but only M = 1536 distinct COLUMNS (coefficient j is column j mod M: the six classes interleave over j, and the last 256 coefficients of a row hold all
of them), so the reference is M Python-integer sums per row and every one of the N results is compared."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle_lib import P0, Q0, Q1, splitmix_rows            # noqa: F401 (P0: the conv context of case_lv_mul_sum is [Q0, Q1], [P0])
from parity_cases import P_CHAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_DIR = os.path.join(ROOT, "tests", "arith_probe")
DEVICE_LIB = os.path.join(PROBE_DIR, "_build", "libsum_probe.so")
HOST_LIB = os.path.join(PROBE_DIR, "_build", "libsum_probe_emu.so")

N = 65536
NCLASS = 6                        # (q-1)(q-1) in every term (and products just below it) | every term 0 | one term (q-1)^2, the rest 0 | (q-1) x 1 | alternating (q-1)^2 and 0 | uniform
M = NCLASS * 256
IDX = np.arange(N) % M
R64 = 1 << 64
POISON = 0xDEADBEEF

Q_TOP32, Q_20, Q_LOW64, Q_60 = 0x7FFE0001, 0xC0001, 0x80140001, 0x1000000000B00001
MODULI = [Q_TOP32, Q_20, Q_LOW64, Q_60, P_CHAIN[0], P_CHAIN[1]]
assert all(q % (1 << 17) == 1 for q in MODULI) and 4 * (Q_TOP32 - 1) ** 2 < R64 < 5 * (Q_TOP32 - 1) ** 2
assert all(7 * (q - 1) ** 2 < q << 64 for q in MODULI) and 8 * (P_CHAIN[0] - 1) ** 2 < P_CHAIN[0] << 64 < 9 * (P_CHAIN[0] - 1) ** 2      # the eight-term bound is tight there
# the leveled context of section 2: every modulus above; limbs 3 and 4 take 4-byte rows under pack32 = 2 (limbs 0 and 1 never do)
CTX_Q, CTX_P = [Q_60, Q_LOW64, P_CHAIN[1], Q_TOP32, Q_20], [P_CHAIN[0]]


def small(q):
    return q < 1 << 31


def obj(values):
    a = np.empty(len(values), dtype=object)
    a[:] = [int(v) for v in values]
    return a


def pattern(q, nterms, seed, shift=0, period=None):
    """X[t][c], Y[t][c]: first operand and multiplicand of term t in column c, Python integers in object arrays of shape (nterms, M). The class of a column is c mod 6 and k = c // 6
    moves what moves with j. The lone term of class 2 is term (k + shift) mod period (period: nterms, or a fixed count above it when the operands of a longer list are shared: then
    some columns of the class hold no product at all), so Y[t] does not depend on how many terms a launch takes."""
    period = period or nterms
    X, Y = np.zeros((nterms, M), dtype=object), np.zeros((nterms, M), dtype=object)
    k, cls, top = np.arange(M) // NCLASS, np.arange(M) % NCLASS, np.uint64(q - 1)
    zero, one = np.uint64(0), np.uint64(1)
    # class 0: q - 1 exactly in every fourth column of the class, and within 1023 of it in the others. A sum T past q 2^64 makes hc_mont_redc wrong only where its Montgomery
    # quotient h = mulhi(lo q^-1, q) falls below hi - q - for nine products below 2^61 one value of T in eight - so the columns near the maximum differ in their low bits
    near = lambda mul, t: np.where(k % 4 == 0, top, top - np.uint64(1) * ((k * mul + 977 * t) % 1024).astype(np.uint64))
    for t in range(nterms):
        ux, uy = splitmix_rows(seed + 7919 * t, q, M), splitmix_rows(seed + 7919 * t + 104729, q, M)
        lone = np.where((k + shift) % period == t, top, zero)
        x = np.select([cls == 0, cls == 1, cls == 2, cls == 3, cls == 4], [near(40503, 0), np.where(k % 3 == 2, top, zero), np.where(k % 2 == 1, top, lone), top, top], default=ux)
        y = np.select([cls == 0, cls == 1, cls == 2, cls == 3, cls == 4],
                      [near(30011, t), np.where(k % 3 == 1, top, zero), np.where(k % 2 == 1, lone, top), one, np.where((t + k + shift) % 2 == 0, top, zero)], default=uy)
        X[t], Y[t] = x.astype(np.uint64).astype(object), y.astype(np.uint64).astype(object)
    return X, Y


def groups(nterms, per, present=None):
    """the reduction groups of a sum of nterms products reduced every `per` terms (None: all at once): lists of the term indices that are present"""
    per = per or nterms
    return [[t for t in range(g, min(g + per, nterms)) if present is None or present[t]] for g in range(0, nterms, per)]


def assert_planted(X, Y, q, grps, what):
    """the planted maximum is reached: in every reduction group the largest exact sum over the columns is count (q - 1)^2. X[t], Y[t]: the operands AS THE KERNEL MULTIPLIES THEM
    (recomputed from the stored words by the caller)"""
    for g in grps:
        if g:
            top = max(sum(X[t] * Y[t] for t in g))
            assert top == len(g) * (q - 1) ** 2, f"{what}: group {g} reaches {top:#x}, planted {len(g) * (q - 1) ** 2:#x}"


def row(values):
    """a row of N 8-byte words from M column values"""
    return np.array([int(v) for v in values], dtype=np.uint64)[IDX]


def row32(values):
    """the 4-byte form of a row: N 4-byte words in the first half of the slot, the other half poisoned (a kernel that reads 8-byte words there cannot pass)"""
    out = np.empty(N, dtype=np.uint64)
    v = out.view(np.uint32)
    v[:N] = np.array([int(x) for x in values], dtype=np.uint32)[IDX]
    v[N:] = POISON
    return out


def unrow32(words):
    return np.ascontiguousarray(words, dtype=np.uint64).view(np.uint32)[:N].astype(np.uint64)


def check(got, want_cols, what):
    """a result row (N words) against the M column values it must hold; exact"""
    want = row(want_cols)
    bad = np.flatnonzero(np.asarray(got, dtype=np.uint64) != want)
    assert bad.size == 0, f"{what}: {bad.size} of {N} residues differ, first at {bad[:4]} (classes {bad[:4] % M % NCLASS}): got {np.asarray(got)[bad[:4]]} want {want[bad[:4]]}"


def redc(T, q):
    """hc_mont_redc as the hardware computes it, for ANY T below 2^128: exact T 2^-64 mod q while T < q 2^64, and what an overlong sum would give beyond it"""
    lo, hi = T % R64, T >> 64
    h = (lo * pow(q, -1, R64) % R64) * q >> 64
    return (hi - h + (q if hi < h else 0)) % R64


def lazy_model(X, Y, q, per, packed=False, start=None):
    """what a kernel with reduction period `per` (None: one group) returns per column: 128-bit sums through hc_mont_redc, or (packed) 64-bit sums modulo 2^64 through an exact
    remainder; the groups' results are joined by hc_addmod - ONE conditional subtraction - onto `start` (None: the first group's result is taken as it is, as the inner products
    do). With the kernels' own period this equals the reference; with a longer one it is the WRONG word - not even canonical - that the planted columns must expose"""
    out = None if start is None else obj([start] * X.shape[1])
    for g in groups(X.shape[0], per):
        T = sum(X[t] * Y[t] for t in g)
        r = obj([(int(v) % R64) % q for v in T]) if packed else obj([redc(int(v) % (1 << 128), q) for v in T])
        out = r if out is None else obj([(int(v) - q if int(v) >= q else int(v)) % R64 for v in out + r])
    return out


# ================================================================ section 3: the key switch's inner products through the probe
class SumProbe:
    """ctypes binding of one build of tests/arith_probe/sum_probe.hip"""

    def __init__(self, lib_path):
        self.L = C.CDLL(lib_path)
        v, i, u = C.c_void_p, C.c_int, C.c_uint64
        self.L.sum_probe_mac_all.restype = i
        self.L.sum_probe_mac_all.argtypes = [i, v, i, i, i, i, i, i, i, v, u, v, u, u, v, u, u, v, u, u, v, v, u, u, u, i]
        self.L.sum_probe_mac_multi.restype = i
        self.L.sum_probe_mac_multi.argtypes = [i, i, i, i, v, i, i, i, i, i, i, i, i, v, u, u, v, u, u, v, u, u, v, u, u, u, v, v, u, u, i]


def build_host_twin():
    subprocess.check_call(["make", "-s", "-C", PROBE_DIR, HOST_LIB])
    return HOST_LIB


def mod_table(qs, row32_flags):
    """HcMod as the kernels read it: q, q^-1 mod 2^64, 2^128 mod q, N^-1 and its companion, floor(2^64 / q), row32"""
    t = []
    for q, r in zip(qs, row32_flags):
        ninv = pow(N, -1, q)
        t += [q, pow(q, -1, R64), pow(2, 128, q), ninv, (ninv << 64) // q, R64 // q, int(r)]
    return np.array(t, dtype=np.uint64)


def _ptr(a):
    return None if a is None else a.ctypes.data


# nl = 2, alpha = 1, nt = 3: Q limbs 0 and 1 (each its own digit: digit T of limb T reads cx), one P limb. Each triple holds a 4-byte limb, an 8-byte limb below 2^32 or at 2^60, and
# a limb just below 2^61
TRIPLES = {"top32": ([Q_TOP32, Q_LOW64], P_CHAIN[0]), "bits20": ([P_CHAIN[1], Q_20], Q_60)}
NL, NT, ALPHA = 2, 3, 1
BETAS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13]            # both sides of PER and of 2 PER for both accumulators; above 6: hc_k_ks_mac_multi's LONG fallback on 8-byte rows
ROWS = [(0, 0), (1, 0), (1, 1)]                        # (pk, row32 of the small limb): 8-byte rows throughout | packed digits and keys | and 4-byte cx, acc, add, pc0 too
ROWS_ID = {(0, 0): "rows8", (1, 0): "pk", (1, 1): "pk-row32"}
MAC_ALL_SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (4, 3), (4, 4), (4, 5), (8, 7), (8, 8), (8, 9)]         # (NB, n): every NB of HC_MAC_ALL, n below, at and above it
# (R, NB, nrot, n, fin, pc0): every (R, NB) of HC_MAC_MULTI with nrot below and at R; plain accumulators, HcRotFin with pc0 and without
MAC_MULTI_SHAPES = [(R, NB, nrot, max(1, NB - (i + j) % 2), fin, pc0) for i, (R, NB) in enumerate([(2, 8), (4, 4), (8, 2), (8, 1)]) for j, nrot in enumerate((R, max(1, R // 2 + 1) if R > 2 else 1))
                    for fin, pc0 in ((0, 0), (1, 1), (1, 0))]


def key_period(q, packed):
    return 4 if packed else 6


def stored_key(y, q, packed):
    """the stored word of a key whose MULTIPLICAND is y. 8-byte rows: the stored word is used as it is. 4-byte rows: hc_k_pack32_rows turns a stored k into the plain k 2^-64, so
    store y 2^64 mod q and pack it the way that kernel does"""
    if not packed:
        return y
    stored = (y << 64) % q
    plain = stored * pow(R64, -1, q) % q          # hc_k_pack32_rows: hc_mont_redc of the stored word
    assert plain == y
    return plain


def mac_inputs(q_all, rowsel, beta, n, nrot, seed):
    """the operands of one launch for every limb T: per rotation the key columns K[r][T] = (Yb, Ya) as multiplied, per image the digit columns Xd[g][T], and the device arrays"""
    pk, r32 = rowsel
    keys = np.full((nrot, beta, 2, NT, N), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    digits = np.full((n, beta + 1, NT, N), 0x0BAD0BAD0BAD0BAD, dtype=np.uint64)         # one row group of padding per image: dg_is = (beta + 1) nt N
    cx = np.full((n, NL + 1, N), 0x0BAD0BAD0BAD0BAD, dtype=np.uint64)                   # cx_is = (nl + 1) N
    cols = {}
    for T, q in enumerate(q_all):
        packed = bool(pk and small(q))
        u32 = packed and r32
        per = key_period(q, packed)
        for g in range(n):
            X, _ = pattern(q, beta, seed + 1000 * T + 10 * g, shift=g)
            for d in range(beta):
                if T < NL and d == T // ALPHA:
                    cx[g, T] = row32(X[d]) if u32 else row(X[d])                   # the digit's own limb: read from cx, in the caller's row form
                else:
                    digits[g, d, T] = row32(X[d]) if packed else row(X[d])
            cols[("x", g, T)] = X
        for r in range(nrot):
            _, Yb = pattern(q, beta, seed + 1000 * T + 100 * r + 1, shift=3 * r)
            _, Ya = pattern(q, beta, seed + 1000 * T + 100 * r + 5, shift=3 * r + 1)
            for d in range(beta):
                for comp, Y in enumerate((Yb, Ya)):
                    w = [stored_key(int(y), q, packed) for y in Y[d]]
                    keys[r, d, comp, T] = row32(w) if packed else row(w)
            cols[("k", r, T)] = (Yb, Ya)
        for g in range(n):                    # every image against every rotation: the planted maximum in every reduction group, both components
            for r in range(nrot):
                for comp in range(2):
                    assert_planted(cols[("x", g, T)], cols[("k", r, T)][comp], q, groups(beta, per), f"inner product limb {T} (q={q:#x}) image {g} rotation {r} component {comp}")
    return keys, digits, cx, cols


def mac_reference(cols, T, q, packed, g, r, comp, model=None):
    """sum_d x_d k_d 2^-64 mod q on 8-byte rows, sum_d x_d k_d mod q on packed rows; model = a reduction period: what a kernel with that period would return instead"""
    X, Y = cols[("x", g, T)], cols[("k", r, T)][comp]
    if model is not None:
        return lazy_model(X, Y, q, model, packed)
    s = sum(X[d] * Y[d] for d in range(X.shape[0]))
    return s % q if packed else s * pow(R64, -1, q) % q


def perm_src(g):
    """ring.PermuteNTTIndex for N = 2^16: source index of every destination i under the Galois element g"""
    def brev16(x):
        x = ((x >> 1) & 0x5555) | ((x & 0x5555) << 1)
        x = ((x >> 2) & 0x3333) | ((x & 0x3333) << 2)
        x = ((x >> 4) & 0x0F0F) | ((x & 0x0F0F) << 4)
        return ((x >> 8) & 0x00FF) | ((x & 0x00FF) << 8)
    i = np.arange(N, dtype=np.int64)
    return brev16(((g * (2 * brev16(i) + 1)) & 0x1FFFF) >> 1)


def case_mac_all(P, triple, rowsel, beta, NB, n, prep=None, seed=0xA11, tamper=None, model=None):
    """hc_k_ks_mac_all<NB> on n images. prep: None, "add" or "noadd" - HcMacPrep on the last Q limb: acc_L * pinv (+ add_L). tamper(acc): alters the result before it is checked;
    model: a reduction period - returns True when a kernel with that period would be caught by this case's columns"""
    Q, p = TRIPLES[triple]
    q_all = Q + [p]
    pk, r32 = rowsel
    mods = mod_table(q_all, [r32 and small(q) for q in q_all])
    keys, digits, cx, cols = mac_inputs(q_all, rowsel, beta, n, 1, seed + 17 * beta)
    acc = np.full((n, 2 * NT + 1, N), 0x1234567, dtype=np.uint64)                      # acc_is = (2 nt + 1) N
    pinv = add = None
    addc = {}
    if prep:
        pinv = np.zeros((NT, 2), dtype=np.uint64)
        for T, q in enumerate(q_all):
            w = q - 1 if T == NL - 1 else int(splitmix_rows(seed + T, q, 1)[0])
            pinv[T] = (w, (w << 64) // q)
        if prep == "add":
            add = np.full((n, 2 * NL + 1, N), 0x0BAD0BAD0BAD0BAD, dtype=np.uint64)      # add_is = (2 nl + 1) N, add_zs = nl N
            qL = q_all[NL - 1]
            for g in range(n):
                for comp in range(2):
                    a = np.where(np.arange(M) % 2 == 0, qL - 1, splitmix_rows(seed + 99 + g + 2 * comp, qL, M).astype(object))
                    addc[(g, comp)] = obj(a)
                    add[g, comp * NL + NL - 1] = row32(a) if (pk and r32 and small(qL)) else row(a)
    if model is None:
        rc = P.L.sum_probe_mac_all(NB, _ptr(mods), len(q_all), NL, NL, NT, ALPHA, beta, n, _ptr(keys), keys[0].size, _ptr(cx), cx[0].size, cx.size, _ptr(digits), digits[0].size, digits.size,
                                   _ptr(acc), acc[0].size, acc.size, _ptr(pinv), _ptr(add), NL * N, 0 if add is None else add[0].size, 0 if add is None else add.size, pk)
        assert rc == 0, f"sum_probe_mac_all returned {rc}"
        if tamper:
            tamper(acc)
    caught = False
    for T, q in enumerate(q_all):
        packed, u32 = bool(pk and small(q)), bool(pk and small(q) and r32)
        for g in range(n):
            for comp in range(2):
                want = mac_reference(cols, T, q, packed, g, 0, comp)
                if model is not None:
                    caught = caught or bool(np.any(mac_reference(cols, T, q, packed, g, 0, comp, model=model) != want))
                    continue
                if prep and T == NL - 1:
                    want = want * int(pinv[T, 0]) % q
                    if prep == "add":
                        want = (want + addc[(g, comp)]) % q
                got = acc[g, comp * NT + T]
                check(unrow32(got) if u32 else got, want, f"mac_all<{NB}> beta={beta} n={n} limb {T} (q={q:#x}) image {g} component {comp}")
    if model is not None:
        return caught
    assert np.all(acc[:, 2 * NT] == 0x1234567), "mac_all wrote into the padding between the images' accumulators"


def case_mac_multi(P, triple, rowsel, beta, shape, lazy=None, seed=0xB22, tamper=None):
    """hc_k_ks_mac_multi<R, NB, FIN, LAZY> on nrot rotations and n images. lazy None: as the host sets it (beta >= 3). fin: the result of rotation r leaves as
    Permute_g(acc_r + pc0 on the Q rows of component 0), stored at hc_perm_src(j, g^-1)"""
    R, NB, nrot, n, fin, with_pc0 = shape
    lazy = (beta >= 3) if lazy is None else lazy
    Q, p = TRIPLES[triple]
    q_all = Q + [p]
    pk, r32 = rowsel
    mods = mod_table(q_all, [r32 and small(q) for q in q_all])
    keys, digits, cx, cols = mac_inputs(q_all, rowsel, beta, n, nrot, seed + 17 * beta)
    out = np.full((nrot, n, 2 * NT + 1, N), 0x1234567, dtype=np.uint64)
    gals = [pow(5, 3 * r + 1, 2 * N) if r % 2 == 0 else (2 * N - pow(5, r, 2 * N)) % (2 * N) for r in range(nrot)]
    ginv = np.array([pow(g, -1, 2 * N) for g in gals], dtype=np.uint32)
    pc0 = None
    pcc = {}
    if with_pc0:
        pc0 = np.full((n, NL + 1, N), 0x0BAD0BAD0BAD0BAD, dtype=np.uint64)
        for g in range(n):
            for T in range(NL):
                q = q_all[T]
                a = obj(np.where(np.arange(M) % 2 == 0, q - 1, splitmix_rows(seed + 77 + g + 5 * T, q, M).astype(object)))
                pcc[(g, T)] = a
                pc0[g, T] = row32(a) if (pk and r32 and small(q)) else row(a)
    rc = P.L.sum_probe_mac_multi(R, NB, fin, int(lazy), _ptr(mods), len(q_all), NL, NL, NT, ALPHA, beta, n, nrot, _ptr(keys), keys[0].size, keys.size, _ptr(cx), cx[0].size, cx.size,
                                 _ptr(digits), digits[0].size, digits.size, _ptr(out), out[0].size, out[0, 0].size, out.size, _ptr(ginv), _ptr(pc0), 0 if pc0 is None else pc0[0].size,
                                 0 if pc0 is None else pc0.size, pk)
    assert rc == 0, f"sum_probe_mac_multi returned {rc}"
    if tamper:
        tamper(out)
    for T, q in enumerate(q_all):
        packed, u32 = bool(pk and small(q)), bool(pk and small(q) and r32)
        for r in range(nrot):
            src = perm_src(gals[r])
            for g in range(n):
                for comp in range(2):
                    want = mac_reference(cols, T, q, packed, g, r, comp)
                    if fin and with_pc0 and comp == 0 and T < NL:
                        want = (want + pcc[(g, T)]) % q
                    got = out[r, g, comp * NT + T]
                    got = unrow32(got) if u32 else got
                    what = f"mac_multi<{R},{NB},{fin},{int(lazy)}> beta={beta} nrot={nrot} n={n} limb {T} (q={q:#x}) rotation {r} image {g} component {comp}"
                    if fin:
                        want_row = row(want)[src]
                        bad = np.flatnonzero(got != want_row)
                        assert bad.size == 0, f"{what}: {bad.size} of {N} residues differ from Permute(acc + pc0), first at {bad[:4]}: got {got[bad[:4]]} want {want_row[bad[:4]]}"
                    else:
                        check(got, want, what)
    assert np.all(out[:, :, 2 * NT] == 0x1234567), "mac_multi wrote into the padding between the images' results"


# ================================================================ section 2: the sums behind the C ABI
def mform_preimage(y, q):
    """the plaintext word that MForm (hc_mont(pt, 2^128 mod q)) turns into the multiplicand y"""
    return y * pow(R64, -1, q) % q


class QpSums:
    """The operands of hc_qp_mul_sum* on one context at its top level, built once: NA rotated ciphertexts of three images (QS words apart, padded), which the terms repeat, and 64
    plaintexts whose MForm is the planted multiplicand. Term t multiplies a[t mod NA] by plaintext u (the caller says which u)."""
    NA, NPT, NIMG = 4, 64, 3

    def __init__(self, ctx):
        self.ctx, self.level = ctx, len(ctx.q) - 1
        self.nl, self.nt = len(ctx.q), len(ctx.q) + len(ctx.p)
        self.mods = list(ctx.q) + list(ctx.p)
        self.QS = (2 * self.nt + 3) * N
        self.X = {}                 # (b, image, comp, row) -> columns
        self.Y = {}                 # (u, row) -> columns of the multiplicand
        a = np.full((self.NA, self.NIMG, self.QS), 0xDEADBEEFCAFE, dtype=np.uint64)
        pt = np.zeros((self.NPT, self.nt, N), dtype=np.uint64)
        for T, q in enumerate(self.mods):
            for z in range(self.NIMG):
                for comp in range(2):
                    X, _ = pattern(q, self.NA, 0xD1A6 + 1000 * T + 10 * z + comp)
                    for b in range(self.NA):
                        xb = obj([q - 1 if c % NCLASS in (2, 4) else X[b, c] for c in range(M)])       # the terms repeat a[]: what moves with the term sits in the plaintexts
                        self.X[(b, z, comp, T)] = xb
                        a[b, z, (comp * self.nt + T) * N:(comp * self.nt + T + 1) * N] = row(xb)
            _, Y = pattern(q, self.NPT, 0xD1A6 + 1000 * T + 7, period=self.NPT)
            for u in range(self.NPT):
                stored = obj([mform_preimage(int(y), q) for y in Y[u]])
                self.Y[(u, T)] = stored * R64 % q                       # what MForm makes of the stored word: the multiplicand
                assert np.all(self.Y[(u, T)] == Y[u])
                pt[u, T] = row(stored)
        self.a = [ctx.buf(np.concatenate([np.concatenate([ctx.pack_rows(a[b, z, :2 * self.nt * N].reshape(-1, N), self.nl, self.nt).reshape(-1), a[b, z, 2 * self.nt * N:]])
                                          for z in range(self.NIMG)])) for b in range(self.NA)]
        self.pt = [ctx.buf(ctx.pack_rows(pt[u], self.nl, self.nt)) for u in range(self.NPT)]

    def free(self):
        for b in self.a + self.pt:
            b.free()

    def run(self, nterms, plan, accumulate, n=1, tamper=None):
        """plan[h][t]: the plaintext index of giant step h for term t, or None (no diagonal). One giant step: hc_qp_mul_sum; two: hc_qp_mul_sum2; more: hc_qp_mul_sum_many.
        An accumulating output starts at q - 1 everywhere. Checks every output against sum_t a_t pt_h,t mod q and the padding between the images"""
        ctx, G = self.ctx, len(plan)
        init = np.full((self.NIMG, self.QS), 0x5EED5EED, dtype=np.uint64)
        start = np.stack([np.full(N, q - 1, dtype=np.uint64) for _ in range(2) for q in self.mods])
        outs, filled = [], []
        for h in range(G):
            o = init.copy()
            if accumulate[h]:
                o[:, :2 * self.nt * N] = ctx.pack_rows(start, self.nl, self.nt).reshape(-1)
            outs.append(ctx.buf(o))
            filled.append(o)
        vp = C.c_void_p
        arr = lambda xs: (vp * len(xs))(*xs)
        a = arr([self.a[t % self.NA].ptr for t in range(nterms)])
        pts = [[None if plan[h][t] is None else self.pt[plan[h][t]].ptr for t in range(nterms)] for h in range(G)]
        for T, q in enumerate(self.mods):                # the planted maximum, per limb, component, image and giant step, in every group of seven terms
            for h in range(G):
                for z in range(n):
                    for comp in range(2):
                        Xs = [self.X[(t % self.NA, z, comp, T)] for t in range(nterms)]
                        Ys = [self.Y[(plan[h][t] or 0, T)] for t in range(nterms)]
                        assert_planted(Xs, Ys, q, groups(nterms, 7, [plan[h][t] is not None for t in range(nterms)]), f"qp_mul_sum limb {T} giant step {h} image {z} component {comp}")
        ctx.set_batch(n, (self.nl + 2) * N, self.QS)
        try:
            if G == 1:
                ctx._ck(ctx.L.hc_qp_mul_sum(ctx.h, self.level, nterms, a, arr(pts[0]), outs[0].ptr, accumulate[0]))
            elif G == 2:
                ctx._ck(ctx.L.hc_qp_mul_sum2(ctx.h, self.level, nterms, a, arr(pts[0]), arr(pts[1]), outs[0].ptr, outs[1].ptr, accumulate[0], accumulate[1]))
            else:
                ctx._ck(ctx.L.hc_qp_mul_sum_many(ctx.h, self.level, nterms, G, a, arr([p for h in range(G) for p in pts[h]]), arr([o.ptr for o in outs]), (C.c_int * G)(*accumulate)))
            ctx.sync()
        finally:
            ctx.set_batch(1)
        for h in range(G):
            full = outs[h].download().reshape(self.NIMG, self.QS)
            outs[h].free()
            if tamper:
                tamper(full)
            assert np.all(full[n:] == filled[h][n:]) and np.all(full[:, 2 * self.nt * N:] == 0x5EED5EED), "qp_mul_sum wrote outside the images it was given"
            for z in range(n):
                got = ctx.unpack_rows(full[z, :2 * self.nt * N].reshape(-1, N), self.nl, self.nt)
                for comp in range(2):
                    for T, q in enumerate(self.mods):
                        s = obj([0] * M)
                        for t in range(nterms):
                            if plan[h][t] is not None:
                                s = s + self.X[(t % self.NA, z, comp, T)] * self.Y[(plan[h][t], T)]           # x_t y_t with y_t = pt_t 2^64: the kernel's own products
                        want = ((q - 1 if accumulate[h] else 0) + s * pow(R64, -1, q)) % q
                        check(got[comp * self.nt + T], want, f"qp_mul_sum G={G} nterms={nterms} giant step {h} image {z} component {comp} limb {T} (q={q:#x})")


QP_COUNTS = [1, 6, 7, 8, 13, 14, 15, 64]


def qp_plan(G, nterms, variant):
    """the diagonals of G giant steps over nterms baby steps. Giant step h takes plaintext (t + 9 h) mod 64 for term t. Variant "edges": giant step 0 has no diagonal on the first
    and last term of a group (t = 0, 6, 7, 13). Variant "nullgroup": the LAST giant step has none in its whole first group (for 7 terms or fewer: none but the last term) and,
    from three giant steps on, giant step 1 misses the edges. Every term keeps a diagonal in some giant step."""
    plan = [[(t + 9 * h) % 64 for t in range(nterms)] for h in range(G)]
    edges = [t for t in (0, 6, 7, 13) if t < nterms]
    if G > 1 and variant == "edges":
        for t in edges:
            plan[0][t] = None
    if G > 1 and variant == "nullgroup":
        for t in range(7 if nterms > 7 else nterms - 1):
            plan[G - 1][t] = None
        if G > 2:
            for t in edges:
                plan[1][t] = None
    return plan


class LinComb:
    """hc_lv_lincomb2's operands at the top level of a context: eight terms of two polynomials, the extremes planted in the ciphertext columns (the multiplicands are per-limb
    constants)"""

    def __init__(self, ctx):
        self.ctx, self.nl, self.level = ctx, len(ctx.q), len(ctx.q) - 1
        self.X, self.bufs = {}, []
        for k in range(2):
            rows_ = np.zeros((8, self.nl, N), dtype=np.uint64)
            for l, q in enumerate(ctx.q):
                X, _ = pattern(q, 8, 0x11C0 + 100 * l + k)
                for t in range(8):
                    self.X[(t, k, l)] = X[t]
                    rows_[t, l] = row(X[t])
            self.bufs.append([ctx.buf(ctx.pack_rows(rows_[t], self.nl)) for t in range(8)])

    def free(self):
        for b in self.bufs[0] + self.bufs[1]:
            b.free()

    def run(self, nterms, consts, with_addc, alias=False, tamper=None):
        """consts "max": every constant is the c with c 2^64 mod q = q - 1; "uniform": random residues. addc: q - 1 on every limb, or NULL. alias: the outputs are the first
        term's own buffers (each element is read before it is written)"""
        ctx, nl = self.ctx, self.nl
        cm = [[(q - 1) if consts == "max" else int(splitmix_rows(0xC0 + 31 * t + l, q, 1)[0]) for l, q in enumerate(ctx.q)] for t in range(nterms)]       # Montgomery forms: the multiplicands
        cv = np.array([[m * pow(R64, -1, q) % q for m, q in zip(cm[t], ctx.q)] for t in range(nterms)], dtype=np.uint64)
        for t in range(nterms):
            for l, q in enumerate(ctx.q):
                assert (int(cv[t, l]) << 64) % q == cm[t][l]
        if consts == "max":
            for l, q in enumerate(ctx.q):
                for k in range(2):
                    assert_planted([self.X[(t, k, l)] for t in range(nterms)], [obj([cm[t][l]] * M) for t in range(nterms)], q, groups(nterms, None), f"lincomb limb {l} polynomial {k}")
        addc = (C.c_uint64 * nl)(*[q - 1 for q in ctx.q]) if with_addc else None
        if alias:
            keep = [self.bufs[k][0].download() for k in range(2)]
            o = [self.bufs[0][0], self.bufs[1][0]]
        else:
            o = [ctx.buf(np.full(nl * N, 0x1234567, dtype=np.uint64)) for _ in range(2)]
        arr = C.c_void_p * nterms
        ctx._ck(ctx.L.hc_lv_lincomb2(ctx.h, self.level, nterms, arr(*[b.ptr for b in self.bufs[0][:nterms]]), arr(*[b.ptr for b in self.bufs[1][:nterms]]),
                                     cv.ctypes.data_as(C.POINTER(C.c_uint64)), addc, o[0].ptr, o[1].ptr))
        ctx.sync()
        got = [ctx.unpack_rows(o[k].download().reshape(nl, N), nl) for k in range(2)]
        if alias:
            for k in range(2):
                self.bufs[k][0].upload(keep[k])
        else:
            for b in o:
                b.free()
        if tamper:
            tamper(got[0])
        for k in range(2):
            for l, q in enumerate(ctx.q):
                want = sum(self.X[(t, k, l)] * int(cv[t, l]) for t in range(nterms))
                if with_addc and k == 0:
                    want = want + (q - 1)
                check(got[k][l], want % q, f"lv_lincomb2 nterms={nterms} consts={consts} addc={with_addc} polynomial {k} limb {l} (q={q:#x})")


def case_lv_mul_sum(ctx, ntaps, tamper=None):
    """hc_lv_mul_sum at level 1 of the conv context: plain modular accumulation today; the planted columns keep it honest if it is ever made lazy (then in groups of at most
    ntaps: the assertion below takes the whole sum as one group)"""
    qs = [Q0, Q1]
    assert list(ctx.q[:2]) == qs
    NA = 4
    X, Y = {}, {}
    cts = np.zeros((NA, 2, 2, N), dtype=np.uint64)
    pts = np.zeros((ntaps, 2, N), dtype=np.uint64)
    for l, q in enumerate(qs):
        for p in range(2):
            Xp, _ = pattern(q, NA, 0x7A9 + 10 * l + p)
            for b in range(NA):
                X[(b, p, l)] = obj([q - 1 if c % NCLASS in (2, 4) else Xp[b, c] for c in range(M)])
                cts[b, p, l] = row(X[(b, p, l)])
        _, Yl = pattern(q, ntaps, 0x7A9 + 10 * l + 5)
        for t in range(ntaps):
            stored = obj([mform_preimage(int(y), q) for y in Yl[t]])
            Y[(t, l)] = stored * R64 % q
            pts[t, l] = row(stored)
        for p in range(2):
            assert_planted([X[(t % NA, p, l)] for t in range(ntaps)], [Y[(t, l)] for t in range(ntaps)], q, groups(ntaps, None), f"lv_mul_sum limb {l} polynomial {p}")
    bufs = [ctx.buf(c) for c in cts]
    bp, out = ctx.buf(pts), ctx.buf(np.full(4 * N, 0x1234567, dtype=np.uint64))
    ctx._ck(ctx.L.hc_lv_mul_sum(ctx.h, 1, (C.c_void_p * ntaps)(*[bufs[t % NA].ptr for t in range(ntaps)]), bp.ptr, ntaps, out.ptr))
    ctx.sync()
    got = out.download((2, 2, N))
    for b in bufs + [bp, out]:
        b.free()
    if tamper:
        tamper(got[0])
    for p in range(2):
        for l, q in enumerate(qs):
            want = sum(X[(t % NA, p, l)] * Y[(t, l)] for t in range(ntaps)) * pow(R64, -1, q) % q
            check(got[p, l], want, f"lv_mul_sum ntaps={ntaps} polynomial {p} limb {l}")


# ================================================================ the parameter lists both test files run
def _launches():
    i = 0
    for triple in TRIPLES:
        for rowsel in ROWS:
            for beta in BETAS:
                yield i, triple, rowsel, beta
                i += 1


MAC_ALL_PARAMS = [(t, r, b) + MAC_ALL_SHAPES[(i + i // len(MAC_ALL_SHAPES)) % len(MAC_ALL_SHAPES)] for i, t, r, b in _launches()]
MAC_ALL_PREP_PARAMS = [("top32", (0, 0), 7, 4, 5, "add"), ("top32", (1, 1), 5, 2, 2, "noadd"), ("bits20", (1, 0), 4, 1, 1, "add"), ("bits20", (1, 1), 9, 8, 3, "add")]
MAC_MULTI_PARAMS = [(t, r, b, MAC_MULTI_SHAPES[i % len(MAC_MULTI_SHAPES)]) for i, t, r, b in _launches()]
# LAZY forced either way at two and three digits (the host's threshold): rotation tails with pc0 on four images, plain accumulators on one
MAC_MULTI_FORCED = [("top32", r, b, sh, lz) for r in ROWS for b in (2, 3) for lz in (0, 1) for sh in ((4, 4, 3, 4, 1, 1), (8, 1, 8, 1, 0, 0))]
QP_G_PARAMS = [(G, nt_, v) for G in (2, 3, 4) for nt_ in QP_COUNTS for v in ("edges", "nullgroup")]
QP_BATCH_PARAMS = [(G, nt_) for G in (2, 3, 4) for nt_ in (7, 8, 15)]
LIN_PARAMS = [(nt_, c, a) for nt_ in range(1, 9) for c in ("max", "uniform") for a in (True, False)]


def mac_all_id(p):
    return f"{p[0]}-{ROWS_ID[p[1]]}-beta{p[2]}-NB{p[3]}-n{p[4]}" + (f"-{p[5]}" if len(p) > 5 else "")


def mac_multi_id(p):
    R, NB, nrot, n, fin, pc0 = p[3]
    return f"{p[0]}-{ROWS_ID[p[1]]}-beta{p[2]}-R{R}-NB{NB}-nrot{nrot}-n{n}-" + ("acc" if not fin else "fin-pc0" if pc0 else "fin") + (f"-lazy{p[4]}" if len(p) > 4 else "")
