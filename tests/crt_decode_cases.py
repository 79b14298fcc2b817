"""Cases of hc_decode_coeffs / hc_decrypt_decode_lv (DecodeCoeffs at any level of the context), shared by the GPU suite (tests/test_gpu_crt_decode.py) and the CPU emulator
(tests/test_crt_decode_cpu.py), in the pattern of coeff_codec_cases.py: each takes factories make_ctx(Q, P) -> optimal_conv_amd.Context, make_oracle(Q, P) -> Oracle.

The expected doubles are Python's: the planted integer itself (never a CRT of the residues: the integers over ALL limbs are where the residues come from), float(int) -
correctly rounded, ties to even (test_crt_decode_cpu.py checks that on this interpreter) - with OverflowError mapped to an infinity, the sign, one IEEE division by the
scale. Doubles are compared as 64-bit words. N is fixed at 2^16, so a case is one or three plaintexts; the levels are those at which the kernel takes another path: 2 (the
first the two-limb kernel does not serve), 4 (another word count), 15 (4-byte rows under pack32 = 2), 27 (20 words, magnitudes beyond 2^1024)."""
import functools
import random
import sys

import numpy as np

import oracle_ckks
from coeff_codec_cases import recover_e
from optimal_conv_amd import HconvError
from parity_cases import N

SCALE = 2.0 ** 30 * 1.37                                  # no power of two: the division rounds
P1 = list(oracle_ckks.P_SET6[:1])
CHAIN5 = (list(oracle_ckks.Q_SET6[:5]), P1)               # levels 2 and 4
CHAIN16 = (list(oracle_ckks.Q_SET6[:16]), P1)             # level 15: limbs 5 .. 15 are ~30-bit primes (4-byte rows under pack32 = 2)
CHAIN28 = (list(oracle_ckks.Q_SET6), P1)                  # level 27: Q has 1248 bits
CHAIN29 = (list(oracle_ckks.Q_SET6) + list(oracle_ckks.P_SET6[:1]), list(oracle_ckks.P_SET6[1:2]))      # one limb more than the kernel is built for
ROLLS = (0, 7777, 40001)                                  # image z holds the targets rolled by ROLLS[z]


def to_f64(t):
    """the double DecodeCoeffs owes for the centred integer t, before the division"""
    try:
        return float(t)
    except OverflowError:
        return float("inf") if t > 0 else float("-inf")


def words(x):
    """doubles (or the (re, im) pairs of complex values) as 64-bit words"""
    a = np.ascontiguousarray(x)
    return (a.view(np.float64) if np.iscomplexobj(a) else a.astype(np.float64)).view(np.uint64)


def same(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
    assert not bad.size, f"{what}: {bad.size} doubles differ, first at {bad[:8]}: got {np.asarray(got).reshape(-1)[bad[:4]]}, want {np.asarray(want).reshape(-1)[bad[:4]]}"


def planted(Q, level):
    """(name, integer) pairs, each with both signs where the rule allows: the centre's two sides, the 53-bit ties and their sticky bits, every 64-bit word boundary of the
    magnitude, what a two-limb shortcut gets wrong, and - where Q reaches it - the two sides of the largest finite double"""
    QQ = 1
    for q in Q[: level + 1]:
        QQ *= q
    t0 = 2 ** 80 + 2 ** 27
    mags = [("0", 0), ("1", 1), ("Q/2", QQ // 2), ("Q/2-1", QQ // 2 - 1), ("tie_even", t0), ("tie_sticky", t0 + 1), ("tie_below", t0 - 1), ("tie_up", 2 ** 80 + 3 * 2 ** 27),
            ("q0q1/2+1", Q[0] * Q[1] // 2 + 1), ("q0q1", Q[0] * Q[1]), ("q0q1+1", Q[0] * Q[1] + 1), ("2^53+1", 2 ** 53 + 1)]
    k = 1
    while 2 ** (64 * k) + 1 <= QQ // 2:
        mags += [(f"2^{64 * k}-1", 2 ** (64 * k) - 1), (f"2^{64 * k}", 2 ** (64 * k)), (f"2^{64 * k}+1", 2 ** (64 * k) + 1), (f"2^{64 * k}+2^{64 * k - 53}", 2 ** (64 * k) + 2 ** (64 * k - 53)),
                 (f"2^{64 * k}+2^{64 * k - 53}+1", 2 ** (64 * k) + 2 ** (64 * k - 53) + 1)]
        k += 1
    if QQ // 2 > 2 ** 1024:
        mags += [("max_finite", 2 ** 1024 - 2 ** 970 - 1), ("first_inf", 2 ** 1024 - 2 ** 970), ("2^1024", 2 ** 1024)]
    out = []
    for name, m in mags:
        assert 0 <= m <= QQ // 2, name
        out.append((name, m))
        out.append(("-" + name, -m))
    return out, QQ


@functools.lru_cache(maxsize=None)
def reference(chain_len, level, seed=0xC27):
    """(rows [level+1][N] uint64: the residues of N centred integers in [-(Q//2), Q//2]; mag [N] float64: float(integer), +-inf beyond the doubles; names -> index).
    Coefficients 0 .. : the planted values, then 3000 random values of full width and of every width; the bulk: random 62-bit values (vectorised); the last coefficients: the
    planted values again, reversed (the last workgroups). Computed once per (chain, level) and shared by every case; never modified."""
    Q = list(oracle_ckks.Q_SET6[:chain_len])
    pl, QQ = planted(Q, level)
    rnd = random.Random(seed * 31 + level)
    T = np.random.default_rng(seed + level).integers(-(1 << 62), 1 << 62, N).tolist()
    head = [m for _, m in pl]
    head += [rnd.randrange(-(QQ // 2), QQ // 2 + 1) for _ in range(2000)]
    head += [rnd.choice((-1, 1)) * rnd.randrange(1 << rnd.randrange(1, QQ.bit_length() - 1)) for _ in range(1000)]
    T[: len(head)] = head
    T[N - len(pl):] = [m for _, m in pl][::-1]
    assert all(-(QQ // 2) <= t <= QQ // 2 for t in T)
    rows = np.array([[t % q for t in T] for q in Q[: level + 1]], dtype=np.uint64)
    mag = np.array([to_f64(t) for t in T], dtype=np.float64)
    idx = {name: i for i, (name, _) in enumerate(pl)}
    rows.setflags(write=False); mag.setflags(write=False)
    return rows, mag, idx


def check_reference(chain_len, level):
    """the planted values came out of the Python side as intended"""
    rows, mag, idx = reference(chain_len, level)
    assert mag[idx["tie_even"]] == 2.0 ** 80 and mag[idx["-tie_even"]] == -(2.0 ** 80), "2^80 + 2^27 is a tie that goes to even: down"
    assert mag[idx["tie_sticky"]] == np.nextafter(2.0 ** 80, np.inf) and mag[idx["tie_below"]] == 2.0 ** 80 and mag[idx["tie_up"]] == 2.0 ** 80 + 2.0 ** 29
    assert mag[idx["2^64+2^11"]] == 2.0 ** 64 and mag[idx["2^64+2^11+1"]] == np.nextafter(2.0 ** 64, np.inf) and mag[idx["2^64-1"]] == 2.0 ** 64
    assert words(mag[idx["0"]]) == 0 and mag[idx["1"]] == 1.0 and mag[idx["-1"]] == -1.0
    Q = oracle_ckks.Q_SET6
    two = Q[0] * Q[1]
    assert rows[0, idx["q0q1"]] == 0 and rows[1, idx["q0q1"]] == 0 and rows[2, idx["q0q1"]] == two % Q[2], "q0 q1 is 0 under limbs 0 and 1: a two-limb shortcut decodes 0"
    assert mag[idx["q0q1"]] == float(two)
    if level == 27:
        assert mag[idx["max_finite"]] == sys.float_info.max and mag[idx["-max_finite"]] == -sys.float_info.max
        assert mag[idx["first_inf"]] == np.inf and mag[idx["-first_inf"]] == -np.inf and mag[idx["Q/2"]] == np.inf and mag[idx["-Q/2"]] == -np.inf
    else:
        assert np.isfinite(mag).all()


def images(a, count):
    return np.stack([np.roll(a, ROLLS[z], axis=-1) for z in range(count)])


def case_planted(make_ctx, make_oracle, chain, level, count, pack32=1, expect32=False):
    """hc_decode_coeffs of planted residues (no encryption): coefficient-domain input == Python's doubles, word for word; NTT-domain input (the oracle's transform of the
    same rows) == the same words. Under pack32 = 2 the binding hands the rows of hc_row_is32 limbs over as 4-byte words, the unused half of each slot poisoned."""
    Q, P = chain
    check_reference(len(Q), level)
    rows, mag, _ = reference(len(Q), level)
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        if pack32 != 1:
            ctx.set_option("pack32", pack32)
        assert any(ctx.row32()[: level + 1]) == expect32, "4-byte rows: the case is meant to cross them exactly when expect32"
        with np.errstate(over="ignore"):
            want = images(mag, count) / np.float64(SCALE)
        pt = images(rows, count)
        got = ctx.decode_coeffs(pt, level, SCALE, from_ntt=False)
        same(got, want, f"decode_coeffs, coefficient domain (level {level}, count {count}, pack32 {pack32})")
        pt_ntt = np.stack([[O.ntt(l, pt[z, l]) for l in range(level + 1)] for z in range(count)])
        same(ctx.decode_coeffs(pt_ntt, level, SCALE, from_ntt=True), want, f"decode_coeffs, NTT domain (level {level}, count {count}, pack32 {pack32})")
    finally:
        ctx.close()


def case_low_levels(make_ctx, make_oracle):
    """levels 0 and 1: hc_decode_coeffs and hc_decrypt_decode_lv give hc_decrypt_decode_coeffs' words (random residues: every CRT value of two limbs, both sides of Q/2)"""
    Q, P = CHAIN5
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        rng = np.random.default_rng(11)
        sk_rows = ctx.sk_rows(O.gen_sk(41))
        for level in (0, 1):
            nl = level + 1
            cts = np.stack([[[rng.integers(0, Q[l], N, dtype=np.uint64) for l in range(nl)] for _ in range(2)] for _ in range(2)])      # [2 images][2][nl][N]
            want = ctx.decrypt_decode_coeffs(cts, level, sk_rows, SCALE)
            same(ctx.decrypt_decode_lv(cts[:, 0], cts[:, 1], level, sk_rows, SCALE), want, f"decrypt_decode_lv at level {level}")
            m = np.stack([ctx.lv_add(level, cts[z, 0], ctx.lv_mul(level, cts[z, 1], sk_rows[:nl])) for z in range(2)])
            same(ctx.decode_coeffs(m, level, SCALE, from_ntt=True), want, f"decode_coeffs(from_ntt = 1) at level {level}")
            mc = np.stack([ctx.lv_intt(level, m[z]) for z in range(2)])
            same(ctx.decode_coeffs(mc, level, SCALE, from_ntt=False), want, f"decode_coeffs(from_ntt = 0) at level {level}")
            same(ctx.decrypt_decode_lv(cts[:, 0], cts[:, 1], level, sk_rows, SCALE, log_slots=12), ctx.decrypt_decode_slots(cts, level, sk_rows, SCALE, 12).view(np.float64),
                 f"decrypt_decode_lv(log_slots = 12) at level {level}")
    finally:
        ctx.close()


def case_decrypt_relation(make_ctx, make_oracle, chain, level, pack32=1):
    """hc_decrypt_decode_lv == hc_decode_coeffs of c0 + c1 s formed with the leveled entry points, for random canonical c0, c1 (count 3, each polynomial in an allocation of
    its own); log_slots 12 and 15 == hc_decode_slots of those coefficients"""
    Q, P = chain
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        if pack32 != 1:
            ctx.set_option("pack32", pack32)
        nl = level + 1
        rng = np.random.default_rng(12 + level)
        sk_rows = ctx.sk_rows(O.gen_sk(42))
        c = np.stack([[[rng.integers(0, Q[l], N, dtype=np.uint64) for l in range(nl)] for _ in range(2)] for _ in range(3)])
        m = np.stack([ctx.lv_add(level, c[z, 0], ctx.lv_mul(level, c[z, 1], sk_rows[:nl])) for z in range(3)])
        want = ctx.decode_coeffs(m, level, SCALE, from_ntt=True)
        assert np.isfinite(want).all() or level > 22
        got = ctx.decrypt_decode_lv(c[:, 0], c[:, 1], level, sk_rows, SCALE)
        same(got, want, f"decrypt_decode_lv == decode_coeffs(c0 + c1 s) (level {level}, pack32 {pack32})")
        if level <= 22:
            for ls in (12, 15):
                same(ctx.decrypt_decode_lv(c[:, 0], c[:, 1], level, sk_rows, SCALE, log_slots=ls).view(np.float64), ctx.decode_slots(want, ls).view(np.float64),
                     f"decrypt_decode_lv(log_slots = {ls}) == decode_slots of the coefficients (level {level})")
    finally:
        ctx.close()


def case_decrypt_l4(make_ctx, make_oracle):
    """one oracle encryption at level 4 whose decryption is the planted targets exactly (m = target - e under every limb, e the oracle's error for that seed, as
    coeff_codec_cases.case_decrypt_l1 plants them): hc_decrypt_decode_lv == Python's doubles, bit for bit"""
    Q, P = CHAIN5
    level = 4
    check_reference(len(Q), level)
    rows, mag, _ = reference(len(Q), level)
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        sk = O.gen_sk(43)
        sk_rows = ctx.sk_rows(sk)
        zero = np.zeros((level + 1, N), dtype=np.uint64)
        e = recover_e(O, sk_rows, O.encrypt(sk, zero, level, 904), zero, level)
        for l in range(1, level + 1):
            assert np.array_equal(e[l], e[0])
        assert 0 < np.abs(e[0]).max() <= 19
        m = np.stack([((rows[l].astype(object) - e[0].astype(object)) % Q[l]).astype(np.uint64) for l in range(level + 1)])
        ct = O.encrypt(sk, m, level, 904)
        got = ctx.decrypt_decode_lv(ct[0][None], ct[1][None], level, sk_rows, SCALE)
        same(got[0], mag / np.float64(SCALE), "decrypt_decode_lv of an oracle encryption at level 4")
    finally:
        ctx.close()


def case_refusals(make_ctx, make_oracle):
    """argument errors are HC_ERR_ARG (1), a level the kernel is not built for is HC_ERR_UNSUPPORTED (4), and the context decodes correctly after each"""
    import ctypes as C
    Q, P = CHAIN29
    rows, mag, _ = reference(5, 2)
    ctx = make_ctx(Q, P)
    try:
        want = mag / np.float64(SCALE)
        ok = lambda what: same(ctx.decode_coeffs(rows, 2, SCALE, from_ntt=False)[0], want, what)
        ok("before any refusal")
        big = np.zeros((29, N), dtype=np.uint64)
        with np.testing.assert_raises_regex(HconvError, r"libhconv error 4: hc_decode_coeffs"):
            ctx.decode_coeffs(big, 28, SCALE, from_ntt=False)
        ok("a valid call after an unsupported level")
        with np.testing.assert_raises_regex(HconvError, r"libhconv error 4: hc_decrypt_decode_lv"):
            ctx.decrypt_decode_lv(big, big, 28, np.zeros((30, N), dtype=np.uint64), SCALE)
        ok("a valid call after an unsupported level of the decryptor")
        d, out = ctx.buf(nwords=3 * N), ctx.buf(nwords=N)
        one = (C.c_void_p * 1)(d.ptr); null1 = (C.c_void_p * 1)(None)
        L, h = ctx.L, ctx.h
        assert L.hc_decode_coeffs(h, d.ptr, 0, 2, 0, SCALE, out.ptr) == 1 and b"hc_decode_coeffs" in L.hc_last_error(h)
        assert L.hc_decode_coeffs(h, d.ptr, 1, 29, 0, SCALE, out.ptr) == 1               # a level outside the context
        assert L.hc_decode_coeffs(h, d.ptr, 1, -1, 0, SCALE, out.ptr) == 1
        assert L.hc_decode_coeffs(h, None, 1, 2, 0, SCALE, out.ptr) == 1
        assert L.hc_decode_coeffs(h, d.ptr, 1, 2, 0, SCALE, None) == 1
        assert L.hc_decrypt_decode_lv(h, 0, 2, one, one, d.ptr, SCALE, -1, out.ptr) == 1 and b"hc_decrypt_decode_lv" in L.hc_last_error(h)
        assert L.hc_decrypt_decode_lv(h, 1, 29, one, one, d.ptr, SCALE, -1, out.ptr) == 1
        assert L.hc_decrypt_decode_lv(h, 1, 2, one, null1, d.ptr, SCALE, -1, out.ptr) == 1
        assert L.hc_decrypt_decode_lv(h, 1, 2, None, one, d.ptr, SCALE, -1, out.ptr) == 1
        assert L.hc_decrypt_decode_lv(h, 1, 2, one, one, None, SCALE, -1, out.ptr) == 1
        assert L.hc_decrypt_decode_lv(h, 1, 2, one, one, d.ptr, SCALE, -2, out.ptr) == 1
        assert L.hc_decrypt_decode_lv(h, 1, 2, one, one, d.ptr, SCALE, 16, out.ptr) == 1
        assert L.hc_decrypt_decode_lv(h, 1, 2, one, one, d.ptr, SCALE, -1, None) == 1
        d.free(); out.free()
        ok("a valid call after the argument errors")
    finally:
        ctx.close()
