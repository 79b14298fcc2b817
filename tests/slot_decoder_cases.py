"""Cases of hc_decode_slots / hc_decrypt_decode_slots (ckks.Encoder.Decode's float half: plaintextToComplex + the forward special FFT, full and sparse slots), shared by the
GPU suite (tests/test_gpu_slot_decoder.py) and the CPU emulator (tests/test_slot_decoder_cpu.py). The reference for the bits is tests/oracle_bl.py (fft_special restates
Lattigo's fft for any n; decrypt_decode_l1 is the level-1 decryptor); doubles are compared as 64-bit words, with no tolerance. One Env per runner: a context over the BL
column's moduli (the decoder itself reads no modulus), its oracle and one secret key, made at first use and shared by the cases; expected values are computed once."""
import ctypes as C

import numpy as np

import coeff_codec_cases as cc
import oracle_bl
from oracle_bl import P_BL, Q1_BL
from oracle_lib import Q0
from parity_cases import N

SCALE = 2.0 ** 30
KINDS = ("mixed", "zero", "one_at_0", "one_at_half")
LOG_SLOTS = (0, 1, 8, 9, 11, 12, 14, 15)      # 0: no stage; 8 x 3 vectors: 768 values, a short last tile; 11: exactly one tile; 12: the first two-pass size (R = 16); 15: R = 128
COUNTS = (1, 3)
_WANT = {}


class Env:
    def __init__(self, make_ctx, make_oracle):
        self.make_ctx, self.make_oracle, self._bl = make_ctx, make_oracle, None

    def bl(self):
        """(context, oracle, secret key, NTT(s) rows) over Q = [Q0, Q1_BL], P = P_BL"""
        if self._bl is None:
            ctx, O = self.make_ctx([Q0, Q1_BL], list(P_BL)), self.make_oracle([Q0, Q1_BL], list(P_BL))
            sk = O.gen_sk(41)
            self._bl = (ctx, O, sk, ctx.sk_rows(sk))
        return self._bl

    def close(self):
        if self._bl is not None:
            self._bl[0].close()
            self._bl = None


def words(a):
    return np.ascontiguousarray(a).view(np.uint64)


def eq_bits(got, want, what):
    g, w = words(got), words(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g.reshape(-1) != w.reshape(-1))
        raise AssertionError(f"{what}: {bad.size} of {g.size} words differ, first at {bad[:8]}")


def grid_values(kind, n, seed):
    """the 2 n coefficients on the gap grid: real parts (coefficients i gap), then imaginary parts (N/2 + i gap)"""
    if kind == "mixed":                                                                         # uniform mantissas over 60 binades, both signs
        rng = np.random.default_rng(seed)
        return rng.uniform(-1, 1, 2 * n) * 2.0 ** rng.integers(-30, 30, 2 * n)
    v = np.zeros(2 * n)
    if kind == "one_at_0":
        v[0] = 1.0
    elif kind == "one_at_half":
        v[n] = 1.0
    return v


def coeff_vector(key, log_slots):
    """[N] doubles: the grid values at stride gap, and for log_slots < 15 non-zero garbage on every coefficient off the grid (the oracle never sees it)"""
    n, gap = 1 << log_slots, (N // 2) >> log_slots
    rng = np.random.default_rng(7000 + key[1])
    cf = rng.uniform(1.0, 2.0, N) * rng.choice([-1e30, 1e-3, 3.0], N)
    cf[::gap] = grid_values(key[0], n, key[1])
    return cf


def expected(key, log_slots):
    k = (key, log_slots)
    if k not in _WANT:
        n = 1 << log_slots
        g = grid_values(key[0], n, key[1])
        w = np.ascontiguousarray(oracle_bl.fft_special(g[:n] + 1j * g[n:]))
        w.setflags(write=False)
        _WANT[k] = w
    return _WANT[k]


def calls(log_slots, count):
    """the four kinds of input in calls of `count` vectors, the last call filled up with further seeded vectors"""
    todo = [(k, 100 + log_slots) for k in KINDS]
    while len(todo) % count:
        todo.append(("mixed", 200 + log_slots + len(todo)))
    return [todo[i:i + count] for i in range(0, len(todo), count)]


def case_decode(env, log_slots, count):
    """hc_decode_slots == oracle_bl.fft_special of the gap-grid coefficients, word for word; at log_slots 15 also == oracle_bl.decode_slots of the whole vector"""
    ctx = env.bl()[0]
    for call in calls(log_slots, count):
        cf = np.stack([coeff_vector(t, log_slots) for t in call])
        got = ctx.decode_slots(cf, log_slots)
        assert got.shape == (count, 1 << log_slots) and got.dtype == np.complex128
        for z, t in enumerate(call):
            eq_bits(got[z], expected(t, log_slots), f"log_slots {log_slots} count {count} vector {z} ({t[0]})")
        if log_slots == 15:
            eq_bits(got[0], oracle_bl.decode_slots(cf[0]), "log_slots 15 == oracle_bl.decode_slots")


def _values(n, count, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (count, n)) + 1j * rng.uniform(-1, 1, (count, n))


def case_decrypt_composed(env, level, log_slots):
    """hc_decrypt_decode_slots == hc_decode_slots(hc_decrypt_decode_coeffs(...)) bit for bit, count 2, on device encryptions of encoded slot vectors; a scale that is no
    power of two, so the division rounds"""
    ctx, O, sk, sk_rows = env.bl()
    pt = ctx.encode_slots_ex(_values(1 << log_slots, 2, 300 + log_slots), log_slots, level, False, SCALE, to_ntt=False)
    cts = ctx.encrypt_sk(pt, level, sk_rows, list(range(1, 9)), 50 + level)
    scale = SCALE * 1.37
    got = ctx.decrypt_decode_slots(cts, level, sk_rows, scale, log_slots)
    two = ctx.decode_slots(ctx.decrypt_decode_coeffs(cts, level, sk_rows, scale), log_slots)
    assert got.shape == (2, 1 << log_slots)
    eq_bits(got, two, f"level {level} log_slots {log_slots}: one call against the two calls composed")
    assert np.abs(got).max() > 0


def case_decrypt_l1_oracle(env):
    """level 1 on the BL moduli, full slots: a ciphertext the oracle encrypted, decrypted and decoded by oracle_bl.decrypt_decode_l1 (CRT in Python integers, float(int),
    fft_special) and by ONE hc_decrypt_decode_slots call over two copies: the same words; and the values are the encoded ones to the encoder's precision"""
    ctx, O, sk, sk_rows = env.bl()
    vals = _values(N // 2, 1, 77)[0]
    m = np.stack(oracle_bl.encode_slots(O, vals, 1, SCALE))
    ct = O.encrypt(sk, m, 1, 902)

    class _BL:
        pass
    bl = _BL(); bl.O = O
    want = oracle_bl.decrypt_decode_l1(bl, sk, ct, SCALE)
    got = ctx.decrypt_decode_slots(np.stack([ct, ct]), 1, sk_rows, SCALE, 15)
    for z in range(2):
        eq_bits(got[z], want, f"level 1, image {z}: hc_decrypt_decode_slots against oracle_bl.decrypt_decode_l1")
    assert np.abs(want - vals).max() < 2.0 ** -10, "the oracle did not decode what it encoded"


def case_round_trip(env, log_slots):
    """independent of the oracle's FFT: |re|, |im| <= 1 -> hc_encode_slots_ex (level 0, scale 2^30, NTT domain) -> the ciphertext (rows, 0) -> hc_decrypt_decode_slots.
    Bound 2^(log_slots - 29): each slot sums 2 n coefficient rounding errors of at most 2^-31 with unit-modulus weights, n 2^-30, doubled for margin; the fp64 error of
    the two transforms is orders of magnitude below. (With the oracle alone the maximum is 2^-31.5 at log_slots 0 and 2^-22 at log_slots 15.)"""
    ctx, O, sk, sk_rows = env.bl()
    vals = _values(1 << log_slots, 2, 500 + log_slots)
    rows = ctx.encode_slots_ex(vals.copy(), log_slots, 0, False, SCALE, to_ntt=True)
    cts = np.zeros((2, 2, 1, N), dtype=np.uint64)
    cts[:, 0, 0] = rows[:, 0]
    got = ctx.decrypt_decode_slots(cts, 0, sk_rows, SCALE, log_slots)
    err = max(np.abs(got.real - vals.real).max(), np.abs(got.imag - vals.imag).max())
    print(f"round trip, log_slots {log_slots}: max error 2^{np.log2(err):.2f} (bound 2^{log_slots - 29})")
    assert err <= 2.0 ** (log_slots - 29)


def case_refusals(env):
    """log_slots -1 and 16, count 0, null pointers: HC_ERR_ARG (1); level 2: HC_ERR_UNSUPPORTED (4) on a context with more than two limbs (on a two-limb one the level is
    outside the chain: HC_ERR_ARG, as hc_decrypt_decode_coeffs answers); a valid call after each refusal gives the right words"""
    ctx = env.bl()[0]
    key, ls = ("mixed", 9), 9
    cf, want = coeff_vector(key, ls), expected(key, ls)
    L, h = ctx.L, ctx.h
    dc, out = ctx.buf(nwords=N), ctx.buf(nwords=2 * N)
    ct, ds = ctx.buf(nwords=4 * N), ctx.buf(nwords=4 * N)
    one, none = (C.c_void_p * 1)(ct.ptr), (C.c_void_p * 1)(None)

    def valid():
        eq_bits(ctx.decode_slots(cf, ls)[0], want, "a valid call after a refused one")
    for args in ((dc.ptr, 1, -1, out.ptr), (dc.ptr, 1, 16, out.ptr), (dc.ptr, 0, ls, out.ptr), (None, 1, ls, out.ptr), (dc.ptr, 1, ls, None)):
        assert L.hc_decode_slots(h, *args) == 1 and b"hc_decode_slots" in L.hc_last_error(h), args
        valid()
    for args in ((1, 1, one, ds.ptr, SCALE, -1, out.ptr), (1, 1, one, ds.ptr, SCALE, 16, out.ptr), (0, 1, one, ds.ptr, SCALE, ls, out.ptr), (1, 1, None, ds.ptr, SCALE, ls, out.ptr),
                 (1, 1, none, ds.ptr, SCALE, ls, out.ptr), (1, 1, one, None, SCALE, ls, out.ptr), (1, 1, one, ds.ptr, SCALE, ls, None), (1, -1, one, ds.ptr, SCALE, ls, out.ptr),
                 (1, 2, one, ds.ptr, SCALE, ls, out.ptr)):
        assert L.hc_decrypt_decode_slots(h, *args) == 1 and b"hc_decrypt_decode_slots" in L.hc_last_error(h), args
        valid()
    for b in (dc, out, ct, ds):
        b.free()
    Q, P = cc.BOOT_CHAIN
    big = env.make_ctx(Q, P)
    try:
        ct, ds, out = big.buf(nwords=6 * N), big.buf(nwords=(len(Q) + len(P)) * N), big.buf(nwords=2 * N)
        one = (C.c_void_p * 1)(ct.ptr)
        assert big.L.hc_decrypt_decode_slots(big.h, 1, 2, one, ds.ptr, SCALE, ls, out.ptr) == 4 and b"hc_decrypt_decode_slots" in big.L.hc_last_error(big.h)
        eq_bits(big.decode_slots(cf, ls)[0], want, "a valid call after the unsupported level")
        for b in (ct, ds, out):
            b.free()
    finally:
        big.close()
