"""Cases of hc_encode_coeffs / hc_encrypt_sk / hc_decrypt_decode_coeffs, shared by the GPU suite (tests/test_gpu_coeff_codec.py) and the CPU emulator
(tests/test_coeff_codec_cpu.py). Each takes factories, as the cases of parity_cases.py do: make_ctx(Q, P) -> optimal_conv_amd.Context, make_oracle(Q, P) -> Oracle.
N is fixed at 2^16, so the cases are small in ROWS: one to three vectors at levels 0 to 3."""
import numpy as np

import oracle_bl
import oracle_ckks
from oracle_bl import Q1_BL, P_BL
from oracle_lib import P0, Q0, Q1
from optimal_conv_amd import HconvError
from parity_cases import N, eq

SCALE = 2.0 ** 30
LIMIT = 1.8446744073709552e+19          # 2^64 as scaleUpVecExact compares it


def edge_values(scale):
    """what the rounding can get wrong, as values v with the intended |v * scale|: zeros, +-1, exact ties (k + 0.5, both signs), negatives that round to 0,
    2^53 - 1 / 2^53 / 2^53 + 2 (the doubles around 2^53 +- 1), 2^63, and the largest double below 2^64. A product that a scale which is no power of two pushes
    beyond 2^64 is replaced by 0 (that branch is case_refusals' subject)."""
    ints = [0.0, 1.0, 0.5, 1.5, 2.5, 7.5, 12345.5, 0.2, 0.49, 0.49999999999999994, 1e-300, float(2 ** 53 - 1), float(2 ** 53), float(2 ** 53 + 2),
            float(2 ** 63), float(np.nextafter(2.0 ** 63, 0)), float(np.nextafter(2.0 ** 64, 0))]
    v = np.array([s * x / scale for x in ints for s in (1.0, -1.0)], dtype=np.float64)
    with np.errstate(over="ignore"):
        v[np.abs(scale * v) > LIMIT] = 0.0
    return v


def vectors(scale, seed):
    """count = 3 vectors of N values: edges then random values over 40 binades; small random values; values whose product with the scale lies in [2^62, 2^64)"""
    rng = np.random.default_rng(seed)
    e = edge_values(scale)
    v = np.empty((3, N), dtype=np.float64)
    v[0] = rng.uniform(-1, 1, N) * 2.0 ** rng.integers(-8, 32, N)
    v[0, : e.size] = e
    v[0, N - e.size:] = e[::-1]                      # and at the far end of the vector (the last workgroups)
    v[1] = rng.uniform(-4, 4, N)
    v[2] = rng.choice([-1.0, 1.0], N) * rng.uniform(2.0 ** 62, 2.0 ** 64 * (1 - 2.0 ** -40), N) / scale
    with np.errstate(over="ignore"):
        v[2][np.abs(scale * v[2]) > LIMIT] = 1.0
    return v


def case_encoder(make_ctx, make_oracle, Q, P, level, scale, pack32=1, expect32=False, seed=0xC0EF):
    """hc_encode_coeffs == or_encode_coeffs word for word (the word q_l of a negative value that rounds to 0 included), nvals in {0, 1, N - 1, N} with the zero fill,
    to_ntt = 0 and 1, and to_ntt = 1 == hc_lv_ntt of the to_ntt = 0 rows. Under pack32 = 2 the binding reads the rows of hc_row_is32 limbs as 4-byte words."""
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        if pack32 != 1:
            ctx.set_option("pack32", pack32)
        nl = level + 1
        assert any(ctx.row32()[:nl]) == expect32, "4-byte rows: the case is meant to cross them exactly when expect32"
        v = vectors(scale, seed)
        for nvals in (N, N - 1, 1, 0):
            want = np.stack([O.encode_coeffs(v[z, :nvals], scale, list(range(nl))) for z in range(3)])
            got = ctx.encode_coeffs(v[:, :nvals], level, scale, to_ntt=False)
            eq(got, want, f"encode_coeffs, coefficient domain (level {level}, nvals {nvals}, pack32 {pack32})")
            assert not got[:, :, nvals:].any(), "coefficients past nvals must be zero"
            if nvals in (N, 1):
                got_ntt = ctx.encode_coeffs(v[:, :nvals], level, scale, to_ntt=True)
                want_ntt = np.stack([[O.ntt(l, want[z, l]) for l in range(nl)] for z in range(3)])
                eq(got_ntt, want_ntt, f"encode_coeffs, NTT domain (level {level}, nvals {nvals}, pack32 {pack32})")
                if nvals == N:
                    eq(got_ntt, np.stack([ctx.lv_ntt(level, got[z]) for z in range(3)]), "to_ntt = 1 == hc_lv_ntt of the to_ntt = 0 rows")
        if level == 0:       # the word q for a negative value that rounds to 0 is really there (the transform canonicalises it)
            assert (ctx.encode_coeffs(np.array([-0.2 / scale]), 0, scale, to_ntt=False)[0, 0, 0]) == Q[0]
    finally:
        ctx.close()


def case_refusals(make_ctx, make_oracle):
    """a value beyond 2^64 / scale, a NaN, an infinity: HC_ERR_UNSUPPORTED (4) and the context stays usable; nvals = N + 1 and count = 0: HC_ERR_ARG (1)"""
    import ctypes as C
    Q, P = [Q0, Q1], [P0]
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        good = vectors(SCALE, 5)[1, :4096]
        want = O.encode_coeffs(good, SCALE, [0, 1])
        for bad in (2.0 ** 64 / SCALE * (1 + 2.0 ** -50), -(2.0 ** 64) / SCALE * (1 + 2.0 ** -50), float("nan"), float("inf")):
            v = good.copy(); v[1234] = bad
            with np.testing.assert_raises_regex(HconvError, r"libhconv error 4: hc_encode_coeffs"):
                ctx.encode_coeffs(v, 1, SCALE, to_ntt=False)
            eq(ctx.encode_coeffs(good, 1, SCALE, to_ntt=False)[0], want, "a valid call after a refused one")
        dv, out = ctx.buf(nwords=N + 1), ctx.buf(nwords=2 * N)
        assert ctx.L.hc_encode_coeffs(ctx.h, dv.ptr, 1, N + 1, 1, SCALE, 0, out.ptr) == 1 and b"hc_encode_coeffs" in ctx.L.hc_last_error(ctx.h)
        assert ctx.L.hc_encode_coeffs(ctx.h, dv.ptr, 0, 16, 1, SCALE, 0, out.ptr) == 1
        assert ctx.L.hc_encode_coeffs(ctx.h, dv.ptr, 1, 16, 2, SCALE, 0, out.ptr) == 1                 # a level outside the context
        assert ctx.L.hc_encode_coeffs(ctx.h, dv.ptr, 1, 16, 1, SCALE, 0, None) == 1
        seed8 = (C.c_uint32 * 8)(*range(8)); one = (C.c_void_p * 1)(out.ptr)
        assert ctx.L.hc_encrypt_sk(ctx.h, 0, 0, dv.ptr, dv.ptr, seed8, 1, one) == 1
        assert ctx.L.hc_encrypt_sk(ctx.h, 1, 0, dv.ptr, dv.ptr, None, 1, one) == 1
        assert ctx.L.hc_encrypt_sk(ctx.h, 1, 0, dv.ptr, dv.ptr, seed8, 1 << 40, one) == 1
        assert ctx.L.hc_decrypt_decode_coeffs(ctx.h, 0, 0, one, dv.ptr, SCALE, out.ptr) == 1
        assert ctx.L.hc_decrypt_decode_coeffs(ctx.h, 1, 5, one, dv.ptr, SCALE, out.ptr) == 1
        dv.free(); out.free()
        eq(ctx.encode_coeffs(good, 1, SCALE, to_ntt=False)[0], want, "a valid call after the argument errors")
    finally:
        ctx.close()


def _centre(r, q):
    r = r.astype(np.int64)
    return np.where(r > q // 2, r - q, r)


def recover_e(O, sk_rows, ct, m, level):
    """the integer polynomial c0 + c1 s - m per limb (inverse transform by the oracle), centred: one array per limb"""
    out = []
    for l in range(level + 1):
        q = O.modulus(l)
        r = O.intt(l, O.add(l, ct[0, l], O.mul(l, ct[1, l], sk_rows[l])))
        out.append(_centre(O.sub(l, r, m[l] % np.uint64(q)), q))
    return out


# The sampler (hc_gauss_e, shared with hc_swk_generate) rounds a Gaussian of sigma 3.2 to the nearest integer and zeroes what falls beyond 6 sigma (probability 2e-9).
# The variance of the rounded variable is sigma^2 + 1/12 = 10.3233 (Sheppard's correction; exact to 1e-9 at this sigma), and the sample variance of n = 3 N = 196 608
# independent draws has standard deviation 10.3233 * sqrt(2 / n) = 0.0329. Six of those either way. (hc_swk_generate's own test, parity_cases.case_swk_generate, bounds
# the switching noise of a key, not the variance of the error: there is no variance bound to take from it.)
E_VAR, E_VAR_TOL = 3.2 * 3.2 + 1.0 / 12.0, 6 * (3.2 * 3.2 + 1.0 / 12.0) * (2.0 / (3 * N)) ** 0.5


def case_encrypt_relation(make_ctx, make_oracle, levels=(1, 0)):
    """hc_encrypt_sk on count = 3 encoded vectors: c0 + c1 s - m is ONE integer polynomial e per image under every limb, |e| <= 19, different between the images; c1 rows
    lie in [0, q) and differ between limbs and images; (seed8, stream_id) decides the ciphertexts; the variance of e is the sampler's. Then the round trip through
    hc_decrypt_decode_coeffs: decrypt(encrypt(encode(v))) * scale - round(v * scale) == e exactly (scale a power of two, values far below 2^53)."""
    Q, P = [Q0, Q1], [P0]
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        sk = O.gen_sk(77)
        sk_rows = ctx.sk_rows(sk)
        eq(sk_rows[0], np.ascontiguousarray(_or_sk_rows(O, sk, 0)), "NTT(s) by the library == or_sk_rows")
        seed8 = [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89]
        v = np.random.default_rng(9).uniform(-512, 512, (3, N))
        for level in levels:
            nl = level + 1
            m = ctx.encode_coeffs(v, level, SCALE, to_ntt=False)
            cts = ctx.encrypt_sk(m, level, sk_rows, seed8, 7)
            es = []
            for z in range(3):
                e = recover_e(O, sk_rows, cts[z], m[z], level)
                for l in range(1, nl):
                    assert np.array_equal(e[l], e[0]), f"image {z}: the error differs between limbs 0 and {l}: not one integer polynomial"
                assert 0 < np.abs(e[0]).max() <= 19, f"image {z}: |e| = {np.abs(e[0]).max()}"
                for l in range(nl):
                    assert (cts[z, 1, l] < np.uint64(Q[l])).all() and (cts[z, 0, l] < np.uint64(Q[l])).all(), "rows must be canonical"
                es.append(e[0])
            rows = [cts[z, 1, l] for z in range(3) for l in range(nl)]
            for a in range(len(rows)):
                for b in range(a):
                    assert (rows[a] != rows[b]).mean() > 0.99, "c1 rows must differ between limbs and images"
            assert not np.array_equal(es[0], es[1]) and not np.array_equal(es[1], es[2]) and not np.array_equal(es[0], es[2]), "the images share an error polynomial"
            var = float(np.var(np.concatenate(es).astype(np.float64)))
            print(f"level {level}: sample variance of e over 3 N draws = {var:.4f} (expected {E_VAR:.4f} +- {E_VAR_TOL:.4f})")
            assert abs(var - E_VAR) <= E_VAR_TOL
            eq(ctx.encrypt_sk(m, level, sk_rows, seed8, 7), cts, "the same (seed8, stream_id) gives the same ciphertexts")
            other = ctx.encrypt_sk(m, level, sk_rows, seed8, 8)
            assert (other[:, 1] != cts[:, 1]).mean() > 0.99, "another stream_id must give another c1"
            assert not np.array_equal(recover_e(O, sk_rows, other[0], m[0], level)[0], es[0]), "another stream_id must give another e"
            # round trip
            dec = ctx.decrypt_decode_coeffs(cts, level, sk_rows, SCALE)
            want = _centre(m[:, 0], Q[0]).astype(np.float64)          # round(v * scale) with its sign, as the encoder rounded it (|.| < 2^40: exact in fp64)
            diff = dec * SCALE - want
            assert np.array_equal(diff, np.stack(es).astype(np.float64)), f"level {level}: decrypt(encrypt(encode(v))) * scale - round(v * scale) != e"
    finally:
        ctx.close()


def _or_sk_rows(O, sk, l):
    import ctypes as C
    s = np.empty(N, dtype=np.uint64)
    O.L.or_sk_rows(O.ctx, sk.ctypes.data_as(C.POINTER(C.c_int64)), l, s.ctypes.data_as(C.POINTER(C.c_uint64)))
    return s


def case_decrypt_l0(make_ctx, make_oracle):
    """hc_decrypt_decode_coeffs at level 0 == or_decrypt_decode_l0 on an oracle encryption, bit-identical doubles: random residues (both sides of q/2), the centre's
    boundary values planted, a scale that is no power of two (the division rounds)"""
    Q, P = [Q0, Q1], [P0]
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    try:
        sk = O.gen_sk(31)
        sk_rows = ctx.sk_rows(sk)
        scale = SCALE * 1.37
        zero = O.decrypt_decode_l0(sk, O.encrypt(sk, np.zeros((1, N), dtype=np.uint64), 0, 900), 1.0)      # the oracle's e for this seed (m = 0, scale 1)
        e = zero.astype(np.int64)
        target = np.random.default_rng(3).integers(-(Q0 // 2), Q0 // 2 + 1, N)                               # centred values in (-q/2, q/2]
        target[:8] = [0, 1, -1, Q0 // 2, -(Q0 // 2), Q0 // 2 - 1, 2 ** 53, -(2 ** 53) - 1]
        m = ((target - e) % Q0).astype(np.uint64).reshape(1, N)
        ct = O.encrypt(sk, m, 0, 900)
        want = O.decrypt_decode_l0(sk, ct, scale)
        assert want[3] == (Q0 // 2) / scale and want[4] == -(Q0 // 2) / scale, "the planted boundary values did not come out of the oracle"
        got = ctx.decrypt_decode_coeffs(np.stack([ct, ct, ct]), 0, sk_rows, scale)
        for z in range(3):
            assert np.array_equal(got[z].view(np.uint64), want.view(np.uint64)), f"level 0, image {z}: {np.flatnonzero(got[z].view(np.uint64) != want.view(np.uint64))[:8]}"
    finally:
        ctx.close()


def case_decrypt_l1(make_ctx, make_oracle, monkeypatch):
    """level 1 == oracle_bl.decrypt_decode_l1 (CRT in Python integers, float(int): correctly rounded) on an oracle encryption, bit-identical. decrypt_decode_l1 goes on
    to decode slots; its coefficient vector is what is compared, so its decode_slots is the identity here. Planted CRT magnitudes: a tie at the 53-bit boundary
    (2^80 + 2^27, both signs: to even, down), the tie that goes up (2^80 + 3 2^27), the tie broken by a sticky bit far below (2^80 + 2^27 + 1), the 64-bit boundary of
    the two-word magnitude, and both sides of Q/2."""
    Q, P = [Q0, Q1_BL], list(P_BL)
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    monkeypatch.setattr(oracle_bl, "decode_slots", lambda c: np.asarray(c, dtype=np.float64))

    class _BL:
        pass
    bl = _BL(); bl.O = O
    try:
        sk = O.gen_sk(32)
        sk_rows = ctx.sk_rows(sk)
        QQ = Q0 * Q1_BL
        e = oracle_bl.decrypt_decode_l1(bl, sk, O.encrypt(sk, np.zeros((2, N), dtype=np.uint64), 1, 901), 1.0).astype(np.int64)
        assert 0 < np.abs(e).max() <= 19
        rng = np.random.default_rng(4)
        target = [int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 52)) * int(rng.choice([-1, 1])) for _ in range(N)]      # up to 114 bits
        small = rng.integers(-(1 << 62), 1 << 62, N)
        for j in range(0, N, 3):
            target[j] = int(small[j]) >> int(rng.integers(0, 62))
        t0 = 2 ** 80 + 2 ** 27
        planted = [t0, -t0, t0 + 1, -t0 - 1, t0 - 1, 2 ** 80 + 3 * 2 ** 27, -(2 ** 80 + 3 * 2 ** 27), 2 ** 80, QQ // 2, -(QQ // 2), QQ // 2 - 1, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1,
                   -(2 ** 64), 2 ** 53 + 1, 2 ** 64 + 2 ** 11, 2 ** 64 + 2 ** 11 + 1, 2 ** 65 + 3 * 2 ** 11, 2 ** 115 + 2 ** 62, 2 ** 115 + 2 ** 62 + 1, 0, 1, -1]
        target[: len(planted)] = planted
        m = np.array([[(t - int(ej)) % q for t, ej in zip(target, e)] for q in Q], dtype=np.uint64)
        ct = O.encrypt(sk, m, 1, 901)
        want = oracle_bl.decrypt_decode_l1(bl, sk, ct, 1.0)
        assert want[0] == 2.0 ** 80 and want[1] == -(2.0 ** 80) and want[2] == np.nextafter(2.0 ** 80, np.inf) and want[5] == 2.0 ** 80 + 2.0 ** 29, "the planted ties did not come out of the oracle"
        assert want[8] == float(QQ // 2) and want[9] == -float(QQ // 2)
        got = ctx.decrypt_decode_coeffs(ct, 1, sk_rows, 1.0)[0]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"level 1, scale 1: {np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:8]}"
        scale = SCALE * 1.37
        want = oracle_bl.decrypt_decode_l1(bl, sk, ct, scale)
        got = ctx.decrypt_decode_coeffs(np.stack([ct, ct]), 1, sk_rows, scale)
        for z in range(2):
            assert np.array_equal(got[z].view(np.uint64), want.view(np.uint64)), f"level 1, image {z}: {np.flatnonzero(got[z].view(np.uint64) != want.view(np.uint64))[:8]}"
    finally:
        ctx.close()


CONV_CHAIN = ([Q0, Q1], [P0])
BOOT_CHAIN = (list(oracle_ckks.Q_SET6[:4]), list(oracle_ckks.P_SET6[:1]))         # level 3 of ckks.DefaultBootstrapParams[6]: its four lowest limbs, all above 2^31
# the chain's ~30-bit limbs start at level 5: the same four rows with limbs 5 and 6 at levels 2 and 3, so that pack32 = 2 really stores 4-byte rows there
BOOT_SMALL = ([oracle_ckks.Q_SET6[0], oracle_ckks.Q_SET6[1], oracle_ckks.Q_SET6[5], oracle_ckks.Q_SET6[6]], list(oracle_ckks.P_SET6[:1]))
