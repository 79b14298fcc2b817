"""Cases of hc_encode_slots_ex (ckks.(*encoderComplex128).Embed + scaleUpVecExact + ToNTT with sparse slots and rows modulo the special primes), shared by the GPU suite
(tests/test_gpu_slot_encoder_ex.py) and the CPU emulator (tests/test_slot_encoder_ex_cpu.py). Each takes factories, as the cases of coeff_codec_cases.py do:
make_ctx(Q, P) -> optimal_conv_amd.Context, make_oracle(Q, P) -> Oracle. N is fixed at 2^16, so a case is small in ROWS and in vectors; the expected words of a
(chain, log_slots, level, with_p, scale) are computed once and shared by whoever asks again."""
import numpy as np

import coeff_codec_cases as cc
import oracle_ckks
from parity_cases import N, eq

BOOT_CHAIN = cc.BOOT_CHAIN                                                                      # level 3 of ckks.DefaultBootstrapParams[6]: four limbs above 2^31
BOOT_CHAIN13 = (list(oracle_ckks.Q_SET6[:13]), list(oracle_ckks.P_SET6[:1]))                    # the same chain up to level 12: limbs 5 .. 12 are ~30-bit primes
BOOT_SMALL = cc.BOOT_SMALL                                                                      # ~30-bit limbs at levels 2 and 3
BOOT_2P = (list(oracle_ckks.Q_SET6[:4]), list(oracle_ckks.P_SET6[:2]))                          # two special primes
CHAINS = {"boot": BOOT_CHAIN, "boot13": BOOT_CHAIN13, "small": BOOT_SMALL, "two_p": BOOT_2P}
KINDS = ("random", "zero", "delta", "alt_real", "alt_imag")
_ENC = []
_WANT = {}


def encoder():
    if not _ENC:
        _ENC.append(oracle_ckks.Encoder(16))
    return _ENC[0]


def scale_of(kind, Q, level):
    """2^30; about 2^60 (the limb itself, as the CoeffsToSlots diagonals are scaled); 2^70: beyond 2^64 for most coefficients (scaleUpVecExact's mantissa branch)"""
    return {"2^30": 2.0 ** 30, "q": float(Q[level]), "2^70": 2.0 ** 70}[kind]


def vector(kind, n, seed):
    if kind == "random":                                                                        # |v| <= 1
        rng = np.random.default_rng(seed)
        return np.sqrt(rng.uniform(0, 1, n)) * np.exp(2j * np.pi * rng.uniform(0, 1, n))
    v = np.zeros(n, dtype=np.complex128)
    if kind == "delta":
        v[0] = 1.0
    elif kind == "alt_real":
        v[:] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    elif kind == "alt_imag":
        v[:] = np.where(np.arange(n) % 2 == 0, 1.0j, -1.0j)
    return v


def inputs(log_slots, count):
    """the five kinds of input, in calls of `count` vectors (the last call is filled up with further seeded vectors): [(vectors, their names)]"""
    n = 1 << log_slots
    todo = [(k, 1000 + log_slots) for k in KINDS]
    while len(todo) % count:
        todo.append(("random", 2000 + log_slots + len(todo)))
    return [todo[i:i + count] for i in range(0, len(todo), count)], {t: vector(t[0], n, t[1]) for t in todo}


def expected(make_oracle, chain, log_slots, level, with_p, scale, key):
    """(coefficient-domain rows, NTT rows) of one input vector: Encoder.slots_to_coeffs, Oracle.encode_coeffs (scaleUpVecExact with its beyond-2^64 branch, what
    parity_cases.case_encode_slots compares hc_encode_slots against), Oracle.ntt"""
    Q, P = CHAINS[chain]
    k = (chain, log_slots, level, bool(with_p), scale, key)
    if k not in _WANT:
        O = make_oracle(Q, P)
        mods = list(range(level + 1)) + ([len(Q) + j for j in range(len(P))] if with_p else [])
        cf = encoder().slots_to_coeffs(vector(key[0], 1 << log_slots, key[1]))
        rows = np.stack([np.asarray(r).reshape(-1) for r in O.encode_coeffs(cf, scale, mods)])
        ntt = np.stack([np.asarray(O.ntt(m, rows[i])).reshape(-1) for i, m in enumerate(mods)])
        rows.setflags(write=False); ntt.setflags(write=False)
        _WANT[k] = (rows, ntt)
    return _WANT[k]


def case(make_ctx, make_oracle, chain, log_slots, level, with_p, scale_kind, count, pack32, kinds=KINDS):
    """hc_encode_slots_ex == the oracle word for word, to_ntt 0 and 1, for every kind of input; off the gap grid the coefficient-domain word is 0; log_slots = 15 gives
    hc_encode_slots' Q rows bit for bit"""
    Q, P = CHAINS[chain]
    scale = scale_of(scale_kind, Q, level)
    ctx = make_ctx(Q, P)
    try:
        if pack32 != 1:
            ctx.set_option("pack32", pack32)
        nl, n, gap = level + 1, 1 << log_slots, (N // 2) >> log_slots
        calls, vecs = inputs(log_slots, count)
        calls = [c for c in calls if any(t[0] in kinds for t in c)]
        for call in calls:
            vals = np.stack([vecs[t] for t in call])
            what = f"{chain} log_slots {log_slots} level {level} with_p {with_p} scale {scale_kind} pack32 {pack32} inputs {[t[0] for t in call]}"
            got_c = ctx.encode_slots_ex(vals.copy(), log_slots, level, with_p, scale, to_ntt=False)
            got_n = ctx.encode_slots_ex(vals.copy(), log_slots, level, with_p, scale, to_ntt=True)
            assert got_c.shape == got_n.shape == (count, nl + (len(P) if with_p else 0), N)
            for z, t in enumerate(call):
                want_c, want_n = expected(make_oracle, chain, log_slots, level, with_p, scale, t)
                eq(got_c[z], want_c, f"coefficient domain, vector {z}: {what}")
                eq(got_n[z], want_n, f"NTT domain, vector {z}: {what}")
            if gap > 1:
                off = np.ones(N, dtype=bool); off[::gap] = False
                assert not got_c[:, :, off].any(), f"a coefficient off the gap grid is not the word 0: {what}"
            if log_slots == 15:
                for to_ntt, got in ((False, got_c), (True, got_n)):
                    old = ctx.unpack_rows(ctx.encode_slots(vals.copy(), level, scale, to_ntt=to_ntt), nl)
                    eq(got[:, :nl], old, f"hc_encode_slots_ex(15, with_p) Q rows == hc_encode_slots, to_ntt {to_ntt}: {what}")
    finally:
        ctx.close()


def case_refusals(make_ctx, make_oracle):
    """log_slots 16 and -1, level = nq, a null pointer: HC_ERR_ARG (1) each, and a valid call afterwards succeeds with the right words"""
    Q, P = BOOT_CHAIN
    ctx = make_ctx(Q, P)
    try:
        v = vector("random", 1 << 9, 5).reshape(1, -1)
        want_c, _ = expected(make_oracle, "boot", 9, 1, True, 2.0 ** 30, ("random", 5))
        dv, out = ctx.buf(nwords=N), ctx.buf(nwords=(len(Q) + len(P)) * N)
        L, h = ctx.L, ctx.h
        for args in ((dv.ptr, 1, 16, 1, 1, 2.0 ** 30, 0, out.ptr), (dv.ptr, 1, -1, 1, 1, 2.0 ** 30, 0, out.ptr), (dv.ptr, 1, 9, len(Q), 1, 2.0 ** 30, 0, out.ptr),
                     (None, 1, 9, 1, 1, 2.0 ** 30, 0, out.ptr), (dv.ptr, 1, 9, 1, 1, 2.0 ** 30, 0, None), (dv.ptr, 0, 9, 1, 1, 2.0 ** 30, 0, out.ptr)):
            assert L.hc_encode_slots_ex(h, *args) == 1 and b"hc_encode_slots_ex" in L.hc_last_error(h), args
            eq(ctx.encode_slots_ex(v, 9, 1, True, 2.0 ** 30, to_ntt=False)[0], want_c, "a valid call after a refused one")
        dv.free(); out.free()
    finally:
        ctx.close()


# (chain, log_slots, level, with_p, scale, count, pack32): every log_slots at which the code takes another path - 0 no stage, 1, 8 in-row stages only, 9 the first
# row-pairing stage, 11 the last single-tile size, 12 the first two-pass size (R = 16), 14, 15 (also == hc_encode_slots) - with Q and P rows and three vectors a call; then
# the other parameters at the sizes the product uses: without P rows, one vector a call, the three scales, the 13-limb chain (~30-bit limbs) under pack32 1 and 2, 4-byte
# rows at levels 2 and 3, two special primes
CASES = [("boot", ls, 3, 1, "2^30", 3, 1) for ls in (0, 1, 8, 9, 11, 12, 14, 15)] + [
    ("boot", 12, 3, 0, "q", 1, 1), ("boot", 15, 3, 0, "2^70", 1, 1), ("boot", 1, 3, 0, "2^70", 3, 1), ("boot", 12, 3, 1, "2^70", 1, 1), ("boot", 14, 3, 1, "q", 3, 2),
    ("boot", 11, 3, 1, "q", 1, 2), ("boot13", 12, 12, 1, "q", 3, 1), ("boot13", 12, 12, 1, "2^30", 1, 2), ("boot13", 15, 12, 0, "q", 1, 2),
    ("small", 9, 3, 1, "2^30", 3, 2), ("small", 15, 3, 1, "q", 1, 2), ("small", 12, 2, 0, "2^70", 1, 2), ("two_p", 12, 3, 1, "q", 3, 1), ("two_p", 8, 3, 1, "2^70", 1, 2)]


def case_id(c):
    return "-".join(str(x) for x in c)


# ---- against the reference binary's own digests (tests/golden/ref_trace_diag_*.json; the recipe of tests/test_oracle_pin_dft.py::test_encoded_diagonals and
# ::test_sparse_encoded_diagonals with the device in the encoder's place)
def mul_2_64(rows, q):
    """rows * 2^64 mod q (the Montgomery form the binary hashes), in numpy: the quotient estimated in 80-bit floats (64-bit mantissa: off by at most 2 for q < 2^62),
    the remainder exactly in wrapping 64-bit words, corrected into [0, q)"""
    assert np.finfo(np.longdouble).nmant >= 63 and q < (1 << 62)
    r = (1 << 64) % q
    a = np.ascontiguousarray(rows, dtype=np.uint64)
    quot = np.floor(a.astype(np.longdouble) * np.longdouble(r) / np.longdouble(q)).astype(np.uint64)
    with np.errstate(over="ignore"):
        d = (a * np.uint64(r) - quot * np.uint64(q)).view(np.int64)
    for _ in range(3):
        d = np.where(d < 0, d + np.int64(q), d)
        d = np.where(d >= np.int64(q), d - np.int64(q), d)
    out = d.view(np.uint64)
    flat_a, flat_o = a.reshape(-1), out.reshape(-1)
    for j in range(0, flat_a.size, max(1, flat_a.size // 61)):
        assert int(flat_o[j]) == int(flat_a[j]) * r % q
    return out


def case_reference_digests(ctx, ls):
    """one of the four sparse bootstrappers' sets (ls = 11 .. 14: diagonals of 2^(ls+1) values) or the full-slot set (ls = 15), on a context over the whole of parameter
    set [6]: the first and the last diagonal of matrix 0 (CoeffsToSlots' first), value vectors from tests/lattigo_dft.py, encoded by hc_encode_slots_ex(with_p = 1,
    to_ntt = 1) at the fixture's level and scale; times 2^64 mod q; SHA-256 of the Q rows plus the spare zero limb and of the P rows == the binary's mQ and mP"""
    import hashlib
    import lattigo_dft as ld
    import test_oracle_pin_dft as pin
    Q, P = list(oracle_ckks.Q_SET6), list(oracle_ckks.P_SET6)
    assert sorted(pin.SPARSE) == [11, 12, 13, 14], "a sparse fixture is missing"
    zero = np.zeros(N, dtype=np.uint64)
    if ls == 15:
        M, diags, slots = ld.compute_dft_matrices(15, 15, 4, ld.cts_diffscale(pin.Q0), True)[0], pin.DIAGS[0], 1 << 15
    else:
        M, diags, slots = ld.compute_dft_matrices(ls, ls + 1, 4, ld.cts_diffscale(pin.Q0), True)[0], pin._sparse_tables(ls)[1][0], 2 << ls
    _, vecs = ld.encoder_inputs(M, slots)
    items = sorted(vecs.items())
    pick = [items[0][1], items[-1][1]]
    ev = [diags[hashlib.sha256(v.bytes()).hexdigest()] for v in pick]                      # a KeyError here: the value vector is not the binary's
    lvl, scale = ev[0]["level"], ev[0]["scale"]
    assert (ev[1]["level"], ev[1]["scale"]) == (lvl, scale) and ev[0]["mQ_limbs"] == lvl + 2 and ev[0]["mP_limbs"] == len(P)
    log_slots = slots.bit_length() - 1
    got = ctx.encode_slots_ex(np.stack([v.complex() for v in pick]), log_slots, lvl, 1, scale, to_ntt=True)
    for z, e in enumerate(ev):
        mq = [mul_2_64(got[z, l], Q[l]) for l in range(lvl + 1)]
        mp = [mul_2_64(got[z, lvl + 1 + j], P[j]) for j in range(len(P))]
        hq = hashlib.sha256(np.concatenate(mq + [zero]).tobytes()).hexdigest()
        hp = hashlib.sha256(np.concatenate(mp).tobytes()).hexdigest()
        assert hq == e["mQ"], f"log_slots {log_slots}, diagonal {z}: mQ differs from the reference binary's"
        assert hp == e["mP"], f"log_slots {log_slots}, diagonal {z}: mP differs from the reference binary's"
