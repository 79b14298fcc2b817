"""Cases of hc_lv_op2(HC_LV_MONOMIAL): out_k = M_e1 (a_k + M_e0 b_k), M_e = NTT(X^e), shared by the GPU suite (tests/test_gpu_monomial.py) and the CPU emulator
(tests/test_monomial_cpu.py). Each takes factories, as the cases of coeff_codec_cases.py do: make_ctx(Q, P) -> optimal_conv_amd.Context, make_oracle(Q, P) -> Oracle.
Expected words come from the CPU oracle: Oracle.ntt of the one-hot polynomial (the value q - 1 at e - N for e >= N: X^N = -1), then Oracle.mul / Oracle.add; every word
of every limb is compared. N is the library's 2^16; levels <= 3 and <= 3 images."""
import ctypes as C

import numpy as np

from coeff_codec_cases import BOOT_CHAIN, BOOT_SMALL, CONV_CHAIN          # noqa: F401 (the runners name the chains through this module)
from optimal_conv_amd import HC_LV_MONOMIAL
from oracle_lib import splitmix_rows
from parity_cases import N, eq

# (chain, level, pack32, 4-byte rows expected): the convolution's two-limb context at both of its levels; the bootstrapping chain's four lowest limbs with and without
# the 4-byte option (none of them is small: nothing may change); the same rows with two ~30-bit limbs at levels 2 and 3, which pack32 = 2 stores as 4-byte words
SETTINGS = [(CONV_CHAIN, 0, 1, False), (CONV_CHAIN, 1, 1, False), (BOOT_CHAIN, 3, 1, False), (BOOT_CHAIN, 3, 2, False), (BOOT_SMALL, 3, 2, True)]
# e1 alone: +1, the first table entries, both sides of the split between the table's two levels (256), i, the last power before -1, -1 and its neighbours, the last exponent
E1_ALONE = [0, 1, 255, 256, 257, N // 2, N - 1, N, N + 1, 2 * N - 1]
_rng = np.random.default_rng(0x4D4F4E4F)
# re + i im; i (a - b); the first stride layer (in_wid 32, max_batch 64: X^1 then -X^(N - 64 * 33)); a second stride layer without the second factor; ...; two random pairs
PAIRS = [(N // 2, 0), (N, N // 2), (1, 128960), (2, 0), (4, 2 * N - 1), (0, 0)] + [tuple(int(x) for x in _rng.integers(0, 2 * N, 2)) for _ in range(2)]


class Ref:
    """the oracle's side: M_e per limb (cached), and the definition"""

    def __init__(self, O):
        self.O, self.m = O, {}

    def M(self, l, e):
        if (l, e) not in self.m:
            v = np.zeros(N, dtype=np.uint64)
            v[e % N] = 1 if e < N else self.O.modulus(l) - 1
            self.m[(l, e)] = self.O.ntt(l, v)
        return self.m[(l, e)]

    def want(self, level, a, e1, b=None, e0=0):
        """a, b: (2, level+1, N)"""
        out = np.empty_like(a)
        for k in range(2):
            for l in range(level + 1):
                s = a[k, l] if b is None else self.O.add(l, a[k, l], self.O.mul(l, self.M(l, e0), b[k, l]))
                out[k, l] = self.O.mul(l, self.M(l, e1), s)
        return out


def operands(Q, level, seed, worst=False):
    """(2, level+1, N): seeded uniform canonical residues, or q_l - 1 everywhere"""
    if worst:
        return np.stack([np.stack([np.full(N, Q[l] - 1, dtype=np.uint64) for l in range(level + 1)])] * 2)
    return np.stack([np.stack([splitmix_rows(seed + 100 * k + l, Q[l], N) for l in range(level + 1)]) for k in range(2)])


def _open(make_ctx, make_oracle, Q, P, pack32, level, expect32):
    ctx, O = make_ctx(Q, P), make_oracle(Q, P)
    if pack32 != 1:
        ctx.set_option("pack32", pack32)
    assert any(ctx.row32()[: level + 1]) == expect32, "4-byte rows: the case is meant to cross them exactly when expect32"
    return ctx, Ref(O)


def case_values(make_ctx, make_oracle, Q, P, level, pack32=1, expect32=False):
    ctx, R = _open(make_ctx, make_oracle, Q, P, pack32, level, expect32)
    try:
        for worst in (False, True):
            a, b = operands(Q, level, 0xA0, worst), operands(Q, level, 0xB0, worst)
            tag = f"level {level}, pack32 {pack32}, {'a = b = q - 1' if worst else 'random operands'}"
            for e1 in E1_ALONE:
                eq(ctx.lv_monomial(level, a, e1), R.want(level, a, e1), f"X^{e1} a ({tag})")
            for e0, e1 in PAIRS:
                eq(ctx.lv_monomial(level, a, e1, b=b, e0=e0), R.want(level, a, e1, b, e0), f"X^{e1} (a + X^{e0} b) ({tag})")
    finally:
        ctx.close()


def case_batch(make_ctx, make_oracle, Q, P, level, pack32=1, expect32=False):
    """n = 3 under Context.batch() with strides padded by one row: each image equals its single-image call (and the oracle)"""
    ctx, R = _open(make_ctx, make_oracle, Q, P, pack32, level, expect32)
    try:
        a = np.stack([operands(Q, level, 0x1A0 + 7 * z) for z in range(3)])
        b = np.stack([operands(Q, level, 0x1B0 + 7 * z) for z in range(3)])
        stride = (level + 2) * N
        for e0, e1, with_b in ((1, 128960, True), (N, N // 2, True), (N // 2, 0, True), (0, 257, False), (0, N, False)):
            with ctx.batch(3, stride, 2 * (level + 1 + len(P)) * N + N):
                got = ctx.lv_monomial(level, a, e1, b=b if with_b else None, e0=e0)
            for z in range(3):
                single = ctx.lv_monomial(level, a[z], e1, b=b[z] if with_b else None, e0=e0)
                eq(got[z], single, f"image {z} of 3 == its single-image call (e0 {e0}, e1 {e1}, b {with_b})")
                eq(single, R.want(level, a[z], e1, b[z] if with_b else None, e0), f"image {z}: the oracle (e0 {e0}, e1 {e1}, b {with_b})")
    finally:
        ctx.close()


def case_aliasing(make_ctx, make_oracle, Q, P, level, pack32=1, expect32=False):
    """out_k == a_k and out_k == b_k: every coefficient is read before it is written, by the same thread"""
    ctx, R = _open(make_ctx, make_oracle, Q, P, pack32, level, expect32)
    try:
        a, b = operands(Q, level, 0x2A0), operands(Q, level, 0x2B0)
        for e0, e1 in ((1, 128960), (N, N // 2), (N // 2, 0), (300, 70000)):
            want = R.want(level, a, e1, b, e0)
            eq(ctx.lv_monomial(level, a, e1, b=b, e0=e0, out="a"), want, f"out == a (e0 {e0}, e1 {e1})")
            eq(ctx.lv_monomial(level, a, e1, b=b, e0=e0, out="b"), want, f"out == b (e0 {e0}, e1 {e1})")
        for e1 in (N // 2, N, 257):
            eq(ctx.lv_monomial(level, a, e1, out="a"), R.want(level, a, e1), f"out == a, no b (e1 {e1})")
    finally:
        ctx.close()


def _one_hot_rows(Q, level, e):
    v = np.zeros((level + 1, N), dtype=np.uint64)
    for l in range(level + 1):
        v[l, e % N] = 1 if e < N else Q[l] - 1
    return v


def case_former_chain(make_ctx, make_oracle, Q, P, level, pack32=1, expect32=False):
    """the two sequences of the bootstrapping chains, through the same library, bit-equal: HC_LV_MUL_PLAIN by hc_lv_ntt of the one-hot X^(N/2) then HC_LV_ADD (re + i im);
    HC_LV_SUB then HC_LV_MUL_PLAIN (i (cc - ct)); and MultByi alone"""
    ctx, _ = _open(make_ctx, make_oracle, Q, P, pack32, level, expect32)
    try:
        mono_i = ctx.lv_ntt(level, _one_hot_rows(Q, level, N // 2))
        for worst in (False, True):
            a, b = operands(Q, level, 0x3A0, worst), operands(Q, level, 0x3B0, worst)
            eq(ctx.lv_monomial(level, a, 0, b=b, e0=N // 2), ctx.lv_op2(1, level, a, ctx.lv_op2(0, level, b, mono_i, shared_b=True)), "re + i im == MUL_PLAIN, ADD")
            eq(ctx.lv_monomial(level, a, N // 2, b=b, e0=N), ctx.lv_op2(0, level, ctx.lv_op2(2, level, a, b), mono_i, shared_b=True), "i (cc - ct) == SUB, MUL_PLAIN")
            eq(ctx.lv_monomial(level, a, N // 2), ctx.lv_op2(0, level, a, mono_i, shared_b=True), "MultByi == MUL_PLAIN")
    finally:
        ctx.close()


def case_former_stride(make_ctx, make_oracle):
    """the stride layers' front end at level 0 of the convolution context: hc_ntt of the one-hot, hc_mul on r2, hc_add into r1, hc_ntt / hc_mul by -X^(N - 64 * 33)
    (or nothing, for the widths that skip it), with e0 = norm / 4 in 1, 2, 4"""
    Q, P = CONV_CHAIN
    ctx = make_ctx(Q, P)
    try:
        r1, r2 = operands(Q, 0, 0x4A0), operands(Q, 0, 0x4B0)
        for e0 in (1, 2, 4):
            for e1 in (128960, 0):
                pt = ctx.ntt(0, _one_hot_rows(Q, 0, e0))[0]
                t = np.stack([ctx.add(0, r1[k, 0], ctx.mul(0, r2[k, 0], pt)) for k in range(2)])
                if e1:
                    pt1 = ctx.ntt(0, _one_hot_rows(Q, 0, e1))[0]
                    t = np.stack([ctx.mul(0, t[k], pt1) for k in range(2)])
                eq(ctx.lv_monomial(0, r1, e1, b=r2, e0=e0, out="a"), t, f"stride front end, e0 {e0}, e1 {e1}")
    finally:
        ctx.close()


def case_refusals(make_ctx, make_oracle):
    """every refusal is HC_ERR_ARG (1), names hc_lv_op2 in hc_last_error and leaves the context usable; hc_qp_op2 keeps refusing code 10"""
    Q, P = CONV_CHAIN
    ctx, R = _open(make_ctx, make_oracle, Q, P, 1, 1, False)
    try:
        a, b = operands(Q, 1, 0x5A0), operands(Q, 1, 0x5B0)
        A = [ctx.buf(a[k]) for k in range(2)]
        B = [ctx.buf(b[k]) for k in range(2)]
        O = [ctx.buf(nwords=2 * N) for _ in range(2)]
        cs = lambda e0, e1: (C.c_uint64 * 2)(e0, e1)

        def call(level, b0, b1, consts, op=HC_LV_MONOMIAL):
            return ctx.L.hc_lv_op2(ctx.h, op, level, A[0].ptr, A[1].ptr, b0, b1, O[0].ptr, O[1].ptr, consts)

        def valid():
            assert call(1, B[0].ptr, B[1].ptr, cs(1, 128960)) == 0, ctx.L.hc_last_error(ctx.h)
            eq(np.stack([O[k].download((2, N)) for k in range(2)]), R.want(1, a, 128960, b, 1), "a valid call after a refused one")

        refused = [("e0 = 2N", lambda: call(1, B[0].ptr, B[1].ptr, cs(2 * N, 0))),
                   ("e1 = 2N", lambda: call(1, B[0].ptr, B[1].ptr, cs(0, 2 * N))),
                   ("e1 = 2N without b", lambda: call(1, None, None, cs(0, 2 * N))),
                   ("e1 = 2^63", lambda: call(1, B[0].ptr, B[1].ptr, cs(0, 1 << 63))),
                   ("consts NULL", lambda: call(1, B[0].ptr, B[1].ptr, None)),
                   ("b1 NULL alone", lambda: call(1, B[0].ptr, None, cs(1, 1))),
                   ("b0 NULL alone", lambda: call(1, None, B[1].ptr, cs(1, 1))),
                   ("level 2 of a two-limb context", lambda: call(2, B[0].ptr, B[1].ptr, cs(1, 1))),
                   ("level -1", lambda: call(-1, B[0].ptr, B[1].ptr, cs(1, 1)))]
        for what, fn in refused:
            assert fn() == 1, f"{what}: not refused with HC_ERR_ARG"
            assert b"hc_lv_op2" in ctx.L.hc_last_error(ctx.h), f"{what}: {ctx.L.hc_last_error(ctx.h)}"
            valid()
        with ctx.batch(2, N, N):                       # strides of one row: below the two rows of a polynomial at level 1
            assert call(1, B[0].ptr, B[1].ptr, cs(1, 1)) == 1, "batch strides below the operands: not refused"
            assert b"hc_lv_op2" in ctx.L.hc_last_error(ctx.h)
        valid()
        assert call(1, None, None, cs(1 << 40, N // 2)) == 0, "e0 is ignored when there is no b"
        eq(np.stack([O[k].download((2, N)) for k in range(2)]), R.want(1, a, N // 2), "no b: M_e1 a, e0 ignored")
        nt = 2 + len(P)
        X = ctx.buf(nwords=2 * nt * N)
        X.upload(np.zeros(2 * nt * N, dtype=np.uint64))
        assert ctx.L.hc_qp_op2(ctx.h, HC_LV_MONOMIAL, 1, X.at(0), X.at(nt * N), X.at(0), X.at(nt * N), X.at(0), X.at(nt * N)) == 1, "hc_qp_op2 must refuse operation 10"
        valid()
        for x in A + B + O + [X]:
            x.free()
    finally:
        ctx.close()


def case_held_decomposition_survives(E, consumers=("hoisted", "rotate_many"), make_oracle=None):
    """the contract of tests/abi_contract_cases.py for this operation: between hc_keyswitch_decompose and a hoisted consumer it changes nothing the consumer reads (rc 0 and
    the words of `decompose; consumer`), and inside the arena it writes its two outputs only (it claims no scratch). E: abi_contract_cases.part_a_env. The operation is
    entered as an intruder of that table for the duration of the call only, so that the table's own completeness tests see it unchanged."""
    import abi_contract_cases as ab
    key = "lv_op2:monomial"

    def intruder(E):
        E.ok("hc_lv_op2", HC_LV_MONOMIAL, E.level, E.a.ptr, E.a1.ptr, E.b.ptr, E.b1.ptr, E.xp[0].ptr, E.xp[1].ptr, (C.c_uint64 * 2)(1, 128960))
        E.xp[0].w(); E.xp[1].w()

    ab.INTRUDERS[key] = ("hc_lv_op2", intruder)
    ab.MUST_SURVIVE.add(key)
    try:
        for cname in consumers:
            assert ab.sequence(E, key, cname, make_oracle) == 0
    finally:
        del ab.INTRUDERS[key]
        ab.MUST_SURVIVE.discard(key)
