"""The leveled entry points in the FORM a host hands operands over, and in the ORDER its calls arrive (tests/test_gpu_a_abi_contract.py on the device,
tests/test_emu_abi_contract.py on the fibre emulator). The value every entry point computes is pinned to the oracle by tests/parity_cases.py; nothing here is a
tolerance: a result must equal, word for word, the same entry point called in the plain form - fresh operands, ascending and contiguous, no output on an input, nothing
between the calls - or an untouched fill.

Every operand and output is carved out of an ARENA: one device allocation whose word i starts as FILL | i, mirrored by a host shadow. A call says which rows it is
documented to write; Arena.verify downloads the arena once, accepts exactly those rows, and requires every other word - the words before and after an output, the rows
above its level, the padding between the images of a batch, every input - to be what the shadow says. That one helper is Part C of all three parts:

  A  a decomposition held by hc_keyswitch_decompose, then one call of the table INTRUDERS, then a hoisted consumer: the consumer returns HC_ERR_STATE with its outputs
     untouched, or HC_OK with the words of `decompose; consumer`. MUST_SURVIVE and MUST_REFUSE say which of the two for the calls where it is settled.
  B  the two polynomials of a ciphertext (or two outputs) as separate pointers in descending, mixed and far-apart placements (PLACED), and the aliased forms the header
     permits or the host uses (ALIASED).

Shapes: Q = pc.Q_MIX[:level + 2] (one modulus above the level), level 4, alpha special primes of pc.P_CHAIN (3: two digits; 2: three digits, hc_k_ks_mac_multi's lazy
form), one image per call or three with case_batched_leveled's padded strides. Under pack32 = 2 rows are converted at the boundary (Context.pack_rows / unpack_rows); the
unused half of a 4-byte row's slot is filled but never asserted on."""
import ctypes as C
import os
import re

import numpy as np

import parity_cases as pc

N = pc.N
FILL = 0xF1A7 << 48                        # above every modulus (all below 2^61), and different in every word of the arena
HC_OK, HC_ERR_ARG, HC_ERR_STATE, HC_ERR_UNSUPPORTED = 0, 1, 3, 4
U = C.c_uint64
HEADERS = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", h) for h in ("hconv.h", "hconv_test_hooks.h")]
GAL, GAL2, GAL3 = pow(5, 7, 2 * N), pow(5, 9, 2 * N), pow(5, 40, 2 * N)
LOW = 2                                   # "another level" of the intruders that have one
K0, K1, K_LOW, K_L1 = 30, 31, 40, 41      # switching keys: two at the held level, one at LOW, one at level 1


def chain(level, alpha):
    return list(pc.Q_MIX[: level + 2]), list(pc.P_CHAIN[:alpha])


class Arena:
    """One device allocation of which `windows` [(first row, rows)] are filled, mirrored and checked (one window: the whole allocation; two: the ends of an allocation
    whose middle only provides address distance and is never touched)."""

    def __init__(self, ctx, windows, total_rows=None):
        self.ctx = ctx
        self.windows = [(r0 * N, nr * N) for r0, nr in windows]
        self.buf = ctx.buf(nwords=(total_rows * N) if total_rows else self.windows[-1][0] + self.windows[-1][1])
        self.shadow = [self._fill(w0, nw) for w0, nw in self.windows]
        for (w0, nw), s in zip(self.windows, self.shadow):
            self.buf.upload(s, w0)
        self.got = [np.empty(nw, dtype=np.uint64) for w0, nw in self.windows]
        self.top = [w0 for w0, nw in self.windows]
        self.writes = []

    @staticmethod
    def _fill(w0, nw):
        return np.arange(w0, w0 + nw, dtype=np.uint64) | np.uint64(FILL)

    def _win(self, off, nw):
        for i, (w0, n) in enumerate(self.windows):
            if w0 <= off and off + nw <= w0 + n:
                return i, off - w0
        raise AssertionError(f"words {off}..{off + nw} lie in no window of the arena")

    def take(self, nwords, window=0):
        assert nwords % N == 0
        off = self.top[window]
        self.top[window] += nwords
        self._win(off, nwords)
        return off

    def put(self, off, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1)
        i, o = self._win(off, arr.size)
        self.shadow[i][o: o + arr.size] = arr
        self.buf.upload(arr, off)

    def refill(self, off, nw):
        self.put(off, self._fill(off, nw))

    def reset(self):
        """back to the fill wherever something was carved; nothing is carved afterwards"""
        for i, (w0, nw) in enumerate(self.windows):
            if self.top[i] > w0:
                self.refill(w0, self.top[i] - w0)
            self.top[i] = w0
        self.writes = []

    def at(self, off):
        return self.buf.at(off)

    def declare(self, off, nw):
        self.writes.append((off, nw))

    def verify(self, what):
        """PART C, the one footprint check: every word of the arena outside the declared writes of the calls since the last verify is what it was. Returns the downloaded
        windows (Slot.read copies payloads out of them; the next verify overwrites them)."""
        got = self.got
        for (w0, nw), g in zip(self.windows, got):                         # into the same host pages every time: the arena is hundreds of MiB
            self.ctx._ck(self.ctx.L.hc_download(self.ctx.h, g.ctypes.data_as(C.c_void_p), self.buf.at(w0), nw * 8))
        for off, nw in self.writes:
            i, o = self._win(off, nw)
            self.shadow[i][o: o + nw] = got[i][o: o + nw]
        self.writes = []
        for i, (w0, nw) in enumerate(self.windows):
            if not np.array_equal(got[i], self.shadow[i]):
                bad = np.flatnonzero(got[i] != self.shadow[i])
                rows_ = sorted({int(b + w0) // N for b in bad[:: max(1, bad.size // 64)]})[:12]
                first = int(bad[0])
                self.shadow[i][:] = got[i]                   # one report per fault: later checks start from what is there
                raise AssertionError(f"{what}: {bad.size} words outside the documented footprint changed; arena rows {rows_}; first at word {first + w0} "
                                     f"(row {(first + w0) // N}, column {(first + w0) % N}): {int(got[i][first]):#x}")
        return got

    def free(self):
        self.buf.free()


class Slot:
    """An operand carved at word `off`: `images` copies `stride` words apart, each `rows` payload rows (row r of modulus mods[r]: nlq limbs, then special primes)."""

    def __init__(self, E, off, stride, images, rows, nlq, per):
        self.E, self.off, self.stride, self.images, self.rows, self.nlq, self.per = E, off, stride, images, rows, nlq, per
        self.data = None

    @property
    def ptr(self):
        return self.E.A.at(self.off)

    def at(self, words):
        return self.E.A.at(self.off + words)

    def put(self, data):
        """data: (images, rows, N) residues, 8-byte words"""
        ctx = self.E.ctx
        self.data = np.ascontiguousarray(data, dtype=np.uint64).reshape(self.images, self.rows, N)
        for z in range(self.images):
            x = self.data[z] if self.nlq is None else ctx.pack_rows(self.data[z], self.nlq, self.per)
            self.E.A.put(self.off + z * self.stride, x)
        return self

    def fill(self):
        for z in range(self.images):
            self.E.A.refill(self.off + z * self.stride, self.rows * N)
        return self

    def w(self, segs=None):
        """declare that the call under test writes rows segs = [(first, count)] of every image (default: all payload rows)"""
        for z in range(self.images):
            for r0, nr in (segs or [(0, self.rows)]):
                self.E.A.declare(self.off + z * self.stride + r0 * N, nr * N)
        return self

    def read(self, got):
        ctx, out = self.E.ctx, []
        for z in range(self.images):
            i, o = self.E.A._win(self.off + z * self.stride, self.rows * N)
            x = got[i][o: o + self.rows * N].reshape(self.rows, N)
            out.append(x.copy() if self.nlq is None else ctx.unpack_rows(x, self.nlq, self.per))
        return np.stack(out)


class Env:
    """One context at (level, n images) with its arena and the operands every call of Part A draws from."""

    def __init__(self, ctx, level, n, arena_rows=None, windows=None, total_rows=None, seed=0xAB1C0):
        self.ctx, self.L, self.h, self.level, self.n = ctx, ctx.L, ctx.h, level, n
        self.Q, self.P = ctx.q, ctx.p
        self.nq, self.alpha, self.nl = len(self.Q), len(self.P), level + 1
        self.nt, self.beta = self.nl + self.alpha, (self.nl + self.alpha - 1) // self.alpha
        self.PS, self.QS = (self.nl + 2) * N, (2 * self.nt + 3) * N           # case_batched_leveled's padded strides
        self.rng = np.random.default_rng(seed + 7 * n + self.alpha)
        self.A = Arena(ctx, windows or [(0, arena_rows)], total_rows)
        self.window = 0
        ctx.set_batch(n, self.PS, self.QS)
        self.wgs0 = getattr(ctx, "wgs0", 0)                                # the context's small_mm_wgs (the test files set it when they make the context)
        self.restore = []                                                  # undo what an intruder did to the context's options or batch
        self.k0, self.k1 = K0, K1                                          # the keys the consumers switch with

    def close(self):
        self.ctx.set_batch(1)
        self.A.free()

    # ---- random residues
    def qmod(self, t, level=None):
        nl = (self.level if level is None else level) + 1
        return self.Q[t] if t < nl else self.P[t - nl]

    def res(self, mods, images=None):
        return np.stack([np.stack([self.rng.integers(0, q, N, dtype=np.uint64) for q in mods]) for _ in range(images or self.n)])

    # ---- carving. Every slot takes images * stride words, so that the last image has its padding too
    def poly(self, level=None, data=True, rows=None, images=None):
        level = self.level if level is None else level
        rows, images = (level + 1) if rows is None else rows, images or self.n
        s = Slot(self, self.A.take(images * self.PS, self.window), self.PS, images, rows, rows, rows)
        return s.put(self.res(self.Q[:rows], images)) if data else s

    def qp(self, level=None, data=True, comps=2, images=None):
        """an extended-basis pair [2][level+1+np][N] (comps = 1: one component of it, for the entry points that take the two separately)"""
        level, images = self.level if level is None else level, images or self.n
        ntl = level + 1 + self.alpha
        s = Slot(self, self.A.take(images * self.QS, self.window), self.QS, images, comps * ntl, level + 1, ntl)
        return s.put(self.res([self.qmod(t, level) for t in range(ntl)] * comps, images)) if data else s

    def raw(self, rows, data=None):
        """rows of 8-byte words outside the leveled layout (one-row primitives, the secret key, doubles)"""
        s = Slot(self, self.A.take(rows * N, self.window), rows * N, 1, rows, None, None)
        return s.put(data) if data is not None else s

    # ---- calls
    def call(self, name, *args):
        return getattr(self.L, name)(self.h, *args)

    def ok(self, name, *args):
        rc = self.call(name, *args)
        assert rc == HC_OK, f"{name} failed ({rc}): {self.L.hc_last_error(self.h).decode()}"

    def consts(self, level=None):
        level = self.level if level is None else level
        return (U * (level + 1))(*[int(self.rng.integers(1, self.Q[l])) for l in range(level + 1)])

    def key_rows(self, level):
        ntl, beta = level + 1 + self.alpha, (level + 1 + self.alpha - 1) // self.alpha
        return np.stack([self.rng.integers(0, self.qmod(t, level), N, dtype=np.uint64) for _ in range(beta * 2) for t in range(ntl)]).reshape(beta, 2, ntl, N)


def ptrs(*slots):
    return (C.c_void_p * len(slots))(*[s.ptr if s is not None else None for s in slots])


# ------------------------------------------------------------------------------------------------ Part A
def part_a_env(ctx, level, n):
    """the operands of Part A: cx and its decomposition's consumers' outputs (co*), the intruders' inputs and outputs (x*)"""
    nl, alpha = level + 1, len(ctx.p)
    nt = nl + alpha
    polys, qps = 16, 11
    E = Env(ctx, level, n, arena_rows=n * (polys * (nl + 2) + qps * (2 * nt + 3)) + 64)
    E.keys = {}
    for kid, lv in ((K0, level), (K1, level), (K_LOW, LOW), (K_L1, 1)):
        E.keys[kid] = E.key_rows(lv)
        ctx.swk_load(kid, lv, E.keys[kid])
    E.cx, E.cx_twin = E.poly(), E.poly()
    E.cx_twin.put(E.cx.data)                                             # another pointer, identical contents
    E.a, E.b, E.a1, E.b1 = E.poly(), E.poly(), E.poly(), E.poly()
    E.la, E.lb = E.poly(LOW), E.poly(LOW)
    E.l1 = E.poly(1)
    E.pt, E.ptq = E.poly(images=1), E.qp(comps=1, images=1)            # ONE plaintext for every image
    E.X, E.Y, E.lX = E.qp(), E.qp(), E.qp(LOW)
    E.accp0, E.accp1, E.accq = E.poly(), E.poly(), E.qp()               # accumulators of the intruders: they hold residues, whatever was added
    E.xp = [E.poly(data=False) for _ in range(3)]
    E.xq = [E.qp(data=False) for _ in range(3)]
    E.cp = [E.poly(data=False) for _ in range(2)]
    E.cq = [E.qp(data=False) for _ in range(3)]
    E.sk = E.raw(E.nq + alpha, E.res(list(E.Q) + list(E.P), 1))
    E.r8 = E.raw(4, E.res([E.Q[0]] * 4, 1))                             # 8-byte rows modulo q_0 for the one-row primitives
    E.ct1 = E.raw(4, E.res([E.Q[0], E.Q[1]] * 2, 1))                    # a level-1 ciphertext in 8-byte rows
    E.ct8 = E.raw(2 * nl, E.res(list(E.Q[:nl]) * 2, 1))                 # a ciphertext at the level in 8-byte rows (the baseline's tap sum)
    E.dbl = E.raw(2, np.stack([E.rng.standard_normal(N), E.rng.standard_normal(N)]).view(np.uint64))      # doubles: slot values (re, im) / coefficients
    E.xr = E.raw(2 * (nt + 2))                                         # raw outputs of the intruders
    E.A.verify("uploading the operands")
    return E


# the consumers of a held decomposition: name -> (hc name, slots of `outs` it writes, call(E, outs) -> rc). outs = {"p": [2 polynomials], "q": [3 pairs]}
def _c_hoisted(E, o):
    return E.call("hc_keyswitch_hoisted", U(E.k0), E.level, E.cx.ptr, o["p"][0].ptr, o["p"][1].ptr)


def _c_rotate(E, o):
    return E.call("hc_keyswitch_rotate", U(E.k1), U(GAL), E.level, E.a.ptr, E.cx.ptr, o["p"][0].ptr, o["p"][1].ptr, 1)


def _c_qp(E, o):
    return E.call("hc_keyswitch_qp", U(E.k0), E.level, E.cx.ptr, o["q"][0].ptr, 1)


def _c_qp_rotate(E, o):
    return E.call("hc_keyswitch_qp_rotate", U(E.k0), U(GAL), E.level, E.b.ptr, E.cx.ptr, o["q"][0].ptr, 1, 0)


def _c_qp_rotate_acc(E, o):
    return E.call("hc_keyswitch_qp_rotate", U(E.k1), U(GAL2), E.level, None, E.cx.ptr, o["q"][0].ptr, 1, 1)


def _c_rotate_many(E, o):
    return E.call("hc_keyswitch_qp_rotate_many", 3, (U * 3)(E.k0, E.k1, E.k0), (U * 3)(GAL, GAL2, GAL3), E.level, E.b.ptr, E.cx.ptr, ptrs(*o["q"]))


CONSUMERS = {
    "hoisted": ("hc_keyswitch_hoisted", ("p0", "p1"), _c_hoisted),
    "rotate": ("hc_keyswitch_rotate", ("p0", "p1"), _c_rotate),
    "qp": ("hc_keyswitch_qp", ("q0",), _c_qp),
    "qp_rotate": ("hc_keyswitch_qp_rotate", ("q0",), _c_qp_rotate),
    "qp_rotate_acc": ("hc_keyswitch_qp_rotate", ("q0",), _c_qp_rotate_acc),
    "rotate_many": ("hc_keyswitch_qp_rotate_many", ("q0", "q1", "q2"), _c_rotate_many),
}


def _outs(o, uses):
    return [o[u[0]][int(u[1])] for u in uses]


def consumer_outs(E):
    return {"p": E.cp, "q": E.cq}


def prepare_consumer(E, cname):
    """the consumer's outputs back to the fill (the accumulating form: to the residues it adds to)"""
    for s in _outs(consumer_outs(E), CONSUMERS[cname][1]):
        if cname == "qp_rotate_acc":
            s.put(E.Y.data)
        else:
            s.fill()


def run_consumer(E, cname, what):
    """rc of the consumer, and its outputs' payloads (None when it refused: verify has then shown its outputs untouched)"""
    outs = _outs(consumer_outs(E), CONSUMERS[cname][1])
    rc = CONSUMERS[cname][2](E, consumer_outs(E))
    assert rc in (HC_OK, HC_ERR_STATE), f"{what}: the consumer returned {rc}: {E.L.hc_last_error(E.h).decode()}"
    if rc == HC_OK:
        for s in outs:
            s.w()
    got = E.A.verify(what)
    return rc, ([s.read(got) for s in outs] if rc == HC_OK else None)


def consumer_reference(E, cname, make_oracle=None):
    """`decompose; consumer` with nothing between: what every sequence that succeeds must give. The plain hoisted key switch is also held to the oracle here."""
    if not hasattr(E, "refs"):
        E.refs = {}
    if cname not in E.refs:
        prepare_consumer(E, cname)
        E.ok("hc_keyswitch_decompose", E.level, E.cx.ptr)
        rc, res = run_consumer(E, cname, f"decompose; {cname}")
        assert rc == HC_OK, f"decompose; {cname} was refused: {E.L.hc_last_error(E.h).decode()}"
        E.refs[cname] = res
        if cname == "hoisted" and make_oracle is not None:
            O = make_oracle(E.Q, E.P)
            w0, w1 = O.keyswitch(E.level, E.cx.data[0], E.keys[K0])
            pc.eq(res[0][0], w0, "decompose; hc_keyswitch_hoisted == oracle (d0, image 0)"); pc.eq(res[1][0], w1, "decompose; hc_keyswitch_hoisted == oracle (d1, image 0)")
    return E.refs[cname]


# ---- the intruders: one valid, representative call of every entry point that takes a context and queues work or changes its state. key -> (hc name, call(E)); a call
# declares what it writes and asserts its own success. Operands are polynomials other than cx (the consumers themselves excepted: they are what a host runs in a row).
def _as_intruder(cname):
    def fn(E):
        o = {"p": E.xp, "q": [E.accq] + E.xq[1:]} if cname == "qp_rotate_acc" else {"p": E.xp, "q": E.xq}
        rc = CONSUMERS[cname][2](E, o)
        assert rc == HC_OK, f"{cname} as an intruder right after the decomposition failed ({rc}): {E.L.hc_last_error(E.h).decode()}"
        for s in _outs(o, CONSUMERS[cname][1]):
            s.w()
    return fn


def _lv(name, level_of=None, shared=False, acc=False, const=False):
    def fn(E):
        lv = E.level if level_of is None else level_of
        a, b = (E.a, E.b) if level_of is None else (E.la, E.lb)
        out = E.accp0 if acc else E.xp[0]
        if const:
            E.ok(name, lv, a.ptr, E.consts(lv), out.ptr)
        elif name in ("hc_lv_ntt", "hc_lv_intt"):
            E.ok(name, lv, a.ptr, out.ptr)
        else:
            E.ok(name, lv, a.ptr, (E.pt if shared else b).ptr, out.ptr)
        out.w([(0, lv + 1)])
    return fn


def _op2(op, shared=False, acc=False, const=False):
    def fn(E):
        o0, o1 = (E.accp0, E.accp1) if acc else (E.xp[0], E.xp[1])
        b0, b1 = (None, None) if const else (E.pt.ptr, None) if shared else (E.b.ptr, E.b1.ptr)
        E.ok("hc_lv_op2", op, E.level, E.a.ptr, E.a1.ptr, b0, b1, o0.ptr, o1.ptr, E.consts() if const else None)
        o0.w(); o1.w()
    return fn


def _rotate_finish(E):
    E.ok("hc_rotate_finish", U(GAL), E.level, E.a.ptr, E.a1.ptr, E.b.ptr, E.xp[0].ptr, E.xp[1].ptr); E.xp[0].w(); E.xp[1].w()


def _lv_permute(E):
    E.ok("hc_lv_permute", U(GAL), E.level, E.a.ptr, E.xp[0].ptr); E.xp[0].w()


def _qp_permute2(E):
    E.ok("hc_qp_permute2", U(GAL), E.level, E.X.ptr, E.xq[0].ptr); E.xq[0].w()


def _lincomb2(E):
    cs = (U * (2 * E.nl))(*[int(E.rng.integers(1, E.Q[l])) for _ in range(2) for l in range(E.nl)])
    E.ok("hc_lv_lincomb2", E.level, 2, ptrs(E.a, E.b), ptrs(E.a1, E.b1), cs, E.consts(), E.xp[0].ptr, E.xp[1].ptr); E.xp[0].w(); E.xp[1].w()


def _tensor(E):
    E.ok("hc_lv_mul_tensor", E.level, E.a.ptr, E.a1.ptr, E.b.ptr, E.b1.ptr, E.xp[0].ptr, E.xp[1].ptr, E.xp[2].ptr)
    for s in E.xp:
        s.w()


def _mod_raise(lv):
    def fn(E):
        E.ok("hc_lv_mod_raise", E.level if lv is None else lv, E.l1.ptr, E.xp[0].ptr); E.xp[0].w([(0, (E.level if lv is None else lv) + 1)])
    return fn


def _div_round_last(lv, two):
    def fn(E):
        lv_ = E.level if lv is None else lv
        x0, x1 = (E.a, E.b) if lv is None else (E.la, E.lb) if lv == LOW else (E.l1, E.l1)
        if two:
            E.ok("hc_div_round_last2", lv_, x0.ptr, x1.ptr, E.xp[0].ptr, E.xp[1].ptr); E.xp[0].w([(0, lv_)]); E.xp[1].w([(0, lv_)])
        else:
            E.ok("hc_div_round_last", lv_, x0.ptr, E.xp[0].ptr); E.xp[0].w([(0, lv_)])
    return fn


def _keyswitch(lv):
    def fn(E):
        lv_, x, k = (E.level, E.a, K0) if lv is None else (lv, E.la, K_LOW)
        E.ok("hc_keyswitch", U(k), lv_, x.ptr, E.xp[0].ptr, E.xp[1].ptr); E.xp[0].w([(0, lv_ + 1)]); E.xp[1].w([(0, lv_ + 1)])
    return fn


def _keyswitch_add(rescale):
    def fn(E):
        E.ok("hc_keyswitch_add_rescale" if rescale else "hc_keyswitch_add", U(K0), E.level, E.a.ptr, E.b.ptr, E.b1.ptr, E.xp[0].ptr, E.xp[1].ptr)
        E.xp[0].w([(0, E.nl - (1 if rescale else 0))]); E.xp[1].w([(0, E.nl - (1 if rescale else 0))])
    return fn


def _ks_rotate_plain(E):
    E.ok("hc_keyswitch_rotate", U(K1), U(GAL), E.level, E.b.ptr, E.a.ptr, E.xp[0].ptr, E.xp[1].ptr, 0); E.xp[0].w(); E.xp[1].w()


def _ks_qp_plain(E):
    E.ok("hc_keyswitch_qp", U(K0), E.level, E.a.ptr, E.xq[0].ptr, 0); E.xq[0].w()


def _ks_qp_rotate_plain(E):
    E.ok("hc_keyswitch_qp_rotate", U(K0), U(GAL), E.level, E.b.ptr, E.a.ptr, E.xq[0].ptr, 0, 0); E.xq[0].w()


def _decompose_other(lv):
    def fn(E):
        E.ok("hc_keyswitch_decompose", E.level if lv is None else lv, (E.a if lv is None else E.la).ptr)
    return fn


def _mod_down2(lv, rescale):
    def fn(E):
        lv_, x = (E.level, E.X) if lv is None else (lv, E.lX)
        ntl = lv_ + 1 + E.alpha
        if rescale:                         # row `level` of both components of x is documented scratch
            E.ok("hc_mod_down2_add_rescale", lv_, x.ptr, None, None, E.xp[0].ptr, E.xp[1].ptr)
            x.w([(lv_, 1), (ntl + lv_, 1)]); E.xp[0].w([(0, lv_)]); E.xp[1].w([(0, lv_)])
        else:
            E.ok("hc_mod_down2", lv_, x.ptr, E.xp[0].ptr, E.xp[1].ptr); E.xp[0].w([(0, lv_ + 1)]); E.xp[1].w([(0, lv_ + 1)])
    return fn


def _qp_op2(op, shared=False, acc=False):
    def fn(E):
        h = E.nt * N
        out = E.accq if acc else E.xq[0]
        E.ok("hc_qp_op2", op, E.level, E.X.ptr, E.X.at(h), (E.ptq if shared else E.Y).ptr, None if shared else E.Y.at(h), out.ptr, out.at(h)); out.w()
    return fn


def _qp_mul_sum(E):
    E.ok("hc_qp_mul_sum", E.level, 2, ptrs(E.X, E.Y), ptrs(E.ptq, E.ptq), E.xq[0].ptr, 0); E.xq[0].w()


def _qp_mul_sum2(E):
    E.ok("hc_qp_mul_sum2", E.level, 2, ptrs(E.X, E.Y), ptrs(E.ptq, None), ptrs(None, E.ptq), E.xq[0].ptr, E.accq.ptr, 0, 1); E.xq[0].w(); E.accq.w()


def _qp_mul_sum_many(E):
    E.ok("hc_qp_mul_sum_many", E.level, 2, 2, ptrs(E.X, E.Y), ptrs(E.ptq, E.ptq, None, E.ptq), ptrs(E.xq[0], E.xq[1]), (C.c_int * 2)(0, 0)); E.xq[0].w(); E.xq[1].w()


def _swk_load(E):
    E.ctx.swk_load(50, E.level, E.keys[K1])


def _swk_generate(E):
    E.ok("hc_swk_generate", U(51), E.level, U(GAL), E.sk.ptr, (C.c_uint32 * 8)(*range(1, 9)))


def _swk_generate_splitmix(E):
    es = np.zeros(E.beta * N, dtype=np.int64); es[::7] = 3; es[::11] = -5
    E.ok("hc_swk_generate_splitmix", U(52), E.level, U(0), E.sk.ptr, U(0x5EED), es.ctypes.data_as(C.POINTER(C.c_int64)))


def _encode_slots(ex, to_ntt=1):
    def fn(E):
        vals = E.xr                                   # the values are overwritten in place: they are an output too
        vals.put(np.concatenate([E.dbl.data.reshape(-1)[:N], np.zeros((E.xr.rows - 1) * N, dtype=np.uint64)]).reshape(1, E.xr.rows, N))
        out = E.xr.at(N)
        if ex:
            E.ok("hc_encode_slots_ex", vals.ptr, 1, 13, E.level, 1, 2.0 ** 30, to_ntt, out); E.xr.w([(0, 1)]); E.xr.w([(1, E.nt)])
        else:
            E.ok("hc_encode_slots", vals.ptr, 1, E.level, 2.0 ** 30, to_ntt, out); E.xr.w([(0, 1 + E.nl)])
    return fn


def _encode_coeffs(to_ntt):
    def fn(E):
        E.ok("hc_encode_coeffs", E.dbl.at(N), 1, N, E.level, 2.0 ** 20, to_ntt, E.xr.ptr); E.xr.w([(0, E.nl)])
    return fn


def _encrypt_sk(E):
    E.ok("hc_encrypt_sk", 1, 1, E.ct1.ptr, E.sk.ptr, (C.c_uint32 * 8)(*range(2, 10)), U(5), (C.c_void_p * 1)(E.xr.ptr)); E.xr.w([(0, 4)])


def _decrypt_decode_coeffs(E):
    E.ok("hc_decrypt_decode_coeffs", 1, 1, (C.c_void_p * 1)(E.ct1.ptr), E.sk.ptr, 2.0 ** 30, E.xr.ptr); E.xr.w([(0, 1)])


def _decrypt_decode_slots(E):
    E.ok("hc_decrypt_decode_slots", 1, 1, (C.c_void_p * 1)(E.ct1.ptr), E.sk.ptr, 2.0 ** 30, 15, E.xr.ptr); E.xr.w([(0, 1)])


def _decrypt_decode_lv(E):
    E.ok("hc_decrypt_decode_lv", 1, E.level, (C.c_void_p * 1)(E.a.ptr), (C.c_void_p * 1)(E.b.ptr), E.sk.ptr, 2.0 ** 30, -1, E.xr.ptr); E.xr.w([(0, 1)])


def _decode_slots(E):
    E.ok("hc_decode_slots", E.dbl.at(N), 1, 15, E.xr.ptr); E.xr.w([(0, 1)])


def _decode_coeffs(lv):
    def fn(E):
        E.ok("hc_decode_coeffs", (E.a if lv is None else E.la).ptr, 1, E.level if lv is None else lv, 1, 2.0 ** 30, E.xr.ptr); E.xr.w([(0, 1)])
    return fn


def _set_batch_same(E):
    E.ok("hc_set_batch", E.n, E.PS if E.n > 1 else 0, E.QS if E.n > 1 else 0)


def _set_batch_other(E):
    """two images where there were one or three; the consumer that follows runs on two images (its words for them are those of the full batch: results are per image)"""
    E.ok("hc_set_batch", 2, E.PS, E.QS)
    E.restore.append(lambda: E.ctx.set_batch(E.n, E.PS, E.QS))


def _set_option(name, value, back):
    def fn(E):
        v = value(E) if callable(value) else value
        E.ok("hc_set_option", name.encode(), v)
        if back is not None:
            E.restore.append(lambda: E.ctx.set_option(name, back(E) if callable(back) else back))
    return fn


def _lv_mul_sum(E):
    rc = E.call("hc_lv_mul_sum", E.level, (C.c_void_p * 1)(E.ct8.ptr), E.a.ptr, 1, E.xr.ptr)
    if E.ctx.L.hc_row_is32(E.h, 2):           # pack32 = 2: the baseline's tap sum is refused, with nothing written
        assert rc == HC_ERR_UNSUPPORTED, rc
        return
    assert rc == HC_OK, rc
    E.xr.w([(0, 2 * E.nl)])


def _l0(name):
    def fn(E):
        r = E.r8
        if name in ("hc_ntt", "hc_intt"):
            E.ok(name, 0, r.ptr, E.xr.ptr, 2)
        elif name == "hc_mul_const":
            E.ok(name, 0, r.ptr, U(12345), E.xr.ptr, 2)
        elif name == "hc_permute":
            E.ok(name, U(GAL), r.ptr, E.xr.ptr, 2)
        else:
            E.ok(name, 0, r.ptr, r.at(2 * N), E.xr.ptr, 2)
        E.xr.w([(0, 2)])
    return fn


def _malloc_free(E):
    """what the host's block pool does between a decomposition and its consumers: another block comes and goes"""
    p = C.c_void_p()
    E.ok("hc_malloc", 3 * N * 8, C.byref(p))
    E.ok("hc_copy", p, E.a.ptr, 3 * N * 8)
    E.ok("hc_free", p)


def _copy(E):
    E.ok("hc_copy", E.xp[0].ptr, E.a.ptr, E.nl * N * 8); E.xp[0].w()


def _upload_download(E):
    host = np.arange(N, dtype=np.uint64)
    E.ok("hc_upload", E.xr.ptr, host.ctypes.data_as(C.c_void_p), N * 8); E.xr.w([(0, 1)])
    E.ok("hc_download", host.ctypes.data_as(C.c_void_p), E.a.ptr, N * 8)
    E.ok("hc_sync")


def _idx_load(E):
    E.ok("hc_idx_load", None)


def _conv_loop_a(E):
    """the convolution's first phase on limbs 0 and 1 (kernel plaintexts loaded from the host and from the device, loop A into the intruder's rows, the handle read back):
    the L1 path shares ws_tmp with the leveled transforms"""
    ker = np.ascontiguousarray(E.ct1.data.reshape(2, 2, N))
    k, k2 = C.c_void_p(), C.c_void_p()
    E.ok("hc_ker_load", ker.ctypes.data_as(C.POINTER(U)), 2, C.byref(k))
    E.ok("hc_ker_load_device", E.ct1.ptr, 2, C.byref(k2))
    E.ok("hc_conv_mult_phase", E.ct1.ptr, 2.0 ** 30, k, 2.0 ** 30, 2, 1, 2.0 ** 30, E.xr.ptr); E.xr.w([(0, 4)])
    back = np.empty((2, 2, N), dtype=np.uint64)
    E.ok("hc_ker_download", k2, back.ctypes.data_as(C.POINTER(U)))
    E.L.hc_ker_free(E.h, k); E.L.hc_ker_free(E.h, k2)


def _prep_ker(which):
    def fn(E):
        ker, bn = np.linspace(-1, 1, 9 * 4 * 4), np.ones(4)
        k = E.ctx.prep_ker(ker, bn, 16, 3, 4, 4, trans=which == "ex", dilation=2 if which == "ex2" else 1)
        E.ctx.ker_free(k)
    return fn


def _bl_post_ker(E):
    E.ok("hc_bl_post_ker_slots", E.dbl.ptr, 16, 3, 1, 4, 0, E.xr.ptr); E.xr.w([(0, 9)])


INTRUDERS = {
    # the consumers themselves, one after another
    **{f"consumer:{c}": (CONSUMERS[c][0], _as_intruder(c)) for c in CONSUMERS},
    # leveled arithmetic at the held level, and at another where a scratch array's size goes by the level
    "lv_ntt": ("hc_lv_ntt", _lv("hc_lv_ntt")), "lv_ntt@low": ("hc_lv_ntt", _lv("hc_lv_ntt", LOW)),
    "lv_intt": ("hc_lv_intt", _lv("hc_lv_intt")), "lv_intt@low": ("hc_lv_intt", _lv("hc_lv_intt", LOW)),
    "lv_mul": ("hc_lv_mul", _lv("hc_lv_mul")), "lv_mul_acc": ("hc_lv_mul_acc", _lv("hc_lv_mul_acc", acc=True)),
    "lv_mul_plain": ("hc_lv_mul_plain", _lv("hc_lv_mul_plain", shared=True)), "lv_mul_acc_plain": ("hc_lv_mul_acc_plain", _lv("hc_lv_mul_acc_plain", shared=True, acc=True)),
    "lv_add": ("hc_lv_add", _lv("hc_lv_add")), "lv_sub": ("hc_lv_sub", _lv("hc_lv_sub")),
    "lv_mul_const": ("hc_lv_mul_const", _lv("hc_lv_mul_const", const=True)), "lv_add_const": ("hc_lv_add_const", _lv("hc_lv_add_const", const=True)),
    "lv_op2:add": ("hc_lv_op2", _op2(1)), "lv_op2:mul_const": ("hc_lv_op2", _op2(3, const=True)), "lv_op2:mul_acc_plain": ("hc_lv_op2", _op2(9, shared=True, acc=True)),
    "rotate_finish": ("hc_rotate_finish", _rotate_finish), "lv_permute": ("hc_lv_permute", _lv_permute), "qp_permute2": ("hc_qp_permute2", _qp_permute2),
    "lv_lincomb2": ("hc_lv_lincomb2", _lincomb2), "lv_mul_tensor": ("hc_lv_mul_tensor", _tensor),
    "lv_mod_raise": ("hc_lv_mod_raise", _mod_raise(None)), "lv_mod_raise@low": ("hc_lv_mod_raise", _mod_raise(LOW)),
    "div_round_last": ("hc_div_round_last", _div_round_last(None, False)), "div_round_last@low": ("hc_div_round_last", _div_round_last(LOW, False)),
    "div_round_last@1": ("hc_div_round_last", _div_round_last(1, False)),
    "div_round_last2": ("hc_div_round_last2", _div_round_last(None, True)), "div_round_last2@low": ("hc_div_round_last2", _div_round_last(LOW, True)),
    "div_round_last2@1": ("hc_div_round_last2", _div_round_last(1, True)),
    # key switching, in the forms that decompose by themselves
    "keyswitch": ("hc_keyswitch", _keyswitch(None)), "keyswitch@low": ("hc_keyswitch", _keyswitch(LOW)),
    "keyswitch_add": ("hc_keyswitch_add", _keyswitch_add(False)), "keyswitch_add_rescale": ("hc_keyswitch_add_rescale", _keyswitch_add(True)),
    "keyswitch_rotate:plain": ("hc_keyswitch_rotate", _ks_rotate_plain), "keyswitch_qp:plain": ("hc_keyswitch_qp", _ks_qp_plain),
    "keyswitch_qp_rotate:plain": ("hc_keyswitch_qp_rotate", _ks_qp_rotate_plain),
    "keyswitch_decompose:other": ("hc_keyswitch_decompose", _decompose_other(None)), "keyswitch_decompose:other@low": ("hc_keyswitch_decompose", _decompose_other(LOW)),
    "mod_down2": ("hc_mod_down2", _mod_down2(None, False)), "mod_down2@low": ("hc_mod_down2", _mod_down2(LOW, False)),
    "mod_down2_add_rescale": ("hc_mod_down2_add_rescale", _mod_down2(None, True)), "mod_down2_add_rescale@low": ("hc_mod_down2_add_rescale", _mod_down2(LOW, True)),
    "qp_op2:add": ("hc_qp_op2", _qp_op2(1)), "qp_op2:mul_acc_plain": ("hc_qp_op2", _qp_op2(9, shared=True, acc=True)),
    "qp_mul_sum": ("hc_qp_mul_sum", _qp_mul_sum), "qp_mul_sum2": ("hc_qp_mul_sum2", _qp_mul_sum2), "qp_mul_sum_many": ("hc_qp_mul_sum_many", _qp_mul_sum_many),
    # keys, encoders, the harness' encryptor and decoders
    "swk_load": ("hc_swk_load", _swk_load), "swk_generate": ("hc_swk_generate", _swk_generate), "swk_generate_splitmix": ("hc_swk_generate_splitmix", _swk_generate_splitmix),
    "encode_slots": ("hc_encode_slots", _encode_slots(False)), "encode_slots_ex": ("hc_encode_slots_ex", _encode_slots(True)), "encode_coeffs": ("hc_encode_coeffs", _encode_coeffs(1)),
    # with to_ntt = 0 the encoders run no transform: the other half of the header's "with to_ntt != 0"
    "encode_slots:coeff": ("hc_encode_slots", _encode_slots(False, 0)), "encode_slots_ex:coeff": ("hc_encode_slots_ex", _encode_slots(True, 0)),
    "encode_coeffs:coeff": ("hc_encode_coeffs", _encode_coeffs(0)),
    "encrypt_sk": ("hc_encrypt_sk", _encrypt_sk), "decrypt_decode_coeffs": ("hc_decrypt_decode_coeffs", _decrypt_decode_coeffs),
    "decrypt_decode_slots": ("hc_decrypt_decode_slots", _decrypt_decode_slots), "decrypt_decode_lv": ("hc_decrypt_decode_lv", _decrypt_decode_lv),
    "decode_slots": ("hc_decode_slots", _decode_slots), "decode_coeffs": ("hc_decode_coeffs", _decode_coeffs(None)), "decode_coeffs@low": ("hc_decode_coeffs", _decode_coeffs(LOW)),
    # context state
    "set_batch:same": ("hc_set_batch", _set_batch_same), "set_batch:other": ("hc_set_batch", _set_batch_other),
    "set_option:chunk_nodes": ("hc_set_option", _set_option("chunk_nodes", 32, 64)), "set_option:small_levels": ("hc_set_option", _set_option("small_levels", 0, 16)),
    "set_option:profile": ("hc_set_option", _set_option("profile", 1, 0)), "set_option:peer_access": ("hc_set_option", _set_option("peer_access", 0, 1)),
    "set_option:rot_fuse": ("hc_set_option", _set_option("rot_fuse", 0, 1)), "set_option:small32": ("hc_set_option", _set_option("small32", 0, 1)),
    "set_option:small_mm_wgs": ("hc_set_option", _set_option("small_mm_wgs", lambda E: 1 << 30, lambda E: E.wgs0)),
    "set_option:pack32": ("hc_set_option", _set_option("pack32", lambda E: E.ctx.L.hc_row_is32(E.h, 2) + 1, None)),      # to the value in force: any other would change the rows of every operand
    # one-row primitives, memory, the level-0 / 1 convolution path
    "lv_mul_sum": ("hc_lv_mul_sum", _lv_mul_sum),
    **{n_[3:]: (n_, _l0(n_)) for n_ in ("hc_ntt", "hc_intt", "hc_mul", "hc_add", "hc_sub", "hc_mul_const", "hc_permute")},
    "malloc_copy_free": ("hc_malloc", _malloc_free), "free": ("hc_free", _malloc_free), "copy": ("hc_copy", _copy),
    "upload": ("hc_upload", _upload_download), "download": ("hc_download", _upload_download), "sync": ("hc_sync", _upload_download),
    "idx_load": ("hc_idx_load", _idx_load), "ker_load": ("hc_ker_load", _conv_loop_a), "ker_load_device": ("hc_ker_load_device", _conv_loop_a),
    "conv_mult_phase": ("hc_conv_mult_phase", _conv_loop_a), "ker_download": ("hc_ker_download", _conv_loop_a),
    "prep_ker": ("hc_prep_ker", _prep_ker("")), "prep_ker_ex": ("hc_prep_ker_ex", _prep_ker("ex")), "prep_ker_ex2": ("hc_prep_ker_ex2", _prep_ker("ex2")),
    "bl_post_ker_slots": ("hc_bl_post_ker_slots", _bl_post_ker),
}
# entries that run the very same call as another entry: run once
_SAME_CALL = {"free": "malloc_copy_free", "download": "upload", "sync": "upload", "ker_load_device": "ker_load", "conv_mult_phase": "ker_load", "ker_download": "ker_load"}
INTRUDER_KEYS = [k for k in INTRUDERS if k not in _SAME_CALL]
INTRUDER_PARTS = 3                         # the table in thirds, so that one parametrised case of the device's full product stays at a few seconds


def intruder_part(i):
    return INTRUDER_KEYS[i::INTRUDER_PARTS]

EXCLUDED = {
    "hc_ctx_create": "makes a context; takes none",
    "hc_version": "takes no context",
    "hc_device_count": "takes no context",
    "hc_copy_peer": "two contexts: tests/test_gpu_b_sharded.py",
    "hc_conv_then_pack_sharded": "several contexts: tests/test_gpu_b_sharded.py",
    "hc_evk_load": "level-0 keys need a context with ONE special prime (HC_ERR_UNSUPPORTED here: these contexts have two or three)",
    "hc_keyswitch_l0": "needs hc_evk_load's key: no context that can hold a general decomposition with alpha >= 2 has one",
    "hc_rotate_gal_l0": "needs hc_evk_load's key (its permitted aliasing is tested on a context of its own: case_rotate_gal_l0_in_place)",
    "hc_conv_then_pack": "its pack tree needs hc_evk_load's keys; loop A, which shares ws_tmp, is in the table as hc_conv_mult_phase",
    "hc_conv_then_pack_batch": "as hc_conv_then_pack",
    "hc_pack_ctxts": "needs hc_evk_load's keys",
    "hc_pack_ctxts_strided": "needs hc_evk_load's keys",
    "hc_row_is32": "reads one field of the context; queues nothing, changes nothing",
    "hc_timer_start": "records an event; no kernel, no state a key switch reads",
    "hc_timer_stop": "as hc_timer_start",
    "hc_profile_get": "reads the profile's totals",
    "hc_profile_names": "reads the profile's names",
}

# Settled outcomes. MUST_SURVIVE: rc 0 and the right words - the host's linear transform and hoisted rotations re-decompose nothing. The calls the product host makes
# between a decomposition and its last consumer, read off the source:
#   Boot::linear_transform_qp (host/hconv_relu.cpp): hc_malloc (block_qp2 per rotation), hc_keyswitch_qp_rotate_many or hc_keyswitch_qp_rotate(hoisted = 1); on the
#     stale-digit path of the stock bootstrap hc_keyswitch_qp(hoisted = 1), hc_malloc, hc_copy, hc_lv_add, hc_qp_permute2 and hc_free of the per-rotation blocks
#   preConv_BL (host/hconv_bl.cpp): hc_malloc (bl_alloc), hc_copy, hc_keyswitch_hoisted, hc_add, hc_permute
MUST_SURVIVE = {f"consumer:{c}" for c in CONSUMERS} | {"mod_down2", "mod_down2_add_rescale", "decode_coeffs", "decode_coeffs@low", "div_round_last@1", "div_round_last2@1",
                                                       "encode_slots:coeff", "encode_slots_ex:coeff", "encode_coeffs:coeff",
                                                       "malloc_copy_free", "copy", "lv_add", "qp_permute2", "add", "permute"}
# MUST_REFUSE: HC_ERR_STATE and untouched outputs - the call rewrote the scratch the digits lie in, or the setting they were taken under
MUST_REFUSE = {"keyswitch", "keyswitch@low", "keyswitch_decompose:other", "keyswitch_decompose:other@low", "div_round_last", "div_round_last@low", "div_round_last2",
               "div_round_last2@low", "keyswitch_add", "keyswitch_add_rescale", "keyswitch_rotate:plain", "keyswitch_qp:plain", "keyswitch_qp_rotate:plain",
               "mod_down2@low", "mod_down2_add_rescale@low", "lv_mod_raise", "lv_mod_raise@low", "set_batch:other"}

def declared_entry_points():
    names = []
    for path in HEADERS:
        with open(path) as f:
            names += re.findall(r"\bint (hc_\w+)\(", f.read())
    return names


def check_table_is_complete(intruders=None, excluded=None):
    intruders, excluded = INTRUDERS if intruders is None else intruders, EXCLUDED if excluded is None else excluded
    declared = declared_entry_points()
    assert len(declared) > 80 and "hc_swk_generate_splitmix" in declared, "the headers were not parsed"
    placed = {v[0] for v in intruders.values()}
    missing = sorted(set(declared) - placed - set(excluded))
    assert not missing, f"entry points in neither INTRUDERS nor EXCLUDED (place them: a held decomposition must survive them or be dropped by them): {missing}"
    both = sorted(placed & set(excluded))
    assert not both, f"both run and excluded: {both}"
    gone = sorted((placed | set(excluded)) - set(declared))
    assert not gone, f"no longer declared: {gone}"
    assert MUST_SURVIVE <= set(intruders) and MUST_REFUSE <= set(intruders) and not (MUST_SURVIVE & MUST_REFUSE)


def sequence(E, ikey, cname, make_oracle=None):
    """decompose(cx); intruder; consumer - refused with untouched outputs, or right. Returns the consumer's rc."""
    ref = consumer_reference(E, cname, make_oracle)
    what = f"decompose; {ikey}; {cname} (n={E.n}, alpha={E.alpha})"
    prepare_consumer(E, cname)
    E.ok("hc_keyswitch_decompose", E.level, E.cx.ptr)
    try:
        INTRUDERS[ikey][1](E)
        full = E.n
        if ikey == "set_batch:other":
            E.n = 2                                                        # the consumer's declared writes: two images
            for s in E.cp + E.cq:
                s.images = 2
        try:
            rc, res = run_consumer(E, cname, what)
        finally:
            E.n = full
            for s in E.cp + E.cq:
                s.images = full
    finally:
        while E.restore:
            E.restore.pop()()
    if rc == HC_OK:
        for i, (g, w) in enumerate(zip(res, ref)):
            pc.eq(g, w[: g.shape[0]], f"{what}: HC_OK with a stale decomposition, output {i}")
    if ikey in MUST_SURVIVE:
        assert rc == HC_OK, f"{what}: refused ({E.L.hc_last_error(E.h).decode()}) - the host would have to decompose again"
    if ikey in MUST_REFUSE:
        assert rc == HC_ERR_STATE, f"{what}: rc {rc}, must be refused with HC_ERR_STATE"
    return rc


def case_held_decomposition(E, cname, ikeys=None, make_oracle=None):
    """Part A over a list of intruders; returns {intruder: rc} (the table the header's paragraph above hc_keyswitch_decompose is written from)"""
    return {k: sequence(E, k, cname, make_oracle) for k in (INTRUDER_KEYS if ikeys is None else ikeys)}


def case_wrong_pointer_or_level(E):
    """a consumer given another pointer with the same contents, or the same pointer at another level, is refused before anything is launched"""
    for cname in CONSUMERS:
        real = E.cx
        for twin, lv in ((E.cx_twin, E.level), (real, LOW)):
            prepare_consumer(E, cname)
            E.ok("hc_keyswitch_decompose", E.level, real.ptr)
            E.cx, held = twin, E.level
            E.level = lv
            if lv != held:
                E.k0 = E.k1 = K_LOW                     # a key of THAT level, so that the key check passes and the comparison of the levels is what refuses
            try:
                rc = CONSUMERS[cname][2](E, consumer_outs(E))
            finally:
                E.cx, E.level, E.k0, E.k1 = real, held, K0, K1
            E.A.verify(f"{cname} on {'another pointer' if twin is not real else 'another level'}")
            assert rc == HC_ERR_STATE, f"{cname} with {'another pointer of identical contents' if twin is not real else 'the held pointer at another level'}: rc {rc}"


def case_scratch_growth(make_ctx, level=4, alpha=3):
    """A decomposition taken at level 1 on a FRESH context (ws_mm sized for level 1), an intruder at the top level that makes ws_mm grow - the block the digits lay in is
    gone -, then the consumer at level 1; and the same with the levels exchanged (no growth, another layout). Either refusal or the words of decompose; consumer."""
    for dec_lv, x_lv in ((1, level), (level, 1)):
        for intruder in ("mod_down2", "keyswitch_qp:plain", "lv_mod_raise", "div_round_last2"):
            Q, P = chain(level, alpha)
            ctx, E = make_ctx(Q, P), None
            try:
                E = Env(ctx, level, 1, arena_rows=8 * (level + 3) + 4 * (2 * (level + 1 + alpha) + 3) + 8)
                E.keys = {K0: E.key_rows(dec_lv), K1: E.key_rows(x_lv)}
                ctx.swk_load(K0, dec_lv, E.keys[K0]); ctx.swk_load(K1, x_lv, E.keys[K1])
                cx, xa, xb, xq = E.poly(dec_lv), E.poly(x_lv), E.poly(x_lv), E.qp(x_lv)
                row = E.poly(0)
                o0, o1, x0, x1, xo = E.poly(data=False), E.poly(data=False), E.poly(data=False), E.poly(data=False), E.qp(data=False)

                def consumer():
                    return E.call("hc_keyswitch_hoisted", U(K0), dec_lv, cx.ptr, o0.ptr, o1.ptr)
                E.ok("hc_keyswitch_decompose", dec_lv, cx.ptr)
                if intruder == "mod_down2":
                    E.ok("hc_mod_down2", x_lv, xq.ptr, x0.ptr, x1.ptr); x0.w([(0, x_lv + 1)]); x1.w([(0, x_lv + 1)])
                elif intruder == "keyswitch_qp:plain":
                    E.ok("hc_keyswitch_qp", U(K1), x_lv, xa.ptr, xo.ptr, 0); xo.w([(0, 2 * (x_lv + 1 + alpha))])
                elif intruder == "lv_mod_raise":
                    E.ok("hc_lv_mod_raise", x_lv, row.ptr, x0.ptr); x0.w([(0, x_lv + 1)])
                else:
                    E.ok("hc_div_round_last2", x_lv, xa.ptr, xb.ptr, x0.ptr, x1.ptr); x0.w([(0, x_lv)]); x1.w([(0, x_lv)])
                rc = consumer()
                what = f"decompose at level {dec_lv}; {intruder} at level {x_lv}; hoisted at level {dec_lv}"
                assert rc in (HC_OK, HC_ERR_STATE), f"{what}: rc {rc}"
                if rc == HC_OK:
                    o0.w([(0, dec_lv + 1)]); o1.w([(0, dec_lv + 1)])
                got = E.A.verify(what)
                if rc == HC_OK:
                    res = [o0.read(got)[:, : dec_lv + 1], o1.read(got)[:, : dec_lv + 1]]
                    o0.fill(); o1.fill()
                    E.ok("hc_keyswitch_decompose", dec_lv, cx.ptr)
                    assert consumer() == HC_OK
                    o0.w([(0, dec_lv + 1)]); o1.w([(0, dec_lv + 1)])
                    got = E.A.verify(what + " (reference)")
                    pc.eq(res[0], o0.read(got)[:, : dec_lv + 1], what + ": d0"); pc.eq(res[1], o1.read(got)[:, : dec_lv + 1], what + ": d1")
            finally:
                if E is not None:
                    E.close()
                ctx.close()


def case_freed_and_recycled(make_ctx, level=4, alpha=3):
    """Under option async_alloc = 1 a freed block of a size is the next block of that size: cx is freed after the decomposition, allocated again - the SAME address, which
    the test asserts as its precondition - and filled with another polynomial. The held digits are those of the old contents: the consumer must be refused."""
    Q, P = chain(level, alpha)
    ctx = make_ctx(Q, P, async_alloc=1)
    try:
        rng = np.random.default_rng(0xF4EE)
        nl, nt = level + 1, level + 1 + alpha
        beta = (nl + alpha - 1) // alpha
        key = np.stack([rng.integers(0, (Q[t] if t < nl else P[t - nl]), N, dtype=np.uint64) for _ in range(2 * beta) for t in range(nt)])
        ctx.swk_load(K0, level, key.reshape(beta, 2, nt, N))
        data = [ctx.pack_rows(np.stack([rng.integers(0, Q[l], N, dtype=np.uint64) for l in range(nl)]), nl) for _ in range(2)]
        out = ctx.buf(np.full(2 * nl * N, FILL, dtype=np.uint64))
        for contains in (False, True):                  # cx is the block; cx lies inside the block
            extra = N if contains else 0
            blk = ctx.buf(nwords=nl * N + extra)
            blk.upload(data[0], extra)
            ctx._ck(ctx.L.hc_keyswitch_decompose(ctx.h, level, blk.at(extra)))
            addr = blk.ptr.value
            blk.free()
            blk = ctx.buf(nwords=nl * N + extra)
            assert blk.ptr.value == addr, "precondition: under async_alloc = 1 the allocator hands the freed block out again for the same size"
            blk.upload(data[1], extra)
            rc = ctx.L.hc_keyswitch_hoisted(ctx.h, U(K0), level, blk.at(extra), out.at(0), out.at(nl * N))
            assert rc == HC_ERR_STATE, f"a consumer on a freed and recycled cx ({'inside' if contains else 'at the start of'} the block) returned {rc}: stale digits"
            assert (out.download() == np.uint64(FILL)).all(), "a refused consumer wrote to its outputs"
            blk.free()
        out.free()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ Part B
# An operation of Part B: groups of slots - (names, kind, role) - and a call over the dict of carved slots. A group of two (or three) names is a pair of polynomials that the
# entry point takes as separate pointers; placement acts on groups. kinds: "p" polynomial at the level, "r" polynomial one level down (the rescaling calls' outputs), "c" one
# component of an extended-basis pair, "x" a whole pair, "P" / "C" one plaintext for all images (polynomial / extended basis). roles: "in", "out", "acc" (read and written).
def _spec(groups, call, pre=None, segs=None):
    return {"groups": groups, "call": call, "pre": pre, "segs": segs or {}}


def _p_lv_op2(op):
    shared, const, acc = op in (8, 9), op == 3, op in (7, 9)
    groups = [(("a0", "a1"), "p", "in")]
    if shared:
        groups.append((("b0",), "P", "in"))
    elif not const:
        groups.append((("b0", "b1"), "p", "in"))
    groups.append((("o0", "o1"), "p", "acc" if acc else "out"))

    def call(E, S):
        E.ok("hc_lv_op2", op, E.level, S["a0"].ptr, S["a1"].ptr, None if const else S["b0"].ptr, None if const or shared else S["b1"].ptr, S["o0"].ptr, S["o1"].ptr,
             E.fixed_consts if const else None)
    return _spec(groups, call)


def _p_qp_op2(op):
    shared, acc = op in (8, 9), op in (7, 9)
    groups = [(("a0", "a1"), "c", "in"), ((("b0",), "C", "in") if shared else (("b0", "b1"), "c", "in")), (("o0", "o1"), "c", "acc" if acc else "out")]
    return _spec(groups, lambda E, S: E.ok("hc_qp_op2", op, E.level, S["a0"].ptr, S["a1"].ptr, S["b0"].ptr, None if shared else S["b1"].ptr, S["o0"].ptr, S["o1"].ptr))


def _decomp(name):
    return lambda E, S: E.ok("hc_keyswitch_decompose", E.level, S[name].ptr)


PLACED = {
    **{f"lv_op2:{nm}": _p_lv_op2(op) for op, nm in ((0, "mul"), (1, "add"), (2, "sub"), (3, "mul_const"), (7, "mul_acc"), (8, "mul_plain"), (9, "mul_acc_plain"))},
    "div_round_last2": _spec([(("x0", "x1"), "p", "in"), (("o0", "o1"), "r", "out")],
                             lambda E, S: E.ok("hc_div_round_last2", E.level, S["x0"].ptr, S["x1"].ptr, S["o0"].ptr, S["o1"].ptr)),
    "rotate_finish": _spec([(("d0", "d1"), "p", "in"), (("c0",), "p", "in"), (("o0", "o1"), "p", "out")],
                           lambda E, S: E.ok("hc_rotate_finish", U(GAL), E.level, S["d0"].ptr, S["d1"].ptr, S["c0"].ptr, S["o0"].ptr, S["o1"].ptr)),
    "keyswitch": _spec([(("cx",), "p", "in"), (("d0", "d1"), "p", "out")], lambda E, S: E.ok("hc_keyswitch", U(K0), E.level, S["cx"].ptr, S["d0"].ptr, S["d1"].ptr)),
    "keyswitch_hoisted": _spec([(("cx",), "p", "in"), (("d0", "d1"), "p", "out")],
                               lambda E, S: E.ok("hc_keyswitch_hoisted", U(K0), E.level, S["cx"].ptr, S["d0"].ptr, S["d1"].ptr), pre=_decomp("cx")),
    "keyswitch_rotate": _spec([(("c0", "c1"), "p", "in"), (("o0", "o1"), "p", "out")],
                              lambda E, S: E.ok("hc_keyswitch_rotate", U(K1), U(GAL), E.level, S["c0"].ptr, S["c1"].ptr, S["o0"].ptr, S["o1"].ptr, 0)),
    "keyswitch_rotate:hoisted": _spec([(("c0", "c1"), "p", "in"), (("o0", "o1"), "p", "out")],
                                      lambda E, S: E.ok("hc_keyswitch_rotate", U(K1), U(GAL), E.level, S["c0"].ptr, S["c1"].ptr, S["o0"].ptr, S["o1"].ptr, 1), pre=_decomp("c1")),
    "keyswitch_add": _spec([(("cx",), "p", "in"), (("a0", "a1"), "p", "in"), (("o0", "o1"), "p", "out")],
                           lambda E, S: E.ok("hc_keyswitch_add", U(K0), E.level, S["cx"].ptr, S["a0"].ptr, S["a1"].ptr, S["o0"].ptr, S["o1"].ptr)),
    "keyswitch_add_rescale": _spec([(("cx",), "p", "in"), (("a0", "a1"), "p", "in"), (("o0", "o1"), "r", "out")],
                                   lambda E, S: E.ok("hc_keyswitch_add_rescale", U(K0), E.level, S["cx"].ptr, S["a0"].ptr, S["a1"].ptr, S["o0"].ptr, S["o1"].ptr)),
    "mod_down2": _spec([(("x",), "x", "in"), (("o0", "o1"), "p", "out")], lambda E, S: E.ok("hc_mod_down2", E.level, S["x"].ptr, S["o0"].ptr, S["o1"].ptr)),
    # row `level` of both components of x is the one documented exception to "inputs stay": nothing else of x may change
    "mod_down2_add_rescale": _spec([(("x",), "x", "acc"), (("a0", "a1"), "p", "in"), (("o0", "o1"), "r", "out")],
                                   lambda E, S: E.ok("hc_mod_down2_add_rescale", E.level, S["x"].ptr, S["a0"].ptr, S["a1"].ptr, S["o0"].ptr, S["o1"].ptr),
                                   segs={"x": lambda E: [(E.level, 1), (E.nt + E.level, 1)]}),
    "lv_mul_tensor": _spec([(("a0", "a1"), "p", "in"), (("b0", "b1"), "p", "in"), (("d0", "d1", "d2"), "p", "out")],
                           lambda E, S: E.ok("hc_lv_mul_tensor", E.level, S["a0"].ptr, S["a1"].ptr, S["b0"].ptr, S["b1"].ptr, S["d0"].ptr, S["d1"].ptr, S["d2"].ptr)),
    "qp_op2:add": _p_qp_op2(1), "qp_op2:mul": _p_qp_op2(0), "qp_op2:mul_acc_plain": _p_qp_op2(9),
    "lv_lincomb2": _spec([(("s0", "s1"), "p", "in"), (("t0", "t1"), "p", "in"), (("o0", "o1"), "p", "out")],
                         lambda E, S: E.ok("hc_lv_lincomb2", E.level, 2, ptrs(S["s0"], S["t0"]), ptrs(S["s1"], S["t1"]), E.fixed_consts2, E.fixed_consts, S["o0"].ptr, S["o1"].ptr)),
}
LAYOUTS = ("descending", "in_asc_out_desc", "in_desc_out_asc", "far")


def _order(groups, layout):
    """[(window, name)] in carving order. ascending: the groups one after another, members in order. descending: member 1 of EVERY group, then member 0 of every group,
    so that polynomial 1 lies below polynomial 0 with other operands between them. far: member 0 of every group in the first window, the others in the far one."""
    def asc(gs):
        return [(0, nm) for names, kind, role in gs for nm in names]

    def desc(gs):
        depth = max(len(names) for names, kind, role in gs)
        return [(0, names[i]) for i in reversed(range(depth)) for names, kind, role in gs if i < len(names)]
    ins, outs = [g for g in groups if g[2] == "in"], [g for g in groups if g[2] != "in"]
    if layout == "ascending":
        return asc(groups)
    if layout == "descending":
        return desc(groups)
    if layout == "in_asc_out_desc":
        return asc(ins) + desc(outs)
    if layout == "in_desc_out_asc":
        return desc(ins) + asc(outs)
    assert layout == "far"
    return [(0, names[0]) for names, kind, role in groups] + [(1, nm) for names, kind, role in groups for nm in names[1:]]


def _carve(E, kind, role):
    data = role != "out"
    if kind == "p":
        return E.poly(data=data)
    if kind == "r":
        return E.poly(data=data, rows=E.level)
    if kind == "c":
        return E.qp(data=data, comps=1)
    if kind == "x":
        return E.qp(data=data)
    if kind == "P":
        return E.poly(images=1)
    assert kind == "C"
    return E.qp(comps=1, images=1)


def run_placed(E, name, layout, data=None, alias=None):
    """carve the operation's slots in `layout`, fill them with `data` ({slot: residues}, drawn on the first run), run, verify the footprint; -> (data, {output: payload}).
    alias = {x: y}: slot x IS slot y (and then reads what y holds)"""
    spec, alias = PLACED[name], alias or {}
    E.A.reset()
    kinds = {nm: (kind, role) for names, kind, role in spec["groups"] for nm in names}
    S, first = {}, data is None
    data = {} if first else data
    for window, nm in _order(spec["groups"], layout):
        if nm in alias:
            continue
        E.window = window
        kind, role = kinds[nm]
        S[nm] = _carve(E, kind, role)
        if role != "out":
            if nm in data:
                S[nm].put(data[nm])
            else:
                data[nm] = S[nm].data
    E.window = 0
    for x, y in alias.items():
        S[x] = S[y]
    E.A.verify(f"{name} / {layout}: uploads")
    if spec["pre"]:
        spec["pre"](E, S)
    spec["call"](E, S)
    written = [nm for nm in kinds if kinds[nm][1] != "in"]
    for nm in written:
        S[nm].w(spec["segs"][nm](E) if nm in spec["segs"] else [(0, E.level)] if kinds[nm][0] == "r" else None)
    got = E.A.verify(f"{name} / {layout}{' / ' + str(alias) if alias else ''}")
    return data, {nm: S[nm].read(got) for nm in written}


def _window_rows(ctx, level, n):
    """hc_qp_op2's six components in one window (the ascending layout); seven polynomials are fewer rows"""
    return n * 6 * (2 * (level + 1 + len(ctx.p)) + 3) + 8


def part_b_env(ctx, level, n, far_rows=None):
    """far_rows: the first row of the far window (None: one window). The arena holds the largest operation in each window."""
    win = _window_rows(ctx, level, n)
    nl = level + 1
    if far_rows is None:
        E = Env(ctx, level, n, arena_rows=win)
    else:
        E = Env(ctx, level, n, windows=[(0, win), (far_rows, win)], total_rows=far_rows + win)
    E.fixed_consts = E.consts()
    E.fixed_consts2 = (U * (2 * nl))(*[int(E.rng.integers(1, E.Q[l])) for _ in range(2) for l in range(nl)])
    for kid in (K0, K1):
        ctx.swk_load(kid, level, E.key_rows(level))
    return E


def case_placement(E, name, layouts=LAYOUTS, refs=None):
    """the operation in every layout == the same call on the contiguous ascending one"""
    refs = {} if refs is None else refs
    if name not in refs:
        refs[name] = run_placed(E, name, "ascending")
    data, want = refs[name]
    for layout in layouts:
        if layout == "far" and len(E.A.windows) < 2:
            continue
        _, got = run_placed(E, name, layout, data)
        for nm in want:
            pc.eq(got[nm], want[nm], f"{name} in layout {layout}: output {nm} (n={E.n})")
    return refs


FAR_ROWS = (1 << 32) // (N * 8) + 8            # polynomial 1 more than 4 GiB above polynomial 0


def far_env(ctx, level, n):
    """the arena of the far-apart layout: more than 4 GiB between the windows where the device has room for the allocation, else half of it, and so on (only a failed
    allocation shortens it; any other error is the test's). -> (Env, distance in bytes)"""
    from optimal_conv_amd.abi import HconvError
    rows = FAR_ROWS
    while True:
        try:
            ctx.buf(nwords=(rows + _window_rows(ctx, level, n)) * N).free()
            break
        except HconvError:
            if rows < 64:
                raise
            rows //= 2
    return part_b_env(ctx, level, n, far_rows=rows), rows * N * 8


# the aliased forms the header permits or the host uses: name -> (operation of PLACED or of ALIAS_OPS, {slot: the slot it is})
def _a_lv(name, const=False, unary=False, acc=False):
    groups = [(("a",), "p", "in")] + ([] if const or unary else [(("b",), "p", "in")]) + [(("o",), "p", "acc" if acc else "out")]

    def call(E, S):
        if const:
            E.ok(name, E.level, S["a"].ptr, E.fixed_consts, S["o"].ptr)
        elif unary:
            E.ok(name, E.level, S["a"].ptr, S["o"].ptr)
        else:
            E.ok(name, E.level, S["a"].ptr, S["b"].ptr, S["o"].ptr)
    return _spec(groups, call)


PLACED.update({
    "lv_add": _a_lv("hc_lv_add"), "lv_sub": _a_lv("hc_lv_sub"), "lv_mul": _a_lv("hc_lv_mul"),
    "lv_mul_plain": _spec([(("a",), "p", "in"), (("b",), "P", "in"), (("o",), "p", "out")], lambda E, S: E.ok("hc_lv_mul_plain", E.level, S["a"].ptr, S["b"].ptr, S["o"].ptr)),
    "lv_mul_const": _a_lv("hc_lv_mul_const", const=True), "lv_add_const": _a_lv("hc_lv_add_const", const=True),
    "lv_ntt": _a_lv("hc_lv_ntt", unary=True), "lv_intt": _a_lv("hc_lv_intt", unary=True), "lv_mul_acc": _a_lv("hc_lv_mul_acc", acc=True),
})
PLACEMENT_OPS = [k for k in PLACED if k.split(":")[0] not in ("lv_add", "lv_sub", "lv_mul", "lv_mul_plain", "lv_mul_const", "lv_add_const", "lv_ntt", "lv_intt", "lv_mul_acc")]
ALIASED = [
    *[(op, {"o": "a"}) for op in ("lv_add", "lv_sub", "lv_mul", "lv_mul_plain", "lv_mul_const", "lv_add_const", "lv_ntt", "lv_intt")],
    *[(op, {"o": "b"}) for op in ("lv_add", "lv_sub", "lv_mul")],               # hc_lv_add(a, t, t): mulRelin's and the linear transform's running sums
    ("lv_mul_acc", {"b": "a"}),                                                   # a square added to the accumulator
    *[(f"lv_op2:{nm}", {"o0": "a0", "o1": "a1"}) for nm in ("add", "sub", "mul", "mul_const", "mul_plain")],
    *[(f"lv_op2:{nm}", {"o0": "b0", "o1": "b1"}) for nm in ("add", "sub", "mul")],
    ("keyswitch_add", {"o0": "a0", "o1": "a1"}), ("keyswitch_add", {"o0": "a0"}),   # the second: mulRelin's call
    ("keyswitch_add_rescale", {"o0": "a0", "o1": "a1"}),
]


def case_aliased(E, name, alias):
    """the aliased call == the call on separate slots holding the same residues. A slot that is aliased to an INPUT starts, in the plain run, from that input's data."""
    kinds = {nm: (kind, role) for names, kind, role in PLACED[name]["groups"] for nm in names}
    data, want = run_placed(E, name, "ascending")
    for x, y in alias.items():
        if kinds[x][1] != "out":                      # an aliased input or accumulator reads y's residues: the plain run must have read the same
            data[x] = data[y]
    if any(kinds[x][1] != "out" for x in alias):
        data, want = run_placed(E, name, "ascending", data)
    _, got = run_placed(E, name, "ascending", data, alias)
    for nm in want:
        g, w = got[nm], want[nm]
        pc.eq(g[:, : w.shape[1]], w, f"{name} with {alias}: output {nm} (n={E.n})")


def case_keyswitch_rotate_refuses_aliasing(E):
    """the one aliasing the library refuses itself: HC_ERR_ARG, nothing written, and the context is fine afterwards"""
    E.A.reset()
    c0, c1, o0, o1 = E.poly(), E.poly(), E.poly(data=False), E.poly(data=False)
    for outs in ((c0, o1), (o0, c1), (c1, o1), (o0, c0)):
        rc = E.call("hc_keyswitch_rotate", U(K1), U(GAL), E.level, c0.ptr, c1.ptr, outs[0].ptr, outs[1].ptr, 0)
        assert rc == HC_ERR_ARG, f"hc_keyswitch_rotate with an output on an input returned {rc}"
        E.A.verify("hc_keyswitch_rotate refusing an aliased output")
    E.ok("hc_keyswitch_rotate", U(K1), U(GAL), E.level, c0.ptr, c1.ptr, o0.ptr, o1.ptr, 0); o0.w(); o1.w()
    E.A.verify("hc_keyswitch_rotate after the refusals")


def case_rotate_gal_l0_in_place(make_ctx):
    """hc_rotate_gal_l0 with its outputs on its inputs (conv.go:291 rotates in place) == on separate rows; the level-0 path needs a context with one special prime"""
    from oracle_lib import P0, Q0, Q1
    ctx = make_ctx([Q0, Q1], [P0])
    try:
        A = Arena(ctx, [(0, 12)])
        gal = 513
        ctx.evk_load(gal, pc.seeded_evk(600 + gal))
        ct = np.stack([pc.splitmix_rows(61, Q0, N), pc.splitmix_rows(62, Q0, N)])
        A.put(2 * N, ct); A.put(8 * N, ct)
        ctx._ck(ctx.L.hc_rotate_gal_l0(ctx.h, U(gal), A.at(2 * N), A.at(3 * N), A.at(5 * N), A.at(6 * N))); A.declare(5 * N, 2 * N)
        want = A.verify("hc_rotate_gal_l0")[0][5 * N: 7 * N].copy()
        ctx._ck(ctx.L.hc_rotate_gal_l0(ctx.h, U(gal), A.at(8 * N), A.at(9 * N), A.at(8 * N), A.at(9 * N))); A.declare(8 * N, 2 * N)
        got = A.verify("hc_rotate_gal_l0 in place")[0][8 * N: 10 * N].copy()
        pc.eq(got, want, "hc_rotate_gal_l0 in place == on separate rows")
        A.free()
    finally:
        ctx.close()
