"""Cases of the convolution with several input ciphertexts (hc_conv_then_pack_batch's grouping rule: consecutive members with one ct_out are the inputs of ONE
convolution), shared by the emulated-library tests and the GPU tests. The yardstick is tests/multiconv_ref.py."""
import ctypes as C

import numpy as np

import multiconv_ref as MR
import parity_cases as pc

N = pc.N
S30 = 2.0 ** 30
HC_ERR_ARG = 1
FILL = 0xA5A5A5A5A5A5A5A5

# (m input ciphertexts per convolution, G convolutions per call, max_ob, norm, chunk_nodes or None)
GROUP_TABLE = [(2, 1, 1, 1, None), (3, 1, 4, 1, 3), (5, 1, 2, 1, None), (2, 2, 4, 2, None), (16, 1, 1, 1, None)]


def group_id(t):
    return "m{}-G{}-B{}-norm{}-chunk{}".format(*t)


def group_inputs(seed, m, G, max_ob, O, inputs="random"):
    """ins[g][j] (2, 2, N), kers[g][j] (max_ob, 2, N), bias[g] (N,): every member its own ciphertext and plaintexts"""
    ins, kers, biases = [], [], []
    for g in range(G):
        pairs = [pc.planted_conv_inputs(seed + 1000 * g + 17 * j, max_ob, O, inputs) for j in range(m)]
        ins.append([p[0] for p in pairs]); kers.append([p[1] for p in pairs])
        biases.append(pc.row_source(inputs)(seed + 5 + g, pc.conv_moduli(O)[0]))
    return ins, kers, biases


def run_groups(ctx, ins, kers, biases, max_ob, norm, calls=1):
    """the grouped call through the binding's _dev form; returns the outputs of every call"""
    G = len(ins)
    hk = [[ctx.ker_load(k) for k in ks] for ks in kers]
    bi = [[ctx.buf(x) for x in xs] for xs in ins]
    bb = [ctx.buf(b) if b is not None else None for b in biases]
    bo = [ctx.buf(np.full(2 * N, FILL, dtype=np.uint64)) for _ in range(G)]
    try:
        res = []
        for _ in range(calls):
            sc = ctx.conv_then_pack_multi_dev([(bi[g], hk[g], bb[g], bo[g]) for g in range(G)], S30, S30, max_ob, norm, S30)
            assert sc == S30
            res.append([b.download((2, N)) for b in bo])
        return res
    finally:
        for b in [x for xs in bi for x in xs] + bo + [x for x in bb if x is not None]:
            b.free()
        for h in [x for xs in hk for x in xs]:
            ctx.ker_free(h)


def case_groups(ctx, O, m, G, max_ob, norm, chunk=None, seed=0x6A0, inputs="random", calls=1):
    """G convolutions of m input ciphertexts each == the yardstick, word for word"""
    evk_all = pc.load_tree_keys(ctx, seed, max_ob, norm, O)
    ctx.idx_load(None)
    ins, kers, biases = group_inputs(seed, m, G, max_ob, O, inputs)
    if G > 1:
        biases[1] = None                       # a group without a bias beside one with
    ctx.set_option("chunk_nodes", chunk if chunk is not None else 64)
    try:
        res = run_groups(ctx, ins, kers, biases, max_ob, norm, calls)
    finally:
        ctx.set_option("chunk_nodes", 64)
    for g in range(G):
        want = MR.multi_conv(O, ins[g], kers[g], evk_all, max_ob, norm, biases[g])
        for n, got in enumerate(res):
            pc.eq(got[g], want, f"group {g} of {G}, m={m} B={max_ob} norm={norm} chunk={chunk} inputs={inputs}, call {n}")


def case_multi_binding(ctx, O, seed=0x6B1):
    """Context.conv_then_pack_multi (host arrays in, host array out) at m = 2, no bias"""
    evk_all = pc.load_tree_keys(ctx, seed, 2, 1, O)
    ctx.idx_load(None)
    ins, kers, _ = group_inputs(seed, 2, 1, 2, O)
    got, sc = ctx.conv_then_pack_multi(ins[0], S30, kers[0], S30, 2, 1, S30)
    assert sc == S30
    pc.eq(got, MR.multi_conv(O, ins[0], kers[0], evk_all, 2, 1, None), "conv_then_pack_multi m=2 B=2")


def case_refusals(ctx, O, seed=0x6C2):
    """unequal groups, a non-adjacent repeat of ct_out and a conflicting bias: HC_ERR_ARG each, and the output buffers keep what they held"""
    max_ob = 1
    ct, ker = pc.planted_conv_inputs(seed, max_ob, O)
    hk = ctx.ker_load(ker)
    cin = ctx.buf(ct)
    b0, b1 = ctx.buf(pc.rows(seed + 1, pc.conv_moduli(O)[0])), ctx.buf(pc.rows(seed + 2, pc.conv_moduli(O)[0]))
    outs = [ctx.buf(np.full(2 * N, FILL, dtype=np.uint64)) for _ in range(3)]
    A, B, Cc = outs
    arr = lambda xs: (C.c_void_p * len(xs))(*[(x.ptr if hasattr(x, "ptr") else x) for x in xs])
    cases = [("groups of unequal size", [A, A, B], [b0, None, None]),
             ("groups of unequal size", [A, B, B], [None, None, None]),
             ("groups of unequal size", [A, A, B, B, Cc], None),
             ("non-adjacent", [A, B, A], [None, None, None]),
             ("non-adjacent", [A, A, B, B, A, A], None),
             ("bias of member 1 conflicts", [A, A], [b0, b1]),
             ("bias of member 1 conflicts", [A, A], [None, b1]),
             ("bias of member 3 conflicts", [A, A, B, B], [b0, b0, b1, b0])]
    try:
        for msg, co, cb in cases:
            n = len(co)
            sc = C.c_double(-1.0)
            rc = ctx.L.hc_conv_then_pack_batch(ctx.h, n, arr([cin] * n), S30, arr([hk] * n), S30, max_ob, 1, S30,
                                               arr([(b.ptr if b is not None else None) for b in cb]) if cb is not None else None, arr(co), C.byref(sc))
            err = ctx.L.hc_last_error(ctx.h).decode()
            assert rc == HC_ERR_ARG and msg in err, (msg, rc, err)
            assert sc.value == -1.0
            for o in outs:
                assert (o.download() == np.uint64(FILL)).all(), f"{msg}: an output buffer was written"
        # the permitted forms of a group's bias entries: the same pointer again, or NULL
        rc = ctx.L.hc_conv_then_pack_batch(ctx.h, 2, arr([cin] * 2), S30, arr([hk] * 2), S30, max_ob, 1, S30, arr([b0.ptr, b0.ptr]), arr([A, A]), None)
        assert rc == 0, ctx.L.hc_last_error(ctx.h).decode()
        first = A.download()
        rc = ctx.L.hc_conv_then_pack_batch(ctx.h, 2, arr([cin] * 2), S30, arr([hk] * 2), S30, max_ob, 1, S30, arr([b0.ptr, None]), arr([B, B]), None)
        assert rc == 0, ctx.L.hc_last_error(ctx.h).decode()
        pc.eq(B.download(), first, "bias named twice vs once")
    finally:
        for b in outs + [cin, b0, b1]:
            b.free()
        ctx.ker_free(hk)


def case_distinct_outputs_unchanged(ctx, O, seed=0x6D3):
    """all ct_out distinct (m = 1): the batch == separate hc_conv_then_pack calls == the oracle, and only the one-input kernels are launched"""
    ctx.set_option("profile", 1)
    try:
        ctx.profile_reset()
        pc.case_conv_batch(ctx, O, 2, 3, seed=seed)
        names = set(ctx.profile())
    finally:
        ctx.set_option("profile", 0)
    assert {"a1_mul_rowsinv", "a3_rowsfwd_rescale"} <= names and not any(n.startswith(("a1g", "a3g")) for n in names), names


def case_branch(make_ctx, triple, inputs, ms=(2, 4, 5, 16)):
    """one modulus-size branch of the convolution at every m of `ms`: one channel through the grouped a1 / a2 / a3 (the kernels branch on the modulus only)"""
    ctx, O = pc._triple_env(make_ctx, triple)
    try:
        ctx.set_option("small_levels", 0)
        for m in ms:
            case_groups(ctx, O, m, 1, 2 if m == 2 else 1, 1, seed=0x6E4 + m, inputs=inputs)
    finally:
        ctx.close()
