"""The yardstick of the convolution with several input ciphertexts, from the oracle's primitives only (no fused oracle call, no device code): what a Lattigo host
computes with the evaluator it has. Per live output channel i

    acc = MulNew(ct_0, pl_0[i]);  Add(acc, MulNew(ct_j, pl_j[i]), acc), j = 1 .. m-1;  SetScale(acc, out_scale / (max_ob / norm))

(SetScale = MultByConst by conv.go:527-528's constant, then the one DivRoundByLastModulusNTT from level 1 to 0), then pack_ctxts (conv.go:266-300) over the sums and
eval.go:258's bias add. tests/test_multiconv_cpu.py pins this file to the oracle's fused calls at m = 1 before anything is measured against it."""
import numpy as np


def setscale_consts(O, ct_scale, ker_scale, max_ob, norm, out_scale):
    """MultByConst's per-limb integers for SetScale(out_scale / (max_ob / norm)) of a product of scales ct_scale * ker_scale (or_conv_then_pack's own bookkeeping)"""
    target = out_scale / (max_ob // norm)
    constant = target / (ct_scale * ker_scale)
    return [O.const_for(constant, 1, l)[0] for l in range(2)], target


def loopA_sum(O, ct_ins, kers, cst):
    """ct_ins: m ciphertexts (2, 2, N) [poly][limb] at level 1; kers: their plaintexts (2, N) [limb] of ONE output channel; cst (2,) -> the level-0 ciphertext (2, N)"""
    N = O.N
    out = np.empty((2, N), dtype=np.uint64)
    for p in range(2):
        a = np.empty((2, N), dtype=np.uint64)
        for l in range(2):
            acc = O.mul(l, ct_ins[0][p][l], kers[0][l])
            for ct, k in zip(ct_ins[1:], kers[1:]):
                acc = O.add(l, acc, O.mul(l, ct[p][l], k[l]))
            a[l] = O.mul_scalar(l, acc, cst[l])
        out[p] = O.div_round_last(1, a)[0]
    return out


def pack_tree(O, cts, evk_all, max_ob, norm, bias):
    """pack_ctxts over cts (max_ob, 2, N) (slots i % norm == 0 live) with conv.go:288-292's node, then the bias add on polynomial 0. evk_all (16, 4, N) as
    parity_cases.load_tree_keys returns it: the key of Galois element 2^j + 1 at row j - 1."""
    cts = np.array(cts, dtype=np.uint64, copy=True)
    idx = O.idx_plaintexts()
    step, log_step = max_ob // 2, 0
    i = step
    while i > 1:
        log_step += 1
        i //= 2
    j = O.logN - log_step
    while step >= norm and step >= 1:
        gal = (1 << j) + 1
        for i in range(0, step, norm):
            x, y = cts[i + step], cts[i]
            t1 = np.stack([O.mul(0, x[p], idx[log_step]) for p in range(2)])          # conv.go:288
            t2 = np.stack([O.sub(0, y[p], t1[p]) for p in range(2)])                  # :289
            t1 = np.stack([O.add(0, y[p], t1[p]) for p in range(2)])                  # :290
            r = O.rotate_gal_l0(t2, gal, evk_all[j - 1])                              # :291
            cts[i] = np.stack([O.add(0, t1[p], r[p]) for p in range(2)])              # :292
        step //= 2
        log_step -= 1
        j += 1
    out = cts[0].copy()
    if bias is not None:
        out[0] = O.add(0, out[0], bias)
    return out


def multi_conv(O, ct_ins, pl_kers, evk_all, max_ob, norm, bias, ct_scale=2.0 ** 30, ker_scale=2.0 ** 30, out_scale=2.0 ** 30):
    """ONE convolution of the m ciphertexts ct_ins with plaintext sets pl_kers[j] (max_ob, 2, N)"""
    cst, _ = setscale_consts(O, ct_scale, ker_scale, max_ob, norm, out_scale)
    cts = np.zeros((max_ob, 2, O.N), dtype=np.uint64)
    for i in range(0, max_ob, norm):
        cts[i] = loopA_sum(O, ct_ins, [k[i] for k in pl_kers], cst)
    return pack_tree(O, cts, evk_all, max_ob, norm, bias)
