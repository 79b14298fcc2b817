"""A numpy restatement of the reference's plaintext layout for Conv and TransConv: prep_Input (main.go:1007-1042),
reshape_ker (conv.go:184-202), prep_Ker's BN scaling and max_bat embedding (conv.go:487-508), encode_ker_final (conv.go:206-237),
the negacyclic product of conv_then_pack (conv.go:527) and the packing tree of pack_ctxts (conv.go:266-300) on plain polynomials.
Every function takes the ring degree N, so the layout can be checked exactly on small rings and on integer data."""
import numpy as np


def prep_input(x, raw_in_wid, in_wid, N, norm=1, trans=False):
    """x: (raw, raw, channels) HWC -> length-N coefficient vector"""
    batch = N // (in_wid * in_wid)
    out = np.zeros(N)
    i, j, b = np.meshgrid(np.arange(raw_in_wid), np.arange(raw_in_wid), np.arange(batch // norm), indexing="ij")
    if trans:      # main.go:1011-1021: the odd grid points
        pos = (2 * i + 1) * in_wid * batch + (2 * j + 1) * batch + b * norm
    else:
        pos = i * in_wid * batch + j * batch + b * norm
    out[pos.reshape(-1)] = np.asarray(x, dtype=np.float64).reshape(-1)[:pos.size]
    return out


def reshape_ker(ker_in, k_sz, out_batch, trans):
    """-> ker_out (out_batch, in_batch * k_sz)"""
    ker_in = np.asarray(ker_in, dtype=np.float64).reshape(-1)
    in_batch = len(ker_in) // (k_sz * out_batch)
    if trans:      # ker_out[i][j*k_sz + (k_sz-k-1)] = ker_in[j + i*in_batch + k*out_batch*in_batch]
        K = ker_in.reshape(k_sz, out_batch, in_batch)
        return K.transpose(1, 2, 0)[:, :, ::-1].reshape(out_batch, in_batch * k_sz)
    # ker_out[i][j*k_sz + k] = ker_in[i + j*out_batch + k*out_batch*in_batch]
    K = ker_in.reshape(k_sz, in_batch, out_batch)
    return K.transpose(2, 1, 0).reshape(out_batch, in_batch * k_sz)


def encode_ker_final(ker_in, i, in_wid, in_batch, ker_wid):
    """pos = 0"""
    vec_size, k_sz = in_wid * in_wid * in_batch, ker_wid * ker_wid
    out = np.zeros(vec_size)
    j, k = np.meshgrid(np.arange(in_batch), np.arange(k_sz), indexing="ij")
    out[((in_wid * (k // ker_wid) + k % ker_wid) * in_batch + j).reshape(-1)] = ker_in[i][((in_batch - 1 - j) * k_sz + (k_sz - 1 - k)).reshape(-1)]
    adj = (in_batch - 1) + in_batch * (in_wid + 1) * (ker_wid - 1) // 2
    assert 2 * adj <= vec_size
    tmp = out[vec_size - adj:].copy()
    out[vec_size - adj:] = -out[:adj]
    out[:vec_size - 2 * adj] = out[adj:vec_size - adj].copy()
    out[vec_size - 2 * adj:vec_size - adj] = tmp
    return out


def prep_ker_coeffs(ker_in, bn_a, in_wid, ker_wid, real_ib, real_ob, N, norm=1, trans=False):
    """prep_Ker before EncodeCoeffs: (max_bat, N) float coefficient vectors, one per output slot"""
    max_bat = N // (in_wid * in_wid)
    k_sz = ker_wid * ker_wid
    ker_rs = reshape_ker(ker_in, k_sz, real_ob, trans) * np.asarray(bn_a, dtype=np.float64)[:, None]
    max_ker_rs = np.zeros((max_bat, max_bat * k_sz))
    for i in range(real_ob):
        for j in range(real_ib):
            max_ker_rs[norm * i, norm * j * k_sz:norm * j * k_sz + k_sz] = ker_rs[i, j * k_sz:(j + 1) * k_sz]
    return np.stack([encode_ker_final(max_ker_rs, i, in_wid, max_bat, ker_wid) for i in range(max_bat)])


def negacyclic_mul(a, b):
    """a * b mod X^N + 1 on integer-valued int64 vectors"""
    N = len(a)
    full = np.convolve(a, b)
    out = full[:N].copy()
    out[:len(full) - N] -= full[N:]
    return out


def automorphism(a, g):
    """X -> X^g mod X^N + 1"""
    N = len(a)
    m = (np.arange(N) * g) % (2 * N)
    out = np.zeros_like(a)
    sign = np.where(m >= N, -1, 1)
    out[m % N] = sign * a
    return out


def pack_ctxts(ctxts, max_cnum):
    """conv.go:266-300 with norm = 1 on plain polynomials (the Scale bookkeeping aside: the result is max_cnum times the collected coefficients)"""
    N = len(ctxts[0])
    logN = N.bit_length() - 1
    cts = [c.copy() for c in ctxts]
    step = max_cnum // 2
    logStep = step.bit_length() - 1 if step > 0 else 0
    j = logN - logStep
    while step >= 1:
        for i in range(step):
            mono = np.zeros(N, dtype=cts[0].dtype)
            mono[1 << logStep] = 1
            tmp1 = negacyclic_mul(cts[i + step], mono)
            tmp2 = cts[i] - tmp1
            tmp1 = cts[i] + tmp1
            cts[i] = tmp1 + automorphism(tmp2, (1 << j) + 1)
        step //= 2
        logStep -= 1
        j += 1
    return cts[0]


def post_process(cfs, raw_in_wid, in_wid):
    batch = len(cfs) // (in_wid * in_wid)
    return np.asarray(cfs).reshape(in_wid, in_wid, batch)[:raw_in_wid, :raw_in_wid, :]


def conv_plain(x, ker_in, bn_a, in_wid, ker_wid, real_ib, real_ob, N, trans):
    """evalConv_BN without the bias (eval.go:224-258) in the clear on integer data: prep_Input, prep_Ker, one negacyclic product per
    output slot, the packing tree. Returns the result on the kp_wid x kp_wid grid (set_Variables), (kp_wid, kp_wid, real_ob)."""
    raw = x.shape[0]
    max_bat = N // (in_wid * in_wid)
    inp = np.rint(prep_input(x, raw, in_wid, N, 1, trans)).astype(np.int64)
    kc = np.rint(prep_ker_coeffs(ker_in, bn_a, in_wid, ker_wid, real_ib, real_ob, N, 1, trans)).astype(np.int64)
    packed = pack_ctxts([negacyclic_mul(inp, kc[i]) for i in range(max_bat)], max_bat)
    assert not np.any(packed % max_bat)
    kp_wid = 2 * raw if trans else raw
    return post_process(packed // max_bat, kp_wid, in_wid)[:, :, :real_ob]


def case_prep_ker_trans(ctx, O, k, i_batch):
    """hc_prep_ker_ex(trans = 1) == EncodeCoeffs + ToNTT of the restatement, both limbs, every slot; trans = 0 == hc_prep_ker"""
    import ctypes as C
    import golden.gen_conv_csv as gen_conv
    import golden.gen_transconv_csv as gen
    B, W, raw, x, ker, bna, bnb = gen.make_case(k, i_batch, 0)
    ob = B // 4
    h = ctx.prep_ker(ker.reshape(-1), bna, W, k, B, ob, trans=True)
    got = ctx.ker_download(h, B)
    ctx.ker_free(h)
    kc = prep_ker_coeffs(ker.reshape(-1), bna, W, k, B, ob, O.N, trans=True)
    for i in range(B):
        enc = O.encode_coeffs(kc[i], 2.0 ** 30, [0, 1])
        for l in range(2):
            assert np.array_equal(got[i, l], O.ntt(l, enc[l])), f"trans prep_ker k={k} B={B} slot {i} limb {l}"
    assert not got[ob:].any()                                # slots past real_ob hold zero plaintexts
    cB, cW, _, _, cker, cbna, _ = gen_conv.make_case(k, i_batch, 0)
    h0 = ctx.prep_ker(cker.reshape(-1), cbna, cW, k, cB, cB)
    L = ctx.L
    f64p = C.POINTER(C.c_double)
    flat = np.ascontiguousarray(cker.reshape(-1))
    h1 = C.c_void_p()
    assert L.hc_prep_ker_ex(ctx.h, flat.ctypes.data_as(f64p), flat.size, np.ascontiguousarray(cbna).ctypes.data_as(f64p), cW, k, cB, cB, 1,
                            2.0 ** 30, 0, C.byref(h1)) == 0
    assert np.array_equal(ctx.ker_download(h0, cB), ctx.ker_download(h1, cB)), "hc_prep_ker_ex(trans = 0) != hc_prep_ker"
    ctx.ker_free(h0)
    ctx.ker_free(h1)


def case_conv_trans(ctx, O, k, i_batch, n, seed=0x7C0E):
    """conv_then_pack (n = 1) or conv_then_pack_batch (n > 1, one kernel handle and one bias for every image, as evalConv_BN_batch
    passes them) on hc_prep_ker_ex(trans = 1) plaintexts == the oracle's conv_then_pack on the downloaded plaintexts, word for word"""
    import golden.gen_transconv_csv as gen
    import parity_cases as pc
    from oracle_lib import Q0, splitmix_rows
    B, W, raw, x, ker, bna, bnb = gen.make_case(k, i_batch, 0)
    h = ctx.prep_ker(ker.reshape(-1), bna, W, k, B, B // 4, trans=True)
    pl = ctx.ker_download(h, B)
    evk_all = pc.load_tree_keys(ctx, seed, B, 1)
    ctx.idx_load(None)
    ins = [pc.planted_conv_inputs(seed + 17 * z, B)[0] for z in range(n)]
    bias = splitmix_rows(seed + 5, Q0, O.N)
    bin_ = [ctx.buf(c) for c in ins]
    bb = ctx.buf(bias)
    bout = [ctx.buf(nwords=2 * O.N) for _ in range(n)]
    if n == 1:
        sc = ctx.conv_then_pack_dev(bin_[0], 2.0 ** 30, h, 2.0 ** 30, B, 1, 2.0 ** 30, bb, bout[0])
    else:
        sc = ctx.conv_then_pack_batch_dev(bin_, 2.0 ** 30, [h] * n, 2.0 ** 30, B, 1, 2.0 ** 30, [bb] * n, bout)
    assert sc == 2.0 ** 30
    idx = O.idx_plaintexts()
    for z in range(n):
        want, _ = O.conv_then_pack(ins[z], 2.0 ** 30, pl, 2.0 ** 30, idx, evk_all, B, 1, 2.0 ** 30, bias)
        assert np.array_equal(bout[z].download((2, O.N)), want), f"trans conv_then_pack k={k} B={B}, image {z} of {n}"
    for b in bin_ + bout + [bb]:
        b.free()
    ctx.ker_free(h)
