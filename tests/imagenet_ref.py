"""The full-packing stride layer (kind "StrConv") and the ImageNet tail (`imagenet`) as plain numpy float64 models, and the case that holds hc_prep_ker_fc to
hc_prep_ker_ex2 on the host-replicated kernel.

THE LAYOUT of the stride layer (its specification; DESIGN.md "Full-packing stride layer"). A ciphertext on the in_wid grid holds coefficient (y, x, c) at index
(y*in_wid + x)*B + c, B = N / in_wid^2 channel slots. The layer keeps (y, x, c) for odd y, x < kp_wid and puts it at (y // 2, x // 2, c + B*pos) of the in_wid/2 grid,
which has 4 B channel slots; every other coefficient of the result is zero."""
import numpy as np

N = 1 << 16


def plain_conv_same(x, ker):
    """'same' zero-padded correlation, HWC x HWIO -> HWO"""
    r, k = x.shape[0], ker.shape[0]
    p = k // 2
    xp = np.zeros((r + 2 * p, r + 2 * p, x.shape[2]))
    xp[p:p + r, p:p + r, :] = x
    out = np.zeros((r, r, ker.shape[3]))
    for di in range(k):
        for dj in range(k):
            out += xp[di:di + r, dj:dj + r, :] @ ker[di, dj]
    return out


def stride_layout(cf, in_wid, kp_wid, pos):
    """the N coefficients of a result on the in_wid grid -> the N coefficients the stride layer leaves, by the layout above"""
    B = N // (in_wid * in_wid)
    g = np.asarray(cf).reshape(in_wid, in_wid, B)
    out = np.zeros((in_wid // 2, in_wid // 2, 4 * B), dtype=g.dtype)
    odd = np.arange(1, kp_wid, 2)
    out[np.ix_(odd // 2, odd // 2, np.arange(B) + B * pos)] = g[np.ix_(odd, odd, np.arange(B))]
    return out.reshape(-1)


def strconv_layer(x, ker, a, b, in_wid, pos):
    """conv 'same' on the kept region (x is kp_wid x kp_wid x cin), * a + b, ReLU, the layout: the N coefficients of the layer's result"""
    kp, B = x.shape[0], N // (in_wid * in_wid)
    y = np.maximum(plain_conv_same(x, ker) * a + b, 0.0)
    grid = np.zeros((in_wid, in_wid, B))
    grid[:kp, :kp, :y.shape[2]] = y
    return stride_layout(grid.reshape(-1), in_wid, kp, pos)


def strided(y, kp_wid):
    """the odd positions below kp_wid of an activation: what the layout keeps, compact"""
    return y[1:kp_wid:2, 1:kp_wid:2, :]


# ---- the network of `imagenet` (test.go:1209-1400): layers is [(ker HWIO, a, b)] * 7 (three of block 1, the stride layer, three of block 2), fc (2 c1, 1000)
KP = {3: (14, 7), 5: (14, 6)}          # kp_wids (test.go:1221-1234); the stride layer keeps 2 * KP[k][1] on the 16-grid
POWS = (6, 6, 5, 5, 5, 5, 6)           # init_pow, mid_pow from the last block-1 layer on, final_pow for the last layer


def network(layers, fc, image, k):
    """-> (scores[1000], the largest |pre-activation| of each layer)"""
    x, peak = image, []
    for li, (w, a, b) in enumerate(layers):
        y = plain_conv_same(x, w) * a + b
        if li == 3:
            y = strided(y, 2 * KP[k][1])
        peak.append(float(np.abs(y).max()))
        x = np.maximum(y, 0.0)
    r = KP[k][1]
    assert x.shape[0] == r
    return x.sum(axis=(0, 1)) / (r * r) @ fc, peak          # the 7 x 7 window at cell (3, 3) of the 8-grid covers the kept r x r cells


# ---- hc_prep_ker_fc == hc_prep_ker_ex2 on the replicated kernel
PREP_FC_SHAPES = [(128, 3, 4, 4, 1, 1), (64, 7, 3, 10, 1, 1), (32, 5, 16, 10, 4, 4), (32, 1, 5, 7, 1, 1)]      # (in_wid, k, real_ib, real_ob, norm, dilation)
PREP_FC_DEVICE_SHAPE = (8, 7, 40, 37, 1, 1)


def case_prep_ker_fc(ctx, in_wid, k, real_ib, real_ob, norm, dilation, seed=0):
    """every word of every row, through hc_ker_download"""
    rng = np.random.default_rng(seed + 1000 * in_wid + k)
    fc = rng.uniform(-1, 1, size=(real_ib, real_ob)) / np.sqrt(k * k * real_ib)
    bna = rng.uniform(0.5, 1.5, size=real_ob)
    max_bat = ctx.N // (in_wid * in_wid)
    h_fc = ctx.prep_ker_fc(fc, bna, in_wid, k, real_ib, real_ob, norm, dilation=dilation)
    got = ctx.ker_download(h_fc, max_bat)
    ctx.ker_free(h_fc)
    rep = np.ascontiguousarray(np.broadcast_to(fc, (k * k, real_ib, real_ob)))
    import ctypes as C
    f64p, h_ex, flat = C.POINTER(C.c_double), C.c_void_p(), rep.reshape(-1)
    ctx._ck(ctx.L.hc_prep_ker_ex2(ctx.h, flat.ctypes.data_as(f64p), flat.size, bna.ctypes.data_as(f64p), in_wid, k, real_ib, real_ob, norm, 2.0 ** 30, 0, dilation, 1, C.byref(h_ex)))
    want = ctx.ker_download(h_ex, max_bat)
    ctx.ker_free(h_ex)
    assert want.any(), "an all-zero handle would compare equal to anything empty"
    assert np.array_equal(got, want), f"hc_prep_ker_fc differs from hc_prep_ker_ex2 on the replicated kernel at {(in_wid, k, real_ib, real_ob, norm, dilation)}"
