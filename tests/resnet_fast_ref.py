"""The reference's full-slot ResNet driver (testResNet_crop_fast_in, test.go:372-636) restated in numpy. TEST INFRASTRUCTURE.

  rot_util.go:226-267  gen_keep_vec_stride                         -> gen_keep_vec_stride
  eval.go:418-431      Conv_inside's dilated kernel (new_ker_in)   -> expand_ker (dilation)
  test.go:484-492      the stride layers' input channels at 2c     -> expand_ker (ib_stride)
  test.go:372-636      the network on the 32-wide grid             -> inside_network

The grid model: a packed ciphertext's coefficients are cells (row, col) of the in_wid x in_wid grid, row-major, each holding max_bat
channel slots (channel c of a layer at norm*c). A convolution with a kd x kd kernel adds, for every tap (ty, tx), the input moved by
(ty - kd//2)*in_wid + (tx - kd//2) cells, with the negacyclic sign flip where the move wraps past the ring's end (X^N + 1).
test_resnet_fast_cpu.py anchors this against the reference's own formulas (transconv_ref.conv_plain) on a small ring."""
import numpy as np


def rev_bits(x, nbits):
    r = np.zeros_like(x)
    for b in range(nbits):
        r |= ((x >> b) & 1) << (nbits - 1 - b)
    return r


def gen_keep_vec_stride(vec_size, in_wid, kp_wid, step, ul, raw_in_wid_odd):
    """rot_util.go:226-267, literally"""
    logN = (2 * vec_size - 1).bit_length()
    idx = np.zeros(vec_size, dtype=np.int64)
    batch = 2 * vec_size // (in_wid * in_wid)
    init = 0 if raw_in_wid_odd else step - 1
    if ul not in (0, 1):
        raise ValueError("ul not 0 nor 1")
    for i in range(kp_wid):
        row = init + i * step
        if (row < in_wid // 2) if ul == 0 else (row >= in_wid // 2):
            r = row - (in_wid // 2 if ul else 0)
            j, b = np.meshgrid(np.arange(kp_wid), np.arange(batch), indexing="ij")
            idx[rev_bits(in_wid * batch * r + batch * (j * step + init) + b, logN - 1).reshape(-1)] = 1
    return idx


def keep_cells(vec_size, in_wid, kp_wid, step, raw_in_wid_odd):
    """the (in_wid, in_wid) grid cells whose every slot both halves' masks keep (the slot index of coefficient v of half ul is rev(v))"""
    logN = (2 * vec_size - 1).bit_length()
    batch = 2 * vec_size // (in_wid * in_wid)
    keep = np.zeros((in_wid, in_wid, batch), dtype=np.int64)
    for ul in (0, 1):
        m = gen_keep_vec_stride(vec_size, in_wid, kp_wid, step, ul, raw_in_wid_odd)
        v = rev_bits(np.nonzero(m)[0], logN - 1)
        keep[v // (in_wid * batch) + ul * in_wid // 2, (v // batch) % in_wid, v % batch] = 1
    assert np.all(keep.min(axis=2) == keep.max(axis=2)), "a mask keeps whole cells"
    return keep[:, :, 0].astype(bool)


def expand_ker(ker, dilation=1, ib_stride=1):
    """ker (k, k, cin, cout) HWIO -> the kernel hc_prep_ker_ex2 encodes: width dilation*(k-1)+1, tap (d*ty, d*tx), input channel ib_stride*c"""
    k, _, cin, cout = ker.shape
    kd = dilation * (k - 1) + 1
    out = np.zeros((kd, kd, cin * ib_stride, cout))
    out[::dilation, ::dilation, ::ib_stride] = ker
    return out


def grid_conv(x, ker, norm):
    """x (W, W, max_bat) cells x slots, ker (kd, kd, cin, cout) HWIO whose input channel c reads slot norm*c; output channel o at slot norm*o"""
    W, _, mb = x.shape
    kd, _, cin, cout = ker.shape
    assert norm * cin <= mb and norm * cout <= mb
    flat = x.reshape(W * W, mb)[:, ::norm][:, :cin]
    out = np.zeros((W * W, mb))
    acc = np.zeros((W * W, cout))
    n = W * W
    p = np.arange(n)
    for ty in range(kd):
        for tx in range(kd):
            if not ker[ty, tx].any():
                continue
            src = p + (ty - kd // 2) * W + (tx - kd // 2)
            sign = np.where((src < 0) | (src >= n), -1.0, 1.0)
            acc += (sign[:, None] * flat[src % n]) @ ker[ty, tx]
    out[:, ::norm][:, :cout] = acc
    return out.reshape(W, W, mb)


RAW = lambda k: [32 - k // 2, 16 - k // 2, 8 - k // 2]        # raw_in_wids (test.go:414)
NORM, STEPS = [4, 2, 1], [1, 2, 4]                            # test.go:409-411


def init_of(k, blk):
    """the first kept position of block blk's outputs on the 32-wide grid (gen_keep_vec_stride: 0 for an odd keep width, else step - 1)"""
    r = RAW(k)[blk]
    return 0 if r % 2 else STEPS[blk] - 1


def place(act, k, blk, logN=16):
    """a block-blk activation (r, r, C) as the fast driver holds it: cell (init + i*step, init + j*step), channel c in slot norm*c"""
    W = 32
    x = np.zeros((W, W, (1 << logN) // (W * W)))
    s, i0, n = STEPS[blk], init_of(k, blk), NORM[blk]
    r = act.shape[0]
    x[i0:i0 + s * r:s, i0:i0 + s * r:s, 0:n * act.shape[2]:n] = act
    return x


def inside_layer(x, k, strided, blk, w, a, b, logN=16):
    """evalConv_BNRelu_new for kinds Conv_inside / StrConv_inside (eval.go:295-302, 418-431) on the grid model: dilated kernel (a stride
    layer's input channels at 2c), bias at every cell, ReLU on every slot, keep_ctxt with both halves of ext_idx[step]"""
    in_step = STEPS[blk] // 2 if strided else STEPS[blk]
    y = grid_conv(x, expand_ker(w, in_step, 2 if strided else 1) * a, NORM[blk])
    y[:, :, 0:NORM[blk] * len(b):NORM[blk]] += b
    y = np.maximum(y, 0)
    r = RAW(k)[blk]
    y[~keep_cells(1 << (logN - 1), 32, r, STEPS[blk], r % 2 == 1)] = 0
    return y


def inside_fc(x, k, fc_w, fc_b):
    """test.go:541-600: reduce-mean and FC as one ker_inf_wid-wide convolution at norm 1, read at (ker_inf_wid/2, ker_inf_wid/2) (prt_mat_one_norm)"""
    raw = RAW(k)
    kf = raw[0] + (raw[0] % 2 == 0)
    fc = np.broadcast_to(fc_w, (kf, kf) + fc_w.shape) / float(raw[2] * raw[2])
    return grid_conv(x, fc, 1)[kf // 2, kf // 2, :fc_w.shape[1]] + fc_b


def inside_network(layers, fc_w, fc_b, image):
    """testResNet_crop_fast_in on the grid model. layers: (strided, block of the output, ker (k,k,cin,cout), bn_a, bn_b) in driver order"""
    k = layers[0][2].shape[0]
    x = place(image, k, 0)
    acts = []
    for strided, blk, w, a, b in layers:
        x = inside_layer(x, k, strided, blk, w, a, b)
        acts.append(x)
    return acts, inside_fc(x, k, fc_w, fc_b)


def case_prep_ker_ex2(ctx, k, dilation, ib_stride, real_ib, real_ob, norm, in_wid=32, seed=0):
    """hc_prep_ker_ex2 on the undilated kernel == hc_prep_ker_ex (trans = 0) on the host-expanded one, every word of every slot"""
    rng = np.random.default_rng(seed + 1000 * k + 100 * dilation + 10 * ib_stride)
    ker = rng.uniform(-1, 1, (k, k, real_ib, real_ob))
    bna = rng.uniform(0.5, 1.5, real_ob)
    max_bat = ctx.N // (in_wid * in_wid)
    kexp = expand_ker(ker, dilation, ib_stride)
    h2 = ctx.prep_ker(ker.reshape(-1), bna, in_wid, k, real_ib, real_ob, norm, dilation=dilation, ib_stride=ib_stride)
    got = ctx.ker_download(h2, max_bat)
    ctx.ker_free(h2)
    h1 = ctx.prep_ker(kexp.reshape(-1), bna, in_wid, kexp.shape[0], real_ib * ib_stride, real_ob, norm)
    want = ctx.ker_download(h1, max_bat)
    ctx.ker_free(h1)
    assert got.any()
    assert np.array_equal(got, want), f"prep_ker_ex2 k={k} dilation={dilation} ib_stride={ib_stride} differs from the host-expanded kernel"


# (k, dilation, ib_stride, real_ib, real_ob, norm): every kernel testResNet_crop_fast_in prepares, at its shapes (ib_stride 2: the file's channel count)
DRIVER_SHAPES = [(3, 1, 1, 16, 16, 4), (3, 2, 1, 32, 32, 2), (3, 4, 1, 64, 64, 1), (3, 1, 2, 16, 32, 2), (3, 2, 2, 32, 64, 1), (5, 2, 2, 32, 64, 1)]


def case_fc_k31(ctx, O, seed=5):
    """the final FC of the fast driver for k = 3: a 31 x 31 kernel at in_wid 32, real_ib 64, real_ob 10, norm 1 (2*adj = 63 486 < N) == the
    restatement of prep_Ker (oracle prep_ker_coeffs, EncodeCoeffs, NTT) on every slot; and hc_prep_ker_ex2 at dilation 15 (3 -> 31 wide)
    == its host expansion"""
    rng = np.random.default_rng(seed)
    kf, rb, fc_out = 31, 64, 10
    fc_w = rng.uniform(-1, 1, (rb, fc_out))
    ker = np.ascontiguousarray(np.broadcast_to(fc_w, (kf, kf, rb, fc_out))).reshape(-1)
    bna = np.full(fc_out, 1.0 / 49.0)
    h = ctx.prep_ker(ker, bna, 32, kf, rb, fc_out, 1)
    got = ctx.ker_download(h, 64)
    ctx.ker_free(h)
    kc = O.prep_ker_coeffs(ker, bna, 32, kf, rb, fc_out, 1)
    for i in range(64):
        enc = O.encode_coeffs(kc[i], 2.0 ** 30, [0, 1])
        for l in range(2):
            assert np.array_equal(got[i, l], O.ntt(l, enc[l])), f"k=31 FC plaintext slot {i} limb {l}"
    assert not got[fc_out:].any()
    case_prep_ker_ex2(ctx, 3, 15, 1, 64, 10, 1)
