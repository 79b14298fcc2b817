"""The packed layout of `resnet_packed` (DESIGN.md "The packed layout") on resnet_fast_ref's grid model. TEST INFRASTRUCTURE.

Block b = 0, 1, 2 of the full-slot network has channel spacing norm = 4, 2, 1 and lattice step s = 1, 2, 4. An image slot of block b is (g, py, px), g < norm,
py, px < s: channel c at channel slot norm*c + g, activation cell (i, j) at grid cell (py + s*i, px + s*j); norm * s^2 = 4, 8, 16 images per ciphertext.
slot_of is the assignment the host states in hconv_host.hpp (packed_slot); everything else here is derived from the layout, not from the host's code."""
import numpy as np

import resnet_fast_ref as F

W, SLOTS, GROUP = 32, 64, 16
NORM, STEPS = F.NORM, F.STEPS
CAP = [n * s * s for n, s in zip(NORM, STEPS)]


def slot_of(blk, m):
    """image m (0..15) of a group in block blk: (ciphertext, g, py, px)"""
    if blk == 0:
        return m // 4, m % 4, 0, 0
    if blk == 1:
        return m // 8, m % 2, (m // 4) % 2, (m // 2) % 2
    return 0, 0, (m // 4) % 2 + 2 * (m // 8), (m // 2) % 2 + 2 * (m % 2)


def n_cts(blk, n_images):
    """ciphertexts of block blk that a group of n_images fills (whole empty ones are not made)"""
    return max(slot_of(blk, m)[0] for m in range(n_images)) + 1


def place(acts, blk):
    """acts: per image an (r, r, C) activation of block blk -> the group's ciphertexts, (32, 32, 64) each"""
    cts = [np.zeros((W, W, SLOTS)) for _ in range(n_cts(blk, len(acts)))]
    n, s = NORM[blk], STEPS[blk]
    for m, a in enumerate(acts):
        q, g, py, px = slot_of(blk, m)
        r, C = a.shape[0], a.shape[2]
        cts[q][py:py + s * r:s, px:px + s * r:s, g:g + n * C:n] = a
    return cts


def unplace(ct, blk, m, r, C):
    """image m's (r, r, C) activation out of its block-blk ciphertext"""
    _, g, py, px = slot_of(blk, m)
    n, s = NORM[blk], STEPS[blk]
    return ct[py:py + s * r:s, px:px + s * r:s, g:g + n * C:n]


def expand_ker(ker, norm_in, norm_out, g_lo, g_cnt):
    """ker (k, k, cin, cout) -> (k, k, 64, 64): for g in g_lo .. g_lo + g_cnt - 1, input slot norm_in*c + g feeds output slot norm_out*o + g % norm_out only"""
    k, _, cin, cout = ker.shape
    out = np.zeros((k, k, SLOTS, SLOTS))
    for g in range(g_lo, g_lo + g_cnt):
        out[:, :, g:g + norm_in * cin:norm_in, g % norm_out:g % norm_out + norm_out * cout:norm_out] = ker
    return out


def keep_cells(k, blk, stride_in=False):
    """(32, 32) bool: the cells the mask of block blk's layers keeps (every phase), or of the stride layer entering it (the phases py, px < s/2)"""
    s, r = STEPS[blk], F.RAW(k)[blk]
    x = np.arange(W)
    live = ((x % s) < (s // 2 if stride_in else s)) & ((x // s) < r)
    return live[:, None] & live[None, :]


def keep_vec(cells, ul, logN=16):
    """a (32, 32) cell mask as the host's keep vector of half ul: index rev(coefficient within the half), every channel slot of a kept cell"""
    half = np.repeat(cells[ul * W // 2:(ul + 1) * W // 2].reshape(-1), SLOTS)
    idx = np.zeros(1 << (logN - 1), dtype=np.int64)
    idx[F.rev_bits(np.nonzero(half)[0], logN - 1)] = 1
    return idx


def conv_bn_relu_mask(x, ker64, a64, b64, dilation, cells):
    y = F.grid_conv(x, F.expand_ker(ker64 * a64, dilation), 1) + b64
    y = np.maximum(y, 0)
    y[~cells] = 0
    return y


def inside_layer(cts, k, blk, w, a, b):
    n = NORM[blk]
    ker = expand_ker(w, n, n, 0, n)
    return [conv_bn_relu_mask(x, ker, np.repeat(a, n), np.repeat(b, n), STEPS[blk], keep_cells(k, blk)) for x in cts]


def shift_cells(x, dy, dx):
    """X^((32 dy + dx) * 64) on the grid: every cell moves up by whole cells, negacyclic past the end"""
    flat = x.reshape(W * W, SLOTS)
    d = W * dy + dx
    out = np.roll(flat, d, axis=0)
    out[:d] *= -1
    return out.reshape(W, W, SLOTS)


def stride_layer(cts, k, blk, w, a, b):
    """the stride layer entering block blk: result r = 2q + h is ciphertext q under the kernel of half h of its channel offsets and the mask of the phases
    its images reach by themselves; results 4o .. 4o + 3 are added into output o, result 4o + t moved by (s/2) * (t // 2, t % 2) cells. Returns (outputs, tails)"""
    n, s = NORM[blk], STEPS[blk]
    res = []
    for x in cts:
        for h in range(2):
            ker = expand_ker(w, 2 * n, n, h * n, n)
            res.append(conv_bn_relu_mask(x, ker, np.repeat(a, n), np.repeat(b, n), s // 2, keep_cells(k, blk, True)))
    outs = []
    for r, y in enumerate(res):
        t = r % 4
        if t == 0:
            outs.append(y.copy())
        else:
            outs[-1] += shift_cells(y, (s // 2) * (t // 2), (s // 2) * (t % 2))
    return outs, len(res)


def fc(ct, k, fc_w, fc_b, n_images):
    """reduce-mean + FC: raw_2 x raw_2 taps of fc_w / raw_2^2 dilated by 4; image m's scores at cell (kd//2 + py, kd//2 + px)"""
    r = F.RAW(k)[2]
    ker = F.expand_ker(np.broadcast_to(fc_w, (r, r) + fc_w.shape) / float(r * r), STEPS[2])
    y = F.grid_conv(ct, ker, 1)
    kd = ker.shape[0]
    out = []
    for m in range(n_images):
        _, _, py, px = slot_of(2, m)
        out.append(y[kd // 2 + py, kd // 2 + px, :fc_w.shape[1]] + fc_b)
    return out


def network(layers, fc_w, fc_b, images):
    """layers: (strided, block of the output, ker, bn_a, bn_b) in driver order; images: up to 16 (r0, r0, 3). Returns (per layer: the ciphertexts handed on, block),
    the images' scores and the number of bootstrapping tails"""
    k = layers[0][2].shape[0]
    cts = place(images, 0)
    handed, tails = [], 0
    for strided, blk, w, a, b in layers:
        if strided:
            cts, t = stride_layer(cts, k, blk, w, a, b)
        else:
            cts, t = inside_layer(cts, k, blk, w, a, b), len(cts)
        tails += t
        handed.append((cts, blk))
    assert len(cts) == 1
    return handed, fc(cts[0], k, fc_w, fc_b, len(images)), tails
