#!/usr/bin/env python3
"""Synthetic test_conv_data/*.csv generator for the `transconv` command (stride-2 transposed convolution; the reference has the
operators but no command or data for them).

File names and sizes follow testTransConv_in (optimal_conv_amd/host/hconv_host.cpp), shaped like test.go:37-40:
  test_transconv{k}_batch_{B}_{in|ker|bna|bnb|out}_{iter}.csv, whitespace separated floats.
Shapes: raw = W/2 - k/2 input width, B input channels, B/4 output channels, 2*raw output width.
Layouts: input HWC flat   in[(i*raw+j)*B+c]                   (main.go:1011-1021 prep_Input, trans = true)
         kernel HWOI flat ker[c + o*B + t*(B/4)*B]             (conv.go:192 reshape_ker, trans = true; TF's conv2d_transpose filter)
         output HWO flat  out[(i*2raw+j)*(B/4)+o]
Expected output = conv_transpose2d(x, w, stride=2, padding=(k-3)//2) cropped to 2raw x 2raw (TF's conv2d_transpose(strides=2,
padding='SAME')), times bn_a plus bn_b.
Seeds: numpy default_rng(5000 + 1000*k + 10*i_batch + iter).
"""
import argparse
import os

import numpy as np

BATCHS = [4, 16, 64, 256, 1024]   # main.go:578
WIDTHS = [128, 64, 32, 16, 8]     # main.go:579


def make_case(k, i_batch, it):
    B, W = BATCHS[i_batch], WIDTHS[i_batch]
    raw = W // 2 - k // 2
    ob = B // 4
    rng = np.random.default_rng(5000 + 1000 * k + 10 * i_batch + it)
    x = rng.uniform(-1, 1, size=(raw, raw, B))
    ker = rng.uniform(-1, 1, size=(k, k, ob, B)) / np.sqrt(k * k * B)
    a = rng.uniform(0.5, 1.5, size=ob)
    b = rng.uniform(-0.5, 0.5, size=ob)
    return B, W, raw, x, ker, a, b


def plain_transconv(x, ker, a, b):
    """stride-2 transposed convolution, HWC x HWOI -> (2raw)(2raw)O, then *a + b."""
    import torch
    import torch.nn.functional as F
    raw, _, B = x.shape
    k, ob = ker.shape[0], ker.shape[2]
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))[None]           # (1, B, raw, raw)
    w = torch.from_numpy(np.ascontiguousarray(ker)).permute(3, 2, 0, 1)              # (in, out, kh, kw)
    y = F.conv_transpose2d(xt, w, stride=2, padding=(k - 3) // 2)[0, :, :2 * raw, :2 * raw]
    return y.permute(1, 2, 0).numpy() * a + b


def write_case(outdir, k, i_batch, it):
    B, W, raw, x, ker, a, b = make_case(k, i_batch, it)
    out = plain_transconv(x, ker, a, b)
    os.makedirs(outdir, exist_ok=True)
    pre = os.path.join(outdir, f"test_transconv{k}_batch_{B}_")
    for name, arr in (("in", x), ("ker", ker), ("bna", a), ("bnb", b), ("out", out)):
        np.savetxt(f"{pre}{name}_{it}.csv", arr.reshape(-1), fmt="%.17g")
    return B, W, raw


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("k", type=int)
    ap.add_argument("i_batch", type=int)
    ap.add_argument("n", type=int)
    args = ap.parse_args()
    os.makedirs(args.outdir, exist_ok=True)
    for it in range(args.n):
        print(write_case(args.outdir, args.k, args.i_batch, it))
