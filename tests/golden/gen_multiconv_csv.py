#!/usr/bin/env python3
"""Synthetic test_conv_data/*.csv generator for `conv multiconv`: a convolution whose m*B input channels fill m input ciphertexts.

  test_multiconv{k}_batch_{B}_in{m}_{in|ker|bna|bnb|out}_{iter}.csv, whitespace separated floats
Layouts: input HWC flat  in[(i*raw+j)*(m*B) + c]        (ciphertext j holds the channels j*B .. (j+1)*B - 1)
         kernel HWIO flat ker[o + c*B + t*B*(m*B)]       (c over the m*B input channels, o over the B output channels)
Expected output = gen_conv_csv.plain_conv on the m*B-channel input: zero-padded 'same' correlation, times bn_a plus bn_b.
Seeds: numpy default_rng(100000*m + 1000*k + 10*i_batch + iter).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_conv_csv import BATCHS, WIDTHS, plain_conv  # noqa: E402


def make_case(k, i_batch, it, m):
    B, W = BATCHS[i_batch], WIDTHS[i_batch]
    raw = W - k // 2
    rng = np.random.default_rng(100000 * m + 1000 * k + 10 * i_batch + it)
    x = rng.uniform(-1, 1, size=(raw, raw, m * B))
    ker = rng.uniform(-1, 1, size=(k, k, m * B, B)) / np.sqrt(k * k * m * B)
    a = rng.uniform(0.5, 1.5, size=B)
    b = rng.uniform(-0.5, 0.5, size=B)
    return B, W, raw, x, ker, a, b


def write_case(outdir, k, i_batch, it, m):
    B, W, raw, x, ker, a, b = make_case(k, i_batch, it, m)
    out = plain_conv(x, ker, a, b)
    os.makedirs(outdir, exist_ok=True)
    pre = os.path.join(outdir, f"test_multiconv{k}_batch_{B}_in{m}_")
    for name, arr in (("in", x), ("ker", ker), ("bna", a), ("bnb", b), ("out", out)):
        np.savetxt(f"{pre}{name}_{it}.csv", arr.reshape(-1), fmt="%.17g")
    return B, W, raw


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("k", type=int)
    ap.add_argument("i_batch", type=int)
    ap.add_argument("n", type=int)
    ap.add_argument("m", type=int)
    args = ap.parse_args()
    for it in range(args.n):
        print(write_case(args.outdir, args.k, args.i_batch, it, args.m))
