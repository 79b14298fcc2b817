#!/usr/bin/env python3
"""Synthetic test_conv_data/*.csv generator for the `strconvReLU` command (the full-packing stride layer, kind "StrConv"): gen_conv_csv's case
(same seeds, same distributions, same layouts) on the raw width kp_wid = 2 (W/2 - k//2) the layer keeps, and
  test_strconv{k}_batch_{B}_reluout_{iter}.csv = max(out, 0)[1:kp_wid:2, 1:kp_wid:2, :],
the ReLU of the stride-2 outputs (odd row and column), (kp_wid/2, kp_wid/2, B) flat: what the command compares the kept cells of its result against.

Range: the chain runs at pow = 4 (test.go:22), as `convReLU` does on gen_conv_csv's case (k, i_batch, it). The draws are that case's with a smaller image, so an
output sums no more taps than there: the same range and the same share of small values, which is what lets a test hold the two commands' precision together.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_conv_csv import BATCHS, WIDTHS, plain_conv  # noqa: E402


def kp_wid(k, i_batch):
    return 2 * (WIDTHS[i_batch] // 2 - k // 2)


def make_case(k, i_batch, it):
    B, W = BATCHS[i_batch], WIDTHS[i_batch]
    if W % 4:
        raise ValueError("input wid not divisible by 4")
    raw = kp_wid(k, i_batch)
    rng = np.random.default_rng(1000 * k + 10 * i_batch + it)
    x = rng.uniform(-1, 1, size=(raw, raw, B))
    ker = rng.uniform(-1, 1, size=(k, k, B, B)) / np.sqrt(k * k * B)
    a = rng.uniform(0.5, 1.5, size=B)
    b = rng.uniform(-0.5, 0.5, size=B)
    return B, W, raw, x, ker, a, b


def write_case(outdir, k, i_batch, it):
    B, W, raw, x, ker, a, b = make_case(k, i_batch, it)
    out = plain_conv(x, ker, a, b)
    relu = np.maximum(out, 0.0)[1:raw:2, 1:raw:2, :]
    os.makedirs(outdir, exist_ok=True)
    pre = os.path.join(outdir, f"test_strconv{k}_batch_{B}_")
    for name, arr in (("in", x), ("ker", ker), ("bna", a), ("bnb", b), ("out", out), ("reluout", relu)):
        np.savetxt(f"{pre}{name}_{it}.csv", arr.reshape(-1), fmt="%.17g")
    return B, W, raw


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("k", type=int)
    ap.add_argument("i_batch", type=int)
    ap.add_argument("n", type=int)
    args = ap.parse_args()
    for it in range(args.n):
        print(write_case(args.outdir, args.k, args.i_batch, it))
