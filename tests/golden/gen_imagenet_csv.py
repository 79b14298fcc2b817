#!/usr/bin/env python3
"""Synthetic weights and images for the `imagenet` command (test.go:1209-1400; the reference ships neither), in its file layout:
  weight_imgnet_ker{k}_h5/w{10+L}-conv.csv, w{11+L}-a.csv, w{11+L}-b.csv for layer L = 0..6 (a layer's BN files carry the NEXT number: test.go:1293-1296), fc.csv
  ker{k}_data/test_image_{i}.csv                                     (14, 14, c1) flat
  ker{k}_plain_result/plain_result_{i}.csv                           the plain float64 model's 1000 scores (tests/imagenet_ref.py network; not a reference file)
Layers 0-2: c1 -> c1 on 14 x 14; layer 3: c1 -> 2 c1, stride 2; layers 4-6: 2 c1 -> 2 c1; fc (2 c1, 1000). Kernels HWIO flat, uniform(-1, 1) / sqrt(k^2 cin).

Range. The chain's ReLU polynomial is valid for |pre-activation| < 2^pow of the layer (pow 6, 6, 5, 5, 5, 5, 6) and loses relative precision towards zero, so each layer's
bn_a is rescaled by one factor per layer that puts the largest |pre-activation| over the generated images at 0.75 * 2^pow (bn_b, uniform(-0.5, 0.5), stays). make()
asserts the bound on the model's own peaks after the rescaling."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import imagenet_ref as R  # noqa: E402

HEADROOM = 0.75


def make(k, n, c1, seed):
    """-> (layers [(ker, a, b)] * 7, fc, images, scores [n][1000], peaks [7])"""
    if k not in R.KP:
        raise ValueError("strange ker name!")
    rng = np.random.default_rng(seed)
    raw = R.KP[k][0]
    images = [rng.uniform(-1, 1, size=(raw, raw, c1)) for _ in range(n)]
    chans = [(c1, c1)] * 3 + [(c1, 2 * c1)] + [(2 * c1, 2 * c1)] * 3
    layers, xs = [], list(images)
    for li, (cin, cout) in enumerate(chans):
        w = rng.uniform(-1, 1, size=(k, k, cin, cout)) / np.sqrt(k * k * cin)
        a = rng.uniform(0.5, 1.5, size=cout)
        b = rng.uniform(-0.5, 0.5, size=cout)
        conv = [R.plain_conv_same(x, w) for x in xs]
        if li == 3:
            conv = [R.strided(c, 2 * R.KP[k][1]) for c in conv]
        limit = HEADROOM * 2.0 ** R.POWS[li]
        a = a * ((limit - 0.5) / max(np.abs(c * a).max() for c in conv))       # |a conv + b| <= |a conv| + 0.5
        xs = [np.maximum(c * a + b, 0.0) for c in conv]
        layers.append((w, a, b))
    fc = rng.uniform(-1, 1, size=(2 * c1, 1000)) / np.sqrt(2 * c1)
    res = [R.network(layers, fc, im, k) for im in images]
    peaks = [max(r[1][li] for r in res) for li in range(7)]
    for li, p in enumerate(peaks):
        assert p <= HEADROOM * 2.0 ** R.POWS[li], f"layer {li}: |pre-activation| {p} leaves 0.75 * 2^{R.POWS[li]}"
    return layers, fc, images, [r[0] for r in res], peaks


def write(outdir, k, n, c1, seed):
    layers, fc, images, scores, peaks = make(k, n, c1, seed)
    wdir, idir, pdir = (os.path.join(outdir, d) for d in (f"weight_imgnet_ker{k}_h5", f"ker{k}_data", f"ker{k}_plain_result"))
    for d in (wdir, idir, pdir):
        os.makedirs(d, exist_ok=True)

    def save(path, arr):
        np.savetxt(path, np.asarray(arr).reshape(-1), fmt="%.17g")
    for li, (w, a, b) in enumerate(layers):
        save(os.path.join(wdir, f"w{10 + li}-conv.csv"), w)
        save(os.path.join(wdir, f"w{11 + li}-a.csv"), a)
        save(os.path.join(wdir, f"w{11 + li}-b.csv"), b)
    save(os.path.join(wdir, "fc.csv"), fc)
    for i, (im, sc) in enumerate(zip(images, scores)):
        save(os.path.join(idir, f"test_image_{i}.csv"), im)
        save(os.path.join(pdir, f"plain_result_{i}.csv"), sc)
    return scores, peaks


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "imagenet_model_scores.json")      # the model's scores for FIXTURE_CASE, pinned
FIXTURE_CASE = dict(k=3, n=2, c1=16, seed=7)


def write_fixture():
    import json
    _, _, _, scores, peaks = make(**FIXTURE_CASE)
    with open(FIXTURE, "w") as f:
        json.dump(dict(FIXTURE_CASE, peaks=peaks, scores=[[float(v) for v in s] for s in scores]), f)
        f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("k", type=int)
    ap.add_argument("n", type=int)
    ap.add_argument("c1", type=int, nargs="?", default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fixture", action="store_true", help="rewrite tests/golden/imagenet_model_scores.json as well")
    args = ap.parse_args()
    if args.fixture:
        write_fixture()
    _, pk = write(args.outdir, args.k, args.n, args.c1, args.seed)
    print("largest |pre-activation| per layer:", " ".join(f"{p:.3f}" for p in pk))
