#!/usr/bin/env python3
"""Images for the `resnet_packed` activation checks: gen_resnet_csv.write_case's network, weights and file layout, the images drawn with amplitude AMPLITUDE.

Why not write_case's own images. tests/test_gpu_resnet_packed.py tells an image's dumped activation from every other image's by d_own < d_other / 4, where d_own is the
chain's error and d_other the distance between two images' plain activations. The chain's ReLU is a polynomial on the range 2^pow = 64 of the pre-activations; near zero it
is off by up to about 0.05 in absolute terms, whatever the input (the sparse and the full-slot drivers alike, one image per ciphertext). write_case's weights shrink the
activations by about 0.6 per layer, and the differences between two images faster: with uniform(-1, 1) images the plain activations alone give
    layer 3: mean 0.074, smallest d_other 0.046;  layer 5: 0.045, 0.015;  layer 6: 0.033, 0.0072
so d_other is at or below the ReLU's absolute error before anything is encrypted. The network is positively homogeneous but for the BN shifts (|b| <= 0.1), so a larger
image moves activations and their differences up and leaves the ReLU's absolute error where it is. AMPLITUDE is the largest power of two that keeps every pre-activation of
every layer, the stride layers' dropped cells included, inside the range: at 16 the largest |pre-activation| of the 16 images is 45.4 (at 32 it is 90.7 > 64). That gives
    layer 3: mean 0.97, smallest d_other 0.72;  layer 5: 0.48, 0.25;  layer 6: 0.22, 0.125
(main() prints these). The seeds are write_case's, default_rng(1000 + i)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gen_resnet_csv as rgen  # noqa: E402
import oracle_resnet as rn  # noqa: E402

AMPLITUDE = 16.0
RANGE = 64.0  # 2^pow, pow = 6: what the drivers scale a pre-activation by before the sine and the ReLU


def images(n, raw0, amplitude=AMPLITUDE):
    return [np.random.default_rng(1000 + i).uniform(-amplitude, amplitude, (raw0, raw0, 3)) for i in range(n)]


def plain(net, image):
    """the plain model on one image: (activation per layer, scores, largest |pre-activation| at any cell the encrypted convolution computes)"""
    x, acts, pre = image, [], 0.0
    for kind, blk, w, a, b in net.layers:
        y = rn.plain_conv_same(x, w) * a + b
        pre = max(pre, float(np.abs(y).max()))  # a stride layer is computed at every cell of its input lattice
        if kind == "StrConv_sparse":
            r = net.raw[blk + 1]
            y = y[0:2 * r:2, 0:2 * r:2]
        x = np.maximum(y, 0)
        acts.append(x)
    return acts, x.mean(axis=(0, 1)) @ net.fc_w + net.fc_b, pre


def write_case(root, ker_wid=3, depth=8, n_images=16, amplitude=AMPLITUDE):
    """gen_resnet_csv.write_case's tree with test_image_{i}.csv and expected_scores_{i}.csv replaced. Returns per image (activations, scores, largest |pre-activation|)"""
    rgen.write_case(root, ker_wid, depth, n_images)
    net = rn.Net(16, ker_wid=ker_wid, depth=depth, seed=0)
    pdir = os.path.join(root, "Resnet_plain_data", f"crop_ker{ker_wid}_d{depth}_wid1")
    W, raw = net.in_wids[0], net.raw[0]
    out = []
    for it, im in enumerate(images(n_images, raw, amplitude)):
        full = np.zeros((W, W, 3))
        full[:raw, :raw] = im
        np.savetxt(os.path.join(pdir, f"test_image_{it}.csv"), full.reshape(-1), fmt="%.17g")
        out.append(plain(net, im))
        np.savetxt(os.path.join(pdir, f"expected_scores_{it}.csv"), out[-1][1], fmt="%.17g")
    return out


def d_other(acts, layer):
    """per image the smallest mean |difference| of its plain activation at `layer` to another image's"""
    ref = np.stack([a[layer].reshape(-1) for a in acts])
    return [float(np.delete(np.abs(ref - ref[i]).mean(axis=1), i).min()) for i in range(len(acts))], float(ref.mean())


def main():
    net = rn.Net(16, ker_wid=3, depth=8, seed=0)
    for amp in (1.0, AMPLITUDE, 2 * AMPLITUDE):
        res = [plain(net, im) for im in images(16, net.raw[0], amp)]
        print(f"amplitude {amp}: largest |pre-activation| {max(r[2] for r in res):.2f} (range {RANGE})")
        for layer in (3, 5, 6):
            d, mean = d_other([r[0] for r in res], layer)
            print(f"  layer {layer}: mean activation {mean:.4f}, smallest d_other {min(d):.4f}")


if __name__ == "__main__":
    main()
