"""`resnet_packed` on the GPU, k = 3, depth 8 (the smallest network with every layer kind: three block-1 layers, both stride layers, a layer in each of blocks 2 and 3, the FC).

Class scores cannot show two images swapped between slots: with tests/golden/gen_resnet_csv.py's synthetic weights they barely depend on the image. So the command dumps
(HCONV_PACKED_DUMP_LAYERS, test mode) every image's unpacked activation after layer 3 (the first stride output, 8 images per ciphertext), 5 (the second, 16) and 6 (the last
activation), and for every image and layer
    d_own   = mean |dumped - the image's own plain activation|
    d_other = the smallest mean |dumped - another image's plain activation|
must satisfy d_own < d_other / 4.

The images are tests/golden/gen_resnet_packed_images.py's: write_case's seeds at amplitude 16. With write_case's own uniform(-1, 1) images the plain activations of two images
differ by 0.046 / 0.015 / 0.0072 at layers 3 / 5 / 6, which is at or below the absolute error (up to about 0.05) that the chain's polynomial ReLU on the range 64 has near
zero, one image per ciphertext or 16: d_other has no room over d_own before anything is packed (that generator's docstring has the figures and the choice of 16).

Measured on an MI355X, 16 images: d_own 0.018 / 0.024 / 0.034 against d_other 0.74 / 0.26 / 0.14 at layers 3 / 5 / 6, largest d_own / d_other 0.2461 (layer 6; 0.2415 for the
group of 5). The run is deterministic under HCONV_SEED (two runs' d_own agree to 3e-6), so the narrow room at layer 6 is the ReLU's error and the images, not noise.

Scores: max |delta| against the plain model < 0.08, test_resnet_fast_cli_depth8's bound (measured 0.0358 and 0.0355); no arg-max assertion."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden.gen_resnet_packed_images as pgen
import oracle_resnet as rn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")
DUMPED = (3, 5, 6)


@pytest.fixture(scope="module")
def plain():
    """the plain model's (activations, scores, largest |pre-activation|) of the 16 images, computed once"""
    net = rn.Net(16, ker_wid=3, depth=8, seed=0)
    return [pgen.plain(net, im) for im in pgen.images(16, net.raw[0])]


def run_packed(root, n, extra=None, dump=True):
    want = pgen.write_case(str(root), 3, 8, n)
    env = dict(os.environ, HCONV_SEED="11", **(extra or {}))
    if dump:
        env["HCONV_PACKED_DUMP_LAYERS"] = ",".join(str(l) for l in DUMPED)
    out = subprocess.run([CLI, "--test-mode", "resnet_packed", "3", "8", "1", str(n), "false"], cwd=root, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    for pat in (r"^Block1, Layer  3 done!$", r"^Block1 to 2 done!$", r"^Block2 to 3 done!$", r"^Block3 done\.$", r"^Final FC done\.$", rf"^Total done in \S+ \({min(n, 16)} images\)$"):
        assert re.search(pat, out.stdout, re.M), pat
    d = root / "Resnet_enc_results" / "results_crop_ker3_d8_wid1"
    scores = [np.loadtxt(d / f"class_result_ker3_{i}.csv") for i in range(n)]
    acts = {(l, i): np.loadtxt(d / f"packed_act_L{l}_{i}.csv") for l in DUMPED for i in range(n)} if dump else {}
    return scores, acts, [w[1] for w in want]


@pytest.fixture(scope="module")
def run16(tmp_path_factory):
    """`resnet_packed 3 8 1 16 false` at one ciphertext per launch set, layers 3, 5 and 6 dumped"""
    return run_packed(tmp_path_factory.mktemp("packed16"), 16)


@pytest.fixture(scope="module")
def run5(tmp_path_factory):
    """a partial group: two block-1 ciphertexts (4 + 1 images), one of block 2, one of block 3, the other image slots empty"""
    return run_packed(tmp_path_factory.mktemp("packed5"), 5)


def distances(plain, acts, n):
    """(layer, image, d_own, d_other) against ALL 16 plain images (a swap with any of them would show, also in a partial group)"""
    out = []
    for l in DUMPED:
        ref = np.stack([plain[i][0][l].reshape(-1) for i in range(16)])
        for i in range(n):
            d = np.abs(ref - acts[(l, i)]).mean(axis=1)
            out.append((l, i, d[i], np.delete(d, i).min()))
            print(f"layer {l} image {i}: d_own {d[i]:.6f} d_other {out[-1][3]:.6f} ratio {d[i] / out[-1][3]:.4f}")
    print(f"largest d_own / d_other {max(t[2] / t[3] for t in out):.4f}")
    return out


def check_scores(plain, scores, want, n):
    delta = [np.max(np.abs(scores[i] - want[i])) for i in range(n)]
    print(f"largest |delta| of a score {max(delta):.5f}")
    for i in range(n):
        np.testing.assert_allclose(want[i], plain[i][1], rtol=0, atol=1e-12)  # the files' expected scores are this module's plain model
        assert scores[i].shape == (10,)
        assert delta[i] < 0.08, (i, scores[i], want[i])


def test_resnet_packed_16_images_d_own_below_a_quarter_of_d_other(plain, run16):
    for l, i, d_own, d_other in distances(plain, run16[1], 16):
        assert d_own < d_other / 4, (l, i, d_own, d_other)


def test_resnet_packed_16_images_scores(plain, run16):
    check_scores(plain, run16[0], run16[2], 16)


def test_resnet_packed_partial_group_d_own_below_a_quarter_of_d_other(plain, run5):
    """`resnet_packed 3 8 1 5 false`"""
    for l, i, d_own, d_other in distances(plain, run5[1], 5):
        assert d_own < d_other / 4, (l, i, d_own, d_other)


def test_resnet_packed_partial_group_scores(plain, run5):
    check_scores(plain, run5[0], run5[2], 5)


def test_resnet_packed_image_batch_equals_single(run16, tmp_path):
    """HCONV_IMAGE_BATCH=4: the group's ciphertexts of a layer, and the stride layers' tails four at a time, as one launch set give the scores of one at a time, exactly
    (same HCONV_SEED; the dump of the single run is an observer)"""
    single = run16[0]
    batch, _, _ = run_packed(tmp_path, 16, {"HCONV_IMAGE_BATCH": "4"}, dump=False)
    for i in range(16):
        assert np.array_equal(single[i], batch[i]), (i, single[i], batch[i])
