"""`resnet_fast` (testResNet_crop_fast_in, test.go:372-636) on the GPU: hc_prep_ker_ex2's dilated / channel-strided plaintexts and the k = 31 FC
kernel bit for bit, and the full-slot network's class scores against the plain model of the same network (tests/golden/gen_resnet_csv.py; for
k = 3 the stride layers keep the even positions, the plain model's phase: tests/test_resnet_fast_cpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden.gen_resnet_csv as rgen
import resnet_fast_ref as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")


@pytest.fixture(scope="module")
def env():
    from optimal_conv_amd import Context
    from oracle_lib import Oracle, P0, Q0, Q1
    ctx = Context([Q0, Q1], [P0], device=0)
    yield ctx, Oracle()
    ctx.close()


@pytest.mark.parametrize("shape", F.DRIVER_SHAPES)
def test_prep_ker_ex2_on_device(env, shape):
    F.case_prep_ker_ex2(env[0], *shape)


def test_prep_ker_fc_k31_on_device(env):
    F.case_fc_k31(*env)


def run_fast(tmp_path, depth, n, extra=None, timeout=900):
    out = subprocess.run([CLI, "--test-mode", "resnet_fast", "3", str(depth), "1", str(n), "false"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=timeout, env=dict(os.environ, HCONV_SEED="11", **(extra or {})))
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout[-1500:])
    for pat in (r"^Block1, Layer  1 done!$", r"^Block1 to 2 done!$", r"^Block2 to 3 done!$", r"^Block3 done\.$", r"^Final FC done\.$", r"^Total done in \S+ "):
        assert re.search(pat, out.stdout, re.M), pat
    d = tmp_path / "Resnet_enc_results" / f"results_crop_ker3_d{depth}_wid1"
    return [np.loadtxt(d / f"class_result_ker3_{i}.csv") for i in range(n)], out.stdout


def test_resnet_fast_cli_depth8(tmp_path):
    """`resnet_fast 3 8 1 1 false`: the bounds test_resnet_cli_depth8 holds for `resnet` (same arg-max, max |delta| < 0.08)"""
    (want, _), = rgen.write_case(str(tmp_path), 3, 8, 1)
    (got,), txt = run_fast(tmp_path, 8, 1)
    assert "Generating bootstrapping keys..." in txt
    assert got.shape == (10,)
    assert got.argmax() == want.argmax(), (got, want)
    assert np.max(np.abs(got - want)) < 0.08, (got, want)


def test_resnet_fast_cli_image_batch_equals_single(tmp_path):
    """HCONV_IMAGE_BATCH=2: both images through every layer as one launch set give the scores of the one-at-a-time run, exactly"""
    want = rgen.write_case(str(tmp_path), 3, 8, 2)
    single, _ = run_fast(tmp_path, 8, 2)
    batch, txt = run_fast(tmp_path, 8, 2, {"HCONV_IMAGE_BATCH": "2"})
    assert "(2 images)" in txt
    for i in range(2):
        assert np.array_equal(single[i], batch[i]), (i, single[i], batch[i])
        assert single[i].argmax() == want[i][0].argmax(), (i, single[i], want[i][0])


def test_resnet_fast_cli_depth20(tmp_path):
    """`resnet_fast 3 20 1 1 false`: 19 full-slot layers and the FC; the sparse driver's depth-20 bound (same arg-max, max |delta| < 0.05)"""
    (want, _), = rgen.write_case(str(tmp_path), 3, 20, 1, native_image=True)
    (got,), txt = run_fast(tmp_path, 20, 1)
    assert re.search(r"^Block1, Layer  7 done!$", txt, re.M) and re.search(r"^Block2, Layer  5 done!$", txt, re.M)
    assert got.argmax() == want.argmax(), (got, want)
    assert np.max(np.abs(got - want)) < 0.05, (got, want)
