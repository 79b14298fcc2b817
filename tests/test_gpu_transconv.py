"""Stride-2 transposed convolution on the GPU: hc_prep_ker_ex(trans = 1) against the restatement of conv.go's formulas bit for bit, the
unchanged conv_then_pack kernels (alone and as an image batch) on its plaintexts against the oracle word for word, and the `transconv`
command decrypting to the torch model with the precision `conv` reaches at the same shape (tests/test_gpu_z_cli.py)."""
import os
import re
import subprocess

import pytest

import golden.gen_transconv_csv as gen
import transconv_ref as R

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


@pytest.mark.parametrize("k,i_batch", [(3, 0), (5, 1), (7, 2), (7, 3)])
def test_prep_ker_ex_on_device(env, k, i_batch):
    R.case_prep_ker_trans(*env, k, i_batch)


@pytest.mark.parametrize("k,i_batch,n", [(5, 1, 1), (5, 1, 3), (3, 2, 1)])
def test_conv_then_pack_on_trans_plaintexts(env, k, i_batch, n):
    R.case_conv_trans(*env, k, i_batch, n)


def run_cli(tmp_path, k, i_batch, extra=None):
    assert os.path.exists(CLI), "host CLI not built (__graft_entry__.build)"
    gen.write_case(str(tmp_path / "test_conv_data"), k, i_batch, 0)
    out = subprocess.run([CLI, "--test-mode", "transconv", str(k), str(i_batch), "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HCONV_SEED="2024", **(extra or {})))
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    return out.stdout


# floors: what `conv` is held to at the same k and batch index (test_gpu_z_cli.py)
@pytest.mark.parametrize("k,i_batch,min_med", [(3, 0, 23.0), (5, 1, 21.0), (7, 3, 17.5)])
def test_transconv_cli(tmp_path, k, i_batch, min_med):
    txt = run_cli(tmp_path, k, i_batch)
    assert re.search(r"^Ours start\.$", txt, re.M) and re.search(r"^\t Pack time:  \S+$", txt, re.M) and "Base Line start." not in txt
    avg = float(re.search(r"^AVG Prec : \(([-0-9.]+), \+Inf\) Log2", txt, re.M).group(1))
    med = float(re.search(r"^MED Prec : \(([-0-9.]+), \+Inf\) Log2", txt, re.M).group(1))
    print(f"transconv {k} {i_batch}: AVG {avg:.2f} bits, MED {med:.2f} bits")
    assert med >= min_med, txt


def test_transconv_cli_image_batch(tmp_path):
    """HCONV_IMAGE_BATCH = 3: three encryptions through one launch set decrypt to the same values up to the scheme's noise"""
    txt = run_cli(tmp_path, 5, 1, {"HCONV_IMAGE_BATCH": "3"})
    assert re.search(r"^Conv \(with BN\) Done in \S+  \(3 images\)$", txt, re.M), txt
    diffs = [float(d) for d in re.findall(r"^image \d of the batch: max \|difference\| to image 0 = (\S+), to the expected output = \S+$", txt, re.M)]
    assert len(diffs) == 2 and max(diffs) < 2.0 ** -15, txt
    assert float(re.search(r"^MED Prec : \(([-0-9.]+), \+Inf\) Log2", txt, re.M).group(1)) >= 21.0, txt
