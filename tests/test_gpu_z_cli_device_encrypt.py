"""HCONV_DEVICE_ENCRYPT on the product CLI (fresh child processes, as tests/test_gpu_z_cli.py): 1 = the input is encoded and encrypted, and the result decrypted and
decoded, on the device (hc_encode_coeffs / hc_encrypt_sk / hc_decrypt_decode_coeffs); 0 = the host encryptor and decryptor; under a replay switch the draws stay the
oracle harness' host draws whatever the switch says. Floors and tolerances are the ones the existing CLI tests hold the same commands to, taken from those tests."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

import golden.gen_conv_csv as gen
import test_gpu_transconv as tc
import test_gpu_z_cli as zc

pytestmark = pytest.mark.gpu
CLI = zc.CLI
DEVICE_LINE = r"^Encryption and decryption on the device \(hc_encrypt_sk / hc_decrypt_decode_coeffs\)$"
# test_conv_cli's floors, by (k, batch index): (baseline MED, Ours MED)
FLOORS = {(k, i): (bl, med) for k, i, bl, med in next(m for m in zc.test_conv_cli.pytestmark if m.name == "parametrize").args[1]}
# test_transconv_cli_image_batch's bound on what two encryptions of one input may differ by after the layer
_m = re.search(r"max\(diffs\) < (2\.0 \*\* -\d+)", inspect.getsource(tc.test_transconv_cli_image_batch))
assert _m, "test_transconv_cli_image_batch no longer states its tolerance as max(diffs) < 2.0 ** -k"
BATCH_TOL = eval(_m.group(1))
MED = r"^MED Prec : \(([-0-9.]+), \+Inf\) Log2"


def run(tmp_path, argv, env):
    assert os.path.exists(CLI), "host CLI not built (__graft_entry__.build)"
    out = subprocess.run([CLI, "--test-mode"] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


@pytest.mark.parametrize("device", [1, 0])
def test_conv_cli_precision_with_the_device_encryptor_and_without(tmp_path, device):
    gen.write_case(str(tmp_path / "test_conv_data"), 3, 0, 0)
    txt = run(tmp_path, ["conv", "3", "0", "1"], {"HCONV_SEED": "1", "HCONV_DEVICE_ENCRYPT": str(device), "HCONV_SKIP_BL": "1"})
    print(txt)
    assert re.search(r"^Ours start\.$", txt, re.M) and re.search(r"^\t Pack time:  \S+$", txt, re.M)
    meds = [float(m) for m in re.findall(MED, txt, re.M)]
    assert len(meds) == 1 and meds[-1] >= FLOORS[(3, 0)][1], txt
    assert bool(re.search(DEVICE_LINE, txt, re.M)) == bool(device), txt


def values_test(txt):
    """the ten decrypted values each iteration prints"""
    return np.array([[float(x) for x in line.split(":", 1)[1].split(",")[:10]] for line in re.findall(r"^ValuesTest:.*$", txt, re.M)])


def test_transconv_cli_image_batch_with_the_device_encryptor(tmp_path):
    """`transconv 3 0 3` under HCONV_IMAGE_BATCH=3 (three encryptions per input from ONE hc_encrypt_sk call, decrypted by ONE hc_decrypt_decode_coeffs call) against the
    same three inputs under HCONV_IMAGE_BATCH=1: other stream ids, so other noise; the decrypted values agree under the bound the existing image-batch test holds the
    images of a batch to, and so do the images of each batch among themselves"""
    import golden.gen_transconv_csv as tgen
    for it in range(3):
        tgen.write_case(str(tmp_path / "test_conv_data"), 3, 0, it)
    env = {"HCONV_SEED": "1", "HCONV_DEVICE_ENCRYPT": "1"}
    batch = run(tmp_path, ["transconv", "3", "0", "3"], dict(env, HCONV_IMAGE_BATCH="3"))
    single = run(tmp_path, ["transconv", "3", "0", "3"], dict(env, HCONV_IMAGE_BATCH="1"))
    print(batch)
    assert re.search(DEVICE_LINE, batch, re.M) and re.search(DEVICE_LINE, single, re.M)
    assert len(re.findall(r"^Conv \(with BN\) Done in \S+  \(3 images\)$", batch, re.M)) == 3, batch
    diffs = [float(d) for d in re.findall(r"^image \d of the batch: max \|difference\| to image 0 = (\S+), to the expected output = \S+$", batch, re.M)]
    print("max |difference| between the images of a batch:", diffs)
    assert len(diffs) == 6 and 0 < min(diffs) and max(diffs) < BATCH_TOL, batch      # 0 would mean the images share their randomness
    vb, vs = values_test(batch), values_test(single)
    assert vb.shape == vs.shape == (3, 10)
    print("max |batch - single| over the printed values:", np.abs(vb - vs).max())
    assert np.abs(vb - vs).max() < BATCH_TOL
    for txt in (batch, single):
        meds = [float(m) for m in re.findall(MED, txt, re.M)]
        assert len(meds) == 3 and min(meds) >= FLOORS[(3, 0)][1], txt


def test_replay_keeps_the_host_draws_under_the_device_switch(tmp_path):
    """HCONV_RESNET_REPLAY=1 with HCONV_DEVICE_ENCRYPT=1: the encryption draws stay the oracle harness' host draws, so the depth-8 network still hands on the oracle
    network's ciphertext after every layer (tests/golden/oracle_resnet_digests.json) and the device encryptor is not announced"""
    import golden.gen_resnet_csv as rgen
    rgen.write_case(str(tmp_path), 3, 8, 1, native_image=True)
    ref = json.load(open(os.path.join(zc.ROOT, "tests", "golden", "oracle_resnet_digests.json")))["depth"]["8"]
    txt = run(tmp_path, ["resnet", "3", "8", "1", "1", "false"], {"HCONV_RESNET_REPLAY": "1", "HCONV_DEVICE_ENCRYPT": "1"})
    got = {int(m.group(1)): m.group(2) for m in re.finditer(r"^replay digest layer (\d+) image 0 level 1 scale \S+ ([0-9a-f]{64})$", txt, re.M)}
    assert sorted(got) == list(range(len(ref["layers"]))), sorted(got)
    for i, w in enumerate(ref["layers"]):
        assert got[i] == w, f"layer {i}: the replayed ciphertext changed under HCONV_DEVICE_ENCRYPT=1"
    assert not re.search(DEVICE_LINE, txt, re.M)
