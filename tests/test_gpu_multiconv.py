"""The convolution with several input ciphertexts on the device: hc_conv_then_pack_batch's members with one ct_out are the inputs of ONE convolution (hc_k_a1g sums the
level-1 products ahead of the one rescale, hc_k_a3g the level-0 products in its epilogue, one pack tree per group). Word for word against tests/multiconv_ref.py, which
tests/test_multiconv_cpu.py pins to the oracle; every modulus-size branch at the group sizes that cross hc_k_a1g's pair boundary (odd m) and reach its 8 pair sums
(m = 16); the `multiconv` command's decrypted precision."""
import os
import re
import subprocess

import pytest

import golden.gen_multiconv_csv as gen
import multiconv_cases as mc
import parity_cases as pc
from optimal_conv_amd import Context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")

GPU = lambda Q, P: Context(Q, P)


@pytest.fixture(scope="module")
def env():
    from oracle_lib import Oracle, P0, Q0, Q1
    ctx = Context([Q0, Q1], [P0], device=0)
    yield ctx, Oracle()
    ctx.close()


@pytest.mark.parametrize("m,G,max_ob,norm,chunk", mc.GROUP_TABLE, ids=[mc.group_id(t) for t in mc.GROUP_TABLE])
def test_groups(env, m, G, max_ob, norm, chunk):
    mc.case_groups(*env, m, G, max_ob, norm, chunk)


def test_groups_on_the_big_level_kernels(env):
    """small_levels = 0: the group's tree on the 256-thread kernels"""
    env[0].set_option("small_levels", 0)
    try:
        mc.case_groups(*env, 3, 2, 4, 1, 5)
    finally:
        env[0].set_option("small_levels", 16)


def test_second_call_gives_the_same_words(env):
    """workspaces sized by an earlier, larger call are reused: two calls, both the yardstick's words"""
    mc.case_groups(*env, 4, 2, 2, 1, None, seed=0x7F1, calls=2)


def test_multi_binding(env):
    mc.case_multi_binding(*env)


def test_refusals(env):
    mc.case_refusals(*env)


def test_distinct_outputs_are_the_batch_of_before(env):
    mc.case_distinct_outputs_unchanged(*env)


@pytest.mark.parametrize("inputs", ["random", "edge"])
@pytest.mark.parametrize("triple", pc.CONV_TRIPLES, ids=pc.conv_triple_id)
def test_every_modulus_branch(triple, inputs):
    mc.case_branch(GPU, triple, inputs)


# MED Prec floors: the floor tests/test_gpu_z_cli.py holds `conv k i` to (23.0 / 21.0 / 17.5 bits), minus 0.5*log2(m) for the m independent ciphertext noises that add, minus
# 0.5 bit of margin for the seed
# the last case: HCONV_DEVICE_ENCRYPT=1, the m * image_batch inputs through one hc_encode_coeffs / hc_encrypt_sk call and the results through one hc_decrypt_decode_coeffs call
@pytest.mark.parametrize("k,i_batch,m,image_batch,floor,device_encrypt", [(3, 0, 2, 1, 22.0, False), (5, 1, 4, 1, 19.5, False), (7, 3, 2, 1, 16.5, False), (3, 0, 2, 2, 22.0, False),
                                                                          (5, 1, 4, 2, 19.5, True)])
def test_multiconv_cli(tmp_path, k, i_batch, m, image_batch, floor, device_encrypt):
    assert os.path.exists(CLI), "host CLI not built (__graft_entry__.build)"
    gen.write_case(str(tmp_path / "test_conv_data"), k, i_batch, 0, m)
    env = dict(os.environ, HCONV_SEED="2024")
    if image_batch > 1:
        env["HCONV_IMAGE_BATCH"] = str(image_batch)
    if device_encrypt:
        env["HCONV_DEVICE_ENCRYPT"] = "1"
    out = subprocess.run([CLI, "--test-mode", "multiconv", str(k), str(i_batch), "1", str(m)], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    txt = out.stdout
    assert re.search(r"^Ours start\.$", txt, re.M) and re.search(rf"^num input ciphertexts:  {m}$", txt, re.M) and re.search(r"^\t Pack time:  \S+$", txt, re.M), txt
    assert "Base Line start." not in txt
    meds = [float(x) for x in re.findall(r"^MED Prec : \(([-0-9.]+), \+Inf\) Log2", txt, re.M)]
    print(f"multiconv {k} {i_batch} 1 {m} image_batch={image_batch}: MED Prec {meds}")
    assert len(meds) == 1 and meds[0] >= floor, txt
    assert ("Encryption and decryption on the device" in txt) == device_encrypt, txt
    if image_batch > 1:
        assert re.search(r"^image 1 of the batch: max \|difference\| to image 0 = \S+, to the expected output = \S+$", txt, re.M), txt
