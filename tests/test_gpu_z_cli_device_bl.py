"""HCONV_DEVICE_ENCRYPT on the Base Line column of the product CLI (fresh child processes, as tests/test_gpu_z_cli.py): 1 = both input halves are encoded and encrypted,
and both results decrypted and decoded, on the device (hc_encode_slots / hc_encrypt_sk / hc_decrypt_decode_slots); 0 = the host codec. The floors are the ones
test_gpu_z_cli.test_conv_cli holds `conv 3 0 1` to, taken from that test."""
import re

import pytest

import golden.gen_conv_csv as gen
import test_gpu_z_cli_device_encrypt as de

pytestmark = pytest.mark.gpu
BL_LINE = r"^Base Line: encryption and decryption on the device \(hc_encode_slots / hc_encrypt_sk / hc_decrypt_decode_slots\)$"


@pytest.mark.parametrize("device", [1, 0])
def test_conv_cli_base_line_with_the_device_codec_and_without(tmp_path, device):
    gen.write_case(str(tmp_path / "test_conv_data"), 3, 0, 0)
    txt = de.run(tmp_path, ["conv", "3", "0", "1"], {"HCONV_SEED": "1", "HCONV_DEVICE_ENCRYPT": str(device)})
    print(txt)
    assert re.search(r"^Ours start\.$", txt, re.M) and re.search(r"^\t Pack time:  \S+$", txt, re.M)
    meds = [float(m) for m in re.findall(de.MED, txt, re.M)]
    min_bl, min_med = de.FLOORS[(3, 0)]
    assert len(meds) == 2 and meds[0] >= min_bl and meds[1] >= min_med, txt
    assert len(re.findall(BL_LINE, txt, re.M)) == (1 if device else 0), txt
    assert bool(re.search(de.DEVICE_LINE, txt, re.M)) == bool(device), txt
