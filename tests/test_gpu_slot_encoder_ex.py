"""hc_encode_slots_ex (ckks.(*encoderComplex128).Embed + scaleUpVecExact + ToNTT: sparse slots, rows modulo the special primes) on the GPU: the cases of
tests/slot_encoder_cases.py against the CPU oracle (shared with the CPU emulator's run of the same kernels), the reference binary's own encodeDiagonal digests
(tests/golden/ref_trace_diag_5_1.json, ref_trace_diag_sparse_ls1{1,2,3,4}.json), and the product CLI with HCONV_DEVICE_ENCODE=1 against =0. N = 2^16 is fixed: a case is
one to six vectors over 4 to 14 rows."""
import os
import re
import subprocess

import pytest

import golden.gen_conv_csv as gen
import oracle_ckks
import slot_encoder_cases as sc
import test_gpu_z_cli as zc
from optimal_conv_amd import Context
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

GPU = (lambda Q, P: Context(Q, P)), (lambda Q, P: Oracle(q=Q, p=P))


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_encoder_equals_the_oracle(c):
    """word for word, to_ntt 0 and 1, five kinds of input; off the gap grid every coefficient is the word 0; log_slots = 15 == hc_encode_slots"""
    sc.case(*GPU, *c)


def test_refusals_leave_the_context_usable():
    sc.case_refusals(*GPU)


@pytest.fixture(scope="module")
def set6_ctx():
    ctx = Context(list(oracle_ckks.Q_SET6), list(oracle_ckks.P_SET6))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("ls", [11, 12, 13, 14, 15])
def test_encoded_diagonals_are_the_reference_binarys(set6_ctx, ls):
    """the first and the last diagonal of matrix 0 of every sparse set (2^(ls+1) values) and of the full-slot set (ls = 15): mQ and mP as the binary hashed them"""
    sc.case_reference_digests(set6_ctx, ls)


def test_conv_relu_cli_device_encode_equals_host_encode(tmp_path):
    """`convReLU 5 1 1` with HCONV_DEVICE_ENCODE=1 and =0: the same digest of every diagonal's values and encoded polynomials (mod Q, mod P), line for line; the stats
    line names where the plaintexts were encoded; the same decrypted result (the encoded words are the same bits, so the seeded run does not change)"""
    gen.write_case(str(tmp_path / "test_conv_data"), 5, 1, 0)
    txt, dig = {}, {}
    for dev in (1, 0):
        path = tmp_path / f"dft_digests_{dev}.jsonl"
        out = subprocess.run([zc.CLI, "--test-mode", "convReLU", "5", "1", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=900,
                             env=dict(os.environ, HCONV_SEED="31", HCONV_SKIP_BL="1", HCONV_BOOT_STATS="1", HCONV_DFT_DIGESTS=str(path), HCONV_DEVICE_ENCODE=str(dev)))
        assert out.returncode == 0, out.stderr[-2000:]
        txt[dev], dig[dev] = out.stdout, open(path).read().splitlines()
    print(txt[1])
    assert len(dig[1]) >= 251 and dig[1] == dig[0], "the digests of the encoded diagonals differ between the device and the host encoder"
    zc.check_dft_digests_against_reference(tmp_path / "dft_digests_1.jsonl")
    stats = {dev: re.findall(r"^boot stats: (\d+) diagonals and (\d+) masks encoded on the (device|host)$", txt[dev], re.M) for dev in (1, 0)}
    assert len(stats[1]) == len(stats[0]) == 1 and stats[1][0][2] == "device" and stats[0][0][2] == "host" and stats[1][0][:2] == stats[0][0][:2], (stats, txt[1][-1500:])
    assert int(stats[1][0][0]) >= 251 and int(stats[1][0][1]) >= 1
    same = r"^(ciphertext digest|AVG Prec|MED Prec|MIN Prec|MAX Prec|ValuesTest|ValuesWant).*$"
    lines = {dev: [m.group(0) for m in re.finditer(same, txt[dev], re.M)] for dev in (1, 0)}
    assert lines[1] and lines[1] == lines[0], "the decrypted result changed with where the plaintexts are encoded"
