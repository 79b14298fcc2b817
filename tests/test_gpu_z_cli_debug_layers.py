"""HCONV_DEBUG_LAYERS=1: the per-stage report of a layer (the reference's evalConv_BNRelu_new(..., debug = true), eval.go:440-604) through the command-line tool, every stage
decoded on the device by ONE hc_decrypt_decode_lv call at the stage's own level; with HCONV_DEBUG_LAYERS_CHECK=1 (test mode) every stage is decoded again by the host path
(limbs 0 and 1, host FFT) and the run ends unless the doubles are bit-identical.

The report is an observer: the run's own final block is textually the switch-off run's, and a replayed network keeps every layer digest.

Precision floors: the figures of the first seeded run on an MI355X (`convReLU 5 1 1`, HCONV_SEED=31; profiles/LEDGER.md) minus 1.0 bit. The run is deterministic; the margin is
for later changes of the draws. Printed (real, imaginary), AVG / MED:
    after CtoS   half 0 (20.99, 20.98) / (21.52, 21.50)    half 1 (20.99, 20.99) / (21.50, 21.51)
    after ReLU   half 0 ( 8.40, 16.79) / (11.54, 18.32)    half 1 ( 8.40, 16.81) / (11.53, 18.30)
    after StoC   half 0  16.92 / 18.63                     half 1  16.83 / 18.43      (coefficients: no imaginary part)"""
import json
import os
import re
import subprocess

import pytest

import golden.gen_conv_csv as gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")

# (AVG real, AVG imag, MED real, MED imag) per half: printed value - 1.0; None: the stage has no imaginary part (+Inf is printed)
FLOORS = {"ctos": [(19.99, 19.98, 20.52, 20.50), (19.99, 19.99, 20.50, 20.51)],
          "relu": [(7.40, 15.79, 10.54, 17.32), (7.40, 15.81, 10.53, 17.30)],
          "stoc": [(15.92, None, 17.63, None), (15.83, None, 17.43, None)]}
STAT = r"MIN Prec : \((\S+), (\S+)\) Log2 \nMAX Prec : \((\S+), (\S+)\) Log2 \nAVG Prec : \((\S+), (\S+)\) Log2 \nMED Prec : \((\S+), (\S+)\) Log2 \nErr stdF :  -Inf Log2 \nErr stdT :  -Inf Log2 \n"
SLOT_BLOCK = r"\nValuesTest:(?:-?\d+\.\d{5}, ){15}\.\.\. \nValuesWant:(?:-?\d+\.\d{5}, ){15}\.\.\. \n" + STAT + r"\n\n"
COEF_BLOCK = (r"len val Want: 65536\nlen val Test: (\d+)\n\nLevel: 1 \(logQ = 104\)\nScale: 2\^\d+\.\d+\nValuesTest:(?:-?\d+\.\d{10}, ){15}\.\.\. \nValuesWant:(?:-?\d+\.\d{10}, ){15}\.\.\. \n"
              + STAT + r"\n" + STAT + r"\n\n")
CHECK = r"stage decode: device == host \((\d+) values\)\n"


def run_cli(tmp_path, argv, **env):
    out = subprocess.run([CLI, "--test-mode"] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def final_block(txt):
    """the run's own result: from its last `ValuesTest:` line to the end of the statistics"""
    m = re.search(r"ValuesTest:[^\n]*\nValuesWant:[^\n]*\n" + STAT, txt[txt.rindex("ValuesTest:"):])
    assert m, txt[-1500:]
    return m.group(0)


def fig(s):
    return float("inf") if s == "+Inf" else float(s)


def check_floors(stage, half, g, where):
    """g: the eight figures of one statistics block (MIN, MAX, AVG, MED as real, imaginary)"""
    got = (fig(g[4]), fig(g[5]), fig(g[6]), fig(g[7]))
    print(f"{where}: {stage} half {half}: AVG ({g[4]}, {g[5]}) MED ({g[6]}, {g[7]})")
    for name, v, floor in zip(("AVG real", "AVG imag", "MED real", "MED imag"), got, FLOORS[stage][half]):
        if floor is None:
            assert v == float("inf"), f"{where}: {stage} half {half}: {name} = {v}: coefficients have no imaginary part"
        else:
            assert v >= floor, f"{where}: {stage} half {half}: {name} = {v} bits, floor {floor}"


def layer_pattern(nimg, halves, check):
    """the report of one layer, in the reference's order, as a regular expression over the tail's output; groups: per stage the check's count, then every block's figures"""
    ck = CHECK if check else ""
    img = lambda z: (rf"image {z}\n" if nimg > 1 else "")
    slot_stage = "".join(img(z) + SLOT_BLOCK * halves for z in range(nimg))
    return (r"layer debug: kind (\S+) log_sparse (\d) images " + str(nimg) + r"\n" + ck + r"Bootstrapping\.\.\. Ours \(until CtoS\):\nDone in \S+ \n" + ck + slot_stage
            + r"(?:Eval: )+ReLU Done in \S+ \nafter Relu:  \S+ lv:  \d+\n" + ck + slot_stage
            + r"Boot \(StoC\) Done in \S+ \n(?:replay digest[^\n]*\n)*Boot out: \n" + ck + "".join(img(z) + COEF_BLOCK for z in range(nimg)))


@pytest.mark.parametrize("nimg", [1, 2])
def test_conv_relu_report_blocks_floors_check_and_unchanged_result(tmp_path, nimg):
    """`convReLU 5 1 1` (kind Conv: two halves; merged as images through the sine and the ReLU), one image and HCONV_IMAGE_BATCH=2: the blocks in the reference's order with
    the counts of the kind, one check line per stage over all images and both halves, every block above its floor, and the run's own final block textually equal to the
    switch-off run's"""
    gen.write_case(str(tmp_path / "test_conv_data"), 5, 1, 0)
    base = dict(HCONV_SEED="31", HCONV_SKIP_BL="1", HCONV_IMAGE_BATCH=str(nimg))
    off = run_cli(tmp_path, ["convReLU", "5", "1", "1"], **base)
    assert "layer debug" not in off and "stage decode" not in off and "Boot out" not in off and "after Relu" not in off
    on = run_cli(tmp_path, ["convReLU", "5", "1", "1"], HCONV_DEBUG_LAYERS="1", HCONV_DEBUG_LAYERS_CHECK="1", **base)
    m = re.search(layer_pattern(nimg, 2, True), on)
    assert m, on[-6000:]
    g = list(m.groups())
    assert g[0] == "Conv" and g[1] == "0"
    g = g[2:]
    assert g.pop(0) == str(nimg * 65536)                                    # the convolution's result: coefficients of every image
    for stage in ("ctos", "relu"):
        assert g.pop(0) == str(nimg * 2 * 32768)                            # both halves of every image in one call: 2^15 slots each
        for z in range(nimg):
            for half in range(2):
                check_floors(stage, half, g[:8], f"image {z}")
                g = g[8:]
    assert g.pop(0) == str(nimg * 65536)
    for z in range(nimg):
        assert g.pop(0) == "65536"
        for half in range(2):
            check_floors("stoc", half, g[:8], f"image {z}")
            g = g[8:]
    assert not g
    assert len(re.findall(CHECK, on)) == 4
    assert final_block(on) == final_block(off), "the report changed the run's own result"


def test_check_switch_is_test_mode_only(tmp_path):
    gen.write_case(str(tmp_path / "test_conv_data"), 5, 1, 0)
    out = subprocess.run([CLI, "convReLU", "5", "1", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, HCONV_SKIP_BL="1", HCONV_DEBUG_LAYERS="1", HCONV_DEBUG_LAYERS_CHECK="1"))
    assert out.returncode == 2 and "HCONV_DEBUG_LAYERS_CHECK is set but the CLI was not started with --test-mode" in out.stderr, out.stderr[-500:]


def test_resnet_report_on_every_sparse_kind_keeps_every_digest(tmp_path):
    """`resnet 3 20 1 1 false` under HCONV_RESNET_REPLAY=1 with the report and the check on: all 19 layer digests still equal tests/golden/oracle_resnet_digests.json (the
    report changed no ciphertext), and every layer - kinds Conv_sparse (log_sparse 2, 3, 4: one packed ciphertext, 2^(16 - log_sparse) slots) and StrConv_sparse
    (log_sparse 1, 2) - printed its blocks with the check's line at every stage"""
    import golden.gen_resnet_csv as rgen
    rgen.write_case(str(tmp_path), 3, 20, 1, native_image=True)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_resnet_digests.json")))["depth"]["20"]
    txt = run_cli(tmp_path, ["resnet", "3", "20", "1", "1", "false"], HCONV_RESNET_REPLAY="1", HCONV_DEBUG_LAYERS="1", HCONV_DEBUG_LAYERS_CHECK="1")
    got_d = {int(m.group(1)): m.group(2) for m in re.finditer(r"^replay digest layer (\d+) image 0 level 1 scale \S+ ([0-9a-f]{64})$", txt, re.M)}
    assert sorted(got_d) == list(range(19)), sorted(got_d)
    for i, w in enumerate(ref["layers"]):
        assert got_d[i] == w, f"layer {i}: the ciphertext differs from the oracle network's with the report on"
    layers = list(re.finditer(layer_pattern(1, 1, True), txt))
    assert len(layers) == 19, len(layers)
    kinds = {}
    for m in layers:
        g = m.groups()
        kind, ls = g[0], int(g[1])
        kinds[(kind, ls)] = kinds.get((kind, ls), 0) + 1
        # conv: N coefficients; CtoS and ReLU: one packed ciphertext of 2^(16 - ls) slots; StoC: N coefficients, of which 2 * 2^(15 - ls) are compared
        assert (g[2], g[3], g[12], g[21], g[22]) == ("65536", str(1 << (16 - ls)), str(1 << (16 - ls)), "65536", str(1 << (16 - ls))), (kind, ls, g[2], g[3], g[12], g[21], g[22])
    assert kinds == {("Conv_sparse", 2): 7, ("Conv_sparse", 3): 5, ("Conv_sparse", 4): 5, ("StrConv_sparse", 1): 1, ("StrConv_sparse", 2): 1}, kinds


def test_resnet_fast_report_on_the_inside_kinds(tmp_path):
    """`resnet_fast 3 8 1 1 false`: the full-slot kinds Conv_inside / StrConv_inside (two halves, kept with the context's stride masks) print their blocks in every layer, the check holds
    at every stage, and the class scores are those of the switch-off run, exactly"""
    import numpy as np
    import golden.gen_resnet_csv as rgen
    rgen.write_case(str(tmp_path), 3, 8, 1)
    res = tmp_path / "Resnet_enc_results" / "results_crop_ker3_d8_wid1" / "class_result_ker3_0.csv"
    run_cli(tmp_path, ["resnet_fast", "3", "8", "1", "1", "false"], HCONV_SEED="11")
    off = np.loadtxt(res)
    txt = run_cli(tmp_path, ["resnet_fast", "3", "8", "1", "1", "false"], HCONV_SEED="11", HCONV_DEBUG_LAYERS="1", HCONV_DEBUG_LAYERS_CHECK="1")
    assert np.array_equal(np.loadtxt(res), off), "the report changed the network's scores"
    layers = list(re.finditer(layer_pattern(1, 2, True), txt))
    kinds = sorted({m.group(1) for m in layers})
    assert layers and len(layers) == txt.count("layer debug:") and kinds == ["Conv_inside", "StrConv_inside"], (len(layers), txt.count("layer debug:"), kinds)
    assert len(re.findall(CHECK, txt)) == 4 * len(layers)
