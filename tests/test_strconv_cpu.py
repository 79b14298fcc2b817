"""The full-packing stride layer and the ImageNet tail without a GPU: (1) the host's gen_comprs_full (header-only in hconv_host.hpp, through a small stand-alone
tool), applied as masks and rotations between the CtoS and StoC slot orders, is the layout tests/imagenet_ref.py states; (2) hc_prep_ker_fc on the emulated kernel
library equals hc_prep_ker_ex2 on the host-replicated kernel word for word, and refuses what it refuses; (3) the generators: strconvReLU's expected output is the
model layer's, gen_imagenet_csv keeps every pre-activation inside the ReLU's range and its model scores are pinned; (4) the two commands' refusals."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import golden.gen_imagenet_csv as igen
import golden.gen_strconv_relu_csv as sgen
import imagenet_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "kernel_emu")
EMU_LIB = os.path.join(EMU_DIR, "_build", "libhconv_emu.so")
N, n = R.N, R.N // 2
BREV = np.array([int(format(i, "015b")[::-1], 2) for i in range(n)])

TOOL_SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include "hconv_host.hpp"
namespace hconv { [[noreturn]] void panic(const std::string &m) { fprintf(stderr, "panic: %s\n", m.c_str()); exit(2); } }
// <vec_size> <in_wid> <kp_wid> <pos> <ul>: one line per rotation, "rot i0 i1 ..." with the mask's set positions
int main(int c, char **v) {
    if (c < 6) return 1;
    for (auto &e : hconv::gen_comprs_full(atoi(v[1]), atoi(v[2]), atoi(v[3]), atoi(v[4]), atoi(v[5]))) {
        printf("%d", e.first);
        for (size_t i = 0; i < e.second.size(); i++) if (e.second[i]) printf(" %zu", i);
        printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def comprs_tool(tmp_path_factory):
    d = tmp_path_factory.mktemp("comprstool")
    src = d / "comprs.cpp"
    src.write_text(TOOL_SRC)
    exe = d / "comprs"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "optimal_conv_amd", "host"), "-o", str(exe), str(src)])

    def run(*args, check=True):
        return subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, check=check)
    return run


def table(tool, in_wid, kp_wid, pos, ul):
    out = {}
    for line in tool(n, in_wid, kp_wid, pos, ul).stdout.splitlines():
        t = [int(x) for x in line.split()]
        m = np.zeros(n)
        m[t[1:]] = 1
        assert t[0] not in out
        out[t[0]] = m
    return out


def through_the_tables(cf, tabs):
    """debugCtoS -> sum over (rot, mask) of Rotate(v * mask, rot) per half -> debugStoC: slot i of half ul is coefficient brev(i) + ul*N/2, both ways"""
    res = np.zeros(N)
    for ul in (0, 1):
        s = cf[BREV + ul * n]
        o = np.zeros(n)
        for rot, mask in tabs[ul].items():
            o += np.roll(s * mask, -rot)                      # Rotate(v, rot)[p] = v[p + rot]
        res[ul * n:(ul + 1) * n] = o[BREV]
    return res


@pytest.mark.parametrize("in_wid,kp_wid", [(16, 14), (16, 12), (32, 30)])
def test_host_gen_comprs_full_is_the_layout(comprs_tool, in_wid, kp_wid):
    cf = np.arange(1, N + 1, dtype=np.float64)               # an index vector: every coefficient names itself
    rots = None
    for pos in range(4):
        tabs = [table(comprs_tool, in_wid, kp_wid, pos, ul) for ul in (0, 1)]
        assert set(tabs[0]) == set(tabs[1]) and len(tabs[0]) == in_wid // 2, "the halves share their rotations: 8 at in_wid 16, 16 at 32"
        assert len({r % n for r in tabs[0]}) == in_wid // 2
        got = through_the_tables(cf, tabs)
        want = R.stride_layout(cf, in_wid, kp_wid, pos)
        assert np.count_nonzero(want) == (kp_wid // 2) ** 2 * (N // in_wid ** 2)
        assert np.array_equal(got, want), (in_wid, kp_wid, pos)
        rots = (rots or set()) | set(tabs[0])
    assert len(rots) == 4 * (in_wid // 2), "the four positions move by different amounts"


def test_host_gen_comprs_full_refusals(comprs_tool):
    for args, msg in (((n, 16, 7, 0, 0), "keep width too small"), ((n, 18, 14, 0, 0), "not divisible by 4"), ((n, 16, 14, 4, 0), "pos not in 0..3"), ((n, 16, 14, 0, 2), "ul not 0 nor 1")):
        r = comprs_tool(*args, check=False)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)


# ---------------------------------------------------------------- hc_prep_ker_fc on the emulated library
@pytest.fixture(scope="module")
def emu():
    from optimal_conv_amd import Context
    from oracle_lib import P0, Q0, Q1
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, EMU_LIB])
    ctx = Context([Q0, Q1], [P0], lib_path=EMU_LIB)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("shape", R.PREP_FC_SHAPES)
def test_prep_ker_fc_emulated(emu, shape):
    R.case_prep_ker_fc(emu, *shape)


def test_prep_ker_fc_refusals(emu):
    """the shapes hc_prep_ker_ex2 refuses on the replicated kernel, by the same rules; and the wrapper's own size check"""
    f64p = C.POINTER(C.c_double)

    def call(in_wid, k, real_ib, real_ob, norm, dil, null=None):
        fc, bna, h = np.zeros(max(1, real_ib * real_ob)) + 0.5, np.ones(max(1, real_ob)), C.c_void_p()
        rc = emu.L.hc_prep_ker_fc(emu.h, None if null == "fc" else fc.ctypes.data_as(f64p), None if null == "bn" else bna.ctypes.data_as(f64p), in_wid, k, real_ib, real_ob, norm, 2.0 ** 30, dil,
                                  None if null == "out" else C.byref(h))
        if rc == 0:
            emu.ker_free(h)
        return rc
    assert call(32, 3, 16, 16, 1, 1) == 0 and call(32, 3, 16, 10, 4, 1) == 0 and call(32, 3, 64, 64, 1, 15) == 0
    for args in ((32, 3, 16, 16, 1, 0), (32, 3, 16, 16, 1, -1), (32, 3, 16, 16, 0, 1), (32, 3, 0, 16, 1, 1), (32, 3, 16, 0, 1, 1), (32, 0, 16, 16, 1, 1), (0, 3, 16, 16, 1, 1),
                 (48, 3, 4, 4, 1, 1),                             # in_wid^2 does not divide N
                 (32, 3, 65, 16, 1, 1), (32, 3, 16, 65, 1, 1), (32, 3, 32, 16, 4, 1),        # norm * batch past max_bat = 64
                 (32, 3, 16, 16, 1, 16), (32, 2, 16, 16, 1, 31)):  # the dilated width past the grid / past 2*adj <= N
        assert call(*args) != 0, args
    for null in ("fc", "bn", "out"):
        assert call(32, 3, 16, 16, 1, 1, null=null) != 0
    from optimal_conv_amd import HconvError
    with pytest.raises(HconvError, match="real_ib\\*real_ob"):
        emu.prep_ker_fc(np.zeros(9 * 16 * 16), np.ones(16), 32, 3, 16, 16)


def test_prep_ker_fc_is_in_the_table_and_the_library():
    from optimal_conv_amd import SYMBOLS, abi
    assert "hc_prep_ker_fc" in SYMBOLS and len(SYMBOLS["hc_prep_ker_fc"][1]) == 11
    if not os.path.exists(abi.DEFAULT_LIB):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(abi.load(), "hc_prep_ker_fc")


def test_prep_ker_scatter_forms_do_not_spill():
    """hipcc's kernel-resource-usage remarks for every instantiation of hc_k_prep_ker, the shared-matrix form among them: no scratch, as tests/test_kernel_resources.py demands of
    the hot kernels (same flags, the shipped library's)"""
    import re
    import shutil
    import __graft_entry__
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    r = subprocess.run([hipcc, *__graft_entry__.HIP_FLAGS, "--cuda-device-only", "-S", "-o", os.devnull, os.path.join(ROOT, "optimal_conv_amd", "csrc", "hconv.hip"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: _Z\d+(\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert names and len(names) == len(scratch)
    forms = {nm: sc for nm, sc in zip(names, scratch) if nm.startswith("hc_k_prep_kerI")}
    assert len(forms) == 4 and any(nm.startswith("hc_k_prep_kerILb0ELb1ELb1E") for nm in forms), sorted(forms)
    assert not any(forms.values()), forms


# ---------------------------------------------------------------- the generators
@pytest.mark.parametrize("k,i_batch", [(3, 3), (5, 3), (3, 2)])
def test_strconv_generator_writes_the_model_layer(tmp_path, k, i_batch):
    """reluout is the kept cells of the model layer's result at any pos, and nothing else of that result is non-zero"""
    B, W, raw = sgen.write_case(str(tmp_path), k, i_batch, 0)
    assert raw == 2 * (W // 2 - k // 2) == sgen.kp_wid(k, i_batch) and W - raw >= k // 2
    _, _, _, x, ker, a, b = sgen.make_case(k, i_batch, 0)
    relu = np.loadtxt(tmp_path / f"test_strconv{k}_batch_{B}_reluout_0.csv").reshape(raw // 2, raw // 2, B)
    for pos in (0, 3):
        res = R.strconv_layer(x, ker, a, b, W, pos).reshape(W // 2, W // 2, 4 * B)
        assert np.array_equal(res[:raw // 2, :raw // 2, B * pos:B * (pos + 1)], relu)
        assert np.count_nonzero(res) == np.count_nonzero(relu)


def test_imagenet_generator_range_and_pinned_scores(tmp_path):
    case = igen.FIXTURE_CASE
    layers, fc, images, scores, peaks = igen.make(**case)
    for li, p in enumerate(peaks):                             # the generator asserts it too; here at both ends: inside the range, and not far below it
        assert 0.5 * 2.0 ** R.POWS[li] < p <= igen.HEADROOM * 2.0 ** R.POWS[li], (li, p)
    pinned = json.load(open(igen.FIXTURE))
    assert {key: pinned[key] for key in case} == case
    np.testing.assert_allclose(np.array(scores), np.array(pinned["scores"]), rtol=1e-9, atol=1e-12)
    assert [int(np.argmax(s)) for s in scores] == [int(np.argmax(s)) for s in pinned["scores"]]
    got, _ = igen.write(str(tmp_path), **case)
    c1, k = case["c1"], case["k"]
    w = tmp_path / f"weight_imgnet_ker{k}_h5"
    assert np.loadtxt(w / "w13-conv.csv").size == k * k * c1 * 2 * c1 and np.loadtxt(w / "w14-a.csv").size == 2 * c1 and np.loadtxt(w / "w16-conv.csv").size == k * k * 4 * c1 * c1
    assert np.loadtxt(w / "fc.csv").size == 2 * c1 * 1000 and not (w / "w10-a.csv").exists() and (w / "w17-b.csv").exists()
    assert np.loadtxt(tmp_path / f"ker{k}_data" / "test_image_1.csv").size == 14 * 14 * c1
    assert np.array_equal(np.loadtxt(tmp_path / f"ker{k}_plain_result" / "plain_result_1.csv"), scores[1])


def test_imagenet_generator_refuses_a_range_it_cannot_keep(monkeypatch):
    monkeypatch.setattr(igen, "HEADROOM", 0.0078125)           # 0.5 of bias alone leaves 2^5 / 128
    with pytest.raises(AssertionError, match="pre-activation"):
        igen.make(3, 1, 4, 1)


# ---------------------------------------------------------------- the commands' refusals
@pytest.mark.parametrize("argv,env,msg", [(["strconvReLU", "3", "3", "1", "4"], {}, "the pack position is 0..3"),
                                          (["strconvReLU", "3", "3", "1", "x"], {}, "the pack position is 0..3"),
                                          (["strconvReLU", "3", "3", "1", "0", "1"], {}, "at most one optional argument"),
                                          (["strconvReLU", "4", "3", "1"], {}, "Wrong kernel wid (not in 3,5,7)"),
                                          (["strconvReLU", "3", "4", "1"], {}, "Too many tests (>10) or too many batch index (>3)"),
                                          (["strconvReLU", "3", "3", "11"], {}, "Too many tests (>10) or too many batch index (>3)"),
                                          (["strconvReLU", "3", "3"], {}, "runtime error: index out of range"),
                                          (["--test-mode", "strconvReLU", "3", "3", "1"], {"HCONV_CHAIN_REPLAY": "5"}, "strconvReLU: HCONV_CHAIN_REPLAY"),
                                          (["imagenet", "4", "1"], {}, "strange ker name!"),
                                          (["imagenet", "7", "1"], {}, "strange ker name!"),
                                          (["imagenet", "3"], {}, "runtime error: index out of range"),
                                          (["imagenet", "3", "1", "16", "x"], {}, "runtime error: index out of range"),
                                          (["imagenet", "3", "0"], {}, "test_num must be at least 1"),
                                          (["imagenet", "3", "1", "0"], {}, "c1 not in 1..256"),
                                          (["imagenet", "3", "1", "257"], {}, "c1 not in 1..256"),
                                          (["--test-mode", "imagenet", "3", "1", "16"], {"HCONV_RESNET_REPLAY": "7"}, "imagenet: HCONV_RESNET_REPLAY"),
                                          (["--test-mode", "imagenet", "3", "1", "16"], {"HCONV_CHAIN_REPLAY": "5"}, "imagenet: HCONV_CHAIN_REPLAY")])
def test_cli_refusals(tmp_path, argv, env, msg):
    """bad arguments and switches end the commands like a Go panic (status 2) before they touch a device"""
    cli = os.path.join(ROOT, "optimal_conv_amd", "host", "conv")
    if not os.path.exists(cli):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([cli] + argv, cwd=tmp_path, capture_output=True, text=True, timeout=60, env=dict(os.environ, **env))
    assert r.returncode == 2 and msg in r.stderr, (argv, r.returncode, r.stderr[-300:])
    assert "CKKS parameters" not in r.stdout
