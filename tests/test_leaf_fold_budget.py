"""hc_k_b1x and hc_k_b5x (hc_kernels.h) are hc_k_b1 and hc_k_b5m without the product by the level's idx plaintext; they must keep the residency of the kernels they stand in
for. Checked without a GPU from hipcc's kernel-resource-usage remarks, as tests/test_b5m_budget.py parses them. hc_k_b1x: no scratch, five workgroups per CU as hc_k_b1 (94
VGPRs) has. Every instantiation of hc_k_b5x: no scratch, at most 32 KiB of LDS per workgroup, min(floor(160 KiB / LDS per workgroup), wavefronts per SIMD the allocated VGPRs
allow) >= HC_B5M_WAVES. A 256-thread workgroup is one wavefront on each of a CU's four SIMDs, so workgroups per CU = wavefronts per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD_LANE = 512       # gfx950: one file for VGPRs and AGPRs, allocated in blocks of 8
B1_WORKGROUPS = 5               # what hc_k_b1 gets
INSTANTIATIONS = {"hc_k_b1x": 1, "hc_k_b5x": 2}        # hc_k_b5x: HC_FM_FREE (the benchmark's) and HC_FM_ALT


def waves_by_vgprs(vgprs, agprs):
    total = (vgprs + 3) // 4 * 4 + agprs if agprs else vgprs
    return min(8, VGPRS_PER_SIMD_LANE // max(8, (total + 7) // 8 * 8))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_folded_leaf_kernels_fit_their_workgroups_per_cu():
    import __graft_entry__                # the flags the shipped libhconv.so is built with
    header = open(os.path.join(ROOT, "optimal_conv_amd", "csrc", "hc_kernels.h")).read()
    b5_want = int(re.search(r"#define HC_B5M_WAVES (\d+)", header).group(1))
    r = subprocess.run([HIPCC, *__graft_entry__.HIP_FLAGS, "--cuda-device-only", "-S", "-o", os.devnull,
                        os.path.join(ROOT, "optimal_conv_amd", "csrc", "hconv.hip"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = dict.fromkeys(INSTANTIATIONS, 0)
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        symbol = blk.split()[0]
        kernel = next((k for k in INSTANTIATIONS if symbol.startswith("_Z%d%s" % (len(k), k))), None)
        if kernel is None:
            continue
        fig = {key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1)) for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")}
        by_lds = LDS_PER_CU // fig["LDS Size [bytes/block]"]
        by_regs = waves_by_vgprs(fig["VGPRs"], fig["AGPRs"])
        want = B1_WORKGROUPS if kernel == "hc_k_b1x" else b5_want
        print(f"{symbol}: {fig['VGPRs']} VGPRs + {fig['AGPRs']} AGPRs -> {by_regs}, {fig['LDS Size [bytes/block]']} bytes of LDS -> {by_lds}, scratch {fig['ScratchSize [bytes/lane]']}, wants {want}")
        seen[kernel] += 1
        assert fig["ScratchSize [bytes/lane]"] == 0, f"{symbol}: {fig['ScratchSize [bytes/lane]']} bytes of scratch per lane"
        assert fig["LDS Size [bytes/block]"] <= 32 * 1024, f"{symbol}: {fig['LDS Size [bytes/block]']} bytes of LDS"
        assert min(by_lds, by_regs) >= want, f"{symbol}: {by_regs} by registers, {by_lds} by LDS, wants {want}"
    assert seen == INSTANTIATIONS, f"instantiations in the build: {seen}, expected {INSTANTIATIONS}"
