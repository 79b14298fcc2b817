"""hc_k_b5m runs through one 32 KiB LDS tile so that at least three of its workgroups fit a CU - four as committed (hc_kernels.h; profiles/LEDGER.md). Checked without a GPU from hipcc's
kernel-resource-usage remarks, as tests/test_twiddle_stage_budget.py parses them. For every instantiation of hc_k_b5m: at most 32 KiB of LDS per workgroup, no scratch,
min(floor(160 KiB / LDS per workgroup), wavefronts per SIMD the allocated VGPRs allow) >= HC_B5M_WAVES, and HC_B5M_WAVES itself at least 3. A 256-thread workgroup is one
wavefront on each of a CU's four SIMDs, so workgroups per CU = wavefronts per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD_LANE = 512       # gfx950: one file for VGPRs and AGPRs, allocated in blocks of 8
KERNEL = "hc_k_b5m"
INSTANTIATIONS = 2              # HC_FM_FREE (the benchmark's) and HC_FM_ALT


def waves_by_vgprs(vgprs, agprs):
    total = (vgprs + 3) // 4 * 4 + agprs if agprs else vgprs
    return min(8, VGPRS_PER_SIMD_LANE // max(8, (total + 7) // 8 * 8))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_b5m_fits_its_workgroups_per_cu():
    import __graft_entry__                # the flags the shipped libhconv.so is built with
    header = open(os.path.join(ROOT, "optimal_conv_amd", "csrc", "hc_kernels.h")).read()
    want = int(re.search(r"#define HC_B5M_WAVES (\d+)", header).group(1))
    assert want >= 3, f"HC_B5M_WAVES = {want}: the one-tile form ships for at least three workgroups per CU"
    r = subprocess.run([HIPCC, *__graft_entry__.HIP_FLAGS, "--cuda-device-only", "-S", "-o", os.devnull,
                        os.path.join(ROOT, "optimal_conv_amd", "csrc", "hconv.hip"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = 0
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        symbol = blk.split()[0]
        if not symbol.startswith("_Z%d%s" % (len(KERNEL), KERNEL)):
            continue
        fig = {key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1)) for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")}
        by_lds = LDS_PER_CU // fig["LDS Size [bytes/block]"]
        by_regs = waves_by_vgprs(fig["VGPRs"], fig["AGPRs"])
        print(f"{symbol}: {fig['VGPRs']} VGPRs + {fig['AGPRs']} AGPRs -> {by_regs}, {fig['LDS Size [bytes/block]']} bytes of LDS -> {by_lds}, scratch {fig['ScratchSize [bytes/lane]']}, wants {want}")
        seen += 1
        assert fig["LDS Size [bytes/block]"] <= 32 * 1024, f"{symbol}: {fig['LDS Size [bytes/block]']} bytes of LDS"
        assert fig["ScratchSize [bytes/lane]"] == 0, f"{symbol}: {fig['ScratchSize [bytes/lane]']} bytes of scratch per lane"
        assert min(by_lds, by_regs) >= want, f"{symbol}: {by_regs} by registers, {by_lds} by LDS, compiled for {want}"
    assert seen == INSTANTIATIONS, f"{seen} instantiations of {KERNEL} in the build, expected {INSTANTIATIONS}"
