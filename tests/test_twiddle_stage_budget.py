"""The rows kernels of the convolution stage the A group of their twiddles through LDS (HcTwL in hc_kernels.h). The image must not cost a kernel the workgroups per CU it is
compiled for: checked without a GPU from hipcc's kernel-resource-usage remarks, as tests/test_kernel_resources.py checks scratch. For every instantiation of hc_k_a1p, hc_k_a3p,
hc_k_b1, hc_k_b3p and hc_k_b5m:  min(floor(160 KiB / LDS per workgroup), wavefronts per SIMD the allocated VGPRs allow)  >=  the kernel's HC_W_* / HC_B5M_WAVES value in
hc_kernels.h (3 for a1p and a3p, 4 for b1 and b3p, 2 for b5m). A 256-thread workgroup is one wavefront on each of a CU's four SIMDs, so workgroups per CU = wavefronts per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD_LANE = 512       # gfx950: one file for VGPRs and AGPRs, allocated in blocks of 8
KERNELS = {"hc_k_a1p": "HC_W_A1", "hc_k_a3p": "HC_W_A3", "hc_k_b1": "HC_W_B1", "hc_k_b3p": "HC_W_B3", "hc_k_b5m": "HC_B5M_WAVES"}


def waves_by_vgprs(vgprs, agprs):
    total = (vgprs + 3) // 4 * 4 + agprs if agprs else vgprs
    return min(8, VGPRS_PER_SIMD_LANE // max(8, (total + 7) // 8 * 8))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_staged_rows_kernels_keep_their_workgroups_per_cu():
    import __graft_entry__                # the flags the shipped libhconv.so is built with
    header = open(os.path.join(ROOT, "optimal_conv_amd", "csrc", "hc_kernels.h")).read()
    want = {k: int(re.search(r"#define %s (\d+)" % macro, header).group(1)) for k, macro in KERNELS.items()}
    r = subprocess.run([HIPCC, *__graft_entry__.HIP_FLAGS, "--cuda-device-only", "-S", "-o", os.devnull,
                        os.path.join(ROOT, "optimal_conv_amd", "csrc", "hconv.hip"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = set()
    for blk in blocks:
        symbol = blk.split()[0]
        kernel = next((k for k in KERNELS if symbol.startswith("_Z%d%s" % (len(k), k))), None)      # the mangled name carries the name's length: hc_k_b1 is not a prefix match
        if kernel is None:
            continue
        fig = {key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1)) for key in ("VGPRs", "AGPRs", "LDS Size [bytes/block]")}
        by_lds = LDS_PER_CU // fig["LDS Size [bytes/block]"]
        by_regs = waves_by_vgprs(fig["VGPRs"], fig["AGPRs"])
        print(f"{symbol}: {fig['VGPRs']} VGPRs + {fig['AGPRs']} AGPRs -> {by_regs}, {fig['LDS Size [bytes/block]']} bytes of LDS -> {by_lds}, wants {want[kernel]}")
        seen.add(kernel)
        assert min(by_lds, by_regs) >= want[kernel], f"{symbol}: {by_regs} by registers, {by_lds} by LDS, compiled for {want[kernel]}"
    assert seen == set(KERNELS), f"kernels not found in the build: {sorted(set(KERNELS) - seen)}"
