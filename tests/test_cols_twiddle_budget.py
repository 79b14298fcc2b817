"""The convolution's cols kernels hc_k_a2, hc_k_b2 and hc_k_b4 keep the colsB twiddles of their two transforms in wave-local LDS images (HcTwC in hc_kernels.h): 8 KiB beside the
16 KiB exchange tile. The images must not cost a kernel workgroups per CU, registers or scratch: checked without a GPU from hipcc's kernel-resource-usage remarks, as
tests/test_twiddle_stage_budget.py checks the rows kernels. For every instantiation of the three kernels: LDS per workgroup <= 24 KiB, no scratch, and
min(floor(160 KiB / LDS per workgroup), wavefronts per SIMD the allocated VGPRs allow) not below what the commit before the images had.

PARENT_WORKGROUPS_PER_CU was measured on that commit (36022c6) with the command this test runs,
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-value -Wno-unused-result --cuda-device-only -S -o /dev/null optimal_conv_amd/csrc/hconv.hip -Rpass-analysis=kernel-resource-usage
which gave 16384 bytes of LDS (10 by LDS) for all eight and, by VGPRs, hc_k_a2<1,1> 126, <2,1> 126, <1,0> 119, <2,0> 118, hc_k_b2<1> 121, <2> 110, hc_k_b4<1> 121, <2> 107: four
wavefronts per SIMD each. A 256-thread workgroup is one wavefront on each of a CU's four SIMDs, so workgroups per CU = wavefronts per SIMD."""
import os
import re
import subprocess

import pytest

from test_twiddle_stage_budget import HIPCC, LDS_PER_CU, ROOT, waves_by_vgprs

LDS_BUDGET = 24 * 1024
PARENT_WORKGROUPS_PER_CU = {
    "_Z7hc_k_a2ILi1ELi1EEv7HcLoopA7HcTwTabS1_": 4, "_Z7hc_k_a2ILi2ELi1EEv7HcLoopA7HcTwTabS1_": 4, "_Z7hc_k_a2ILi1ELi0EEv7HcLoopA7HcTwTabS1_": 4, "_Z7hc_k_a2ILi2ELi0EEv7HcLoopA7HcTwTabS1_": 4,
    "_Z7hc_k_b2ILi1EEv7HcLoopB7HcTwTabS1_": 4, "_Z7hc_k_b2ILi2EEv7HcLoopB7HcTwTabS1_": 4,
    "_Z7hc_k_b4ILi1EEv7HcLoopB7HcTwTabS1_": 4, "_Z7hc_k_b4ILi2EEv7HcLoopB7HcTwTabS1_": 4,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_cols_kernels_keep_their_workgroups_per_cu_with_the_twiddle_images():
    import __graft_entry__                # the flags the shipped libhconv.so is built with
    r = subprocess.run([HIPCC, *__graft_entry__.HIP_FLAGS, "--cuda-device-only", "-S", "-o", os.devnull,
                        os.path.join(ROOT, "optimal_conv_amd", "csrc", "hconv.hip"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        symbol = blk.split()[0]
        if not re.match(r"_Z7hc_k_(a2|b2|b4)I", symbol):
            continue
        fig = {key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1)) for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")}
        by_lds = LDS_PER_CU // fig["LDS Size [bytes/block]"]
        by_regs = waves_by_vgprs(fig["VGPRs"], fig["AGPRs"])
        print(f"{symbol}: {fig['VGPRs']} VGPRs + {fig['AGPRs']} AGPRs -> {by_regs}, {fig['LDS Size [bytes/block]']} bytes of LDS -> {by_lds}, scratch {fig['ScratchSize [bytes/lane]']}")
        seen.add(symbol)
        assert symbol in PARENT_WORKGROUPS_PER_CU, f"{symbol}: an instantiation this test has no parent figure for"
        assert fig["LDS Size [bytes/block]"] <= LDS_BUDGET, f"{symbol}: {fig['LDS Size [bytes/block]']} bytes of LDS per workgroup"
        assert fig["ScratchSize [bytes/lane]"] == 0, f"{symbol}: {fig['ScratchSize [bytes/lane]']} bytes of scratch per lane"
        assert min(by_lds, by_regs) >= PARENT_WORKGROUPS_PER_CU[symbol], f"{symbol}: {by_regs} by registers, {by_lds} by LDS, the parent had {PARENT_WORKGROUPS_PER_CU[symbol]}"
    assert seen == set(PARENT_WORKGROUPS_PER_CU), f"instantiations not found in the build: {sorted(set(PARENT_WORKGROUPS_PER_CU) - seen)}"
