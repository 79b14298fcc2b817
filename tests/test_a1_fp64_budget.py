"""hc_k_a1p and hc_k_a1g with the fp64 product on 8-byte c' operands (hc_f64_mulmod_q): no instantiation may spill, pass 32 KiB of LDS or lose a workgroup per CU. Checked
without a GPU from hipcc's kernel-resource-usage remarks, with the command tests/test_cols_twiddle_budget.py runs. For hc_k_a1p<0>, <1> and hc_k_a1g<0>, <1>: no scratch,
LDS per workgroup <= 32 KiB, and min(floor(160 KiB / LDS per workgroup), wavefronts per SIMD the allocated VGPRs allow) >= 3 (HC_W_A1 = 3: the four-workgroup build of
hc_k_a1p<1> needs 44 bytes of scratch per lane and was not taken, profiles/LEDGER.md)."""
import os
import re
import subprocess

import pytest

from test_twiddle_stage_budget import HIPCC, LDS_PER_CU, ROOT, waves_by_vgprs

LDS_BUDGET = 32 * 1024
WORKGROUPS_PER_CU = 3
INSTANTIATIONS = {"_Z8hc_k_a1pILi0E", "_Z8hc_k_a1pILi1E", "_Z8hc_k_a1gILi0E", "_Z8hc_k_a1gILi1E"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_a1_kernels_keep_their_workgroups_per_cu_without_scratch():
    import __graft_entry__                # the flags the shipped libhconv.so is built with
    r = subprocess.run([HIPCC, *__graft_entry__.HIP_FLAGS, "--cuda-device-only", "-S", "-o", os.devnull,
                        os.path.join(ROOT, "optimal_conv_amd", "csrc", "hconv.hip"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = set()
    for blk in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        symbol = blk.split()[0]
        m = re.match(r"_Z8hc_k_a1[pg]ILi\dE", symbol)
        if not m:
            continue
        fig = {key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1)) for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")}
        by_lds = LDS_PER_CU // fig["LDS Size [bytes/block]"]
        by_regs = waves_by_vgprs(fig["VGPRs"], fig["AGPRs"])
        print(f"{symbol}: {fig['VGPRs']} VGPRs + {fig['AGPRs']} AGPRs -> {by_regs}, {fig['LDS Size [bytes/block]']} bytes of LDS -> {by_lds}, scratch {fig['ScratchSize [bytes/lane]']}")
        seen.add(m.group(0))
        assert fig["ScratchSize [bytes/lane]"] == 0, f"{symbol}: {fig['ScratchSize [bytes/lane]']} bytes of scratch per lane"
        assert fig["LDS Size [bytes/block]"] <= LDS_BUDGET, f"{symbol}: {fig['LDS Size [bytes/block]']} bytes of LDS per workgroup"
        assert min(by_lds, by_regs) >= WORKGROUPS_PER_CU, f"{symbol}: {by_regs} workgroups per CU by registers, {by_lds} by LDS"
    assert seen == INSTANTIATIONS, f"instantiations not found in the build: {sorted(INSTANTIATIONS - seen)}; unexpected: {sorted(seen - INSTANTIATIONS)}"
