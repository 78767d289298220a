# -*- coding: utf-8 -*-
"""Register guard for flag_step_kernel (csrc/flag_step.hip) on the shipped code objects: no GPU, no recompilation."""
import re

from test_abi import _shipped_kernel_registers

NETS, GROUPS, NTU = (0, 1), (8, 16, 32, 64), (0, 1, 3)  # Linear / FM; lanes per row: D = 32, 64, 128, 256; K1_NT


def test_flag_step_kernels_fit_three_waves_per_simd(tmp_path):
    """The kernel is launched two workgroups per CU and its resident cap is (occupancy - 1) per CU: at most 168 VGPRs
    (three waves per SIMD) keep that at two — above, c4's 512-workgroup grid would fall back to two launches without a
    word.  No scratch.  All 2 nets x 4 row shapes x 3 NTU = 24 instances are in the library, and no other."""
    found = _shipped_kernel_registers(tmp_path)
    seen = {n: v for n, v in found.items() if re.search(r"\d+flag_step_kernelI", n)}
    want = {f"flag_step_kernelILi{net}ELi{g}ELi{ntu}EE" for net in NETS for g in GROUPS for ntu in NTU}
    got = {re.search(r"flag_step_kernelI(?:Li\d+E){3}E", n).group(0) for n in seen}
    assert got == want and len(seen) == 24, sorted(seen)
    for n, (vgpr, scratch) in seen.items():
        assert scratch == 0 and vgpr <= 168, (n, vgpr, scratch)
