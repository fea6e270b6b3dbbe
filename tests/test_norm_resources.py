"""What the compiler makes of the persistent exact-row LayerNorm backward kernels (csrc/pswin_norm.hip): the host sizes their grid for
four resident waves per SIMD and the row loop carries a whole row of requests in registers, so every instantiation must stay within
128 VGPRs without scratch.  Compiles pswin_norm.hip for gfx950 with the flags of build.py (device code only, no GPU needed, about a
minute) and reads the figures of -Rpass-analysis=kernel-resource-usage; nothing else of the assembly is looked at."""
import os
import re
import subprocess

from panoswintransformerobjectdetection_amd import build as pbuild

KERNELS = ("ln_bwd_rows_kernel", "ln_nchw_bwd_rows_kernel")
FIELDS = {"scratch": r"ScratchSize \[bytes/lane\]: (\d+)", "occupancy": r"Occupancy \[waves/SIMD\]: (\d+)",
          "sgpr_spill": r"SGPRs Spill: (\d+)", "vgpr_spill": r"VGPRs Spill: (\d+)"}


def _resource_usage(tmp_path):
    """mangled kernel name -> {scratch, occupancy, sgpr_spill, vgpr_spill} for every kernel of pswin_norm.hip"""
    cmd = [pbuild.HIPCC] + pbuild.FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                           os.path.join(pbuild.CSRC, "pswin_norm.hip"), "-o", str(tmp_path / "pswin_norm.s")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    usage = {}
    for block in p.stdout.split("remark: Function Name: ")[1:]:
        name = block.split()[0]
        usage[name] = {k: int(re.search(pat, block).group(1)) for k, pat in FIELDS.items()}
    return usage


def test_backward_row_kernels_need_no_scratch_and_keep_four_waves(tmp_path):
    usage = _resource_usage(tmp_path)
    for kernel in KERNELS:
        mine = {n: u for n, u in usage.items() if re.search(r"\d+%sI" % kernel, n)}      # Itanium: <length><name>I<template arguments>E
        assert len(mine) >= 4, (kernel, sorted(usage))
        for name, u in mine.items():
            assert u["scratch"] == 0, (name, u)
            assert u["sgpr_spill"] == 0 and u["vgpr_spill"] == 0, (name, u)
            assert u["occupancy"] >= 4, (name, u)
