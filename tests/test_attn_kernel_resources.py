"""Build hygiene of the linear-attention kernels (csrc/linattn.hip): no scratch memory and no spilled VGPRs in any of
them — the attention-core passes keep a 4x4 or 2x4 accumulator patch (and, in the depthwise weight gradient, 36 sums)
per thread in registers.  Same hipcc remarks and parsing as tests/test_kernel_resources.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = ["linattn_ctx_partialILb0", "linattn_ctx_partialILb1", "linattn_ctx_combine", "linattn_outILb0", "linattn_outILb1",
           "linattn_bwd_qILb0", "linattn_bwd_qILb1", "linattn_dctx_combine", "linattn_bwd_kvILb0", "linattn_bwd_kvILb1",
           "chan_norm_fwd_kernelILb0", "chan_norm_fwd_kernelILb1", "chan_norm_bwd_kernelILb0", "chan_norm_bwd_kernelILb1",
           "dwconv3x3_kernelILb0", "dwconv3x3_kernelILb1", "dwconv3x3_wgrad_kernelILb0", "dwconv3x3_wgrad_kernelILb1",
           "reduce_slices_kernel"]


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_attention_kernels_use_no_scratch(tmp_path):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "linattn.hip"), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk)
        spill = re.search(r"VGPRs Spill: (\d+)", blk)
        vgprs = re.search(r" VGPRs: (\d+)", blk)
        lds = re.search(r"LDS Size \[bytes/block\]: (\d+)", blk)
        seen[name] = (int(scratch.group(1)) if scratch else None, int(spill.group(1)) if spill else None)
        print(name, "VGPRs", vgprs.group(1) if vgprs else "?", "LDS", lds.group(1) if lds else "?", "scratch", seen[name][0])
    for k in KERNELS:
        hits = {n: v for n, v in seen.items() if k in n}
        assert hits, (k, sorted(seen))
        for n, (scratch, spill) in hits.items():
            assert scratch == 0 and spill == 0, (n, "scratch bytes/lane", scratch, "spilled VGPRs", spill)
