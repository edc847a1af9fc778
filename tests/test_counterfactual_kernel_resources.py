"""Build hygiene of the counterfactual edit kernel (csrc/style_edit.hip): no scratch memory and no spilled VGPRs — one value
per thread, the edit list in LDS.  Same hipcc remarks and parsing as tests/test_variants_kernel_resources.py; the per-file
flags come from csrc/Makefile."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import _makefile_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_style_edit_kernel_uses_no_scratch(tmp_path):
    source, kernels = "style_edit.hip", ["style_edit_levels_kernel"]
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function"]
                         + _makefile_flags(source[:-4]) + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source),
                                                           "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
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
    for k in kernels:
        hits = {n: v for n, v in seen.items() if k in n}
        assert hits, (k, sorted(seen))
        for n, (scratch, spill) in hits.items():
            assert scratch == 0 and spill == 0, (n, "scratch bytes/lane", scratch, "spilled VGPRs", spill)
