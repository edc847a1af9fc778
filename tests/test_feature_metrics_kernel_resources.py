"""Build hygiene of the pairwise feature-metric kernels (csrc/feature_metrics.hip): no scratch memory and no spilled VGPRs in
any of them — the pair kernel keeps its 16 x 16 fp64 tile, the k-th-smallest kernel its eight-entry sorted list in
registers.  Compiled with the Makefile's flags for this file; same hipcc remarks and parsing as
tests/test_fid_kernel_resources.py."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

KERNELS = ["rownorm_f64_kernel", "pair_f64_kernelILi0", "pair_f64_kernelILi1", "sum_f64_kernel", "row_kth_smallest_kernel",
           "col_any_within_kernel"]


def _makefile_flags(stem):
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"CXXFLAGS_%s\s*=\s*(.*)" % re.escape(stem), line)
        if m:
            return m.group(1).split()
    return []


def test_the_makefile_builds_the_file_without_the_slp_vectoriser():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "feature_metrics.hip" in re.search(r"^SRCS\s*=(.*)$", text, re.M).group(1).split()
    assert _makefile_flags("feature_metrics") == ["-fno-slp-vectorize"]


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_feature_metric_kernels_use_no_scratch(tmp_path):
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function"]
                         + _makefile_flags("feature_metrics")
                         + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "feature_metrics.hip"),
                            "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk)
        spill = re.search(r"VGPRs Spill: (\d+)", blk)
        vgprs = re.search(r" VGPRs: (\d+)", blk)
        seen[name] = (int(scratch.group(1)) if scratch else None, int(spill.group(1)) if spill else None)
        print(name, "VGPRs", vgprs.group(1) if vgprs else "?", "scratch", seen[name][0])
    for k in KERNELS:
        hits = {n: v for n, v in seen.items() if k in n}
        assert hits, (k, sorted(seen))
        for n, (scratch, spill) in hits.items():
            assert scratch == 0 and spill == 0, (n, "scratch bytes/lane", scratch, "spilled VGPRs", spill)
