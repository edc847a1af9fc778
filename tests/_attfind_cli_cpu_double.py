"""Launcher used by tests/test_attfind_newarch_cpu.py: the product's attfind_cli.main() with the CPU test double installed
as the op surface (a fresh interpreter has no GPU here).  The double is installed at import, so the ranks that
``--multi_gpus`` spawns — which import this file again, not as __main__ — run on it too."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd", "stylex")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

torch.set_num_threads(2)
import attfind_cli  # noqa: E402
import ops  # noqa: E402
from cpu_ops import CpuOracleOps  # noqa: E402

ops.use_impl(CpuOracleOps)
if __name__ == "__main__":
    attfind_cli.main()
