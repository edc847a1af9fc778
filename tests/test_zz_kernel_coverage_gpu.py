"""-m gpu, runs LAST in the suite (file name): every conv kernel instantiation that one benchmark step at BASELINE config 2
launches must also have been launched by a test that compares results with a definition (tests marked `against_definition`,
collected by tests/conftest.py).  Round-5 VERDICT weak 1 / 3: a selector threshold (`wg_np64`: >= 48 stages per block) sent
the benchmark's largest weight-gradient launches to a tile that no parity shape reached.
When the rows of tests/test_conv_exact_gpu.py ran in the session, every (class, instantiation) of the step must also have been
launched by a row that passed there, i.e. compared BIT FOR BIT with its definition (EXACT_KERNELS)."""
import argparse
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import conftest  # noqa: E402
import hip_backend as hb  # noqa: E402
import ops  # noqa: E402
import test_conv_exact_gpu as exact  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bench_step_kernels(tmp_path, image_size=256, batch=32, gae=2, calls=4):
    """Kernel names (cls, name) -> launches of `calls` train() calls of the benchmark's Trainer, from step 0 (call 0 carries
    the gradient penalty), in the benchmarked bf16 mode; stream concurrency off as in bench.py's instrumented steps."""
    import bench

    prev = os.environ.get("STYLEX_STREAMS")
    os.environ["STYLEX_STREAMS"] = "0"
    ops.set_precision("bf16")
    try:
        hb.pack_cache_clear()
        a = argparse.Namespace(batch=batch, image_size=image_size, gae=gae, classifier="resnet", workdir=str(tmp_path), precision="bf16")
        bench.seed_all(42)
        tr = bench.build_trainer(a, torch.device("cuda:0"), 0, 1)
        tr.graphs = False
        tr.train()
        torch.cuda.synchronize()
        tr.steps = 0
        hb.timing_enable(1)
        for _ in range(calls):
            tr.train()
        torch.cuda.synchronize()
        rows = hb.timing_kernels()
        hb.timing_enable(0)
        del tr
        torch.cuda.empty_cache()
    finally:
        ops.set_precision("fp32")
        if prev is None:
            os.environ.pop("STYLEX_STREAMS", None)
        else:
            os.environ["STYLEX_STREAMS"] = prev
    return {(r["cls"], r["kernel"]): r["launches"] for r in rows if r["kernel"]}


def test_bench_step_launches_only_kernels_the_parity_tests_launched(tmp_path):
    if len(conftest.DEFINITION_TESTS_RUN) < 100:
        pytest.skip("needs the definition-comparing tests of the same session (run the whole `-m gpu` suite): %d ran"
                    % len(conftest.DEFINITION_TESTS_RUN))
    launched = bench_step_kernels(tmp_path)
    assert len(launched) >= 20, launched
    names = {k for _, k in launched}
    missing = sorted(names - set(conftest.KERNELS_CHECKED))
    exact_ran = len(exact.EXACT_KERNELS) >= 20  # the exact table ran in this session (its rows fill the mapping as they pass)
    convs = {ck for ck in launched if ck[1].startswith("conv")}  # (the table is about the conv kernels: to-RGB, losses etc. name no class)
    missing_exact = sorted(convs - set(exact.EXACT_KERNELS)) if exact_ran else []
    out = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(out):  # record for the round's profiles/ (the GPU box merges gpurun_out/ back)
        with open(os.path.join(out, "kernel_coverage.txt"), "w") as f:
            f.write("# conv kernel instantiations of 4 train() calls at config 2 (bf16, B = 32, GAE 2, 256 px): launches, and the\n"
                    "# number of definition-comparing tests of this session that launched the same instantiation; exact tests: the rows\n"
                    "# of tests/test_conv_exact_gpu.py that launched it in the same class and matched their definition bit for bit\n")
            for (cls, k), n in sorted(launched.items(), key=lambda kv: (kv[0][1], kv[0][0])):
                f.write("%-11s %5d launches  %3d tests  %3d exact tests  %s\n" % (cls, n, len(conftest.KERNELS_CHECKED.get(k, ())),
                                                                                  len(exact.EXACT_KERNELS.get((cls, k), ())), k))
            f.write("# checked by tests but not launched by the step:\n")
            for k in sorted(set(conftest.KERNELS_CHECKED) - names):
                f.write("#   %s\n" % k)
    assert not missing, "kernel instantiations the benchmark step launches that no definition-comparing test launched: %s" % missing
    assert not missing_exact, "(class, conv instantiation) pairs of the benchmark step that no row of the exact table launched: %s" % missing_exact
