"""Fused attention core (csrc/linattn.hip) against the same formula on stock ATen ops (the composable path of
ops.linear_attention_core), on the same GPU, at the two config-2 shapes (B = 64; 128 x 128 and 64 x 64 pixels; 8 heads of
64 channels; bf16 NHWC).  Per-launch forward and forward + backward times, measured A/B/B/A inside one process so that
the A/A and B/B spreads are known; plus ChanNorm and the depthwise conv at the host widths, and (--step) one Trainer
step time at config 2 with attn_layers=[1, 2], fused vs composable.

    python tools/bench_attn.py [--iters 20] [--step] [--out profiles/attn_core_ab.txt]

Bytes: `algorithmic` = every operand read once and every result written once at the storage width; `moved` adds what the
kernels' structure moves on top of that (the fp32 chunk partials and their re-read, the saved pre-GELU tensor).  Both are
computed from the launch plan, not read from hardware counters.
"""
import argparse
import functools
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd", "stylex")]

import torch  # noqa: E402

import hip_backend as hb  # noqa: E402
import ops  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, iters):
    """median / min of `iters` single launches bracketed by events, after 3 warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def abba(make, iters):
    """make(fused) -> callable; returns {fused: [median of run 1, median of run 2]} in the order A B B A"""
    out = {True: [], False: []}
    for fused in (True, False, False, True):
        ops.set_attn_fused(fused)
        out[fused].append(timed(make(fused), iters)[0])
    ops.set_attn_fused(True)
    return out


def report(lines, label, res, alg_bytes=None, moved_bytes=None):
    a, b = res[True], res[False]
    spread = max(abs(a[0] - a[1]) / min(a), abs(b[0] - b[1]) / min(b))
    fa, fb = sum(a) / 2, sum(b) / 2
    line = "%-44s fused %8.3f %8.3f ms | ATen %8.3f %8.3f ms | ATen/fused %5.2fx | A/A, B/B spread %4.1f %%" % (
        label, a[0], a[1], b[0], b[1], fb / fa, 100 * spread)
    if alg_bytes:
        line += " | algorithmic %.2f GB (%.2f TB/s), moved %.2f GB (%.2f TB/s)" % (
            alg_bytes / 1e9, alg_bytes / fa / 1e9, moved_bytes / 1e9, moved_bytes / fa / 1e9)
    print(line, flush=True)
    lines.append(line)


def core_case(lines, b, side, iters):
    heads, n = 8, side * side
    gen = torch.Generator(device=DEV).manual_seed(side)
    cl = torch.channels_last
    q = (torch.randn(b, 512, side, side, device=DEV, generator=gen) * 2).bfloat16().contiguous(memory_format=cl)
    kv = (torch.randn(b, 1024, side, side, device=DEV, generator=gen) * 2).bfloat16().contiguous(memory_format=cl)
    r = torch.randn(b, 512, side, side, device=DEV, generator=gen).bfloat16().contiguous(memory_format=cl)
    k, v = kv.chunk(2, dim=1)
    nch = hb.load_library().stylex_linattn_chunks(hb._shape(b, n, heads))
    t = b * n * 512 * 2.0  # bytes of one bf16 [B, N, 512] tensor
    part = b * heads * nch * 64 * 64 * 4.0

    def fwd(fused):
        def run():
            with torch.no_grad():
                ops.linear_attention_core(q, k, v, heads)
        return run

    def fwd_bwd(fused):
        ql, kvl = q.clone().requires_grad_(), kv.clone().requires_grad_()

        def run():
            k_, v_ = kvl.chunk(2, dim=1)
            y = ops.linear_attention_core(ql, k_, v_, heads)
            torch.autograd.grad(y, [ql, kvl], r)
        return run

    ops.set_fast(True)
    tag = "core B=%d %dx%d (%d chunks)" % (b, side, side, nch)
    report(lines, tag + " forward", abba(fwd, iters), 4 * t, 5 * t + 2 * part)
    # backward: q, pre, gy, k, v read; dq, dk, dv written (+ the chunk's dC partials)
    report(lines, tag + " forward+backward", abba(fwd_bwd, iters), 4 * t + 8 * t, 5 * t + 2 * part + 8 * t + 2 * part)
    ops.set_fast(False)


def host_case(lines, b, c, side, iters):
    gen = torch.Generator(device=DEV).manual_seed(c)
    x = (torch.randn(b, c, side, side, device=DEV, generator=gen)).bfloat16().contiguous(memory_format=torch.channels_last)
    r = torch.randn_like(x)
    g = torch.ones(1, c, 1, 1, device=DEV).requires_grad_()
    bb = torch.zeros(1, c, 1, 1, device=DEV).requires_grad_()
    w = (torch.randn(c, 1, 3, 3, device=DEV, generator=gen) / 3).requires_grad_()
    t = x.numel() * 2.0
    ops.set_fast(True)

    def norm(fused):
        xl = x.clone().requires_grad_()

        def run():
            torch.autograd.grad(ops.chan_norm(xl, g, bb), [xl, g, bb], r)
        return run

    def dw(fused):
        xl = x.clone().requires_grad_()

        def run():
            torch.autograd.grad(ops.depthwise_conv3x3(xl, w), [xl, w], r)
        return run

    report(lines, "ChanNorm B=%d C=%d %dx%d forward+backward" % (b, c, side, side), abba(norm, iters), 5 * t, 5 * t)
    # the composable depthwise path is F.conv2d(groups=C); the product always takes the kernels on the GPU
    report(lines, "depthwise B=%d C=%d %dx%d forward+backward" % (b, c, side, side), abba(dw, iters), 6 * t, 6 * t)
    ops.set_fast(False)


def step_times(lines, steps):
    """One Trainer.train() at config 2 (256 px, batch 32, GAE 2, bf16) with attn_layers=[1, 2]: mean over `steps` calls
    after 3 warm-up calls, fused vs composable, A/B/B/A with a fresh Trainer each."""
    import time

    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    import stylex_train as st

    a = argparse.Namespace(batch=32, image_size=256, gae=2, classifier="resnet", pl_every=32, workdir="/tmp/sb_attn",
                           precision="bf16", device_rng=0, graphs=0)
    plain = st.Trainer
    res = {True: [], False: []}
    try:
        st.Trainer = functools.partial(plain, attn_layers=[1, 2])
        for fused in (True, False, False, True):
            ops.set_attn_fused(fused)
            tr = bench.build_trainer(a, DEV, 0, 1)
            for _ in range(3):
                tr.train()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train()
            torch.cuda.synchronize()
            res[fused].append((time.perf_counter() - t0) / steps * 1e3)
            del tr
            torch.cuda.empty_cache()
    finally:
        st.Trainer = plain
        ops.set_attn_fused(True)
    report(lines, "train() 256 px B=32 GAE=2 attn_layers=[1,2], %d calls" % steps, res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--step", type=int, default=0, help="also time this many Trainer.train() calls per variant")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    hb.load_library()
    ops.set_precision("bf16")
    lines = ["# tools/bench_attn.py --iters %d --batch %d: medians of single launches, order fused / ATen / ATen / fused"
             % (args.iters, args.batch), "# %s" % torch.cuda.get_device_name(0)]
    for side in (128, 64):
        core_case(lines, args.batch, side, args.iters)
    host_case(lines, args.batch, 64, 128, args.iters)
    host_case(lines, args.batch, 128, 64, args.iters)
    if args.step:
        step_times(lines, args.step)
    ops.set_precision("fp32")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
