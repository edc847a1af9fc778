"""Time of the image-pair statistics of one batch (hip_backend.image_pair_stats, csrc/image_metrics.hip) next to the torch
composition it replaces, on the same GPU: device time (hipEvents, median of --rounds after warm-up, one process) at 64 px and
256 px, B = 32, for the two operand forms a reconstruction report meets — dense fp32 against dense fp32, and dense fp32
against bf16 channels-last (the generator's output in the bf16 mode).

The composition: the value rule (mul / add / clamp / floor / div), |d| and d^2 sums, and SSIM as one grouped F.conv2d with
the 11 x 11 Gaussian window over the five maps x, y, x^2, y^2, xy (15 planes), the quotient and the mean — about ten
intermediate maps.  The kernel's rate is given as the bytes it has to read (both operands once) over its time, against the
achievable HBM rate of 6.3 TB/s; at these sizes the batch fits the caches, so that share says how far the kernel is from a
pure stream, not where the bytes came from.  The two routes' SSIM are compared on the timed batch.

    python tools/bench_recon.py [--out profiles/recon_timing.txt] [--batch 32] [--rounds 20]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd")
for p in (ROOT, PKG, os.path.join(PKG, "stylex")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hip_backend as hb  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # achievable (float4 copy), of 8 TB/s peak


def device_ms(fn, rounds, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def window(device):
    d = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-d * d / (2 * 1.5 ** 2))
    g = g / g.sum()
    return torch.outer(g, g).float().to(device)


def torch_composition(x, y, w2, quantise=True):
    """[B, 4] per image: sum |d|, sum d^2 (of bytes with quantise), mean SSIM — the passes the kernel fuses."""
    x, y = x.float(), y.float()
    if quantise:
        bx, by = x.mul(255).add(0.5).clamp(0, 255).floor(), y.mul(255).add(0.5).clamp(0, 255).floor()
        vx, vy = bx / 255, by / 255
    else:
        bx, by = x.clamp(0, 1), y.clamp(0, 1)
        vx, vy = bx, by
    d = bx - by
    c = x.shape[1]
    maps = torch.cat((vx, vy, vx * vx, vy * vy, vx * vy), dim=1)
    m = F.conv2d(maps, w2.expand(5 * c, 1, 11, 11), groups=5 * c)
    mx, my, exx, eyy, exy = m.split(c, dim=1)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    ssim = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    return torch.stack((d.abs().double().sum((1, 2, 3)), (d * d).double().sum((1, 2, 3)), ssim.double().mean((1, 2, 3))), dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_recon.py measures on the GPU; there is none here (speed not measured)")
    dev = torch.device("cuda:0")
    w2 = window(dev)
    B = a.batch
    lines = ["# tools/bench_recon.py: device time per batch of %d image pairs, 3 channels, quantise = 1 (median of %d), %s"
             % (B, a.rounds, torch.cuda.get_device_name(0)),
             "# rate = bytes of both operands, read once, over the kernel's time; share of the achievable HBM rate (%.1f TB/s)"
             % (HBM_BYTES_PER_S / 1e12)]
    for S in (64, 256):
        g = torch.Generator().manual_seed(S)
        x = torch.rand(B, 3, S, S, generator=g).to(dev)
        y32 = (x + 0.05 * torch.randn(B, 3, S, S, generator=g).to(dev)).contiguous()
        for name, y in (("fp32 / fp32", y32), ("fp32 / bf16 channels_last", y32.bfloat16().contiguous(memory_format=torch.channels_last))):
            k_ms = device_ms(lambda: hb.image_pair_sums(x, y, 3, True), a.rounds)
            t_ms = device_ms(lambda: torch_composition(x, y, w2, True), a.rounds)
            nbytes = x.numel() * x.element_size() + y.numel() * y.element_size()
            rate = nbytes / (k_ms * 1e-3)
            got = hb.image_pair_stats(x, y, 3, True).ssim
            ref = torch_composition(x, y, w2, True)[:, 2]
            lines.append("%3d px %-26s kernel (2 launches) %8.4f ms   torch composition %8.4f ms   %6.2fx   %8.1f GB/s = %5.2f %% of HBM"
                         "   max |SSIM difference| %.2g"
                         % (S, name, k_ms, t_ms, t_ms / k_ms, rate / 1e9, 100 * rate / HBM_BYTES_PER_S, float((got - ref).abs().max())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
