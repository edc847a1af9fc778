"""Where the time of one Trainer.calculate_fid goes (stylex/fid.py): per batch of 256 px images, device time (hipEvents,
median of --rounds after warm-up, one process) of

* stylex_fid_prep, and the ATen composition it replaces (float / mul / add / clamp / floor / div / interpolate / mul / sub);
* the Inception-v3 forward with fused tails and slice writes, and the same module's plain ATen forward;
* stylex_fid_moments_acc, and the ATen composition it replaces (adaptive_avg_pool2d, cast to fp64, f^T f and the column sum);
* the host side once: mean / covariance from the moments and the two 2048 x 2048 eigendecompositions of frechet_distance;
* the JPEG round trip of the generated images (Trainer(fid_jpeg=True)): stylex_jpeg_roundtrip + stylex_fid_prep_u8 on the
  device, next to the host route it replaces — bytes to the host, Pillow save + open per image, upload, stylex_fid_prep_u8
  (wall time of one core, synchronised; the device route is also given as wall time for that comparison).

Totals are scaled to --images (default: calculate_fid_num_images = 12800) for reals + fakes.  Weights: random:1 (the time
does not depend on their values).

    python tools/bench_fid.py [--out profiles/fid_timing.txt] [--batch 64] [--rounds 10] [--images 12800]
    python tools/bench_fid.py --jpeg_only --append --out profiles/fid_timing.txt     (the JPEG rows alone, appended)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd")
for p in (ROOT, PKG, os.path.join(PKG, "stylex")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fid  # noqa: E402
import fid_inception  # noqa: E402
import hip_backend as hb  # noqa: E402


def device_ms(fn, rounds, warmup=2):
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


def wall_ms(fn, rounds, warmup=1):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def pillow_route(x, quality=75):
    """What the device round trip replaces: save_image's bytes to the host, Pillow's JPEG encoder and decoder per image (in
    memory, no disk), the decoded bytes back to the device."""
    import io

    import numpy as np
    from PIL import Image

    q = x[:, :3].float().mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    out = np.empty_like(q)
    for i in range(q.shape[0]):
        buf = io.BytesIO()
        Image.fromarray(q[i]).save(buf, format="JPEG", quality=quality)
        buf.seek(0)
        out[i] = np.asarray(Image.open(buf).convert("RGB"))
    return torch.from_numpy(out).to(x.device).permute(0, 3, 1, 2).contiguous()


def jpeg_rows(x, name, rounds, n_fake_batches):
    """Report lines of the JPEG round trip of one generated batch."""
    dev_ms = device_ms(lambda: hb.fid_prep_u8(hb.jpeg_roundtrip(x, 75)), rounds)
    rt_ms = device_ms(lambda: hb.jpeg_roundtrip(x, 75), rounds)
    dev_wall = wall_ms(lambda: hb.fid_prep_u8(hb.jpeg_roundtrip(x, 75)), rounds)
    host_wall = wall_ms(lambda: hb.fid_prep_u8(pillow_route(x, 75)), max(3, rounds // 3))
    same = bool(torch.equal(hb.jpeg_roundtrip(x, 75), pillow_route(x, 75)))
    fmt = "%-58s %9.3f ms/batch %10.2f s total"
    lines = ["# JPEG round trip of the generated batches (fid_jpeg), %s; total = %d batches (the fakes only); quality 75" % (name, n_fake_batches),
             fmt % ("JPEG round trip + prep_u8 kernels (device time)", dev_ms, dev_ms * n_fake_batches / 1e3),
             fmt % ("  of which the round trip (2 launches)", rt_ms, rt_ms * n_fake_batches / 1e3),
             fmt % ("JPEG round trip + prep_u8 kernels (wall, synchronised)", dev_wall, dev_wall * n_fake_batches / 1e3),
             fmt % ("host route: copy down, Pillow save + open, upload, prep_u8", host_wall, host_wall * n_fake_batches / 1e3),
             "# device route: %.4fx the wall time of the host route (%s); bytes equal to Pillow's on this batch: %s"
             % (dev_wall / host_wall, "faster" if dev_wall < host_wall else "NOT faster", same)]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--images", type=int, default=12800)
    ap.add_argument("--image_size", type=int, default=256)
    ap.add_argument("--jpeg_only", action="store_true", help="measure the JPEG round-trip rows alone")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = a.batch, a.image_size
    # the generator's output layout in the bf16 mode, and the loader's
    x_bf16 = torch.rand(B, 3, S, S, device=dev).bfloat16().contiguous(memory_format=torch.channels_last)
    x_f32 = torch.rand(B, 3, S, S, device=dev)
    # generated images are smooth, noise is the encoder's worst case: the timed batch is a blend of both
    yy, xx = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
    smooth = (0.5 + 0.4 * torch.sin(xx / 17.0 + yy / 29.0)).expand(B, 3, S, S)
    x_gen = (0.85 * smooth + 0.15 * x_f32).bfloat16().contiguous(memory_format=torch.channels_last)
    jpeg_lines = jpeg_rows(x_gen, "bf16 channels_last, %d images at %d px, %s" % (B, S, torch.cuda.get_device_name(0)), a.rounds,
                           -(-a.images // B))
    if a.jpeg_only:
        text = "\n".join(jpeg_lines) + "\n"
        print(text, end="")
        if a.out:
            with open(a.out, "a" if a.append else "w") as f:
                f.write(text)
        return
    net = fid_inception.build("random:1", dev)

    def aten_prep(x):
        q = x.float().mul(255).add(0.5).clamp(0, 255).floor() / 255
        return 2 * F.interpolate(q, size=(299, 299), mode="bilinear", align_corners=False) - 1

    rows = []
    for name, x in (("bf16 channels_last", x_bf16), ("fp32 NCHW", x_f32)):
        rows.append(("prep kernel, %s" % name, device_ms(lambda: hb.fid_prep(x), a.rounds)))
        rows.append(("prep ATen composition, %s" % name, device_ms(lambda: aten_prep(x), a.rounds)))
    inp = hb.fid_prep(x_f32)
    with torch.no_grad():
        rows.append(("Inception forward, fused tails + slice writes", device_ms(lambda: net(inp, plain=False), a.rounds)))
        rows.append(("Inception forward, plain ATen", device_ms(lambda: net(inp, plain=True), a.rounds)))
        fm = net(inp, plain=False)
    total = torch.zeros(2048, dtype=torch.float64, device=dev)
    gram = torch.zeros(2048, 2048, dtype=torch.float64, device=dev)

    def aten_moments():
        f = F.adaptive_avg_pool2d(fm, 1).flatten(1).double()
        gram.addmm_(f.T, f)
        total.add_(f.sum(0))

    rows.append(("moments kernel (pool + fp64 Gram)", device_ms(lambda: hb.fid_moments_acc(fm, total, gram), a.rounds)))
    rows.append(("moments ATen composition (pool, fp64 cast, addmm, sum)", device_ms(aten_moments, a.rounds)))

    st = fid.FIDStats(2048, dev)
    feats = torch.randn(4096, 2048, 1, 1, device=dev).abs()
    st.update(feats)
    torch.cuda.synchronize()
    t = time.perf_counter()
    mu, sigma = st.mean_cov()
    t_cov = time.perf_counter() - t
    t = time.perf_counter()
    fid.frechet_distance(mu, sigma, mu * 1.01, sigma * 1.02)
    t_fd = time.perf_counter() - t

    n_batches = 2 * -(-a.images // B)  # reals + fakes
    lines = ["# tools/bench_fid.py: device time per batch of %d images at %d px (median of %d), %s" % (B, S, a.rounds, torch.cuda.get_device_name(0)),
             "# total = scaled to 2 x %d images (reals + fakes, %d batches)" % (a.images, n_batches)]
    for name, ms in rows:
        lines.append("%-58s %9.3f ms/batch %10.2f s total" % (name, ms, ms * n_batches / 1e3))
    lines.append("%-58s %9.3f s   (host, once per set)" % ("mean / covariance from the moments (copy + fp64)", t_cov))
    lines.append("%-58s %9.3f s   (host, once)" % ("frechet_distance: eigh + eigvalsh at 2048 x 2048", t_fd))
    d = dict(rows)
    for new, old in (("prep kernel, bf16 channels_last", "prep ATen composition, bf16 channels_last"),
                     ("prep kernel, fp32 NCHW", "prep ATen composition, fp32 NCHW"),
                     ("moments kernel (pool + fp64 Gram)", "moments ATen composition (pool, fp64 cast, addmm, sum)"),
                     ("Inception forward, fused tails + slice writes", "Inception forward, plain ATen")):
        verdict = "faster" if d[new] < d[old] else "SLOWER"
        lines.append("# %s: %.2fx the time of what it replaces (%s)" % (new, d[new] / d[old], verdict))
    text = "\n".join(lines + jpeg_lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
