"""Times KID (100 subsets of 1000) and precision / recall at N = M = 12800, D = 2048 on random features: the fp64 pairwise
kernels of csrc/feature_metrics.hip (fid.kid, fid.precision_recall) against the torch fp64 composition on the same device
in the same run — torch.mm in fp64 for the polynomial kernel, torch.cdist and topk in row blocks of the same size for the
radii and the membership passes.  Order A / B / B / A (A = kernels, B = composition), wall time with a synchronise around
each pass, after one untimed pass of each.  Writes profiles/feature_metrics_timing.txt (or --out).

    python tools/bench_feature_metrics.py [--n 12800] [--d 2048] [--out profiles/feature_metrics_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd")
for p in (PKG, os.path.join(PKG, "stylex")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fid  # noqa: E402


def torch_kid(fx, fy, subsets):
    d, vals = fx.shape[1], []
    for ix, iy in subsets:
        x = fx.index_select(0, torch.from_numpy(ix).to(fx.device)).double()
        y = fy.index_select(0, torch.from_numpy(iy).to(fy.device)).double()
        s = len(ix)
        kxx, kyy, kxy = (torch.mm(x, x.T) / d + 1) ** 3, (torch.mm(y, y.T) / d + 1) ** 3, (torch.mm(x, y.T) / d + 1) ** 3
        vals.append((kxx.sum() - kxx.diagonal().sum() + kyy.sum() - kyy.diagonal().sum()) / (s * (s - 1)) - 2 * kxy.sum() / (s * s))
    v = torch.stack(vals).cpu().numpy()
    return float(v.mean()), float(v.std())


def torch_precision_recall(fr, ff, k=3, row_block=1024):
    fr, ff = fr.double(), ff.double()

    def radii(f):
        out = []
        for r0 in range(0, f.shape[0], row_block):
            blk = torch.cdist(f[r0:r0 + row_block], f)
            out.append(blk.topk(k + 1, dim=1, largest=False).values[:, k])  # the point itself is the nearest
        return torch.cat(out)

    def inside(ref, r, q):
        flags = torch.zeros(q.shape[0], dtype=torch.bool, device=q.device)
        for r0 in range(0, ref.shape[0], row_block):
            flags |= (torch.cdist(ref[r0:r0 + row_block], q) <= r[r0:r0 + row_block, None]).any(0)
        return flags

    p, r = inside(fr, radii(fr), ff), inside(ff, radii(ff), fr)
    return float(p.double().mean().cpu()), float(r.double().mean().cpu())


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def abba(a, b):
    a(), b()  # untimed: allocator, library initialisation, code objects
    ta1, ra = timed(a)
    tb1, rb = timed(b)
    tb2, _ = timed(b)
    ta2, _ = timed(a)
    return (ta1, ta2), (tb1, tb2), ra, rb


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=12800)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feature_metrics_timing.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    fr = torch.rand(a.n, a.d, generator=g).to(dev)
    ff = (torch.rand(a.n, a.d, generator=g) * 1.05).to(dev)
    subsets = fid.kid_subsets(a.n, a.n, 100, 1000, 0)
    lines = ["# tools/bench_feature_metrics.py: N = M = %d, D = %d, uniform random features, %s; wall seconds per pass,"
             % (a.n, a.d, torch.cuda.get_device_name(0)),
             "# order kernels / composition / composition / kernels after one untimed pass of each"]
    for name, ours, theirs in (("KID, 100 subsets of %d" % min(a.n, 1000), lambda: fid.kid(fr, ff, subsets=subsets), lambda: torch_kid(fr, ff, subsets)),
                               ("precision / recall, k = 3, row blocks of 1024", lambda: fid.precision_recall(fr, ff),
                                lambda: torch_precision_recall(fr, ff))):
        ta, tb, ra, rb = abba(ours, theirs)
        ratio = np.mean(ta) / np.mean(tb)
        lines += ["%-48s fp64 pairwise kernels   %.3f s, %.3f s   -> %s" % (name, ta[0], ta[1], ra),
                  "%-48s torch fp64 composition  %.3f s, %.3f s   -> %s" % ("", tb[0], tb[1], rb),
                  "# %s: %.2fx the time of the torch composition (%s)" % (name.split(",")[0], ratio, "faster" if ratio < 1 else "slower")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
