"""Counterfactual experiment timing (record only): the top-K sweep of attfind.counterfactual_images on one MI355X against the
structure of the reference's stylex/FID_TensorFlow.ipynb (cell 20: batch 1, the whole generator per image and level, style
biases mutated in place), and the edit kernel against its torch composition.  Seeded random model, classifier (ResNet-18)
and latents; the K edited coordinates are drawn over the whole style vector (their blocks are printed: prefix sharing
saves the blocks in front of the first edited one).  Host clock around work that ends in a device synchronise; every
variant is warmed up on the shapes it times.

    python tools/bench_counterfactual.py [--sizes 64 256] [--images 250] [--k 10] [--image_batch 32] [--precision fp32]
        [--notebook_images N]   (variant (a) on the first N images only; its totals are then marked as scaled)
        [--out profiles/counterfactual_timing.txt] [--errors_out profiles/counterfactual_errors.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd")
sys.path[:0] = [os.path.join(PKG, "stylex"), PKG, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import attfind  # noqa: E402
import hip_backend as hb  # noqa: E402
import ops  # noqa: E402
import stylex_train as st  # noqa: E402
from resnet_classifier import ResNet  # noqa: E402


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


@torch.no_grad()
def notebook_structure(G, clf, latents, noise, edits, smin, smax, k, shift):
    """Cell 20 for one level with the parent commit's public modules: per latent the base pass and its class, k bias
    mutations (the style vector recomputed before each), one generator pass at batch 1, the biases restored."""
    flips = 0
    for w in latents:
        w = w[None]
        w_tensor = attfind.styles_def_to_tensor([(w, G.num_layers)])
        base = clf.classify_images(G(w_tensor, noise)).argmax(dim=-1)
        flip = int(base) == 0
        undo = []
        for d, s in edits[:k]:
            li, j = attfind._block_of(G, s)
            block = G.blocks[li]
            lin, j = (block.to_style1, j) if j < block.input_channels else (block.to_style2, j - block.input_channels)
            cur = lin(w)[0, j]
            target = smin[s] if (d == 0) != flip else smax[s]
            delta = (target - cur) * shift
            lin.bias[j] += delta
            undo.append((lin, j, delta))
        flips += int(clf.classify_images(G(w_tensor, noise)).argmax(dim=-1) != base)
        for lin, j, delta in undo:
            lin.bias[j] -= delta
    return flips


@torch.no_grad()
def engine(G, clf, latents, noise, edits, smin, smax, k, shift, image_batch, share, per_level=None):
    flips, base = torch.zeros(k, dtype=torch.int64, device=latents.device), None
    t = time.perf_counter()
    for lv, _, logits in attfind.counterfactual_images(G, clf, latents.cpu().numpy(), edits[:k], smin, smax, noise,
                                                       list(range(k + 1)), shift_size=shift, image_batch=image_batch,
                                                       share_prefix=share):
        if lv == 0:
            base = logits.argmax(dim=-1)
        else:
            flips[lv - 1] += (logits.argmax(dim=-1) != base).sum()
        if per_level is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            per_level[lv] += now - t
            t = now
    return flips.tolist()


def run_size(size, a, lines, err_lines):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = st.StylEx(size, rank=0).eval()
    G = m.G
    clf = ResNet(None, 0, output_size=2, image_size=size)
    noise = st.image_noise(1, size, dev)
    with torch.no_grad():
        lat, coords = [], []
        for lo in range(0, a.images, a.image_batch):
            imgs = torch.rand(min(a.image_batch, a.images - lo), 3, size, size, device=dev)
            w = torch.cat((m.encoder(imgs).reshape(imgs.shape[0], -1), clf.classify_images(imgs)), dim=1)
            lat.append(w)
            coords.append(G(attfind.styles_def_to_tensor([(w, G.num_layers)]), noise.expand(w.shape[0], -1, -1, -1),
                            get_style_coords=True)[1].float())
    latents, coords = torch.cat(lat), torch.cat(coords)
    smin, smax = coords.min(dim=0)[0], coords.max(dim=0)[0]
    n_coords = coords.shape[1]
    rng = np.random.RandomState(1)
    edits = [(int(rng.randint(2)), int(c)) for c in rng.choice(n_coords, a.k, replace=False)]
    blocks = [attfind._block_of(G, s)[0] for _, s in edits]
    lines.append("== %d px, %d images, K = %d, %s, image_batch %d, %d style coordinates; blocks of the edits (list order): %s"
                 % (size, a.images, a.k, a.precision, a.image_batch, n_coords, blocks))

    # (a) the notebook's structure
    n_nb = min(a.notebook_images or a.images, a.images)
    notebook_structure(G, clf, latents[:2], noise, edits, smin, smax, a.k, a.shift)  # warm-up
    t_a = [clock(lambda k=k: notebook_structure(G, clf, latents[:n_nb], noise, edits, smin, smax, k, a.shift))[0]
           for k in range(1, a.k + 1)]
    scale = a.images / n_nb
    lines.append("(a) notebook structure, batch 1, whole generator, measured on %d images%s: per level [s] %s total %.2f s"
                 % (n_nb, "" if n_nb == a.images else " and SCALED by %.1f to %d" % (scale, a.images),
                    " ".join("%.2f" % (t * scale) for t in t_a), sum(t_a) * scale))
    for tag, share in (("(b) engine, share_prefix=False", False), ("(c) engine, share_prefix=True", True)):
        engine(G, clf, latents[:a.image_batch + 1], noise, edits, smin, smax, a.k, a.shift, a.image_batch, share)  # warm-up
        total = min(clock(lambda: engine(G, clf, latents, noise, edits, smin, smax, a.k, a.shift, a.image_batch, share))[0]
                    for _ in range(a.repeats))
        per = [0.0] * (a.k + 1)
        clock(lambda: engine(G, clf, latents, noise, edits, smin, smax, a.k, a.shift, a.image_batch, share, per))
        lines.append("%s: base pass %.3f s, per level [s] %s (a synchronise after every level); total without them %.3f s "
                     "(best of %d)" % (tag, per[0], " ".join("%.3f" % t for t in per[1:]), total, a.repeats))

    # the edit kernel against its torch composition, one image batch, all K + 1 levels
    seg = attfind.style_segments(G)
    cb = coords[:a.image_batch].contiguous()
    base = torch.randint(0, 2, (cb.shape[0],), device=dev, dtype=torch.int32)
    levels = list(range(a.k + 1))
    call = {"kernel": lambda: attfind.edited_styles(cb, edits, smin, smax, base, levels, seg, a.shift),
            "torch composition": lambda: attfind.edited_styles_composition(cb, edits, smin, smax, base, levels, seg, a.shift)}
    for name, fn in call.items():
        fn()
        dt = min(clock(lambda: [fn() for _ in range(50)])[0] for _ in range(3)) / 50
        lines.append("edited styles of %d images, %d levels, %s: %.1f us per call (host clock, 50 calls per synchronise)"
                     % (cb.shape[0], len(levels), name, dt * 1e6))
    same = all(torch.equal(x, y) for x, y in zip(call["kernel"](), call["torch composition"]()))
    lines.append("kernel == torch composition bit for bit: %s" % same)

    if size == a.sizes[0]:  # engine against the definition (tests/_counterfactual_defs.py) on a few images
        from _counterfactual_defs import edit_levels, naive_images

        n_err = min(8, a.images)
        got = {}
        with torch.no_grad():
            bc = clf.classify_images(G(attfind.styles_def_to_tensor([(latents[:n_err], G.num_layers)]),
                                       noise.expand(n_err, -1, -1, -1))).argmax(dim=-1)
        for lv, img, _ in attfind.counterfactual_images(G, clf, latents[:n_err].cpu().numpy(), edits, smin, smax, noise, levels,
                                                        shift_size=a.shift, image_batch=n_err):
            got[lv] = img
        styles = edit_levels(coords[:n_err].cpu().numpy(), smin.cpu().numpy(), smax.cpu().numpy(), edits, bc.cpu().numpy(),
                             levels, a.shift)
        worst = 0.0
        for i in range(n_err):
            want = naive_images(G, latents.cpu().numpy(), noise, styles[:, i], i)
            for lv in levels:
                worst = max(worst, float((got[lv][i] - want[lv]).abs().max() / want[lv].abs().max()))
        err_lines.append("%d px, %s, %d images x %d levels: worst max|engine - naive loop on the definition's styles| / max|image| "
                         "= %.3e" % (size, a.precision, n_err, len(levels), worst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--images", type=int, default=250)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--shift", type=float, default=1.0)
    ap.add_argument("--image_batch", type=int, default=32)
    ap.add_argument("--notebook_images", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--errors_out", default=None)
    a = ap.parse_args()
    hb.load_library()
    if not torch.cuda.is_available():
        raise SystemExit("bench_counterfactual measures on the GPU; there is none")
    ops.set_precision(a.precision)
    lines, err_lines = [], []
    for size in a.sizes:
        run_size(size, a, lines, err_lines)
        hb.pack_cache_clear()
    for path, text in ((a.out, lines), (a.errors_out, err_lines)):
        print("\n".join(text))
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
