"""Reconstruction fidelity report (recon_metrics.py; the reference has none):

    python recon_cli.py --name <run> --models_dir <dir> --data <folder> --num_images N [--new_architecture] [--no_quantise]
        [--load_from N] [--batch 32] [--results_dir <dir>] [--classifier_name resnet --classifier_path PATH] [--precision fp32]
    python recon_cli.py --a DIR --b DIR [--no_quantise] [--batch 64] [--out FILE.json] [--device cuda:0]

The first form builds the model as ``attfind_cli.py`` does (``Trainer.load`` reads ``<models_dir>/<name>/.config.json`` and
the checkpoint), reconstructs N images of the folder through encoder -> EMA generator and writes
``<results_dir>/<name>/reconstruction.json`` (recon_metrics.summary: mean, standard deviation and count of MAE, MSE, PSNR,
SSIM, LPIPS, the classifier KL and probability shift, the agreement rate, the number of infinite PSNRs) and
``reconstruction.npz`` (the per-image arrays).

The second form needs no model: it pairs the image files of two folders BY NAME (the stem: ``7.png`` pairs with ``7.jpg``) —
saved reconstructions, the reference's for instance, against their originals — and reports the image-pair metrics only.
A name without its partner is an error that lists every such name.  Files are decoded with PIL (``convert('RGB')``); a pair
must agree in size.  Prints the summary as one JSON line, and writes it to ``--out`` when given.

``--no_quantise`` compares clamp(v, 0, 1) in fp32 instead of the bytes an image file would hold (for decoded files the two
see the same values).
"""
import json
import os
import sys

import numpy as np
import torch

import recon_metrics
from cli import parse_flags, set_seed
from fid_cli import EXTENSIONS

DEFAULTS = dict(
    data="./data", results_dir="./results", models_dir="./models", name="default", new_architecture=False, load_from=-1,
    image_size=64, network_capacity=16, fmap_max=512, classifier_name="resnet", classifier_path="mobilenet-64px-gender.pth",
    num_images=64, batch=32, no_quantise=False, seed=42, precision="fp32", a=None, b=None, out=None, device="cuda:0",
)


def by_stem(folder):
    """stem -> path of every image file in `folder`; two files with one stem are an error."""
    out = {}
    for f in sorted(os.listdir(folder)):
        if f.lower().endswith(EXTENSIONS):
            stem = os.path.splitext(f)[0]
            if stem in out:
                raise SystemExit("%s holds two images named %s" % (folder, stem))
            out[stem] = os.path.join(folder, f)
    if not out:
        raise SystemExit("no image files in %s" % folder)
    return out


def paired_files(a, b):
    fa, fb = by_stem(a), by_stem(b)
    only_a, only_b = sorted(set(fa) - set(fb)), sorted(set(fb) - set(fa))
    if only_a or only_b:
        raise SystemExit("unpaired images: only in %s: %s; only in %s: %s" % (a, ", ".join(only_a) or "-", b,
                                                                               ", ".join(only_b) or "-"))
    return [(fa[s], fb[s]) for s in sorted(fa)]


def folder_pair_metrics(a, b, quantise=True, batch=64, device="cuda:0"):
    """Per-image mae, mse, psnr, ssim (fp64 arrays, in the order of the sorted names) of the files of `a` against `b`."""
    import hip_backend as hb
    from PIL import Image

    device = torch.device(device)
    arrays = {k: [] for k in ("mae", "mse", "psnr", "ssim")}
    pending, size = [], None

    def flush():
        if pending:
            xs = [torch.from_numpy(np.stack(p)).to(device).permute(0, 3, 1, 2).float().div_(255.) for p in zip(*pending)]
            pair = hb.image_pair_stats(xs[0], xs[1], channels=3, quantise=quantise)  # channels-last views, read by stride
            for k in arrays:
                arrays[k].append(getattr(pair, k).cpu().numpy())
            pending.clear()

    for pa, pb in paired_files(a, b):
        with Image.open(pa) as im:
            xa = np.asarray(im.convert("RGB"), dtype=np.uint8)
        with Image.open(pb) as im:
            xb = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if xa.shape != xb.shape:
            raise SystemExit("%s is %s, %s is %s" % (pa, xa.shape[:2], pb, xb.shape[:2]))
        if xa.shape != size or len(pending) == batch:
            flush()
            size = xa.shape
        pending.append((xa, xb))
    flush()
    return {k: np.concatenate(v) for k, v in arrays.items()}


def run_folders(a):
    per_image = folder_pair_metrics(str(a["a"]), str(a["b"]), not a["no_quantise"], int(a["batch"]), a["device"])
    out = recon_metrics.pair_summary(per_image)
    line = json.dumps(out, sort_keys=True)
    if a["out"]:
        with open(str(a["out"]), "w") as f:
            f.write(line + "\n")
    print(line)
    return out


def run_model(a):
    import ops
    from attfind_cli import load_model, loader_items

    set_seed(a["seed"])
    ops.set_precision(a["precision"])
    model = load_model(a, 0)
    model.set_data_src(a["data"])
    ev = recon_metrics.ReconEvaluator(model.StylEx, model.classifier, model.lpips_fn, model.new_architecture,
                                      quantise=not a["no_quantise"])
    if ev.lpips is None:
        from stylex_train import get_lpips

        ev.lpips = get_lpips(model.device)
    pending = []
    for i, item in enumerate(loader_items(model.dataset)):
        if i >= int(a["num_images"]):
            break
        pending.append(item)
        if len(pending) == int(a["batch"]):
            ev.add(torch.cat(pending).to(model.device))
            pending = []
    if pending:
        ev.add(torch.cat(pending).to(model.device))
    out = ev.summary()
    folder = model.results_dir / model.name
    folder.mkdir(parents=True, exist_ok=True)
    with open(str(folder / "reconstruction.json"), "w") as f:
        json.dump(out, f, sort_keys=True)
    np.savez(str(folder / "reconstruction.npz"), **ev.per_image())
    print(json.dumps(out, sort_keys=True))
    return out


def main(argv=None):
    flags = parse_flags(sys.argv[1:] if argv is None else argv)
    unknown = set(flags) - set(DEFAULTS)
    if unknown:
        raise SystemExit("unknown arguments: %s" % ", ".join(sorted(unknown)))
    a = dict(DEFAULTS, **flags)
    if (a["a"] is None) != (a["b"] is None):
        raise SystemExit("--a and --b go together")
    return run_folders(a) if a["a"] is not None else run_model(a)


if __name__ == "__main__":
    main()
