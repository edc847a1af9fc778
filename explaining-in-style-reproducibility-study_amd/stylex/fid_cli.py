"""FID of one image folder against another, the usage of ``python -m pytorch_fid REAL FAKE`` (which the reference's
``Trainer.calculate_fid`` calls on its two folders, stylex_train.py:1622) on this project's device path:

    python fid_cli.py --real DIR --fake DIR --weights PATH [--batch 256] [--device cuda:0]
                      [--metrics kid,pr [--kid_subsets 100 --kid_subset_size 1000 --pr_k 3]]

Files are decoded with PIL (``convert('RGB')``), batched per image size and handed to fid.FIDEvaluator: 8-bit values
-> [-1, 1] -> 299 px -> Inception-v3 -> fp64 moments on the GPU, the distance in fp64 on the host.  ``--weights`` is the
weight file of pytorch_fid (pt_inception-2015-12-05-6726825d.pth), ``random:<seed>`` for a dry run; without it
$STYLEX_FID_WEIGHTS and torch hub's checkpoint folder are tried.  Prints one line: ``FID: <value>``; with ``--metrics`` the
lines ``KID: <mean> +- <std>`` (kid) and ``Precision: <p>``, ``Recall: <r>`` (pr) follow it, computed from the same pooled
features (fid.kid, fid.precision_recall).
"""
import os
import sys

import numpy as np
import torch

from cli import parse_flags

DEFAULTS = dict(real=None, fake=None, weights=None, batch=256, device="cuda:0", metrics=(), kid_subsets=100, kid_subset_size=1000,
                pr_k=3)
EXTENSIONS = (".bmp", ".jpg", ".jpeg", ".pgm", ".png", ".ppm", ".tif", ".tiff", ".webp")  # pytorch_fid's list


def image_files(folder):
    files = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(EXTENSIONS))
    if not files:
        raise SystemExit("no image files in %s" % folder)
    return files


def add_folder(add, folder, batch, device):
    """Feed every image of `folder` to `add` in batches of at most `batch` images of one size."""
    from PIL import Image

    pending, size = [], None

    def flush():
        if pending:
            x = torch.from_numpy(np.stack(pending)).to(device).permute(0, 3, 1, 2).float().div_(255.)
            add(x)  # a channels_last view: the prep kernel reads it through its strides
            pending.clear()

    for path in image_files(folder):
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"), dtype=np.uint8)
        if a.shape != size or len(pending) == batch:
            flush()
            size = a.shape
        pending.append(a)
    flush()


def folder_fid(real, fake, weights=None, batch=256, device="cuda:0"):
    import fid
    import fid_inception

    device = torch.device(device)
    ev = fid.FIDEvaluator(fid_inception.build(weights, device))
    add_folder(ev.add_real, real, batch, device)
    add_folder(ev.add_fake, fake, batch, device)
    return ev.value()


def folder_metrics(real, fake, weights=None, batch=256, device="cuda:0", metrics=("kid", "pr"), kid_subsets=100, kid_subset_size=1000,
                   pr_k=3):
    """folder_fid with the features kept: {"fid": value, "kid": (mean, std), "precision": p, "recall": r}, the last three as
    `metrics` asks."""
    import fid
    import fid_inception

    device = torch.device(device)
    ev = fid.FIDEvaluator(fid_inception.build(weights, device), keep_features=True)
    add_folder(ev.add_real, real, batch, device)
    add_folder(ev.add_fake, fake, batch, device)
    out = {"fid": ev.value()}
    if "kid" in metrics:
        out["kid"] = ev.kid(num_subsets=int(kid_subsets), max_subset_size=int(kid_subset_size))
    if "pr" in metrics:
        out["precision"], out["recall"] = ev.precision_recall(k=int(pr_k))
    return out


def main(argv=None):
    flags = parse_flags(sys.argv[1:] if argv is None else argv)
    unknown = set(flags) - set(DEFAULTS)
    if unknown:
        raise SystemExit("unknown arguments: %s" % ", ".join(sorted(unknown)))
    a = dict(DEFAULTS, **flags)
    if not a["real"] or not a["fake"]:
        raise SystemExit(__doc__)
    metrics = a["metrics"].split(",") if isinstance(a["metrics"], str) else list(a["metrics"] or ())
    if set(metrics) - {"kid", "pr"}:
        raise SystemExit("--metrics takes kid and pr, got %s" % ",".join(metrics))
    if not metrics:
        value = folder_fid(str(a["real"]), str(a["fake"]), a["weights"], int(a["batch"]), a["device"])
        print("FID: %s" % value)
        return value
    got = folder_metrics(str(a["real"]), str(a["fake"]), a["weights"], int(a["batch"]), a["device"], metrics, a["kid_subsets"],
                         a["kid_subset_size"], a["pr_k"])
    print("FID: %s" % got["fid"])
    if "kid" in got:
        print("KID: %s +- %s" % got["kid"])
    if "precision" in got:
        print("Precision: %s" % got["precision"])
        print("Recall: %s" % got["recall"])
    return got["fid"]


if __name__ == "__main__":
    main()
