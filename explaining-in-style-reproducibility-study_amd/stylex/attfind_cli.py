"""Command-line entry point of the AttFind workflow (attfind.py; the reference has only the notebook
``stylex/run_attfind_combined.ipynb``): load a trained model of either architecture, run the threshold pass or the
StyleSpace extraction on an image folder, and write the records, the selected coordinates and their image strips.

    python attfind_cli.py --name <run> --models_dir <dir> --data <folder> [--new_architecture] [--load_from N]
        --num_images N [--shift_size 1] [--chunk 256] [--first_pass_batch 1]
        [--use_discriminator --discriminator_threshold X | --find_threshold] [--num_indices 5] [--multi_gpus] [--precision fp32]
        [--counterfactual_fid K --fid_weights SPEC [--counterfactual_shift 1]]

The model is built as ``cli.py --generate`` builds it (``Trainer.load`` reads ``<models_dir>/<name>/.config.json`` and
the checkpoint), the classifier through the Trainer's ``classifier_name`` / ``classifier_path``.  Everything is written
by rank 0 to ``<results_dir>/<name>/attfind``: ``discriminator_threshold.{hdf5|npz}`` with ``--find_threshold``, else
``style_change_records.{hdf5|npz}``, ``significant_styles.json`` (cells 14-16: ``find_significant_styles`` per class after
``split_by_class``) and one ``visualize_style_by_distance_in_s`` PNG per selected coordinate (cell 23).  With
``--counterfactual_fid K`` (default 0: off) rank 0 then runs the counterfactual experiment of the reference's
``stylex/FID_TensorFlow.ipynb`` on the records: the attributes ranked across the two classes
(``attfind.rank_class_directions``), the top-k changed together for k = 1..K (``attfind.counterfactual_sweep``),
``counterfactual_fid.csv`` (the notebook's table: FID(original, generated), FID(original, counterfactual_k)) and
``counterfactual.json`` (the ranked list, flip counts and rates, base classes).  ``--fid_weights`` names the Inception
weights as ``Trainer(fid_weights=)`` does (``random:<seed>`` for tests).

Multi-GPU: the sweep shards over images (attfind.py).  ``--multi_gpus`` starts one process per GPU (``--num_gpus N`` to
use fewer); the parent counts the GPUs in a short-lived child process and spawns the ranks without ever touching the
GPU itself.  Under ``python -m torch.distributed.run`` (WORLD_SIZE > 1 in the environment) the process joins that
group instead.
"""
import json
import os
import subprocess
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import attfind
from cli import parse_flags, set_seed

# flag -> default.  image_size / network_capacity / fmap_max only matter for a run folder without a .config.json
DEFAULTS = dict(
    data="./data", results_dir="./results", models_dir="./models", name="default", new_architecture=False, load_from=-1,
    image_size=64, network_capacity=16, fmap_max=512, classifier_name="resnet", classifier_path="mobilenet-64px-gender.pth",
    num_images=10, shift_size=1.0, chunk=256, first_pass_batch=1, use_discriminator=False, discriminator_threshold=None,
    find_threshold=False, num_indices=5, max_image_effect=2.5, split_by_class=True, max_images=10, visualize_shift_size=2.0,
    multi_gpus=False, num_gpus=None, seed=42, precision="fp32", counterfactual_fid=0, fid_weights=None,
    counterfactual_shift=1.0,
)


def count_gpus():
    """Number of visible GPUs, asked of a child process: the caller's own process stays off the GPU."""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True,
                         text=True, check=True)
    return int(out.stdout.strip().splitlines()[-1])


def load_model(a, device_index):
    from stylex_train import Trainer

    model = Trainer(name=a["name"], results_dir=a["results_dir"], models_dir=a["models_dir"], image_size=a["image_size"],
                    network_capacity=a["network_capacity"], fmap_max=a["fmap_max"], batch_size=1, num_workers=0,
                    classifier_name=a["classifier_name"], classifier_path=a["classifier_path"], tensorboard_dir=None,
                    new_architecture=a["new_architecture"], rank=device_index, device_pipeline=False)
    if not list((model.models_dir / model.name).glob("model_*.pt")):
        raise SystemExit("no checkpoint model_*.pt under %s" % (model.models_dir / model.name))
    model.load(a["load_from"])
    model.StylEx.eval()
    return model


def loader_items(dataset):
    """The dataset's images as [1,3,S,S] batches in path order — the same order on every rank (the sweep's sharding
    relies on it), where the notebook's shuffled batch-1 loader would give each rank its own."""
    for i in sorted(range(len(dataset)), key=lambda i: str(dataset.paths[i])):
        yield dataset[i][None]


def select_and_visualize(a, model, records, folder):
    """Cells 14-16 and 23 on the written records: per class the greedy selection, per selected coordinate one strip."""
    from PIL import Image

    split = attfind.split_by_class(records["base_prob"], records["style_change"], records["latents"], records["distances"],
                                   records["style_coordinates"])
    noise = torch.from_numpy(records["noise"])
    selection, written = {}, []
    for c in (0, 1):
        found = []
        if len(split[c]["index"]) > 0:  # the notebook stops on a class without images (its cell 13)
            found = attfind.find_significant_styles(split[c]["effect"], a["num_indices"], c,
                                                    max_image_effect=a["max_image_effect"])
        selection["class_%d" % c] = [[int(d), int(s)] for d, s in found]
        w, distances = (split[c]["w"], split[c]["dist"]) if a["split_by_class"] else (records["latents"], records["distances"])
        for direction, sindex in selection["class_%d" % c]:
            strip = attfind.visualize_style_by_distance_in_s(model.StylEx.G, model.classifier, w, distances, records["minima"],
                                                             records["maxima"], sindex, direction, a["max_images"],
                                                             a["visualize_shift_size"], noise, class_index=c)
            if strip.size == 0:
                print("class %d, coordinate %d: fewer than three images, no strip" % (c, sindex))
                continue
            written.append("style_class%d_dir%d_s%d.png" % (c, direction, sindex))
            Image.fromarray(strip).save(os.path.join(folder, written[-1]))
    with open(os.path.join(folder, "significant_styles.json"), "w") as f:
        json.dump(dict(selection, num_indices=a["num_indices"], max_image_effect=a["max_image_effect"], images=written), f)
    print("selected (direction, coordinate):", selection)


def counterfactual_experiment(a, model, records, folder):
    """FID_TensorFlow.ipynb cells 11 (filter_unstable_images, its defaults), 13, 20, 24 and 25 on the written records."""
    import numpy as np

    import fid
    import fid_inception

    effect = attfind.filter_unstable_images(np.array(records["style_change"], copy=True))
    ranked = attfind.rank_class_directions(effect, records["base_prob"])
    evaluator = fid.FIDEvaluator(fid_inception.build(a["fid_weights"], model.device))
    out = attfind.counterfactual_sweep(model.StylEx, model.classifier, records, ranked, num_attributes=a["counterfactual_fid"],
                                       shift_size=a["counterfactual_shift"], fid=evaluator)
    attfind.write_fid_table(out["fid"], os.path.join(folder, "counterfactual_fid.csv"))
    with open(os.path.join(folder, "counterfactual.json"), "w") as f:
        json.dump(dict(ranked=[[d, s] for d, s in ranked], k=out["k"], flips=out["flips"], flip_rate=out["flip_rate"],
                       base_class=[int(c) for c in out["base_class"]], shift_size=a["counterfactual_shift"]), f)
    print("counterfactual FID (generated, top-1 .. top-%d):" % len(out["k"]), ["%.2f" % v for v in out["fid"]],
          "flip rate:", out["flip_rate"])


def run(rank, world_size, a, local_rank=None, spawned=True):
    on_gpu = torch.cuda.is_available()
    device_index = (rank if local_rank is None else local_rank) % max(1, torch.cuda.device_count()) if on_gpu else 0
    if world_size > 1:
        if spawned:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "12356")
        if on_gpu:
            torch.cuda.set_device(device_index)
        dist.init_process_group("nccl" if on_gpu else "gloo", rank=rank, world_size=world_size)  # "nccl" is RCCL on ROCm
        print(f"{rank + 1}/{world_size} process initialized.")
    import ops

    set_seed(a["seed"])  # every rank draws the same noise plane
    ops.set_precision(a["precision"])
    model = load_model(a, device_index)
    model.set_data_src(a["data"])
    noise = torch.empty(1, model.image_size, model.image_size, 1).uniform_(0., 1.)
    folder = str(model.results_dir / model.name / "attfind")
    if rank == 0:
        os.makedirs(folder, exist_ok=True)
    if a["find_threshold"]:
        if rank == 0:  # one batch-1 pass over the images: nothing to shard
            out = attfind.find_discriminator_threshold(model.StylEx, model.classifier, loader_items(model.dataset),
                                                       a["num_images"], noise, threshold_folder=folder,
                                                       first_pass_batch=a["first_pass_batch"])
            d = out["discriminator_outputs"].reshape(-1)
            print("discriminator outputs of %d images: min %.4f median %.4f max %.4f" % (d.numel(), d.min(), d.median(), d.max()))
    else:
        attfind.attfind_extraction(model.StylEx, model.classifier, loader_items(model.dataset), a["num_images"], noise,
                                   shift_size=a["shift_size"], discriminator_threshold=a["discriminator_threshold"],
                                   use_discriminator=a["use_discriminator"], chunk=a["chunk"],
                                   results_folder=folder if rank == 0 else None, first_pass_batch=a["first_pass_batch"])
        if rank == 0:
            records = attfind.load_records(folder)
            select_and_visualize(a, model, records, folder)
            if a["counterfactual_fid"] > 0:
                counterfactual_experiment(a, model, records, folder)
    if world_size > 1:
        dist.barrier()
        dist.destroy_process_group()


def main(argv=None):
    flags = parse_flags(sys.argv[1:] if argv is None else argv)
    unknown = set(flags) - set(DEFAULTS)
    if unknown:
        raise SystemExit("unknown arguments: %s" % ", ".join(sorted(unknown)))
    a = dict(DEFAULTS, **flags)
    if a["use_discriminator"] and a["discriminator_threshold"] is None:
        raise SystemExit("--use_discriminator needs --discriminator_threshold (run --find_threshold to choose one)")
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if env_world > 1:  # launched by torch.distributed.run: one process per GPU already exists
        run(int(os.environ["RANK"]), env_world, a, local_rank=int(os.environ.get("LOCAL_RANK", os.environ["RANK"])),
            spawned=False)
        return
    world_size = 1
    if a["multi_gpus"]:
        world_size = a["num_gpus"] if a["num_gpus"] is not None else count_gpus()
    if world_size <= 1:
        run(0, 1, a)
        return
    # "spawn" start method: every rank is a fresh interpreter; this process has made no GPU call and makes none
    mp.spawn(run, args=(world_size, a), nprocs=world_size, join=True)


if __name__ == "__main__":
    main()
