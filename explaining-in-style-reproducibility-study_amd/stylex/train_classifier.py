"""Train the classifier that StylEx explains: ``trained_classifiers/<name>.pt`` for Trainer, AttFind and calculate_fid.

The reference makes that file with stylex/train_mobilenet_classifier.py (MobileNetV2, torch.hub weights, the first 15
feature layers frozen) and with classifier_training_celeba.ipynb (ResNet-18, fc = Linear(512, 2), nothing frozen); both
need torch.hub and torchvision.  Here the two networks are tv_models.MobileNetV2 / ResNet18 (torchvision's state-dict
keys) and the pretrained weights come from a local file (``--pretrained``; nothing is ever downloaded).  On the GPU the
batch-norm / activation / residual groups and the cross-entropy can run on the kernels of csrc/bn_train.hip
(bn_train.fuse_for_training, bn_train.softmax_cross_entropy); by default (``--fused_shapes measured``) only the shapes do
at which they were measured faster than ATen — large planes; the classifier's own B x 2 loss and every plane of 14 x 14 and
below stay on ATen — and ``--fused_shapes all`` sends every group there.  The convolutions, max-pool, global mean, Dropout
(torch's own RNG stream) and Linear are torch ops either way.

The loop is the reference's: Adam(lr) over all parameters, mean cross-entropy, zero_grad / backward / step per batch; after
each epoch train and validation accuracy in eval mode under no_grad; model.state_dict() is saved when the validation accuracy
strictly improves; the best checkpoint is reloaded at the end, the test split is run and
``classifier_results/<stem>.json`` holds {"accuracy": ...}.  Accuracy counts accumulate on the device; the host reads are
the reference's loss.item() per batch and one read per evaluation.

    python train_classifier.py --data ROOT [--arch mobilenet_v2|resnet18] [--pretrained PATH|random:<seed>] ...
"""
import argparse
import csv
import functools
import json
import os
import sys
import time

import numpy as np
import torch
from torch import nn
from torch.utils.data import DataLoader, Dataset, random_split

# imported before the first convolution: it takes the library's faulting backward-data solver out of the solver list
import hip_backend  # noqa: F401
import bn_train
import tv_models

_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_IMAGE_EXT = (".jpg", ".jpeg", ".png", ".bmp", ".webp")
GENDER = {"male": 0, "female": 1}
ARCH_DEFAULTS = {"mobilenet_v2": {"lr": 0.01, "batch_size": 200}, "resnet18": {"lr": 1e-4, "batch_size": 128}}


def set_seed(seed):
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False  # as the reference; the library's exhaustive search also reaches a faulting solver


class LabelledImages(Dataset):
    """Images with integer labels, from either layout:

    * class sub-folders ``root/<class>/*.jpg``: the classes are the sub-folder names in sorted order;
    * a flat folder ``root/*.jpg`` with ``labels_csv`` and its column ``label``: the file list is SORTED; a row is matched
      by the csv's ``image_number`` column against the file stem (as integers where both are numbers) where that column
      exists, otherwise by row order against the sorted list.  The ``{"male": 0, "female": 1}`` mapping applies for
      ``label == "gender"``, sorted unique values otherwise.

    Deliberate deviation: the reference (data/Kaggle_FFHQ_Resized_256px/data_loader.py) pairs an UNSORTED os.listdir with
    the csv's row order, so which label an image gets depends on the file system.  The csv is read with the csv module.

    Transform (the reference's, on the host through PIL): Resize(image_size) of the smaller edge, bilinear; ToTensor;
    Normalize with the ImageNet mean / std."""

    def __init__(self, root, labels_csv=None, label=None, image_size=224):
        self.root, self.image_size = root, int(image_size)
        if labels_csv is None:
            self.classes = sorted(d for d in os.listdir(root) if os.path.isdir(os.path.join(root, d)))
            if not self.classes:
                raise ValueError("%s has no class sub-folders; give labels_csv= and label= for a flat folder" % root)
            self.samples = [(os.path.join(root, c, f), i) for i, c in enumerate(self.classes)
                            for f in sorted(os.listdir(os.path.join(root, c))) if f.lower().endswith(_IMAGE_EXT)]
        else:
            files = sorted(f for f in os.listdir(root) if f.lower().endswith(_IMAGE_EXT))
            with open(labels_csv, newline="") as fh:
                rows = list(csv.DictReader(fh))
            if not rows or label not in rows[0]:
                raise ValueError("%s has no column %r" % (labels_csv, label))
            if "image_number" in rows[0]:
                by_key = {self._key(r["image_number"]): r[label] for r in rows}
                values = []
                for f in files:
                    k = self._key(os.path.splitext(f)[0])
                    if k not in by_key:
                        raise ValueError("%s: no row with image_number %s in %s" % (f, k, labels_csv))
                    values.append(by_key[k])
            else:
                if len(rows) != len(files):
                    raise ValueError("%d images in %s but %d rows in %s" % (len(files), root, len(rows), labels_csv))
                values = [r[label] for r in rows]
            mapping = GENDER if label == "gender" else {v: i for i, v in enumerate(sorted(set(values)))}
            self.classes = sorted(mapping, key=mapping.get)
            self.samples = [(os.path.join(root, f), mapping[v]) for f, v in zip(files, values)]
        if not self.samples:
            raise ValueError("no images under %s" % root)

    @staticmethod
    def _key(s):
        s = str(s).strip()
        return int(s) if s.isdigit() else s

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, index):
        from PIL import Image

        path, target = self.samples[index]
        with Image.open(path) as im:
            im = im.convert("RGB")
            w, h = im.size
            s = self.image_size
            if (w <= h and w != s) or (h < w and h != s):  # torchvision's Resize(int): the smaller edge becomes s
                nw, nh = (s, int(s * h / w)) if w <= h else (int(s * w / h), s)
                im = im.resize((nw, nh), Image.BILINEAR)
            x = torch.from_numpy(np.asarray(im, dtype=np.uint8).copy()).permute(2, 0, 1).float().div_(255.0)
        mean, std = torch.tensor(_MEAN).view(3, 1, 1), torch.tensor(_STD).view(3, 1, 1)
        return (x - mean) / std, target


def split_dataset(dataset, valid_ratio=0.15, test_ratio=0.15):
    """The reference's split (ffhq_utils.get_train_valid_test_dataset): int(len * 0.7) + remainder / int(len * 0.15) /
    int(len * 0.15), random_split under Generator().manual_seed(42)."""
    n = len(dataset)
    train, valid, test = int(n * (1 - valid_ratio - test_ratio)), int(n * valid_ratio), int(n * test_ratio)
    train += n - train - valid - test
    return random_split(dataset, [train, valid, test], generator=torch.Generator().manual_seed(42))


def _loader(dataset, batch_size, num_workers, device):
    return DataLoader(dataset, batch_size=batch_size, generator=torch.Generator().manual_seed(42),
                      pin_memory=device.type == "cuda", num_workers=num_workers)


def build_model(arch, pretrained=None, amount_frozen_layers=15, freeze_all_layers=False, num_classes=2):
    """The reference's load_mobilenet (or the notebook's ResNet-18): pretrained weights, then the new head, then the freeze.
    pretrained: a torchvision state-dict file, 'random:<seed>' (tests, timing) or None (torch's default initialisation)."""
    if arch not in ARCH_DEFAULTS:
        raise ValueError("--arch must be one of %s" % sorted(ARCH_DEFAULTS))
    if pretrained is not None and str(pretrained).startswith("random:"):
        state = torch.random.get_rng_state()
        torch.manual_seed(int(str(pretrained).split(":", 1)[1]))
        model = tv_models.MobileNetV2() if arch == "mobilenet_v2" else tv_models.ResNet18()
        head = nn.Linear(1280 if arch == "mobilenet_v2" else 512, num_classes)
        torch.random.set_rng_state(state)
    else:
        model = tv_models.MobileNetV2() if arch == "mobilenet_v2" else tv_models.ResNet18()
        if pretrained is not None:
            if not os.path.isfile(pretrained):
                raise FileNotFoundError("--pretrained %s: no such file (a torchvision %s state dict; nothing is downloaded)"
                                        % (pretrained, arch))
            model.load_state_dict(torch.load(pretrained, map_location="cpu"))
        head = nn.Linear(1280 if arch == "mobilenet_v2" else 512, num_classes)
    if arch == "resnet18":
        model.fc = head  # the notebook's recipe: nothing frozen
        return model
    if freeze_all_layers:
        for p in model.parameters():
            p.requires_grad = False
    model.classifier[1] = head
    for layer in range(amount_frozen_layers):
        for p in model.features[layer].parameters():
            p.requires_grad = False
    return model


def training_module(model, device, shape_rule=None):
    """What the loop calls: the fused module (it shares every tensor with `model`, which must already be on `device`).  On the
    GPU its BatchNormAct layers run the kernels in training mode; on the CPU they are the composable formula, bit for bit
    what `model` computes."""
    assert next(model.parameters()).device.type == device.type
    return bn_train.fuse_for_training(model, shape_rule)


def evaluate_model(net, loader, device, loss_fn=bn_train.softmax_cross_entropy):
    """Accuracy of `net` over `loader`: the counts stay on the device, one host read at the end."""
    correct = torch.zeros((), dtype=torch.int64, device=device)
    seen = 0
    for images, targets in loader:
        images, targets = images.to(device), targets.to(device)
        _, n_ok = loss_fn(net(images), targets)
        correct += n_ok
        seen += len(targets)
    return correct.item() / max(seen, 1)


class _Log:
    """train_log.jsonl always; TensorBoard scalars when the package is importable."""

    def __init__(self, save_dir):
        os.makedirs(save_dir, exist_ok=True)
        self.path = os.path.join(save_dir, "train_log.jsonl")
        self.fh = open(self.path, "a")
        try:
            from torch.utils.tensorboard import SummaryWriter

            self.tb = SummaryWriter(log_dir=os.path.join(save_dir, "tboard_logs"))
        except Exception:  # noqa: BLE001  (the package is optional)
            self.tb = None

    def scalar(self, tag, value, step):
        self.fh.write(json.dumps({"tag": tag, "step": int(step), "value": float(value)}) + "\n")
        self.fh.flush()
        if self.tb is not None:
            self.tb.add_scalar(tag, value, step)

    def close(self):
        self.fh.close()
        if self.tb is not None:
            self.tb.close()


def train_model(model, lr, batch_size, epochs, checkpoint_path, device, train_dataset, val_dataset, num_workers=0, log=None,
                net=None, loss_fn=bn_train.softmax_cross_entropy):
    """The reference's train_model.  Returns the per-batch losses; `model` holds the best-on-validation weights afterwards.
    net: the module the loop calls (default: training_module(model)); loss_fn(logits, targets) -> (loss, n_correct)."""
    assert epochs > 0, "To train the model the amount of epochs has to be higher than 1."
    net = net if net is not None else training_module(model, device)
    train_loader = _loader(train_dataset, batch_size, num_workers, device)
    valid_loader = _loader(val_dataset, batch_size, num_workers, device)
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    best, losses = 0, []
    net.train()
    for epoch in range(epochs):
        t0, epoch_losses = time.time(), []
        for batch_num, (images, targets) in enumerate(train_loader):
            images, targets = images.to(device), targets.to(device)
            batch_loss, _ = loss_fn(net(images), targets)
            epoch_losses.append(batch_loss.item())
            if log is not None:
                log.scalar("Loss/train", epoch_losses[-1], epoch * len(train_loader) + batch_num)
            print("\r", "Epoch: %d: batch %d/%d, running loss: %s" % (epoch, batch_num + 1, len(train_loader),
                                                                       np.average(epoch_losses)), end="")
            optimizer.zero_grad()
            batch_loss.backward()
            optimizer.step()
        losses += epoch_losses
        net.eval()
        with torch.no_grad():
            train_acc = evaluate_model(net, train_loader, device, loss_fn)
            valid_acc = evaluate_model(net, valid_loader, device, loss_fn)
        print(", train accuracy: %s, validation accuracy: %s, epoch took: %.2f minutes" % (train_acc, valid_acc,
                                                                                           (time.time() - t0) / 60))
        if valid_acc > best:
            os.makedirs(os.path.dirname(checkpoint_path) or ".", exist_ok=True)
            torch.save(model.state_dict(), checkpoint_path)
            best = valid_acc
        if log is not None:
            log.scalar("Accuracy/train", train_acc, epoch)
            log.scalar("Accuracy/validation", valid_acc, epoch)
        net.train()
    if os.path.isfile(checkpoint_path):
        model.load_state_dict(torch.load(checkpoint_path, map_location=device))
    return losses


def test_model(model, batch_size, device, seed, test_dataset, num_workers=0, net=None, loss_fn=bn_train.softmax_cross_entropy):
    set_seed(seed)
    net = net if net is not None else training_module(model, device)
    net.eval()
    with torch.no_grad():
        accuracy = evaluate_model(net, _loader(test_dataset, batch_size, num_workers, device), device, loss_fn)
    print("Test accuracy: %.4f" % accuracy)
    net.train()
    return {"accuracy": accuracy}


def make_parser():
    p = argparse.ArgumentParser(description="Train a classifier")
    # the reference script's flags and defaults
    p.add_argument("--freeze_all_layers", dest="freeze_all_layers", action="store_true")
    p.add_argument("--amount_frozen_layers", dest="amount_frozen_layers", type=int, default=15)
    p.add_argument("--dataset", type=str, default="FFHQ-Aging", help="Dataset to train on")
    p.add_argument("--labels", type=str, default="gender", help="Labels to train on")
    p.add_argument("--lr", default=None, type=float, help="Learning rate to use (0.01; 1e-4 with --arch resnet18)")
    p.add_argument("--batch_size", default=None, type=int, help="Minibatch size (200; 128 with --arch resnet18)")
    p.add_argument("--epochs", default=50, type=int, help="Max number of epochs")
    p.add_argument("--seed", default=42, type=int, help="Seed to use for reproducing results")
    p.add_argument("--checkpoint_name", default="FFHQ-Gender.pth", type=str, help="Name of the model checkpoint")
    p.add_argument("--continue_training", dest="continue_training", action="store_true")
    # additions
    p.add_argument("--arch", default="mobilenet_v2", choices=sorted(ARCH_DEFAULTS))
    p.add_argument("--pretrained", default=None, help="torchvision state dict to start from, or random:<seed>; never downloaded")
    p.add_argument("--save_dir", default="saved_models")
    p.add_argument("--data", default="data/Kaggle_FFHQ_Resized_256px", help="class sub-folders, or a flat folder with --labels_csv")
    p.add_argument("--labels_csv", default=None, help="csv with a column named by --labels (and optionally image_number)")
    p.add_argument("--image_size", default=224, type=int)
    p.add_argument("--num_workers", default=6, type=int)
    p.add_argument("--fused_shapes", default="measured", choices=["measured", "all"],
                   help="batch-norm and loss calls that run on the HIP kernels: those measured faster than ATen's (default), or all")
    return p


def parse_args(argv=None):
    args = make_parser().parse_args(argv)
    for k, v in ARCH_DEFAULTS[args.arch].items():
        if getattr(args, k) is None:
            setattr(args, k, v)
    return args


def main(args):
    device = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    set_seed(args.seed)
    dataset = LabelledImages(args.data, args.labels_csv, args.labels if args.labels_csv else None, args.image_size)
    train_dataset, valid_dataset, test_dataset = split_dataset(dataset)
    model = build_model(args.arch, args.pretrained, args.amount_frozen_layers, args.freeze_all_layers,
                        num_classes=max(2, len(dataset.classes))).to(device)
    every = args.fused_shapes == "all"
    net = training_module(model, device, bn_train.every_shape if every else None)
    loss_fn = functools.partial(bn_train.softmax_cross_entropy, shape_rule=bn_train.every_shape) if every else bn_train.softmax_cross_entropy
    checkpoint_path = os.path.join(args.save_dir, args.checkpoint_name)
    log = _Log(args.save_dir)
    run = dict(lr=args.lr, batch_size=args.batch_size, epochs=args.epochs, checkpoint_path=checkpoint_path, device=device,
               train_dataset=train_dataset, val_dataset=valid_dataset, num_workers=args.num_workers, log=log, net=net,
               loss_fn=loss_fn)
    if not os.path.exists(checkpoint_path):
        train_model(model, **run)
    else:
        model.load_state_dict(torch.load(checkpoint_path, map_location=device))
        if args.continue_training:
            train_model(model, **run)
    results = test_model(model, args.batch_size, device, args.seed, test_dataset, args.num_workers, net=net, loss_fn=loss_fn)
    log.close()
    os.makedirs("classifier_results", exist_ok=True)
    with open(os.path.join("classifier_results", args.checkpoint_name.split(".")[0] + ".json"), "w") as f:
        json.dump(results, f)
    loader = "mobilenet_classifier.MobileNet" if args.arch == "mobilenet_v2" else "resnet_classifier.ResNet"
    print("checkpoint: %s — copy it to trained_classifiers/%s; %s('%s', 0) then loads it (strict)"
          % (checkpoint_path, args.checkpoint_name, loader, args.checkpoint_name))
    return results


if __name__ == "__main__":
    main(parse_args(sys.argv[1:]))
