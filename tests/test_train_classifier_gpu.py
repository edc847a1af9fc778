"""Three optimiser steps of the classifier training loop on the GPU, both architectures (32 px, B = 4, random:<seed> weights,
dropout p = 0): the fused path (bn_train.fuse_for_training + softmax_cross_entropy on csrc/bn_train.hip), the plain tv_models
module on the GPU, and the plain module in float64 on the CPU, from the same start.

The fused path and the plain fp32 path are two fp32 evaluations of one function in different rounding orders.  Against float64
the fused one may deviate at most twice as much as the plain one (the margin tests/test_fid_gpu.py grants a fused fp32 path
over the library path), plus one float32 rounding of the compared quantity: 2^-24 * max |reference|.  Compared quantities,
each as one vector in the maximum norm (the norm of that test): the per-step losses, the final trainable parameters, every
running statistic.

The learning rate is 1e-6 because of what the PLAIN path does at this size (measured, MI355X): at B = 4 the first-step
gradients of either fp32 path are 1e-4 (ResNet-18) to 2.5e-3 (MobileNetV2) from float64, relatively; Adam at lr = 1e-3 grows
that to 1e-3 in the second loss and 1e-2 in the third, for both paths alike, and then which of the two is closer is chance
(plain / fused third-step loss error 0.009 / 0.031 in one run, 0.031 / 0.022 in another).  At 1e-6 the three steps stay where
a deviation is rounding.  Measured then (MobileNetV2; fused / plain): losses 2.0e-5 / 1.0e-4, running statistics 8.3e-4 /
1.0e-3 (Euclidean).

This test is a check that three whole steps run, stay finite, deterministic and close to float64; it is NOT what holds the
backward of the fused nodes: at lr = 1e-6 no parameter can move more than 3e-6, whatever its gradient.  The gradients
themselves are compared with float64 autograd in tests/test_bn_train_grads_gpu.py (one call and whole networks, before any
optimiser).  The parameter leg here sits, in the maximum norm, on elements whose gradient is zero in exact arithmetic (the shift
of a MobileNetV2 projection BatchNorm, which the next block's BatchNorm removes: 1e-16 in float64, 1e-8 in fp32) or below Adam's
eps: g / (|g| + eps) turns fp32 noise on them into steps of order lr in both paths while float64 stays put.  In the Euclidean
norm the fused MobileNetV2 parameters were 1.66e-4 from float64 and the plain path's 6.5e-5 in the recorded run.  Cause (found
with the gradient comparison at this size, see that file's docstring): one ReLU6 unit of features.18 whose float64
pre-activation is +6.9e-5, where the fp32 activations of either path are 1e-4 off; the fused run landed below zero, the plain
run above, and the closed gate moves every gradient of features.15 - 18 by 1e-2 of its size, enough to change the sign of the
Adam step of some thousand small-gradient elements.  Which path draws that lot is chance.

Also: frozen parameters keep their bits while their BatchNorm buffers move; two runs give the same bits; one command-line run
on a generated folder writes a checkpoint that the frozen-classifier wrappers load strictly.

With STYLEX_BN_RECORD=<file> the measured deviations are appended to that file (profiles/bn_train_errors.txt)."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import bn_train  # noqa: E402
import hip_backend as hb  # noqa: E402
import train_classifier as tc  # noqa: E402

DEV = torch.device("cuda:0")
STEPS, LR = 3, 1e-6


@pytest.fixture(autouse=True)
def need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    hb.load_library()
    assert torch.backends.cudnn.benchmark is False
    prev_det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True  # what train_classifier.set_seed pins: the library's reproducible algorithms only
    yield
    torch.backends.cudnn.deterministic = prev_det


def start(arch):
    model = tc.build_model(arch, "random:7")
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    return model


def batches():
    g = torch.Generator().manual_seed(21)
    return [(torch.randn(4, 3, 32, 32, generator=g), torch.randint(0, 2, (4,), generator=g)) for _ in range(STEPS)]


def run(arch, mode):
    """mode: 'fused' (GPU), 'plain' (GPU, nn.CrossEntropyLoss), 'f64' (CPU, float64).  Returns (losses, model)."""
    model = start(arch)
    if mode == "f64":
        model, dev = model.double(), torch.device("cpu")
    else:
        model, dev = model.to(DEV), DEV
    # every_shape: at 32 px and B = 4 the measured rule (bn_train.measured_shape_rule) would hand every layer to ATen
    net = tc.training_module(model, dev, bn_train.every_shape) if mode == "fused" else model
    if mode == "fused":
        bns = [m for m in net.modules() if isinstance(m, bn_train.BatchNormAct)]
        assert len(bns) == (52 if arch == "mobilenet_v2" else 20) and bns[0].fused(torch.zeros(4, bns[0].num_features, 16, 16, device=dev))
    net.train()
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    losses = []
    for x, t in batches():
        x, t = x.to(dev, next(model.parameters()).dtype), t.to(dev)
        if mode == "fused":
            loss, n_ok = bn_train.softmax_cross_entropy(net(x), t, bn_train.every_shape)
            assert type(loss.grad_fn).__name__ == "_SoftmaxCEFnBackward" and 0 <= int(n_ok) <= 4
        else:
            loss = nn.CrossEntropyLoss()(net(x), t)
        losses.append(loss.detach().double().cpu())
        opt.zero_grad()
        loss.backward()
        opt.step()
    return torch.stack(losses), model


def groups(model):
    train = [p.detach().double().cpu().reshape(-1) for p in model.parameters() if p.requires_grad]
    stats = [b.detach().double().cpu().reshape(-1) for n, b in model.named_buffers() if n.endswith(("running_mean", "running_var"))]
    return torch.cat(train), torch.cat(stats)


@pytest.mark.parametrize("arch", ["mobilenet_v2", "resnet18"])
def test_three_steps_against_plain_fp32_and_float64(arch):
    ref_l, ref_m = run(arch, "f64")
    pl_l, pl_m = run(arch, "plain")
    fu_l, fu_m = run(arch, "fused")
    fu2_l, fu2_m = run(arch, "fused")
    ref, plain, fused = (ref_l,) + groups(ref_m), (pl_l,) + groups(pl_m), (fu_l,) + groups(fu_m)
    lines = []
    ok = True
    for name, r, p, f in zip(("per-step loss", "trainable parameters", "running statistics"), ref, plain, fused):
        e_p, e_f, rnd = float((p - r).abs().max()), float((f - r).abs().max()), 2.0 ** -24 * float(r.abs().max())
        lines.append("%-13s %-21s fused %.3e  plain %.3e  rounding %.3e  fused / (2 plain + rounding) %.3f   (Euclidean: fused %.3e  plain %.3e)"
                     % (arch, name, e_f, e_p, rnd, e_f / (2 * e_p + rnd), float((f - r).norm()), float((p - r).norm())))
        ok = ok and e_f <= 2 * e_p + rnd
    print("\n".join(lines))
    out = os.environ.get("STYLEX_BN_RECORD")
    if out:
        with open(out, "a") as fh:
            fh.write("# tests/test_train_classifier_gpu.py, %s: max |path - float64| after %d Adam steps (lr %g, 32 px, B = 4)\n" % (arch, STEPS, LR))
            fh.write("\n".join(lines) + "\n")
    assert ok, lines
    # two identical runs: the same bits
    assert torch.equal(fu_l, fu2_l)
    assert all(torch.equal(a, b) for a, b in zip(fu_m.state_dict().values(), fu2_m.state_dict().values()))
    # frozen parameters keep their bits, their BatchNorm buffers have moved (the reference runs them in train mode)
    first = start(arch)
    frozen = [n for n, p in fu_m.named_parameters() if not p.requires_grad]
    assert bool(frozen) == (arch == "mobilenet_v2")
    sd0, sd1 = first.state_dict(), fu_m.state_dict()
    for n in frozen:
        assert torch.equal(sd0[n], sd1[n].cpu()), n
    if frozen:
        assert not torch.equal(sd0["features.0.1.running_mean"], sd1["features.0.1.running_mean"].cpu())
        assert int(sd1["features.0.1.num_batches_tracked"]) == STEPS == int(sd1["features.18.1.num_batches_tracked"])
    for n, p in fu_m.named_parameters():
        if p.requires_grad:
            assert not torch.equal(sd0[n], sd1[n].cpu()), n


@pytest.mark.parametrize("arch", ["mobilenet_v2", "resnet18"])
def test_command_line_end_to_end(arch, tmp_path, monkeypatch):
    from PIL import Image

    rng = np.random.RandomState(3)
    for i in range(24):
        d = tmp_path / "data" / ("bright" if i % 2 else "dark")
        d.mkdir(parents=True, exist_ok=True)
        Image.fromarray((rng.randint(0, 60, (32, 32, 3)) + (150 if i % 2 else 0)).astype(np.uint8)).save(d / ("%03d.png" % i))
    monkeypatch.chdir(tmp_path)
    name = "tiny-%s.pth" % arch
    res = tc.main(tc.parse_args(["--arch", arch, "--data", str(tmp_path / "data"), "--pretrained", "random:3", "--epochs", "2",
                                 "--image_size", "32", "--batch_size", "6", "--num_workers", "0", "--checkpoint_name", name,
                                 "--fused_shapes", "all"]))
    assert os.path.isfile(os.path.join("saved_models", name))
    assert json.load(open(os.path.join("classifier_results", "tiny-%s.json" % arch))) == res and 0.0 <= res["accuracy"] <= 1.0
    log = [json.loads(line) for line in open(os.path.join("saved_models", "train_log.jsonl"))]
    assert sum(r["tag"] == "Loss/train" for r in log) == 2 * 3 and sum(r["tag"] == "Accuracy/validation" for r in log) == 2
    assert all(np.isfinite(r["value"]) for r in log)
    os.makedirs("trained_classifiers")
    shutil.copy(os.path.join("saved_models", name), os.path.join("trained_classifiers", name))
    if arch == "mobilenet_v2":
        from mobilenet_classifier import MobileNet

        clf = MobileNet(name, 0, image_size=32)
    else:
        from resnet_classifier import ResNet

        clf = ResNet(name, 0, image_size=32)
    saved = torch.load(os.path.join("saved_models", name), map_location="cpu")
    assert all(torch.equal(v.cpu(), saved[k]) for k, v in clf.model.state_dict().items()) and len(saved) == len(clf.model.state_dict())
