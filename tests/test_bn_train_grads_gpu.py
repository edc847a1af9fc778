"""The gradients of the fused autograd nodes (stylex/bn_train.py) against float64 autograd, BEFORE any optimiser touches them:

* one BatchNormAct call: dx, dgamma, dbeta, dresidual for every activation, with and without residual, and with only some of
  the inputs requiring a gradient (the node returns exactly the gradients that were asked for);
* softmax_cross_entropy: dlogits under a non-trivial upstream gradient;
* the whole networks (MobileNetV2 with 15 frozen layers, ResNet-18; 64 px, B = 16, random:<seed> weights, dropout p = 0): the
  .grad of every trainable parameter after one backward.

Rule, as in tests/test_train_classifier_gpu.py: against float64 the fused path may err at most twice as much as the plain fp32
path (F.batch_norm + activation, F.cross_entropy, the plain tv_models module on the GPU) plus one float32 rounding of the
quantity.  One call: each gradient in the maximum norm.  Networks: every parameter's gradient error is divided by that
parameter's largest float64 gradient, and the concatenation over all trainable parameters is compared in the Euclidean norm
(millions of elements: the figure is stable run to run, and a wrong gradient in any one parameter tensor is an error of
order 1 in a quantity that is 1e-4 for the plain path); no parameter tensor may be 10 times worse than plain on its own.
Parameters whose gradient is zero in exact arithmetic (the shift of a MobileNetV2 projection BatchNorm, which the next block's
BatchNorm removes: below 1e-12 in float64) have no scale to divide by; for them both fp32 paths must stay below 1e-6 absolutely.

Why 64 px and B = 16 and not the 32 px, B = 4 of the three-step test (measured there, MI355X): at 32 px the last MobileNetV2
layers are 1 x 1 planes normalised over 4 values, and the fp32 activations that reach features.18 are 4e-5 (plain) to 1.5e-4
(fused) from float64 in either path.  One ReLU6 unit of that layer (channel 346, sample 3) has the float64 pre-activation
+6.9e-5; the plain run saw +1.1e-4 and the fused run -8.2e-5, so the fused run closed a gate that float64 and plain left
open.  That one unit is the whole of that layer's shift-gradient error (5.8e-4 of 1.35e-2 against 1e-6 plain), makes every
gradient upstream of it (features.15 - 18) 1e-2 instead of 1e-3 from float64, and with it the excess of sign-changed Adam steps
that the three-step test records; on the 12 747 elements with a float64 gradient below 1e-7 the fused path's first gradient is
closer than the plain one's (4.3e-9 against 6.6e-9).  Which path lands on which side of such a zero is chance, and a comparison
at that size measures the chance.  At 64 px and B = 16 the tail normalises 2 x 2 planes over 64 values and fewer units sit that
close to zero; measured there (recorded run): MobileNetV2 Euclidean 0.72 fused against 1.14 plain, ResNet-18 0.0741 both, and the
worst tensors carry the same error in both paths (features.18.1.bias 2.4e-2 in each: a gate both fp32 paths close alike).

With STYLEX_BN_RECORD=<file> the figures are appended to that file (profiles/bn_train_errors.txt)."""
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

import bn_train  # noqa: E402
import hip_backend as hb  # noqa: E402
import train_classifier as tc  # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    hb.load_library()
    prev_det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev_det


def record(lines):
    print("\n".join(lines))
    out = os.environ.get("STYLEX_BN_RECORD")
    if out:
        with open(out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def torch_act(v, act):
    return {"none": lambda t: t, "relu": F.relu, "relu6": F.relu6}[act](v)


def one_call(x, gamma, beta, res, gy, act, needs, mode):
    """Gradients of act(bn(x) (+ res)) with respect to the inputs named in `needs`; mode 'f64' (CPU), 'plain' or 'fused' (GPU)."""
    dt, dev = (torch.float64, torch.device("cpu")) if mode == "f64" else (torch.float32, DEV)
    t = {k: (v.to(dev, dt).requires_grad_(k in needs) if v is not None else None)
         for k, v in (("x", x), ("gamma", gamma), ("beta", beta), ("res", res))}
    if mode == "fused":
        m = bn_train.BatchNormAct(x.shape[1], act=act).to(DEV).train()
        m.shape_rule = bn_train.every_shape
        m.weight, m.bias = nn.Parameter(t["gamma"], requires_grad="gamma" in needs), nn.Parameter(t["beta"], requires_grad="beta" in needs)
        y = m(t["x"], t["res"])
        assert type(y.grad_fn).__name__ == "_BatchNormActFnBackward"
        t["gamma"], t["beta"] = m.weight, m.bias
    else:
        out = F.batch_norm(t["x"], None, None, t["gamma"], t["beta"], True, 0.1, 1e-5)
        y = torch_act(out if t["res"] is None else out + t["res"], act)
    y.backward(gy.to(dev, dt))
    for k in ("x", "gamma", "beta", "res"):
        if t[k] is not None and k not in needs:
            assert t[k].grad is None, (mode, k)
    return {k: t[k].grad.detach().double().cpu() for k in needs}


@pytest.mark.parametrize("shape", [(3, 24, 7, 7), (4, 20, 1, 1), (6, 16, 28, 28)])
@pytest.mark.parametrize("act", ["none", "relu", "relu6"])
@pytest.mark.parametrize("needs", [("x", "gamma", "beta", "res"), ("x", "gamma", "beta"), ("gamma", "beta"), ("x",), ("res", "beta")])
def test_one_call_gradients(shape, act, needs):
    g = torch.Generator().manual_seed(sum(shape) + len(needs))
    x, gy = 1 + torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    res = torch.randn(shape, generator=g) if "res" in needs else None
    gamma, beta = 1 + 0.3 * torch.randn(shape[1], generator=g), 0.5 * torch.randn(shape[1], generator=g)
    ref, plain, fused = (one_call(x, gamma, beta, res, gy, act, needs, mode) for mode in ("f64", "plain", "fused"))
    lines, ok = [], True
    for k in needs:
        e_p, e_f, rnd = float((plain[k] - ref[k]).abs().max()), float((fused[k] - ref[k]).abs().max()), U * float(ref[k].abs().max())
        lines.append("one call %-14s %-6s d%-6s fused %.3e  plain %.3e  rounding %.3e  fused / (2 plain + rounding) %.3f"
                     % ("x".join(map(str, shape)), act, k, e_f, e_p, rnd, e_f / (2 * e_p + rnd)))
        ok = ok and e_f <= 2 * e_p + rnd
    print("\n".join(lines))
    assert ok, lines


@pytest.mark.parametrize("b,k", [(4, 2), (200, 2), (33, 10), (128, 1000)])
def test_cross_entropy_gradient(b, k):
    g = torch.Generator().manual_seed(b + k)
    z, t, w = torch.randn(b, k, generator=g) * 3, torch.randint(0, k, (b,), generator=g), 1.7
    zr = z.double().requires_grad_()
    (F.cross_entropy(zr, t) * w).backward()
    zp = z.to(DEV).requires_grad_()
    (F.cross_entropy(zp, t.to(DEV)) * w).backward()
    zf = z.to(DEV).requires_grad_()
    loss, _ = bn_train.softmax_cross_entropy(zf, t.to(DEV), bn_train.every_shape)
    assert type(loss.grad_fn).__name__ == "_SoftmaxCEFnBackward"
    (loss * w).backward()
    e_p, e_f = float((zp.grad.double().cpu() - zr.grad).abs().max()), float((zf.grad.double().cpu() - zr.grad).abs().max())
    rnd = U * float(zr.grad.abs().max())
    print("dlogits %dx%d fused %.3e  plain %.3e  rounding %.3e  fused / (2 plain + rounding) %.3f" % (b, k, e_f, e_p, rnd, e_f / (2 * e_p + rnd)))
    assert e_f <= 2 * e_p + rnd


def network_grads(arch, mode):
    model = tc.build_model(arch, "random:7")
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    g = torch.Generator().manual_seed(21)
    x, t = torch.randn(16, 3, 64, 64, generator=g), torch.randint(0, 2, (16,), generator=g)
    if mode == "f64":
        model, dev = model.double(), torch.device("cpu")
    else:
        model, dev = model.to(DEV), DEV
    net = tc.training_module(model, dev, bn_train.every_shape) if mode == "fused" else model
    net.train()
    logits = net(x.to(dev, next(model.parameters()).dtype))
    loss = bn_train.softmax_cross_entropy(logits, t.to(dev), bn_train.every_shape)[0] if mode == "fused" else F.cross_entropy(logits, t.to(dev))
    loss.backward()
    assert all((p.grad is not None) == p.requires_grad for p in model.parameters())
    return {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("arch", ["mobilenet_v2", "resnet18"])
def test_network_gradients_after_one_backward(arch):
    ref, plain, fused = (network_grads(arch, mode) for mode in ("f64", "plain", "fused"))
    assert list(ref) == list(plain) == list(fused)
    rel_p, rel_f, worst, tiny, gauge = [], [], [], [0, 0.0, 0.0], []
    for n in ref:
        scale = float(ref[n].abs().max())
        dp, df = (plain[n] - ref[n]).abs(), (fused[n] - ref[n]).abs()
        if scale < 1e-12:  # zero in exact arithmetic
            gauge.append((n, float(df.max()), float(dp.max())))
            continue
        rel_p.append((dp / scale).reshape(-1))
        rel_f.append((df / scale).reshape(-1))
        worst.append((float(df.max()) / (2 * float(dp.max()) + U * scale), n, float(df.max()) / scale, float(dp.max()) / scale))
        small = (ref[n].abs() < 1e-7) & (ref[n] != 0)  # where Adam's g / (|g| + 1e-8) is sensitive to an absolute error of 1e-8
        tiny = [tiny[0] + int(small.sum()), tiny[1] + float(dp[small].sum()), tiny[2] + float(df[small].sum())]
    rel_p, rel_f = torch.cat(rel_p), torch.cat(rel_f)
    e_p, e_f = float(rel_p.norm()), float(rel_f.norm())
    rnd = U * rel_f.numel() ** 0.5
    worst.sort(reverse=True)
    lines = ["# tests/test_bn_train_grads_gpu.py, %s: parameter gradients after one backward (64 px, B = 16), error / max |float64 gradient| per tensor" % arch,
             "%-13s %d trainable elements, Euclidean: fused %.3e  plain %.3e  fused / (2 plain + rounding) %.3f;  maximum: fused %.3e  plain %.3e"
             % (arch, rel_f.numel(), e_f, e_p, e_f / (2 * e_p + rnd), float(rel_f.max()), float(rel_p.max())),
             "%-13s %d elements with 0 < |float64 gradient| < 1e-7: mean absolute error fused %.3e  plain %.3e"
             % (arch, tiny[0], tiny[2] / max(tiny[0], 1), tiny[1] / max(tiny[0], 1))]
    lines += ["%-13s worst tensor %-34s fused / (2 plain + rounding) %.3f  (fused %.3e  plain %.3e)" % ((arch, w[1], w[0]) + w[2:]) for w in worst[:4]]
    lines += ["%-13s zero in exact arithmetic: %-30s largest fp32 gradient fused %.3e  plain %.3e" % ((arch,) + g) for g in gauge]
    record(lines)
    assert all(g[1] < 1e-6 and g[2] < 1e-6 for g in gauge), lines
    assert (len(gauge) > 0) == (arch == "mobilenet_v2")
    assert e_f <= 2 * e_p + rnd, lines
    assert worst[0][0] <= 5.0, lines  # no single tensor 10 times worse than plain (2 plain + rounding, times 5)
