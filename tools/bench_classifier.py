"""Classifier training (stylex/train_classifier.py): the fused batch-norm / activation / cross-entropy path (csrc/bn_train.hip)
against plain torch on the same GPU in the same process, device time by hipEvents.

* per launch group: every distinct (B, C, H, W, act, residual) BatchNormAct call of the network at the workload shape, forward
  + backward, fused module against F.batch_norm + activation (+ add) under autograd;
* the cross-entropy forward + backward against F.cross_entropy;
* per step: zero_grad / forward / loss / backward / Adam step of the whole network, fused module against the plain tv_models one.

Every pair is timed A / B / B / A (fused, plain, plain, fused; median of --rounds each) and the two halves are averaged, so a
drift of the clock or of a neighbour's load falls on both sides.  Workloads: MobileNetV2 at 224 px, B = 200, 15 layers frozen;
ResNet-18 at 224 px, B = 128 (the reference's two recipes).  Weights random:1 (the time does not depend on their values).

    python tools/bench_classifier.py [--out profiles/classifier_train_timing.txt] [--rounds 5] [--archs mobilenet_v2,resnet18]
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

import hip_backend as hb  # noqa: E402,F401  (before the first convolution)
import bn_train  # noqa: E402
import train_classifier as tc  # noqa: E402

WORKLOADS = {"mobilenet_v2": dict(batch=200, frozen=15), "resnet18": dict(batch=128, frozen=0)}


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


def abba(fused, plain, rounds):
    a1, b1, b2, a2 = device_ms(fused, rounds), device_ms(plain, rounds), device_ms(plain, rounds), device_ms(fused, rounds)
    return (a1 + a2) / 2, (b1 + b2) / 2


def collect_groups(net, x):
    """(shape, act, residual?, input needs grad?, parameters need grad?) of every BatchNormAct call, with its count."""
    seen = {}

    def hook(m, args, kwargs):
        res = args[1] if len(args) > 1 else kwargs.get("residual")
        key = (tuple(args[0].shape), m.act, res is not None, bool(args[0].requires_grad), bool(m.weight.requires_grad))
        seen[key] = seen.get(key, 0) + 1

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in net.modules() if isinstance(m, bn_train.BatchNormAct)]
    net.train()
    net(x)
    for h in hs:
        h.remove()
    return seen


def group_pair(key, dev):
    shape, act, has_res, x_grad, p_grad = key
    m = bn_train.BatchNormAct(shape[1], act=act).to(dev).train()
    m.shape_rule = bn_train.every_shape  # the measurement behind bn_train.measured_shape_rule: every shape on the kernels
    for p in m.parameters():
        p.requires_grad_(p_grad)
    x = torch.randn(shape, device=dev).add_(1).requires_grad_(x_grad)
    res = torch.randn(shape, device=dev).requires_grad_(x_grad) if has_res else None
    gy = torch.randn(shape, device=dev)
    wants = [t for t in (x, res, m.weight, m.bias) if t is not None and t.requires_grad]

    def fused():
        y = m(x, res)
        if wants:
            torch.autograd.grad(y, wants, gy)

    def plain():
        y = F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, True, m.momentum, m.eps)
        y = bn_train._activate(y if res is None else y + res, act)
        if wants:
            torch.autograd.grad(y, wants, gy)

    return fused, plain


def step_fns(arch, dev, size):
    """One training step three ways: the fused module under the measured shape rule (what train_classifier.py runs), the fused
    module with every shape on the kernels, the plain module."""
    w = WORKLOADS[arch]
    fns = []
    for fused, rule in ((True, None), (True, bn_train.every_shape), (False, None)):
        model = tc.build_model(arch, "random:1", amount_frozen_layers=w["frozen"]).to(dev)
        net = tc.training_module(model, dev, rule) if fused else model
        net.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)
        x = torch.randn(w["batch"], 3, size, size, device=dev)
        t = torch.randint(0, 2, (w["batch"],), device=dev)

        def step(net=net, opt=opt, x=x, t=t, fused=fused):
            loss = bn_train.softmax_cross_entropy(net(x), t)[0] if fused else F.cross_entropy(net(x), t)
            opt.zero_grad()
            loss.backward()
            opt.step()

        fns.append((step, net, x))
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--archs", default="mobilenet_v2,resnet18")
    ap.add_argument("--image_size", type=int, default=224)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_classifier.py measures on the GPU; there is no CPU figure"
    dev = torch.device("cuda:0")
    lines = ["# tools/bench_classifier.py: device time (hipEvents, median of %d per leg, A/B/B/A), %s" % (a.rounds, torch.cuda.get_device_name(0))]
    for arch in a.archs.split(","):
        w = WORKLOADS[arch]
        (f_step, f_net, x), (a_step, a_net, _), (p_step, _, _) = step_fns(arch, dev, a.image_size)
        lines.append("## %s, %d px, B = %d, %d feature layers frozen" % (arch, a.image_size, w["batch"], w["frozen"]))
        tf, tp = abba(f_step, p_step, a.rounds)
        lines.append("%-64s fused %9.3f ms  plain %9.3f ms  fused / plain %.3f" % ("training step, measured shape rule (the default)", tf, tp, tf / tp))
        ta, tp = abba(a_step, p_step, a.rounds)
        lines.append("%-64s fused %9.3f ms  plain %9.3f ms  fused / plain %.3f" % ("training step, every shape on the kernels", ta, tp, ta / tp))
        lines.append("# per group, every shape on the kernels (a row marked ATEN is one the measured shape rule hands to ATen):")
        groups = collect_groups(a_net, x)
        sum_f = sum_p = 0.0
        for key in sorted(groups):
            fused, plain = group_pair(key, dev)
            gf, gp = abba(fused, plain, a.rounds)
            sum_f, sum_p = sum_f + gf * groups[key], sum_p + gp * groups[key]
            shape, act, has_res, x_grad, p_grad = key
            what = "%s %-5s%s%s x%d" % ("x".join(str(v) for v in shape), act, " +res" if has_res else "",
                                        "" if x_grad or p_grad else " (frozen: forward only)", groups[key])
            on_aten = not bn_train.measured_shape_rule(shape[0], shape[1], shape[2] * shape[3], x_grad or p_grad)
            lines.append("%-64s fused %9.3f ms  plain %9.3f ms  fused / plain %.3f%s%s"
                         % (what, gf, gp, gf / gp, "  SLOWER" if gf > gp else "", "  ATEN" if on_aten else ""))
        lines.append("%-64s fused %9.3f ms  plain %9.3f ms  fused / plain %.3f" % ("all normalisation groups of one step (sum of the rows above)", sum_f, sum_p, sum_f / sum_p))
        for b, k in ((w["batch"], 2), (w["batch"], 1000), (4096, 1000)):
            z = torch.randn(b, k, device=dev, requires_grad=True)
            t = torch.randint(0, k, (b,), device=dev)

            def plain_ce(z=z, t=t):
                torch.autograd.grad(F.cross_entropy(z, t), z)
                return (torch.argmax(z.detach(), dim=1) == t).sum()

            cf, cp = abba(lambda: torch.autograd.grad(bn_train.softmax_cross_entropy(z, t, bn_train.every_shape)[0], z), plain_ce, a.rounds)
            lines.append("%-64s fused %9.3f ms  plain %9.3f ms  fused / plain %.3f%s%s"
                         % ("cross-entropy + correct count, forward + backward, %d x %d" % (b, k), cf, cp, cf / cp,
                            "  SLOWER" if cf > cp else "", "" if bn_train.measured_ce_rule(b, k) else "  ATEN"))
        del f_step, a_step, p_step, f_net, a_net, x
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
