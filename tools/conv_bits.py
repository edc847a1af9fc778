"""SHA-256 of everything the plain conv path computes (ops.conv2d, ops.blur_down: ops._conv_plan, the _Conv / _Dgrad / _Wgrad
triad, _ConvBiasActFast / _ConvBiasActDD), for comparing two trees bit for bit on ONE machine (the 1x1 GEMM route goes
through hipBLASLt, whose algorithm choice may differ between machines).  Cases, each in fp32 and bf16: the routes of
ops.conv2d and ops.blur_down under set_fast True and False; double backward (the gradient-penalty form) through a two-layer
stack and a 64-channel stack ending in blur_down, once more in bf16 with STYLEX_RES_GEMM_DD=0; a whole DiscriminatorE(64)
first order, one gradient-penalty step on it by double backward and by the tangent pass; one block used twice in one backward.
python tools/conv_bits.py [--tree ROOT_OF_ANOTHER_CHECKOUT]"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(ap.parse_args().tree)
PKG = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(PKG, "stylex")]

import torch  # noqa: E402

import gp_tangent  # noqa: E402
import hip_backend as hb  # noqa: E402
import ops  # noqa: E402
import stylex_train as st  # noqa: E402

DEV = "cuda:0"
# tag, (B, C, N, H, W), kernel, stride, pad, bias, lrelu, residual scale (None: no residual)
CONV_CASES = [("3x3 bias lrelu", (2, 16, 16, 9, 9), 3, 1, 1, True, True, None),
              ("3x3 residual 0.7", (2, 16, 16, 9, 9), 3, 1, 1, True, False, 0.7),
              ("1x1 stride 2", (2, 16, 32, 12, 12), 1, 2, 0, True, False, None),
              ("3x3 rgb in", (2, 3, 16, 8, 8), 3, 1, 1, True, True, None),
              ("1x1 rgb out bias", (2, 16, 3, 8, 8), 1, 1, 0, True, False, None),
              ("1x1 rgb out lrelu", (2, 16, 3, 8, 8), 1, 1, 0, True, True, None),
              # LPIPS-AlexNet's first two layers; as in a frozen network only the input takes a gradient.  (The library
              # refuses the first through ops.conv2d, the same printed line in either tree: the product runs it as _StemBf16.)
              ("11x11 stride 4 relu frozen", (2, 3, 64, 35, 35), 11, 4, 2, True, "relu", None),
              ("5x5 relu frozen", (2, 64, 192, 7, 7), 5, 1, 2, True, "relu", None)]
BLUR_CASES = [(1, 64, 64, 32, 32), (1, 128, 64, 48, 80), (2, 64, 64, 16, 16)]  # the last: not space-to-depth


def sha(t):
    if t is None:
        return "none"
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:32] + " %s%s" % (
        str(t.dtype).replace("torch.", ""), list(t.shape))


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=g) * scale).requires_grad_()


def report(tag, y, named):
    r = torch.randn(y.shape, device=DEV, generator=gen(3)).to(y.dtype)
    (y.float() * r.float()).sum().backward()
    show(tag, [("out", y)] + [("g." + n, p.grad) for n, p in named])


def show(tag, named):
    for name, t in named:
        print(tag, name, sha(t))


def conv_case(tag, case, k, stride, pad, bias, lrelu, res_scale):
    B, C, N, H, W = case
    g = gen(7)
    named = [("x", rand(g, B, C, H, W)), ("W", rand(g, N, C, k, k, scale=(C * k * k) ** -0.5))]
    b = rand(g, N) if bias else None
    if "frozen" in tag:
        named, b = [named[0], ("W", named[1][1].detach())], b.detach()
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = rand(g, B, N, ho, wo) if res_scale is not None else None
    y = ops.conv2d(named[0][1], named[1][1], b, stride, pad, lrelu=lrelu, residual=res, res_scale=res_scale or 1.0)
    report(tag, y, named + [(n, t) for n, t in (("b", b), ("res", res)) if t is not None])


def blur_case(tag, case):
    B, C, N, H, W = case
    g = gen(8)
    named = [("x", rand(g, B, C, H, W)), ("W", rand(g, N, C, 3, 3, scale=(C * 9) ** -0.5)), ("b", rand(g, N)),
             ("res", rand(g, B, N, H // 2, W // 2))]
    report(tag, ops.blur_down(*[t for _, t in named], 0.7), named)


def penalty_case(tag, wide):
    """Double backward: the gradient-penalty form through a stack of plain convs, parameter and input gradients hashed."""
    g = gen(11)
    if wide:   # the composable DiscriminatorBlock: 1x1 / stride-2 residual path, 3x3 + lrelu, blur_down with the merge
        x = rand(g, 1, 64, 32, 32)
        named = [("x", x), ("Wr", rand(g, 64, 64, 1, 1, scale=1 / 8)), ("br", rand(g, 64)),
                 ("W1", rand(g, 64, 64, 3, 3, scale=1 / 24)), ("b1", rand(g, 64)),
                 ("W3", rand(g, 64, 64, 3, 3, scale=1 / 24)), ("b3", rand(g, 64))]
        _, wr, br, w1, b1, w3, b3 = [t for _, t in named]
        y = ops.blur_down(ops.conv2d(x, w1, b1, 1, 1, lrelu=True), w3, b3, ops.conv2d(x, wr, br, stride=2), 0.7)
    else:      # 1x1 with bias (the GEMM route in bf16), then 3x3 + lrelu
        x = rand(g, 2, 16, 8, 8)
        named = [("x", x), ("W1", rand(g, 16, 16, 1, 1, scale=1 / 4)), ("b1", rand(g, 16)),
                 ("W2", rand(g, 16, 16, 3, 3, scale=1 / 12))]
        _, w1, b1, w2 = [t for _, t in named]
        y = ops.conv2d(ops.conv2d(x, w1, b1), w2, None, 1, 1, lrelu=True)
    norms = st.gradient_norms(x, y)
    norms.mean().backward()
    show(tag, [("out", y), ("norms", norms)] + [("g." + n, p.grad) for n, p in named])


def discriminator(seed=21):
    torch.manual_seed(seed)
    D = st.DiscriminatorE(64, network_capacity=16, fmap_max=512).to(DEV)
    with torch.no_grad():
        for p in D.parameters():  # biases away from zero, weights as initialised
            if p.dim() == 1:
                p.normal_(0, 0.1)
    return D, torch.rand(4, 3, 64, 64, device=DEV, generator=gen(5))


def d_first_order(tag):
    D, real = discriminator()
    real.requires_grad_()
    ops.set_fast(True)
    out = D(real)
    (out.float() * torch.tensor([1.0, -0.5, 0.25, 1.0], device=DEV)).sum().backward()
    show(tag, [("out", out), ("g.real", real.grad)] + [("g." + n, p.grad) for n, p in D.named_parameters()])


def d_penalty(tag, tangent):
    D, real = discriminator()
    if tangent:
        if not gp_tangent.supported(D, real):
            print(tag, "not supported")
            return
        ops.set_fast(True)
        out, norms = gp_tangent.d_real_with_norms(D, real)
        ops.set_fast(False)
    else:
        ops.set_fast(False)
        real.requires_grad_()
        out = D(real)
        norms = st.gradient_norms(real, out)
    (out.float().mean() + 10 * ((norms - 1) ** 2).mean()).backward()
    show(tag, [("out", out), ("norms", norms)] + [("g." + n, p.grad) for n, p in D.named_parameters()])


def twice_used_block(tag):
    """Encoder-style: one block in two branches of ONE backward (gradients added inside the weight-gradient launches)."""
    torch.manual_seed(31)
    blk = st.DiscriminatorBlock(64, 64, downsample=True).to(DEV)
    g = gen(12)
    x1, x2 = rand(g, 2, 64, 32, 32), rand(g, 2, 64, 32, 32)
    ops.set_fast(True)
    y1, y2 = blk(x1), blk(x2)
    r = torch.randn(y1.shape, device=DEV, generator=gen(13)).to(y1.dtype)
    ((y1.float() * r.float()).sum() + (y2.float() * r.float()).sum() * 0.5).backward()
    show(tag, [("out1", y1), ("out2", y2), ("g.x1", x1.grad), ("g.x2", x2.grad)] +
         [("g." + n, p.grad) for n, p in blk.named_parameters()])


def main():
    hb.load_library()
    for prec in ("fp32", "bf16"):
        ops.set_precision(prec)
        for fast in (True, False):
            ops.set_fast(fast)
            for tag, *case in CONV_CASES:
                try:
                    conv_case("conv2d %s fast=%d %s" % (prec, fast, tag), *case)
                except (hb.StylexHipError, AssertionError) as e:  # a form this mode does not run: the same line in both trees
                    print("conv2d %s fast=%d %s" % (prec, fast, tag), "refused:", type(e).__name__)
            for case in BLUR_CASES:
                blur_case("blur_down %s fast=%d %s" % (prec, fast, "x".join(map(str, case))), case)
    ops.set_fast(False)
    for prec, dd in (("fp32", None), ("bf16", None), ("bf16", "0")):
        ops.set_precision(prec)
        if dd is not None:
            os.environ["STYLEX_RES_GEMM_DD"] = dd
        for wide in (False, True):
            penalty_case("penalty %s gemm_dd=%s %s" % (prec, dd or "default", "64ch blur_down" if wide else "1x1 3x3"), wide)
        os.environ.pop("STYLEX_RES_GEMM_DD", None)
    os.environ["STYLEX_GP_TANGENT"] = "2"  # the tangent pass in any precision
    for prec in ("fp32", "bf16"):
        ops.set_precision(prec)
        d_first_order("D64 %s first order" % prec)
        d_penalty("D64 %s penalty double backward" % prec, False)
        d_penalty("D64 %s penalty tangent" % prec, True)
        twice_used_block("block twice %s" % prec)
    ops.set_fast(False)


if __name__ == "__main__":
    main()
