"""SHA-256 of everything the fused modulated conv (ops._ModConvFast) computes, for comparing two trees bit for bit on ONE
machine.  Cases: ops.modconv_noise_act over MODCONV_CASES of tests/test_bwd_glue_gpu.py in fp32, bf16 and bf16 with
STYLEX_FOLD_D=0; ops.modulated_conv2d without noise (12->12 3x3 demodulated; the 16->3 1x1 to-RGB conv: padded fused
route in fp32, streaming kernel in bf16); a whole Generator(64) forward with style coordinates and backward on the fast
path in both precisions, once more with STYLEX_NOISE_NAT=0.
python tools/modconv_bits.py [--tree ROOT_OF_ANOTHER_CHECKOUT]"""
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

import hip_backend as hb  # noqa: E402
import networks  # noqa: E402
import ops  # noqa: E402

DEV = "cuda:0"
MODCONV_CASES = [(3, 12, 12, 9, 9, 12), (2, 40, 40, 10, 13, 16), (2, 64, 40, 8, 8, 8), (2, 6, 12, 9, 9, 9),
                 (16, 512, 512, 4, 4, 4)]  # B, Cin, Cout, H, W, side of the noise plane


def sha(t):
    if t is None:
        return "none"
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:32] + " %s%s" % (
        str(t.dtype).replace("torch.", ""), list(t.shape))


def rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=g) * scale).requires_grad_()


def report(tag, y, named, extra=0.0):
    r = torch.randn(y.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(y.dtype)
    ((y.float() * r.float()).sum() + extra).backward()
    for name, t in [("out", y)] + [("g." + n, p.grad) for n, p in named]:
        print(tag, name, sha(t))


def conv_case(tag, case, k, demod, noise):
    B, ci, co, H, W, side = case
    g = torch.Generator(device=DEV).manual_seed(7)
    x, style, w = rand(g, B, ci, H, W), rand(g, B, ci, scale=0.5), rand(g, co, ci, k, k, scale=(ci * k * k) ** -0.5)
    named = [("x", x), ("style", style), ("W", w)]
    if noise:
        nw, nb, inoise = rand(g, co), rand(g, co), torch.rand(B, side, side, 1, device=DEV, generator=g)
        y = ops.modconv_noise_act(x, style, w, inoise, nw, nb)
        named += [("nw", nw), ("nb", nb)]
    else:
        y = ops.modulated_conv2d(x, style, w, demod=demod)
    report(tag, y, named)


def generator_case(tag):
    torch.manual_seed(31)
    G = networks.Generator(64, latent_dim=512, network_capacity=16).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(9)
    styles, inoise = rand(g, 2, G.num_layers, 512), torch.rand(2, 64, 64, 1, device=DEV, generator=g)
    img, coords = G(styles, inoise, get_style_coords=True)
    print(tag, "coords", sha(coords))
    report(tag, img, [("styles", styles)] + list(G.named_parameters()), extra=coords.float().square().sum() * 1e-3)


def main():
    hb.load_library()
    ops.set_fast(True)
    for prec, fold in (("fp32", None), ("bf16", None), ("bf16", "0")):
        ops.set_precision(prec)
        if fold is not None:
            os.environ["STYLEX_FOLD_D"] = fold
        for case in MODCONV_CASES:
            conv_case("modconv %s fold=%s %s" % (prec, fold or "default", "x".join(map(str, case))), case, 3, True, True)
        os.environ.pop("STYLEX_FOLD_D", None)
    for prec in ("fp32", "bf16"):
        ops.set_precision(prec)
        conv_case("conv3x3 %s 12->12 demod" % prec, (3, 12, 12, 9, 9, 0), 3, True, False)
        conv_case("torgb %s 16->3" % prec, (3, 16, 3, 8, 8, 0), 1, False, False)
    for nat in (None, "0"):
        if nat is not None:
            os.environ["STYLEX_NOISE_NAT"] = nat
        for prec in ("fp32", "bf16"):
            ops.set_precision(prec)
            generator_case("generator %s noise_nat=%s" % (prec, nat or "default"))


if __name__ == "__main__":
    main()
