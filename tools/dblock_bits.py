"""SHA-256 of everything the fused DiscriminatorBlock and the gradient-penalty tangent pass compute, for comparing two
trees bit for bit on ONE machine (the residual GEMM goes through hipBLASLt, whose algorithm choice may differ between
machines).  Cases: the fused side of tests/test_hip_parity.py::test_fused_dblock_matches_composable_path, both sides of
::test_fused_dblock_with_and_without_bit_masks, and DiscriminatorE(64) at batch 4 through gp_tangent in bf16 and fp32 with
STYLEX_RES_FOLD at its default and 0.      python tools/dblock_bits.py [--tree ROOT_OF_ANOTHER_CHECKOUT]"""
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


def sha(t):
    if t is None:
        return "none"
    t = t.detach().contiguous().cpu()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:32] + " %s%s" % (
        str(t.dtype).replace("torch.", ""), list(t.shape))


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def block_case(tag, cin, cout, size, down, seeds):
    torch.manual_seed(seeds[0])
    blk = st.DiscriminatorBlock(cin, cout, downsample=down).to(DEV)
    xr = torch.randn(3, cin, size, size, device=DEV, generator=gen(seeds[1])).requires_grad_()
    prev = ops.set_fast(True)
    try:
        y = blk(xr)
        r = torch.randn(y.shape, device=DEV, generator=gen(seeds[2])).to(y.dtype)
        (y.float() * r.float()).sum().backward()
    finally:
        ops.set_fast(prev)
    for name, t in [("out", y), ("gx", xr.grad)] + [("g." + n, p.grad) for n, p in blk.named_parameters()]:
        print(tag, name, sha(t))


def tangent_case(tag, prec):
    ops.set_precision(prec)
    torch.manual_seed(21)
    D = st.DiscriminatorE(64, network_capacity=16, fmap_max=512).to(DEV)
    with torch.no_grad():
        for p in D.parameters():  # biases away from zero, weights as initialised
            if p.dim() == 1:
                p.normal_(0, 0.1)
    real = torch.rand(4, 3, 64, 64, device=DEV, generator=gen(5))
    a = torch.tensor([1.0, 0.0, 1.0, 1.0], device=DEV) / 4
    assert gp_tangent.supported(D, real)
    ops.set_fast(True)
    try:
        out, norms = gp_tangent.d_real_with_norms(D, real)
    finally:
        ops.set_fast(False)
    ((out.float() * a).sum() + 10 * ((norms - 1) ** 2).mean()).backward()
    for name, t in [("out", out), ("norms", norms)] + [("g." + n, p.grad) for n, p in D.named_parameters()]:
        print(tag, name, sha(t))


def main():
    hb.load_library()
    for prec in ("fp32", "bf16"):
        ops.set_precision(prec)
        for cin, cout, size, down in [(3, 64, 64, True), (64, 64, 64, True), (64, 128, 32, True), (32, 48, 16, True),
                                      (64, 64, 8, True), (64, 64, 2, False)]:
            block_case("block %s %d->%d@%d%s" % (prec, cin, cout, size, "" if down else " last"), cin, cout, size, down,
                       (11, 12, 13))
    ops.set_precision("bf16")
    os.environ["STYLEX_GATE_MASK_MIN_PIXELS"] = "0"  # masks at 64^2 as well
    for cin, cout, size in ((3, 64, 64), (64, 128, 64)):
        for masks in ("1", "0"):
            os.environ["STYLEX_GATE_MASK"] = masks
            block_case("masks=%s %d->%d@%d" % (masks, cin, cout, size), cin, cout, size, True, (21, 22, 23))
    del os.environ["STYLEX_GATE_MASK"], os.environ["STYLEX_GATE_MASK_MIN_PIXELS"]
    os.environ["STYLEX_GP_TANGENT"] = "2"  # the tangent pass in any precision
    for fold in (None, "0"):
        if fold is not None:
            os.environ["STYLEX_RES_FOLD"] = fold
        for prec in ("bf16", "fp32"):
            tangent_case("tangent %s res_fold=%s" % (prec, "default" if fold is None else fold), prec)


if __name__ == "__main__":
    main()
