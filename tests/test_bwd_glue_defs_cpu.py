"""The float64 definitions of tests/_bwd_glue_defs.py against autograd of the compositions they are the backward of (CPU).
The GPU tests compare the kernels of csrc/fused_bwd.hip with these definitions; this file is what ties the definitions to
the network's formulas: y = lrelu(d * z + plane * nw + nb) (GeneratorBlock), lrelu((conv + res) * scale) (DiscriminatorBlock)
and x * s (Conv2DMod's modulation)."""
import pytest
import torch

import _bwd_glue_defs as D

F64 = torch.float64
TOL = 1e-12


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def lrelu64(p):
    return torch.where(p > 0, p, 0.2 * p)


@pytest.mark.parametrize("shape,ns", [((3, 12, 9, 7), 10), ((2, 8, 5, 11), 11), ((1, 4, 6, 6), 6)])
@pytest.mark.parametrize("lrelu", [True, False])
def test_modconv_prep_is_the_backward_of_the_noise_activation(shape, ns, lrelu):
    """S0 / d, sum_b S1, sum_b S2 and the stored gz * d are autograd's gradients of sum(gy * act(d*z + plane*nw + nb)) with
    respect to d, nw, nb and z — the plane read transposed, on non-square shapes cropped from a larger plane."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(11)
    z = torch.randn(B, C, H, W, dtype=F64, generator=g).requires_grad_()
    d = (torch.rand(B, C, dtype=F64, generator=g) + 0.5).requires_grad_()
    nw, nb = (torch.randn(C, dtype=F64, generator=g).requires_grad_() for _ in range(2))
    noise = torch.rand(B, ns, ns, dtype=F64, generator=g)
    gy = torch.randn(B, C, H, W, dtype=F64, generator=g)
    plane = torch.empty(B, H, W, dtype=F64)
    for h in range(H):
        for w in range(W):
            plane[:, h, w] = noise[:, w, h]
    pre = d[:, :, None, None] * z + plane[:, None] * nw.view(1, C, 1, 1) + nb.view(1, C, 1, 1)
    y = lrelu64(pre) if lrelu else pre
    gz_, gd, gnw, gnb = torch.autograd.grad((gy * y).sum(), [z, d, nw, nb])
    r = D.modconv_prep(gy, y.detach(), noise, nw.detach(), nb.detach(), lrelu, d.detach())
    assert rel(r.S[:, 0] / d.detach(), gd) <= TOL
    assert rel(r.S[:, 1].sum(0), gnw) <= TOL
    assert rel(r.S[:, 2].sum(0), gnb) <= TOL
    assert rel(r.gz, gz_) <= TOL
    # without d the stored tensor is the gradient with respect to the pre-activation; the sums do not change
    r1 = D.modconv_prep(gy, y.detach(), noise, nw.detach(), nb.detach(), lrelu, None)
    assert rel(r1.gz * d.detach()[:, :, None, None], gz_) <= TOL and torch.equal(r1.S, r.S)
    assert (r.abs_S >= r.S.abs() - 1e-12).all()


def test_modconv_prep_without_noise():
    B, C, H, W = 2, 4, 3, 5
    g = torch.Generator().manual_seed(12)
    z = torch.randn(B, C, H, W, dtype=F64, generator=g)
    d = (torch.rand(B, C, dtype=F64, generator=g) + 0.5).requires_grad_()
    gy = torch.randn(B, C, H, W, dtype=F64, generator=g)
    y = lrelu64(d[:, :, None, None] * z)
    gd, = torch.autograd.grad((gy * y).sum(), [d])
    r = D.modconv_prep(gy, y.detach(), None, None, None, True, None)
    assert rel(r.S[:, 0] / d.detach(), gd) <= TOL
    assert r.S[:, 1].abs().max() == 0
    with pytest.raises(AssertionError):
        D.modconv_prep(gy, y.detach(), None, None, None, "relu", None)


@pytest.mark.parametrize("mode", ["none", "lrelu", "relu"])
def test_act_bwd_is_the_backward_of_the_scaled_activation(mode):
    """dx and its sums against autograd of act((p + bias) * scale): gradient wrt p, and wrt bias per channel / per sample."""
    B, C, H, W = 3, 8, 5, 7
    g = torch.Generator().manual_seed(13)
    p = torch.randn(B, C, H, W, dtype=F64, generator=g).requires_grad_()
    bias = torch.zeros(C, dtype=F64, requires_grad=True)
    bias_bc = torch.zeros(B, C, dtype=F64, requires_grad=True)
    dy = torch.randn(B, C, H, W, dtype=F64, generator=g)
    scale = 2 ** -0.5
    pre = (p + bias.view(1, C, 1, 1) + bias_bc[:, :, None, None]) * scale
    y = {"none": pre, "lrelu": lrelu64(pre), "relu": pre.clamp_min(0)}[mode]
    gp, gb, gbc = torch.autograd.grad((dy * y).sum(), [p, bias, bias_bc])
    r = D.act_bwd(dy, None if mode == "none" else y.detach(), mode, scale)
    assert rel(r.dx, gp) <= TOL and rel(r.sum_bhw, gb) <= TOL and rel(r.sum_hw, gbc) <= TOL
    assert rel(r.abs_bhw, gp.abs().sum(dim=(0, 2, 3))) <= TOL and rel(r.abs_hw, gp.abs().sum(dim=(2, 3))) <= TOL


def test_gate_takes_the_slope_at_both_zeros_in_float64():
    y = torch.tensor([0.0, -0.0, 1e-30, -1e-30], dtype=torch.bfloat16)
    assert D.gate(y, True).dtype == F64
    assert D.gate(y, True).tolist() == [0.2, 0.2, 1.0, 0.2]  # the float64 0.2, not float32's
    assert D.gate(y, "relu").tolist() == [0.0, 0.0, 1.0, 0.0]
    assert D.gate(y, False) is None and D.gate(y, "none") is None


def test_scale_reduce_is_the_backward_of_the_modulation():
    B, C, H, W = 2, 12, 4, 6
    g = torch.Generator().manual_seed(14)
    x = torch.randn(B, C, H, W, dtype=F64, generator=g).requires_grad_()
    s = (torch.rand(B, C, dtype=F64, generator=g) + 0.5).requires_grad_()
    t = torch.randn(B, C, H, W, dtype=F64, generator=g)  # the gradient arriving at x * s
    gx, gs = torch.autograd.grad((t * (x * s[:, :, None, None])).sum(), [x, s])
    r = D.scale_reduce(x.detach(), t, s.detach())
    assert rel(r.gx, gx) <= TOL and rel(r.sum_hw, gs) <= TOL
    assert rel(r.abs_hw, (x.detach() * t).abs().sum(dim=(2, 3))) <= TOL
