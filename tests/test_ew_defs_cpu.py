"""The float64 definitions of tests/_ew_defs.py against the reference's formulas (CPU): the oracle's blur / bilinear x2 (both
the executed and the explicit-index forms), the outputs recorded from the reference (tests/golden/ops.npz), float64 autograd
for every adjoint and gradient, and the per-sample-weight grouped convolution for to-RGB.  The GPU tests compare the kernels
of csrc/elementwise.hip and csrc/torgb.hip with these definitions; this file is what ties the definitions to the network.

Bound: 1e-12 relative to the reference's max-abs (float64 against float64, as tests/test_bwd_glue_defs_cpu.py).  The one
exception is ops.npz, which holds fp32 results of an fp32 evaluation: there the bound is the oracle's own against that file,
1e-6 of max(1, max-abs) (tests/test_oracle_vs_golden.py)."""
import pytest
import torch
import torch.nn.functional as F

import _ew_defs as D
import stylex_oracle as so
from conftest import load_golden

F64 = torch.float64
TOL = 1e-12
SHAPES = [(2, 3, 2, 2), (1, 4, 2, 5), (2, 5, 7, 3), (3, 2, 8, 6), (1, 1, 9, 9)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def rel(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rnd(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def dominates(s):
    assert (s.abs_terms >= s.value.abs() * (1 - 1e-12)).all(), "abs_terms < |result|"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_blur_and_x2_are_the_oracles(shape):
    x = rnd(*shape, seed=1)
    for got, refs in ((D.blur(x), (so.blur3x3_reflect(x), so.blur3x3_reflect_explicit(x))),
                      (D.up2(x), (so.upsample2x_bilinear(x), so.upsample2x_bilinear_explicit(x)))):
        for ref in refs:
            assert rel(got.value, ref) <= TOL
        dominates(got)
    assert rel(D.blur(x.abs()).value, D.blur(x).abs_terms) <= TOL and rel(D.up2(x.abs()).value, D.up2(x).abs_terms) <= TOL


def test_blur_and_x2_against_the_recorded_reference_outputs():
    g = load_golden("ops")
    for key, fn, adj in (("blur", D.blur, D.blur_adj), ("up", D.up2, D.up2_adj)):
        x, y = torch.from_numpy(g[key + "/x"]), torch.from_numpy(g[key + "/y"]).double()
        got = fn(x).value
        assert got.shape == y.shape
        assert (got - y).abs().max().item() <= 1e-6 * max(1.0, y.abs().max().item()), key
        # the recorded backward: gx = the reference's own gradient of sum(y * r)
        r, gx = torch.from_numpy(g[key + "/r"]), torch.from_numpy(g[key + "/gx"]).double()
        got = adj(r).value
        assert got.shape == gx.shape
        assert (got - gx).abs().max().item() <= 1e-6 * max(1.0, gx.abs().max().item()), key + " adjoint"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_adjoints_are_autograd_of_the_forwards(shape):
    b, c, h, w = shape
    x = rnd(*shape, seed=2).requires_grad_()
    for fwd, adj, scale in ((so.blur3x3_reflect, D.blur_adj, 1), (so.upsample2x_bilinear, D.up2_adj, 2)):
        dy = rnd(b, c, scale * h, scale * w, seed=3)
        gx, = torch.autograd.grad((fwd(x) * dy).sum(), [x])
        got = adj(dy)
        assert rel(got.value, gx) <= TOL
        dominates(got)
        assert rel(adj(dy.abs()).value, got.abs_terms) <= TOL


@pytest.mark.parametrize("shape", [(1, 8, 1, 1), (3, 4, 4, 4), (2, 3, 5, 7), (1, 4, 2, 1), (2, 4, 8, 16)],
                         ids=["1x8x1x1", "3x4x4x4", "2x3x5x7", "1x4x2x1", "2x4x8x16"])
@pytest.mark.parametrize("with_prev", [True, False], ids=["prev", "no-prev"])
def test_rgb_tail_is_blur_of_the_interpolation(shape, with_prev):
    b, c, h, w = shape
    rgb = rnd(*shape, seed=4).requires_grad_()
    prev = rnd(*shape, seed=5).requires_grad_() if with_prev else None
    s = rgb + prev if with_prev else rgb
    ref = so.blur3x3_reflect(F.interpolate(s, scale_factor=2, mode="bilinear", align_corners=False))
    got = D.rgb_tail(rgb.detach(), prev.detach() if with_prev else None)
    assert rel(got.value, ref) <= TOL
    dominates(got)
    assert rel(got.value, D.blur(D.up2(s.detach()).value).value) <= TOL
    dy = rnd(b, c, 2 * h, 2 * w, seed=6)
    grads = torch.autograd.grad((ref * dy).sum(), [rgb, prev] if with_prev else [rgb])
    adj = D.rgb_tail_adj(dy)
    for gr in grads:
        assert rel(adj.value, gr) <= TOL
    dominates(adj)
    assert rel(adj.value, D.up2_adj(D.blur_adj(dy).value).value) <= TOL


def test_s2d_layout_and_its_inverse():
    b, c, h, w = 2, 3, 4, 6
    x = torch.arange(b * c * h * w, dtype=F64).view(b, c, h, w)
    y = D.to_s2d(x)
    assert tuple(y.shape) == (b, 4 * c, h // 2, w // 2)
    for hh in range(h):
        for ww in range(w):
            for cc in range(c):
                assert torch.equal(y[:, ((hh & 1) * 2 + (ww & 1)) * c + cc, hh >> 1, ww >> 1], x[:, cc, hh, ww])
    assert torch.equal(D.from_s2d(y), x)
    # the space-to-depth blur pair is the plain pair through the relayout: adjoint by autograd
    xr = rnd(b, c, h, w, seed=7).requires_grad_()
    dy2 = rnd(b, 4 * c, h // 2, w // 2, seed=8)
    gx, = torch.autograd.grad((D.to_s2d(so.blur3x3_reflect(xr)) * dy2).sum(), [xr])
    assert rel(D.blur_adj(D.from_s2d(dy2)).value, gx) <= TOL


def test_gate_takes_the_slope_at_both_zeros():
    g = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 2.0], dtype=torch.bfloat16)
    v = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0])
    assert D.gate(v, g, 0.5).tolist() == [0.5, 1.0, 3.0, 2.0, 5.0]
    assert D.gate(v, g).dtype == F64
    assert D.SLOPE != 0.2 and abs(D.SLOPE - 0.2) < 2 ** -26  # the fp32 constant, not the double
    assert D.gate(v, g).tolist() == [D.SLOPE, 2 * D.SLOPE, 3.0, 4 * D.SLOPE, 5.0]
    assert torch.equal(D.bias_act_bwd(v, g), D.gate(v, g))
    # as the gradient of the activation in terms of its output
    p = rnd(2, 3, 4, 5, seed=9).requires_grad_()
    dy = rnd(2, 3, 4, 5, seed=10)
    y = torch.where(p > 0, p, D.SLOPE * p)
    gp, = torch.autograd.grad((y * dy).sum(), [p])
    assert rel(D.bias_act_bwd(dy, y.detach()), gp) <= TOL


@pytest.mark.parametrize("form", ["bias", "noise", "bias+noise"])
def test_bias_act_reads_the_noise_plane_transposed(form):
    b, c, h, w, ns = 2, 5, 4, 7, 10  # a non-square crop of a larger plane
    x, bias = rnd(b, c, h, w, seed=11), rnd(c, seed=12)
    noise, nw, nb = rnd(b, ns, ns, seed=13), rnd(c, seed=14), rnd(c, seed=15)
    pre = x
    if "bias" in form:
        pre = pre + bias.view(1, c, 1, 1)
    if "noise" in form:
        pre = pre + noise[:, :w, :h].transpose(1, 2)[:, None] * nw.view(1, c, 1, 1) + nb.view(1, c, 1, 1)
    ref = F.leaky_relu(pre, D.SLOPE)
    got = D.bias_act(x, bias if "bias" in form else None, *((noise, nw, nb) if "noise" in form else (None, None, None)))
    assert rel(got.value, ref) <= TOL
    assert (got.abs_terms >= pre.abs() * (1 - 1e-12)).all() and (got.abs_terms >= got.value.abs() * (1 - 1e-12)).all()
    assert rel(got.value, F.leaky_relu(pre, 0.2)) <= 2 ** -26  # float32(0.2) against the double 0.2 of the reference
    if form == "noise":
        assert rel(D.noise_plane(noise, h, w), noise[:, :w, :h].transpose(1, 2)) == 0


def test_rowwise_sumsq():
    x = rnd(5, 37, seed=16)
    got = D.rowwise_sumsq(x)
    assert rel(got.value, x.norm(2, dim=1) ** 2) <= TOL and torch.equal(got.value, got.abs_terms)


@pytest.mark.parametrize("shape", [(2, 8, 3, 5), (3, 16, 2, 2), (1, 4, 1, 1)], ids=["2x8x3x5", "3x16x2x2", "1x4x1x1"])
def test_torgb_and_its_gradients_are_the_grouped_conv(shape):
    """The per-sample-weight grouped-conv formulation of Conv2DMod.forward, demod=False (as test_torgb_streaming_kernels)."""
    b, c, h, w = shape
    x, s1 = rnd(*shape, seed=17).requires_grad_(), (rnd(b, c, seed=18) * 0.5 + 1).requires_grad_()
    wt, r = (rnd(3, c, 1, 1, seed=19) / c ** 0.5).requires_grad_(), rnd(b, 3, h, w, seed=20)
    wmod = wt[None] * s1[:, None, :, None, None]
    y = F.conv2d(x.reshape(1, b * c, h, w), wmod.reshape(b * 3, c, 1, 1), groups=b).reshape(b, 3, h, w)
    gx, gs, gw = torch.autograd.grad((y * r).sum(), [x, s1, wt])
    xd, sd, wd = x.detach(), s1.detach(), wt.detach()
    fwd, bwd = D.torgb(xd, sd, wd), D.torgb_bwd(xd, r, sd, wd)
    assert rel(fwd.value, y.detach()) <= TOL
    dominates(fwd)
    assert rel(bwd.gx, gx) <= TOL and (bwd.abs_gx >= bwd.gx.abs() * (1 - 1e-12)).all()
    assert (bwd.abs_T >= bwd.T.abs() * (1 - 1e-12)).all()
    ds, dw = D.torgb_dstyle(bwd.T, wd, bwd.abs_T), D.torgb_dw(bwd.T, sd, bwd.abs_T)
    assert rel(ds.value, gs) <= TOL and rel(dw.value.reshape(3, c, 1, 1), gw) <= TOL
    dominates(ds)
    dominates(dw)
    # abs_terms is the formula on the absolute values
    assert rel(D.torgb(xd.abs(), sd.abs(), wd.abs()).value, fwd.abs_terms) <= TOL
    assert rel(D.torgb_bwd(xd.abs(), r.abs(), sd.abs(), wd.abs()).T, bwd.abs_T) <= TOL
