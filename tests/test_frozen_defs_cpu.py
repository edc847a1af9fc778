"""The float64 definitions of tests/_frozen_defs.py against independent float64 statements of the same things (CPU): ATen's
bilinear interpolation, max-pools and conv2d_input with autograd, the LPIPS composition written with torch ops, and
Tensor.to(bfloat16).  Bound: 1e-12 of abs_terms per element (float64 against float64).

Also asserted here, on the reference alone, are the conditions tests/test_frozen_ew_gpu.py relies on: the share of pooling
windows with a near tie, that no LPIPS pixel of the seeded inputs is all-zero, and the fp32 index rule of the resize kernels
(rs_index) at every (in, out) pair the GPU file uses."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _frozen_defs as D

F64 = torch.float64
TOL = 1e-12
# every (in, out) pair of tests/test_frozen_ew_gpu.py (it asserts its resize cases against these two lists)
GAUSS_PAIRS = [(256, 224), (32, 224), (64, 224), (40, 33), (56, 97), (224, 224), (7, 3), (5, 11), (1, 3), (5, 1), (7, 1)]
EXACT_PAIRS = [(32, 64), (64, 32), (8, 32), (16, 16)]
POOL_SHAPES = [(3, 5, 7, 7), (2, 8, 12, 10), (1, 2, 1, 1), (1, 3, 2, 5)]
LPIPS_SHAPES = [(2, 192, 5, 7), (2, 384, 3, 5), (1, 256, 1, 1), (2, 130, 8, 8), (2, 129, 5, 13), (3, 64, 9, 9), (2, 1, 5, 5), (2, 35, 8, 9),
                (2, 72, 1, 65)]


def rnd(*shape, seed=0):
    return torch.randn(*shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def within(got, want, abs_terms, what=""):
    assert got.shape == want.shape == abs_terms.shape, (what, got.shape, want.shape, abs_terms.shape)
    assert (abs_terms >= want.abs() * (1 - 1e-12)).all(), what + ": abs_terms < |result|"
    assert ((got - want).abs() <= TOL * abs_terms).all(), (what, ((got - want).abs() / abs_terms.clamp_min(1e-300)).max().item())


# ---- affine (+ residual) (+ ReLU) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("res", [True, False])
def test_affine_act_is_eval_batchnorm_and_autograd(res, relu):
    x, r = rnd(2, 5, 6, 7, seed=1).requires_grad_(), rnd(2, 5, 6, 7, seed=2).requires_grad_()
    s, t, gy = rnd(5, seed=3), rnd(5, seed=4), rnd(2, 5, 6, 7, seed=5)
    gamma, var, mean = s * 2.0, torch.full((5,), 4.0, dtype=F64) - 1e-5, rnd(5, seed=6)
    beta = t + mean * s  # s = gamma / sqrt(var + eps), t = beta - mean * s
    v = F.batch_norm(x, mean, var, gamma, beta, False, 0.0, 1e-5)
    v = v + r if res else v
    y = torch.relu(v) if relu else v
    want = D.affine_act(x, s, t, r if res else None, relu)
    assert ((y - want.value).abs() <= 1e-10 * want.abs_terms).all()  # batch_norm's own rsqrt: not the 1e-12 class
    y2 = x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1) + (r if res else 0)
    y2 = torch.relu(y2) if relu else y2
    within(y2.detach(), want.value.detach(), want.abs_terms.detach(), "affine_act")
    gx, gr = torch.autograd.grad((y2 * gy).sum(), [x, r], allow_unused=True)
    dgx, dgres = D.affine_act_bwd(gy, y2.detach(), s, relu)
    within(gx, dgx.value, dgx.abs_terms, "gx")
    if res:
        assert torch.equal(gr, dgres)


def test_affine_act_bwd_blocks_both_zeros():
    y = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0]).view(1, 1, 1, 6)
    gx, gres = D.affine_act_bwd(torch.ones(1, 1, 1, 6), y, torch.tensor([-0.5]), True)
    assert gres.flatten().tolist() == [0, 0, 0, 0, 1, 1] and gx.value.flatten().tolist() == [0, 0, 0, 0, -0.5, -0.5]


# ---- pool ------------------------------------------------------------------------------------------------------------------------
def pool_inputs(shape, kind, seed=0):
    """The seeded pooling operands of the GPU file: gauss, or tie-rich (half the rows rounded to multiples of 0.5)."""
    b, c, h, w = shape
    g = torch.Generator().manual_seed(1000 + seed + h * 31 + w)
    x = torch.randn(b, c, h, w, generator=g)
    if kind == "ties":
        x[:, :, : (h + 1) // 2] = torch.round(x[:, :, : (h + 1) // 2] * 2) / 2
    s, t = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    s[0] = -s[0]
    if kind == "negative":
        t = t - 8.0
        s = s.abs()
        x = -x.abs()
    return x, s, t


@pytest.mark.parametrize("kind", ["gauss", "ties", "negative"])
@pytest.mark.parametrize("shape", POOL_SHAPES + [(4, 16, 57, 61)])
def test_affine_relu_maxpool_is_atens_and_its_ties_are(shape, kind):
    x, s, t = pool_inputs(shape, kind)
    xr = x.double().requires_grad_()
    aff = xr * s.double().view(1, -1, 1, 1) + t.double().view(1, -1, 1, 1)
    ref = F.max_pool2d(torch.relu(aff), 3, 2, 1)
    d = D.affine_relu_maxpool(x, s, t)
    within(d.y, ref.detach(), d.abs_terms + (ref.detach() == 0), "pool")
    gy = rnd(*ref.shape, seed=7)
    gx, = torch.autograd.grad((ref * gy).sum(), [xr])
    bw = D.affine_relu_maxpool_bwd(gy, d.idx, s, shape[2:])
    # ATen pools relu(aff): among equal maxima it takes the first, and a window whose maximum is 0 passes nothing through the ReLU
    clean = ~d.near_tie
    assert clean.float().mean().item() >= 0.999, "more than 0.1 %% of the windows have a near tie: %d" % int(d.near_tie.sum())
    if bool(clean.all()):
        within(bw.value, gx, bw.abs_terms + (gx == 0), "pool gradient, incl. which element of a tie receives it")
    if kind == "negative":
        assert (d.idx == 255).all() and (d.y == 0).all() and (bw.value == 0).all()
    if kind == "ties" and shape[2] > 2:  # the planes are tie-rich: windows whose positive maximum occurs more than once
        taps = D._taps3s2p1(aff.detach(), -float("inf"))
        top = taps.max(dim=0).values
        assert (((taps == top).sum(dim=0) > 1) & (top > 0)).any()


def test_near_tie_share_of_a_large_gauss_plane():
    x, s, t = pool_inputs((4, 16, 57, 61), "gauss")
    d = D.affine_relu_maxpool(x, s, t)
    assert d.near_tie.numel() == 57536 and int(d.near_tie.sum()) <= 57


def test_pool_index_is_window_local_first_strict_maximum():
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 1, 1] = x[0, 0, 1, 2] = x[0, 0, 2, 1] = 3.0
    d = D.affine_relu_maxpool(x, torch.ones(1), torch.zeros(1))
    # window (oh, ow) covers rows 2 oh - 1 .. 2 oh + 1: (1, 1) has its three equal maxima at taps 0, 1, 3; (0, 0) sees (1, 1) as
    # tap (2, 2); (0, 1) sees (1, 1) and (1, 2) as taps 6 and 7; (2, 2) holds zeros only: the ReLU blocks it
    assert d.idx[0, 0, 1, 1].item() == 0 and d.idx[0, 0, 0, 0].item() == 8 and d.idx[0, 0, 0, 1].item() == 6
    assert d.idx[0, 0, 2, 2].item() == 255 and d.y[0, 0].tolist() == [[3, 3, 0], [3, 3, 0], [0, 0, 0]]
    gx = D.affine_relu_maxpool_bwd(torch.ones(1, 1, 3, 3), d.idx, torch.full((1,), 2.0), (5, 5)).value
    assert gx[0, 0, 1, 1].item() == 8.0 and gx.sum().item() == 8.0  # four windows name (1, 1), none names its equals


# ---- resize ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [((7, 5), (3, 11)), ((40, 56), (33, 97)), ((8, 8), (32, 32)), ((16, 12), (16, 12)), ((1, 1), (3, 3)),
                                ((5, 7), (1, 1)), ((32, 32), (64, 64)), ((64, 64), (32, 32))])
@pytest.mark.parametrize("norm", [True, False])
def test_resize_norm_is_atens_bilinear_and_its_autograd(hw, norm):
    (h, w), size = hw
    x = rnd(2, 3, h, w, seed=11).requires_grad_()
    mean, std = (rnd(3, seed=12), rnd(3, seed=13).abs() + 0.5) if norm else (None, None)
    ref = F.interpolate(x, size=list(size), mode="bilinear", align_corners=False)
    if norm:
        ref = (ref - mean.view(1, -1, 1, 1)) / std.view(1, -1, 1, 1)
    d = D.resize_norm(x.detach(), size, mean, std)
    within(d.value, ref.detach(), d.abs_terms + 1e-300, "resize_norm")
    assert (d.dy_terms >= 0).all() and (d.dx_terms >= 0).all()
    gy = rnd(*ref.shape, seed=14)
    gx, = torch.autograd.grad((ref * gy).sum(), [x])
    a = D.resize_norm_adj(gy, (h, w), std)
    within(a.value, gx, a.abs_terms + 1e-300, "resize_norm_adj")
    # the coordinate terms are derivatives: shifting every row coordinate by eps moves the output by eps * (G x) to first order
    if h > 1 and not norm:
        eps, (my, gmat), (mx, _) = 1e-7, D.resize_matrices(h, size[0]), D.resize_matrices(w, size[1])
        moved = torch.matmul(torch.matmul(my + eps * gmat, x.detach()), mx.t())
        assert ((moved - d.value).abs() <= eps * d.dy_terms * (1 + 1e-6) + 1e-15).all()


@pytest.mark.parametrize("pair", GAUSS_PAIRS + EXACT_PAIRS, ids=lambda p: "%d-%d" % p)
def test_rs_index_of_the_kernel_names_the_exact_cell(pair):
    """rs_index in numpy float32, with and without the fma contraction: i0 is the exact floor and i0 + lambda within
    3 * 2^-24 * in of the exact coordinate (one rounding of the ratio, one of the product, one of the subtraction);
    power-of-two ratios and the identity are exact."""
    n_in, n_out = pair
    worst = 0.0
    for fma in (False, True):
        for dst in range(n_out):
            i0, _, lam = D.resize_coord(dst, n_in, n_out)
            k0, l1 = D.rs_index_f32(dst, n_in, n_out, fma)
            assert k0 == i0, (pair, dst, fma, k0, i0)
            err = abs(float(k0) + float(l1) - float(i0 + lam))
            worst = max(worst, err / (2.0 ** -24 * n_in))
            if pair in EXACT_PAIRS:
                assert float(l1) == float(lam)
    assert worst <= 3.0, (pair, worst)


# ---- LPIPS ---------------------------------------------------------------------------------------------------------------------------
def lpips_inputs(shape, seed=0):
    """The seeded LPIPS operands of the GPU file (fp32 values)."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(2000 + seed + C * 7 + H * W)
    f0 = torch.randn(B, C, H, W, generator=g)
    f1 = f0 + 0.3 * torch.randn(B, C, H, W, generator=g)
    lin = torch.rand(C, generator=g) / C
    gout = torch.randn(B, generator=g)
    return f0, f1, lin, gout


@pytest.mark.parametrize("shape", LPIPS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_lpips_tap_is_the_published_composition(shape):
    f0, f1, lin, gout = lpips_inputs(shape)
    for f in (f0, f1, f0.bfloat16().float(), f1.bfloat16().float()):
        assert (f.abs().sum(1) > 0).all(), "an all-zero pixel: 0 / 0 in the reference too"
    a, b = f0.double().requires_grad_(), f1.double().requires_grad_()

    def normalize_tensor(t, eps=1e-10):  # lpips 0.1.4
        return t / (torch.sqrt(torch.sum(t ** 2, dim=1, keepdim=True)) + eps)

    diff = (normalize_tensor(a) - normalize_tensor(b)) ** 2
    val = F.conv2d(diff, lin.double().view(1, -1, 1, 1)).mean([2, 3]).flatten()
    g0, g1 = torch.autograd.grad((val * gout.double()).sum(), [a, b])
    d = D.lpips_tap(f0, f1, lin, gout)
    within(d.dist, val.detach(), d.abs_dist, "distance")
    assert torch.allclose(d.r0, f0.double().pow(2).sum(1).sqrt().reshape(shape[0], -1), rtol=1e-14, atol=0)
    within(d.g0, g0, d.own0 + d.cross0, "g0")
    within(d.g1, g1, d.own1 + d.cross1, "g1")
    # the closed form the kernel's comment states, term by term under the magnitudes returned
    x, y, l = f0.double(), f1.double(), lin.double().view(1, -1, 1, 1)
    B, C, H, W = shape
    r0, r1 = d.r0.view(B, 1, H, W), d.r1.view(B, 1, H, W)
    A, Bn = r0 + 1e-10, r1 + 1e-10
    t = x / A - y / Bn
    gs = (gout.double() / (H * W)).view(B, 1, 1, 1)
    dot0, dot1 = (l * t * x).sum(1, keepdim=True), (l * t * y).sum(1, keepdim=True)
    assert (dot0.abs() <= d.abs_dot0 * (1 + 1e-12)).all() and (dot1.abs() <= d.abs_dot1 * (1 + 1e-12)).all()
    within(gs * (2 * l * t / A - 2 * dot0 / (A * A * r0) * x), g0, d.own0 + d.cross0, "closed form g0")
    within(gs * (2 * dot1 / (Bn * Bn * r1) * y - 2 * l * t / Bn), g1, d.own1 + d.cross1, "closed form g1")


# ---- bridges, relu_gate_add -----------------------------------------------------------------------------------------------------------
def test_bridges_round_as_tensor_to_bfloat16():
    x = torch.randn(3, 8, 5, 7, generator=torch.Generator().manual_seed(21))
    x.view(-1)[:6] = torch.tensor([0.0, -0.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38])  # two exact ties (to even: down, up)
    for relu in (False, True):
        want = (x.relu() if relu else x).to(torch.bfloat16).double()
        assert torch.equal(D.bridge_fwd(x, relu), want)
    g, gate = torch.randn(2, 8, 3, 3).bfloat16(), torch.tensor([-1.0, -0.0, 0.0, 2.0]).repeat(36).view(2, 8, 3, 3).bfloat16()
    assert torch.equal(D.bridge_bwd(g), g.double())
    assert torch.equal(D.bridge_bwd(g, gate), (g.double() * (gate.double() > 0)))
    b = torch.randn(2, 8, 3, 3).bfloat16()
    r = D.relu_gate_add(g, b, gate)
    assert torch.equal(r.value, (g.double() + b.double()) * (gate.double() > 0)) and (r.abs_terms >= r.value.abs()).all()
    assert torch.equal(D.relu_gate_add(g, None, gate).value, g.double() * (gate.double() > 0))
    assert torch.equal(r.value.float().bfloat16(), ((g.float() + b.float()) * (gate.float() > 0)).to(torch.bfloat16))


# ---- MaxPool2d(3, 2) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8, 9, 9), (1, 8, 3, 3), (2, 16, 8, 11), (1, 24, 4, 7), (1, 8, 3, 4), (1, 8, 4, 3), (2, 16, 5, 6)])
def test_maxpool3s2_is_atens_including_ties_and_nans(shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(22)
    x = (torch.randn(B, C, H, W, generator=g).relu() * 4).round() / 4
    if H * W > 20:
        x[0, 0, 1, 1] = float("nan")
    xr = x.double().requires_grad_()
    ref = F.max_pool2d(xr, 3, 2)
    d = D.maxpool3s2(x)
    assert torch.equal(torch.nan_to_num(d.y, nan=-7.0), torch.nan_to_num(ref.detach(), nan=-7.0))
    gy = rnd(*ref.shape, seed=23)
    ref.backward(gy)
    bw = D.maxpool3s2_bwd(gy, d.pos, (H, W))
    within(bw.value, xr.grad, bw.abs_terms + 1e-300, "max-pool gradient: which element of a tie receives it")


# ---- image gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 5, 3, 11, 4, 2, 37, 45), (1, 8, 1, 5, 4, 0, 21, 17), (2, 5, 3, 7, 2, 3, 33, 130), (2, 13, 2, 5, 2, 2, 19, 23),
                                  (1, 6, 3, 4, 1, 2, 9, 11), (1, 3, 2, 2, 1, 0, 6, 7), (1, 7, 3, 1, 1, 0, 5, 5), (1, 5, 3, 9, 2, 4, 23, 21)],
                         ids=lambda c: "-".join(map(str, c)))
def test_conv_image_grad_is_conv2d_input(case):
    B, N, C, K, S, pad, H, W = case
    Ho, Wo = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    dy, w = rnd(B, N, Ho, Wo, seed=31), rnd(N, C, K, K, seed=32)
    ref = torch.nn.grad.conv2d_input((B, C, H, W), w, dy, stride=S, padding=pad)
    d = D.conv_image_grad(dy, w, (H, W), S, pad)
    within(d.value, ref, d.abs_terms + 1e-300, "image gradient")
