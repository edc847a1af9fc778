"""The definitions of tests/_conv_exact_defs.py, on the CPU:
  * on Gaussian float64 inputs each equals F.conv2d + float64 autograd of its docstring formula (space-to-depth layouts and
    the bit-mask packing included);
  * on the integer operands the fp32 and the fp64 evaluation are identical (the exactness argument, checked);
  * power, on the reference alone: with ONE non-zero input element set to zero, at least 90 % of the outputs that element
    reaches through a non-zero weight differ from the stored expected value — a kernel that loses a single product fails
    torch.equal on nearly every output the product belongs to.  The misses are bf16 outputs above 256, where the format no
    longer resolves integers.  Smallest and deepest-K case of every family."""
import pytest
import torch
import torch.nn.functional as F

import _conv_exact_defs as D

F64 = torch.float64
POWER_CAP = 0.90


def randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def close(a, b, tol=1e-9):
    assert a.shape == b.shape, (a.shape, b.shape)
    err, scale = float((a - b).abs().max()), max(1e-30, float(b.abs().max()))
    assert err <= tol * scale, (err, scale)


# ---- Gaussian float64 inputs against autograd -------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 6, 10, 9, 7, 3, 1, 1), (2, 8, 12, 8, 8, 1, 2, 0), (2, 5, 4, 9, 7, 5, 1, 2), (3, 8, 8, 10, 12, 3, 2, 1)])
@pytest.mark.parametrize("natural", [False, True])
@pytest.mark.parametrize("act", ["none", "relu", "lrelu"])
def test_forward_definition_is_conv2d_with_the_documented_epilogue(case, natural, act):
    B, C, N, H, W, k, s, p = case
    g = D.gen("fwd", case)
    x, w = randn(g, B, C, H, W), randn(g, N, C, k, k)
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    si, so, bias, nw, nb = randn(g, B, C).abs() + 0.5, randn(g, B, N).abs() + 0.5, randn(g, N), randn(g, N), randn(g, N)
    noise, res = torch.rand(B, max(ho, wo) + 2, max(ho, wo) + 2, generator=g, dtype=F64), randn(g, B, N, ho, wo)
    xs, wres = randn(g, B, 3, ho, wo), randn(g, N, 3)
    got = D.forward(x, w, s, p, in_scale=si, out_scale=so, bias=bias, noise=noise, noise_w=nw, noise_b=nb, natural=natural,
                    residual=res, res_scale=0.7, second=(xs, wres), act=act, dt=F64, exact=False)
    want = torch.zeros(B, N, ho, wo, dtype=F64)
    z = F.conv2d(x * si[:, :, None, None], w, None, s, p)
    for b in range(B):
        for n in range(N):
            for i in range(ho):
                for j in range(wo):
                    plane = noise[b, i, j] if natural else noise[b, j, i]
                    v = z[b, n, i, j] * so[b, n] + (xs[b, :, i, j] * wres[n]).sum() + bias[n] + plane * nw[n] + nb[n]
                    want[b, n, i, j] = (v + res[b, n, i, j]) * 0.7
    want = {"none": want, "relu": F.relu(want), "lrelu": F.leaky_relu(want, D.SLOPE)}[act]
    close(got.y, want)
    assert bool((got.A >= got.y.abs() * (1 - 1e-12)).all())
    plain = D.forward(x, w, s, p, dt=F64, exact=False)
    close(plain.y, F.conv2d(x, w, None, s, p))
    assert abs(D.SLOPE - 0.2) < 1e-8 and D.SLOPE != 0.2


@pytest.mark.parametrize("case", [(2, 6, 10, 9, 7, 3, 1, 1), (2, 8, 12, 8, 8, 1, 2, 0), (3, 8, 8, 10, 12, 3, 2, 1), (2, 8, 4, 6, 6, 5, 1, 2)])
def test_data_gradient_definition_is_autograd_of_conv2d(case):
    B, C, N, H, W, k, s, p = case
    g = D.gen("dgrad", case)
    x = randn(g, B, C, H, W).requires_grad_()
    w = randn(g, N, C, k, k)
    y = F.conv2d(x, w, None, s, p)
    dy, si, so, gate = randn(g, *y.shape), randn(g, B, N).abs() + 0.5, randn(g, B, C).abs() + 0.5, randn(g, B, C, H, W)
    gate.view(-1)[:4] = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=F64)
    (gx,) = torch.autograd.grad((y * dy * si[:, :, None, None]).sum(), x)
    close(D.dgrad(dy, w, x.shape, s, p, dt=F64, exact=False).y, torch.autograd.grad((F.conv2d(x, w, None, s, p) * dy).sum(), x)[0])
    got = D.dgrad(dy, w, x.shape, s, p, in_scale=si, out_scale=so, gate=gate, dt=F64, exact=False)
    want = gx * so[:, :, None, None] * torch.where(gate > 0, 1.0, D.GATE_SLOPE)
    close(got.y, want)
    assert got.y.view(-1)[0] == D.GATE_SLOPE * (gx * so[:, :, None, None]).view(-1)[0]  # +0.0 takes the slope
    # gated by the bit mask: the mask of the gate selects the same elements (C % 8 == 0 cases)
    if C % 8 == 0:
        m = D.pack_mask(gate)
        bits = ((m[..., None].to(torch.int32) >> torch.arange(8, dtype=torch.int32)) & 1).reshape(B, H, W, C).permute(0, 3, 1, 2)
        assert torch.equal(bits.bool(), gate > 0)


@pytest.mark.parametrize("case", [(2, 6, 10, 9, 7, 3, 1, 1), (2, 8, 12, 8, 8, 1, 2, 0), (3, 8, 8, 10, 12, 3, 2, 1)])
def test_weight_gradient_definition_is_autograd_of_conv2d(case):
    B, C, N, H, W, k, s, p = case
    g = D.gen("wgrad", case)
    x, w = randn(g, B, C, H, W), randn(g, N, C, k, k).requires_grad_()
    xsc, dsc = randn(g, B, C).abs() + 0.5, randn(g, B, N).abs() + 0.5
    y = F.conv2d(x * xsc[:, :, None, None], w, None, s, p)
    dy, acc, acc_b = randn(g, *y.shape), randn(g, N, C, k, k), randn(g, N)
    (gw,) = torch.autograd.grad((y * dy * dsc[:, :, None, None]).sum(), w)
    got = D.wgrad(x, dy, w.shape, s, p, x_scale=xsc, dy_scale=dsc, out_scale=0.5, acc=acc, acc_b=acc_b, dt=F64, exact=False)
    close(got.dw, acc + 0.5 * gw)
    close(got.db, acc_b + 0.5 * dy.sum(dim=(0, 2, 3)))
    plain = D.wgrad(x, dy, w.shape, s, p, dt=F64, exact=False)
    (gw0,) = torch.autograd.grad((F.conv2d(x, w, None, s, p) * dy).sum(), w)
    close(plain.dw, gw0)
    close(plain.db, dy.sum(dim=(0, 2, 3)))


def test_space_to_depth_forms():
    B, C, N, H, W = 2, 8, 8, 4, 6  # half-resolution H x W
    g = D.gen("s2d")
    x = randn(g, B, C, 2 * H, 2 * W).requires_grad_()
    w = randn(g, N, C, 3, 3).requires_grad_()
    x2 = D.s2d(x.detach())
    for b, c, h, wd, sy, sx in [(0, 0, 0, 0, 0, 0), (1, 5, 3, 2, 1, 0), (1, 7, 2, 5, 0, 1), (0, 3, 3, 5, 1, 1)]:
        assert x2[b, (sy * 2 + sx) * C + c, h, wd] == x[b, c, 2 * h + sy, 2 * wd + sx]
    bias, res, xs, wres = randn(g, N), randn(g, B, N, H, W), randn(g, B, 3, H, W), randn(g, N, 3)
    y0 = F.conv2d(x, w, bias, 2, 1)
    close(D.s2d_forward(x.detach(), w.detach(), bias=bias, dt=F64, exact=False).y, y0.detach())
    close(D.s2d_forward(x.detach(), w.detach(), bias=bias, residual=res, res_scale=0.7, dt=F64, exact=False).y, ((y0 + res) * 0.7).detach())
    close(D.s2d_forward(x.detach(), w.detach(), bias=bias, second=(xs, wres), res_scale=0.7, dt=F64, exact=False).y,
          ((y0 + F.conv2d(xs, wres[:, :, None, None])) * 0.7).detach())
    dy = randn(g, B, N, H, W)
    gx, gw = torch.autograd.grad((F.conv2d(x, w, None, 2, 1) * dy).sum(), (x, w))
    close(D.s2d_dgrad(dy, w.detach(), dt=F64, exact=False).y, D.s2d(gx))
    acc = randn(g, N, C, 3, 3)
    close(D.s2d_wgrad(x.detach(), dy, w.shape, out_scale=0.5, acc=acc, dt=F64, exact=False).dw, acc + 0.5 * gw)


def test_bit_mask_packing():
    g = D.gen("mask")
    t = D.gate_like(g, (2, 16, 3, 5))
    m = D.pack_mask(t)
    assert m.shape == (2, 3, 5, 2) and m.dtype == torch.uint8
    flat = t.permute(0, 2, 3, 1).reshape(-1)
    for i in range(m.numel()):
        want = sum(1 << k for k in range(8) if flat[8 * i + k] > 0)
        assert int(m.view(-1)[i]) == want
    assert (t == 0).any() and torch.signbit(t[t == 0]).any() and (~torch.signbit(t[t == 0])).any()


def test_to_rgb_definitions():
    B, C, H, W = 3, 8, 5, 4
    g = D.gen("torgb")
    x, s1, w = randn(g, B, C, H, W).requires_grad_(), (randn(g, B, C).abs() + 0.5).requires_grad_(), randn(g, 3, C, 1, 1).requires_grad_()
    wmod = w[None] * s1[:, None, :, None, None]
    y = F.conv2d(x.reshape(1, B * C, H, W), wmod.reshape(B * 3, C, 1, 1), groups=B).reshape(B, 3, H, W)
    got = D.torgb_fwd(x.detach(), s1.detach(), w.detach(), dt=F64, exact=False)
    close(got.y[:, :3], y.detach())
    assert float(got.y[:, 3].abs().max()) == 0.0
    gy = torch.cat([randn(g, B, 3, H, W), randn(g, B, 1, H, W)], dim=1)  # the fourth channel must not matter
    gx, gs, gw = torch.autograd.grad((y * gy[:, :3]).sum(), (x, s1, w))
    bw = D.torgb_bwd(x.detach(), gy, s1.detach(), w.detach(), dt=F64, exact=False)
    close(bw.gx, gx)
    close((bw.T * w.detach().reshape(1, 3, C)).sum(dim=1), gs)  # the caller's style and weight gradients from T
    close((bw.T * s1.detach()[:, None, :]).sum(dim=0).reshape(3, C, 1, 1), gw)


# ---- integer operands: fp32 == fp64, and the power of torch.equal -----------------------------------------------------
# (B, C, N, H, W): the smallest and the deepest-K case of each family of tests/test_conv_exact_gpu.py
SMALL, DEEP, DEEP_S = (1, 64, 64, 16, 32), (1, 512, 64, 16, 32), (2, 512, 128, 4, 4)


def _families(case):
    """name -> (function of the perturbed operand `t` returning the stored outputs, the operand, its reach function)."""
    B, C, N, H, W = case
    o = D.operands("power", B, C, N, H, W)
    o2 = D.operands("power-s2", B, C, N, 2 * H, 2 * W, 3, 2, 1, c_res=8)
    ts = D.operands("power-rgb", B, C, 3, H, W, 1, 1, 0)
    gy = torch.cat([ts["dy"], torch.zeros(B, 1, H, W)], dim=1)
    nz = lambda t: (t != 0).float()  # noqa: E731
    fam = {
        "forward": (lambda x, dt: [D.store(D.forward(x, o["w"], 1, 1, in_scale=o["s_c"], out_scale=o["s_n"], bias=o["bias"], noise=o["noise"],
                                                     noise_w=o["nw"], noise_b=o["nb"], residual=o["res"], res_scale=0.5, act="lrelu", dt=dt).y, "bf16")],
                    o["x"], lambda e: [F.conv2d(e, nz(o["w"]), None, 1, 1)]),
        "dgrad": (lambda dy, dt: [D.store(D.dgrad(dy, o["w"], o["x"].shape, 1, 1, in_scale=o["s_n"], out_scale=o["s_c"], gate=o["gate_in"], dt=dt).y, "bf16")],
                  o["dy"], lambda e: [torch.nn.grad.conv2d_input(o["x"].shape, nz(o["w"]), e, 1, 1)]),
        "wgrad": (lambda x, dt: list(D.wgrad(x, o["dy"], o["w"].shape, 1, 1, x_scale=o["s_c"], out_scale=0.5, acc=o["acc"], acc_b=o["acc_b"], dt=dt)[0:1]),
                  o["x"], lambda e: [torch.nn.grad.conv2d_weight(e, o["w"].shape, nz(o["dy"]), 1, 1)]),
        "s2d_forward": (lambda x, dt: [D.store(D.s2d_forward(x, o2["w"], bias=o2["bias"], second=(o2["xs"], o2["w_res"]), res_scale=0.5, dt=dt).y, "bf16")],
                        o2["x"], lambda e: [F.conv2d(e, nz(o2["w"]), None, 2, 1)]),
        "s2d_dgrad": (lambda dy, dt: [D.store(D.s2d_dgrad(dy, o2["w"], dt=dt).y, "bf16")],
                      o2["dy"], lambda e: [D.s2d(torch.nn.grad.conv2d_input(o2["x"].shape, nz(o2["w"]), e, 2, 1))]),
        "s2d_wgrad": (lambda x, dt: [D.s2d_wgrad(x, o2["dy"], o2["w"].shape, out_scale=0.5, acc=o2["acc"], dt=dt).dw],
                      o2["x"], lambda e: [torch.nn.grad.conv2d_weight(e, o2["w"].shape, nz(o2["dy"]), 2, 1)]),
        "torgb_fwd": (lambda x, dt: [D.store(D.torgb_fwd(x, ts["s_c"], ts["w"], dt=dt).y, "bf16")],
                      ts["x"], lambda e: [D.torgb_fwd(e, ts["s_c"], nz(ts["w"]), exact=False).y]),
        "torgb_bwd": (lambda x, dt: [D.torgb_bwd(x, gy, ts["s_c"], ts["w"], dt=dt).T],
                      ts["x"], lambda e: [D.torgb_bwd(e, nz(gy), ts["s_c"], ts["w"], exact=False).T]),
        "torgb_bwd_gx": (lambda g_, dt: [D.store(D.torgb_bwd(ts["x"], g_, ts["s_c"], ts["w"], dt=dt).gx, "bf16")],
                         gy, lambda e: [D.torgb_bwd(ts["x"], e, ts["s_c"], nz(ts["w"]), exact=False).gx]),
    }
    return fam


FAMILIES = ["forward", "dgrad", "wgrad", "s2d_forward", "s2d_dgrad", "s2d_wgrad", "torgb_fwd", "torgb_bwd", "torgb_bwd_gx"]
_CACHE = {}


def families(case):
    if case not in _CACHE:
        _CACHE[case] = _families(case)
    return _CACHE[case]


@pytest.mark.parametrize("case", [SMALL, DEEP, DEEP_S], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("family", FAMILIES)
def test_integer_operands_fp32_and_fp64_evaluations_are_identical(family, case):
    fn, t, _ = families(case)[family]
    for a, b in zip(fn(t, torch.float32), fn(t, torch.float64)):
        assert torch.equal(a.double(), b.double())


@pytest.mark.parametrize("case", [SMALL, DEEP, DEEP_S], ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("family", FAMILIES)
def test_one_lost_product_changes_at_least_90_percent_of_the_outputs_it_reaches(family, case):
    fn, t, reach = families(case)[family]
    want = fn(t, torch.float32)
    g = D.gen("flip", family, case)
    moved_all = reached_all = 0
    for _ in range(16 if family.startswith("torgb") else 4):  # (a to-RGB product reaches 3 outputs or C: pooled over the flips)
        flat_nz = torch.nonzero(t.reshape(-1) != 0).view(-1)
        if family.startswith("torgb"):  # (the zero fourth channel of gy is no input)
            flat_nz = flat_nz[(flat_nz // (t.shape[2] * t.shape[3])) % t.shape[1] < (3 if family == "torgb_bwd_gx" else t.shape[1])]
        i = int(flat_nz[torch.randint(0, flat_nz.numel(), (1,), generator=g)])
        t2 = t.clone()
        t2.view(-1)[i] = 0.0
        e = torch.zeros_like(t)
        e.view(-1)[i] = 1.0
        got = fn(t2, torch.float32)
        reached = sum(int((r != 0).sum()) for r in reach(e))
        moved = sum(int(((a.float() != b.float()) & (r != 0)).sum()) for a, b, r in zip(got, want, reach(e)))
        outside = sum(int(((a.float() != b.float()) & (r == 0)).sum()) for a, b, r in zip(got, want, reach(e)))
        assert reached > 0 and outside == 0
        moved_all, reached_all = moved_all + moved, reached_all + reached
    worst = moved_all / reached_all
    print("%s %s: %.4f of the reached outputs move" % (family, case, worst))
    assert worst >= POWER_CAP, worst
