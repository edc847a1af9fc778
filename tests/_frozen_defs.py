"""Float64 definitions of the kernels of csrc/frozen_ew.hip (the elementwise tails of the frozen ResNet-18 classifier, its
input resize, the LPIPS tap in both layouts, the layout bridges, the bf16 max-pool and the image gradient of a stem
convolution): plain torch, no HIP, none of the project's ops.  Tensors are logical NCHW on whatever device the operands are
on; every input is promoted to float64 and every constant is built in float64.

A result that is a sum comes with abs_terms: the same formula on the absolute values of its terms, the scale of the
rounding-error bound of an fp32 evaluation in any order.  tests/test_frozen_defs_cpu.py ties these to ATen's float64 ops and
autograd; tests/test_frozen_ew_gpu.py holds the kernels to them."""
import collections
from fractions import Fraction

import numpy as np
import torch

from _ew_defs import Sum

F64 = torch.float64
LPIPS_EPS = 1e-10
Pool = collections.namedtuple("Pool", "y abs_terms idx near_tie")
Resize = collections.namedtuple("Resize", "value abs_terms dy_terms dx_terms")
Lpips = collections.namedtuple("Lpips", "dist abs_dist r0 r1 g0 g1 abs_dot0 abs_dot1 own0 own1 cross0 cross1")
NhwcPool = collections.namedtuple("NhwcPool", "y pos")


def _c(v, like):
    """A per-channel vector as [1, C, 1, 1] float64 on the device of `like`."""
    return v.to(device=like.device, dtype=F64).view(1, -1, 1, 1)


# ---- eval BatchNorm as an affine map (+ residual) (+ ReLU) ---------------------------------------------------------------
def affine_act(x, s, t, r=None, relu=True):
    x = x.to(F64)
    p, sh = x * _c(s, x), _c(t, x)
    v, a = p + sh, p.abs() + sh.abs()
    if r is not None:
        v, a = v + r.to(F64), a + r.to(F64).abs()
    return Sum(torch.relu(v) if relu else v, a)


def affine_act_bwd(gy, y, s, relu=True):
    """(gx, gres) with the SAVED output y handed in: gres = gy where y > 0 (both zeros block), gx = gres * s[c]."""
    gy = gy.to(F64)
    gres = torch.where(y.to(F64) > 0, gy, torch.zeros_like(gy)) if relu else gy
    gx = gres * _c(s, gy)
    return Sum(gx, gx.abs()), gres


# ---- BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) -----------------------------------------------------------------------------------
def _taps3s2p1(v, fill):
    """[9, B, C, Ho, Wo]: tap kh * 3 + kw of the 3x3 / stride 2 / pad 1 window, `fill` outside the plane."""
    H, W = v.shape[2:]
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    vp = torch.nn.functional.pad(v, (1, 1, 1, 1), value=fill)
    return torch.stack([vp[:, :, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2] for kh in range(3) for kw in range(3)])


def affine_relu_maxpool(x, s, t):
    """y = max over the window of relu(x * s + t) and idx = kh * 3 + kw of the first strict maximum in scan order over the
    in-bounds taps, taken on float32(x * s + t) (one fma rounding), 255 where that maximum is not positive.  near_tie marks the
    windows whose two largest DISTINCT float64 values lie within 2^-20 of the larger: there an fp32 and an fp64 evaluation may
    name different elements."""
    x = x.to(F64)
    p, sh = x * _c(s, x), _c(t, x)
    v = p + sh
    inf = float("inf")
    taps = _taps3s2p1(v, -inf)
    y = torch.relu(taps.max(dim=0).values)
    a = _taps3s2p1(p.abs() + sh.abs(), 0.0).max(dim=0).values
    t32 = _taps3s2p1(v.float(), -inf)
    best = t32.max(dim=0).values
    first = (t32 == best).to(torch.uint8).argmax(dim=0)  # argmax of a 0 / 1 plane: the first 1
    idx = torch.where(best > 0, first, torch.full_like(first, 255)).to(torch.uint8)
    top = taps.max(dim=0).values
    second = torch.where(taps < top, taps, torch.full_like(taps, -inf)).max(dim=0).values
    near = ((top - second) <= 2.0 ** -20 * top.abs()) & (top > 0)  # rounding keeps the sign: a maximum <= 0 is 255 either way
    return Pool(y, a, idx, near)


def affine_relu_maxpool_bwd(gy, idx, s, in_hw):
    """gx[h, w] = s[c] * sum of gy over the windows whose index names (h, w): a scatter by a GIVEN index plane."""
    gy = gy.to(F64)
    H, W = in_hw
    B, C, ho, wo = gy.shape
    out = []
    for g in (gy, gy.abs()):
        acc = torch.zeros(B, C, 2 * ho + 1, 2 * wo + 1, dtype=F64, device=gy.device)
        for k in range(9):
            kh, kw = divmod(k, 3)
            acc[:, :, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2] += torch.where(idx == k, g, torch.zeros_like(g))
        out.append(acc[:, :, 1:1 + H, 1:1 + W])
    sc = _c(s, gy)
    return Sum(out[0] * sc, out[1] * sc.abs())


# ---- bilinear resize (align_corners=False) + normalisation ---------------------------------------------------------------------
def resize_coord(dst, n_in, n_out):
    """The exact source coordinate in / out * (dst + 0.5) - 0.5 clamped at 0, as (i0, i1, lambda: a Fraction)."""
    src = max(Fraction(n_in * (2 * dst + 1) - n_out, 2 * n_out), Fraction(0))
    i0 = src.numerator // src.denominator
    return i0, min(i0 + 1, n_in - 1), src - i0


def resize_matrices(n_in, n_out, device="cpu"):
    """M [out, in]: the interpolation weights; G [out, in]: -1 at i0 and +1 at i1 (zero where they coincide), the derivative of
    a row of M with respect to its coordinate."""
    m, g = torch.zeros(n_out, n_in, dtype=F64), torch.zeros(n_out, n_in, dtype=F64)
    for o in range(n_out):
        i0, i1, lam = resize_coord(o, n_in, n_out)
        m[o, i0] += float(1 - lam)
        m[o, i1] += float(lam)
        if i1 != i0:
            g[o, i0], g[o, i1] = -1.0, 1.0
    return m.to(device), g.to(device)


def _sep(my, x, mx):
    return torch.matmul(torch.matmul(my, x), mx.t())


def resize_norm(x, size, mean=None, std=None):
    x = x.to(F64)
    (my, gy), (mx, gx) = resize_matrices(x.shape[2], size[0], x.device), resize_matrices(x.shape[3], size[1], x.device)
    v, a = _sep(my, x, mx), _sep(my, x.abs(), mx)
    dy, dx = torch.matmul(torch.matmul(gy, x).abs(), mx.t()), torch.matmul(my, torch.matmul(x, gx.t()).abs())
    if mean is not None:
        m, sd = _c(mean, x), _c(std, x)
        v, a, dy, dx = (v - m) / sd, (a + m.abs()) / sd.abs(), dy / sd.abs(), dx / sd.abs()
    return Resize(v, a, dy, dx)


def resize_norm_adj(gy, in_hw, std=None):
    """The adjoint: gx[iy, ix] = sum_{oy, ox} My[oy, iy] Mx[ox, ix] gy[oy, ox] / std[c].  dy_terms / dx_terms: |gy| through the
    |derivative| of one axis's weights and the other axis's weights."""
    gy = gy.to(F64)
    (my, dgy), (mx, dgx) = resize_matrices(in_hw[0], gy.shape[2], gy.device), resize_matrices(in_hw[1], gy.shape[3], gy.device)
    a = gy.abs()
    v, av = _sep(my.t(), gy, mx.t()), _sep(my.t(), a, mx.t())
    dy, dx = _sep(dgy.abs().t(), a, mx.t()), _sep(my.t(), a, dgx.abs().t())
    if std is not None:
        sd = _c(std, gy)
        v, av, dy, dx = v / sd, av / sd.abs(), dy / sd.abs(), dx / sd.abs()
    return Resize(v, av, dy, dx)


def rs_index_f32(dst, n_in, n_out, fma):
    """The kernel's rs_index in numpy float32: (i0, lambda1).  fma: ratio * (dst + 0.5f) - 0.5f contracted into one rounding."""
    f = np.float32
    ratio = f(n_in) / f(n_out)
    d = f(dst) + f(0.5)
    src = f(np.float64(ratio) * np.float64(d) - 0.5) if fma else f(ratio * d) - f(0.5)  # a float64 product of two floats is exact
    src = f(0) if src < 0 else src
    i0 = int(src)
    return i0, f(src - f(i0))


# ---- the LPIPS tap (lpips 0.1.4: normalize_tensor, lin, spatial_average) -------------------------------------------------------
def lpips_tap(f0, f1, lin, gout=None):
    """dist[b] = mean_p sum_c lin[c] (f0 / (|f0| + eps) - f1 / (|f1| + eps))^2, the per-pixel norms r0 / r1 [B, HW], and by
    float64 autograd the gradients of sum_b gout[b] dist[b].  The absolute-term sums: abs_dist (the distance on
    T = |f0| / A + |f1| / B in place of the difference), abs_dot0 / abs_dot1 [B, 1, H, W] of the backward's two dot products
    sum_c lin t f, and per element the magnitudes of the gradient's own term (2 lin T / A) and of its cross term
    (2 abs_dot / (A^2 r) |f|), both times |gout| / HW."""
    x, y = f0.detach().to(F64).requires_grad_(), f1.detach().to(F64).requires_grad_()
    l = _c(lin, x)
    B, C, H, W = x.shape
    r0, r1 = x.pow(2).sum(1, keepdim=True).sqrt(), y.pow(2).sum(1, keepdim=True).sqrt()
    t = x / (r0 + LPIPS_EPS) - y / (r1 + LPIPS_EPS)
    dist = (l * t * t).sum(1).mean(dim=(1, 2))
    g0 = g1 = None
    if gout is not None:
        g0, g1 = torch.autograd.grad((dist * gout.to(F64)).sum(), [x, y])
    with torch.no_grad():
        xa, ya, la = x.abs(), y.abs(), l.abs()
        A, Bn = r0 + LPIPS_EPS, r1 + LPIPS_EPS
        T = xa / A + ya / Bn
        abs_dist = (la * T * T).sum(1).mean(dim=(1, 2))
        d0, d1 = (la * T * xa).sum(1, keepdim=True), (la * T * ya).sum(1, keepdim=True)
        gs = (gout.to(F64).abs() / (H * W)).view(B, 1, 1, 1) if gout is not None else torch.ones(B, 1, 1, 1, dtype=F64, device=x.device)
        own0, own1 = gs * 2 * la * T / A, gs * 2 * la * T / Bn
        cross0, cross1 = gs * 2 * d0 / (A * A * r0) * xa, gs * 2 * d1 / (Bn * Bn * r1) * ya
    return Lpips(dist.detach(), abs_dist, r0.detach().reshape(B, -1), r1.detach().reshape(B, -1), g0, g1, d0, d1, own0, own1, cross0,
                 cross1)


# ---- layout bridges, relu_gate_add -----------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32(x) rounded to bfloat16, round-to-nearest-even on the bit pattern, as float64 (finite values)."""
    bits = x.float().contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    bits = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffff0000
    bits = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
    return bits.view(torch.float32).double()


def bridge_fwd(x, relu=False):
    """fp32 NCHW -> bf16 NHWC: bf16(relu ? max(x, 0) : x); logical NCHW values."""
    x = x.to(F64)
    return bf16_rne(torch.clamp_min(x, 0.0) if relu else x)


def bridge_bwd(g, gate=None):
    """bf16 NHWC -> fp32 NCHW: g where gate > 0 (both zeros block), all of g without a gate."""
    g = g.to(F64)
    return g if gate is None else torch.where(gate.to(F64) > 0, g, torch.zeros_like(g))


def relu_gate_add(a, b, y):
    a = a.to(F64)
    v, t = (a, a.abs()) if b is None else (a + b.to(F64), a.abs() + b.to(F64).abs())
    live = y.to(F64) > 0
    return Sum(torch.where(live, v, torch.zeros_like(v)), torch.where(live, t, torch.zeros_like(t)))


# ---- MaxPool2d(3, 2) on NHWC values ------------------------------------------------------------------------------------------
def maxpool3s2(x):
    """The literal scan: m = -inf, pos = 0; a tap replaces the maximum when it is greater or when it is a NaN."""
    x = x.to(F64)
    B, C, H, W = x.shape
    ho, wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    m = torch.full((B, C, ho, wo), -float("inf"), dtype=F64, device=x.device)
    pos = torch.zeros((B, C, ho, wo), dtype=torch.uint8, device=x.device)
    for k in range(9):
        kh, kw = divmod(k, 3)
        v = x[:, :, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2]
        upd = (v > m) | torch.isnan(v)
        m, pos = torch.where(upd, v, m), torch.where(upd, torch.full_like(pos, k), pos)
    return NhwcPool(m, pos)


def maxpool3s2_bwd(gy, pos, in_hw):
    gy = gy.to(F64)
    B, C, ho, wo = gy.shape
    out = []
    for g in (gy, gy.abs()):
        acc = torch.zeros(B, C, in_hw[0], in_hw[1], dtype=F64, device=gy.device)
        for k in range(9):
            kh, kw = divmod(k, 3)
            acc[:, :, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2] += torch.where(pos == k, g, torch.zeros_like(g))
        out.append(acc)
    return Sum(out[0], out[1])


# ---- image gradient of a K x K / stride-S convolution ------------------------------------------------------------------------
def conv_image_grad(dy, w, in_hw, S, pad):
    """dx[b][c][ih][iw] = sum_n sum_{kh,kw} dy[b][n][(ih + pad - kh) / S][(iw + pad - kw) / S] * w[n][c][kh][kw], exact divisions
    and in-range rows / columns only."""
    dy, w = dy.to(F64), w.to(F64)
    B, N, Ho, Wo = dy.shape
    C, K = w.shape[1], w.shape[2]
    Hi, Wi = in_hw
    val = torch.zeros(B, C, Hi, Wi, dtype=F64, device=dy.device)
    ab = torch.zeros_like(val)
    ih, iw = torch.arange(Hi, device=dy.device), torch.arange(Wi, device=dy.device)
    for kh in range(K):
        qh = ih + pad - kh
        mh = (qh % S == 0) & (qh >= 0) & (qh < S * Ho)
        if not mh.any():
            continue
        for kw in range(K):
            qw = iw + pad - kw
            mw = (qw % S == 0) & (qw >= 0) & (qw < S * Wo)
            if not mw.any():
                continue
            g = dy[:, :, qh[mh] // S][:, :, :, qw[mw] // S]
            ii, jj = ih[mh][:, None], iw[mw][None, :]
            val[:, :, ii, jj] += torch.einsum("bnhw,nc->bchw", g, w[:, :, kh, kw])
            ab[:, :, ii, jj] += torch.einsum("bnhw,nc->bchw", g.abs(), w[:, :, kh, kw].abs())
    return Sum(val, ab)
