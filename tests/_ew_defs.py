"""Float64 definitions of the streaming kernels of csrc/elementwise.hip (3x3 reflect blur and its adjoint, plain and
space-to-depth, with the fused activation gate; the fused RGB tail blur(up2(rgb + prev)); bias (+ transposed noise) +
LeakyReLU and its gradient; row-wise sums of squares) and of csrc/torgb.hip (the to-RGB product, its input gradient, the
pixel reduction T and the caller's two contractions of T): plain torch on the CPU, written from the reference's formulas as
explicit index rules and small dense matrices.  No HIP, none of the project's ops.  Tensors are logical NCHW; every input is
promoted to float64 and every constant is built in float64.

A result that is a sum comes as Sum(value, abs_terms): abs_terms is the same formula applied to the absolute values of the
operands (coefficients included), the scale of the rounding-error bound of an fp32 evaluation in any order.
tests/test_ew_defs_cpu.py ties these to the oracle, the recorded reference outputs and autograd;
tests/test_ew_torgb_gpu.py holds the kernels to them."""
import collections

import numpy as np
import torch

F64 = torch.float64
SLOPE = float(np.float32(0.2))  # the kernels' LeakyReLU slope: the fp32 constant 0.2f, evaluated as a double
Sum = collections.namedtuple("Sum", "value abs_terms")
TorgbBwd = collections.namedtuple("TorgbBwd", "gx abs_gx T abs_T")


# ---- index rules as dense matrices -------------------------------------------------------------------------------------
def reflect(i, n):
    """The 'reflect' border of a pad of 1: -1 -> 1, n -> n - 2."""
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


def blur_matrix(n):
    """M [n, n] of the (1, 2, 1) / 4 filter with the reflect border: out[o] = sum_d f[d] * in[reflect(o + d)], n >= 2."""
    assert n >= 2, n
    m = torch.zeros(n, n, dtype=F64)
    for o in range(n):
        for d, f in ((-1, 0.25), (0, 0.5), (1, 0.25)):
            m[o, reflect(o + d, n)] += f
    return m


def up_matrix(n):
    """U [2n, n] of bilinear x2, align_corners=False: out[2k] = .25 in[max(k-1, 0)] + .75 in[k],
    out[2k+1] = .75 in[k] + .25 in[min(k+1, n-1)]."""
    u = torch.zeros(2 * n, n, dtype=F64)
    for k in range(n):
        u[2 * k, max(k - 1, 0)] += 0.25
        u[2 * k, k] += 0.75
        u[2 * k + 1, k] += 0.75
        u[2 * k + 1, min(k + 1, n - 1)] += 0.25
    return u


def _apply(m, x, dim):
    """out = m applied along `dim` of x, by the index rule the matrix stands for: row o of m has a handful of non-zero
    entries (3 for the filters, up to 6 for the adjoint of the RGB tail), gathered with index_select (the cost stays linear in
    the tensor at any size)."""
    nz = m != 0
    k = int(nz.sum(dim=1).max())
    order = torch.argsort(nz.to(torch.int8), dim=1, descending=True, stable=True)[:, :k]  # columns of the non-zeros first
    coef = torch.gather(m, 1, order)  # padded with entries that are zero
    view = [1] * x.dim()
    view[dim] = m.shape[0]
    out = 0
    for j in range(k):
        out = out + coef[:, j].view(view) * x.index_select(dim, order[:, j])
    return out


def _sep(mh, x, mw):
    """out[b,c,p,q] = sum_{h,w} mh[p,h] * x[b,c,h,w] * mw[q,w]; all coefficients here are >= 0, so abs_terms = f(|x|)."""
    x = x.to(F64)
    return Sum(_apply(mw, _apply(mh, x, 2), 3), _apply(mw, _apply(mh, x.abs(), 2), 3))


def _sep_adj(mh, dy, mw):
    """dx[b,c,h,w] = sum_{p,q} mh[p,h] * dy[b,c,p,q] * mw[q,w]."""
    return _sep(mh.t().contiguous(), dy, mw.t().contiguous())


# ---- blur, x2, RGB tail ------------------------------------------------------------------------------------------------
def blur(x):
    """The 3x3 (1,2,1) x (1,2,1) / 16 filter with reflect border (Blur of the reference)."""
    return _sep(blur_matrix(x.shape[2]), x, blur_matrix(x.shape[3]))


def blur_adj(dy):
    """Its transpose: dx[i] = sum_o M[o, i] dy[o]."""
    return _sep_adj(blur_matrix(dy.shape[2]), dy, blur_matrix(dy.shape[3]))


def up2(x):
    return _sep(up_matrix(x.shape[2]), x, up_matrix(x.shape[3]))


def up2_adj(dy):
    return _sep_adj(up_matrix(dy.shape[2] // 2), dy, up_matrix(dy.shape[3] // 2))


def rgb_tail(rgb, prev=None):
    """blur(up2(rgb + prev)): one linear map of the low-resolution sum; abs_terms takes |rgb| + |prev|."""
    rgb = rgb.to(F64)
    s, a = rgb, rgb.abs()
    if prev is not None:
        s, a = s + prev.to(F64), a + prev.to(F64).abs()
    h, w = rgb.shape[2:]
    mh, mw = blur_matrix(2 * h) @ up_matrix(h), blur_matrix(2 * w) @ up_matrix(w)
    return Sum(_apply(mw, _apply(mh, s, 2), 3), _apply(mw, _apply(mh, a, 2), 3))


def rgb_tail_adj(dy):
    """The adjoint of rgb_tail with respect to rgb (and to prev: the same tensor)."""
    h, w = dy.shape[2] // 2, dy.shape[3] // 2
    return _sep_adj(blur_matrix(2 * h) @ up_matrix(h), dy, blur_matrix(2 * w) @ up_matrix(w))


def to_s2d(x):
    """[B, C, H, W] -> [B, 4C, H/2, W/2] with channel = ((h & 1) * 2 + (w & 1)) * C + c."""
    b, c, h, w = x.shape
    assert h % 2 == 0 and w % 2 == 0, x.shape
    out = x.new_zeros(b, 4 * c, h // 2, w // 2)
    for ph in (0, 1):
        for pw in (0, 1):
            k = (ph * 2 + pw) * c
            out[:, k:k + c] = x[:, :, ph::2, pw::2]
    return out


def from_s2d(y):
    b, c4, h2, w2 = y.shape
    assert c4 % 4 == 0, y.shape
    c = c4 // 4
    out = y.new_zeros(b, c, 2 * h2, 2 * w2)
    for ph in (0, 1):
        for pw in (0, 1):
            k = (ph * 2 + pw) * c
            out[:, :, ph::2, pw::2] = y[:, k:k + c]
    return out


def gate(v, g, slope=SLOPE):
    """v where g > 0, else slope * v: +0.0 and -0.0 both take the slope.  slope is a double."""
    v = v.to(F64)
    return torch.where(g.to(F64) > 0, v, float(slope) * v)


# ---- bias (+ noise) + LeakyReLU ----------------------------------------------------------------------------------------
def noise_plane(noise, h, w):
    """plane[b, h, w] = noise[b, w, h]: the transposed read of the top-left corner of an ns x ns plane, ns >= max(h, w)."""
    assert noise.dim() == 3 and noise.shape[1] == noise.shape[2] and noise.shape[1] >= max(h, w), (noise.shape, h, w)
    i, j = torch.arange(h)[:, None], torch.arange(w)[None, :]
    return noise.to(F64)[:, j, i]  # [B, h, w]: element (b, i, j) is noise[b, j, i]


def bias_act(x, bias=None, noise=None, nw=None, nb=None):
    """lrelu(x + bias[c] + noise[b, w, h] * nw[c] + nb[c]), slope float32(0.2) as a double; bias and / or the noise term may
    be absent.  abs_terms: the sum of the absolute values of the terms of the pre-activation."""
    x = x.to(F64)
    b, c, h, w = x.shape
    t, a = x, x.abs()
    if bias is not None:
        bv = bias.to(F64).view(1, c, 1, 1)
        t, a = t + bv, a + bv.abs()
    if noise is not None:
        plane = noise_plane(noise, h, w)[:, None]
        nwv, nbv = nw.to(F64).view(1, c, 1, 1), nb.to(F64).view(1, c, 1, 1)
        t, a = t + (plane * nwv + nbv), a + (plane * nwv).abs() + nbv.abs()
    return Sum(torch.where(t > 0, t, SLOPE * t), a)


def bias_act_bwd(dy, y):
    """dy where the saved OUTPUT y > 0, else float32(0.2) * dy."""
    return gate(dy, y, SLOPE)


def rowwise_sumsq(x):
    x = x.to(F64)
    s = (x * x).sum(dim=1)
    return Sum(s, s.clone())


# ---- to-RGB ------------------------------------------------------------------------------------------------------------
def _w2(w):
    return w.to(F64).reshape(3, -1)


def torgb(x, s1, w):
    """y[b, n, p] = sum_c x[b, c, p] * s1[b, c] * W[n, c]  (Conv2DMod(C, 3, 1, demod=False), s1 = style + 1)."""
    x, s1, w = x.to(F64), s1.to(F64), _w2(w)
    return Sum(torch.einsum("bchw,bc,nc->bnhw", x, s1, w), torch.einsum("bchw,bc,nc->bnhw", x.abs(), s1.abs(), w.abs()))


def torgb_bwd(x, gy, s1, w):
    """gx[b, c, p] = sum_n gy[b, n, p] * s1[b, c] * W[n, c];  T[b, n, c] = sum_p x[b, c, p] * gy[b, n, p].
    gy: [B, 3, H, W] (the first three channels of the kernel's 4-channel storage)."""
    x, gy, s1, w = x.to(F64), gy.to(F64), s1.to(F64), _w2(w)
    assert gy.shape[1] == 3, gy.shape
    return TorgbBwd(torch.einsum("bnhw,bc,nc->bchw", gy, s1, w), torch.einsum("bnhw,bc,nc->bchw", gy.abs(), s1.abs(), w.abs()),
                    torch.einsum("bchw,bnhw->bnc", x, gy), torch.einsum("bchw,bnhw->bnc", x.abs(), gy.abs()))


def torgb_dstyle(T, w, abs_T=None):
    """The caller's contraction: dstyle[b, c] = sum_n W[n, c] * T[b, n, c]."""
    w = _w2(w)
    a = T.abs() if abs_T is None else abs_T
    return Sum(torch.einsum("nc,bnc->bc", w, T.to(F64)), torch.einsum("nc,bnc->bc", w.abs(), a.to(F64)))


def torgb_dw(T, s1, abs_T=None):
    """dW[n, c] = sum_b s1[b, c] * T[b, n, c]."""
    s1 = s1.to(F64)
    a = T.abs() if abs_T is None else abs_T
    return Sum(torch.einsum("bc,bnc->nc", s1, T.to(F64)), torch.einsum("bc,bnc->nc", s1.abs(), a.to(F64)))
