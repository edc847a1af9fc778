"""Float64 definitions of the kernels of csrc/linattn.hip (the attention core forward and backward, ChanNorm forward and
backward, the depthwise 3x3 with its weight gradient): plain torch on any device, no HIP, none of the project's ops.  Every
input is promoted to float64.  Each definition is a function of exactly what the kernel entry point receives: the backward
ones take the saved operands (pre, context, lse; mean, std) as arguments and are the closed forms the kernels implement, not
autograd of the forward.  Activations are logical NCHW.

A result that is a sum comes as Sum(value, abs_terms[, arg_terms]): abs_terms is the same formula on the absolute values of
the operands, the scale of the rounding-error bound of an fp32 evaluation in any order; arg_terms (attention only, in units of
2^-24 like N * abs_terms) carries the rounded differences that feed an exponential: a term that holds exp(k - m) moves by
|k - m| * 2^-24 of itself when k - m is rounded (the tile, chunk and combine differences telescope to k - M), and one that
holds exp(k - lse) by |k - lse| * 2^-23.
tests/test_linattn_defs_cpu.py ties these to autograd, to the definitions of tests/test_attn_gpu.py and to the recorded
reference outputs; tests/test_linattn_gpu.py holds the kernels to them."""
import collections
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
HD = 64
Sum = collections.namedtuple("Sum", "value abs_terms arg_terms", defaults=(None,))
AttnFwd = collections.namedtuple("AttnFwd", "K Q kmax context lse log_s lse_arg pre y")
AttnBwd = collections.namedtuple("AttnBwd", "G dQ dC r dq dk dv")
ChanNormFwd = collections.namedtuple("ChanNormFwd", "y mean std")
ChanNormBwd = collections.namedtuple("ChanNormBwd", "gx dg db")
GELU_GRAD_MAX = 1.13  # max |gelu'| = 1.1289 (at x = 1.4142)


def heads_of(t, heads):
    """[B, 64 heads, H, W] -> float64 [B, heads, N, 64] (pixel-major, as the kernels read NHWC)."""
    b, c, h, w = t.shape
    assert c == HD * heads, (t.shape, heads)
    return t.to(F64).reshape(b, heads, HD, h * w).transpose(2, 3)


def unheads(t, shape):
    """[B, heads, N, 64] -> [B, 64 heads, H, W]"""
    return t.transpose(2, 3).reshape(shape)


def gelu_erf(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def gelu_erf_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_erf_grad_abs(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0)).abs()) + x.abs() * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def row_softmax(q):
    """(Q = softmax over the 64 channels * 64^-0.5, spread = max - min of the row): q [B, heads, N, 64]."""
    m = q.amax(dim=3, keepdim=True)
    e = torch.exp(q - m)
    return e / e.sum(dim=3, keepdim=True) * HD ** -0.5, m - q.amin(dim=3, keepdim=True)


# ---- attention core ----------------------------------------------------------------------------------------------------------
def attn_fwd(q, k, v, heads):
    """K = softmax over the pixels of k per channel, Q = softmax over the channels of q * 64^-0.5,
    context[d, e] = sum_n K[n, d] v[n, e], lse[d] = log sum_n exp(k[n, d]), pre = Q context, y = gelu_erf(pre).
    context [B, heads, 64, 64], lse [B, heads, 64]; pre, y [B, 64 heads, H, W].  lse = kmax + log_s; lse_arg = sum_n K |k - kmax|."""
    shape = q.shape
    q, k, v = heads_of(q, heads), heads_of(k, heads), heads_of(v, heads)
    kmax = k.amax(dim=2, keepdim=True)
    e = torch.exp(k - kmax)
    s = e.sum(dim=2, keepdim=True)
    K = e / s
    karg = kmax - k  # >= 0
    s_arg = (K * karg).sum(dim=2)  # [B, h, d]: the relative argument term of the column sum
    ctx = torch.einsum("bhnd,bhne->bhde", K, v)
    ctx_abs = torch.einsum("bhnd,bhne->bhde", K, v.abs())
    ctx_arg = torch.einsum("bhnd,bhne->bhde", K * karg, v.abs()) + ctx_abs * s_arg[..., None]
    Q, spread = row_softmax(q)
    pre = torch.einsum("bhnd,bhde->bhne", Q, ctx)
    pre_abs = torch.einsum("bhnd,bhde->bhne", Q, ctx_abs)
    pre_arg = torch.einsum("bhnd,bhde->bhne", Q, ctx_arg) + 2 * spread * pre_abs
    pre_v = unheads(pre, shape)
    log_s = torch.log(s).squeeze(2)
    return AttnFwd(K, Q, kmax.squeeze(2), Sum(ctx, ctx_abs, ctx_arg), kmax.squeeze(2) + log_s, log_s, s_arg,
                   Sum(pre_v, unheads(pre_abs, shape), unheads(pre_arg, shape)), gelu_erf(pre_v))


def attn_bwd(q, k, v, pre, gy, context, lse, heads):
    """G = gy gelu'(pre), dQ = G context^T, dq = Q (dQ - sum_d' softmax[d'] dQ[d']), dC = Q^T G, r[d] = sum_e dC[d, e] context[d, e],
    K = exp(k - lse), dv = K dC, dk = K (v dC^T - r)."""
    shape = q.shape
    q, k, v, pre, gy = (heads_of(t, heads) for t in (q, k, v, pre, gy))
    C, lse = context.to(F64), lse.to(F64)
    G, G_abs = gy * gelu_erf_grad(pre), gy.abs() * gelu_erf_grad_abs(pre)
    Q, spread = row_softmax(q)
    qarg = 2 * spread  # relative argument term of one factor Q
    dQ = torch.einsum("bhne,bhde->bhnd", G, C)
    dQ_abs = torch.einsum("bhne,bhde->bhnd", G_abs, C.abs())
    soft = Q * HD ** 0.5
    dot = (soft * dQ).sum(dim=3, keepdim=True)
    dq = Q * (dQ - dot)
    dq_abs = Q * (dQ_abs + (soft * dQ_abs).sum(dim=3, keepdim=True))
    dC = torch.einsum("bhnd,bhne->bhde", Q, G)
    dC_abs = torch.einsum("bhnd,bhne->bhde", Q, G_abs)
    dC_arg = torch.einsum("bhnd,bhne->bhde", Q * qarg, G_abs)
    r = (dC * C).sum(dim=3)
    r_abs, r_arg = (dC_abs * C.abs()).sum(dim=3), (dC_arg * C.abs()).sum(dim=3)
    K = torch.exp(k - lse[:, :, None, :])
    karg = 2 * (k - lse[:, :, None, :]).abs()
    dv = torch.einsum("bhnd,bhde->bhne", K, dC)
    dv_abs = torch.einsum("bhnd,bhde->bhne", K, dC_abs)
    dv_arg = torch.einsum("bhnd,bhde->bhne", K, dC_arg) + torch.einsum("bhnd,bhde->bhne", K * karg, dC_abs)
    vd = torch.einsum("bhne,bhde->bhnd", v, dC)
    vd_abs = torch.einsum("bhne,bhde->bhnd", v.abs(), dC_abs)
    vd_arg = torch.einsum("bhne,bhde->bhnd", v.abs(), dC_arg)
    vd, vd_abs, vd_arg = vd - r[:, :, None, :], vd_abs + r_abs[:, :, None, :], vd_arg + r_arg[:, :, None, :]
    dk, dk_abs = K * vd, K * vd_abs
    dk_arg = K * vd_arg + karg * dk_abs
    u = lambda t: unheads(t, shape)
    return AttnBwd(Sum(G, G_abs), Sum(dQ, dQ_abs), Sum(dC, dC_abs, dC_arg), Sum(r, r_abs, r_arg),
                   Sum(u(dq), u(dq_abs), u(2 * qarg * dq_abs)), Sum(u(dk), u(dk_abs), u(dk_arg)), Sum(u(dv), u(dv_abs), u(dv_arg)))


# ---- ChanNorm ----------------------------------------------------------------------------------------------------------------
def chan_norm_fwd(x, g, b, eps):
    """y = (x - mean) / (std + eps) * g + b over the channels of a pixel, std = sqrt(biased variance); mean, std [B * H * W]
    in pixel order.  The error of the mean is an absolute error of every x - mean: abs_terms of std and y carry mean|x| for it
    (a pixel whose std is 1e-3 of its mean loses three digits there, in any fp32 evaluation)."""
    x, g, b = x.to(F64), g.to(F64).view(1, -1, 1, 1), b.to(F64).view(1, -1, 1, 1)
    mean = x.mean(dim=1, keepdim=True)
    mean_abs = x.abs().mean(dim=1, keepdim=True)
    d = x - mean
    std = (d * d).mean(dim=1, keepdim=True).sqrt()
    inv = 1.0 / (std + eps)
    y = d * inv * g + b
    y_abs = g.abs() * inv * (x.abs() + mean_abs) * (1 + d.abs() * inv) + b.abs()
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1)
    return ChanNormFwd(Sum(y, y_abs), Sum(flat(mean), flat(mean_abs)), Sum(flat(std), flat(std + mean_abs)))


def chan_norm_bwd(x, gy, g, mean, std, eps):
    """From the saved mean and std [B * H * W]:  gh = gy g,  gx = inv (gh - mean_c gh) - inv^2 sum_c(gh d) / (C std) d,
    inv = 1 / (std + eps), the second term 0 at a pixel with std == 0;  dg[c] = sum_p gy d inv,  db[c] = sum_p gy."""
    x, gy, g = x.to(F64), gy.to(F64), g.to(F64).view(1, -1, 1, 1)
    bsz, c, h, w = x.shape
    mu, sd = (t.to(F64).view(bsz, 1, h, w) for t in (mean, std))
    d, inv, gh = x - mu, 1.0 / (sd + eps), gy * g
    s2, s2_abs = (gh * d).sum(dim=1, keepdim=True), (gh * d).abs().sum(dim=1, keepdim=True)
    pos = sd > 0
    safe = torch.where(pos, sd, torch.ones_like(sd))
    coef, coef_abs = (torch.where(pos, inv * inv * t / (c * safe), torch.zeros_like(sd)) for t in (s2, s2_abs))
    gx = inv * (gh - gh.mean(dim=1, keepdim=True)) - coef * d
    gx_abs = inv * (gh.abs() + gh.abs().mean(dim=1, keepdim=True)) + coef_abs * d.abs()
    t = gy * d * inv
    return ChanNormBwd(Sum(gx, gx_abs), Sum(t.sum(dim=(0, 2, 3)), t.abs().sum(dim=(0, 2, 3))),
                       Sum(gy.sum(dim=(0, 2, 3)), gy.abs().sum(dim=(0, 2, 3))))


# ---- depthwise 3x3, pad 1 ----------------------------------------------------------------------------------------------------
def dwconv3x3(x, w):
    """y[b, c, i, j] = sum_{kh, kw} x[b, c, i + kh - 1, j + kw - 1] w[c, 0, kh, kw], zero outside."""
    x, w = x.to(F64), w.to(F64)
    c, (h, wd) = x.shape[1], x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    y, a = torch.zeros_like(x), torch.zeros_like(x)
    for kh in range(3):
        for kw in range(3):
            t = xp[:, :, kh:kh + h, kw:kw + wd] * w[:, 0, kh, kw].view(1, c, 1, 1)
            y, a = y + t, a + t.abs()
    return Sum(y, a)


def dwconv3x3_bwd_data(gy, w):
    """The same operation on the mirrored taps."""
    return dwconv3x3(gy, w.flip(2, 3))


def dwconv3x3_bwd_weight(x, gy):
    """dw[c, 0, kh, kw] = sum_{b, i, j} x[b, c, i + kh - 1, j + kw - 1] gy[b, c, i, j]."""
    x, gy = x.to(F64), gy.to(F64)
    bsz, c, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    dw, a = torch.zeros(c, 1, 3, 3, dtype=F64, device=x.device), torch.zeros(c, 1, 3, 3, dtype=F64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            t = xp[:, :, kh:kh + h, kw:kw + wd] * gy
            dw[:, 0, kh, kw], a[:, 0, kh, kw] = t.sum(dim=(0, 2, 3)), t.abs().sum(dim=(0, 2, 3))
    return Sum(dw, a)
