"""Float64 definitions of the kernels that touch parameters: csrc/adam_pack.hip (the Adam step and the operand copies it
refreshes), csrc/style_coeffs.hip (tap sum of squares, s1, demodulation coefficient and their backward) and
csrc/initial_block.hip (forward, data gradient, weight gradient).  Plain torch on the CPU, no HIP, none of the project's ops.
Every input is promoted to float64; hyper-parameters stay unrounded Python floats.

A result that is a sum comes as Sum(value, abs_terms[, arg_terms]) (the tuple of tests/_linattn_defs.py): abs_terms is the same
formula on the absolute values of the operands, the scale of the rounding-error bound of an fp32 evaluation in any order;
arg_terms, in units of 2^-24 like N * abs_terms, carries what the chain count cannot: the rounding of a constant that enters
through a difference (float(beta) inside 1 - beta moves the gradient term by beta / (1 - beta) of itself), and the error of
a library call's argument (the second moment under the square root; for d the unit d / 2 that one rounding of rsqrt's
argument is worth: tests/test_param_defs_cpu.py multiplies it by the argument's chain).
The backward definitions are functions of the SAVED operands (d, s1), which is the kernels' contract.  The operand copies are
bit-exact definitions: bfloat16(float32(scale) * w), one fp32 product, then round-to-nearest-even.
tests/test_param_defs_cpu.py ties these to torch.optim.Adam, autograd and conv2d; tests/test_param_kernels_gpu.py holds the
kernels to them."""
import collections
import math

import torch

from _linattn_defs import Sum

F64 = torch.float64
AdamStep = collections.namedtuple("AdamStep", "p m v")
ModBwd = collections.namedtuple("ModBwd", "gstyle gw")


# ---- Adam ------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, step, lr, b1, b2, eps):
    """One step, no weight decay / amsgrad / maximize; `step` is the count AFTER the increment (t >= 1).
        m' = b1 m + (1 - b1) g,   v' = b2 v + (1 - b2) g^2,   p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
    arg_terms: m' and v' carry b |g| and b g^2 (the rounding of float(b) seen through 1 - b); p' carries those of m' scaled
    by step_size / denom, and half the relative argument term of v' on the update (the square root halves it)."""
    p, g, m, v = (t.to(F64) for t in (p, g, m, v))
    m1 = b1 * m + (1 - b1) * g
    m1_abs, m1_arg = b1 * m.abs() + (1 - b1) * g.abs(), b1 * g.abs()
    v1 = b2 * v + (1 - b2) * g * g
    v1_arg = b2 * g * g
    ss = lr / (1 - b1 ** step)
    denom = v1.sqrt() / math.sqrt(1 - b2 ** step) + eps
    p1 = p - ss * m1 / denom
    rv = torch.where(v1 > 0, v1_arg / torch.where(v1 > 0, v1, torch.ones_like(v1)), torch.zeros_like(v1))
    upd_abs = ss * m1_abs / denom
    return AdamStep(Sum(p1, p.abs() + upd_abs, ss * m1_arg / denom + upd_abs * rv / 2), Sum(m1, m1_abs, m1_arg), Sum(v1, v1, v1_arg))


# ---- operand copies ----------------------------------------------------------------------------------------------------------
def bf16_of(w32, scale=None):
    """bfloat16(float32(scale) * w): w fp32; the product is one fp32 operation."""
    assert w32.dtype == torch.float32
    if scale is not None:
        w32 = w32 * torch.tensor(scale, dtype=torch.float32)
    return w32.bfloat16()


def pack_fwd(w32, scale=None):
    """[N][T][C], T = kh * kw, of an OIHW weight."""
    n, c = w32.shape[:2]
    return bf16_of(w32, scale).reshape(n, c, -1).permute(0, 2, 1).contiguous()


def pack_bwd(w32, scale=None):
    """[C][T][N]"""
    n, c = w32.shape[:2]
    return bf16_of(w32, scale).reshape(n, c, -1).permute(1, 2, 0).contiguous()


def matrix(w32, scale=None):
    """The bf16 [N][C] matrix of a 1x1 weight, and with N = D the [D][16 C] `initw` matrix of the [D][C][4][4] weight."""
    return bf16_of(w32, scale).reshape(w32.shape[0], -1).contiguous()


def space_to_depth(x):
    """[B, C, 2H, 2W] -> [B, 4C, H, W]: channel (2 sy + sx) C + c of pixel (i, j) is x[c] at (2 i + sy, 2 j + sx)."""
    b, c, h, w = x.shape
    assert h % 2 == 0 and w % 2 == 0
    return x.reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(b, 4 * c, h // 2, w // 2)


def s2d_weight(w):
    """The [N][4C][3][3] weight whose stride-1 / pad-1 convolution over space_to_depth(x) is the 3x3 / stride-2 / pad-1
    convolution of x with w [N][C][3][3].  Output pixel i reads input row 2 i + kh - 1 = 2 (i + oy) + sy, so tap kh sits at
    row offset oy = floor((kh - 1) / 2) in parity plane sy = (kh - 1) mod 2: the taps of offset +1 stay zero."""
    n, c, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    w2 = torch.zeros(n, 4 * c, 3, 3, dtype=w.dtype)
    for a in range(3):
        oy, sy = (a - 1) // 2, (a - 1) % 2
        for b in range(3):
            ox, sx = (b - 1) // 2, (b - 1) % 2
            s = 2 * sy + sx
            w2[:, s * c:(s + 1) * c, oy + 1, ox + 1] = w[:, :, a, b]
    return w2


def s2d_pack_fwd(w32, scale=None):
    """[N][9][4C]: the forward pack of the space-to-depth weight (the zero taps included)."""
    return pack_fwd(s2d_weight(w32), scale)


def s2d_pack_bwd(w32, scale=None):
    """[4C][9][N]"""
    return pack_bwd(s2d_weight(w32), scale)


def wsq(w):
    """wsq[n][c] = sum over the taps of w[n][c][.]^2; every term is positive: abs_terms is the value."""
    w = w.to(F64)
    q = (w * w).reshape(w.shape[0], w.shape[1], -1).sum(dim=2)
    return Sum(q, q)


# ---- style coefficients ------------------------------------------------------------------------------------------------------
def s1_of(style):
    style = style.to(F64)
    return Sum(style + 1, style.abs() + 1)


def demod(style, wsq_, eps):
    """d[b][o] = rsqrt(sum_i (style[b][i] + 1)^2 wsq[o][i] + eps), from the wsq handed in.  Every term of the argument is
    positive, so one rounding on its chain moves d by at most d / 2: arg_terms is that unit."""
    s = style.to(F64) + 1
    d = torch.rsqrt((s * s) @ wsq_.to(F64).t() + eps)
    return Sum(d, d, d / 2)


def _dq(gd, d):
    gd, d = gd.to(F64), d.to(F64)
    return -0.5 * gd * d ** 3


def modcoeff_bwd(gd, d, s1, wsq_, w, gs1=None):
    """gstyle[b][i] = gs1[b][i] + 2 s1[b][i] sum_o dq[b][o] wsq[o][i],  gw[o][i][k] = 2 w[o][i][k] sum_b dq[b][o] s1[b][i]^2,
    dq = -0.5 gd d^3, from the saved d and s1."""
    dq, s1, wsq_, w = _dq(gd, d), s1.to(F64), wsq_.to(F64), w.to(F64)
    g1 = torch.zeros_like(s1) if gs1 is None else gs1.to(F64)
    gs = g1 + 2 * s1 * (dq @ wsq_)
    gs_abs = g1.abs() + 2 * s1.abs() * (dq.abs() @ wsq_)
    acc, acc_abs = dq.t() @ (s1 * s1), dq.abs().t() @ (s1 * s1)
    sh = (w.shape[0], w.shape[1]) + (1,) * (w.dim() - 2)
    return ModBwd(Sum(gs, gs_abs), Sum(2 * w * acc.view(sh), 2 * w.abs() * acc_abs.view(sh)))


# ---- initial block -----------------------------------------------------------------------------------------------------------
def _ib(styles, w):
    styles, w = styles.to(F64), w.to(F64)
    return styles.mean(dim=1), styles.abs().mean(dim=1), w.reshape(w.shape[0], -1)  # avg [B, D], its scale, W [D][16 C]


def initial_block(styles, w):
    """x[b][c][i][j] = sum_d avg[b][d] W[d][c][i][j], avg = mean over L of styles [B, L, D]; W [D, C, 4, 4].  The error of
    avg scales with mean |styles|: abs_terms carries that."""
    avg, avg_abs, wm = _ib(styles, w)
    sh = (styles.shape[0],) + tuple(w.shape[1:])
    return Sum((avg @ wm).view(sh), (avg_abs @ wm.abs()).view(sh))


def initial_block_dstyles(gx, w, l):
    """dstyles[b][l][d] = (1 / L) sum_{c, i, j} gx[b][c][i][j] W[d][c][i][j], the same row for every l."""
    g, wm = gx.to(F64).reshape(gx.shape[0], -1), w.to(F64).reshape(w.shape[0], -1)
    ex = lambda t: (t / l)[:, None, :].expand(-1, l, -1).contiguous()
    return Sum(ex(g @ wm.t()), ex(g.abs() @ wm.abs().t()))


def initial_block_dw(styles, gx):
    """dW[d][c][i][j] = sum_b avg[b][d] gx[b][c][i][j]"""
    avg, avg_abs, _ = _ib(styles, torch.zeros(styles.shape[2], 1))
    g = gx.to(F64).reshape(gx.shape[0], -1)
    sh = (styles.shape[2],) + tuple(gx.shape[1:])
    return Sum((avg.t() @ g).view(sh), (avg_abs.t() @ g.abs()).view(sh))
