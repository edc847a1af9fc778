"""CPU: the float64 definitions of tests/_linattn_defs.py against independent sources, and the comparison that
tests/test_linattn_gpu.py applies to the kernels of csrc/linattn.hip applied to an fp32 torch model of their pass structure.

(a) The forward definitions agree with linattn_def / chan_norm_def / depthwise_def of tests/test_attn_gpu.py, the closed-form
    backward with float64 autograd of those (1e-12 relative), and both with the reference's recorded attn_ops vectors (2e-5 of
    max(1, |tensor|): the fixture is float32).
(b) The model (32-pixel tiles, the chunk plan of attn_plan re-stated in plan_of, the online rescale, the combine in chunk
    order, per-block partials of the parameter sums) stays inside the limits on every input of the GPU file.  The inputs,
    the chain counts N and the limits are fixed here; the GPU file imports them.
(c) Mutations of the model break the same comparison: the exact class is unequal and the Gauss class at least 4 times over
    its limit on some element."""
import collections
import math
import zlib

import numpy as np
import pytest
import torch

import _linattn_defs as D
from conftest import load_golden

F64 = torch.float64
U = 2.0 ** -24
EW = {"fp32": 2.0 ** -22, "bf16": 2.0 ** -8}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
PRECS = ("fp32", "bf16")
TP, HD, MAXCHUNK, NT = 32, 64, 64, 256
ULP_EXP, ULP_LOG, ULP_ERF = 3, 3, 16  # OpenCL full profile


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rnd(t, prec):
    """Rounded to the activation dtype, kept as float32."""
    return t.to(DT[prec]).float()


# ---- the plans, re-stated from csrc/linattn.hip -----------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "nch chunk tiles")  # chunks, pixels per chunk, tiles per chunk


def plan_of(B, heads, HW):
    want = -(-2048 // (B * heads))
    tiles = -(-HW // TP)
    want = max(1, min(want, tiles, MAXCHUNK))
    per = -(-tiles // want)
    return Plan(-(-HW // (per * TP)), per * TP, per)


Stream = collections.namedtuple("Stream", "blocks ppb passes PPB lp")  # blocks, pixels per block, passes of a lane, pixels per pass


def stream_of(P, C):
    lp = int(math.log2(C // 4))
    assert C == 4 << lp and 0 <= lp <= 6, C
    PPB = NT >> lp
    blocks = max(1, min(1024, -(-P // (8 * PPB))))
    ppb = -(-P // blocks)
    return Stream(blocks, ppb, -(-ppb // PPB), PPB, lp)


# ---- chain counts: fp32 roundings on the longest path of a term, without contraction ----------------------------------------
N_Q = ULP_EXP + 1 + (ULP_EXP + 3 + 4 + 1)  # exp; e * s; s = scale / sum(e): exp, 3 lane adds, 4 shuffle adds, the division
N_G = ULP_ERF + 12  # erff, its argument, 1 + ., 0.5 *; x * x, expf, two products, the sum; * gy (x^2 / 2 of the exponent's argument term < 1)


def attn_counts(pl):
    T, nch = pl.tiles, pl.nch
    n_s = ULP_EXP + 8 + 3 + 1 + (ULP_EXP + 2) * (T - 1) + (ULP_EXP + 1 + nch)  # e; 8 + 3 LDS adds; s_run; per further tile al, *, +; combine
    n_ctx = (ULP_EXP + 1 + TP) + (ULP_EXP + 1 + TP) * (T - 1) + (ULP_EXP + 1 + nch + 1) + (1 + n_s)  # tile; rescaled tiles; combine, * invS; 1 / S
    n_dc = N_Q + N_G + 1 + TP * T + nch
    return dict(S=n_s, ctx=n_ctx, pre=n_ctx + N_Q + 1 + HD, G=N_G, dq=N_Q + (N_G + 1 + HD) + (N_Q + 1 + 3 + 4) + 2, dC=n_dc,
                dv=ULP_EXP + n_dc + 1 + HD, dk=ULP_EXP + n_dc + 1 + HD + 2)


def norm_counts(st):
    n_mu = 3 + st.lp  # 1 / C is a power of two
    n_std = n_mu + 1 + (1 + 3 + st.lp) / 2 + 1  # x - mu; half of the sum of squares' chain; sqrt
    tail = st.passes + st.PPB + st.blocks  # a lane's passes, the block's LDS sum, the slices
    return dict(mean=n_mu, std=n_std, y=(n_mu + 1) + (n_std + 2) + 3, gx=18 + st.lp, dg=5 + tail, db=tail, dw=1 + tail, conv=10)


# ---- the comparison, shared with the GPU file -----------------------------------------------------------------------------
def limit(want, n, prec):
    """EW |want| + 2^-24 (N abs_terms + arg_terms), per element."""
    terms = n * want.abs_terms if want.arg_terms is None else n * want.abs_terms + want.arg_terms
    return EW[prec] * want.value.abs() + U * terms


def worst(got, want, lim):
    """max |got - want| / lim; where lim == 0 the result must be exactly 0."""
    got, want = got.detach().to(want.device).double(), want.double()
    assert got.shape == want.shape == lim.shape, (got.shape, want.shape, lim.shape)
    err = (got - want).abs()
    if not bool(torch.isfinite(got).all()) or bool((err[lim == 0] != 0).any()):
        return float("inf")
    nz = lim > 0
    return float((err[nz] / lim[nz]).max()) if bool(nz.any()) else 0.0


def equal_exact(got, want, prec):
    """got == float32(definition), or bfloat16(float32(definition))."""
    expect = want.float() if prec == "fp32" else want.float().bfloat16()
    return got.dtype == DT[prec] and torch.equal(got.detach().to(expect.device), expect)


def fwd_limits(d, cnt, prec):
    """name -> (want, limit, output precision) of the attention forward."""
    lse_lim = EW["fp32"] * d.lse.abs() + U * (ULP_LOG * d.log_s.abs() + cnt["S"] + d.lse_arg)
    pre_terms = cnt["pre"] * d.pre.abs_terms + d.pre.arg_terms
    y_lim = EW[prec] * d.y.abs() + U * ((ULP_ERF / 2 + 3) * d.pre.value.abs() + D.GELU_GRAD_MAX * pre_terms)
    return {"context": (d.context.value, limit(d.context, cnt["ctx"], "fp32"), "fp32"), "lse": (d.lse, lse_lim, "fp32"),
            "pre": (d.pre.value, limit(d.pre, cnt["pre"], prec), prec), "y": (d.y, y_lim, prec)}


def exact_y_limit(d, prec):
    """(want, limit) of y in the exact class: pre equals float32(definition) there (asserted bit for bit), so y is held to
    gelu_erf of that fp32 value with the gelu terms of the limit alone.  (The float64 definition keeps exp(-128) = 2.6e-56 where
    fp32 has 0, so an element whose every fp32 term is 0 has a float64 pre of 1e-57: no fp32 result can be held to that.)"""
    pre = d.pre.value.float().double()
    want = D.gelu_erf(pre)
    return want, EW[prec] * want.abs() + U * (ULP_ERF / 2 + 3) * pre.abs()


def bwd_limits(d, cnt, prec):
    return {n: (getattr(d, n).value, limit(getattr(d, n), cnt[n], prec), prec) for n in ("dq", "dk", "dv")}


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# (B, heads, H, W) -> plan
CORE = {(1, 1, 1, 1): Plan(1, 32, 1), (3, 2, 3, 11): Plan(2, 32, 1), (1, 1, 32, 64): Plan(64, 32, 1), (1, 1, 45, 47): Plan(34, 64, 2),
        (1, 1, 50, 82): Plan(43, 96, 3), (128, 8, 7, 10): Plan(2, 64, 2), (256, 8, 5, 8): Plan(1, 64, 2)}
BIG = [(128, 8, 7, 10), (256, 8, 5, 8)]
GAUSS_CORE = [(c, "plain") for c in CORE] + [(c, kind) for c in CORE if c not in BIG for kind in ("spread", "peaked")]


def _first(scores, size, dim):
    """True at the `size` smallest scores along dim (size broadcasts)."""
    return scores.argsort(dim=dim).argsort(dim=dim) < size


def attn_gauss_inputs(case, kind, prec):
    """q, k, v, gy [B, 64 heads, H, W].  plain: randn * 2.  spread: k uniform in [-30, 30], and column 0 of every head dominated by
    the last pixel (45: the other pixels of the column weigh exp(-75) .. exp(-15), normal fp32 numbers whose products with the
    O(1) factors of dk stay normal).  peaked: every q row has one channel 30 higher.  The two are separate inputs because
    their product, exp(-75) of k times the 1e-13 of a column of dC that no q row favours, lies below 2^-126, where no fp32
    evaluation has a relative precision to be held to."""
    B, heads, H, W = case
    g = gen("attn", case, kind)
    shape = (B, HD * heads, H, W)
    q, k, v, gy = (torch.randn(shape, generator=g) * s for s in (2, 2, 2, 1))
    if kind == "spread":
        k = torch.rand(shape, generator=g) * 60 - 30
        k[:, ::HD, H - 1, W - 1] = 45.0
    elif kind == "peaked":
        top = torch.randint(0, HD, (B, heads, 1, H, W), generator=g)
        q = (q.view(B, heads, HD, H, W) + 30.0 * (torch.arange(HD).view(1, 1, HD, 1, 1) == top)).view(shape)
    else:
        assert kind == "plain", kind
    return tuple(rnd(t, prec) for t in (q, k, v, gy))


def attn_exact_inputs(case):
    """q, k, v, gy, context, lse of the exact class (every value is a bf16 number).  k: 0 on S_d, -128 elsewhere, |S_d| a power of
    two; S_0 = the last pixels of chunk 0 (inside its last tile), S_1 = the last pixels of the last chunk, the others seeded
    subsets that differ per (sample, head, channel).  q: 0 on 2^j channels of a row, j in [0, 3] per pixel.  v in [-4, 4], gy even
    integers in [-8, 8], context k / 4."""
    B, heads, H, W = case
    N = H * W
    pl = plan_of(B, heads, N)
    g = gen("attn-exact", case)
    jmax = int(math.log2(N))
    size = 2 ** (torch.arange(HD) % (jmax + 1))
    member = _first(torch.rand(B, heads, N, HD, generator=g), size.view(1, 1, 1, HD), 2)
    end0 = min(pl.chunk, N)
    n0 = 2 ** int(math.log2(end0 - (end0 - 1) // TP * TP))
    n1 = 2 ** int(math.log2(N - (pl.nch - 1) * pl.chunk))
    pix = torch.arange(N)
    member[:, :, :, 0] = (pix >= end0 - n0) & (pix < end0)
    member[:, :, :, 1] = pix >= N - n1
    assert bool((member.sum(dim=2) == torch.where(torch.arange(HD) == 0, n0, torch.where(torch.arange(HD) == 1, n1, size))).all())
    k = torch.where(member, 0.0, -128.0)
    qsize = 2 ** torch.randint(0, 4, (B, heads, N, 1), generator=g)
    q = torch.where(_first(torch.rand(B, heads, N, HD, generator=g), qsize, 3), 0.0, -128.0)
    shape = (B, HD * heads, H, W)
    nchw = lambda t: D.unheads(t, shape).contiguous()
    v = torch.randint(-4, 5, shape, generator=g).float()
    gy = 2 * torch.randint(-4, 5, shape, generator=g).float()
    context = torch.randint(-4, 5, (B, heads, HD, HD), generator=g).float() / 4
    return nchw(q), nchw(k), v, gy, context, torch.zeros(B, heads, HD)


HOST_C = (4, 8, 16, 32, 64, 128, 256)
PLANES = [(2, 5, 7), (3, 1, 1), (3, 1, 9), (3, 6, 1)]  # (B, H, W): ragged; 1 x 1, 1 x W and H x 1 with B = 3
HOST = [(b, c, h, w) for c in HOST_C for b, h, w in PLANES]
EPS = 1e-5


def norm_inputs(shape, cls, prec, dev="cpu"):
    """x, gy, g, b, eps of a ChanNorm case.  exact: every pixel is m +- s, half the channels on either side, m an integer and s a
    power of two (1 / 2 or 1) per pixel, g and b multiples of 1 / 2, gy integers in [-4, 4], eps = 0: gx, the finest result, is a
    multiple of 2^-11 below 2^8.  gauss: half the pixels randn * 1.5 + 0.3, the others mean * (1 + 1e-3 randn)."""
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(repr(("norm", shape, cls)).encode()))
    r = lambda *s: torch.rand(*s, generator=g, device=dev)
    if cls == "exact":
        sign = torch.where(_first(r(B, C, H, W), C // 2, 1), 1.0, -1.0)
        m = torch.randint(-8, 9, (B, 1, H, W), generator=g, device=dev).float()
        s = 2.0 ** torch.randint(-1, 1, (B, 1, H, W), generator=g, device=dev).float()
        x, gy = m + s * sign, torch.randint(-4, 5, shape, generator=g, device=dev).float()
        gg, bb = (torch.randint(-8, 9, (C,), generator=g, device=dev).float() / 2 for _ in range(2))
        return x, gy, gg, bb, 0.0
    n = lambda *s: torch.randn(*s, generator=g, device=dev)
    x = n(*shape) * 1.5 + 0.3
    tight = (3 + n(B, 1, H, W)) * (1 + 1e-3 * n(*shape))
    x = torch.where(r(B, 1, H, W) < 0.5, x, tight)
    return rnd(x, prec), rnd(n(*shape), prec), 1 + 0.3 * n(C), 0.2 * n(C), EPS


def norm_flat_inputs(shape):
    """The exact class with a pixel of std 0: s = 1 / 2 everywhere and eps = 1 / 2 (std + eps = 1), pixel 0 all channels equal."""
    x, gy, gg, bb, _ = norm_inputs(shape, "exact", "fp32")
    m = (x.amax(dim=1, keepdim=True) + x.amin(dim=1, keepdim=True)) / 2
    x = m + 0.5 * torch.sign(x - m)
    x[0, :, 0, 0] = m[0, 0, 0, 0]
    return x, gy, gg, bb, 0.5


def conv_inputs(shape, cls, prec, dev="cpu"):
    """x, gy, w of a depthwise case.  exact: integers in [-4, 4], weights k / 4."""
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(repr(("dw", shape, cls)).encode()))
    if cls == "exact":
        i = lambda s, lim: torch.randint(-lim, lim + 1, s, generator=g, device=dev).float()
        return i(shape, 4), i(shape, 4), i((C, 1, 3, 3), 8) / 4
    n = lambda *s: torch.randn(*s, generator=g, device=dev)
    return rnd(n(*shape), prec), rnd(n(*shape), prec), n(C, 1, 3, 3) / 3


# ---- the fp32 model of the pass structure --------------------------------------------------------------------------------------
F32 = torch.float32


def _h(t, heads):
    return D.heads_of(t, heads).float()


def _gelu_grad32(x):
    return 0.5 * (1 + torch.erf(x * 0.70710678118654752)) + x * 0.39894228040143268 * torch.exp(-0.5 * x * x)


def _softmax32(q):
    e = torch.exp(q - q.amax(dim=3, keepdim=True))
    return e * (0.125 / e.sum(dim=3, keepdim=True))


def _chunks(t, pl, fill):
    """[B, h, N, 64] -> [B, h, nch, tiles, 32, 64], padded with `fill`."""
    B, h, N, _ = t.shape
    pad = torch.full((B, h, pl.nch * pl.chunk - N, HD), fill, dtype=t.dtype)
    return torch.cat([t, pad], dim=2).view(B, h, pl.nch, pl.tiles, TP, HD)


def model_attn_fwd(q, k, v, heads, prec, mut=None):
    """(y, pre, context, lse) as the three forward kernels compute them, in fp32 torch."""
    shape = q.shape
    q, k, v = _h(q, heads), _h(k, heads), _h(v, heads)
    if mut == "swap_kv":
        k, v = v, k
    B, _, N, _ = k.shape
    pl = plan_of(B, heads, N)
    if mut == "drop_pixel":  # the first pixel of chunk 1 (or of the tensor) never reaches its tile
        p = pl.chunk if pl.nch > 1 else 0
        k, v = k.clone(), v.clone()
        k[:, :, p], v[:, :, p] = -math.inf, 0.0
    kc, vc = _chunks(k, pl, -math.inf), _chunks(v, pl, 0.0)
    if mut == "pad_zero":  # the ragged last tile padded with 0
        flat = kc.view(B, heads, -1, HD)
        flat[:, :, N:-(-N // TP) * TP] = 0.0
    m_run = torch.full((B, heads, pl.nch, HD), -math.inf)
    s_run = torch.zeros(B, heads, pl.nch, HD)
    acc = torch.zeros(B, heads, pl.nch, HD, HD)
    for t in range(pl.tiles):
        kt, vt = kc[:, :, :, t], vc[:, :, :, t]
        m_new = torch.maximum(m_run, kt.amax(dim=3))
        al = torch.exp(m_run - m_new)
        al = torch.where(torch.isnan(al), torch.ones_like(al), al)  # never in the kernel: a chunk's first tile holds a pixel
        e = torch.exp(kt - m_new[:, :, :, None, :])
        s_run = s_run * al + e.sum(dim=3)
        scale = al[..., None]
        if mut == "skip_rescale" and t == pl.tiles - 1:
            scale = scale.clone()
            scale[:, :, 0] = 1.0
        acc = acc * scale + torch.einsum("bhcnd,bhcne->bhcde", e, vt)
        m_run = m_new
    M = m_run.amax(dim=2)
    w = torch.exp(m_run - M[:, :, None])
    S = torch.zeros_like(M)
    ctx = torch.zeros(B, heads, HD, HD)
    wc = w.roll(1, dims=2) if mut == "wrong_max" else w
    for c in range(pl.nch):
        S = S + s_run[:, :, c] * w[:, :, c]
        ctx = ctx + acc[:, :, c] * wc[:, :, c, :, None]
    ctx = ctx * (1.0 / S)[..., None]
    lse = M + torch.log(S)
    use = ctx.roll(1, dims=1) if mut == "next_head" else ctx
    pre = torch.einsum("bhnd,bhde->bhne", _softmax32(q), use)
    y = 0.5 * pre * (1 + torch.erf(pre * 0.70710678118654752))
    out = lambda t: D.unheads(t, shape).to(DT[prec])
    return out(y), out(pre), ctx, lse


def model_attn_bwd(q, k, v, pre, gy, context, lse, heads, prec, mut=None):
    shape = q.shape
    q, k, v, pre, gy = (_h(t, heads) for t in (q, k, v, pre, gy))
    B, _, N, _ = k.shape
    pl = plan_of(B, heads, N)
    C, lse = context.float(), lse.float()
    G = gy * _gelu_grad32(pre)
    Q = _softmax32(q)
    a = torch.einsum("bhne,bhde->bhnd", G, C)
    dot = (Q * a).sum(dim=3, keepdim=True) * 8.0
    dq = Q * (a - dot)
    Qc, Gc = _chunks(Q, pl, 0.0).view(B, heads, pl.nch, pl.chunk, HD), _chunks(G, pl, 0.0).view(B, heads, pl.nch, pl.chunk, HD)
    pdc = torch.einsum("bhcnd,bhcne->bhcde", Qc, Gc)
    dC = torch.zeros(B, heads, HD, HD)
    for c in range(pl.nch):
        dC = dC + pdc[:, :, c]
    r = (dC * C).sum(dim=3)
    if mut == "no_r":
        r = torch.zeros_like(r)
    K = torch.exp(k - lse[:, :, None, :])
    dv = torch.einsum("bhnd,bhde->bhne", K, dC)
    dk = K * (torch.einsum("bhne,bhde->bhnd", v, dC) - r[:, :, None, :])
    out = lambda t: D.unheads(t, shape).to(DT[prec])
    return out(dq), out(dk), out(dv)


def _slices(t, st):
    """[P, ...] -> the per-block partial sums, added in block order."""
    P = t.shape[0]
    pad = torch.zeros((st.blocks * st.ppb - P,) + t.shape[1:], dtype=t.dtype)
    part = torch.cat([t, pad]).view((st.blocks, st.ppb) + t.shape[1:]).sum(dim=1)
    out = torch.zeros_like(part[0])
    for b in range(st.blocks):
        out = out + part[b]
    return out


def model_norm_fwd(x, g, b, eps, prec):
    x, g, b = x.float(), g.float().view(1, -1, 1, 1), b.float().view(1, -1, 1, 1)
    C = x.shape[1]
    mu = x.sum(dim=1, keepdim=True) * (1.0 / C)
    d = x - mu
    sd = torch.sqrt((d * d).sum(dim=1, keepdim=True) * (1.0 / C))
    y = d * (1.0 / (sd + eps)) * g + b
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(-1)
    return y.to(DT[prec]), flat(mu), flat(sd)


def model_norm_bwd(x, gy, g, mean, std, eps, prec, mut=None):
    x, gy, g = x.float(), gy.float(), g.float().view(1, -1, 1, 1)
    B, C, H, W = x.shape
    mu, sd = mean.float().view(B, 1, H, W), std.float().view(B, 1, H, W)
    d, inv, gh = x - mu, 1.0 / (sd + eps), gy * g
    m1 = gh.sum(dim=1, keepdim=True) * (1.0 / C)
    s2 = (gh * d).sum(dim=1, keepdim=True)
    coef = torch.where(sd > 0, inv * inv * s2 * (1.0 / C) / torch.where(sd > 0, sd, torch.ones_like(sd)), torch.zeros_like(sd))
    gx = inv * (gh - m1) - coef * d
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)
    tg, tb = rows(gy * d * inv).clone(), rows(gy).clone()
    if mut == "drop_pixel":
        tg[B * H * W // 2], tb[B * H * W // 2] = 0.0, 0.0
    st = stream_of(B * H * W, C)
    return gx.to(DT[prec]), _slices(tg, st), _slices(tb, st)


def model_conv(x, w, prec, mut=None):
    x, w = x.float(), w.float()
    B, C, H, W = x.shape
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    if mut == "border_tap":  # the tap above the first row reads the first row
        xp[:, :, 0] = xp[:, :, 1]
    y = torch.zeros_like(x)
    for kh in range(3):
        for kw in range(3):
            y = y + xp[:, :, kh:kh + H, kw:kw + W] * w[:, 0, kh, kw].view(1, C, 1, 1)
    return y.to(DT[prec])


def model_conv_wgrad(x, gy, mut=None):
    x, gy = x.float(), gy.float()
    B, C, H, W = x.shape
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    st = stream_of(B * H * W, C)
    dw = torch.zeros(C, 1, 3, 3)
    for kh in range(3):
        for kw in range(3):
            t = (xp[:, :, kh:kh + H, kw:kw + W] * gy).permute(0, 2, 3, 1).reshape(-1, C).clone()
            if mut == "drop_pixel" and (kh, kw) == (1, 1):
                t[B * H * W // 2] = 0.0
            dw[:, 0, kh, kw] = _slices(t, st)
    return dw


# ---- running a model through the comparison ------------------------------------------------------------------------------------
def saved_for_bwd(d, prec):
    """What the backward entry point is handed in the Gauss class: the definition's pre rounded to the activation dtype, its
    context and lse rounded to fp32."""
    return rnd(d.pre.value, prec), d.context.value.float().contiguous(), d.lse.float().contiguous()


def attn_gauss_ratios(case, kind, prec, fwd, bwd):
    """name -> worst error / limit of every output of fwd(q, k, v) -> (y, pre, context, lse) and
    bwd(q, k, v, pre, gy, context, lse) -> (dq, dk, dv)."""
    heads = case[1]
    q, k, v, gy = attn_gauss_inputs(case, kind, prec)
    cnt = attn_counts(plan_of(case[0], heads, case[2] * case[3]))
    d = D.attn_fwd(q, k, v, heads)
    y, pre, context, lse = fwd(q, k, v)
    got = dict(y=y, pre=pre, context=context, lse=lse)
    res = {}
    for name, (want, lim, op) in fwd_limits(d, cnt, prec).items():
        assert got[name].dtype == DT[op], name
        res[name] = worst(got[name], want, lim)
    pre_s, ctx_s, lse_s = saved_for_bwd(d, prec)
    db = D.attn_bwd(q, k, v, pre_s, gy, ctx_s, lse_s, heads)
    got = dict(zip(("dq", "dk", "dv"), bwd(q, k, v, pre_s, gy, ctx_s, lse_s)))
    for name, (want, lim, op) in bwd_limits(db, cnt, prec).items():
        assert got[name].dtype == DT[op], name
        res[name] = worst(got[name], want, lim)
    return res


def attn_exact_results(case, prec, fwd, bwd):
    """name -> bool: pre, context of fwd and dq, dk, dv of bwd equal the rounded definition; the sums are asserted to be exact in
    fp32 (abs_terms in units of the terms' granularity below 2^24)."""
    heads = case[1]
    q, k, v, gy, context, lse = attn_exact_inputs(case)
    d = D.attn_fwd(q, k, v, heads)
    jmax = int(math.log2(case[2] * case[3]))
    assert float(d.context.abs_terms.max()) * 2 ** jmax < 2 ** 24 and float(d.pre.abs_terms.max()) * 2 ** (jmax + 6) < 2 ** 24
    y, pre, ctx, lse_got = fwd(q, k, v)
    res = dict(pre=equal_exact(pre, d.pre.value, prec), context=equal_exact(ctx, d.context.value, "fp32"))
    pre0 = torch.zeros_like(q)
    db = D.attn_bwd(q, k, v, pre0, gy, context, lse, heads)
    for s, gran in ((db.dC, 6), (db.r, 8), (db.dq, 8), (db.dk, 8), (db.dv, 6)):
        assert float(s.abs_terms.max()) * 2 ** gran < 2 ** 24
    dq, dk, dv = bwd(q, k, v, pre0, gy, context, lse)
    res.update(dq=equal_exact(dq, db.dq.value, prec), dk=equal_exact(dk, db.dk.value, prec), dv=equal_exact(dv, db.dv.value, prec))
    return res, (d, y, lse_got)


# ---- (a) the definitions against independent sources ---------------------------------------------------------------------------
def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_definitions_agree_with_the_older_ones_and_with_autograd():
    import test_attn_gpu as old

    g = gen("defs")
    heads, shape = 2, (2, 128, 3, 5)
    q, k, v, r = (torch.randn(shape, generator=g, dtype=F64) * 2 for _ in range(4))
    d = D.attn_fwd(q, k, v, heads)
    y, (gq, gk, gv) = old.grads_of(lambda a, b, c: old.linattn_def(a, b, c, heads), [q, k, v], r)
    assert rel(d.y, y) <= 1e-12
    db = D.attn_bwd(q, k, v, d.pre.value, r, d.context.value, d.lse, heads)
    for name, want in (("dq", gq), ("dk", gk), ("dv", gv)):
        assert rel(getattr(db, name).value, want) <= 1e-12, name
        assert bool((getattr(db, name).abs_terms >= getattr(db, name).value.abs() * (1 - 1e-12)).all()), name
    x, gy = torch.randn(2, 16, 3, 5, generator=g, dtype=F64) * 1.5 + 0.3, torch.randn(2, 16, 3, 5, generator=g, dtype=F64)
    gg, bb, w = torch.randn(16, generator=g, dtype=F64), torch.randn(16, generator=g, dtype=F64), torch.randn(16, 1, 3, 3, generator=g, dtype=F64)
    f = D.chan_norm_fwd(x, gg, bb, EPS)
    y, (gx, dg, dbb) = old.grads_of(lambda a, b, c: old.chan_norm_def(a, b.view(1, -1, 1, 1), c.view(1, -1, 1, 1), EPS), [x, gg, bb], gy)
    bw = D.chan_norm_bwd(x, gy, gg, f.mean.value, f.std.value, EPS)
    assert rel(f.y.value, y) <= 1e-12 and rel(bw.gx.value, gx) <= 1e-12 and rel(bw.dg.value, dg) <= 1e-12 and rel(bw.db.value, dbb) <= 1e-12
    y, (gx, dw) = old.grads_of(old.depthwise_def, [x, w], gy)
    assert rel(D.dwconv3x3(x, w).value, y) <= 1e-12 and rel(D.dwconv3x3_bwd_data(gy, w).value, gx) <= 1e-12
    assert rel(D.dwconv3x3_bwd_weight(x, gy).value, dw) <= 1e-12


def _close_to_fixture(gold, got, what):
    a = torch.from_numpy(np.asarray(gold)).double()
    assert a.shape == got.shape, (what, a.shape, got.shape)
    err, scale = float((a - got).abs().max()), max(1.0, float(a.abs().max()))
    assert err <= 2e-5 * scale, "%s: %.3e of %.3e" % (what, err, scale)


@pytest.mark.parametrize("case", ["a", "b"])
def test_definitions_agree_with_the_recorded_reference(case):
    g = load_golden("attn_ops")
    t = lambda key: torch.from_numpy(g[key]).double()
    tag = "chan_norm_" + case
    x, r, gg, bb = t(tag + "/x"), t(tag + "/r"), t(tag + "/sd/g").flatten(), t(tag + "/sd/b").flatten()
    f = D.chan_norm_fwd(x, gg, bb, EPS)
    bw = D.chan_norm_bwd(x, r, gg, f.mean.value, f.std.value, EPS)
    for key, got in (("/y", f.y.value), ("/gx", bw.gx.value), ("/g/g", bw.dg.value.view(1, -1, 1, 1)), ("/g/b", bw.db.value.view(1, -1, 1, 1))):
        _close_to_fixture(g[tag + key], got, tag + key)
    tag = "depthwise_" + case
    x, r, w0, w1 = t(tag + "/x"), t(tag + "/r"), t(tag + "/sd/net.0.weight"), t(tag + "/sd/net.1.weight")[:, :, 0, 0]
    mid = D.dwconv3x3(x, w0).value
    gmid = torch.einsum("oc,bohw->bchw", w1, r)
    _close_to_fixture(g[tag + "/y"], torch.einsum("oc,bchw->bohw", w1, mid), tag + "/y")
    _close_to_fixture(g[tag + "/gx"], D.dwconv3x3_bwd_data(gmid, w0).value, tag + "/gx")
    _close_to_fixture(g[tag + "/g/net.0.weight"], D.dwconv3x3_bwd_weight(x, gmid).value, tag + "/g/net.0.weight")
    tag = "linattn_" + case
    heads = int(g["heads"][list(g["cases"]).index(case)])
    x, r = t(tag + "/x"), t(tag + "/r")
    wq, wkv, wo = (t(tag + "/sd/" + n)[:, :, 0, 0] for n in ("to_q.weight", "to_kv.net.1.weight", "to_out.weight"))
    conv1 = lambda w, a: torch.einsum("oc,bchw->bohw", w, a)
    mid = D.dwconv3x3(x, t(tag + "/sd/to_kv.net.0.weight")).value
    q, (k, v) = conv1(wq, x), conv1(wkv, mid).chunk(2, dim=1)
    d = D.attn_fwd(q, k, v, heads)
    _close_to_fixture(g[tag + "/y"], conv1(wo, d.y) + t(tag + "/sd/to_out.bias").view(1, -1, 1, 1), tag + "/y")
    db = D.attn_bwd(q, k, v, d.pre.value, torch.einsum("oc,bohw->bchw", wo, r), d.context.value, d.lse, heads)
    _close_to_fixture(g[tag + "/g/to_q.weight"][:, :, 0, 0], torch.einsum("bohw,bchw->oc", db.dq.value, x), tag + " to_q")
    _close_to_fixture(g[tag + "/g/to_kv.net.1.weight"][:, :, 0, 0],
                      torch.einsum("bohw,bchw->oc", torch.cat([db.dk.value, db.dv.value], dim=1), mid), tag + " to_kv")


# ---- (b) the unmutated model stays inside the limits -----------------------------------------------------------------------------
def test_the_plans_are_the_ones_listed():
    for (B, heads, H, W), pl in CORE.items():
        assert plan_of(B, heads, H * W) == pl, (B, heads, H, W)
    assert stream_of(33024, 256)[:3] == (1024, 33, 9) and stream_of(1025 * 2048, 4)[:3] == (1024, 2050, 9)


def model_pair(prec, mut=None):
    fwd = lambda q, k, v: model_attn_fwd(q, k, v, q.shape[1] // HD, prec, mut)
    bwd = lambda q, k, v, pre, gy, c, l: model_attn_bwd(q, k, v, pre, gy, c, l, q.shape[1] // HD, prec, mut)
    return fwd, bwd


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case,kind", GAUSS_CORE, ids=["%s-%s" % ("x".join(map(str, c)), k) for c, k in GAUSS_CORE])
def test_attention_model_is_inside_the_gauss_limits(case, kind, prec):
    res = attn_gauss_ratios(case, kind, prec, *model_pair(prec))
    print(case, kind, prec, {k: round(v, 4) for k, v in res.items()})
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", [c for c in CORE if c not in BIG], ids=lambda c: "x".join(map(str, c)))
def test_attention_model_is_exact_on_the_exact_class(case, prec):
    res, (d, y, lse) = attn_exact_results(case, prec, *model_pair(prec))
    assert all(res.values()), res
    want, lim, _ = fwd_limits(d, attn_counts(plan_of(case[0], case[1], case[2] * case[3])), prec)["lse"]
    assert worst(lse, want, lim) <= 1.0 and worst(y, *exact_y_limit(d, prec)) <= 1.0


NORM_GRAN = dict(y=1, mean=1, std=1, gx=11, dg=1, db=0)  # the exact class: -log2 of the unit the terms are multiples of


def norm_ratios(shape, cls, prec, fwd, bwd, inputs=None, only=None):
    """ChanNorm: name -> error / limit (gauss) or equality (exact) of y, mean, std, gx, dg, db (or of those named in `only`)."""
    x, gy, gg, bb, eps = inputs or norm_inputs(shape, cls, prec)
    B, C, H, W = shape
    cnt = norm_counts(stream_of(B * H * W, C))
    f = D.chan_norm_fwd(x, gg, bb, eps)
    y, mean, std = fwd(x, gg, bb, eps)
    mean_s, std_s = f.mean.value.float(), f.std.value.float()  # the backward's saved operands: the definition's, rounded
    bw = D.chan_norm_bwd(x, gy, gg, mean_s, std_s, eps)
    gx, dg, db = bwd(x, gy, gg, mean_s, std_s, eps)
    res = {}
    for name, got, want, op in (("y", y, f.y, prec), ("mean", mean, f.mean, "fp32"), ("std", std, f.std, "fp32"), ("gx", gx, bw.gx, prec),
                                ("dg", dg, bw.dg, "fp32"), ("db", db, bw.db, "fp32")):
        if only and name not in only:
            continue
        if cls == "exact":
            assert float(want.abs_terms.max()) * 2 ** NORM_GRAN[name] < 2 ** 24, name
            res[name] = equal_exact(got, want.value, op)
        else:
            assert got.dtype == DT[op], name
            res[name] = worst(got, want.value, limit(want, cnt[name], op))
    return res


def conv_ratios(shape, cls, prec, conv, wgrad, inputs=None):
    x, gy, w = inputs or conv_inputs(shape, cls, prec)
    B, C, H, W = shape
    res = {}
    wants = []
    if conv is not None:
        wants = [("fwd", conv(x, w), D.dwconv3x3(x, w), prec, 10), ("bwd_data", conv(gy, w.flip(2, 3)), D.dwconv3x3_bwd_data(gy, w), prec, 10)]
    if wgrad is not None:
        wants.append(("bwd_weight", wgrad(x, gy), D.dwconv3x3_bwd_weight(x, gy), "fp32", norm_counts(stream_of(B * H * W, C))["dw"]))
    for name, got, want, op, n in wants:
        if cls == "exact":
            assert float(want.abs_terms.max()) * (1 if name == "bwd_weight" else 4) < 2 ** 24, name  # products of integers; weights k / 4
            res[name] = equal_exact(got, want.value, op)
        else:
            assert got.dtype == DT[op], name
            res[name] = worst(got, want.value, limit(want, n, op))
    return res


def model_norm_pair(prec, mut=None):
    return (lambda x, g, b, eps: model_norm_fwd(x, g, b, eps, prec)), (lambda x, gy, g, m, s, eps: model_norm_bwd(x, gy, g, m, s, eps, prec, mut))


def model_conv_pair(prec, mut=None, mut_w=None):
    return (lambda x, w: model_conv(x, w, prec, mut)), (lambda x, gy: model_conv_wgrad(x, gy, mut_w))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", HOST, ids=lambda s: "x".join(map(str, s)))
def test_host_width_models_are_inside_the_limits(shape, prec):
    for cls in ("exact", "gauss"):
        for res in (norm_ratios(shape, cls, prec, *model_norm_pair(prec)), conv_ratios(shape, cls, prec, *model_conv_pair(prec))):
            assert all((v is True) if cls == "exact" else v <= 1.0 for v in res.values()), (cls, res)
    res = norm_ratios(shape, "exact", prec, *model_norm_pair(prec), inputs=norm_flat_inputs(shape))
    assert all(res.values()), res


# ---- (c) mutations ---------------------------------------------------------------------------------------------------------------
MUT_CASE = (2, 2, 45, 47)  # 34 chunks of 2 tiles, the last of 3 pixels; two heads
ATTN_MUTATIONS = {"drop_pixel": ("context", "pre"), "skip_rescale": ("context",), "wrong_max": ("context",), "swap_kv": ("context", "pre"),
                  "next_head": ("pre",), "pad_zero": ("context",), "no_r": ("dk",)}


def test_mutation_case_has_the_plan_it_is_chosen_for():
    assert plan_of(2, 2, 45 * 47) == Plan(34, 64, 2)


@pytest.mark.parametrize("mut", list(ATTN_MUTATIONS))
def test_attention_mutations_break_the_comparison(mut):
    exact, _ = attn_exact_results(MUT_CASE, "fp32", *model_pair("fp32", mut))
    gauss = attn_gauss_ratios(MUT_CASE, "plain", "fp32", *model_pair("fp32", mut))
    print(mut, exact, {k: round(v, 2) for k, v in gauss.items()})
    for name in ATTN_MUTATIONS[mut]:
        assert not exact[name], (mut, name, "exact class")
        assert gauss[name] >= 4.0, (mut, name, gauss[name])


def test_host_width_mutations_break_the_comparison():
    shape = (2, 16, 5, 7)
    for cls in ("exact", "gauss"):
        bad = lambda v: (v is False) if cls == "exact" else v >= 4.0
        res = norm_ratios(shape, cls, "fp32", *model_norm_pair("fp32", "drop_pixel"))
        assert bad(res["dg"]) and bad(res["db"]), (cls, res)
        res = conv_ratios(shape, cls, "fp32", *model_conv_pair("fp32", "border_tap"))
        assert bad(res["fwd"]) and bad(res["bwd_data"]), (cls, res)
        res = conv_ratios(shape, cls, "fp32", *model_conv_pair("fp32", None, "drop_pixel"))
        assert bad(res["bwd_weight"]), (cls, res)
