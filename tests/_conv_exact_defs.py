"""Definitions of the conv kernels (forward, data gradient, weight gradient, their space-to-depth forms, to-RGB) and seeded
small-integer operands on which they are EXACT: plain torch on the CPU, no HIP.  Tensors are logical NCHW.

Exactness.  Operands are small integers (per-sample scales: powers of two), all exactly representable in bf16.  Every product
and every partial sum of a definition is then a multiple of `grid` (the product of the smallest scales, a power of two)
bounded by A = the same formula on absolute values.  A / grid < 2^24 — asserted by every definition — makes each of them an
exact fp32 (and fp64) number in ANY summation order, tile shape, K chunking or split-K plan: a kernel that multiplies bf16 by
bf16 and accumulates in fp32 must return the definition bit for bit, and the definition may be evaluated in fp32 or fp64.
The only inexact operation is the fixed LeakyReLU slope: v * float32(0.2), one fp32 multiplication (the kernels' `0.2f * v`).
A bf16 output is ONE round-to-nearest-even of the fp32 value (`.bfloat16()`); the gate slope of the data gradient is 0.25 in
every test, a power of two, which commutes with that rounding; the activation bit mask is the sign of the STORED output.

With exact=False the same formulas run on arbitrary float64 inputs (tests/test_conv_exact_defs_cpu.py checks them against
autograd; the Gaussian layer of tests/test_conv_exact_gpu.py bounds the kernels by r * 2^-8 |want| + TOL32 * A)."""
import collections
import zlib

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
SLOPE32 = torch.tensor(0.2, dtype=F32)       # the kernels' 0.2f
SLOPE = float(SLOPE32)                       # ... as a double: 0.20000000298
GATE_SLOPE = 0.25
Out = collections.namedtuple("Out", "y A")   # the exact value and the sum of the absolute values of its terms
WGrad = collections.namedtuple("WGrad", "dw A db A_db")
ToRGBBwd = collections.namedtuple("ToRGBBwd", "gx A_gx T A_T")


# ---- operands ----------------------------------------------------------------------------------------------------------
def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, shape, lo, hi):
    """Uniform integers of [lo, hi] as float32."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F32)


def scales(g, shape):
    """Per-sample scales drawn from {0.5, 1, 2}."""
    return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, tuple(shape), generator=g)]


def gate_like(g, shape):
    """A gate tensor: non-zero integers of [-3, 3] with about 0.5 % exact +0.0 and 0.5 % exact -0.0 (first / last element too)."""
    t = ints(g, shape, 1, 3) * (ints(g, shape, 0, 1) * 2 - 1)
    f = t.view(-1)
    u = torch.rand(f.numel(), generator=g)
    f[u < 0.005] = 0.0
    f[(u >= 0.005) & (u < 0.01)] = -0.0
    f[0], f[f.numel() - 1] = 0.0, -0.0
    return t


def operands(key, B, C, N, H, W, k=3, stride=1, pad=1, c_res=0, gaussian=False):
    """The seeded integer operands of one conv case (never written after creation): x in [-3, 3] (input grid H x W), w in
    [-2, 2], dy / residual in [-3, 3] and the gate of the output side on the output grid, a gate of the input side, bias /
    noise weight / noise bias in [-4, 4], a noise plane in [0, 3] one to four pixels larger than the output (a multiple of 4: the natural-order epilogue's rule), per-sample scales of
    both channel counts, integer accumulators of the weight and bias gradients, and (c_res > 0) the operands of a merged 1x1
    residual conv over c_res channels on the output grid.
    Deep K (more than 2304 products per output, i.e. 512 channels at 3x3): x, dy and w in [-1, 1] — with the full ranges a
    fifth of the bf16 outputs lies above 256, where bf16 no longer resolves integers (with per-sample scales and the 0.2 slope:
    eighths and fortieths), and the power check of tests/test_conv_exact_defs_cpu.py (>= 90 % of the reached outputs move
    when one product is lost) fell to 0.876 with [-3, 3] x [-2, 2] and to 0.893 with [-2, 2] x [-1, 1].
    gaussian=True: the tensors and the weights are standard normal values rounded to bf16 instead (the second layer of
    tests/test_conv_exact_gpu.py); scales stay powers of two, the fp32 vectors, the noise plane and the accumulators normal."""
    g = gen(key, B, C, N, H, W, k, stride, pad, c_res, gaussian)
    if gaussian:
        rb = lambda *sh: torch.randn(*sh, generator=g).bfloat16().float()  # noqa: E731
        rn = lambda *sh: torch.randn(*sh, generator=g)  # noqa: E731
        ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        ns = (max(ho, wo) + 4) // 4 * 4
        r = dict(x=rb(B, C, H, W), w=rb(N, C, k, k), dy=rb(B, N, ho, wo), res=rb(B, N, ho, wo), gate_in=gate_like(g, (B, C, H, W)),
                 bias=rn(N), nw=rn(N), nb=rn(N), noise=torch.rand(B, ns, ns, generator=g), s_c=scales(g, (B, C)),
                 s_n=scales(g, (B, N)), acc=rn(N, C, k, k), acc_b=rn(N))
        if c_res:
            r["xs"], r["w_res"] = rb(B, c_res, ho, wo), rb(N, c_res)
        return r
    xr, wr = (1, 1) if max(C, N) * k * k > 2304 else (3, 2)
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    ns = (max(ho, wo) + 4) // 4 * 4
    r = dict(x=ints(g, (B, C, H, W), -xr, xr), w=ints(g, (N, C, k, k), -wr, wr), dy=ints(g, (B, N, ho, wo), -xr, xr),
             res=ints(g, (B, N, ho, wo), -3, 3), gate_in=gate_like(g, (B, C, H, W)), bias=ints(g, (N,), -4, 4),
             nw=ints(g, (N,), -4, 4), nb=ints(g, (N,), -4, 4), noise=ints(g, (B, ns, ns), 0, 3), s_c=scales(g, (B, C)),
             s_n=scales(g, (B, N)), acc=ints(g, (N, C, k, k), -64, 64), acc_b=ints(g, (N,), -64, 64))
    if c_res:
        r["xs"], r["w_res"] = ints(g, (B, c_res, ho, wo), -3, 3), ints(g, (N, c_res), -2, 2)
    return r


def s2d(x):
    """Space-to-depth: [B, C, 2H, 2W] -> [B, 4C, H, W], channel (sy * 2 + sx) * C + c = x[b, c, 2h + sy, 2w + sx]."""
    b, c, h2, w2 = x.shape
    return x.view(b, c, h2 // 2, 2, w2 // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(b, 4 * c, h2 // 2, w2 // 2)


def pack_mask(t):
    """uint8 [B, H, W, C/8]: bit k of byte i = (element 8 i + k of the NHWC tensor > 0)."""
    b, c, h, w = t.shape
    bits = (t.permute(0, 2, 3, 1) > 0).reshape(b, h, w, c // 8, 8).to(torch.int32)
    return (bits << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)


def store(v, prec):
    """The kernels' store: fp32 as it is, bf16 by one round-to-nearest-even."""
    v = v.to(F32)
    return v.bfloat16() if prec == "bf16" else v


def _bc(s):
    return None if s is None else s[:, :, None, None]


def _exact(A, grid):
    assert float(A.max()) / grid < 2 ** 24, "sum|terms| / grid = %g: not exact in fp32" % (float(A.max()) / grid)


def _conv(x, w, stride, pad):
    """F.conv2d; on the device (float64 operands of the many-tile cases) as unfold + matmul, which every build serves."""
    if not x.is_cuda:
        return F.conv2d(x, w, None, stride, pad)
    b, _, h, wd = x.shape
    n, _, k, _ = w.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride)  # [B, C k k, Ho Wo]
    return (w.reshape(n, -1) @ cols).reshape(b, n, ho, wo)


def _conv_input(x_shape, w, d, stride, pad):
    if not d.is_cuda:
        return torch.nn.grad.conv2d_input(tuple(x_shape), w, d, stride, pad)
    assert stride == 1 and 2 * pad == w.shape[2] - 1, "device evaluation: same-size stride-1 convs only"
    return _conv(d, w.transpose(0, 1).flip(2, 3), 1, pad)


def _act(v, act, exact):
    if act in (None, False, "none"):
        return v
    if act == "relu":
        return torch.where(v > 0, v, torch.zeros_like(v))
    assert act in (True, "lrelu"), act
    neg = (v.to(F32) * SLOPE).to(v.dtype) if exact else v * SLOPE
    return torch.where(v > 0, v, neg)


# ---- forward -----------------------------------------------------------------------------------------------------------
def forward(x, w, stride, pad, in_scale=None, out_scale=None, bias=None, noise=None, noise_w=None, noise_b=None,
            natural=False, residual=None, res_scale=1.0, second=None, act=None, dt=F32, exact=True, grid=2.0 ** -4):
    """y = act((conv(x * in_scale[b,c], w) * out_scale[b,n] + conv1x1(second) + bias[n] + plane[b,h,w] * noise_w[n] + noise_b[n]
    + residual) * res_scale);  plane = noise[b, w, h] (the reference's transposed read) or noise[b, h, w] (natural=True) of
    the top-left corner of an ns x ns plane;  second = (xs, w_res [N, C_res]): the merged 1x1 residual conv of a block tail.
    Without a residual / second segment res_scale is not applied."""
    def core(x, w, bias, nw, nb, res, sec):
        xs = x if in_scale is None else x * _bc(in_scale.to(dt))
        v = _conv(xs, w, stride, pad)
        if out_scale is not None:
            v = v * _bc(out_scale.to(dt))
        if sec is not None:
            v = v + F.conv2d(sec[0], sec[1][:, :, None, None])
        if bias is not None:
            v = v + bias.view(1, -1, 1, 1)
        if noise is not None:
            ho, wo = v.shape[2:]
            plane = noise.to(dt)[:, :ho, :wo] if natural else noise.to(dt)[:, :wo, :ho].transpose(1, 2)
            v = v + plane[:, None] * nw.view(1, -1, 1, 1) + nb.view(1, -1, 1, 1)
        if res is not None:
            v = v + res
        if res is not None or sec is not None:
            v = v * res_scale
        return v

    c = lambda t: None if t is None else t.to(dt)  # noqa: E731
    a = lambda t: None if t is None else t.to(dt).abs()  # noqa: E731
    sec = None if second is None else (c(second[0]), c(second[1]))
    asec = None if second is None else (a(second[0]), a(second[1]))
    v = core(c(x), c(w), c(bias), c(noise_w), c(noise_b), c(residual), sec)
    A = core(a(x), a(w), a(bias), a(noise_w), a(noise_b), a(residual), asec)
    if exact:
        _exact(A, grid)
    return Out(_act(v, act, exact), A)


# ---- data gradient -----------------------------------------------------------------------------------------------------
def dgrad(dy, w, x_shape, stride, pad, in_scale=None, out_scale=None, gate=None, slope=GATE_SLOPE, dt=F32, exact=True,
          grid=2.0 ** -4):
    """dx = d/dx sum(conv(x, w) * dy * in_scale[b,n]) * out_scale[b,c] * (gate > 0 ? 1 : slope)   (+0.0 and -0.0 take the slope)."""
    def core(dy, w):
        d = dy if in_scale is None else dy * _bc(in_scale.to(dt))
        v = _conv_input(x_shape, w, d, stride, pad)
        return v if out_scale is None else v * _bc(out_scale.to(dt))

    v, A = core(dy.to(dt), w.to(dt)), core(dy.to(dt).abs(), w.to(dt).abs())
    if gate is not None:
        pos = gate.to(dt) > 0
        v, A = torch.where(pos, v, slope * v), torch.where(pos, A, slope * A)
    if exact:
        _exact(A, grid)
    return Out(v, A)


# ---- weight gradient ---------------------------------------------------------------------------------------------------
def wgrad(x, dy, w_shape, stride, pad, x_scale=None, dy_scale=None, out_scale=1.0, acc=None, acc_b=None, dt=F32, exact=True,
          grid=2.0 ** -4):
    """dw = acc + out_scale * d/dw sum(conv(x * x_scale[b,c], w) * dy * dy_scale[b,n]);  db = acc_b + out_scale * sum_bhw dy."""
    def core(x, dy, acc, acc_b):
        xs = x if x_scale is None else x * _bc(x_scale.to(dt))
        ds = dy if dy_scale is None else dy * _bc(dy_scale.to(dt))
        dw = torch.nn.grad.conv2d_weight(xs, tuple(w_shape), ds, stride, pad) * out_scale
        db = dy.sum(dim=(0, 2, 3)) * out_scale
        return (dw if acc is None else dw + acc), (db if acc_b is None else db + acc_b)

    c = lambda t: None if t is None else t.to(dt)  # noqa: E731
    a = lambda t: None if t is None else t.to(dt).abs()  # noqa: E731
    dw, db = core(c(x), c(dy), c(acc), c(acc_b))
    A, A_db = core(a(x), a(dy), a(acc), a(acc_b))
    if exact:
        _exact(A, grid)
        _exact(A_db, grid)
    return WGrad(dw, A, db, A_db)


# ---- space-to-depth forms of the 3x3 / stride-2 / pad-1 conv -----------------------------------------------------------
def s2d_forward(x, w, bias=None, residual=None, res_scale=1.0, second=None, **kw):
    """The stride-2 conv whose input the kernels read space-to-depth (s2d(x)): bias only, (conv + bias + residual) * c, and the
    block tail (conv + bias + conv1x1(xs, w_res)) * c."""
    return forward(x, w, 2, 1, bias=bias, residual=residual, res_scale=res_scale, second=second, **kw)


def s2d_dgrad(dy, w, **kw):
    """Data gradient of the stride-2 conv, STORED space-to-depth: [B, 4C, H, W] for dy [B, N, H, W]."""
    b, _, h, wd = dy.shape
    o = dgrad(dy, w, (b, w.shape[1], 2 * h, 2 * wd), 2, 1, **kw)
    return Out(s2d(o.y), s2d(o.A))


def s2d_wgrad(x, dy, w_shape, out_scale=1.0, acc=None, **kw):
    """Weight gradient of the stride-2 conv in the parameter layout [N, C, 3, 3] (the kernels read s2d(x))."""
    return wgrad(x, dy, w_shape, 2, 1, out_scale=out_scale, acc=acc, **kw)


# ---- to-RGB ------------------------------------------------------------------------------------------------------------
def torgb_fwd(x, s1, w, dt=F32, exact=True, grid=2.0 ** -4):
    """y[b, n] = sum_c x[b, c] * s1[b, c] * w[n, c], n < 3; stored with a fourth channel of zeros.  w: [3, C, 1, 1]."""
    def core(x, w):
        wm = w.reshape(1, 3, -1) * s1.to(dt)[:, None, :]
        y = torch.einsum("bchw,bnc->bnhw", x, wm)
        return torch.cat([y, torch.zeros_like(y[:, :1])], dim=1)

    y, A = core(x.to(dt), w.to(dt)), core(x.to(dt).abs(), w.to(dt).abs())
    if exact:
        _exact(A, grid)
    return Out(y, A)


def torgb_bwd(x, gy, s1, w, dt=F32, exact=True, grid=2.0 ** -4):
    """gx[b, c] = s1[b, c] * sum_n w[n, c] * gy[b, n];  T[b, n, c] = sum_hw x[b, c] * gy[b, n].  gy: 4 channels, the fourth unused."""
    def core(x, gy, w):
        wm = w.reshape(1, 3, -1) * s1.to(dt)[:, None, :]
        return torch.einsum("bnhw,bnc->bchw", gy[:, :3], wm), torch.einsum("bchw,bnhw->bnc", x, gy[:, :3])

    gx, T = core(x.to(dt), gy.to(dt), w.to(dt))
    A_gx, A_T = core(x.to(dt).abs(), gy.to(dt).abs(), w.to(dt).abs())
    if exact:
        _exact(A_gx, grid)
        _exact(A_T, grid)
    return ToRGBBwd(gx, A_gx, T, A_T)
