"""Float64 definitions of the backward glue kernels of csrc/fused_bwd.hip (act_bwd_reduce, modconv_bwd_prep, scale_reduce):
plain torch, no HIP.  Tensors are logical NCHW; every input is promoted to float64 and every constant is built in float64
(`torch.where(c, 1.0, 0.2)` would yield a float32 0.2: 3e-9 off).  Each sum comes with the sum of the absolute values of its
terms, the scale of a rounding-error bound of an fp32 accumulation in any order.
tests/test_bwd_glue_defs_cpu.py checks these against autograd; tests/test_bwd_glue_gpu.py checks the kernels against these."""
import collections

import torch

F64 = torch.float64
ActBwd = collections.namedtuple("ActBwd", "dx sum_bhw abs_bhw sum_hw abs_hw")
ModconvPrep = collections.namedtuple("ModconvPrep", "gz S abs_S")  # S, abs_S: [B, 3, C]
ScaleReduce = collections.namedtuple("ScaleReduce", "gx sum_hw abs_hw")


def _mode(mode):
    """The `lrelu` argument of the hb wrappers: False / None / 0 = no activation, True / 1 = LeakyReLU(0.2), "relu"."""
    if isinstance(mode, str):
        assert mode in ("none", "lrelu", "relu"), mode
        return mode
    return "lrelu" if mode else "none"


def gate(y, mode):
    """Derivative of the activation in terms of its OUTPUT y: 1 where y > 0, else the slope (+0.0 and -0.0 take the slope)."""
    mode = _mode(mode)
    if mode == "none":
        return None
    slope = 0.2 if mode == "lrelu" else 0.0
    y = y.to(F64)
    return torch.where(y > 0, torch.ones((), dtype=F64), torch.full((), slope, dtype=F64))


def noise_plane(noise, h, w):
    """plane[b, h, w] = noise[b, w, h]: the transposed read of the top-left corner of an ns x ns plane, ns >= max(h, w)."""
    assert noise.dim() == 3 and noise.shape[1] == noise.shape[2] and noise.shape[1] >= max(h, w), (noise.shape, h, w)
    return noise.to(F64)[:, :w, :h].transpose(1, 2)


def act_bwd(dy, y, mode, scale):
    """dx = dy * scale * g(y); its sums over (b, h, w) [C] and over (h, w) [B, C]."""
    dx = dy.to(F64) * float(scale)
    g = gate(y, mode)
    if g is not None:
        dx = dx * g
    a = dx.abs()
    return ActBwd(dx, dx.sum(dim=(0, 2, 3)), a.sum(dim=(0, 2, 3)), dx.sum(dim=(2, 3)), a.sum(dim=(2, 3)))


def modconv_prep(gy, y, noise, nw, nb, lrelu, d):
    """Backward prologue of y = act(d[b,c] * z + plane * nw[c] + nb[c]) in terms of the saved y:
    gz = gy * g(y);  t = act^-1(y);  S0 = sum_hw gz * (t - (plane * nw + nb)) (= sum gz * d * z),  S1 = sum_hw gz * plane,
    S2 = sum_hw gz.  Returned tensor: gz * d[b,c] when d is given; the sums always use the unscaled gz.  noise None: no plane."""
    assert _mode(lrelu) in ("none", "lrelu"), "the pre-activation cannot be recovered from a ReLU output"
    gy, y = gy.to(F64), y.to(F64)
    b, c, h, w = gy.shape
    g = gate(y, lrelu)
    gz = gy if g is None else gy * g
    t = y if g is None else torch.where(y > 0, y, 5.0 * y)
    if noise is not None:
        plane = noise_plane(noise, h, w)[:, None]
        n = plane * nw.to(F64).view(1, c, 1, 1) + nb.to(F64).view(1, c, 1, 1)
    else:
        plane, n = torch.zeros(b, 1, h, w, dtype=F64), torch.zeros((), dtype=F64)
    terms = torch.stack([gz * (t - n), gz * plane, gz], dim=1)  # [B, 3, C, H, W]
    out = gz if d is None else gz * d.to(F64)[:, :, None, None]
    return ModconvPrep(out, terms.sum(dim=(3, 4)), terms.abs().sum(dim=(3, 4)))


def scale_reduce(x, t, s):
    """gx = t * s[b,c];  sum_hw x * t  [B, C]  (the gradient with respect to the modulation scale)."""
    x, t = x.to(F64), t.to(F64)
    terms = x * t
    return ScaleReduce(t * s.to(F64)[:, :, None, None], terms.sum(dim=(2, 3)), terms.abs().sum(dim=(2, 3)))
