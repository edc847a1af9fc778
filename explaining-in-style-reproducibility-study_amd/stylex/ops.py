"""Differentiable ops of the StylEx hot path on the HIP kernels.

Every op is a ``torch.autograd.Function`` whose backward is itself built from
Functions of this file, so arbitrary-order differentiation works — needed for
``gradient_penalty`` (double backward through D, reference
stylex/stylex_train.py:296-303) and ``calc_pl_lengths`` (through G, :306-316).
The three convolution roles are closed under differentiation:

    Conv(x,w)    --bwd-->  Dgrad(gy,w), Wgrad(x,gy)
    Dgrad(gy,w)  --bwd-->  Conv(ggx,w), Wgrad(ggx,gy)
    Wgrad(x,gy)  --bwd-->  Dgrad(gy,ggw), Conv(x,ggw)

Tensors are logically NCHW (reference API) and physically NHWC
(``torch.channels_last``); activations are fp32 in the parity mode and bf16 in
the speed mode (``set_precision``).  First-order-only passes take the fused
once-differentiable Functions (``set_fast``); double-differentiable passes use
the same fused forward kernels with a backward composed of the Functions above.

The module-level functions (``conv2d`` …) dispatch to an *implementation
object*.  The default and only product implementation is the HIP one below; it
raises if the library or a GPU is missing.  ``tests/`` may install a CPU test
double with ``use_impl`` to exercise the host logic without a GPU.
"""
import collections
import math
import os

import torch
from contextlib import nullcontext as _nullcontext
import torch.nn.functional as F

import hip_backend as hb

_PRECISION = hb.F32


_NAMES = {"fp32": hb.F32, "f32": hb.F32, "bf16": hb.BF16_ACT, "bf16_f32act": hb.BF16}


def set_precision(name):
    """'fp32'        exact f32 MFMA, fp32 tensors (parity mode);
    'bf16'        bf16 MFMA operands + bf16 activation tensors in HBM, fp32 accumulate / parameters / reductions;
    'bf16_f32act' bf16 MFMA operands with fp32 activation tensors."""
    global _PRECISION
    _PRECISION = _NAMES[name]


def get_precision():
    return {hb.F32: "fp32", hb.BF16_ACT: "bf16", hb.BF16: "bf16_f32act"}[_PRECISION]


def act_dtype():
    return hb.act_dtype(_PRECISION)


def _cl(t):
    """channels_last + the activation dtype of the current precision mode."""
    return hb.to_cl(t, hb.act_dtype(_PRECISION))


def _act(t):
    """Differentiable cast of an incoming tensor to the activation dtype (no-op in fp32 modes)."""
    if t is None:
        return None
    adt = hb.act_dtype(_PRECISION)
    return t if t.dtype == adt else t.to(adt)


# ------------------------------------------------------------------------------------------
# convolution triad
# ------------------------------------------------------------------------------------------


_INPUTS_ONLY = False


class inputs_only:
    """Context for `torch.autograd.grad(..., inputs=<activations>)` calls (gradient penalty, path length):
    autograd asks every Function for ALL its input gradients even when only the data path is wanted, so the
    weight/bias gradients of that first backward would be computed and thrown away.  Inside this context the
    conv Functions skip them."""

    def __enter__(self):
        global _INPUTS_ONLY
        self.prev, _INPUTS_ONLY = _INPUTS_ONLY, True

    def __exit__(self, *exc):
        global _INPUTS_ONLY
        _INPUTS_ONLY = self.prev


def _want_param_grad(ctx, i):
    return ctx.needs_input_grad[i] and not _INPUTS_ONLY


# How the launches of one plain conv run: stride, pad, s2d (C of the original stride-2 conv when the input is its
# space-to-depth image, else 0) and gemm (the static half of _gemm_1x1).  Made by _conv_plan; the triad and _ConvBiasActDD keep
# it in ctx and hand it to the nodes their backward creates, so a double backward takes the route its forward chose.
_ConvLaunch = collections.namedtuple("_ConvLaunch", "stride pad s2d gemm")


def _gemm_1x1(t, launch):
    """A 1x1 / stride-1 conv in the bf16 mode is a plain GEMM: forward and data gradient of the composable
    (double-differentiable) triad go to hipBLASLt like the fused DiscriminatorBlock's residual conv (17-130 TF/s on the
    generic kernel, 3.2 ms per gradient-penalty step).  The WEIGHT gradient stays on the deterministic split-K kernel:
    letting ATen differentiate an addmm instead made two identically seeded Trainers diverge (its K = B*H*W weight-
    gradient GEMM takes a split-K algorithm with atomic accumulation; tools/determinism_check.py 4 of 4 runs).
    launch.gemm: what shapes, mode and switches say (_conv_plan); what the tensor says is asked here."""
    return launch.gemm and t.is_cuda and t.dtype == torch.bfloat16


def _fwd(x, w, launch, **epi):
    """conv forward; the GEMM has no epilogue other than the bias."""
    if _gemm_1x1(x, launch) and not any(v is not None and v is not False for k, v in epi.items()
                                        if k not in ("bias", "res_scale")):
        return hb.conv1x1_gemm_fwd(_cl(x), w, epi.get("bias"))
    if launch.s2d:
        return hb.conv2d_fwd_s2d(x, w, _PRECISION, **epi)
    return hb.conv2d_fwd(x, w, launch.stride, launch.pad, _PRECISION, **epi)


def _bwd_data(gy, w, x_shape, launch):
    if _gemm_1x1(gy, launch):
        return hb.conv1x1_gemm_bwd_data(_cl(gy), w)
    if launch.s2d:
        return hb.conv2d_bwd_data_s2d(gy, w, x_shape, _PRECISION)
    return hb.conv2d_bwd_data(gy, w, x_shape, launch.stride, launch.pad, _PRECISION)


def _bwd_weight(x, gy, w_shape, launch):
    if launch.s2d:
        return hb.conv2d_bwd_weight_s2d(x, gy, tuple(w_shape), _PRECISION)
    return hb.conv2d_bwd_weight(x, gy, w_shape, launch.stride, launch.pad, _PRECISION)


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, launch):
        x = _cl(x)
        ctx.save_for_backward(x, w)
        ctx.launch = launch
        return _fwd(x, w, launch)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _Dgrad.apply(gy, w, tuple(x.shape), ctx.launch)
        if _want_param_grad(ctx, 1):
            gw = _Wgrad.apply(x, gy, tuple(w.shape), ctx.launch)
        return gx, gw, None


class _Dgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gy, w, x_shape, launch):
        gy = _cl(gy)
        ctx.save_for_backward(gy, w)
        ctx.launch = launch
        return _bwd_data(gy, w, x_shape, launch)

    @staticmethod
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        d_gy = d_w = None
        if ctx.needs_input_grad[0]:
            d_gy = _Conv.apply(ggx, w, ctx.launch)
        if _want_param_grad(ctx, 1):
            d_w = _Wgrad.apply(ggx, gy, tuple(w.shape), ctx.launch)
        return d_gy, d_w, None, None


class _Wgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gy, w_shape, launch):
        x, gy = _cl(x), _cl(gy)
        ctx.save_for_backward(x, gy)
        ctx.launch = launch
        return _bwd_weight(x, gy, w_shape, launch)

    @staticmethod
    def backward(ctx, ggw):
        x, gy = ctx.saved_tensors
        d_x = d_gy = None
        ggw = ggw.contiguous()
        if ctx.needs_input_grad[0]:
            d_x = _Dgrad.apply(gy, ggw, tuple(x.shape), ctx.launch)
        if ctx.needs_input_grad[1]:
            d_gy = _Conv.apply(x, ggw, ctx.launch)
        return d_x, d_gy, None, None


# ------------------------------------------------------------------------------------------
# bias + LeakyReLU(0.2)
# ------------------------------------------------------------------------------------------


class _BiasAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        x = _cl(x)
        y = hb.bias_act_fwd(x, bias)
        ctx.save_for_backward(y)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gx = _BiasActBwd.apply(gy, y)
        gb = None
        if ctx.has_bias and _want_param_grad(ctx, 1):
            gb = _channel_sum(gx) if (not torch.is_grad_enabled() and gx.is_cuda and hb.is_cl(gx)) else gx.sum(dim=(0, 2, 3), dtype=torch.float32)
        return gx, gb


class _BiasActBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gy, y):
        gy = _cl(gy)
        ctx.save_for_backward(y)
        return hb.bias_act_bwd(gy, y)

    @staticmethod
    def backward(ctx, ggx):
        (y,) = ctx.saved_tensors
        return _BiasActBwd.apply(ggx, y), None


# ------------------------------------------------------------------------------------------
# resampling (both linear: the adjoint's adjoint is the op itself)
# ------------------------------------------------------------------------------------------


class _Up(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return hb.upsample2x_fwd(_cl(x))

    @staticmethod
    def backward(ctx, gy):
        return _UpBwd.apply(gy)


class _UpBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gy):
        return hb.upsample2x_bwd(_cl(gy))

    @staticmethod
    def backward(ctx, ggx):
        return _Up.apply(ggx)


class _Blur(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return hb.blur3x3_fwd(_cl(x))

    @staticmethod
    def backward(ctx, gy):
        return _BlurBwd.apply(gy)


class _BlurBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gy):
        return hb.blur3x3_bwd(_cl(gy))

    @staticmethod
    def backward(ctx, ggx):
        return _Blur.apply(ggx)


class _Subsample2(torch.autograd.Function):
    """x[:, :, ::2, ::2] (dense); adjoint = zero insertion; the pair is closed under differentiation."""

    @staticmethod
    def forward(ctx, x):
        ctx.hw = tuple(x.shape[2:])
        return hb.subsample2_fwd(_cl(x))

    @staticmethod
    def backward(ctx, gy):
        return _ZeroInsert2.apply(gy, ctx.hw)


class _ZeroInsert2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gy, hw):
        return hb.subsample2_bwd(_cl(gy), hw)

    @staticmethod
    def backward(ctx, ggx):
        return _Subsample2.apply(ggx), None


class _RowSumSq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x2d):
        ctx.save_for_backward(x2d)
        return hb.rowwise_sumsq(x2d)

    @staticmethod
    def backward(ctx, g):
        (x2d,) = ctx.saved_tensors
        return 2.0 * x2d * g[:, None]


# ------------------------------------------------------------------------------------------
# K10: the scalar losses of the step as one forward + one backward launch each (csrc/losses.hip).  First-order nodes:
# none of these losses is differentiated twice (the gradient penalty and the path-length term differentiate D / G
# twice, not the reduction on top — the backward of `pl_lengths` only FEEDS the double-backward graph of G).
# STYLEX_FUSED_LOSSES=0 keeps the torch compositions (A/B, bisecting).
# ------------------------------------------------------------------------------------------

_FUSED_LOSSES = os.environ.get("STYLEX_FUSED_LOSSES", "1") != "0"


def _loss_fusable(*ts):
    return (_FUSED_LOSSES and _IMPL is HipOps and
            all(t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and t.numel() > 0 for t in ts))


class _Hinge(torch.autograd.Function):
    """mode 0: mean(relu(1 + real) + relu(1 - fake)) (reference hinge_loss :386-387); mode 1: fake.mean() (:382-383)."""

    @staticmethod
    def forward(ctx, real, fake, mode):
        real = hb._f32c(real) if real is not None else None
        fake = hb._f32c(fake)
        ctx.save_for_backward(real, fake)
        ctx.mode = mode
        return hb.hinge_fwd(real, fake, mode)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        real, fake = ctx.saved_tensors
        greal, gfake = hb.hinge_bwd(real, fake, hb._f32c(g), ctx.mode == 0 and ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                    ctx.mode)
        return greal, gfake, None


class _HingeRel(torch.autograd.Function):
    """rel_disc_loss (reference :1338-1342): the hinge of real - mean(fake) and fake - mean(real); both means carry gradient."""

    @staticmethod
    def forward(ctx, real, fake):
        real, fake = hb._f32c(real), hb._f32c(fake)
        ctx.save_for_backward(real, fake)
        return hb.hinge_rel_fwd(real, fake)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        real, fake = ctx.saved_tensors
        return hb.hinge_rel_bwd(real, fake, hb._f32c(g), ctx.needs_input_grad[0], ctx.needs_input_grad[1])


class _TopKMean(torch.autograd.Function):
    """top_k_training (reference :1401-1407): mean of the k smallest values; among equal values the lower index is taken."""

    @staticmethod
    def forward(ctx, v, k):
        v = hb._f32c(v)
        ctx.save_for_backward(v)
        ctx.k = k
        return hb.topk_mean_fwd(v, k)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return hb.topk_mean_bwd(v, hb._f32c(g), ctx.k), None


class _PLLengths(torch.autograd.Function):
    """sqrt(mean_l(sum_d g^2)) per sample (reference calc_pl_lengths :316)."""

    @staticmethod
    def forward(ctx, g):
        g = hb._f32c(g)
        lengths = hb.pl_lengths_fwd(g)
        ctx.save_for_backward(g, lengths)
        return lengths

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, glen):
        g, lengths = ctx.saved_tensors
        return hb.pl_lengths_bwd(g, lengths, hb._f32c(glen))


class _KLLogits(torch.autograd.Function):
    """KLDivLoss(batchmean, log_target=True)(log_softmax(fake), log_softmax(real)) (reference :421-438)."""

    @staticmethod
    def forward(ctx, real, fake):
        real, fake = hb._f32c(real), hb._f32c(fake)
        ctx.save_for_backward(real, fake)
        return hb.kl_logits_fwd(real, fake)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        real, fake = ctx.saved_tensors
        return hb.kl_logits_bwd(real, fake, hb._f32c(g), ctx.needs_input_grad[0], ctx.needs_input_grad[1])


class _L1Mean(torch.autograd.Function):
    """nn.L1Loss() (reference :404-405): mean |a - b|."""

    @staticmethod
    def forward(ctx, a, b, walk):
        ctx.save_for_backward(a, b)
        ctx.walk = walk
        return hb.l1_mean_fwd(a, b, walk)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga, gb = hb.l1_mean_bwd(a, b, hb._f32c(g), ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.walk)
        return ga, gb, None


def hinge_loss(real, fake, relativistic=False):
    """relativistic (rel_disc_loss, reference :1338-1342): each side is taken relative to the mean of the other."""
    if relativistic:
        if _loss_fusable(real, fake) and real.shape == fake.shape and real.numel() < (1 << 24):
            return _HingeRel.apply(real, fake)
        real, fake = real - fake.mean(), fake - real.mean()
    elif _loss_fusable(real, fake) and real.shape == fake.shape:
        return _Hinge.apply(real, fake, 0)
    return (F.relu(1 + real) + F.relu(1 - fake)).mean()


def gen_hinge_loss(fake, k=None):
    """k (top_k_training, reference :1401-1407): the mean of the k smallest logits instead of all of them.  Which of
    several EQUAL logits count is left open by torch.topk; the fused kernel takes the lower index (same loss value)."""
    if k is not None and k != fake.numel():
        if _loss_fusable(fake) and fake.dim() == 1 and fake.numel() <= hb.topk_mean_max_n():
            return _TopKMean.apply(fake, int(k))
        return fake.topk(k=int(k), largest=False)[0].mean()
    if _loss_fusable(fake):
        return _Hinge.apply(None, fake, 1)
    return fake.mean()


def pl_lengths(pl_grads):
    if _loss_fusable(pl_grads) and pl_grads.dim() == 3:
        return _PLLengths.apply(pl_grads)
    return (pl_grads ** 2).sum(dim=2).mean(dim=1).sqrt()


def kl_logits(real_logits, fake_logits):
    if _loss_fusable(real_logits, fake_logits) and real_logits.dim() == 2 and real_logits.shape == fake_logits.shape:
        return _KLLogits.apply(real_logits, fake_logits)
    return F.kl_div(F.log_softmax(fake_logits, dim=1), F.log_softmax(real_logits, dim=1), reduction="batchmean", log_target=True)


def l1_mean(a, b):
    if _loss_fusable(a, b):
        walk = hb.l1_walk(a, b)
        if walk is not None:
            return _L1Mean.apply(a, b, walk)
    return F.l1_loss(a, b)


# ------------------------------------------------------------------------------------------
# fused fast path: ONE forward kernel per conv (scales, bias, noise, residual merge, LeakyReLU in the
# epilogue) and fused backward bookkeeping.  Backward is NOT differentiable again, so it is used
# only when no double backward can be requested: under no_grad, or when the Trainer has declared
# the phase free of gradient-penalty / path-length terms (set_fast).
# ------------------------------------------------------------------------------------------

_FAST = False


def set_fast(flag):
    """Trainer hook: True when the coming forward/backward needs first-order gradients only."""
    global _FAST
    prev = _FAST
    _FAST = bool(flag)
    return prev


def fast_enabled():
    return _FAST or not torch.is_grad_enabled()


def _reducible(c):
    return c % 4 == 0 and c <= 1024


def _grad_prologue(gy, y, lrelu, scale, want_gb):
    """(gz, gb): gz = scale * lrelu'(y) * gy (gy itself when there is nothing to apply) and, with want_gb, its per-channel
    sum in fp32 — one reduce launch where the channel count allows it, else ATen."""
    want_dx = lrelu or scale != 1.0
    if not (want_dx or want_gb):
        return gy, None
    if _reducible(gy.shape[1]):
        gz, gb = hb.act_bwd_reduce(gy, y, lrelu, scale, want_dx=want_dx, want_sum=want_gb)
        return (gz if want_dx else gy), gb
    gz = hb.bias_act_bwd(gy, y) if lrelu else gy
    if scale != 1.0:
        gz = gz * scale
    return gz, (gz.sum(dim=(0, 2, 3), dtype=torch.float32) if want_gb else None)


# The fused plain conv: conv + bias + residual merge + activation in one forward launch.  How it runs is decided ONCE, by
# _conv_plan in the calling op (HipOps.conv2d / .blur_down), and reaches the Functions as the plan's launch record.
_ConvEpi = collections.namedtuple("_ConvEpi", "launch lrelu scale has_bias has_res untimed")
_ConvSaved = collections.namedtuple("_ConvSaved", "x w y")


def _conv_forward(launch, x, w, bias, residual, lrelu, res_scale):
    """(y, epi, saved): y = lrelu?( (conv(x, w) + bias + residual) * res_scale ).  With launch.s2d, x is the space-to-depth
    image of a stride-2 conv's input: a 3x3/s1 conv over 4C channels on the LDS-halo kernels, structurally-zero taps skipped
    (exactly the original 9*C work)."""
    x = _cl(x)
    if residual is not None:
        residual = _cl(residual)
    y = _fwd(x, w, launch, bias=bias, lrelu=lrelu, residual=residual, res_scale=res_scale)
    # untimed: built inside hb.timing_pause() (a frozen network's layer): so is its fused backward
    epi = _ConvEpi(launch, lrelu, float(res_scale) if residual is not None else 1.0, bias is not None,
                   residual is not None, hb.timing_paused())
    return y, epi, _ConvSaved(x, w, y if lrelu else None)


def _conv_backward(epi, saved, gy, need):
    """(gx, gw, gb, gres), first order only; need = the node's needs_input_grad."""
    x, w, y = saved
    # (no bias gradient in the generator phase, D frozen: no reduction launch)
    gz, gb = _grad_prologue(_cl(gy), y, epi.lrelu, epi.scale, epi.has_bias and need[2])
    with (hb.timing_pause() if epi.untimed else _nullcontext()):
        gx = _bwd_data(gz, w, tuple(x.shape), epi.launch) if need[0] else None
        gw = _bwd_weight(x, gz, tuple(w.shape), epi.launch) if need[1] else None
    return gx, gw, gb, (gz if epi.has_res and need[3] else None)


class _ConvBiasActFast(torch.autograd.Function):
    """_conv_forward / _conv_backward as a once-differentiable node; the class only saves and restores their state."""

    @staticmethod
    def forward(ctx, x, w, bias, residual, launch, lrelu, res_scale):
        y, ctx.epi, saved = _conv_forward(launch, x, w, bias, residual, lrelu, res_scale)
        ctx.save_for_backward(*saved)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        return _conv_backward(ctx.epi, _ConvSaved(*ctx.saved_tensors), gy, ctx.needs_input_grad) + (None, None, None)


class _ConvBiasActDD(_ConvBiasActFast):
    """The same forward (inherited) with a backward composed of differentiable Functions (activation-derivative kernel, the
    conv triad), so it can be differentiated again: this is what the real branch of a gradient-penalty step runs."""

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        launch, lrelu, scale, has_bias, has_res, _ = ctx.epi
        gz = _BiasActBwd.apply(gy, y.detach()) if lrelu else gy
        if scale != 1.0:
            gz = gz * scale
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _Dgrad.apply(gz, w, tuple(x.shape), launch)
        if _want_param_grad(ctx, 1):
            gw = _Wgrad.apply(x, gz, tuple(w.shape), launch)
        if has_bias and _want_param_grad(ctx, 2):
            # a backward that is not itself recorded (the ordinary loss.backward() of a penalty step) takes the read-only
            # reduction kernel: 2.4x faster than the ATen reduce on the 256^2 tensors (.118 vs .285 ms at B=64)
            gb = _channel_sum(gz) if (not torch.is_grad_enabled() and gz.is_cuda and hb.is_cl(gz)) else gz.sum(dim=(0, 2, 3), dtype=torch.float32)
        return gx, gw, gb, (gz if has_res and ctx.needs_input_grad[3] else None), None, None, None


_NAT_NOISE = {}
import atexit as _atexit  # noqa: E402

_atexit.register(_NAT_NOISE.clear)  # device tensors are released before the interpreter / HIP runtime shut down


def _natural_noise(inoise):
    """The generator's noise plane in natural order, nat[b][h][w] = inoise[b][w][h][0] (the reference permutes the
    projected noise (0,3,2,1), :696-698, i.e. reads the plane transposed).  Transposed ONCE per generator forward (all
    14 noise layers of a forward share the plane, each cropping its top-left h x w corner) so that the conv epilogues
    read 4 consecutive pixels with one 16-byte load instead of 16 strided 4-byte loads: measured on the modulated convs
    with noise, 64->32 @256^2 .60 -> .31 ms and 32->32 @256^2 .49 -> .19 ms per launch (tools/bench_modconv.py)."""
    # one entry, keyed by the tensor OBJECT (held alive by the entry, so its address cannot be recycled by another
    # noise tensor) and its version counter (static graph input buffers are refilled in place)
    hit = _NAT_NOISE.get("k")
    if (hit is not None and hit[0] is inoise and hit[1] == inoise._version
            and not (inoise.is_cuda and torch.cuda.is_current_stream_capturing())):
        return hit[2]
    nat = inoise[:, :, :, 0].transpose(1, 2).contiguous().float()
    _NAT_NOISE["k"] = (inoise, inoise._version, nat)
    return nat


# The fused modulated conv (Conv2DMod + noise + LeakyReLU), the generator's hot node.  As for the fused DiscriminatorBlock
# below, how it runs is decided ONCE, by _modconv_plan in the forward; the backward reads the plan and the named saved
# state, never the environment or the library, and a pass outside autograd can drive the two stage functions directly.
_ModConvPlan = collections.namedtuple(
    "_ModConvPlan", "prec pad lrelu pre nat fwd_noise prep prep_ok bwd_noise fold dgrad scale_reduce")
_ModConvSaved = collections.namedtuple("_ModConvSaved", "x s1 d w noise nw nb y noise_nat")


def _modconv_plan(x_shape, w_shape, x_cuda, has_d, has_style, has_noise, has_nat, nat_side, pad, lrelu, prec,
                  has_symbol=hb.has_symbol):
    """Every decision of one fused modulated conv, from shapes, what is present, the precision mode and the two environment
    switches (read per call: tests toggle them).  has_nat: the noise plane is at hand in natural order (_natural_noise) —
    or, asked by the call site before it transposes, can be; nat_side: its side length.  The library probe is an argument
    so that the rules can be evaluated without the kernel library."""
    def on(name):
        return os.environ.get(name, "1") != "0"

    cin, cout, bf16 = x_shape[1], w_shape[0], prec == hb.BF16_ACT
    # <= 8x8 px layers: the modulation is applied to the (tiny) input tensor up front, so that the launch can take the
    # LDS-DMA implicit-GEMM kernel (conv_gather.hip: a DMA cannot scale in flight); same rounding as the in-kernel
    # staging (product rounded to bf16 once)
    pre = bf16 and has_style and x_shape[2] * x_shape[3] <= 64 and cin % 64 == 0
    # the natural-order plane serves device inputs (STYLEX_NOISE_NAT=0: every read is the transposed one)
    nat = bool(has_nat and x_cuda and on("STYLEX_NOISE_NAT"))
    # The two reads are decided separately and may differ: the forward epilogue loads 4 pixels of a row at once, so it
    # takes the natural plane only at a side that is a multiple of 4; the prep pass reads rows of it at any side, if the
    # library has the entry point (one from before it — STYLEX_HIP_LIB=<older build>, A/B runs — keeps the transposed
    # plane).  Side 9: transposed forward, natural backward.
    fwd_noise = "none" if not has_noise else "natural" if nat and nat_side % 4 == 0 else "transposed"
    bwd_noise = "natural" if nat and has_symbol("stylex_modconv_bwd_prep_nat") else "transposed"
    # modconv_bwd_prep (LeakyReLU mask, noise / bias sums, the demodulation gradient's sum) runs over the saved y; where
    # the channel count rules it out, the BACKWARD raises: a forward under no_grad works at any count
    prep, prep_ok = bool(lrelu or has_d or has_noise), _reducible(cout)
    # the gradient leaves the prep pass pre-multiplied by d: a scale-free operand for the data gradient, eligible for the
    # LDS-DMA kernels (halo / small-spatial gather), and no dy scale in the weight gradient
    fold = prep and prep_ok and has_d and prec != hb.F32 and on("STYLEX_FOLD_D")
    # else, small layer: d applied to the (tiny) gradient tensor up front; else the data gradient's in_scale (d or None)
    dgrad = "folded" if fold else "prescaled" if pre and has_d else "in_scale"
    return _ModConvPlan(prec, pad, bool(lrelu), pre, nat, fwd_noise, prep, prep_ok, bwd_noise, fold, dgrad,
                        _reducible(cin))


def _modconv_forward(plan, x, s1, d, w, noise, nw, nb, noise_nat):
    """(y, saved): y = lrelu?( d[b,o] * conv(x * s1[b,i], w) + noise[b,w,h]*nw[o] + nb[o] )"""
    x = _cl(x)
    if plan.pre:
        x_in, s_in = (x.float() * s1[:, :, None, None]).to(x.dtype).contiguous(memory_format=torch.channels_last), None
    else:
        x_in, s_in = x, s1
    read = dict(noise=noise_nat, noise_natural=True) if plan.fwd_noise == "natural" else dict(noise=noise)
    y = hb.conv2d_fwd(x_in, w, 1, plan.pad, plan.prec, in_scale=s_in, out_scale=d, noise_w=nw, noise_b=nb,
                      lrelu=plan.lrelu, **read)
    # x: the unmodulated input, also with plan.pre (the backward's reductions are over it)
    return y, _ModConvSaved(x, s1, d, w, noise, nw, nb, y if plan.prep else None, noise_nat if plan.nat else None)


def _modconv_backward(plan, saved, gy, need):
    """(gx, gs1, gd, gw, gnw, gnb); need = (x, s1, w): which of those three gradients are wanted (gd, gnw and gnb come
    out of the prep pass either way)."""
    x, s1, d, w, noise, nw, nb, y, noise_nat = saved
    want_x, want_s1, want_w = need
    prec = plan.prec
    gz = _cl(gy)
    gd = gnw = gnb = None
    if plan.prep:
        if not plan.prep_ok:
            raise hb.StylexHipError("fused modulated conv needs C_out % 4 == 0")
        natural = plan.bwd_noise == "natural"
        gz, sums = hb.modconv_bwd_prep(gz, y, noise_nat if natural else noise, nw, nb, plan.lrelu,
                                       gz_scale=d if plan.fold else None, noise_natural=natural)
        if d is not None:
            gd = sums[:, 0] / d
        if noise is not None:
            gnw, gnb = sums[:, 1:3].sum(0)  # one reduction launch for both (the same per-element sums)
    gx = gs1 = gw = None
    if want_x or want_s1:
        if plan.dgrad == "prescaled":
            gzd = (gz.float() * d[:, :, None, None]).to(gz.dtype).contiguous(memory_format=torch.channels_last)
            t = hb.conv2d_bwd_data(gzd, w, tuple(x.shape), 1, plan.pad, prec)
        else:
            t = hb.conv2d_bwd_data(gz, w, tuple(x.shape), 1, plan.pad, prec, in_scale=None if plan.fold else d)
        if plan.scale_reduce:
            gx, gs1 = hb.scale_reduce(x, t, s1, want_gx=want_x)
        else:
            gs1 = (x.float() * t.float()).sum(dim=(2, 3))
            gx = (t.float() * s1[:, :, None, None]).to(t.dtype)
    if want_w:
        gw = hb.conv2d_bwd_weight(x, gz, tuple(w.shape), 1, plan.pad, prec, x_scale=s1, dy_scale=None if plan.fold else d)
    return gx, gs1, gd, gw, gnw, gnb


class _ModConvFast(torch.autograd.Function):
    """y = lrelu?( d[b,o] * conv(x * s1[b,i], w) + noise[b,w,h]*nw[o] + nb[o] )   (Conv2DMod + noise + act).  The work
    is in _modconv_forward / _modconv_backward; this class only builds the plan and saves and restores their state."""

    @staticmethod
    def forward(ctx, x, s1, d, w, noise, nw, nb, pad, lrelu, noise_nat=None):
        ctx.plan = _modconv_plan(tuple(x.shape), tuple(w.shape), x.is_cuda, d is not None, s1 is not None,
                                 noise is not None, noise_nat is not None,
                                 noise_nat.shape[1] if noise_nat is not None else 0, pad, lrelu, _PRECISION)
        y, saved = _modconv_forward(ctx.plan, x, s1, d, w, noise, nw, nb, noise_nat)
        ctx.save_for_backward(*saved)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        need = ctx.needs_input_grad
        gx, gs1, gd, gw, gnw, gnb = _modconv_backward(ctx.plan, _ModConvSaved(*ctx.saved_tensors), gy,
                                                      (need[0], need[1], need[3]))
        return gx, gs1, gd, gw, None, gnw, gnb, None, None, None


def _modconv_fused(x, s1, d, weight, inoise=None, nw=None, nb=None):
    """One Conv2DMod — with `inoise` plus its noise and LeakyReLU — on the fused node, or None when the composable path
    must run: a double backward may be requested, or the output channels are no multiple of 4.  The 3 outputs of a to-RGB
    conv run as 4 (a zero filter, d = 1) and are sliced back; a noise layer with 3 outputs takes the composition."""
    n_out = weight.shape[0]
    pad_out = n_out == 3 and inoise is None
    if not fast_enabled() or (n_out + pad_out) % 4 != 0:
        return None
    if pad_out:
        weight = torch.cat([weight, weight.new_zeros(1, *weight.shape[1:])], dim=0)
        if d is not None:
            d = torch.cat([d, d.new_ones(d.shape[0], 1)], dim=1)
    pad = (weight.shape[2] - 1) // 2  # _get_same_padding for stride 1, dilation 1 (:644-645)
    if inoise is None:
        y = _ModConvFast.apply(x, s1, d, weight, None, None, None, pad, False)
        return y[:, :3] if pad_out else y
    # asked before the transpose (once per generator forward): would this conv read the natural-order plane?
    want_nat = _modconv_plan(tuple(x.shape), tuple(weight.shape), x.is_cuda, has_d=d is not None, has_style=True,
                             has_noise=True, has_nat=True, nat_side=inoise.shape[1], pad=pad, lrelu=True,
                             prec=_PRECISION).nat
    return _ModConvFast.apply(x, s1, d, weight, inoise[:, :, :, 0], nw, nb, pad, True,
                              _natural_noise(inoise) if want_nat else None)


def _torgb_route(x, weight, demod):
    """Does this modulated conv over the (activation-dtype) x run as the streaming to-RGB kernel (_ToRGBFast)?  The 1x1,
    3-output, non-demodulated conv of RGBBlock, first order only, where hb.torgb_ok takes the input."""
    return (fast_enabled() and weight.shape[0] == 3 and tuple(weight.shape[2:]) == (1, 1) and not demod
            and hb.torgb_ok(x))


class _ToRGBFast(torch.autograd.Function):
    """RGBBlock's Conv2DMod(C, 3, 1, demod=False) (reference :611, :621) as one streaming kernel each way.
    Returns the 4-channel storage (channel 3 zero); the caller slices [:, :3]."""

    @staticmethod
    def forward(ctx, x, s1, w):
        x = _cl(x)
        ctx.save_for_backward(x, s1, w)
        return hb.torgb_fwd(x, s1, w)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, s1, w = ctx.saved_tensors
        gx, t = hb.torgb_bwd(x, _cl(gy), s1, w, want_gx=ctx.needs_input_grad[0])
        gs1 = gw = None
        if ctx.needs_input_grad[1]:
            gs1 = (t * w.reshape(1, 3, -1).float()).sum(dim=1)
        if ctx.needs_input_grad[2]:
            gw = (t * s1.float()[:, None, :]).sum(dim=0).reshape(w.shape).to(w.dtype)
        return gx, gs1, gw


class _RGBTailFast(torch.autograd.Function):
    """blur(upsample2x(rgb + prev)) of RGBBlock.forward (reference :622-626) as one kernel each way (4-channel NHWC
    storage of the RGB chain; once-differentiable: the composable chain serves steps that differentiate twice)."""

    @staticmethod
    def forward(ctx, rgb, prev):
        return hb.rgb_up_blur_add_fwd(_cl(rgb), _cl(prev) if prev is not None else None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        g = hb.rgb_up_blur_add_bwd(_cl(gy))
        return g, (g if ctx.needs_input_grad[1] else None)


class _BlurS2D(torch.autograd.Function):
    """blur3x3 whose output is stored space-to-depth ([B,4C,H/2,W/2]) for the stride-2 conv that follows."""

    @staticmethod
    def forward(ctx, x):
        return hb.blur3x3_s2d_fwd(_cl(x))

    @staticmethod
    def backward(ctx, gy2):
        return _BlurS2DBwd.apply(gy2)


class _BlurS2DBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gy2):
        return hb.blur3x3_s2d_bwd(_cl(gy2))

    @staticmethod
    def backward(ctx, ggx):
        return _BlurS2D.apply(ggx)


def _s2d_eligible(c, h, w, prec):
    """Does a 3x3 / stride-2 conv over c channels at h x w run as a 3x3 / stride-1 conv over the space-to-depth image of its
    (blurred) input (LDS-DMA kernels)?  The rule of the fused DiscriminatorBlock's tail and of blur_down."""
    return prec != hb.F32 and c % 64 == 0 and h % 2 == 0 and w % 2 == 0 and w // 2 >= 16 and h // 2 >= 16


def _rgb_extra(dtype):
    """Zero channels that pad an RGB tensor of this dtype to one 16-byte slot: 8 bf16 or 4 fp32 channels."""
    return 5 if dtype == torch.bfloat16 else 1


# One plain conv call (HipOps.conv2d, .blur_down): zero input channels added, 3 outputs run as 4, even-pixel gather first,
# route "fused" (_ConvBiasActFast) / "composable" (_ConvBiasActDD) / "triad" (_Conv + torch epilogue), the conv's launch.
_ConvPlan = collections.namedtuple("_ConvPlan", "extra_in pad_out subsample route launch")


def _conv_plan(x_shape, x_dtype, w_shape, stride, pad, prec, fast, blurred=False):
    """Every decision of one plain conv call, from shapes, the input's dtype (it has been through _act), precision mode,
    fast_enabled() and the two GEMM switches (read per call: tests toggle them; their only reader on this path).  blurred:
    the call is blur_down, whose blur can write its output space-to-depth.  In this order, each step seeing the earlier:"""
    cin, (h, w), n, kernel = x_shape[1], x_shape[2:], w_shape[0], tuple(w_shape[2:])
    # 1. blur_down over the space-to-depth blur output: the shared rule and, on top of it, this form's own two conditions
    n_mult_of_4, is_3x3 = n % 4 == 0, kernel == (3, 3)
    s2d = cin if blurred and (stride, pad) == (2, 1) and n_mult_of_4 and is_3x3 and _s2d_eligible(cin, h, w, prec) else 0
    # 2. RGB: the vector (16-byte) load paths want whole slots: C_in 3 padded to one, N 3 -> 4.  x_dtype is the mode's
    #    activation dtype here, so this agrees with _dblock_plan, which asks by the mode
    extra_in, pad_out = (_rgb_extra(x_dtype) if cin == 3 else 0), n == 3
    # 3. 1x1 / stride 2 (conv_res): contiguous 1x1 / stride-1 GEMMs over the gathered even pixels
    subsample = stride == 2 and pad == 0 and kernel == (1, 1) and (cin + extra_in) % 4 == 0
    stride = 1 if s2d or subsample else stride  # both forms run a stride-1 conv
    # 4. the fused Functions cannot slice their output: a padded one takes the triad, in the fast mode too
    route = "triad" if pad_out else "fused" if fast else "composable"
    # 5. the static half of _gemm_1x1; the fused route keeps the project's own kernel for 1x1 convs
    gemm = (route != "fused" and not s2d and stride == 1 and pad == 0 and kernel == (1, 1) and prec == hb.BF16_ACT
            and os.environ.get("STYLEX_RES_GEMM", "1") != "0" and os.environ.get("STYLEX_RES_GEMM_DD", "1") != "0")
    return _ConvPlan(extra_in, pad_out, subsample, route, _ConvLaunch(stride, pad, s2d, gemm))


# The fused DiscriminatorBlock.  How a block runs is decided ONCE, by _dblock_plan in the forward; the backward and the
# gradient-penalty tangent pass (gp_tangent.py) read the plan and the named saved state, never the environment.  The fused
# modulated conv (_modconv_plan, _ModConvSaved, _modconv_forward / _modconv_backward) and the plain conv path (_conv_plan,
# the _ConvLaunch record its nodes pass on, _ConvSaved, _conv_forward / _conv_backward) keep the same promise.
_DBlockPlan = collections.namedtuple(
    "_DBlockPlan", "prec downsample cin pad extra res_gemm s2d fold_res mask1 mask2 alg wgrad_bias c")
_DBlockSaved = collections.namedtuple("_DBlockSaved", "x xs y1 y2 xb m1 m2 w_res w1 w2 w3")


def _dblock_plan(x_shape, x_dtype, x_cuda, w_shapes, downsample, prec, s2d_res_supported=hb.s2d_res_supported,
                 blur_mask_ok=hb.blur_mask_ok):
    """Every decision of one fused DiscriminatorBlock, from shapes, precision mode and the environment switches (read per
    call: tests toggle them).  w_shapes: of (w_res, w1, w2, w3), w3's None without a stride-2 tail.  The two probes are
    arguments so that the rules can be evaluated without the kernel library."""
    def on(name):
        return os.environ.get(name, "1") != "0"

    b, cin, h, w = x_shape
    n_res, n2 = w_shapes[0][0], w_shapes[2][0]
    downsample, bf16 = bool(downsample), prec == hb.BF16_ACT
    # RGB input: zero-padded to one 16-byte channel slot (8 bf16 / 4 fp32 channels), gradients are sliced back.  The bf16
    # mode casts, lays out and pads in ONE pass (pad_rgb8); STYLEX_PAD_RGB=0 and the other modes concatenate (_pad_rgb)
    pad, extra = None, 0
    if cin == 3:
        rgb8 = bf16 and x_cuda and x_dtype in (torch.float32, torch.bfloat16) and on("STYLEX_PAD_RGB")
        pad, extra = ("pad_rgb8" if rgb8 else "_pad_rgb"), _rgb_extra(hb.act_dtype(prec))
    # the 1x1 conv of the residual path is a plain GEMM: hipBLASLt in the bf16 mode (2-3x the generic kernel)
    res_gemm = bf16 and on("STYLEX_RES_GEMM")
    # the stride-2 conv as a 3x3/s1 conv over the space-to-depth image of the blur output (LDS-DMA kernels)
    s2d = downsample and _s2d_eligible(n2, h, w, prec)
    # Such blocks take the residual conv as a second K segment of that launch (hb.conv2d_s2d_res_fwd): no GEMM, no bf16
    # `res` tensor written and read back (round 4; STYLEX_RES_FOLD=0 = the separate GEMM).  Only the s2d tail consumes it.
    fold_res = (s2d and res_gemm and (cin + extra) % 8 == 0 and on("STYLEX_RES_FOLD")
                and bool(s2d_res_supported((b, 4 * n2, h // 2, w // 2), n_res, n2, cin + extra)))
    # Activation bit masks: the backward needs y2 ONLY for its sign (the LeakyReLU derivative fused into the blur adjoint)
    # and y1 for its sign plus as the weight-gradient operand; where the forward kernel can write the sign bits alongside
    # (1/16 of the bytes) the gated backward passes read those instead of the tensors, and y2 is not kept for the backward
    # at all.  STYLEX_GATE_MASK=0: gate on the tensors.
    # (measured per launch at B=64, tools/bench_masks.py: gated data gradient 64->64 @256^2 .534 -> .445 ms, gated blur
    # adjoint .323 -> .273, 128 @128^2 .356 -> .327 / .159 -> .141; writing the mask costs the forward 0 - .012 ms;
    # at 64^2 and below the saving no longer covers that, so the masks are used from 128^2 up)
    mask1 = bf16 and on("STYLEX_GATE_MASK") and h * w >= int(os.environ.get("STYLEX_GATE_MASK_MIN_PIXELS", 128 * 128))
    mask2 = mask1 and s2d and bool(blur_mask_ok((b, n2, h, w), hb.act_dtype(prec)))
    # (. + res) / sqrt(2).  In the bf16 modes the constant c never touches the activation gradient: it is folded into
    # the packed data-gradient operands (c*w3, c*w_res) and into the (small) weight / bias gradients, which removes one
    # full pass over the block's output gradient; the fp32 parity mode scales explicitly.
    alg = downsample and prec != hb.F32
    return _DBlockPlan(prec, downsample, cin, pad, extra, res_gemm, s2d, fold_res, mask1, mask2, alg,
                       on("STYLEX_WGRAD_BIAS"), 1 / math.sqrt(2))


def _dblock_input(plan, x):
    """The block's input, or a tangent of it, as the kernels read it: activation dtype, channels_last, RGB padded."""
    if plan.pad == "pad_rgb8":
        return hb.pad_rgb8(x.detach())
    x = _cl(_act(x))
    if plan.pad:
        x = _cl(torch.cat([x, x.new_zeros(x.shape[0], plan.extra, x.shape[2], x.shape[3])], dim=1))
    return x


def _dblock_weights(plan, w1, w_res):
    """(w1p, wrp, owner1, owner_res): the weights that read the (padded) input, and the Parameters under whose
    modification stamp the operand copies of a padded weight are cached (None: the weight is the Parameter itself).
    The padded weights are cached too (they used to be rebuilt — zeros, cat, pack, cast — in every pass of block 0)."""
    if not plan.pad:
        return w1, w_res, None, None
    return hb.pad_in_channels(w1, plan.extra), hb.pad_in_channels(w_res, plan.extra), w1, w_res


def _owned_pack(w, owner, fwd, prec):
    """conv keyword arguments that hand the launch a padded weight's operand pack, cached under its Parameter."""
    if not isinstance(owner, torch.nn.Parameter):
        return {}
    return dict(packed=hb.pack_weight(w, fwd, not fwd, prec, owner=owner)[0 if fwd else 1], w_shape=tuple(w.shape))


def _dblock_res_conv(plan, xs, wrp, owner, bias=None):
    """The 1x1 residual conv over the (gathered) input: GEMM or generic kernel."""
    if plan.res_gemm:
        return hb.conv1x1_gemm_fwd(xs, wrp, bias, owner=owner)
    return hb.conv2d_fwd(xs, wrp, 1, 0, plan.prec, bias=bias)


def _dblock_tail(plan, y2, res, w3, b3=None, fold=None):
    """(out, xb): blur, stride-2 conv and the merge with the residual path, (conv3x3_s2(blur(y2)) + b3 + res) / sqrt(2);
    without a stride-2 tail (y2 + res) / sqrt(2).  fold = (xs, wrp, owner, b_res) when plan.fold_res: res is computed
    inside the launch."""
    c, prec = plan.c, plan.prec
    if not plan.downsample:
        return (y2 + res) * c, None
    if not plan.s2d:
        xb = hb.blur3x3_fwd(y2)
        return hb.conv2d_fwd(xb, w3, 2, 1, prec, bias=b3, residual=res, res_scale=c), xb
    xb = hb.blur3x3_s2d_fwd(y2)
    if fold is None:
        return hb.conv2d_fwd_s2d(xb, w3, prec, bias=b3, residual=res, res_scale=c), xb
    xs, wrp, owner, b_res = fold
    bsum = hb.cached_vector("sum32", lambda a, b: a.float() + b.float(), b3, b_res)
    return hb.conv2d_s2d_res_fwd(xb, hb.pack_weight_s2d(w3)[0], xs, hb._bf16_matrix(wrp, owner=owner), bsum, w3.shape[0],
                                 y2.shape[1], c), xb


def _dblock_forward(x, params, downsample):
    """(out, plan, saved) of one block; params = (w_res, b_res, w1, b1, w2, b2, w3, b3), w3 / b3 None without a tail."""
    w_res, b_res, w1, b1, w2, b2, w3, b3 = params
    plan = _dblock_plan(tuple(x.shape), x.dtype, x.is_cuda, [None if p is None else tuple(p.shape) for p in params[::2]],
                        downsample, _PRECISION)
    prec = plan.prec
    x = _dblock_input(plan, x)
    w1p, wrp, own1, own_res = _dblock_weights(plan, w1, w_res)
    xs = hb.subsample2_fwd(x) if plan.downsample else x
    res = None if plan.fold_res else _dblock_res_conv(plan, xs, wrp, own_res, b_res)
    y1 = hb.conv2d_fwd(x, w1p, 1, 1, prec, bias=b1, lrelu=True, want_mask=plan.mask1, **_owned_pack(w1p, own1, True, prec))
    y1, m1 = y1 if plan.mask1 else (y1, None)
    y2 = hb.conv2d_fwd(y1, w2, 1, 1, prec, bias=b2, lrelu=True, want_mask=plan.mask2)
    y2, m2 = y2 if plan.mask2 else (y2, None)
    out, xb = _dblock_tail(plan, y2, res, w3, b3, (xs, wrp, own_res, b_res) if plan.fold_res else None)
    return out, plan, _DBlockSaved(x, xs, y1, y2 if m2 is None else None, xb, m1, m2, w_res, w1, w2, w3)


def _dblock_backward(plan, saved, g_out, need):
    """((gx, gw_res, gb_res, gw1, gb1, gw2, gb2, gw3, gb3), (gz3, gz2, gz1)): every gradient that `need` (the block's
    needs_input_grad) asks for, and the three pre-activation gradients (gz3 without its 1/sqrt(2) when plan.alg)."""
    x, xs, y1, y2, xb, m1, m2, w_res, w1, w2, w3 = saved
    prec, c, cin, alg = plan.prec, plan.c, plan.cin, plan.alg
    want_x = need[0]
    want_b = need[2] or need[4] or need[6] or need[8]  # bias gradients (False for the frozen D of the G phase)
    want_w = need[1] or need[3] or need[5] or need[7]
    g_out = _cl(g_out)
    if alg:
        gz3, gsum3 = g_out, (_channel_sum(g_out, c) if want_b else None)  # the sum with its 1/sqrt(2)
    else:
        gz3, gsum3 = _grad_prologue(g_out, None, False, c, want_b)
    # factor owed by the gradients computed from the unscaled gz3: the out_scale of their reduce launches (round 5: it was
    # a multi-tensor multiply of 26 us per block, 0.47 ms per step)
    wsc = c if alg else 1.0
    w1p, wrp, own1, own_res = _dblock_weights(plan, w1, w_res)
    gw3 = None
    if plan.downsample:
        if plan.s2d:
            gxb = hb.conv2d_bwd_data_s2d(gz3, w3, tuple(xb.shape), prec, scale=c if alg else None)
        else:
            wb3 = hb.pack_weight(w3, False, True, prec, scale=c)[1] if alg else None
            gxb = hb.conv2d_bwd_data(gz3, w3, tuple(xb.shape), 2, 1, prec, packed=wb3, w_shape=tuple(w3.shape))
        if want_w:
            a3 = _gacc_get(w3)
            if plan.s2d:
                gw3 = hb.conv2d_bwd_weight_s2d(xb, gz3, tuple(w3.shape), prec, out_scale=wsc, accumulate_into=a3)
            else:
                gw3 = hb.conv2d_bwd_weight(xb, gz3, tuple(w3.shape), 2, 1, prec, out_scale=wsc, accumulate_into=a3)
            if a3 is None and need[7]:
                _gacc_put(w3, gw3)
        # blur adjoint + LeakyReLU derivative of y2, one pass
        gz2 = hb.blur3x3_s2d_bwd(gxb, gate=y2, gate_mask=m2) if plan.s2d else hb.blur3x3_bwd_gate(gxb, y2)
    else:
        gz2 = hb.bias_act_bwd(gz3, y2)
    # bias gradients = per-channel sums of gz2 / gz1: taken from the weight-gradient kernel (which stages those
    # tensors anyway) where it can, else a read-only reduction pass
    fuse_b = want_b and want_w and plan.wgrad_bias

    def layer_grads(w, w_shape, xin, gz, acc, need_w, need_b):
        """(gw, gb) of a 3x3 layer; acc: its gradients may be added into / named as the first use's (_gacc_*)."""
        gw = gb = None
        if want_w:
            aw = _gacc_get(w) if acc else None
            ab = _gacc_get(w, "b") if aw is not None else None
            gw = hb.conv2d_bwd_weight(xin, gz, w_shape, 1, 1, prec, want_bias_sum=fuse_b, accumulate_into=aw,
                                      accumulate_bias_into=ab)
            if fuse_b:
                gw, gb = gw
                if gb is True:  # added into the first use's bias gradient
                    return gw, None
            if aw is None and acc:  # (only what this node really hands to the engine may be named)
                if need_w:
                    _gacc_put(w, gw)
                if need_b:
                    _gacc_put(w, gb, "b")
        if want_b and gb is None:
            gb = _channel_sum(gz)
        return gw, gb

    gw2, gb2 = layer_grads(w2, tuple(w2.shape), y1, gz2, True, need[5], need[6])
    gz1 = hb.conv2d_bwd_data(gz2, w2, tuple(y1.shape), 1, 1, prec, gate=y1, gate_mask=m1)  # + LeakyReLU derivative of y1
    # (the padded-RGB block returns a slice of its gradients: nothing of it is accumulated into or named)
    gw1, gb1 = layer_grads(w1, tuple(w1p.shape), x, gz1, cin != 3, need[3], need[4])
    gx = gw_res = None
    if want_x:
        gx = hb.conv2d_bwd_data(gz1, w1p, tuple(x.shape), 1, 1, prec, **_owned_pack(w1p, own1, False, prec))
    if want_w:
        a_res = _gacc_get(w_res) if cin != 3 else None
        gw_res = hb.conv2d_bwd_weight(xs, gz3, tuple(wrp.shape), 1, 0, prec, out_scale=wsc, accumulate_into=a_res)
        if a_res is None and cin != 3 and need[1]:
            _gacc_put(w_res, gw_res)
        if cin == 3:
            gw1, gw_res = gw1[:, :3].contiguous(), gw_res[:, :3].contiguous()
    if want_x:
        if plan.res_gemm:  # [M, N] x [N, C] on hipBLASLt, the 1/sqrt(2) folded into the bf16 weight copy as below
            gxs = hb.conv1x1_gemm_bwd_data(gz3, wrp, scale=c if alg else None, owner=own_res)
        else:
            wbr = hb.pack_weight(wrp, False, True, prec, scale=c)[1] if alg else None
            gxs = hb.conv2d_bwd_data(gz3, wrp, tuple(xs.shape), 1, 0, prec, packed=wbr, w_shape=tuple(wrp.shape))
        if plan.downsample:
            hb.add_at_even_(gx, gxs)  # adjoint of the even-pixel gather, summed in place
        else:
            gx += gxs
        if cin == 3:
            gx = gx[:, :3]
    # the per-channel sum of the output gradient is the bias gradient of BOTH conv_res and the down conv
    return (gx, gw_res, gsum3, gw1, gb1, gw2, gb2, gw3, gsum3 if plan.downsample else None), (gz3, gz2, gz1)


class _DBlockFast(torch.autograd.Function):
    """A whole DiscriminatorBlock (reference :721-744) as ONE autograd node on the fused kernels:

        res = conv1x1_s2(x) + b_r ;  y1 = lrelu(conv3x3(x) + b1) ;  y2 = lrelu(conv3x3(y1) + b2)
        out = (conv3x3_s2(blur(y2)) + b3 + res) / sqrt(2)              (last block: (y2 + res) / sqrt(2))

    Why one node: the backward can then fuse ACROSS the layers — the LeakyReLU derivative of y1 rides the store of
    conv2's data gradient and that of y2 the store of the blur adjoint (STYLEX_EPI_GATE: no separate
    activation-derivative pass over the two largest tensors of the block), the bias gradient of the residual conv and
    of the down conv is the same reduction, and the gradient of the 1x1/stride-2 path is added into the 3x3 path's
    input gradient at the even pixels in place (no zero-inserted tensor, no full-resolution add).  First-order only
    (used when no double backward can be requested, see set_fast).  The work is in _dblock_forward / _dblock_backward,
    which gp_tangent drives directly; this class only saves and restores their state."""

    @staticmethod
    def forward(ctx, x, w_res, b_res, w1, b1, w2, b2, w3, b3, downsample):
        out, ctx.plan, saved = _dblock_forward(x, (w_res, b_res, w1, b1, w2, b2, w3, b3), downsample)
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        need = ctx.needs_input_grad
        grads, _ = _dblock_backward(ctx.plan, _DBlockSaved(*ctx.saved_tensors), g_out, need)
        return tuple(g if wanted else None for g, wanted in zip(grads, need)) + (None,)


# Gradient accumulation inside the weight-gradient launches (round 5).  A parameter used by several fast-path nodes of ONE
# backward pass (the encoder of a generator phase: E(x) and E(G(x)), reference stylex_train.py:1383-1395) used to hand the
# autograd engine one gradient tensor per use, which the engine sums with an add launch per parameter (117 per step).  Now
# the first node to run hands the engine its tensor and notes it through a WEAK reference (hb.RawGrad: a strong one would keep
# AccumulateGrad from stealing the tensor; the weak one also tells if the engine dropped it for an out-of-place sum); a later node of the same graph task adds into that tensor in its reduce launch
# (stylex_conv2d_bwd_weight_ex, accumulate) and returns None.  The engine keeps the first tensor alive, unmodified, until
# the parameter's AccumulateGrad node runs — after every use, by its dependency count.  Same two rounded fp32 operations as
# the engine's add: bit-identical gradients (tests/test_hip_parity.py::test_twice_used_block_accumulates_in_the_reduce_launch).
#
# Stream ordering (round 6, ADVICE medium).  The engine knows nothing of the later node's write, so the two orderings it would
# have provided are made explicit: (1) a node running on ANOTHER HIP stream than the tensor's producer (E(x) on the caller's
# stream, E(G(x)) on a Trainer._fork side stream) first makes its stream wait for the producer's; (2) the stream it added on
# is joined into the stream backward() was called from by an engine callback at the end of the pass (what the engine's own
# leaf-stream sync does for gradients it knows of), and GradSync's in-backward bucket launches wait for it as well
# (parallel.py::_launch reads _GACC_STREAMS).  tests/test_hip_parity.py::test_twice_used_block_on_two_streams.
_GACC = {}
_GACC_TASK = [-2]
_GACC_ON = os.environ.get("STYLEX_GRAD_ACC", "1") != "0"
_GACC_STREAMS = set()  # streams that added into a gradient produced on another stream, during the current backward pass
_GACC_WAITED = {}  # (waiting stream, producer stream) -> production number up to which the wait already holds
_GACC_SEQ = [0]


def _gacc_join():
    """End of the backward pass (engine callback, on the thread and stream that called backward())."""
    if _GACC_STREAMS:
        cur = torch.cuda.current_stream()
        for st in _GACC_STREAMS:
            if st != cur:
                cur.wait_stream(st)
        _GACC_STREAMS.clear()


def _gacc_get(w, tag=""):
    """The gradient tensor an earlier node of this backward pass produced for parameter w (tag: "b" = its layer's bias)."""
    if not _GACC_ON or not w.is_cuda:
        return None
    task = torch._C._current_graph_task_id()
    if task < 0:
        return None
    if task != _GACC_TASK[0]:
        _GACC.clear()
        _GACC_STREAMS.clear()
        _GACC_WAITED.clear()
        _GACC_TASK[0] = task
    slot = _GACC.get((w.data_ptr(), tag))
    if slot is not None and not slot.alive():  # the engine no longer holds that tensor (replaced by an out-of-place sum)
        del _GACC[(w.data_ptr(), tag)]
        return None
    if slot is not None:
        cur = torch.cuda.current_stream()
        if slot.stream != cur:
            # the tensor's producer ran on another stream: its kernel must have finished.  One wait covers every tensor that
            # stream had produced by then (slots are numbered in production order), so a whole encoder costs one event
            key = (cur, slot.stream)
            if _GACC_WAITED.get(key, 0) <= slot.seq:
                cur.wait_stream(slot.stream)
                _GACC_WAITED[key] = _GACC_SEQ[0]
            if not _GACC_STREAMS:
                torch.autograd.Variable._execution_engine.queue_callback(_gacc_join)
            _GACC_STREAMS.add(cur)
    return slot


def _gacc_put(w, g, tag=""):
    if _GACC_ON and g is not None and w.is_cuda and torch._C._current_graph_task_id() == _GACC_TASK[0] and g.is_contiguous():
        slot = _GACC[(w.data_ptr(), tag)] = hb.RawGrad(g)
        slot.seq = _GACC_SEQ[0]
        _GACC_SEQ[0] += 1


def _channel_sum(t, scale=1.0):
    """per-channel sum over (b, h, w) of scale * t in fp32 (bias gradient): read-only reduction kernel, fixed order."""
    if _reducible(t.shape[1]):
        return hb.act_bwd_reduce(t, None, False, scale, want_dx=False, want_sum=True)[1]
    r = t.sum(dim=(0, 2, 3), dtype=torch.float32)
    return r if scale == 1.0 else r * scale


# ------------------------------------------------------------------------------------------
# the HIP implementation object
# ------------------------------------------------------------------------------------------


def _pad_rgb(x, weight, extra_in, pad_out):
    """Zero-pad C_in by extra_in (input + weight) and, with pad_out, N 3 -> 4 (weight; the caller slices the output): exact."""
    if extra_in:
        x = torch.cat([x, x.new_zeros(x.shape[0], extra_in, x.shape[2], x.shape[3])], dim=1)
        weight = torch.cat([weight, weight.new_zeros(weight.shape[0], extra_in, weight.shape[2], weight.shape[3])], dim=1)
    if pad_out:
        weight = torch.cat([weight, weight.new_zeros(1, *weight.shape[1:])], dim=0)
    return x, weight


def _conv_apply(plan, x, weight, bias, residual, lrelu, res_scale):
    """Prepare the operands the plan names and apply the Function it names; x and residual in the activation dtype."""
    n_out = weight.shape[0]
    x, weight = _pad_rgb(x, weight, plan.extra_in, plan.pad_out)
    if plan.subsample:
        x = _Subsample2.apply(x)
    if plan.route != "triad":
        fn = _ConvBiasActFast if plan.route == "fused" else _ConvBiasActDD
        return fn.apply(x, weight, bias, residual, plan.launch, lrelu, res_scale)
    y = _Conv.apply(x, weight, plan.launch)[:, :n_out]
    if lrelu:
        assert residual is None
        return _BiasAct.apply(y, bias)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if residual is not None:
        y = (y + residual) * res_scale
    return y


class HipOps:
    """Functional surface used by the network modules (networks.py)."""

    name = "hip"

    @staticmethod
    def conv2d(x, weight, bias=None, stride=1, padding=0, lrelu=False, residual=None, res_scale=1.0):
        """nn.Conv2d (+ LeakyReLU(0.2)) — reference :724-736, :771, :881; with `residual` the block
        merge (conv + bias + residual) * res_scale of :743 is fused into the same kernel."""
        x = _act(x)
        plan = _conv_plan(tuple(x.shape), x.dtype, tuple(weight.shape), stride, padding, _PRECISION, fast_enabled())
        return _conv_apply(plan, x, weight, bias, _act(residual), lrelu, res_scale)

    @staticmethod
    def modulated_conv2d(x, style, weight, demod=True, eps=1e-8, coeffs=None):
        """Conv2DMod.forward (:647-667) without materialising per-sample weights:
        y = d[b,o] * conv(x * (style+1)[b,i], W),  d = rsqrt(((style+1)^2) @ sum_k W^2 + eps).
        `coeffs` = mod_coeffs(style, weight, demod, eps) when the caller computed them ahead (side stream)."""
        x = _act(x)
        s1, d_pre = coeffs if coeffs is not None else mod_coeffs(style, weight, demod, eps)
        if _torgb_route(x, weight, demod):
            return _ToRGBFast.apply(x, s1, weight)[:, :3]  # to-RGB: a 3-column GEMM is an HBM stream, not MFMA work
        y = _modconv_fused(x, s1, d_pre, weight)
        if y is not None:
            return y
        n_out = weight.shape[0]
        w_run = torch.cat([weight, weight.new_zeros(1, *weight.shape[1:])], dim=0) if n_out == 3 else weight
        plan = _conv_plan(tuple(x.shape), x.dtype, tuple(w_run.shape), 1, (weight.shape[2] - 1) // 2, _PRECISION, False)
        y = _Conv.apply(x * s1[:, :, None, None], w_run, plan.launch)
        if n_out == 3:
            y = y[:, :3]
        if demod:
            y = y * d_pre[:, :, None, None]
        return y

    @staticmethod
    def modconv_noise_act(x, style, weight, inoise, noise_w, noise_b, demod=True, eps=1e-8, coeffs=None):
        """lrelu(Conv2DMod(x, style) + noise) of GeneratorBlock (:696-714) as one fused kernel when no
        double backward can be requested, else the differentiable composition."""
        x = _act(x)
        coeffs = coeffs if coeffs is not None else mod_coeffs(style, weight, demod, eps)
        y = _modconv_fused(x, *coeffs, weight, inoise, noise_w, noise_b)
        if y is not None:
            return y
        return HipOps.noise_act(HipOps.modulated_conv2d(x, style, weight, demod, eps, coeffs=coeffs), inoise, noise_w,
                                noise_b)

    @staticmethod
    def noise_act(x, inoise, noise_w, noise_b):
        """lrelu(x + noise) with noise[b,c,h,w] = inoise[b,w,h,0]*noise_w[c] + noise_b[c]
        (the (0,3,2,1) permute of :696-698 is a spatial transpose)."""
        h, w = x.shape[2], x.shape[3]
        plane = inoise[:, :h, :w, 0].transpose(1, 2)  # [B, h(w-index), ...] -> value at (h,w) = inoise[b,w,h]
        n = plane[:, None, :, :] * noise_w.view(1, -1, 1, 1) + noise_b.view(1, -1, 1, 1)
        return _BiasAct.apply(_act(x + n), None)

    @staticmethod
    def upsample2x(x):
        return _Up.apply(_act(x))

    @staticmethod
    def blur3x3(x):
        return _Blur.apply(_act(x))

    @staticmethod
    def blur_down(x, weight, bias, residual, res_scale):
        """(conv3x3_s2(blur(x)) + bias + residual) * res_scale — the tail of DiscriminatorBlock (:733-743)."""
        x = _act(x)
        plan = _conv_plan(tuple(x.shape), x.dtype, tuple(weight.shape), 2, 1, _PRECISION, fast_enabled(), blurred=True)
        xb = _BlurS2D.apply(x) if plan.launch.s2d else _Blur.apply(x)
        return _conv_apply(plan, xb, weight, bias, _act(residual), False, res_scale)

    @staticmethod
    def rgb_block(x, prev_rgb, style, weight, upsample):
        """Whole RGBBlock (reference :618-629) on the streaming kernels: to-RGB (1x1 modulated conv, no demodulation),
        skip add, bilinear x2 and blur — two launches per direction.  The chain keeps the 4-channel storage of the
        to-RGB kernel (channel 3 is zero); returns None when the composable path must run."""
        if not fast_enabled() or os.environ.get("STYLEX_RGB_TAIL", "1") == "0":
            return None
        x = _act(x)
        if not _torgb_route(x, weight, demod=False):
            return None
        if prev_rgb is not None and (prev_rgb.shape[1] != 4 or prev_rgb.dtype != x.dtype):
            return None
        rgb = _ToRGBFast.apply(x, style + 1, weight)
        if upsample:
            return _RGBTailFast.apply(rgb, prev_rgb)
        return rgb if prev_rgb is None else rgb + prev_rgb

    @staticmethod
    def residual_merge(x, res):
        return (x + res) * (1 / math.sqrt(2))

    @staticmethod
    def dblock(x, conv_res, conv1, conv2, down):
        """Whole DiscriminatorBlock as one fused autograd node, or None when the composable path must run (a double
        backward may be requested, or STYLEX_DBLOCK=0)."""
        if not fast_enabled() or os.environ.get("STYLEX_DBLOCK", "1") == "0":
            return None
        if conv1.weight.shape[0] % 4 != 0:
            return None
        return _DBlockFast.apply(x, conv_res.weight, conv_res.bias, conv1.weight, conv1.bias, conv2.weight, conv2.bias,
                                 down.weight if down is not None else None, down.bias if down is not None else None,
                                 down is not None)

    @staticmethod
    def style_edit_levels(coords, smin, smax, sindex, direction, base_class, level_k, seg_start, shift_size):
        """The edited style vectors of attfind.counterfactual_images for all levels of an image batch, one launch; the
        blocks' style segments as dense [L, N, w] tensors."""
        return hb.style_edit_levels(coords, smin, smax, sindex, direction, base_class, level_k, seg_start, shift_size)

    @staticmethod
    def rowwise_sumsq(x2d):
        return _RowSumSq.apply(x2d)


_IMPL = HipOps


def use_impl(impl):
    """Install another implementation object (tests only: a CPU test double)."""
    global _IMPL
    prev = _IMPL
    _IMPL = impl
    return prev


def impl():
    return _IMPL


class _EqualLinearFast(torch.autograd.Function):
    """lrelu(x @ (W * lr_mul)^T + b * lr_mul) — one EqualLinear (+ LeakyReLU) of the mapping network (reference
    :576-601) as one autograd node: the scaled parameters come from a per-version cache, forward = one addmm + one
    in-place LeakyReLU, backward = activation derivative, two GEMMs, one scale, one column sum (the ATen composition
    was 4-5 launches forward and 8-9 backward per layer).  First-order only: the mapping network is never
    differentiated twice (the path-length penalty differentiates G with respect to its styles, reference :306-316)."""

    @staticmethod
    def forward(ctx, x, w, b, lr_mul, slope):
        ws, bs = hb.scaled_linear_params(w, b, lr_mul)
        y = torch.addmm(bs, x, ws.t()) if bs is not None else torch.mm(x, ws.t())
        if slope is not None:
            y = F.leaky_relu_(y, slope)
        ctx.save_for_backward(x, ws, y if slope is not None else None)
        ctx.cfg = (lr_mul, slope, b is not None)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, ws, y = ctx.saved_tensors
        lr_mul, slope, has_b = ctx.cfg
        if y is not None:
            g = torch.ops.aten.leaky_relu_backward(g, y, slope, True)
        gx = torch.mm(g, ws) if ctx.needs_input_grad[0] else None
        gw = gb = None
        if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
            gs = g * lr_mul  # d(W * lr_mul) / dW: scale the (small) activation gradient once instead of both results
            gw = torch.mm(gs.t(), x) if ctx.needs_input_grad[1] else None
            gb = gs.sum(0) if has_b and ctx.needs_input_grad[2] else None
        return gx, gw, gb, None, None


def equal_linear(x, weight, bias, lr_mul, slope=None):
    """EqualLinear (+ LeakyReLU(slope)) on the fused node when first-order gradients suffice, else the composition."""
    if (_IMPL is HipOps and x.is_cuda and x.dim() == 2 and fast_enabled() and x.dtype == torch.float32
            and os.environ.get("STYLEX_EQL", "1") != "0"):
        return _EqualLinearFast.apply(x, weight, bias, lr_mul, slope)
    y = F.linear(x, weight * lr_mul, bias=None if bias is None else bias * lr_mul)
    return y if slope is None else F.leaky_relu(y, slope)


class _StyleAffines(torch.autograd.Function):
    """The three affine style maps of a GeneratorBlock on ONE input — to_style1, to_style2 and to_rgb.to_style (reference
    :682-688, :609: three nn.Linear(latent, C) applied to the block's style vector) — as one GEMM each way over the
    concatenated weights (round 6).  Separately they are 3 addmm forward and, backward, 3 data-gradient GEMMs whose results
    the engine sums with two add_ launches, 3 weight-gradient GEMMs and 3 bias sums: 14 launches per block and pass, all on
    the generator's serial chain; here 1 forward (the concatenated weight is cached per parameter stamp) and 4 backward.
    The parameters stay the reference's three modules (state dict, AttFind's in-place bias edits)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3):
        wcat, bcat = hb.vectors.get((w1, b1, w2, b2, w3, b3), "vec", lambda: (
            torch.cat((w1.detach(), w2.detach(), w3.detach()), dim=0), torch.cat((b1.detach(), b2.detach(), b3.detach()))), tag="affines")
        y = torch.addmm(bcat, x, wcat.t())
        ctx.save_for_backward(x, wcat)
        n1, n2, n3 = ctx.sizes = (w1.shape[0], w2.shape[0], w3.shape[0])
        # four views of ONE result: style1, style2, the to-RGB style, and [style1 | style2] = the block's style coordinates.
        # (Slicing the result outside the node cost a zero-filled full-width tensor + an add_ per slice in the backward.)
        return y[:, :n1], y[:, n1:n1 + n2], y[:, n1 + n2:], y[:, :n1 + n2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g1, g2, g3, gc):
        x, wcat = ctx.saved_tensors
        n1, n2, n3 = ctx.sizes
        need = ctx.needs_input_grad
        z = lambda n: x.new_zeros(x.shape[0], n)  # noqa: E731  (a style nobody used)
        gy = torch.cat((g1 if g1 is not None else z(n1), g2 if g2 is not None else z(n2), g3 if g3 is not None else z(n3)), dim=1)
        if gc is not None:  # a consumer of the style coordinates (get_style_coords=True under autograd)
            gy[:, :n1 + n2] += gc
        gx = gy @ wcat if need[0] else None
        gws = gbs = (None, None, None)
        if any(need[1:7]):
            gws = (gy.t() @ x).split((n1, n2, n3), dim=0)  # row blocks of one matrix: contiguous tensors
            gbs = gy.sum(dim=0).split((n1, n2, n3))
        return (gx, gws[0] if need[1] else None, gbs[0] if need[2] else None, gws[1] if need[3] else None,
                gbs[1] if need[4] else None, gws[2] if need[5] else None, gbs[2] if need[6] else None)


def style_affines(istyle, lin1, lin2, lin3):
    """(to_style1(w), to_style2(w), to_rgb.to_style(w), [style1 | style2]) as four views of one GEMM result (the fused node
    above), or None when the composable path must run (CPU double, double backward, non-fp32 / non-2D input)."""
    if not (_IMPL is HipOps and istyle.is_cuda and istyle.dim() == 2 and fast_enabled() and istyle.dtype == torch.float32
            and os.environ.get("STYLEX_STYLE_FUSE", "1") != "0"):
        return None
    for lin in (lin1, lin2, lin3):
        if lin.bias is None or lin.weight.dtype != torch.float32:
            return None
    return _StyleAffines.apply(istyle, lin1.weight, lin1.bias, lin2.weight, lin2.bias, lin3.weight, lin3.bias)


class _ModCoeffs(torch.autograd.Function):
    """(style + 1, demodulation coefficient) of a modulated conv as ONE launch (csrc/style_coeffs.hip; `wsq`, the
    weight-only factor, is cached per parameter version) with a two-launch first-order backward — the ATen composition
    below is ~8 launches forward and ~15 backward per call, 28 calls per step."""

    @staticmethod
    def forward(ctx, style, weight, eps):
        wsq = hb.weight_sumsq(weight)
        s1, d = hb.modcoeff_fwd(style, wsq, eps)
        ctx.save_for_backward(s1, d, wsq, weight)
        return s1, d

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gs1, gd):
        s1, d, wsq, weight = ctx.saved_tensors
        need_s, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if gd is None:  # the coefficient was not used: only the direct gradient of s1 remains
            return (gs1 if need_s else None), None, None
        gstyle, gw = hb.modcoeff_bwd(gd, d, s1, wsq, weight, gs1, need_s, need_w)
        return gstyle, gw, None


def mod_coeffs(style, weight, demod=True, eps=1e-8):
    """(s+1, demodulation coefficient) of a modulated conv (:650-656 in the batched form): small dense math on
    [B,C] / [O,I] tensors, independent of the activations — the Generator evaluates it for all layers ahead of
    the conv chain on a companion stream."""
    if (demod and _IMPL is HipOps and style.is_cuda and fast_enabled() and style.dim() == 2
            and os.environ.get("STYLEX_MODCOEFF", "1") != "0"):
        return _ModCoeffs.apply(style, weight, eps)
    s1 = style + 1
    d = None
    if demod:
        wsq = weight.pow(2).sum(dim=(2, 3))  # [O, I]
        d = torch.rsqrt((s1 * s1) @ wsq.t() + eps)  # [B, O]
    return s1, d


def conv2d(*a, **k):
    return _IMPL.conv2d(*a, **k)


def modulated_conv2d(*a, **k):
    return _IMPL.modulated_conv2d(*a, **k)


def noise_act(*a, **k):
    return _IMPL.noise_act(*a, **k)


def modconv_noise_act(*a, **k):
    return _IMPL.modconv_noise_act(*a, **k)


def upsample2x(x):
    return _IMPL.upsample2x(x)


def blur3x3(x):
    return _IMPL.blur3x3(x)


def blur_down(*a, **k):
    return _IMPL.blur_down(*a, **k)


def rgb_block(*a, **k):
    fn = getattr(_IMPL, "rgb_block", None)
    return fn(*a, **k) if fn is not None else None


def residual_merge(x, res):
    return _IMPL.residual_merge(x, res)


def rowwise_sumsq(x2d):
    return _IMPL.rowwise_sumsq(x2d)


# ------------------------------------------------------------------------------------------
# linear-attention blocks (attn_layers; reference stylex/stylex_train.py:100-206): ChanNorm, the depthwise 3x3 of
# to_kv and the attention core.  Each op has a COMPOSABLE path (the reference's formula in plain torch ops: CPU
# tensors, shapes the kernels do not cover, and every pass that is differentiated twice) and a FUSED path
# (csrc/linattn.hip) for CUDA tensors.  These three do not go through the implementation object: on CPU tensors they
# never touch hip_backend, so the CPU suite runs them as they are.
# ------------------------------------------------------------------------------------------

_ATTN_FUSED = os.environ.get("STYLEX_ATTN_FUSED", "1") != "0"


def set_attn_fused(flag):
    """False: CUDA tensors take the composable (ATen) path too — the baseline of tools/bench_attn.py."""
    global _ATTN_FUSED
    prev = _ATTN_FUSED
    _ATTN_FUSED = bool(flag)
    return prev


def _wide(t):
    """fp32 working precision for the composable formulas (bf16 activations are widened; fp32 / fp64 stay)."""
    return t.float() if t.dtype in (torch.bfloat16, torch.float16) else t


def _narrow(y, like):
    """Result dtype of a composable op: the activation dtype on the GPU, the input's own dtype on the CPU."""
    if like.is_cuda:
        return _act(y)
    return y if y.dtype == like.dtype else y.to(like.dtype)


def _chan_norm_composable(x, g, b, eps):
    x = _wide(x)
    mean = x.mean(dim=1, keepdim=True)
    std = x.var(dim=1, unbiased=False, keepdim=True).sqrt()
    return (x - mean) / (std + eps) * g + b  # eps joins the standard deviation, not the variance


def _depthwise_composable(x, w):
    return F.conv2d(_wide(x), w, None, stride=1, padding=1, groups=w.shape[0])


def _linattn_composable(q, k, v, heads):
    b, c, h, w = q.shape
    d, n = c // heads, h * w
    q, k, v = (_wide(t).reshape(b, heads, d, n) for t in (q, k, v))
    q = q.softmax(dim=2) * d ** -0.5  # over the channels of a head, per pixel
    k = k.softmax(dim=3)  # over the pixels, per (sample, head, channel)
    context = torch.matmul(k, v.transpose(2, 3))  # [b, heads, d, e]
    out = torch.matmul(context.transpose(2, 3), q)  # [b, heads, e, n]
    return F.gelu(out.reshape(b, c, h, w))  # exact (erf) GELU


def _second_order_grads(ctx, fn, inputs, n_data, gy):
    """Backward of a fused Function while the backward pass itself is being recorded (create_graph=True: gradient
    penalty, path length): the composable formula is re-evaluated on the saved inputs and differentiated by autograd,
    so the returned gradients carry a graph.  inputs[:n_data] are activations, the rest parameters."""
    idx = [i for i in range(len(inputs))
           if ctx.needs_input_grad[i] and inputs[i].requires_grad and (i < n_data or not _INPUTS_ONLY)]
    out = [None] * len(inputs)
    if idx:
        with torch.enable_grad():
            y = fn(*inputs)
            grads = torch.autograd.grad(y, [inputs[i] for i in idx], gy.to(y.dtype), create_graph=True, allow_unused=True)
        for i, g in zip(idx, grads):
            out[i] = g
    return out


class _ChanNormFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, b, eps):
        y, mean, std = hb.chan_norm_fwd(_cl(x), g, b, eps)
        ctx.save_for_backward(x, g, b, mean, std)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, gy):
        x, g, b, mean, std = ctx.saved_tensors
        eps = ctx.eps
        if torch.is_grad_enabled():
            return (*_second_order_grads(ctx, lambda x_, g_, b_: _act(_chan_norm_composable(x_, g_, b_, eps)), (x, g, b), 1, gy),
                    None)
        want_p = (_want_param_grad(ctx, 1) or _want_param_grad(ctx, 2))
        gx, dg, db = hb.chan_norm_bwd(_cl(x), _cl(gy), g, mean, std, eps, want_params=want_p)
        return (gx if ctx.needs_input_grad[0] else None, dg.view_as(g) if want_p and ctx.needs_input_grad[1] else None,
                db.view_as(b) if want_p and ctx.needs_input_grad[2] else None, None)


class _DWConv(torch.autograd.Function):
    """Depthwise 3x3 / pad 1.  Closed under differentiation like the dense triad above:
    DW(x, w) --bwd--> DW(gy, flip w), DWW(x, gy);   DWW(x, gy) --bwd--> DW(gy, flip ggw), DW(x, ggw)."""

    @staticmethod
    def forward(ctx, x, w):
        x = _cl(x)
        ctx.save_for_backward(x, w)
        return hb.dwconv3x3_fwd(x, w)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = _DWConv.apply(gy, w.flip(2, 3)) if ctx.needs_input_grad[0] else None
        gw = _DWWgrad.apply(x, gy) if _want_param_grad(ctx, 1) else None
        return gx, gw


class _DWWgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gy):
        x, gy = _cl(x), _cl(gy)
        ctx.save_for_backward(x, gy)
        return hb.dwconv3x3_bwd_weight(x, gy)

    @staticmethod
    def backward(ctx, ggw):
        x, gy = ctx.saved_tensors
        ggw = ggw.contiguous()
        d_x = _DWConv.apply(gy, ggw.flip(2, 3)) if ctx.needs_input_grad[0] else None
        d_gy = _DWConv.apply(x, ggw) if ctx.needs_input_grad[1] else None
        return d_x, d_gy


class _LinAttnFused(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, heads):
        y, pre, context, lse = hb.linattn_fwd(q, k, v, heads)
        ctx.save_for_backward(q, k, v, pre, context, lse)
        ctx.heads = heads
        return y

    @staticmethod
    def backward(ctx, gy):
        q, k, v, pre, context, lse = ctx.saved_tensors
        heads = ctx.heads
        if torch.is_grad_enabled():
            return (*_second_order_grads(ctx, lambda q_, k_, v_: _act(_linattn_composable(q_, k_, v_, heads)), (q, k, v), 3, gy),
                    None)
        dq, dk, dv = hb.linattn_bwd(q, k, v, pre, context, lse, _cl(gy), heads)
        return dq, dk, dv, None


def _attn_fused(x):
    return x.is_cuda and _ATTN_FUSED


def chan_norm(x, g, b, eps=1e-5):
    """ChanNorm: per pixel over the channels, (x - mean) / (sqrt(biased var) + eps) * g + b; g, b: [1, C, 1, 1]."""
    if _attn_fused(x) and hb.chan_norm_supported(x.shape[1]):
        return _ChanNormFused.apply(_act(x), g, b, float(eps))
    return _narrow(_chan_norm_composable(x, g, b, eps), x)


def depthwise_conv3x3(x, weight):
    """nn.Conv2d(C, C, 3, padding=1, groups=C, bias=False); weight: [C, 1, 3, 3]."""
    if _attn_fused(x) and hb.dwconv3x3_supported(x.shape[1]):
        return _DWConv.apply(_act(x), weight)
    return _narrow(_depthwise_composable(x, weight), x)


def linear_attention_core(q, k, v, heads):
    """gelu(softmax_channels(q) * d^-0.5 @ (softmax_pixels(k)^T @ v)) per (sample, head); q, k, v: [B, heads * d, H, W]."""
    if _attn_fused(q) and hb.linattn_supported(q.shape[1], heads):
        return _LinAttnFused.apply(_act(q), _act(k), _act(v), int(heads))
    return _narrow(_linattn_composable(q, k, v, heads), q)


# ------------------------------------------------------------------------------------------
# no_const (reference stylex/stylex_train.py:766-769, :798-802): the generator's first activation is a transposed conv of
# the layer-averaged style instead of a learned constant.  On its 1x1 input that is x = mean_l(styles) @ W, bilinear in
# (styles, W), and like the dense conv triad it is closed under differentiation (csrc/initial_block.hip):
#
#     IB(s, w)    --bwd-->  IBD(gx, w), IBW(s, gx)
#     IBD(gx, w)  --bwd-->  IB(ggs, w), IBW(ggs, gx)
#     IBW(s, gx)  --bwd-->  IBD(gx, ggw), IB(s, ggw)
#
# so the path-length step (styles -> x -> image differentiated twice) stays on the three launches.  CPU tensors and shapes
# the kernels do not cover take the reference's formula in plain torch ops; like the attention ops this one does not go
# through the implementation object.
# ------------------------------------------------------------------------------------------

_INITIAL_BLOCK_FUSED = os.environ.get("STYLEX_INITIAL_BLOCK_FUSED", "1") != "0"


def set_initial_block_fused(flag):
    """False: CUDA tensors take the composable (ATen) path too — the baseline of an A/B."""
    global _INITIAL_BLOCK_FUSED
    prev = _INITIAL_BLOCK_FUSED
    _INITIAL_BLOCK_FUSED = bool(flag)
    return prev


def _initial_block_composable(styles, w):
    return F.conv_transpose2d(_wide(styles).mean(dim=1)[:, :, None, None], w)


class _InitialBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, styles, w, out_dtype):
        styles = hb._f32c(styles)
        ctx.save_for_backward(styles, w)
        return hb.initial_block_fwd(styles, w, _PRECISION, out_dtype)

    @staticmethod
    def backward(ctx, gx):
        styles, w = ctx.saved_tensors
        ds = _InitialBlockDgrad.apply(gx, w, styles.shape[1]) if ctx.needs_input_grad[0] else None
        dw = _InitialBlockWgrad.apply(styles, gx) if _want_param_grad(ctx, 1) else None
        return ds, dw, None


class _InitialBlockDgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gx, w, layers):
        gx = hb.to_cl(gx)
        ctx.save_for_backward(gx, w)
        return hb.initial_block_bwd_data(gx, w, layers, _PRECISION)

    @staticmethod
    def backward(ctx, ggs):
        gx, w = ctx.saved_tensors
        d_gx = _InitialBlock.apply(ggs, w, gx.dtype) if ctx.needs_input_grad[0] else None
        d_w = _InitialBlockWgrad.apply(ggs, gx) if _want_param_grad(ctx, 1) else None
        return d_gx, d_w, None


class _InitialBlockWgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, styles, gx):
        styles, gx = hb._f32c(styles), hb.to_cl(gx)
        ctx.save_for_backward(styles, gx)
        return hb.initial_block_bwd_weight(styles, gx)

    @staticmethod
    def backward(ctx, ggw):
        styles, gx = ctx.saved_tensors
        d_s = _InitialBlockDgrad.apply(gx, ggw, styles.shape[1]) if ctx.needs_input_grad[0] else None
        d_gx = _InitialBlock.apply(styles, ggw, gx.dtype) if ctx.needs_input_grad[1] else None
        return d_s, d_gx


def initial_block(styles, weight):
    """ConvTranspose2d(D, C, 4, 1, 0, bias=False)(styles.mean(dim=1)[:, :, None, None]); styles [B, L, D], weight
    [D, C, 4, 4].  On the GPU the result is channels-last in the activation dtype."""
    if (styles.is_cuda and _INITIAL_BLOCK_FUSED and styles.dim() == 3 and weight.dim() == 4 and tuple(weight.shape[2:]) == (4, 4)
            and weight.shape[0] == styles.shape[2] and weight.dtype == torch.float32
            and hb.initial_block_supported(*styles.shape, weight.shape[1])):
        return _InitialBlock.apply(styles, weight, act_dtype())
    return _narrow(_initial_block_composable(styles, weight), styles)
