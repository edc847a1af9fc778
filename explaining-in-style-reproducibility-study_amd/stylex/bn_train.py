"""Training-mode BatchNorm2d with its activation / residual tail, and the softmax cross-entropy, on the kernels of
csrc/bn_train.hip — what sits between the library's convolutions when the classifier that StylEx explains is trained
(stylex/train_classifier.py; reference stylex/train_mobilenet_classifier.py and classifier_training_celeba.ipynb).

``BatchNormAct`` is an ``nn.BatchNorm2d`` (same parameters, buffers and state-dict keys) with an ``act`` attribute
('none' | 'relu' | 'relu6') and an optional residual argument: ``act(bn(x) (+ residual))``.

Selection rule (explicit tests): the kernels run when the module is in training mode, ``affine`` and
``track_running_stats`` are on, ``momentum`` is a number, the input (and residual) is a dense fp32 CUDA NCHW tensor
(with fewer than 2 values per channel: torch's ValueError) and the module's ``shape_rule`` admits the shape — by default
``measured_shape_rule``: the shapes at which the fused group was measured faster than ATen's.  Every other case is the
composable formula, ``F.batch_norm`` + activation.  A launch that fails raises (hip_backend._check); the composable formula is never a
fallback for it.

First-order gradients only: the fused node's backward is ``once_differentiable`` and raises under ``create_graph=True``.
"""
import functools

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

import hip_backend as hb
import tv_models

ACTS = ("none", "relu", "relu6")
NEED_MORE_VALUES = "Expected more than 1 value per channel when training, got input size {}"


def measured_shape_rule(b, c, hw, needs_grad):
    """Which [B, C, H, W] calls run on the kernels: those at which tools/bench_classifier.py measured the fused group faster
    than F.batch_norm + activation on an MI355X (profiles/classifier_train_timing.txt; MobileNetV2 at B = 200 and ResNet-18 at
    B = 128, 224 px).  The fused group is 4 launches forward and 3 backward; below these sizes their fixed cost exceeds what
    the single passes save, and ATen's kernels for small planes are as fast per byte.
      forward only (nothing needs a gradient: the frozen layers): H * W >= 784 and at least 4 M elements
          (won at 28 x 28 from 5.0 M elements and at every larger plane; lost at every 14 x 14 and 7 x 7 shape, up to 22.6 M);
      with a backward: H * W >= 3136 and at least 16 M elements
          (won 2.1 - 2.6 x at 56 x 56 / 25.7 M and 112 x 112; lost at 28 x 28 / 12.8 M and below; nothing between was measured)."""
    numel = b * c * hw
    if needs_grad:
        return hw >= 3136 and numel >= 16000000
    return hw >= 784 and numel >= 4000000


def every_shape(*shape):
    """The shape rule that sends every supported call to the kernels (tests, tools/bench_classifier.py, --fused_shapes all)."""
    return True


CE_MIN_LOGITS = 1 << 23


def measured_ce_rule(b, k):
    """Which [B, K] logits take the cross-entropy kernels: B * K >= CE_MIN_LOGITS.  Measured (tools/bench_classifier.py, forward
    + backward with the correct count, MI355X): both forms are launch-bound at every size tried (4096 x 1000 takes the time of
    128 x 2: 0.07 - 0.13 ms), and the fused form took 1.12 - 1.26 x ATen's time in three of the four sections of two runs and
    0.89 - 0.91 x in the fourth: at no measured size is it faster.  So everything up to the largest size measured (4 M logits)
    stays on F.cross_entropy + argmax, the classifier's own B x 2 logits included.  The kernels take 8 M logits and more, twice
    that size, where seven passes over 32 MB cost ATen more than its launches (not measured)."""
    return b * k >= CE_MIN_LOGITS


def _activate(v, act):
    if act == "relu":
        return F.relu(v)
    if act == "relu6":
        return F.relu6(v)
    return v


def _dense_cuda_f32(t):
    return t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.is_contiguous()


def _first_order_only(fn):
    """backward of a fused node: raises when the backward pass itself is being recorded (create_graph=True), and is
    once_differentiable besides (a later attempt to differentiate its results raises too)."""
    inner = once_differentiable(fn)

    @functools.wraps(fn)
    def backward(ctx, *grads):
        if torch.is_grad_enabled():
            raise RuntimeError("%s has first-order gradients only (create_graph=True was requested); use the composable "
                               "formula (F.batch_norm / F.cross_entropy) for second derivatives" % type(ctx).__name__)
        return inner(ctx, *grads)

    return backward


class _BatchNormActFn(torch.autograd.Function):
    """stats -> fused normalise / activation forward; reduce -> apply backward.  Saves x, y (when there is an activation),
    the batch statistics and gamma — or nothing at all when no input needs a gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, momentum, eps, act):
        mean, var = hb.bn_stats(x, running_mean, running_var, momentum)
        y = hb.bn_act_fwd(x, mean, var, gamma, beta, eps, residual, act)
        ctx.act, ctx.eps = act, eps
        if any(ctx.needs_input_grad[:4]):
            ctx.save_for_backward(x, y if act != "none" else None, mean, var, gamma)
        return y

    @staticmethod
    @_first_order_only
    def backward(ctx, gy):
        x, y, mean, var, gamma = ctx.saved_tensors
        need_x, need_g, need_b, need_r = ctx.needs_input_grad[:4]
        gy = gy.contiguous()
        dgamma, dbeta = hb.bn_act_bwd_reduce(gy, y, x, mean, var, ctx.eps, ctx.act)
        gx = gres = None
        if need_x or (need_r and ctx.act != "none"):
            gx, gres = hb.bn_act_bwd_apply(gy, y, x, mean, var, gamma, dgamma, dbeta, ctx.eps, ctx.act, want_gx=need_x,
                                           want_res=need_r and ctx.act != "none")
        if need_r and ctx.act == "none":
            gres = gy  # no gate: the residual's gradient is gy itself
        return (gx, dgamma if need_g else None, dbeta if need_b else None, gres if need_r else None, None, None, None, None,
                None)


class BatchNormAct(nn.BatchNorm2d):
    """act(BatchNorm2d(x) (+ residual)); the parent's parameters, buffers (num_batches_tracked included) and state-dict keys."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, act="none", **kw):
        super().__init__(num_features, eps, momentum, affine, track_running_stats, **kw)
        assert act in ACTS, act
        self.act = act
        self.shape_rule = measured_shape_rule

    def extra_repr(self):
        return super().extra_repr() + ", act=" + self.act

    def fused(self, x, residual=None):
        """The explicit test: True when this call runs on the kernels."""
        if not (self.training and self.affine and self.track_running_stats and self.momentum is not None
                and _dense_cuda_f32(x) and (residual is None or (_dense_cuda_f32(residual) and residual.shape == x.shape))
                and self.weight.dtype == torch.float32 and self.weight.is_cuda
                and x.numel() <= 0x7fffffff and x.shape[1] <= 65535):
            return False
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad or self.bias.requires_grad
                                                  or (residual is not None and residual.requires_grad))
        return bool(self.shape_rule(x.shape[0], x.shape[1], x.shape[2] * x.shape[3], needs_grad))

    def forward(self, x, residual=None):
        if not self.fused(x, residual):
            out = super().forward(x)  # F.batch_norm with the parent's bookkeeping
            return _activate(out if residual is None else out + residual, self.act)
        if x.numel() // x.shape[1] < 2:
            raise ValueError(NEED_MORE_VALUES.format(x.size()))
        self.num_batches_tracked.add_(1)
        return _BatchNormActFn.apply(x, self.weight, self.bias, residual, self.running_mean, self.running_var,
                                     float(self.momentum), float(self.eps), self.act)


def _share(bn, act):
    """A BatchNormAct on the SAME parameter and buffer tensors as `bn`."""
    assert type(bn) is nn.BatchNorm2d, type(bn)
    m = BatchNormAct(bn.num_features, bn.eps, bn.momentum, bn.affine, bn.track_running_stats, act=act, device="meta")
    for k in list(m._parameters):
        m._parameters[k] = bn._parameters[k]
    for k in list(m._buffers):
        m._buffers[k] = bn._buffers[k]
    m.train(bn.training)
    return m


class _FusedBasicBlock(nn.Module):
    def __init__(self, blk):
        super().__init__()
        self.conv1, self.bn1 = blk.conv1, _share(blk.bn1, "relu")
        self.conv2, self.bn2 = blk.conv2, _share(blk.bn2, "relu")
        self.downsample = None
        if blk.downsample is not None:
            self.downsample = nn.Sequential(blk.downsample[0], _share(blk.downsample[1], "none"))

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        return self.bn2(self.conv2(self.bn1(self.conv1(x))), idt)


class _FusedResNet18(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.conv1, self.bn1, self.maxpool = net.conv1, _share(net.bn1, "relu"), net.maxpool
        for i in range(1, 5):
            setattr(self, "layer%d" % i, nn.Sequential(*[_FusedBasicBlock(b) for b in getattr(net, "layer%d" % i)]))
        self.avgpool, self.fc = net.avgpool, net.fc

    def forward(self, x):
        x = self.maxpool(self.bn1(self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def _fused_conv_bn_relu6(seq):
    return nn.Sequential(seq[0], _share(seq[1], "relu6"))


class _FusedInvertedResidual(nn.Module):
    def __init__(self, blk):
        super().__init__()
        self.use_res = blk.use_res
        layers = [_fused_conv_bn_relu6(m) for m in list(blk.conv)[:-2]]
        self.conv = nn.Sequential(*layers, blk.conv[-2], _share(blk.conv[-1], "none"))

    def forward(self, x):
        h = x
        for m in list(self.conv)[:-1]:
            h = m(h)
        return self.conv[-1](h, x if self.use_res else None)


class _FusedMobileNetV2(nn.Module):
    def __init__(self, net):
        super().__init__()
        feats = [_FusedInvertedResidual(m) if isinstance(m, tv_models.InvertedResidual) else _fused_conv_bn_relu6(m)
                 for m in net.features]
        self.features = nn.Sequential(*feats)
        self.classifier = net.classifier

    def forward(self, x):
        return self.classifier(self.features(x).mean(dim=(2, 3)))


def fuse_for_training(model, shape_rule=None):
    """A module that computes what `model` (tv_models.ResNet18 / MobileNetV2) computes, with every (bn, relu), (bn, relu6),
    (bn) and (bn + identity, relu) group on one BatchNormAct.  It SHARES the parameters and buffers of `model` (the same
    tensor objects: an optimiser step, a running-statistics update or a load_state_dict on either is seen by both) and has the
    same state-dict keys; `model` itself is not changed.  Fuse after moving `model` to its device: Module.to() gives each
    module new buffer tensors.  shape_rule(b, c, hw, needs_grad) -> bool picks the calls that run on the kernels among those the
    selection rule admits (default: measured_shape_rule; every_shape: all of them)."""
    if isinstance(model, tv_models.ResNet18):
        fused = _FusedResNet18(model)
    elif isinstance(model, tv_models.MobileNetV2):
        fused = _FusedMobileNetV2(model)
    else:
        raise TypeError("fuse_for_training takes a tv_models.ResNet18 or MobileNetV2, got %s" % type(model).__name__)
    for m in fused.modules():
        if isinstance(m, BatchNormAct):
            m.shape_rule = shape_rule or measured_shape_rule
    fused.train(model.training)
    return fused


class _SoftmaxCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        loss, n_correct = hb.softmax_ce_fwd(logits, targets)
        ctx.save_for_backward(logits, targets)
        ctx.mark_non_differentiable(n_correct)
        return loss, n_correct

    @staticmethod
    @_first_order_only
    def backward(ctx, gloss, _gcount):
        logits, targets = ctx.saved_tensors
        return hb.softmax_ce_bwd(logits, targets, gloss.contiguous().float()), None


def softmax_ce_fused(logits, targets):
    """The explicit test of softmax_cross_entropy: dense fp32 CUDA logits [B, K <= 1024] with int64 targets [B]."""
    return (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
            and 1 <= logits.shape[1] <= hb.SOFTMAX_CE_MAX_K and logits.shape[0] >= 1 and targets.is_cuda
            and targets.dtype == torch.int64 and targets.dim() == 1 and targets.is_contiguous()
            and targets.shape[0] == logits.shape[0])


def softmax_cross_entropy(logits, targets, shape_rule=measured_ce_rule):
    """(loss, n_correct): nn.CrossEntropyLoss() (mean) of `logits` against class indices `targets`, and the number of rows
    whose argmax (lowest index on ties) equals the target, as a 0-d int64 tensor on the logits' device — no host read.
    shape_rule(b, k) -> bool picks the shapes that run on the kernels among those softmax_ce_fused admits."""
    if softmax_ce_fused(logits, targets) and shape_rule(logits.shape[0], logits.shape[1]):
        return _SoftmaxCEFn.apply(logits, targets)
    return F.cross_entropy(logits, targets), (torch.argmax(logits.detach(), dim=1) == targets).sum()
