"""attn_layers on the MI355X: the kernels of csrc/linattn.hip against float64 definitions written here, the fused path
against the composable one, the reference's networks and Trainer steps (tests/golden/attn_*.npz, steps_attn*.npz) on the
HIP path, run-to-run bit identity, and the config-2 sized launches.  fp32 at TOL32, bf16 at TOLBF (the constants of
tests/test_hip_parity.py), bf16 cases compared on bf16-rounded inputs.  Every figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_backend as hb  # noqa: E402
import ops  # noqa: E402
import stylex_train as st  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_attn_cpu import ATTN, attn_model, check_module_case, check_nets, check_steps  # noqa: E402
from test_hip_parity import DEV, TOL32, TOLBF  # noqa: E402
from test_host_logic_cpu import make_trainer, run_steps  # noqa: E402


@pytest.fixture(autouse=True)
def hip_impl():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    prev = ops.use_impl(ops.HipOps)
    ops.set_precision("fp32")
    hb.load_library()
    prev_fast, prev_fused = ops.set_fast(False), ops.set_attn_fused(True)
    yield
    ops.set_fast(prev_fast)
    ops.set_attn_fused(prev_fused)
    ops.set_precision("fp32")
    ops.use_impl(prev)


def close(a, b, tol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1e-3, a.abs().max().item())
    err = (a - b).abs().max().item()
    print("%-28s max err %.3e  scale %.3e  (%.2e of scale, tol %.1e)" % (what, err, scale, err / scale, tol))
    assert math.isfinite(err) and err <= tol * scale, "%s: max err %.3e (scale %.3e, tol %.1e)" % (what, err, scale, tol)


def tol_of(prec):
    return TOL32 if prec == "fp32" else TOLBF


def rounded(t, prec):
    """the values the kernels see: bf16-rounded in the speed mode"""
    return t.bfloat16().float() if prec == "bf16" else t


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


# ---- float64 definitions ------------------------------------------------------------------------------------------------

def chan_norm_def(x, g, b, eps=1e-5):
    mean = x.mean(dim=1, keepdim=True)
    std = ((x - mean) ** 2).mean(dim=1, keepdim=True).sqrt()
    return (x - mean) / (std + eps) * g + b


def depthwise_def(x, w):
    b, c, h, wd = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    y = torch.zeros_like(x)
    for kh in range(3):
        for kw in range(3):
            y = y + xp[:, :, kh:kh + h, kw:kw + wd] * w[:, 0, kh, kw].view(1, c, 1, 1)
    return y


def linattn_def(q, k, v, heads):
    b, c, h, w = q.shape
    d = c // heads
    q, k, v = (t.reshape(b, heads, d, h * w) for t in (q, k, v))  # [b, head, channel, pixel]
    q = torch.exp(q - q.amax(dim=2, keepdim=True))
    q = q / q.sum(dim=2, keepdim=True) * d ** -0.5
    k = torch.exp(k - k.amax(dim=3, keepdim=True))
    k = k / k.sum(dim=3, keepdim=True)
    context = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhdn,bhde->bhen", q, context).reshape(b, c, h, w)
    return 0.5 * out * (1 + torch.erf(out / math.sqrt(2.0)))


def grads_of(fn, inputs, r):
    """y and the gradients of sum(y * r) with respect to `inputs` (fresh leaves)"""
    leaves = [t.detach().clone().requires_grad_() for t in inputs]
    y = fn(*leaves)
    return y.detach(), torch.autograd.grad((y.to(r.dtype) * r).sum(), leaves)


def check_against_definition(kernel_fn, def_fn, inputs, prec, names, act=(0,)):
    """`inputs`: fp32 device tensors; those listed in `act` are activations (NHWC, bf16-rounded in the speed mode)."""
    ops.set_precision(prec)
    ops.set_fast(True)  # first-order-only pass: the backward runs the fused kernels
    tol = tol_of(prec)
    inputs = [nhwc(rounded(t, prec)) if i in act else t for i, t in enumerate(inputs)]
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        shape = kernel_fn(*inputs).shape
    r = rounded(torch.randn(shape, generator=gen), prec).to(DEV)
    y, grads = grads_of(kernel_fn, inputs, nhwc(r))
    y64, grads64 = grads_of(def_fn, [t.double() for t in inputs], r.double())
    close(y64, y, tol, "forward")
    for n, a, b in zip(names, grads64, grads):
        close(a, b, tol, "gradient " + n)


# (B, C, H, W): both config-2 pixel counts at batch 1, a ragged H*W, host widths 16 / 64 / 128
HOST_CASES = [(1, 64, 128, 128), (1, 128, 64, 64), (2, 16, 5, 7), (3, 64, 9, 11)]


@pytest.mark.against_definition
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", HOST_CASES)
def test_chan_norm_kernels_vs_definition(shape, prec):
    gen = torch.Generator().manual_seed(sum(shape))
    c = shape[1]
    x = (torch.randn(shape, generator=gen) * 1.5 + 0.3).to(DEV)
    g = (1 + 0.3 * torch.randn(1, c, 1, 1, generator=gen)).to(DEV)
    b = (0.2 * torch.randn(1, c, 1, 1, generator=gen)).to(DEV)
    assert hb.chan_norm_supported(c)
    check_against_definition(lambda x_, g_, b_: ops.chan_norm(x_, g_, b_, 1e-5), lambda x_, g_, b_: chan_norm_def(x_, g_, b_, 1e-5),
                             [x, g, b], prec, ["x", "g", "b"])


@pytest.mark.against_definition
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", HOST_CASES)
def test_depthwise_kernels_vs_definition(shape, prec):
    gen = torch.Generator().manual_seed(sum(shape) + 1)
    c = shape[1]
    x = torch.randn(shape, generator=gen).to(DEV)
    w = (torch.randn(c, 1, 3, 3, generator=gen) / 3).to(DEV)
    assert hb.dwconv3x3_supported(c)
    check_against_definition(ops.depthwise_conv3x3, depthwise_def, [x, w], prec, ["x", "w"])


# (B, heads, H, W)
CORE_CASES = [(1, 8, 128, 128), (1, 8, 64, 64), (2, 8, 5, 7), (2, 2, 9, 11), (1, 1, 1, 1)]


def core_inputs(case, seed=0):
    b, heads, h, w = case
    gen = torch.Generator().manual_seed(seed + b * 1000 + h * w)
    q = (torch.randn(b, 64 * heads, h, w, generator=gen) * 2).to(DEV)
    kv = (torch.randn(b, 128 * heads, h, w, generator=gen) * 2).to(DEV)
    return q, kv


@pytest.mark.against_definition
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CORE_CASES)
def test_attention_core_kernels_vs_definition(case, prec):
    """k and v are the two channel halves of one NHWC tensor, as LinearAttention hands them over (strided, no copy)."""
    heads = case[1]
    q, kv = core_inputs(case)

    def fused(q_, kv_):
        k_, v_ = kv_.chunk(2, dim=1)
        return ops.linear_attention_core(q_, k_, v_, heads)

    def definition(q_, kv_):
        k_, v_ = kv_.chunk(2, dim=1)
        return linattn_def(q_, k_, v_, heads)

    check_against_definition(fused, definition, [q, kv], prec, ["q", "kv"], act=(0, 1))


@pytest.mark.against_definition
def test_config2_sized_launches_vs_definition():
    """The config-2 shapes (B = 64 at 128^2 and 64^2, inner width 512, host widths 64 / 128, bf16) once through the fused
    forward + backward: the large-launch plans (4 and 4 pixel chunks per (sample, head), 1024-block streams) get a
    definition test.  The float64 definition runs on the GPU, eight samples at a time."""
    ops.set_precision("bf16")
    ops.set_fast(True)
    for b, c_host, side in ((64, 64, 128), (64, 128, 64)):
        gen = torch.Generator(device=DEV).manual_seed(side)
        q = nhwc((torch.randn(b, 512, side, side, device=DEV, generator=gen) * 2).bfloat16())
        kv = nhwc((torch.randn(b, 1024, side, side, device=DEV, generator=gen) * 2).bfloat16())
        r = nhwc(torch.randn(b, 512, side, side, device=DEV, generator=gen).bfloat16())
        ql, kvl = q.clone().requires_grad_(), kv.clone().requires_grad_()
        k_, v_ = kvl.chunk(2, dim=1)
        y = ops.linear_attention_core(ql, k_, v_, 8)
        gq, gkv = torch.autograd.grad((y.float() * r.float()).sum(), [ql, kvl])
        worst = {}
        for s in range(0, b, 8):
            q64, kv64 = q[s:s + 8].double().requires_grad_(), kv[s:s + 8].double().requires_grad_()
            k64, v64 = kv64.chunk(2, dim=1)
            y64 = linattn_def(q64, k64, v64, 8)
            gq64, gkv64 = torch.autograd.grad((y64 * r[s:s + 8].double()).sum(), [q64, kv64])
            for name, a, got in (("y", y64, y[s:s + 8]), ("dq", gq64, gq[s:s + 8]), ("dkv", gkv64, gkv[s:s + 8])):
                scale = max(1e-3, a.abs().max().item())
                worst[name] = max(worst.get(name, 0.0), (a - got.double()).abs().max().item() / scale)
            del q64, kv64, y64, gq64, gkv64
        print("attention core B=%d %dx%d: worst error / scale %s (tol %.1e)" % (b, side, side, worst, TOLBF))
        assert all(math.isfinite(v) and v <= TOLBF for v in worst.values()), worst
        del q, kv, r, ql, kvl, y, gq, gkv
        # ChanNorm and the depthwise conv at the host width of this resolution
        x = nhwc((torch.randn(b, c_host, side, side, device=DEV, generator=gen) * 1.5).bfloat16())
        g = 1 + 0.3 * torch.randn(1, c_host, 1, 1, device=DEV, generator=gen)
        bb = 0.2 * torch.randn(1, c_host, 1, 1, device=DEV, generator=gen)
        w = torch.randn(c_host, 1, 3, 3, device=DEV, generator=gen) / 3
        rr = nhwc(torch.randn(b, c_host, side, side, device=DEV, generator=gen).bfloat16())
        for name, fn, dfn, params in (("chan_norm", lambda x_, g_, b_: ops.chan_norm(x_, g_, b_), chan_norm_def, [g, bb]),
                                      ("depthwise", ops.depthwise_conv3x3, depthwise_def, [w])):
            y, grads = grads_of(fn, [x] + params, rr)
            y64, grads64 = grads_of(dfn, [x.double()] + [p.double() for p in params], rr.double())
            close(y64, y, TOLBF, "%s B=%d %dx%d forward" % (name, b, side, side))
            for i, (a, got) in enumerate(zip(grads64, grads)):
                close(a, got, TOLBF, "%s B=%d %dx%d gradient %d" % (name, b, side, side, i))
        torch.cuda.empty_cache()


@pytest.mark.against_definition
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_fused_path_equals_composable_path(prec):
    """Same inputs through the kernels and through the ATen composition, first order (fused backward kernels) and the
    second-order quantity d ||d sum(r y) / d x||^2 / d inputs (the fused Functions' recorded backward)."""
    ops.set_precision(prec)
    tol = tol_of(prec)
    gen = torch.Generator().manual_seed(11)
    x = nhwc(rounded(torch.randn(2, 64, 12, 10, generator=gen) * 1.5, prec).to(DEV))
    g = (1 + 0.3 * torch.randn(1, 64, 1, 1, generator=gen)).to(DEV)
    b = (0.2 * torch.randn(1, 64, 1, 1, generator=gen)).to(DEV)
    w = (torch.randn(64, 1, 3, 3, generator=gen) / 3).to(DEV)
    q = nhwc(rounded(torch.randn(2, 128, 12, 10, generator=gen) * 2, prec).to(DEV))
    kv = nhwc(rounded(torch.randn(2, 256, 12, 10, generator=gen) * 2, prec).to(DEV))

    def core(q_, kv_):
        k_, v_ = kv_.chunk(2, dim=1)
        return ops.linear_attention_core(q_, k_, v_, 2)

    for name, fn, inputs in (("chan_norm", lambda x_, g_, b_: ops.chan_norm(x_, g_, b_), [x, g, b]),
                             ("depthwise", ops.depthwise_conv3x3, [x, w]), ("core", core, [q, kv])):
        with torch.no_grad():
            shape = fn(*inputs).shape
        r = nhwc(rounded(torch.randn(shape, generator=gen), prec).to(DEV))
        res = {}
        for fused in (True, False):
            ops.set_attn_fused(fused)
            ops.set_fast(True)
            y, grads = grads_of(fn, inputs, r)
            ops.set_fast(False)
            leaves = [t.detach().clone().requires_grad_() for t in inputs]
            (gx,) = torch.autograd.grad((fn(*leaves).float() * r.float()).sum(), leaves[0], create_graph=True)
            second = torch.autograd.grad(gx.float().pow(2).sum(), leaves, allow_unused=True)
            res[fused] = [y] + list(grads) + [torch.zeros_like(l) if s is None else s for l, s in zip(leaves, second)]
        ops.set_attn_fused(True)
        for i, (a, got) in enumerate(zip(res[False], res[True])):
            close(a.float(), got.float(), tol, "%s %s #%d" % (name, prec, i))


@pytest.mark.against_definition
@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("kind", ["chan_norm", "depthwise", "linattn"])
def test_isolated_modules_vs_reference_on_hip(kind, case):
    check_module_case(load_golden("attn_ops"), kind, case, device=torch.device(DEV), tol=TOL32)


@pytest.mark.against_definition
def test_networks_vs_reference_on_hip():
    """attn_nets_32 in the fp32 mode, including the gradient penalty and the path lengths (the second-order rule)."""
    g = load_golden("attn_nets_32")
    check_nets(g, attn_model(g, torch.device(DEV)), device=torch.device(DEV), tol=TOL32)


@pytest.mark.parametrize("name", ["steps_attn", "steps_attn_pl"])
def test_trainer_step_parity_with_attention_gpu(name, tmp_path):
    check_steps(name, tmp_path, device=torch.device(DEV))


def test_bf16_steps_with_attention_are_finite_and_inside_the_band(tmp_path):
    """The speed mode on steps_attn: finite everywhere; call 0 inside the arithmetic part of the suite's bf16 band
    (test_bf16_step_band_vs_reference_golden: 5e-2 of max(1, |x|) for d / g / rec / kl, 1e-1 for the gradient penalty)."""
    g = load_golden("steps_attn")
    ops.set_precision("bf16")
    try:
        tr, n = make_trainer(g, tmp_path, device=torch.device(DEV), trainer_cls=functools.partial(st.Trainer, attn_layers=ATTN))
        rows = run_steps(tr, n)
    finally:
        ops.set_precision("fp32")
    gold = g["scalars"]
    print("bf16 rows\n", rows, "\ngolden\n", gold)
    assert np.isfinite(rows[:, :5]).all()
    assert all(torch.isfinite(p).all() for p in tr.StylEx.parameters())
    scale = np.maximum(1.0, np.abs(gold[0, :4]))
    assert (np.abs(rows[0, :4] - gold[0, :4]) <= 5e-2 * scale).all(), (rows[0], gold[0])
    assert abs(rows[0, 4] - gold[0, 4]) <= 1e-1 * max(1.0, abs(gold[0, 4])), (rows[0, 4], gold[0, 4])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_two_attention_trainers_are_bit_identical(prec, tmp_path):
    """Two identically seeded 3-call Trainers with attn_layers=[1, 2] (call 0 is a gradient-penalty step: fused forward,
    recorded ATen backward, fused backward) end with bit-identical parameters.  As in tools/determinism_check.py the
    frozen networks' MIOpen algorithms are pinned and a throw-away Trainer runs first."""
    g = load_golden("steps_attn")
    prev_det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    ops.set_precision(prec)
    try:
        runs = []
        for i in range(3):
            tr, _ = make_trainer(g, tmp_path / str(i), device=torch.device(DEV),
                                 trainer_cls=functools.partial(st.Trainer, attn_layers=ATTN))
            rows = run_steps(tr, 1 if i == 0 else 3)
            if i:
                runs.append((rows, {k: v.detach().clone() for k, v in tr.StylEx.named_parameters()}))
            del tr
    finally:
        ops.set_precision("fp32")
        torch.backends.cudnn.deterministic = prev_det
    print(runs[0][0], runs[1][0], sep="\n")
    diff = [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
    assert not diff, diff[:10]
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True)
