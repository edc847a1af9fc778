"""no_const, rel_disc_loss and top_k_training on the MI355X: the kernels of csrc/initial_block.hip and the two new
reductions of csrc/losses.hip against float64 definitions, run-to-run bit identity, a guard-band run for the ragged
D = 514, and the Trainer on the HIP path (step fixtures of tools/make_golden_variants.py, determinism, the path-length
call, graphs, the drop-in CLI).  Every figure is printed before it is asserted.

Tolerances.  fp32 kernels: TOL32 of tests/test_hip_parity.py (2e-5 of the tensor's max), what the fp32 conv definition
tests use.  bf16 mode of the initial block: twice the bf16-vs-fp32 deviation of the constant path's own first layer (the
3x3 initial_conv) measured in the same test on the same first activation, as a fraction of the tensor's max.  The loss
reductions: 2e-6 of the value's scale, the bound of test_fused_loss_kernels_match_the_torch_compositions (fp32 sums of
at most 1024 terms: 4 serial additions per thread and 8 tree levels, 12 roundings of 6e-8)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import hip_backend as hb  # noqa: E402
import ops  # noqa: E402
import stylex_train as st  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_hip_parity import DEV, TOL32  # noqa: E402
from test_host_logic_cpu import assert_param_stats, make_trainer, run_steps  # noqa: E402
from test_variants_cpu import ALL_ON, variant_trainer  # noqa: E402

LOSS_TOL = 2e-6


@pytest.fixture(autouse=True)
def hip_impl():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    prev = ops.use_impl(ops.HipOps)
    ops.set_precision("fp32")
    hb.load_library()
    prev_fast = ops.set_fast(False)
    yield
    ops.set_fast(prev_fast)
    ops.set_initial_block_fused(True)
    ops.set_precision("fp32")
    ops.use_impl(prev)


def err_of(a, b, what, floor=1e-3):
    """max |a - b| as a fraction of max(floor, max |a|); a = the reference"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(floor, a.abs().max().item())
    err = (a - b).abs().max().item() / scale
    print("%-34s err %.3e of scale %.3e" % (what, err, scale))
    assert math.isfinite(err), what
    return err


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


# ---- the initial block -------------------------------------------------------------------------------------------------

IB_CASES = [(b, l, d, c) for b in (1, 3, 64) for l in (2, 7) for d in (18, 514) for c in (16, 64, 512)]


def ib_inputs(case, prec):
    b, l, d, c = case
    gen = torch.Generator().manual_seed(b * 100003 + l * 1009 + d * 31 + c)
    styles = torch.randn(b, l, d, generator=gen)
    w = torch.randn(d, c, 4, 4, generator=gen) / d ** 0.5
    r = torch.randn(b, c, 4, 4, generator=gen)
    if prec == "bf16":
        r = r.bfloat16().float()  # the incoming gradient is a bf16 tensor in the speed mode
    return styles, w, r


def ib_quantities(fn, s, p, r):
    """forward, both gradients of sum(r x), and d ||d sum(r x) / d styles||^2 / d W; s, p: leaves that require grad"""
    x = fn(s, p)
    gs, gw = torch.autograd.grad((x.to(r.dtype) * r).sum(), [s, p])
    (gs2,) = torch.autograd.grad((fn(s, p).to(r.dtype) * r).sum(), s, create_graph=True)
    (second,) = torch.autograd.grad(gs2.pow(2).sum(), p)
    return {"forward": x.detach(), "d styles": gs, "d W": gw, "second order d W": second}


def ib_definition(styles, w, r):
    """nn.ConvTranspose2d(D, C, 4, 1, 0, bias=False) on the layer-averaged style, float64 on the CPU"""
    return ib_quantities(lambda s, p: F.conv_transpose2d(s.mean(dim=1)[:, :, None, None], p), styles.double().requires_grad_(),
                         w.double().requires_grad_(), r.double())


def bf16_budget(x64, c, gen):
    """bf16-vs-fp32 deviation of the constant path's first layer on the same first activation: the 3x3 initial_conv
    (C -> C, seeded weight) in both precision modes."""
    cw = (torch.randn(c, c, 3, 3, generator=gen) / (9 * c) ** 0.5).to(DEV)
    x = nhwc(x64.float().to(DEV))
    ops.set_precision("fp32")
    y32 = ops.conv2d(x, cw, None, 1, 1)
    ops.set_precision("bf16")
    ybf = ops.conv2d(x, cw, None, 1, 1)
    return err_of(y32, ybf.float(), "initial_conv bf16 vs fp32")


@pytest.mark.against_definition
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", IB_CASES)
def test_initial_block_kernels_vs_conv_transpose(case, prec, monkeypatch):
    b, l, d, c = case
    assert hb.initial_block_supported(b, l, d, c)
    styles, w, r = ib_inputs(case, prec)
    want = ib_definition(styles, w, r)
    tol = TOL32
    if prec == "bf16":
        dev = bf16_budget(want["forward"], c, torch.Generator().manual_seed(c))
        tol = 2 * dev
        print("case %s: initial_conv bf16-vs-fp32 deviation %.3e -> bf16 tolerance %.3e" % (case, dev, tol))
    ops.set_precision(prec)

    def boom(*a, **k):
        raise AssertionError("the composable (ATen) formula ran for a supported shape")

    monkeypatch.setattr(ops, "_initial_block_composable", boom)
    wp = torch.nn.Parameter(w.to(DEV))  # a Parameter: the bf16 mode reads its packed copy
    fn = lambda s, p: ops.initial_block(s, p)  # noqa: E731
    s_dev, r_dev = styles.to(DEV).requires_grad_(), nhwc(r.to(DEV))
    hb.KERNELS_SEEN.clear()
    got = ib_quantities(fn, s_dev, wp, r_dev)
    hb.timing_kernels()
    x = got["forward"]
    assert x.dtype == ops.act_dtype() and x.is_contiguous(memory_format=torch.channels_last) and tuple(x.shape) == (b, c, 4, 4)
    assert got["d styles"].dtype == torch.float32 and got["d W"].dtype == torch.float32
    worst = {k: err_of(want[k], got[k].float(), "%s %s %s" % (case, prec, k)) for k in want}
    print("case %s %s: worst %s (tol %.3e)" % (case, prec, worst, tol))
    assert all(v <= tol for v in worst.values()), (worst, tol)
    seen = {k for _, k in hb.KERNELS_SEEN}
    assert {"initial_block_fwd_kernel", "initial_block_dgrad_kernel", "initial_block_wgrad_kernel"} <= seen, seen
    if prec == "bf16":
        e = hb.packs.lookup((wp,), "initw")
        assert e is not None and torch.equal(e.value[0], wp.detach().reshape(d, -1).bfloat16())
    # run to run: the same bits
    again = ib_quantities(fn, s_dev, wp, r_dev)
    for k in got:
        assert torch.equal(got[k], again[k]), (case, prec, k)


def guarded(t, band=8192):
    """a copy of `t` (same strides) between two NaN bands of its own allocation"""
    flat = torch.full((t.numel() + 2 * band,), float("nan"), dtype=t.dtype, device=t.device)
    view = flat.as_strided(t.shape, t.stride(), band)
    view.copy_(t)
    return flat, view


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_initial_block_guard_bands_for_the_ragged_d(prec, monkeypatch):
    """D = 514 (not a multiple of 4), B = 3, L = 7, C = 64 with every operand and (STYLEX_POISON=2 mode of hip_backend)
    every result between NaN guard bands: a read before / past a tensor poisons the result, a write lands in a band."""
    case = (3, 7, 514, 64)
    styles, w, r = ib_inputs(case, prec)
    ops.set_precision(prec)
    s_dev, w_dev, r_dev = styles.to(DEV), w.to(DEV), nhwc(r.to(DEV)).to(ops.act_dtype())
    x0 = hb.initial_block_fwd(s_dev, w_dev, hb.F32, ops.act_dtype())
    ds0 = hb.initial_block_bwd_data(r_dev, w_dev, 7, hb.F32)
    dw0 = hb.initial_block_bwd_weight(s_dev, r_dev)
    monkeypatch.setattr(hb, "_POISON", True)
    monkeypatch.setattr(hb, "_GUARD", 8192)
    keep, (s_g, w_g, r_g) = zip(*[guarded(t) for t in (s_dev, w_dev, r_dev)])
    x1 = hb.initial_block_fwd(s_g, w_g, hb.F32, ops.act_dtype())
    ds1 = hb.initial_block_bwd_data(r_g, w_g, 7, hb.F32)
    dw1 = hb.initial_block_bwd_weight(s_g, r_g)
    torch.cuda.synchronize()
    for name, a, b_ in (("forward", x0, x1), ("d styles", ds0, ds1), ("d W", dw0, dw1)):
        assert torch.isfinite(b_.float()).all(), name
        assert torch.equal(a, b_), name
        store = torch.empty(0, dtype=b_.dtype, device=b_.device).set_(b_.untyped_storage())
        assert store.numel() == b_.numel() + 2 * 8192 and b_.storage_offset() == 8192, name
        assert torch.isnan(store[:8192].float()).all() and torch.isnan(store[-8192:].float()).all(), name + ": a guard band was written"
    for flat in keep:
        assert torch.isnan(flat[:8192].float()).all() and torch.isnan(flat[-8192:].float()).all()


def test_unsupported_shapes_take_the_composable_path():
    assert not hb.initial_block_supported(2, 65, 514, 64) and not hb.initial_block_supported(2, 7, 1025, 64)
    assert not hb.initial_block_supported(2, 7, 514, 513) and hb.initial_block_supported(64, 7, 514, 512)
    gen = torch.Generator().manual_seed(1)
    styles = torch.randn(2, 3, 20, generator=gen).to(DEV).requires_grad_()
    w = (torch.randn(20, 520, 4, 4, generator=gen) / 20 ** 0.5).to(DEV).requires_grad_()
    x = ops.initial_block(styles, w)
    assert "_InitialBlock" not in type(x.grad_fn).__name__
    want = F.conv_transpose2d(styles.detach().double().mean(dim=1)[:, :, None, None], w.detach().double())
    assert err_of(want, x.float(), "C = 520 on ATen") <= TOL32
    x.float().sum().backward()
    assert styles.grad is not None and w.grad is not None


# ---- relativistic hinge ----------------------------------------------------------------------------------------------------

def rel_hinge_def(real, fake):
    return (F.relu(1 + (real - fake.mean())) + F.relu(1 - (fake - real.mean()))).mean()


def rel_hinge_inputs(n):
    """seeded logits whose hinge arguments all stay 1e-3 away from the kink in float64 (asserted by the test)"""
    for seed in range(100 + n, 100 + n + 50):
        gen = torch.Generator().manual_seed(seed)
        real, fake = torch.randn(n, generator=gen) * 2, torch.randn(n, generator=gen) * 2
        r64, f64 = real.double(), fake.double()
        margin = min((1 + (r64 - f64.mean())).abs().min().item(), (1 - (f64 - r64.mean())).abs().min().item())
        if margin >= 1e-3:
            return real, fake
    raise AssertionError("no seed with a margin for n = %d" % n)


@pytest.mark.against_definition
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256, 257, 1000])
def test_relativistic_hinge_vs_float64(n, monkeypatch):
    real, fake = rel_hinge_inputs(n)
    r64, f64 = real.double().requires_grad_(), fake.double().requires_grad_()
    args = torch.cat([1 + (r64 - f64.mean()), 1 - (f64 - r64.mean())]).detach()
    assert args.abs().min().item() >= 1e-3, "a hinge argument sits on the kink"
    assert n < 63 or ((args > 0).any() and (args < 0).any()), "both sides of the kink should occur"
    upstream = 0.7
    (rel_hinge_def(r64, f64) * upstream).backward()

    def run():
        r, f = real.to(DEV).requires_grad_(), fake.to(DEV).requires_grad_()
        out = ops.hinge_loss(r, f, True)
        (out * upstream).backward()
        return out, r.grad, f.grad

    out, gr, gf = run()
    assert type(out.grad_fn).__name__ == "_HingeRelBackward"
    worst = [err_of(rel_hinge_def(r64, f64), out, "rel hinge n=%d value" % n), err_of(r64.grad, gr, "rel hinge n=%d d real" % n),
             err_of(f64.grad, gf, "rel hinge n=%d d fake" % n)]
    assert max(worst) <= LOSS_TOL, worst
    out2, gr2, gf2 = run()
    assert torch.equal(out, out2) and torch.equal(gr, gr2) and torch.equal(gf, gf2)
    monkeypatch.setattr(ops, "_FUSED_LOSSES", False)  # the composable expression on the device
    outc, grc, gfc = run()
    assert type(outc.grad_fn).__name__ == "MeanBackward0"
    worst = [err_of(outc, out, "fused vs composable value"), err_of(grc, gr, "fused vs composable d real"),
             err_of(gfc, gf, "fused vs composable d fake")]
    assert max(worst) <= LOSS_TOL, worst


# ---- top-k -----------------------------------------------------------------------------------------------------------------

def topk_cases():
    out = []
    for n in (1, 2, 4, 64, 65, 256, 257, 1024):
        for k in sorted({1, (n + 1) // 2, n - 1, n}):
            if 1 <= k <= n:
                out.append((n, k))
    return out


def run_topk(v, k, upstream):
    x = v.to(DEV).requires_grad_()
    out = ops._TopKMean.apply(x, k)
    (out * upstream).backward()
    return out, x.grad


@pytest.mark.against_definition
@pytest.mark.parametrize("n,k", topk_cases())
def test_top_k_mean_vs_float64(n, k):
    gen = torch.Generator().manual_seed(n * 7 + k)
    upstream = 1.3
    gk = float(np.float32(upstream) / np.float32(k))  # g / k: the correctly rounded fp32 quotient (IEEE division on the host)
    # distinct values
    v = (torch.randperm(n, generator=gen).float() - n / 2) * 0.37 + 0.01
    small, idx = v.double().topk(k, largest=False)
    out, grad = run_topk(v, k, upstream)
    scale = max(1e-3, small.abs().max().item())
    err = abs(out.item() - small.mean().item()) / scale
    print("top-k n=%d k=%d distinct: value err %.3e of %.3e" % (n, k, err, scale))
    assert err <= LOSS_TOL
    want = torch.zeros(n)
    want[idx] = gk
    assert torch.equal(grad.cpu(), want), (grad.cpu() - want).abs().max()
    out2, grad2 = run_topk(v, k, upstream)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    if n < 4:
        return
    # duplicates planted at the k-th smallest value, on both sides of it in index order
    kth = small.max().float()
    at = int((v == kth).nonzero()[0])
    larger = (v > kth).nonzero().reshape(-1)
    plant = [int(i) for i in larger[torch.randperm(len(larger), generator=gen)[:3]]]
    vd = v.clone()
    vd[plant] = kth
    ties = sorted(plant + [at])
    small_d = vd.double().topk(k, largest=False)[0]
    out, grad = run_topk(vd, k, upstream)
    err = abs(out.item() - small_d.mean().item()) / max(1e-3, small_d.abs().max().item())
    print("top-k n=%d k=%d duplicates %s: value err %.3e" % (n, k, ties, err))
    assert err <= LOSS_TOL
    g = grad.cpu()
    nz = g.nonzero().reshape(-1)
    assert len(nz) == k and (g[nz] == gk).all()
    assert (vd[nz] <= kth).all()
    assert abs(g.double().sum().item() - upstream) <= 1e-6 * upstream
    # the documented rule: among the equal values the lower indices are taken
    n_ties_in = int((vd[nz] == kth).sum())
    assert sorted(int(i) for i in nz[vd[nz] == kth]) == ties[:n_ties_in]
    out2, grad2 = run_topk(vd, k, upstream)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)


def test_generator_loss_dispatch():
    v = torch.randn(6, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_()
    assert type(ops.gen_hinge_loss(v, 3).grad_fn).__name__ == "_TopKMeanBackward"
    assert type(ops.gen_hinge_loss(v, 6).grad_fn).__name__ == "_HingeBackward"  # k == n: the plain mean
    assert type(ops.gen_hinge_loss(v).grad_fn).__name__ == "_HingeBackward"
    big = torch.randn(hb.topk_mean_max_n() + 1, generator=torch.Generator().manual_seed(3)).to(DEV).requires_grad_()
    out = ops.gen_hinge_loss(big, 5)  # past the one-block kernel: torch.topk
    assert type(out.grad_fn).__name__ == "MeanBackward0"
    assert abs(out.item() - big.detach().double().topk(5, largest=False)[0].mean().item()) <= 1e-5


# ---- the Trainer on the HIP path ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["steps_no_const", "steps_no_const_pl", "steps_rel_disc", "steps_top_k", "steps_newarch_variants"])
def test_trainer_step_parity_with_variants_gpu(name, tmp_path):
    """The bounds of tests/test_hip_parity.py::test_trainer_step_parity_gpu: call 0 to rtol 2e-4 / atol 2e-5; every call
    inside assert_trajectory's band max(2e-3, 4 x the reference's own spread) capped at 5e-2, with the fixture's 1- vs
    8-thread spread as that spread; parameter statistics with head_atol = calls x 3e-4."""
    g = load_golden(name)
    assert (g["thread_spread"] <= 1e-4).all()
    tr, n = variant_trainer(g, tmp_path, device=torch.device(DEV))
    rows = run_steps(tr, n)
    gold = g["scalars"]
    print(name, "rows", rows, "gold", gold, sep="\n")
    np.testing.assert_allclose(rows[0], gold[0], rtol=2e-4, atol=2e-5, equal_nan=True)
    for k in range(n):
        tol = min(5e-2, max(2e-3, 4.0 * float(g["thread_spread"][k])))
        np.testing.assert_allclose(rows[k], gold[k], rtol=tol, atol=tol, equal_nan=True, err_msg="train() call %d" % k)
    assert_param_stats(tr, g, head_atol=n * 3e-4)


def all_on_trainer(tmp_path, graphs=None):
    g = load_golden("steps_top_k")  # starts at step 1000: k = 2 of 4
    return make_trainer(g, tmp_path, device=torch.device(DEV), trainer_cls=functools.partial(st.Trainer, graphs=graphs, **ALL_ON))


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_two_trainers_with_the_three_options_are_bit_identical(prec, tmp_path):
    """Two identically seeded 3-call Trainers at 32 px with no_const, rel_disc_loss and top_k_training on end with
    bit-identical parameters and scalars.  As in tests/test_attn_gpu.py the frozen networks' MIOpen algorithms are pinned
    and a throw-away Trainer runs first.  In the bf16 mode the cached bf16 copy of the transposed-conv weight must have
    been rewritten by the fused Adam launch: valid for the stepped weight, and equal to its bf16 rounding."""
    prev_det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    ops.set_precision(prec)
    try:
        runs = []
        for i in range(3):
            tr, _ = all_on_trainer(tmp_path / str(i))
            assert tr._generator_top_k() == 2
            rows = run_steps(tr, 1 if i == 0 else 3)
            if i:
                runs.append((rows, {k: v.detach().clone() for k, v in tr.StylEx.named_parameters()}))
            if i == 2 and prec == "bf16":
                w = tr.StylEx.G.to_initial_block.weight
                e = hb.packs.lookup((w,), "initw")
                assert e is not None, "the packed weight copy was not revalidated by the optimiser step"
                assert torch.equal(e.value[0], w.detach().reshape(w.shape[0], -1).bfloat16())
            del tr
    finally:
        ops.set_precision("fp32")
        torch.backends.cudnn.deterministic = prev_det
    print(runs[0][0], runs[1][0], sep="\n")
    assert np.isfinite(runs[0][0][:, :5]).all()
    diff = [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
    assert not diff, diff[:10]
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_path_length_call_with_no_const_stays_on_the_kernels(prec, tmp_path, monkeypatch):
    """steps_no_const_pl, call 0 (gradient penalty and path length): styles -> x -> image is differentiated twice and every
    pass of the initial block is one of the three launches; the ATen formula is never evaluated."""
    def boom(*a, **k):
        raise AssertionError("the composable (ATen) initial block ran inside a supported path-length step")

    monkeypatch.setattr(ops, "_initial_block_composable", boom)
    monkeypatch.setenv("STYLEX_STREAMS", "0")  # one stream while the timing hook counts, as in the kernel-coverage test
    g = load_golden("steps_no_const_pl")
    ops.set_precision(prec)
    try:
        tr, _ = variant_trainer(g, tmp_path, device=torch.device(DEV))
        hb.KERNELS_SEEN.clear()
        hb.timing_enable(1)
        try:
            tr.train()
            torch.cuda.synchronize()
            rows = hb.timing_kernels()
        finally:
            hb.timing_enable(0)
    finally:
        ops.set_precision("fp32")
    launches = {r["kernel"]: r["launches"] for r in rows if r["kernel"].startswith("initial_block")}
    print(prec, launches, "pl_mean", tr.pl_mean)
    # D phase: 1 forward.  G phase: forward; d image / d styles (data gradient); then the backward of the step: through the
    # path-length term (forward + weight gradient of the data-gradient node) and through the image (data + weight gradient)
    assert launches == {"initial_block_fwd_kernel": 3, "initial_block_dgrad_kernel": 2, "initial_block_wgrad_kernel": 2}, launches
    assert tr.pl_mean is not None and math.isfinite(tr.pl_mean) and math.isfinite(tr.g_loss)


def test_graphs_are_refused_with_top_k_training(tmp_path):
    tr, _ = all_on_trainer(tmp_path, graphs=True)
    assert tr.graphs and not tr._graphs_enabled()
    g = load_golden("steps_no_const")
    tr2, _ = make_trainer(g, tmp_path / "b", device=torch.device(DEV),
                          trainer_cls=functools.partial(st.Trainer, graphs=True, no_const=True, rel_disc_loss=True))
    assert tr2._graphs_enabled()


def test_cli_with_the_three_flags_on_gpu_bf16(tmp_path):
    from PIL import Image

    import cli

    data = tmp_path / "imgs"
    data.mkdir()
    rng = np.random.RandomState(0)
    for i in range(8):
        Image.fromarray(rng.randint(0, 255, (40, 48, 3), dtype=np.uint8)).save(data / f"{i}.png")
    try:
        cli.train_from_folder(data=str(data), results_dir=str(tmp_path / "results"), models_dir=str(tmp_path / "models"), name="v",
                              new=True, image_size=32, network_capacity=4, fmap_max=64, batch_size=4, gradient_accumulate_every=2,
                              num_train_steps=4, num_workers=0, save_every=2, evaluate_every=2, tensorboard_dir=None,
                              classifier_path=None, precision="bf16", no_const=True, rel_disc_loss=True, top_k_training=True,
                              generator_top_k_gamma=0.01)
        mdir = tmp_path / "models" / "v"
        assert json.loads((mdir / ".config.json").read_text())["no_const"] is True
        ck = torch.load(mdir / "model_1.pt")
        assert "G.to_initial_block.weight" in ck["StylEx"] and "G.initial_block" not in ck["StylEx"]
        assert all(torch.isfinite(v).all() for v in ck["StylEx"].values() if torch.is_floating_point(v))
        assert "1-from_encoder.png" in os.listdir(tmp_path / "results" / "v")
        # reload through the config file and generate
        tr = st.Trainer(name="v", results_dir=str(tmp_path / "results"), models_dir=str(tmp_path / "models"), image_size=32,
                        tensorboard_dir=None, classifier_path=None, device=torch.device(DEV))
        tr.load(-1)
        assert tr.no_const
        m = tr.StylEx
        m.eval()
        with torch.no_grad():
            w = st.styles_def_to_tensor(st.latent_to_w(m.S, st.noise_list(2, m.G.num_layers, m.G.latent_dim, tr.device)))
            img = m.GE(w, st.image_noise(2, 32, tr.device))
        assert img.shape == (2, 3, 32, 32) and torch.isfinite(img).all()
    finally:
        ops.set_precision("fp32")
