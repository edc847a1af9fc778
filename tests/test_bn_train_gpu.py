"""The kernels of csrc/bn_train.hip against their float64 definitions (tests/_bn_train_defs.py; every bound and its constant
is derived there): statistics with the running update, the fused forward, both backward launches, the cross-entropy.

Shapes (B, C, HW): n = 2; odd HW without 16-byte lanes; C that is no multiple of anything; a channel spread over several
first-stage blocks (HW = 3136: 2 chunks, HW = 12544: 13 chunks, the last one ragged); a 16-byte-able shape behind a pointer that
is not 16-byte aligned.  Inputs N(1, 1) and the shifted 100 + 0.01 N(0, 1).  Integer inputs must give exact sums.  Every
output and workspace sits between NaN guard bands once; every result is the same bits run to run.

With STYLEX_BN_RECORD=<file> the worst error / bound per kernel is appended to that file (profiles/bn_train_errors.txt is the
record of one run)."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.against_definition]

import _bn_train_defs as D  # noqa: E402
import bn_train  # noqa: E402
import hip_backend as hb  # noqa: E402

DEV = torch.device("cuda:0")
EPS = 1e-5
WORST = {}  # kernel quantity -> (worst error / bound, case)


@pytest.fixture(autouse=True)
def need_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    hb.load_library()
    yield


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("STYLEX_BN_RECORD")
    if out and WORST:
        with open(out, "a") as f:
            f.write("# tests/test_bn_train_gpu.py: per quantity the worst observed error / bound over all cases (<= 1 passes) and the case\n"
                    "# that gave it.  Bound = c * 2^-24 * abs_terms with c of tests/_bn_train_defs.py; cross-entropy: 2e-6 * max(1e-3, max |ref|).\n")
            for k in sorted(WORST):
                f.write("%-22s %.4f   %s\n" % (k, WORST[k][0], WORST[k][1]))


def held(name, got, want, c, case):
    """got (fp32, GPU) within c * 2^-24 * abs_terms of want.value, element by element; records the worst ratio."""
    got = got.detach().double().cpu()
    assert got.shape == want.value.shape, (name, got.shape, want.value.shape)
    assert torch.isfinite(got).all(), (name, case)
    bound = c * D.U * want.abs_terms
    err = (got - want.value).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print("%-22s %-40s worst error / bound %.4f" % (name, case, ratio))
    if ratio > WORST.get(name, (-1.0, None))[0]:
        WORST[name] = (ratio, str(case))
    assert (err <= bound).all(), (name, case, ratio)


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    t = D.gen_inputs(shape, kind)
    return t, {k: v.to(DEV) for k, v in t.items()}


def misaligned(t):
    """The same values behind a pointer that is 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


CASES = [(s, k, False) for s in D.SHAPES for k in ("gauss", "shifted")] + [((2, 16, 196), "gauss", True)]
IDS = ["%dx%dx%d-%s%s" % (s + (k, "-misaligned" if m else "")) for s, k, m in CASES]


@pytest.mark.parametrize("shape,kind,mis", CASES, ids=IDS)
@pytest.mark.parametrize("running", [False, True])
def test_stats_against_definition(shape, kind, mis, running):
    cpu, dev = inputs(shape, kind)
    x = misaligned(dev["x"]) if mis else dev["x"]
    case = (shape, kind, "misaligned" if mis else "", "running" if running else "")
    rm, rv = (dev["rm"].clone(), dev["rv"].clone()) if running else (None, None)
    mean, var = hb.bn_stats(x, rm, rv, 0.1)
    m, v = D.mean(cpu["x"]), D.var(cpu["x"])
    held("mean", mean, m, D.C_MEAN, case)
    held("var", var, v, D.C_VAR, case)
    if running:
        n = D.count(cpu["x"])
        bn = torch.nn.BatchNorm2d(shape[1]).double().train()
        bn.running_mean.copy_(cpu["rm"])
        bn.running_var.copy_(cpu["rv"])
        bn(cpu["x"].double())
        want_rm, want_rv = D.running(m, cpu["rm"], 0.1), D.running(v, cpu["rv"], 0.1, n / (n - 1))
        assert torch.allclose(want_rm.value, bn.running_mean, rtol=1e-12, atol=0) and torch.allclose(want_rv.value, bn.running_var, rtol=1e-9, atol=0)
        held("running_mean", rm, D.Sum(bn.running_mean, want_rm.abs_terms), D.C_RUNNING, case)
        held("running_var", rv, D.Sum(bn.running_var, want_rv.abs_terms), D.C_RUNNING, case)
    again = hb.bn_stats(x, None, None, 0.1)
    assert torch.equal(again[0], mean) and torch.equal(again[1], var), case  # run to run, with or without the update


@pytest.mark.parametrize("shape,kind,mis", CASES, ids=IDS)
@pytest.mark.parametrize("act", D.ACTS)
@pytest.mark.parametrize("with_res", [False, True])
def test_forward_and_backward_against_definition(shape, kind, mis, act, with_res):
    cpu, dev = inputs(shape, kind)
    fix = misaligned if mis else (lambda t: t)
    x, gy, res = fix(dev["x"]), fix(dev["gy"]), fix(dev["res"]) if with_res else None
    case = (shape, kind, act, "res" if with_res else "", "misaligned" if mis else "")
    mean, var = hb.bn_stats(x)
    y = hb.bn_act_fwd(x, mean, var, dev["gamma"], dev["beta"], EPS, res, act)
    mu, v = mean.cpu(), var.cpu()
    held("fwd", y, D.bn_act_fwd(cpu["x"], mu, v, cpu["gamma"], cpu["beta"], EPS, cpu["res"] if with_res else None, act), D.C_FWD, case)
    if act == "relu":
        assert (y >= 0).all()
    if act == "relu6":
        assert (y >= 0).all() and (y <= 6).all()
    ysaved = y if act != "none" else None
    dgamma, dbeta = hb.bn_act_bwd_reduce(gy, ysaved, x, mean, var, EPS, act)
    want_db, want_dg = D.bwd_sums(cpu["gy"], y.cpu(), cpu["x"], mu, v, EPS, act)
    held("dbeta", dbeta, want_db, D.C_DBETA, case)
    held("dgamma", dgamma, want_dg, D.C_DGAMMA, case)
    gx, gres = hb.bn_act_bwd_apply(gy, ysaved, x, mean, var, dev["gamma"], dgamma, dbeta, EPS, act, want_gx=True, want_res=with_res)
    want_gx, want_g = D.bwd_apply(cpu["gy"], y.cpu(), cpu["x"], mu, v, cpu["gamma"], dgamma.cpu(), dbeta.cpu(), EPS, act)
    held("gx", gx, want_gx, D.C_APPLY, case)
    if with_res:
        assert torch.equal(gres.cpu().double(), want_g), case  # gy or 0: exact
        only_res = hb.bn_act_bwd_apply(gy, ysaved, None, mean, var, dev["gamma"], dgamma, dbeta, EPS, act, want_gx=False, want_res=True)
        assert only_res[0] is None and torch.equal(only_res[1], gres)
    # run to run: the same bits
    assert torch.equal(hb.bn_act_fwd(x, mean, var, dev["gamma"], dev["beta"], EPS, res, act), y)
    d2 = hb.bn_act_bwd_reduce(gy, ysaved, x, mean, var, EPS, act)
    assert torch.equal(d2[0], dgamma) and torch.equal(d2[1], dbeta)
    assert torch.equal(hb.bn_act_bwd_apply(gy, ysaved, x, mean, var, dev["gamma"], dgamma, dbeta, EPS, act)[0], gx)


@pytest.mark.parametrize("shape", [(3, 5, 49), (2, 16, 196), (8, 3, 12544)])
@pytest.mark.parametrize("act", D.ACTS)
def test_reduce_is_exact_on_integers(shape, act):
    """mean = 0, var = 1 - eps (xhat = x), x and gy in {-3 .. 3}: both sums equal the integer sums."""
    b, c, hw = shape
    h, w = D.HW2[hw]
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (b, c, h, w), generator=g).float()
    gy = torch.randint(-3, 4, (b, c, h, w), generator=g).float()
    y = torch.randint(-2, 9, (b, c, h, w), generator=g).float()  # the gate's input: <= 0, inside (0, 6), 6 and above
    gate = D.gate(y, act).float()
    mean, var = torch.zeros(c), torch.full((c,), 1.0 - EPS)
    dgamma, dbeta = hb.bn_act_bwd_reduce(gy.to(DEV), y.to(DEV), x.to(DEV), mean.to(DEV), var.to(DEV), EPS, act)
    assert torch.equal(dbeta.cpu(), (gy * gate).sum(dim=(0, 2, 3)))
    assert torch.equal(dgamma.cpu(), (gy * gate * x).sum(dim=(0, 2, 3)))


@pytest.mark.parametrize("shape", [(2, 3, 1), (4, 5, 16), (8, 3, 4096), (2, 2, 16384)])
def test_stats_are_exact_on_balanced_integers(shape):
    """n a power of two, every channel holds as many +k as -k: mean exactly 0, variance exactly the mean of k^2."""
    b, c, hw = shape
    n = b * hw
    g = torch.Generator().manual_seed(9)
    k = torch.randint(0, 8, (c, n // 2), generator=g).float()
    vals = torch.cat([k, -k], dim=1)
    vals = torch.stack([row[torch.randperm(n, generator=g)] for row in vals])  # [C, n]
    side = int(round(hw ** 0.5))
    x = vals.view(c, b, hw).permute(1, 0, 2).reshape(b, c, side, hw // side).contiguous()
    mean, var = hb.bn_stats(x.to(DEV))
    assert torch.equal(mean.cpu(), torch.zeros(c))
    assert torch.equal(var.cpu(), (k * k).sum(dim=1) * 2 / n)


def guarded(t, band=8192):
    """a copy of `t` between two NaN bands of its own allocation"""
    flat = torch.full((t.numel() + 2 * band,), float("nan"), dtype=t.dtype, device=t.device)
    view = flat.as_strided(t.shape, t.stride(), band)
    view.copy_(t)
    return flat, view


def bands_intact(t, name):
    store = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())
    assert store.numel() == t.numel() + 2 * 8192 and t.storage_offset() == 8192, name
    assert torch.isnan(store[:8192]).all() and torch.isnan(store[-8192:]).all(), name + ": a guard band was written"


def run_all(t, act):
    mean, var = hb.bn_stats(t["x"], t["rm"], t["rv"], 0.1)
    y = hb.bn_act_fwd(t["x"], mean, var, t["gamma"], t["beta"], EPS, t["res"], act)
    dgamma, dbeta = hb.bn_act_bwd_reduce(t["gy"], y, t["x"], mean, var, EPS, act)
    gx, gres = hb.bn_act_bwd_apply(t["gy"], y, t["x"], mean, var, t["gamma"], dgamma, dbeta, EPS, act, want_res=True)
    return dict(mean=mean, var=var, y=y, dgamma=dgamma, dbeta=dbeta, gx=gx, gres=gres)


@pytest.mark.parametrize("shape", [(3, 24, 49), (2, 16, 196), (5, 7, 3136)])
def test_guard_bands(shape, monkeypatch):
    """Every operand, output and workspace between NaN guard bands (the STYLEX_POISON=2 mode of hip_backend): a read before or
    past a tensor poisons a result, a write lands in a band."""
    _, dev = inputs(shape, "gauss")
    plain = {k: v.clone() for k, v in dev.items()}
    want = run_all(plain, "relu6")
    monkeypatch.setattr(hb, "_POISON", True)
    monkeypatch.setattr(hb, "_GUARD", 8192)
    keep, views = zip(*[guarded(v) for v in dev.values()])
    g = dict(zip(dev.keys(), views))
    got = run_all(g, "relu6")
    z, tg = D.ce_inputs(200, 10)
    (fz, zg), tgt = guarded(z.to(DEV)), tg.to(DEV)
    loss, n_ok = hb.softmax_ce_fwd(zg, tgt)
    gl = hb.softmax_ce_bwd(zg, tgt, torch.ones((), device=DEV))
    torch.cuda.synchronize()
    for name in want:
        assert torch.isfinite(got[name]).all(), name
        assert torch.equal(got[name], want[name]), name
        bands_intact(got[name], name)
    assert torch.equal(g["rm"], plain["rm"]) and torch.equal(g["rv"], plain["rv"])
    for flat in keep + (fz,):
        assert torch.isnan(flat[:8192]).all() and torch.isnan(flat[-8192:]).all()
    monkeypatch.setattr(hb, "_POISON", False)
    monkeypatch.setattr(hb, "_GUARD", 0)
    loss0, n0 = hb.softmax_ce_fwd(z.to(DEV), tgt)
    assert torch.isfinite(loss) and torch.equal(loss, loss0) and torch.equal(n_ok, n0)
    assert torch.equal(gl, hb.softmax_ce_bwd(z.to(DEV), tgt, torch.ones((), device=DEV)))
    bands_intact(gl, "glogits")
    bands_intact(loss, "loss")


def sentinel_guarded(t, band=1024, sentinel=-77):
    """the integer analogue: a copy of `t` between two bands of a sentinel value"""
    flat = torch.full((t.numel() + 2 * band,), sentinel, dtype=t.dtype, device=t.device)
    view = flat[band:band + t.numel()].view(t.shape)
    view.copy_(t)
    return flat, view


@pytest.mark.parametrize("shape", [(3, 24, 49), (5, 7, 3136), (8, 4, 12544)])
def test_workspaces_and_integer_tensors_between_bands(shape):
    """The workspaces, handed in by the caller with exactly the size the query gives: nothing is written past either end, and
    what the kernels read of them they wrote (a NaN-filled workspace gives the results of a fresh one).  The cross-entropy's
    int64 targets and count sit between sentinel bands."""
    _, dev = inputs(shape, "gauss")
    b, c, hw = shape
    lib = hb.load_library()
    nbytes = lib.stylex_bn_train_workspace_bytes(b, c, hw)
    assert nbytes == 2 * c * -(-b * hw // 8192) * 8
    flat, ws = guarded(torch.empty(nbytes // 4, device=DEV))
    ws.fill_(float("nan"))
    mean, var = hb.bn_stats(dev["x"], workspace=ws)
    want = hb.bn_stats(dev["x"])
    assert torch.equal(mean, want[0]) and torch.equal(var, want[1])
    assert torch.isnan(flat[:8192]).all() and torch.isnan(flat[-8192:]).all() and torch.isfinite(ws.view(torch.float64)).all()
    ws.fill_(float("nan"))
    y = hb.bn_act_fwd(dev["x"], mean, var, dev["gamma"], dev["beta"], EPS, None, "relu")
    dgamma, dbeta = hb.bn_act_bwd_reduce(dev["gy"], y, dev["x"], mean, var, EPS, "relu", workspace=ws)
    want = hb.bn_act_bwd_reduce(dev["gy"], y, dev["x"], mean, var, EPS, "relu")
    assert torch.equal(dgamma, want[0]) and torch.equal(dbeta, want[1])
    assert torch.isnan(flat[:8192]).all() and torch.isnan(flat[-8192:]).all() and torch.isfinite(ws.view(torch.float64)).all()
    for bb, kk in ((200, 10), (257, 1000)):
        z, tg = D.ce_inputs(bb, kk)
        (ft, tgt), (fn, cnt) = sentinel_guarded(tg.to(DEV)), sentinel_guarded(torch.zeros((), dtype=torch.int64, device=DEV))
        cflat, cws = guarded(torch.empty(lib.stylex_softmax_ce_workspace_bytes(bb, kk) // 4, device=DEV))
        cws.fill_(float("nan"))
        loss, n_ok = hb.softmax_ce_fwd(z.to(DEV), tgt, workspace=cws, n_correct=cnt)
        grad = hb.softmax_ce_bwd(z.to(DEV), tgt, torch.ones((), device=DEV))
        loss0, n0 = hb.softmax_ce_fwd(z.to(DEV), tg.to(DEV))
        assert n_ok is cnt and torch.equal(loss, loss0) and torch.equal(n_ok, n0)
        assert torch.equal(grad, hb.softmax_ce_bwd(z.to(DEV), tg.to(DEV), torch.ones((), device=DEV)))
        assert torch.isnan(cflat[:8192]).all() and torch.isnan(cflat[-8192:]).all()
        assert (ft[:1024] == -77).all() and (ft[-1024:] == -77).all() and (fn[:1024] == -77).all() and (fn[-1024:] == -77).all()


def ce_ratio(name, got, want, case):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), (name, case)
    ratio = (got - want).abs().max().item() / (D.CE_TOL * max(1e-3, want.abs().max().item()))
    print("%-22s %-40s worst error / bound %.4f" % (name, case, ratio))
    if ratio > WORST.get(name, (-1.0, None))[0]:
        WORST[name] = (ratio, str(case))
    assert ratio <= 1.0, (name, case, ratio)


@pytest.mark.parametrize("b", [1, 3, 200, 257])
@pytest.mark.parametrize("k", [2, 3, 10, 1000])
def test_cross_entropy_against_definition(b, k):
    z, t = D.ce_inputs(b, k)
    zd = z.to(DEV).requires_grad_()
    loss, n_ok = bn_train.softmax_cross_entropy(zd, t.to(DEV), bn_train.every_shape)
    assert type(loss.grad_fn).__name__ == "_SoftmaxCEFnBackward" and not n_ok.requires_grad and n_ok.dtype == torch.int64
    (loss * 1.5).backward()
    want, arg = D.cross_entropy(z, t)
    ce_ratio("ce_loss", loss, want, (b, k))
    ce_ratio("ce_grad", zd.grad, D.cross_entropy_grad(z, t, 1.5), (b, k))
    assert int(n_ok) == int((arg == t).sum())  # the definition's rule: the lowest index on ties
    assert int(n_ok) == int((torch.argmax(z, dim=1) == t).sum())  # torch.argmax on the CPU, every row, the tied ones included
    loss2, n2 = hb.softmax_ce_fwd(zd.detach(), t.to(DEV))
    assert torch.equal(loss2, loss.detach()) and torch.equal(n2, n_ok)
    assert torch.equal(hb.softmax_ce_bwd(zd.detach(), t.to(DEV), torch.full((), 1.5, device=DEV)), zd.grad)


def test_selection_rule_and_module_semantics():
    """BatchNormAct on the GPU: the fused node in training mode on dense fp32 input; the composable formula for eval mode,
    non-dense input, affine=False, momentum=None, and K > 1024 logits; num_batches_tracked as torch; nothing saved when nothing
    needs a gradient; create_graph=True raises."""
    _, dev = inputs((3, 24, 49), "gauss")
    x = dev["x"].clone().requires_grad_()
    m = bn_train.BatchNormAct(24, act="relu6").to(DEV)
    assert m.shape_rule is bn_train.measured_shape_rule and not m.fused(x)  # a small shape: ATen's kernels are faster there
    m.shape_rule = bn_train.every_shape
    ref = torch.nn.BatchNorm2d(24).to(DEV)
    y = m(x, dev["res"])
    assert type(y.grad_fn).__name__ == "_BatchNormActFnBackward"
    want = F.relu6(ref(x.detach()) + dev["res"])
    assert (y - want).abs().max() <= 1e-5 * want.abs().max()
    assert int(m.num_batches_tracked) == 1 == int(ref.num_batches_tracked)
    assert torch.allclose(m.running_mean, ref.running_mean, rtol=1e-5, atol=1e-7) and torch.allclose(m.running_var, ref.running_var, rtol=1e-5)
    with pytest.raises(RuntimeError, match="first-order"):
        torch.autograd.grad(y.sum(), x, create_graph=True)
    for p in m.parameters():
        p.requires_grad_(False)
    y0 = m(dev["x"])
    assert y0.grad_fn is None and not y0.requires_grad and int(m.num_batches_tracked) == 2
    for prepare, arg in ((lambda: m.eval(), x), (lambda: m.train(), x.permute(0, 1, 3, 2)),
                         (lambda: bn_train.BatchNormAct(24, affine=False).to(DEV), x),
                         (lambda: bn_train.BatchNormAct(24, momentum=None).to(DEV), x)):
        mod = prepare()
        mod.shape_rule = bn_train.every_shape
        assert not mod.fused(arg)
        out = mod(arg)
        assert out.grad_fn is not None and "_BatchNormActFn" not in type(out.grad_fn).__name__, (mod, type(out.grad_fn))
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        one = bn_train.BatchNormAct(3).to(DEV)
        one.shape_rule = bn_train.every_shape
        one(torch.zeros(1, 3, 1, 1, device=DEV))
    # the measured rule: the workload shapes the timing record has as wins, and their neighbours that lost
    rule = bn_train.measured_shape_rule
    assert rule(200, 32, 112 * 112, False) and rule(200, 32, 28 * 28, False) and rule(128, 64, 56 * 56, True) and rule(128, 64, 112 * 112, True)
    assert not rule(200, 576, 14 * 14, False) and not rule(200, 160, 49, False) and not rule(128, 128, 28 * 28, True) and not rule(200, 960, 49, True)
    big = bn_train.BatchNormAct(64, act="relu").to(DEV)
    xb = torch.randn(8, 64, 112, 112, device=DEV)
    assert not big.fused(xb) and type(big(xb.clone().requires_grad_()).grad_fn).__name__ != "_BatchNormActFnBackward"  # 6.4 M with a backward
    for p in big.parameters():
        p.requires_grad_(False)
    assert big.fused(xb) and big(xb).grad_fn is None  # forward only: 6.4 M elements at 112 x 112 run on the kernels
    z = torch.randn(4, 1025, device=DEV, requires_grad=True)
    loss, n_ok = bn_train.softmax_cross_entropy(z, torch.tensor([0, 5, 1024, 7], device=DEV), bn_train.every_shape)
    assert "_SoftmaxCEFn" not in type(loss.grad_fn).__name__ and torch.equal(loss.detach(), F.cross_entropy(z.detach(), torch.tensor([0, 5, 1024, 7], device=DEV)))
    z2, t2 = torch.randn(200, 2, device=DEV, requires_grad=True), torch.randint(0, 2, (200,), device=DEV)
    small = bn_train.softmax_cross_entropy(z2, t2)[0]
    assert "_SoftmaxCEFn" not in type(small.grad_fn).__name__  # the measured rule: 200 x 2 is no faster on the kernels
    assert not bn_train.measured_ce_rule(4096, 1000) and bn_train.measured_ce_rule(8192, 1024)  # every measured size: ATen
    big_z = torch.randn(8192, 1024, device=DEV, requires_grad=True)
    assert type(bn_train.softmax_cross_entropy(big_z, torch.randint(0, 1024, (8192,), device=DEV))[0].grad_fn).__name__ == "_SoftmaxCEFnBackward"
