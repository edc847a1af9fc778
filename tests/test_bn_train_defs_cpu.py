"""tests/_bn_train_defs.py against torch: the float64 definitions are F.batch_norm / F.cross_entropy and what autograd derives
from them; and the bounds c * 2^-24 * abs_terms have teeth on the GPU test's own inputs (a definition that loses ONE element
of a channel lands outside them; an fp32 E[x^2] - mean^2 lands outside the variance bound on the shifted input)."""
import pytest
import torch
import torch.nn.functional as F

import _bn_train_defs as D

F64 = torch.float64
EPS = 1e-5
SMALL = [s for s in D.SHAPES if s[0] * s[1] * s[2] <= 20000]


def close(a, b, tol=1e-11):
    assert a.shape == b.shape, (a.shape, b.shape)
    err, scale = float((a - b).abs().max()), max(1e-30, float(b.abs().max()))
    assert err <= tol * scale, (err, scale)


def torch_act(v, act):
    return {"none": lambda t: t, "relu": F.relu, "relu6": F.relu6}[act](v)


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("kind", ["gauss", "shifted"])
def test_statistics_and_running_update_are_batch_norm(shape, kind):
    t = D.gen_inputs(shape, kind)
    x = t["x"].double()
    rm, rv = t["rm"].double(), t["rv"].double()
    F.batch_norm(x, rm, rv, None, None, True, 0.1, EPS)
    n = D.count(x)
    close(D.mean(x).value, x.mean(dim=(0, 2, 3)))
    close(D.var(x).value, x.var(dim=(0, 2, 3), unbiased=False), 1e-9)
    close(D.running(D.mean(x), t["rm"], 0.1).value, rm)
    close(D.running(D.var(x), t["rv"], 0.1, n / (n - 1)).value, rv, 1e-9)


@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("act", D.ACTS)
@pytest.mark.parametrize("with_res", [False, True])
def test_forward_and_backward_are_batch_norm_under_autograd(shape, act, with_res):
    t = D.gen_inputs(shape, "gauss")
    x, gamma, beta = (t[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    res = t["res"].double().requires_grad_() if with_res else None
    out = F.batch_norm(x, None, None, gamma, beta, True, 0.1, EPS)
    y = torch_act(out if res is None else out + res, act)
    gy = t["gy"].double()
    y.backward(gy)
    mu, v = D.mean(t["x"]).value, D.var(t["x"]).value
    close(D.bn_act_fwd(t["x"], mu, v, t["gamma"], t["beta"], EPS, t["res"] if with_res else None, act).value, y.detach(), 1e-9)
    dbeta, dgamma = D.bwd_sums(gy, y.detach(), t["x"], mu, v, EPS, act)
    close(dbeta.value, beta.grad, 1e-9)
    close(dgamma.value, gamma.grad, 1e-8)
    gx, gres = D.bwd_apply(gy, y.detach(), t["x"], mu, v, t["gamma"], dgamma.value, dbeta.value, EPS, act)
    close(gx.value, x.grad, 1e-7)
    if with_res:
        assert torch.equal(gres, res.grad)
    assert (gx.abs_terms >= gx.value.abs() * (1 - 1e-12)).all() and (dgamma.abs_terms >= dgamma.value.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("b,k", [(1, 2), (3, 3), (200, 10), (257, 1000)])
def test_cross_entropy_definition(b, k):
    z, t = D.ce_inputs(b, k)
    zd = z.double().requires_grad_()
    want = F.cross_entropy(zd, t)
    want.backward()
    loss, arg = D.cross_entropy(z, t)
    close(loss, want.detach())
    close(D.cross_entropy_grad(z, t), zd.grad, 1e-9)
    ties = (z == z.max(dim=1, keepdim=True).values).sum(dim=1) > 1
    assert torch.equal(arg[~ties], torch.argmax(z, dim=1)[~ties])
    if b > 2 and k > 2:
        assert ties[1] and ties[2] and arg[1] == 0 and arg[2] == 1


def test_bounds_notice_one_dropped_element():
    """Over the channels of every GPU shape (N(1, 1) inputs): the mean, the variance and both backward sums of a channel that
    lost its middle element are outside c * 2^-24 * abs_terms in at least 95 % of the channels."""
    moved = {"mean": [], "var": [], "dbeta": [], "dgamma": []}
    for shape in D.SHAPES:
        t = D.gen_inputs(shape, "gauss")
        x, gy = t["x"].double(), t["gy"].double()
        b, c, h, w = x.shape
        n = D.count(x)
        keep = torch.ones(b, 1, h, w, dtype=F64)
        keep[b // 2, 0, h // 2, w // 2] = 0
        m, v = D.mean(x), D.var(x)
        m_drop = (x * keep).sum(dim=(0, 2, 3)) / (n - 1)
        v_drop = (((x - m_drop.view(1, -1, 1, 1)) ** 2) * keep).sum(dim=(0, 2, 3)) / (n - 1)
        moved["mean"].append((m_drop - m.value).abs() > D.C_MEAN * D.U * m.abs_terms)
        moved["var"].append((v_drop - v.value).abs() > D.C_VAR * D.U * v.abs_terms)
        full = D.bwd_sums(gy, None, x, m.value, v.value, EPS)
        drop = D.bwd_sums(gy, None, x, m.value, v.value, EPS, keep=keep)
        moved["dbeta"].append((drop[0].value - full[0].value).abs() > D.C_DBETA * D.U * full[0].abs_terms)
        moved["dgamma"].append((drop[1].value - full[1].value).abs() > D.C_DGAMMA * D.U * full[1].abs_terms)
    for name, flags in moved.items():
        frac = torch.cat(flags).double().mean().item()
        print("%-7s moved outside the bound in %.1f %% of %d channels" % (name, 100 * frac, torch.cat(flags).numel()))
        assert frac >= 0.95, (name, frac)


def test_variance_bound_rejects_the_uncentred_fp32_formula():
    """x = 100 + 0.01 N(0, 1): E[x^2] - mean^2 evaluated in fp32 misses the variance bound (in every channel of every shape)."""
    for shape in D.SHAPES:
        x = D.gen_inputs(shape, "shifted")["x"]
        v = D.var(x)
        naive = (x * x).mean(dim=(0, 2, 3)) - x.mean(dim=(0, 2, 3)) ** 2
        assert naive.dtype == torch.float32
        bad = (naive.double() - v.value).abs() > D.C_VAR * D.U * v.abs_terms
        assert bad.all(), (shape, naive, v.value)
