"""attn_layers on the CPU: the composable paths of ops.chan_norm / depthwise_conv3x3 / linear_attention_core and the
modules built on them against vectors captured from the reference (tools/make_golden_attn.py), the seeded init, both
step fixtures through the CPU test double, the checkpoint round trip and AttFind.  Bound for tensors: 2e-5 of the
tensor's max (the suite's fp32 bound; the reference's own float32-vs-float64 spread on these tensors is <= 1.6e-6)."""
import functools
import os

import numpy as np
import pytest
import torch

import attfind
import networks
import ops
import stylex_train as st
from cpu_ops import CpuOracleOps
from conftest import load_golden
from test_host_logic_cpu import assert_param_stats, make_trainer, run_steps
from test_oracle_vs_golden import assert_same_stats, build_nets_model, close_stats, stats

ATTN = [1, 2]
TOL = 2e-5


@pytest.fixture(autouse=True)
def cpu_double():
    prev = ops.use_impl(CpuOracleOps)
    yield
    ops.use_impl(prev)


def close(gold, got, tol=TOL, what=""):
    a = torch.as_tensor(np.asarray(gold)).double()
    b = got.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, a.abs().max().item())
    err = (a - b).abs().max().item()
    print("%s: max err %.3e (scale %.3e)" % (what, err, scale))
    assert err <= tol * scale, "%s: max err %.3e (scale %.3e)" % (what, err, scale)


def build_module(g, tag, kind, case):
    c = g[tag + "/x"].shape[1]
    if kind == "chan_norm":
        mod = networks.ChanNorm(c)
    elif kind == "depthwise":
        mod = networks.DepthWiseConv2d(c, 2 * c, 3, padding=1, bias=False)
    else:
        heads = int(g["heads"][list(g["cases"]).index(case)])
        mod = networks.LinearAttention(c, heads=heads)
    prefix = tag + "/sd/"
    sd = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
    assert set(sd) == set(mod.state_dict()), (sorted(sd), sorted(mod.state_dict()))
    mod.load_state_dict(sd)
    return mod


def check_module_case(g, kind, case, device=None, tol=TOL):
    """forward, first-order gradients and the second-order quantity of one isolated-module case"""
    tag = "%s_%s" % (kind, case)
    mod = build_module(g, tag, kind, case)
    x = torch.from_numpy(g[tag + "/x"])
    r = torch.from_numpy(g[tag + "/r"])
    if device is not None:
        mod, x, r = mod.to(device), x.to(device), r.to(device)
    params = dict(mod.named_parameters())
    x.requires_grad_()
    y = mod(x)
    close(g[tag + "/y"], y, tol, tag + " y")
    grads = torch.autograd.grad((y.float() * r).sum(), [x] + list(params.values()), allow_unused=True)
    close(g[tag + "/gx"], grads[0], tol, tag + " gx")
    for k, got in zip(params, grads[1:]):
        close(g["%s/g/%s" % (tag, k)], torch.zeros_like(params[k]) if got is None else got, tol, tag + " g " + k)
    (gx,) = torch.autograd.grad((mod(x).float() * r).sum(), x, create_graph=True)
    second = torch.autograd.grad(gx.float().pow(2).sum(), list(params.values()), allow_unused=True)
    for k, got in zip(params, second):
        close(g["%s/gg/%s" % (tag, k)], torch.zeros_like(params[k]) if got is None else got, tol, tag + " gg " + k)


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("kind", ["chan_norm", "depthwise", "linattn"])
def test_isolated_modules_vs_reference(kind, case):
    check_module_case(load_golden("attn_ops"), kind, case)


def test_ops_do_not_need_the_implementation_object():
    """the three new ops run on CPU tensors with the product's own (HIP) implementation object installed"""
    ops.use_impl(ops.HipOps)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 16, 4, 4, generator=g)
    assert ops.chan_norm(x, torch.ones(1, 16, 1, 1), torch.zeros(1, 16, 1, 1)).shape == x.shape
    assert ops.depthwise_conv3x3(x, torch.randn(16, 1, 3, 3, generator=g)).shape == x.shape
    q = torch.randn(1, 128, 4, 4, generator=g)
    assert ops.linear_attention_core(q, q, q, 2).shape == q.shape


def attn_model(g, device=None):
    m = build_nets_model(g, cls=functools.partial(st.StylEx, attn_layers=[int(v) for v in g["attn_layers"]],
                                                  **({} if device is None else {"rank": device})))
    return m


def test_state_dict_keys_and_seeded_init():
    g = load_golden("attn_nets_32")
    sd = attn_model(g).state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    for probe in ("G.attns.2.0.fn.fn.to_q.weight", "G.attns.2.0.fn.fn.to_kv.net.0.weight", "G.attns.2.0.fn.fn.to_kv.net.1.weight",
                  "G.attns.2.0.fn.fn.to_out.bias", "G.attns.2.0.fn.norm.g", "G.attns.3.1.fn.fn.0.weight",
                  "G.attns.3.1.fn.fn.2.bias", "G.attns.3.1.fn.norm.b", "D.attn_blocks.0.0.fn.fn.to_out.weight",
                  "encoder.attn_blocks.1.1.fn.fn.2.weight"):
        assert probe in sd, probe
    for i, (k, v) in enumerate(sd.items()):
        assert ",".join(map(str, v.shape)) == str(g["shapes"][i]), k
        assert_same_stats(g["stats"][i], stats(v), k)


def check_grad_stats(model, names, gold, tol=1e-4):
    """Every gradient the reference produced, by checksum.  A gradient that is structurally zero (a bias behind the last
    attention block in the gradient penalty) is a zero tensor in the reference and may be absent here; nothing else may
    be absent, and nothing may have a gradient that the reference does not."""
    params = dict(model.named_parameters())
    names = [str(n) for n in names]
    extra = [n for n, p in model.named_parameters() if p.grad is not None and n not in names]
    assert not extra, extra
    for n, gs in zip(names, gold):
        if params[n].grad is None:
            assert gs[1] == 0.0, "%s has no gradient, the reference's has abs-sum %g" % (n, gs[1])
        else:
            close_stats(gs, params[n].grad.detach().cpu(), tol)


def check_nets(g, m, device=None, tol=TOL, stat_tol=1e-4):
    """outputs, gradients, gradient penalty and path lengths of the attention networks against attn_nets_32"""
    dev = device or torch.device("cpu")
    w, inoise, x, r_rgb, r_enc = (torch.from_numpy(g[n]).to(dev) for n in ("w", "inoise", "x", "r_rgb", "r_enc"))
    wr = w.clone().requires_grad_()
    rgb, coords = m.G(wr, inoise, get_style_coords=True)
    close(g["rgb"], rgb, tol, "rgb")
    close(g["coords"], coords, tol, "coords")
    m.G.zero_grad()
    ((rgb * r_rgb).sum() + coords.sum() * 0.01).backward()
    close(g["g/grad_w"], wr.grad, tol, "g/grad_w")
    check_grad_stats(m.G, g["g/grad_names"], g["g/grad_stats"], stat_tol)
    for tag, net, weight in (("d", m.D, None), ("enc", m.encoder, r_enc)):
        xr = x.clone().requires_grad_()
        y = net(xr)
        close(g[tag + "_out"], y, tol, tag + "_out")
        net.zero_grad()
        (y.sum() if weight is None else (y * weight).sum()).backward()
        close(g[tag + "/grad_x"], xr.grad, tol, tag + "/grad_x")
        check_grad_stats(net, g[tag + "/grad_names"], g[tag + "/grad_stats"], stat_tol)
    close(g["d_of_g"], m.D(rgb.detach()), tol, "d_of_g")
    xr = x.clone().requires_grad_()
    gp = st.gradient_penalty(xr, m.D(xr))
    close(g["gp/value"], gp, tol, "gp/value")
    m.D.zero_grad()
    gp.backward()
    close(g["gp/grad_fc_w"], m.D.fc.weight.grad, 1e-4, "gp/grad_fc_w")
    check_grad_stats(m.D, g["gp/grad_names"], g["gp/grad_stats"], stat_tol)
    wr = w.clone().requires_grad_()
    img = m.G(wr, inoise)
    torch.manual_seed(int(g["pl/noise_seed"]))
    pl = st.calc_pl_lengths(wr, img)
    close(g["pl/lengths"], pl, tol, "pl/lengths")
    m.G.zero_grad()
    ((pl - 0.3) ** 2).mean().backward()
    close(g["pl/grad_w"], wr.grad, tol, "pl/grad_w")
    check_grad_stats(m.G, g["pl/grad_names"], g["pl/grad_stats"], stat_tol)


def test_networks_vs_reference():
    g = load_golden("attn_nets_32")
    check_nets(g, attn_model(g))


def check_steps(name, tmp_path, device=None):
    g = load_golden(name)
    assert (g["thread_spread"] <= 1e-4).all()  # the reference against itself, a tenth of the bound below
    tr, n = make_trainer(g, tmp_path, device=device, trainer_cls=functools.partial(st.Trainer, attn_layers=ATTN))
    rows = run_steps(tr, n)
    gold = g["scalars"]
    print(name, "rows", rows, "gold", gold, sep="\n")
    np.testing.assert_allclose(rows[0], gold[0], rtol=5e-5, atol=5e-6, equal_nan=True)
    np.testing.assert_allclose(rows, gold, rtol=1e-3, atol=1e-3, equal_nan=True)
    assert_param_stats(tr, g)
    return tr


@pytest.mark.parametrize("name", ["steps_attn", "steps_attn_pl"])
def test_trainer_step_parity_with_attention_cpu(name, tmp_path):
    check_steps(name, tmp_path)


def test_checkpoint_round_trip_with_attention(tmp_path):
    g = load_golden("steps_attn")
    tr, _ = make_trainer(g, tmp_path, trainer_cls=functools.partial(st.Trainer, attn_layers=ATTN))
    del tr.save  # make_trainer stubs it out
    tr.train()
    tr.save(0)
    want = {k: v.clone() for k, v in tr.StylEx.state_dict().items()}
    tr2 = st.Trainer(name="t", base_dir=str(tmp_path), image_size=8, classifier=tr.classifier, lpips_fn=tr.lpips_fn,
                     classifier_name="resnet")  # the configuration comes from the saved config file
    tr2.load(0)
    assert tr2.attn_layers == ATTN and tr2.image_size == 32
    got = tr2.StylEx.state_dict()
    assert list(got) == list(want)
    for k in want:
        assert torch.equal(got[k].cpu(), want[k].cpu()), k


def test_attfind_with_attention_equals_unbatched_generator_forwards():
    """16 px model with attention: every coordinate's perturbed image from the batched prefix / suffix walk equals a
    plain G(...) forward with the block's style bias moved (what the reference notebook does)."""
    torch.manual_seed(5)
    m = st.StylEx(16, network_capacity=4, fmap_max=32, attn_layers=ATTN)
    G = m.G
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in G.parameters():  # leave the zero-initialised noise maps and the unit ChanNorm gains non-trivial
            if p.abs().sum() == 0 or (p == 1).all():
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
        w = torch.randn(1, 514, generator=gen)
        noise = torch.rand(1, 16, 16, 1, generator=gen)
        w_tensor = attfind.styles_def_to_tensor([(w, G.num_layers)])
        states = attfind._prefix_states(G, w_tensor, noise)
        for k, block in enumerate(G.blocks):
            x_k, rgb_k, s1, s2 = states[k]
            for coord in range(block.num_style_coords):
                d1, d2 = torch.zeros_like(s1), torch.zeros_like(s2)
                (d1 if coord < block.input_channels else d2)[0, coord % block.input_channels if coord < block.input_channels
                                                             else coord - block.input_channels] = 0.7
                got = attfind._suffix(G, k, x_k, rgb_k, w_tensor, noise, (s1 + d1, s2 + d2))
                lin = block.to_style1 if coord < block.input_channels else block.to_style2
                j = coord if coord < block.input_channels else coord - block.input_channels
                lin.bias[j] += 0.7
                want = G(w_tensor, noise)
                lin.bias[j] -= 0.7
                assert (got - want).abs().max().item() <= 1e-5, (k, coord)
