"""TEST INFRASTRUCTURE — golden vectors of the linear-attention variant (attn_layers).  Runs only where the reference
source tree is present (STYLEX_REFERENCE): it imports the reference through oracle/ref_shim.py (einops must be
importable) and writes data-only fixtures to tests/golden/:

    attn_ops.npz        ChanNorm / DepthWiseConv2d / LinearAttention in isolation: inputs, parameters, outputs, first-order
                        gradients of a random-weighted sum, and d ||d sum / d x||^2 / d parameters (second order)
    attn_nets_32.npz    seeded-init Generator / DiscriminatorE (as D and as the encoder) with attn_layers=[1, 2]
    steps_attn.npz      4 Trainer.train() calls from step 0        (format of the other steps_* fixtures)
    steps_attn_pl.npz   2 calls from step 5024 (call 0 is a gradient-penalty AND a path-length step)

Both step fixtures are run twice, with 1 and with 8 CPU threads; the per-call spread between the two runs,
max |a - b| / (1 + |b|) over the six scalars (the form of the tests' rtol = atol rule), is stored, and a fixture whose
spread exceeds 1e-4 — a tenth of the 1e-3 the tests assert — is not written.

    python tools/make_golden_attn.py [--only ops,nets,steps,steps_pl]
"""
import argparse
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ATTN = [1, 2]
SPREAD_LIMIT = 1e-4
NETS_SEED = 233  # 232 is refused by the float64 check of gen_nets


def stats(t):
    t = t.detach().double().reshape(-1)
    return np.concatenate([[t.sum().item(), t.abs().sum().item()], t[:8].numpy(), np.zeros(max(0, 8 - t.numel()))])


def save(name, **arrs):
    clean = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        clean[k] = np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **clean)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


def _module_case(out, tag, mod, x, gen):
    """forward, gradients of sum(r * y), and the gradient of ||d sum(r * y) / d x||^2 with respect to the parameters"""
    params = dict(mod.named_parameters())
    for k, v in params.items():
        out["%s/sd/%s" % (tag, k)] = v.detach().clone()
    x = x.clone().requires_grad_()
    y = mod(x)
    r = torch.randn(y.shape, generator=gen)
    out[tag + "/x"], out[tag + "/y"], out[tag + "/r"] = x.detach(), y.detach(), r
    grads = torch.autograd.grad((y * r).sum(), [x] + list(params.values()), allow_unused=True)
    out[tag + "/gx"] = grads[0]
    for k, g_ in zip(params, grads[1:]):
        out["%s/g/%s" % (tag, k)] = torch.zeros_like(params[k]) if g_ is None else g_
    (gx,) = torch.autograd.grad((mod(x) * r).sum(), x, create_graph=True)
    second = torch.autograd.grad(gx.pow(2).sum(), list(params.values()), allow_unused=True)
    for k, g_ in zip(params, second):
        out["%s/gg/%s" % (tag, k)] = torch.zeros_like(params[k]) if g_ is None else g_


def gen_ops(st):
    out = {}
    gen = torch.Generator().manual_seed(51)
    # (B, C, H, W), heads: a ragged H*W (35) with a host width of 16 at the default 8 heads, and a wider case whose
    # attention has 2 heads (the projection weights of two 8-head cases would not fit the size limit of a
    # committed fixture)
    shapes = {"a": (2, 16, 5, 7), "b": (1, 32, 8, 8)}
    heads = {"a": 8, "b": 2}
    for s, shape in shapes.items():
        c = shape[1]
        norm = st.ChanNorm(c)
        with torch.no_grad():
            norm.g.copy_(1 + 0.3 * torch.randn(norm.g.shape, generator=gen))
            norm.b.copy_(0.2 * torch.randn(norm.b.shape, generator=gen))
        _module_case(out, "chan_norm_" + s, norm, torch.randn(shape, generator=gen) * 1.5 + 0.3, gen)
        torch.manual_seed(60 + c)
        _module_case(out, "depthwise_" + s, st.DepthWiseConv2d(c, 2 * c, 3, padding=1, bias=False),
                     torch.randn(shape, generator=gen), gen)
        torch.manual_seed(70 + c)
        att = st.LinearAttention(c, heads=heads[s])
        with torch.no_grad():  # default init keeps the soft-max inputs tiny: widen them so both soft-maxes matter
            att.to_q.weight.mul_(4.0)
            att.to_kv.net[1].weight.mul_(4.0)
            att.to_out.bias.copy_(0.1 * torch.randn(att.to_out.bias.shape, generator=gen))
        _module_case(out, "linattn_" + s, att, torch.randn(shape, generator=gen), gen)
    out["cases"] = np.array(sorted(shapes))
    out["heads"] = np.array([heads[s] for s in sorted(shapes)])
    save("attn_ops", **out)


def _grad_stats(model):
    names, gs = [], []
    for n, p in model.named_parameters():
        if p.grad is not None:
            names.append(n)
            gs.append(stats(p.grad))
    return np.array(names), np.stack(gs)


def _nets_outputs(st, seed, dt):
    size, cap, fmax = 32, 4, 64
    torch.manual_seed(seed)
    m = st.StylEx(image_size=size, network_capacity=cap, fmap_max=fmax, attn_layers=ATTN)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for blk in m.G.blocks:
            for lin in (blk.to_noise1, blk.to_noise2):
                lin.weight.copy_(torch.randn(lin.weight.shape, generator=g) * 0.3)
                lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    sd = m.state_dict()
    out = {"seed": seed, "config": np.array([size, cap, fmax]), "attn_layers": np.array(ATTN),
           "keys": np.array(list(sd.keys())), "shapes": np.array([",".join(map(str, v.shape)) for v in sd.values()]),
           "stats": np.stack([stats(v) for v in sd.values()])}
    w = torch.randn(2, m.G.num_layers, 514, generator=g)
    inoise = torch.rand(2, size, size, 1, generator=g)
    x = torch.rand(2, 3, size, size, generator=g)
    r_rgb = torch.randn(2, 3, size, size, generator=g)
    r_enc = torch.randn(2, 512, generator=g)
    out.update(w=w, inoise=inoise, x=x, r_rgb=r_rgb, r_enc=r_enc)
    m = m.to(dt)
    w, inoise, x, r_rgb, r_enc = (t.to(dt) for t in (w, inoise, x, r_rgb, r_enc))
    # generator: outputs, input and parameter gradients
    wr = w.clone().requires_grad_()
    rgb, coords = m.G(wr, inoise, get_style_coords=True)
    m.G.zero_grad()
    ((rgb * r_rgb).sum() + coords.sum() * 0.01).backward()
    out["rgb"], out["coords"], out["g/grad_w"] = rgb.detach(), coords.detach(), wr.grad
    out["g/grad_names"], out["g/grad_stats"] = _grad_stats(m.G)
    # discriminator and encoder (the same class)
    for tag, net, weight in (("d", m.D, None), ("enc", m.encoder, r_enc)):
        xr = x.clone().requires_grad_()
        y = net(xr)
        net.zero_grad()
        (y.sum() if weight is None else (y * weight).sum()).backward()
        out[tag + "_out"], out[tag + "/grad_x"] = y.detach(), xr.grad
        out[tag + "/grad_names"], out[tag + "/grad_stats"] = _grad_stats(net)
    out["d_of_g"] = m.D(rgb.detach())
    # gradient penalty (double backward through D's attention)
    xr = x.clone().requires_grad_()
    gp = st.gradient_penalty(xr, m.D(xr))
    m.D.zero_grad()
    gp.backward()
    out["gp/value"] = gp.detach()
    out["gp/grad_names"], out["gp/grad_stats"] = _grad_stats(m.D)
    out["gp/grad_fc_w"] = m.D.fc.weight.grad
    # path lengths (double backward through G's attention)
    wr = w.clone().requires_grad_()
    img = m.G(wr, inoise)
    torch.manual_seed(seed + 2)
    pl = st.calc_pl_lengths(wr, img)
    m.G.zero_grad()
    ((pl - 0.3) ** 2).mean().backward()
    out["pl/noise_seed"], out["pl/lengths"], out["pl/grad_w"] = seed + 2, pl.detach(), wr.grad
    out["pl/grad_names"], out["pl/grad_stats"] = _grad_stats(m.G)
    return {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


NETS_TENSOR_LIMIT, NETS_STATS_LIMIT = 2e-6, 1e-5  # a tenth of the bounds the tests assert (2e-5 of the max; 1e-4 of the abs-sum)


def gen_nets(st, seed=232):
    """The float32 run is stored.  A second run in float64 measures the reference's own float32 error on every stored
    result (a LeakyReLU whose input rounds to the other side of zero moves a gradient by far more than a rounding
    error: such a seed is refused here instead of loosening the tests' bound)."""
    a, b = _nets_outputs(st, seed, torch.float32), _nets_outputs(st, seed, torch.float64)
    worst_t = worst_s = 0.0
    for k, v in a.items():
        if isinstance(v, torch.Tensor) and v.dtype == torch.float32 and k not in ("w", "inoise", "x", "r_rgb", "r_enc"):
            ref = b[k].double()
            e = (v.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
            worst_t = max(worst_t, e)
            print("  %-14s float32 vs float64: %.2e" % (k, e))
        elif k.endswith("grad_stats"):
            e = max(np.abs(v[:, :2] - b[k][:, :2]).max(axis=1) / np.maximum(1.0, np.abs(b[k][:, 1])))
            worst_s = max(worst_s, e)
            print("  %-14s float32 vs float64 (checksums): %.2e" % (k, e))
    if worst_t > NETS_TENSOR_LIMIT or worst_s > NETS_STATS_LIMIT:
        raise SystemExit("attn_nets_32, seed %d: the reference's float32 error (%.2e tensors, %.2e checksums) exceeds a "
                         "tenth of the tests' bounds: fixture NOT written" % (seed, worst_t, worst_s))
    a["fp64_spread"] = np.array([worst_t, worst_s])
    save("attn_nets_32", **a)


def _param_stats(model):
    names, st_ = [], []
    for n, p in model.named_parameters():
        names.append(n)
        st_.append(stats(p))
    return np.array(names), np.stack(st_)


def _run_steps(st, n, start, pl0, threads):
    size, cap, fmax, bs, gae = 32, 4, 64, 2, 2
    torch.set_num_threads(threads)
    cls = ref_shim.TinyClassifier(seed=99)
    gd = torch.Generator().manual_seed(7)
    batches = [torch.rand(bs, 3, size, size, generator=gd) for _ in range(8)]
    seed_all(42)
    tr = ref_shim.make_reference_trainer(st, tempfile.mkdtemp(), cls, batches, image_size=size, network_capacity=cap,
                                         fmap_max=fmax, batch_size=bs, gradient_accumulate_every=gae,
                                         alternating_training=True, lr=2e-4, ttur_mult=1.5, rec_scaling=1, kl_scaling=1,
                                         aug_prob=0., attn_layers=ATTN)
    tr.init_StylEx()
    tr.steps = start
    tr.pl_mean = pl0
    rows = []
    for i in range(n):
        tr.train()
        rows.append([tr.d_loss, tr.g_loss, tr.total_rec_loss, tr.total_kl_loss,
                     tr.last_gp_loss if tr.last_gp_loss is not None else np.nan,
                     tr.pl_mean if tr.pl_mean is not None else np.nan])
        print("threads=%d call %d" % (threads, i), rows[-1])
    names, pst = _param_stats(tr.StylEx)
    return np.array(rows, dtype=np.float64), names, pst, (size, cap, fmax, bs, gae)


def gen_steps(st, name, n, start, pl0):
    a, names, pst, (size, cap, fmax, bs, gae) = _run_steps(st, n, start, pl0, 1)
    b = _run_steps(st, n, start, pl0, 8)[0]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    spread = np.nanmax(np.abs(a - b) / (1 + np.abs(b)), axis=1)
    print(name, "1-thread vs 8-thread spread per call:", spread)
    if not (spread <= SPREAD_LIMIT).all():
        raise SystemExit("%s: the reference's own 1- vs 8-thread spread %s exceeds %g: fixture NOT written"
                         % (name, spread, SPREAD_LIMIT))
    save(name, config=np.array([size, cap, fmax, bs, gae, 1, n, start]), pl_mean0=np.nan if pl0 is None else pl0,
         data_seed=7, seed=42, cls_seed=99, lpips_seed=4242, scalars=a, scalars_8_threads=b, thread_spread=spread,
         param_names=names, param_stats=pst, aug_prob=0., attn_layers=np.array(ATTN))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ops,nets,steps,steps_pl")
    ap.add_argument("--nets-seed", type=int, default=NETS_SEED)
    args = ap.parse_args()
    only = args.only.split(",")
    st = ref_shim.import_reference()
    if "ops" in only:
        gen_ops(st)
    if "nets" in only:
        gen_nets(st, args.nets_seed)
    if "steps" in only:
        gen_steps(st, "steps_attn", 4, 0, None)
    if "steps_pl" in only:
        gen_steps(st, "steps_attn_pl", 2, 5024, 0.05)


if __name__ == "__main__":
    main()
