"""-m gpu: the device path of the Frechet Inception Distance — the three entry points of csrc/fid.hip against their
definitions, the fused Inception forward against the same module's plain and fp64 forwards, FIDEvaluator against the
composition it replaces (torch ops, np.cov, scipy's matrix square root) and Trainer.calculate_fid end to end."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

import fid  # noqa: E402
import fid_inception as fi  # noqa: E402
import hip_backend as hb  # noqa: E402

DEV = "cuda:0"
SENTINEL = -12345.0


def _record(lines):
    """Print measured figures, and append them to $STYLEX_PROFILE_DIR/fid_parity.txt where that variable names a folder
    (profiles/fid_parity.txt is the record of one such run)."""
    out = os.environ.get("STYLEX_PROFILE_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "fid_parity.txt"), "a") as f:
            for line in lines:
                f.write(line + "\n")
    for line in lines:
        print(line)


# ---- stylex_fid_moments_acc -----------------------------------------------------------------------------------------------

def _integer_maps(B, D, HW, gen):
    """x [B, D, HW, 1] of small integers whose spatial sums are divisible by HW, and the integer features f = mean."""
    if HW == 1:
        f = torch.randint(-7, 8, (B, D), generator=gen)
        return f.float().view(B, D, 1, 1), f
    f = torch.randint(-4, 5, (B, D), generator=gen)
    a, c = torch.randint(-3, 4, (B, D), generator=gen), torch.randint(-3, 4, (B, D), generator=gen)
    x = torch.stack([f + a, f - a, f + c, f - c], dim=2)  # values in [-7, 7], sum = 4 f
    assert HW == 4 and int(x.abs().max()) <= 7
    return x.float().view(B, D, 2, 2), f


def _fresh_moments(D):
    total = torch.zeros(D, dtype=torch.float64, device=DEV)
    gram = torch.zeros(D, D, dtype=torch.float64, device=DEV)
    gram += torch.tril(torch.full((D, D), SENTINEL, dtype=torch.float64, device=DEV), -1)
    return total, gram


def _check_exact(total, gram, fs):
    f = torch.cat(fs).to(torch.int64)
    D = f.shape[1]
    want_sum, want_gram = f.sum(0), f.T @ f
    assert torch.equal(total.cpu(), want_sum.double())
    got = gram.cpu()
    assert torch.equal(torch.triu(got), torch.triu(want_gram).double())
    low = torch.tril(torch.ones(D, D, dtype=torch.bool), -1)
    assert bool((got[low] == SENTINEL).all()), "the lower triangle was written"


@pytest.mark.parametrize("HW", [1, 4])
@pytest.mark.parametrize("B", [1, 3, 4, 33])
@pytest.mark.parametrize("D", [16, 48])
def test_moments_on_integer_features_bit_for_bit(D, B, HW):
    gen = torch.Generator().manual_seed(1000 * D + 10 * B + HW)
    total, gram = _fresh_moments(D)
    fs = []
    for _ in range(3):  # three accumulating calls
        x, f = _integer_maps(B, D, HW, gen)
        feat = hb.fid_moments_acc(x.to(DEV), total, gram)
        assert torch.equal(feat.cpu(), f.float())
        fs.append(f)
    _check_exact(total, gram, fs)


def test_moments_on_integer_features_full_width():
    gen = torch.Generator().manual_seed(7)
    total, gram = _fresh_moments(2048)
    x, f = _integer_maps(5, 2048, 1, gen)
    hb.fid_moments_acc(x.to(DEV), total, gram)
    _check_exact(total, gram, [f])


@pytest.mark.parametrize("B,D,h,w", [(37, 64, 3, 3), (16, 32, 8, 8)])
def test_moments_on_random_features(B, D, h, w):
    """Products of fp32 values are exact in fp64, so the kernel and numpy differ by the order of n additions only:
    |difference| <= n 2^-52 sum |f_i f_j| per entry."""
    x = torch.randn(B, D, h, w, generator=torch.Generator().manual_seed(B)).to(DEV)
    total, gram = _fresh_moments(D)
    feat = hb.fid_moments_acc(x, total, gram)
    pool_err = float((feat - F.adaptive_avg_pool2d(x, 1).flatten(1)).abs().max())
    f = feat.double().cpu().numpy()
    want, bound = f.T @ f, B * 2.0 ** -52 * (np.abs(f).T @ np.abs(f))
    got = gram.cpu().numpy()
    up = np.triu(np.ones((D, D), dtype=bool))
    gram_err = np.abs(got - want)[up]
    sum_err = np.abs(total.cpu().numpy() - f.sum(0))
    print("B %d D %d HW %d: pooled features vs adaptive_avg_pool2d %.3g; gram error / bound (max) %.3g; sum error / bound %.3g"
          % (B, D, h * w, pool_err, float((gram_err / bound[up]).max()), float((sum_err / (B * 2.0 ** -52 * np.abs(f).sum(0))).max())))
    assert pool_err <= 1e-6
    assert (gram_err <= bound[up]).all()
    assert (sum_err <= B * 2.0 ** -52 * np.abs(f).sum(0)).all()
    assert (got[~up] == SENTINEL).all()
    total2, gram2 = _fresh_moments(D)
    feat2 = hb.fid_moments_acc(x, total2, gram2)
    assert torch.equal(feat, feat2) and torch.equal(total, total2) and torch.equal(gram, gram2)


# ---- stylex_fid_prep ------------------------------------------------------------------------------------------------------

def _prep_composition(x, dtype=torch.float32):
    """The passes the kernel replaces, on the host: save_image's byte, ToTensor's q / 255 (a true division there; ATen's GPU
    kernel multiplies by a rounded reciprocal instead), the bilinear resize, 2 v - 1."""
    q = x.cpu().contiguous().to(dtype).mul(255).add(0.5).clamp(0, 255).floor() / 255
    return 2 * F.interpolate(q, size=(299, 299), mode="bilinear", align_corners=False) - 1


@pytest.mark.parametrize("layout", ["f32_nchw", "bf16_channels_last", "four_channel_view"])
@pytest.mark.parametrize("B,H", [(2, 8), (2, 64), (1, 256), (1, 299), (1, 320)])
def test_prep_against_the_composition(B, H, layout):
    gen = torch.Generator().manual_seed(H)
    if layout == "f32_nchw":
        x = (torch.rand(B, 3, H, H, generator=gen) * 1.2 - 0.1).to(DEV)  # some values outside [0, 1]: the clamp
        ref_in = x
    elif layout == "bf16_channels_last":
        x = (torch.rand(B, 3, H, H, generator=gen) * 1.2 - 0.1).to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
        ref_in = x.float()
    else:  # four channels out of six: only the first three are read (RGBA drops alpha), through the view's strides
        x = (torch.rand(B, 6, H, H, generator=gen) * 1.2 - 0.1).to(DEV)[:, 1:5]
        assert x.shape[1] == 4 and x.storage_offset() > 0 and x.stride(0) == 6 * H * H
        ref_in = x[:, :3]
    got = hb.fid_prep(x)
    want = _prep_composition(ref_in).to(DEV)
    assert got.shape == (B, 3, 299, 299) and got.is_contiguous()
    err = float((got - want).abs().max() / want.abs().max())
    print("prep %s B %d H %d: %.3g of the largest element" % (layout, B, H, err))
    assert err <= 1e-6
    if H == 299:
        assert torch.equal(got, want)


# ---- stylex_affine_act_nchw_slice_fwd -------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(35, 35), (8, 8), (5, 3)])
def test_slice_tail_equals_tail_and_cat(h, w):
    gen = torch.Generator().manual_seed(h)
    widths, B = (8, 20, 4), 3
    xs = [torch.randn(B, c, h, w, generator=gen).to(DEV) for c in widths]
    ss = [(torch.rand(c, generator=gen) + 0.5).to(DEV) for c in widths]
    ts = [torch.randn(c, generator=gen).to(DEV) for c in widths]
    want = torch.cat([hb.affine_act_fwd(x, s, t, relu=True) for x, s, t in zip(xs, ss, ts)], 1)
    out = torch.full((B, sum(widths) + 4, h, w), SENTINEL, dtype=torch.float32, device=DEV)
    c0 = 0
    for x, s, t in zip(xs, ss, ts):
        hb.affine_act_slice_fwd(x, s, t, out, c0, relu=True)
        c0 += x.shape[1]
    assert torch.equal(out[:, :c0], want)
    assert bool((out[:, c0:] == SENTINEL).all())
    lin = torch.empty_like(out)
    hb.affine_act_slice_fwd(xs[1], ss[1], ts[1], lin, 3, relu=False)
    assert torch.equal(lin[:, 3:3 + widths[1]], hb.affine_act_fwd(xs[1], ss[1], ts[1], relu=False))


# ---- the Inception forward ------------------------------------------------------------------------------------------------

def test_inception_device_path_against_plain_and_fp64():
    """The fused forward (library convolutions, folded BatchNorm + ReLU tails, slice writes instead of torch.cat) and the plain
    ATen forward are two fp32 evaluations of one function in different rounding orders: against the fp64 forward the fused
    one may err at most twice as much as the plain one."""
    net = fi.FIDInceptionV3().init_random(5)
    x = torch.rand(2, 3, 299, 299, generator=torch.Generator().manual_seed(3)) * 2 - 1
    with torch.no_grad():
        ref = fi.FIDInceptionV3().init_random(5).double()(x.double()).mean((2, 3))
        gnet = net.to(DEV)
        taps_f, taps_p = {}, {}
        fused = gnet(x.to(DEV), plain=False, taps=taps_f)
        plain = gnet(x.to(DEV), plain=True, taps=taps_p)
    assert fused.shape == plain.shape == (2, 2048, 8, 8)
    err_fused = float((fused.double().mean((2, 3)).cpu() - ref).abs().max())
    err_plain = float((plain.double().mean((2, 3)).cpu() - ref).abs().max())
    _record(["# tests/test_fid_gpu.py::test_inception_device_path_against_plain_and_fp64 (random:5 weights, B = 2): largest "
             "error of a pooled feature against the fp64 CPU forward; largest feature %.4g" % float(ref.abs().max()),
             "inception fused tails + slice writes (device path): %.4g" % err_fused,
             "inception plain ATen forward on the GPU:            %.4g" % err_plain])
    for name in taps_p:  # the blocks agree on the way, too (a wrong slice offset would show here first)
        scale = float(taps_p[name].abs().max())
        assert float((taps_f[name] - taps_p[name]).abs().max()) <= 1e-3 * scale, name
    assert err_fused <= 2 * err_plain


# ---- FIDEvaluator -----------------------------------------------------------------------------------------------------------

class _StandIn(nn.Module):
    """Two conv layers: [B, 3, 299, 299] -> [B, 32, 36, 36]."""

    def __init__(self, seed=11):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.c1, self.c2 = nn.Conv2d(3, 16, 7, 4), nn.Conv2d(16, 32, 3, 2)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / math.sqrt(max(p[0].numel(), 1))))
                p.requires_grad_(False)

    def forward(self, x):
        return F.relu(self.c2(F.relu(self.c1(x))))


def _images(n, size, seed):
    """Images whose bytes do not depend on the precision of x * 255 + 0.5: every value sits in the middle half of its
    quantisation cell."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, (n, 3, size, size), generator=g).float()
    base = torch.rand(n, 3, 1, 1, generator=g) * 0.5 + 0.25  # per-image colour cast: the two sets differ in more than noise
    q = (q * base + torch.randint(0, 64, (n, 3, size, size), generator=g).float()).clamp(0, 255).floor()
    return (q + (torch.rand(n, 3, size, size, generator=g) - 0.5) * 0.5) / 255


def _composition_features(net, x, dtype, device):
    """Pooled features of the composition (torch ops) on `device` in `dtype`, as an fp64 array."""
    with torch.no_grad():
        return net(_prep_composition(x, dtype).to(device)).mean((2, 3)).double().cpu().numpy()


def _scipy_fid(f1, f2):
    from scipy import linalg

    mu1, s1, mu2, s2 = f1.mean(0), np.cov(f1, rowvar=False), f2.mean(0), np.cov(f2, rowvar=False)
    root = linalg.sqrtm(s1.dot(s2))
    return float((mu1 - mu2).dot(mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(np.real(root)))


def test_evaluator_against_the_composition():
    """The reference is the composition in fp64 (host).  The yardstick for "as good as fp32 gets" is the same composition in
    fp32 with its network on the GPU: the device path's convolutions are the GPU library's, whose rounding (algorithm choice
    included) is part of every fp32 evaluation on this device, as in the Inception test above; the host library's fp32
    figure is recorded next to it."""
    pytest.importorskip("scipy.linalg")
    real, fake = _images(64, 32, 1), _images(64, 32, 2)
    f64 = [_composition_features(_StandIn().double(), x, torch.float64, "cpu") for x in (real, fake)]
    f32_gpu = [_composition_features(_StandIn().to(DEV), x, torch.float32, DEV) for x in (real, fake)]
    f32_cpu = [_composition_features(_StandIn(), x, torch.float32, "cpu") for x in (real, fake)]
    want64, want32, want32_cpu = _scipy_fid(*f64), _scipy_fid(*f32_gpu), _scipy_fid(*f32_cpu)
    ev = fid.FIDEvaluator(_StandIn().to(DEV))
    feats = [[], []]
    for i in range(0, 64, 16):  # four batches each: the moments accumulate
        for k, (x, stats) in enumerate(((real, "real"), (fake, "fake"))):
            fm = ev.features(x[i:i + 16].to(DEV))
            if getattr(ev, stats) is None:
                setattr(ev, stats, fid.FIDStats(fm.shape[1], fm.device))
            feats[k].append(getattr(ev, stats).update(fm).double().cpu().numpy())
    got = ev.value()
    assert ev.real.n == ev.fake.n == 64
    ferr = lambda fs: max(float(np.abs(a - b).max()) for a, b in zip(fs, f64))  # noqa: E731
    _record(["# tests/test_fid_gpu.py::test_evaluator_against_the_composition (stand-in net, D = 32, 64 + 64 images at 32 px)",
             "largest pooled-feature error against fp64: device path %.3g; fp32 composition on the GPU %.3g; on the host %.3g"
             % (ferr([np.concatenate(f) for f in feats]), ferr(f32_gpu), ferr(f32_cpu)),
             "FID device path %.12g; composition fp64 %.12g; fp32 on the GPU %.12g; fp32 on the host %.12g"
             % (got, want64, want32, want32_cpu),
             "|device - fp64| = %.4g; |fp32 GPU - fp64| = %.4g (the bound is 10 x this); |fp32 host - fp64| = %.4g"
             % (abs(got - want64), abs(want32 - want64), abs(want32_cpu - want64))])
    assert abs(got - want64) <= 10 * abs(want32 - want64)
    same = fid.FIDEvaluator(ev.net)
    for i in range(0, 64, 16):
        same.add_real(real[i:i + 16].to(DEV))
        same.add_fake(real[i:i + 16].to(DEV))
    print("identical sets: FID %.3g" % same.value())
    assert abs(same.value()) <= 1e-6


# ---- Trainer.calculate_fid ------------------------------------------------------------------------------------------------

class _CountingLoader:
    def __init__(self, batches):
        self.batches, self.taken = batches, 0

    def __iter__(self):
        return self

    def __next__(self):
        self.taken += 1
        return self.batches[(self.taken - 1) % len(self.batches)]


def _trainer(module, tmp_path, name, **kw):
    from lpips_standin import LPIPSStandIn
    from standins import TinyClassifier

    dev = torch.device(DEV)
    tr = module.Trainer(name=name, base_dir=str(tmp_path), image_size=32, network_capacity=4, fmap_max=64, batch_size=8,
                        gradient_accumulate_every=1, classifier=TinyClassifier(seed=99).to(dev),
                        lpips_fn=LPIPSStandIn(seed=4242).to(dev), classifier_name="resnet", evaluate_every=10 ** 9,
                        save_every=10 ** 9, device=dev, tensorboard_dir=None, **kw)
    gen = torch.Generator().manual_seed(5)
    tr.loader = _CountingLoader([torch.rand(8, 3, 32, 32, generator=gen) for _ in range(4)])
    return tr


def test_trainer_calculate_fid(tmp_path):
    import stylex_train as st

    torch.manual_seed(0)
    tr = _trainer(st, tmp_path, "f", fid_weights="random:1", calculate_fid_num_images=16)
    tr.init_StylEx()
    v = tr.calculate_fid(2)
    assert isinstance(v, float) and math.isfinite(v)
    cache = tmp_path / "fid" / "f" / "real_stats.npz"
    assert cache.exists() and tr.loader.taken == 2
    v2 = tr.calculate_fid(2)
    assert math.isfinite(v2) and tr.loader.taken == 2, "the cached real statistics were not reused"
    tr.clear_fid_cache = True
    assert math.isfinite(tr.calculate_fid(2)) and tr.loader.taken == 4
    tr.clear_fid_cache = False
    # a train() call on an FID step appends one line (reference :1497-1503)
    tr.calculate_fid_every, tr.steps = 1, 1
    tr.train()
    lines = (tmp_path / "results" / "f" / "fid_scores.txt").read_text().splitlines()
    assert len(lines) == 1 and lines[0].startswith("1,") and math.isfinite(float(lines[0].split(",")[1]))
    assert tr.last_fid == float(lines[0].split(",")[1])
    # no weights, no number
    bad = _trainer(st, tmp_path, "g", fid_weights=str(tmp_path / "absent_inception.pth"))
    with pytest.raises(FileNotFoundError, match="absent_inception.pth"):
        bad.calculate_fid(2)


def test_trainer_calculate_fid_new_architecture(tmp_path):
    import stylex_train_new as stn

    torch.manual_seed(0)
    tr = _trainer(stn, tmp_path, "n", fid_weights="random:1")
    tr.init_StylEx()
    v = tr.calculate_fid(2)
    assert isinstance(v, float) and math.isfinite(v) and tr.loader.taken == 2


# ---- fid_cli: folder against folder -----------------------------------------------------------------------------------------

def _write_folder(path, n, seed, sizes=((40, 48), (32, 32))):
    from PIL import Image

    path.mkdir()
    rng = np.random.RandomState(seed)
    for i in range(n):
        h, w = sizes[i * len(sizes) // n]  # sorted by name, the files of one size are neighbours: one batch per size
        a = (rng.randint(0, 256, (h, w, 3)) * (0.4 + 0.6 * seed / 3)).astype(np.uint8)
        Image.fromarray(a).save(path / ("%02d.png" % i))
    (path / "notes.txt").write_text("not an image")


def test_fid_cli_folder_against_folder(tmp_path, monkeypatch):
    import fid_cli

    _write_folder(tmp_path / "a", 12, 1)
    _write_folder(tmp_path / "b", 12, 2)
    net, asked = fi.build("random:1", torch.device(DEV)), []
    monkeypatch.setattr(fi, "build", lambda spec, device: asked.append((spec, str(device))) or net)  # one network for both parts
    v = fid_cli.main(["--real", str(tmp_path / "a"), "--fake", str(tmp_path / "b"), "--weights", "random:1", "--batch", "6"])
    assert isinstance(v, float) and math.isfinite(v) and v > 0 and asked == [("random:1", DEV)]
    # the same folder twice, in batches of another size: the two evaluations agree as far as two fp32 forwards do (1e-5 of a
    # feature, profiles/fid_parity.txt), and with 12 images for 2048 features the covariance is rank-deficient, where the
    # matrix square root is only Lipschitz of order 1/2 on the null directions — hence 1e-4 of the traces, not 1e-10
    ev = fid.FIDEvaluator(net)
    fid_cli.add_folder(ev.add_real, str(tmp_path / "a"), 6, torch.device(DEV))
    fid_cli.add_folder(ev.add_fake, str(tmp_path / "a"), 4, torch.device(DEV))
    assert ev.real.n == ev.fake.n == 12
    same, traces = ev.value(), float(np.trace(ev.real.mean_cov()[1]) + np.trace(ev.fake.mean_cov()[1]))
    print("fid_cli: a vs b %.6g; a vs a %.3g; traces %.6g" % (v, same, traces))
    assert abs(same) <= 1e-4 * traces and abs(same) < 1e-2 * v
    with pytest.raises(SystemExit):
        fid_cli.main(["--real", str(tmp_path / "a")])
