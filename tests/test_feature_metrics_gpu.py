"""The pairwise feature-metric kernels (csrc/feature_metrics.hip) and fid.kid / fid.precision_recall on the GPU against
their fp64 definitions (tests/_feature_metrics_defs.py): bit for bit on integer operands, per element within the derived
bounds on real-valued ones (flags equal, no column left out), run to run, between NaN guard bands; then the evaluator, the
Trainer and the command line.  The worst observed errors against their bounds are written to
$STYLEX_PROFILE_DIR/feature_metrics_errors.txt where that variable names a folder (profiles/feature_metrics_errors.txt is
the record of one such run)."""
import functools
import math
import os
import random

import numpy as np
import pytest
import torch

import _feature_metrics_defs as fd
import fid
import hip_backend as hb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.cpu().numpy()


def _worst(what, err, bound):
    """Record the largest err / bound of `what`; the assertion is the caller's."""
    ratio = float(np.max(np.asarray(err) / np.maximum(np.asarray(bound), 1e-300)))
    cur = WORST.get(what)
    if cur is None or ratio > cur[0]:
        WORST[what] = (ratio, float(np.max(err)), float(np.max(bound)))
    out = os.environ.get("STYLEX_PROFILE_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "feature_metrics_errors.txt"), "w") as f:
            f.write("# worst observed error against its bound, tests/test_feature_metrics_gpu.py (error / bound, largest error, largest bound)\n")
            for k in sorted(WORST):
                f.write("%-44s %.3g  %.3g  %.3g\n" % ((k,) + WORST[k]))


def blocks_of(n, rows):
    return [(r0, min(rows, n - r0)) for r0 in range(0, n, rows)]


def gpu_dist2(x, y, rows):
    """The whole matrix from row blocks of `rows` rows (tests only: the product never holds it)."""
    xd, yd = dev(x), dev(y)
    nx, ny = hb.feat_rownorm(xd), hb.feat_rownorm(yd)
    return torch.cat([hb.feat_dist2_block(xd, yd, nx, ny, r0, r) for r0, r in blocks_of(len(x), rows)]), nx, ny


def gpu_radii2(x, k, rows):
    xd = dev(x)
    nx = hb.feat_rownorm(xd)
    return torch.cat([hb.feat_row_kth(hb.feat_dist2_block(xd, xd, nx, nx, r0, r), k, self0=r0) for r0, r in blocks_of(len(x), rows)])


def gpu_inside(ref, q, k, rows):
    rd, qd = dev(ref), dev(q)
    nr, nq = hb.feat_rownorm(rd), hb.feat_rownorm(qd)
    r2 = gpu_radii2(ref, k, rows)
    flags = torch.zeros(len(q), dtype=torch.uint8, device=DEV)
    for r0, r in blocks_of(len(ref), rows):
        hb.feat_col_any(hb.feat_dist2_block(rd, qd, nr, nq, r0, r), r2, r0, flags)
    return flags


INT_CASES = [(n, m, d) for d in (16, 64) for n, m in fd.INT_SHAPES] + [(17, 33, 2048)]


# ---- bit for bit on integer operands -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,d", INT_CASES)
def test_poly_sums_are_exact_on_integers(n, m, d):
    """Entries in {0..3}, D a power of two: dot / D + 1, its cube and every partial sum are exact in fp64 in any order."""
    x, y = fd.integer_features(n, m, d)
    assert fd.poly(x, y).sum() * d ** 3 < 2.0 ** 53
    xd, yd = dev(x), dev(y)
    for a, b, ad, bd, sym in ((x, y, xd, yd, False), (x, x, xd, xd, True), (y, y, yd, yd, True), (x, x, xd, xd, False)):
        got = hb.feat_poly_sum(ad, bd, symmetric=sym)
        assert torch.equal(got.cpu(), torch.tensor([fd.poly_sum(a, b, sym)], dtype=torch.float64)), (n, m, d, sym)


@pytest.mark.parametrize("n,m,d", INT_CASES)
def test_distances_radii_and_flags_are_exact_on_integers(n, m, d):
    x, y = fd.integer_features(n, m, d)
    want = fd.dist2(x, y)
    assert (want == 0).any(), "the copied rows give distance exactly 0"
    for rows in sorted({16, 17, n}):
        got, nx, ny = gpu_dist2(x, y, rows)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (n, m, d, rows)
        assert torch.equal(nx.cpu(), torch.from_numpy(fd.model_rownorm(x))) and torch.equal(ny.cpu(), torch.from_numpy(fd.model_rownorm(y)))
    if n < 2:
        return
    for k in sorted({1, min(3, n - 1), min(8, n - 1)}):
        r2 = fd.radii2(x, k)
        flags = fd.inside(x, y, k)
        if (n, m, k) in ((17, 33, 3), (48, 31, 3)) and d <= 64:
            ties = int((want == r2[:, None]).sum())
            print("(%d, %d, %d): %d pairs exactly at their radius" % (n, m, d, ties))
            assert ties >= 10, "exact ties at the radius are what <= against < is tested on"
        for rows in sorted({16, 17, n}):
            assert torch.equal(gpu_radii2(x, k, rows).cpu(), torch.from_numpy(r2)), (n, m, d, k, rows)
            assert torch.equal(gpu_inside(x, y, k, rows).cpu(), torch.from_numpy(flags)), (n, m, d, k, rows)


# ---- per element on real-valued operands ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def real_case(n, m, d):
    x, y = fd.real_features(n, m, d)
    return x, y  # shared: nobody writes to them


@functools.lru_cache(maxsize=None)
def real_definition(n, m, d, k):
    x, y = real_case(n, m, d)
    return fd.inside(x, y, k), fd.inside(y, x, k), fd.undecided_pairs(x, y, k) + fd.undecided_pairs(y, x, k)


@pytest.mark.parametrize("n,m,d", fd.REAL_SHAPES)
def test_distances_radii_and_flags_within_their_bounds(n, m, d):
    x, y = real_case(n, m, d)
    want, bound = fd.dist2(x, y), fd.dist2_bound(x, y)
    for rows in (16, 17, n):
        got, _, _ = gpu_dist2(x, y, rows)
        err = np.abs(host(got) - want)
        _worst("dist2 (%d, %d, %d)" % (n, m, d), err, bound)
        assert (err <= bound).all(), (rows, float((err / bound).max()))
    r2, rb = fd.radii2(x, 3), fd.radius_bound(x)
    err = np.abs(host(gpu_radii2(x, 3, 16)) - r2)
    _worst("radius (%d, %d, %d)" % (n, m, d), err, rb)
    assert (err <= rb).all(), float((err / rb).max())
    p_flags, r_flags, undecided = real_definition(n, m, d, 3)
    assert undecided == 0, "the inputs must leave no pair within the bounds of its radius: every flag is decided"
    for flags in (p_flags, r_flags):
        assert 0.05 <= flags.mean() <= 0.95, "both flag values must occur (%.2f)" % flags.mean()
    print("(%d, %d, %d): precision %.2f recall %.2f in the definition" % (n, m, d, p_flags.mean(), r_flags.mean()))
    for rows in (16, 64, n):
        assert torch.equal(gpu_inside(x, y, 3, rows).cpu(), torch.from_numpy(p_flags)), rows
        assert torch.equal(gpu_inside(y, x, 3, rows).cpu(), torch.from_numpy(r_flags)), rows


def _tile_sums(k):
    n, m = k.shape
    pad = np.zeros(((n + 15) // 16 * 16, (m + 15) // 16 * 16))
    pad[:n, :m] = k
    return pad.reshape(pad.shape[0] // 16, 16, pad.shape[1] // 16, 16).sum((1, 3))


@pytest.mark.parametrize("n,m,d", fd.REAL_SHAPES)
def test_poly_tile_sums_and_totals_within_their_bounds(n, m, d):
    x, y = real_case(n, m, d)
    for a, b, sym in ((x, y, False), (x, x, True), (y, y, True)):
        k = fd.poly(a, b)
        if sym:
            np.fill_diagonal(k, 0.0)
        # poly_sum_bound on the pairs of one tile / of the whole: entry bounds plus (number of pairs) u sum |k|
        entry = fd.poly_entry_bound(a, b)
        tile_bound = _tile_sums(entry) + 256 * fd.U * _tile_sums(np.abs(k))
        ws = torch.empty(hb.feat_poly_tiles(len(a), len(b)), dtype=torch.float64, device=DEV)
        got = hb.feat_poly_sum(dev(a), dev(b), symmetric=sym, ws=ws)
        terr = np.abs(host(ws).reshape(tile_bound.shape) - _tile_sums(k))
        _worst("poly tile sum (%d, %d, %d)" % (n, m, d), terr, tile_bound)
        assert (terr <= tile_bound).all(), float((terr / tile_bound).max())
        err, bound = abs(float(got.cpu()[0]) - float(k.sum())), fd.poly_sum_bound(a, b)
        _worst("poly total (%d, %d, %d)" % (n, m, d), err, bound)
        assert err <= bound, (err, bound)


# ---- fid.kid -------------------------------------------------------------------------------------------------------------

def test_kid_against_the_definition():
    """n = 300, m = 280, D = 64, 5 subsets of 100.  Per subset the three sums are within B_xx, B_yy, B_xy (poly_sum_bound), so
    MMD^2 is within (B_xx + B_yy) / (s (s - 1)) + 2 B_xy / s^2 plus the host's own four roundings of the same expression,
    4 u (|S_xx| + |S_yy|) / (s (s - 1)) + 8 u |S_xy| / s^2; the mean moves by at most the mean of these, the standard
    deviation (a norm of the centred values over sqrt(q)) by at most the largest — 8.8e-12 and 9.0e-12 here (KID 0.577 +- 0.182), plus 8 u of the
    values for the two reductions."""
    x, y = fd.real_features(300, 280, 64, seed=3)
    subsets = fd.draw_subsets(300, 280, 5, 100, seed=11)
    want_mean, want_std = fd.kid(x, y, subsets)
    got_mean, got_std = fid.kid(dev(x), dev(y), subsets=subsets)
    s, per = 100, []
    for ix, iy in subsets:
        a, b = x[ix], y[iy]
        sxx, syy, sxy = abs(fd.poly_sum(a, a, True)), abs(fd.poly_sum(b, b, True)), abs(fd.poly_sum(a, b))
        per.append((fd.poly_sum_bound(a, a) + fd.poly_sum_bound(b, b)) / (s * (s - 1)) + 2 * fd.poly_sum_bound(a, b) / (s * s)
                   + 4 * fd.U * (sxx + syy) / (s * (s - 1)) + 8 * fd.U * sxy / (s * s))
    slack = 8 * fd.U * (abs(want_mean) + want_std)
    mean_bound, std_bound = float(np.mean(per)) + slack, float(np.max(per)) + slack
    print("KID %.12g +- %.12g (definition %.12g +- %.12g); propagated bounds %.3g, %.3g"
          % (got_mean, got_std, want_mean, want_std, mean_bound, std_bound))
    _worst("kid mean (300, 280, 64)", abs(got_mean - want_mean), mean_bound)
    _worst("kid std (300, 280, 64)", abs(got_std - want_std), std_bound)
    assert want_std > 1e3 * std_bound, "the subsets must differ by far more than the bound"
    assert abs(got_mean - want_mean) <= mean_bound and abs(got_std - want_std) <= std_bound
    # drawn subsets: the definition's generator, defaults clipped to the set sizes
    assert fid.kid(dev(x), dev(y), num_subsets=5, max_subset_size=100, seed=11) == (got_mean, got_std)


def test_kid_of_a_set_with_itself_is_exact_on_integers():
    x, _ = fd.integer_features(48, 31, 64)
    rng = np.random.RandomState(1)
    subsets = [(rng.permutation(48)[:40], rng.permutation(48)[:40])]
    want = fd.kid(x, x, subsets)
    assert fid.kid(dev(x), dev(x), subsets=subsets) == want and want[1] == 0.0
    both = [(np.arange(48), np.arange(48))]
    assert fid.kid(dev(x), dev(x), subsets=both) == fd.kid(x, x, both)


# ---- fid.precision_recall ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("row_block", [16, 64, 1024])
@pytest.mark.parametrize("n,m,d", fd.REAL_SHAPES)
def test_precision_recall_equals_the_definition(n, m, d, row_block, k):
    x, y = real_case(n, m, d)
    p_flags, r_flags, undecided = real_definition(n, m, d, k)
    assert undecided == 0
    got = fid.precision_recall(dev(x), dev(y), k=k, row_block=row_block)
    assert got == (float(p_flags.mean()), float(r_flags.mean())), (got, p_flags.mean(), r_flags.mean())


def test_precision_recall_with_too_few_points_is_an_error():
    x, y = real_case(17, 33, 16)
    with pytest.raises(hb.StylexHipError):
        fid.precision_recall(dev(x[:3]), dev(y), k=3)
    with pytest.raises(hb.StylexHipError):
        fid.precision_recall(dev(x), dev(y[:8]), k=8)
    with pytest.raises(hb.StylexHipError):
        fid.precision_recall(dev(x), dev(y), k=9)
    xd = dev(x)
    nx = hb.feat_rownorm(xd)
    blk = hb.feat_dist2_block(xd, xd[:3].contiguous(), nx, nx[:3].contiguous(), 0, 3)
    with pytest.raises(hb.StylexHipError):  # the entry point itself: 3 columns, one left out, k = 3
        hb.feat_row_kth(blk, 3, self0=0)
    assert hb.feat_row_kth(blk, 3, self0=-1).shape == (3,)


# ---- run to run, guard bands ---------------------------------------------------------------------------------------------

def test_every_entry_point_gives_the_same_bits_twice():
    x, y = real_case(100, 130, 64)
    xd, yd = dev(x), dev(y)

    def run():
        nx, ny = hb.feat_rownorm(xd), hb.feat_rownorm(yd)
        ws = torch.empty(hb.feat_poly_tiles(100, 130), dtype=torch.float64, device=DEV)
        tot = hb.feat_poly_sum(xd, yd, ws=ws)
        sym = hb.feat_poly_sum(xd, xd, symmetric=True)
        blk = hb.feat_dist2_block(xd, yd, nx, ny, 16, 50)
        own = hb.feat_dist2_block(xd, xd, nx, nx, 16, 50)
        r2 = torch.zeros(100, dtype=torch.float64, device=DEV)
        hb.feat_row_kth(own, 3, self0=16, out=r2[16:66])
        flags = hb.feat_col_any(blk, r2, 16, torch.zeros(130, dtype=torch.uint8, device=DEV))
        return nx, ny, ws, tot, sym, blk, own, r2, flags, torch.tensor(fid.kid(xd, yd, num_subsets=3, max_subset_size=50)), \
            torch.tensor(fid.precision_recall(xd, yd, row_block=32))

    assert all(torch.equal(a, b) for a, b in zip(run(), run()))


def _banded(shape, dtype=torch.float64, band=64):
    """(allocation, view of `shape`) with `band` poisoned elements on either side: NaN for fp64, 0xAB for bytes."""
    n = int(np.prod(shape))
    fill = float("nan") if dtype.is_floating_point else 0xAB
    flat = torch.full((n + 2 * band,), fill, dtype=dtype, device=DEV)
    return flat, flat[band:band + n].view(shape)


def _bands_intact(flat, n, band=64):
    ends = torch.cat([flat[:band], flat[band + n:]])
    return bool(torch.isnan(ends).all()) if flat.dtype.is_floating_point else bool((ends == 0xAB).all())


def test_outputs_and_workspace_stay_between_their_guard_bands():
    x, y = real_case(17, 33, 16)
    xd, yd = dev(x), dev(y)
    watch = []

    def banded(shape, dtype=torch.float64):
        flat, view = _banded(shape, dtype)
        watch.append((flat, int(np.prod(shape))))
        return view

    nx, ny = hb.feat_rownorm(xd, out=banded((17,))), hb.feat_rownorm(yd, out=banded((33,)))
    ws, tot = banded((hb.feat_poly_tiles(17, 33),)), banded((1,))
    hb.feat_poly_sum(xd, yd, ws=ws, out=tot)
    ws2, tot2 = banded((hb.feat_poly_tiles(17, 17),)), banded((1,))
    hb.feat_poly_sum(xd, xd, symmetric=True, ws=ws2, out=tot2)
    r2 = banded((17,))
    flags = banded((33,), torch.uint8)
    flags.zero_()
    for r0, rows in ((0, 16), (16, 1)):  # a full and a ragged row block
        own = hb.feat_dist2_block(xd, xd, nx, nx, r0, rows, out=banded((rows, 17)))
        hb.feat_row_kth(own, 3, self0=r0, out=r2[r0:r0 + rows])
    for r0, rows in ((0, 16), (16, 1)):
        blk = hb.feat_dist2_block(xd, yd, nx, ny, r0, rows, out=banded((rows, 33)))
        hb.feat_col_any(blk, r2, r0, flags)
    torch.cuda.synchronize()
    assert all(_bands_intact(flat, n) for flat, n in watch)
    assert not torch.isnan(torch.cat([nx, ny, ws, tot, ws2, tot2, r2])).any()
    assert torch.equal(flags.cpu(), torch.from_numpy(fd.inside(x, y, 3)))
    assert abs(float(tot.cpu()[0]) - fd.poly_sum(x, y)) <= fd.poly_sum_bound(x, y)


# ---- evaluator, Trainer, command lines -----------------------------------------------------------------------------------

class _StandIn(torch.nn.Module):
    """A small frozen network in place of Inception: [B, 3, 299, 299] -> [B, 32, 4, 4]."""
    weights_id = "standin"

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.conv = torch.nn.Conv2d(3, 32, 7, stride=4)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(32, 3, 7, 7, generator=g) * 0.2)
            self.conv.bias.copy_(torch.randn(32, generator=g) * 0.1)

    def forward(self, x):
        return torch.nn.functional.adaptive_avg_pool2d(torch.relu(self.conv(x)), 4).contiguous()


def _images(n, size, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(n, 3, 1, 1, generator=g) * (0.5 + 0.1 * seed)
    return (base + 0.3 * torch.rand(n, 3, size, size, generator=g)).clamp(0, 1)


def test_evaluator_keeps_features_only_when_asked():
    real, fake = _images(48, 32, 1), _images(40, 32, 2)
    net = _StandIn().to(DEV)
    plain, keep = fid.FIDEvaluator(net), fid.FIDEvaluator(net, keep_features=True)
    feats = {"real": [], "fake": []}
    for ev in (plain, keep):
        for i in range(0, 48, 16):
            ev.add_real(real[i:i + 16].to(DEV))
        for i in range(0, 40, 8):
            ev.add_fake(fake[i:i + 8].to(DEV))
    assert keep.value() == plain.value()
    assert plain._feats == {"real": [], "fake": []}
    with pytest.raises(AssertionError):
        plain.kid()
    with pytest.raises(AssertionError):
        plain.precision_recall()
    fr, ff = keep.real_features, keep.fake_features
    assert tuple(fr.shape) == (48, 32) and tuple(ff.shape) == (40, 32) and fr.dtype == torch.float32 and fr.is_cuda
    # the kept rows are what FIDStats.update returned: their fp64 moments are the statistics'
    assert torch.allclose(fr.double().sum(0), keep.real.sum, rtol=1e-12, atol=0)
    x, y = host(fr), host(ff)
    subsets = fd.draw_subsets(48, 40, 4, 30, seed=5)
    got, want = keep.kid(num_subsets=4, max_subset_size=30, seed=5), fd.kid(x, y, subsets)
    assert abs(got[0] - want[0]) <= 1e-9 * abs(want[0]) + 1e-12 and abs(got[1] - want[1]) <= 1e-9 * abs(want[0]) + 1e-12, (got, want)
    if fd.undecided_pairs(x, y, 3) + fd.undecided_pairs(y, x, 3) == 0:
        assert keep.precision_recall() == fd.precision_recall(x, y, 3)
    assert keep.precision_recall(k=2, row_block=16) == fid.precision_recall(fr, ff, k=2, row_block=16)


@pytest.fixture
def deterministic_library(monkeypatch):
    """Two FID evaluations are compared bit for bit below.  The Inception convolutions run on the stock library, whose
    default algorithm choice is not reproducible run to run; cli.py's set_seed pins it as the reference does, and so does
    this fixture for the duration of a test (the fixture of tests/test_jpeg_gpu.py)."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


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

    d = torch.device(DEV)
    tr = module.Trainer(name=name, base_dir=str(tmp_path), image_size=32, network_capacity=4, fmap_max=64, batch_size=8,
                        gradient_accumulate_every=1, classifier=TinyClassifier(seed=99).to(d),
                        lpips_fn=LPIPSStandIn(seed=4242).to(d), classifier_name="resnet", evaluate_every=10 ** 9,
                        save_every=10 ** 9, device=d, tensorboard_dir=None, **kw)
    gen = torch.Generator().manual_seed(5)
    tr.loader = _CountingLoader([torch.rand(8, 3, 32, 32, generator=gen) for _ in range(4)])
    return tr


def _fid_run(module, tmp_path, name, metrics):
    """init, one calculate_fid, one train() call on an FID step; (trainer, first FID, fid_scores.txt bytes)."""
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)  # the train step draws from all three (mixing regularisation)
    tr = _trainer(module, tmp_path, name, fid_weights="random:1", calculate_fid_num_images=16, fid_metrics=metrics)
    tr.init_StylEx()
    first = tr.calculate_fid(2)
    tr.calculate_fid_every, tr.steps = 1, 1
    tr.train()
    return tr, first, (tmp_path / "results" / name / "fid_scores.txt").read_bytes()


@pytest.mark.parametrize("arch", ["stylex_train", "stylex_train_new"])
def test_trainer_fid_metrics(tmp_path, arch, deterministic_library):
    import importlib

    module = importlib.import_module(arch)
    plain, fid_plain, scores_plain = _fid_run(module, tmp_path / "p", "m", ())
    tr, fid_with, scores_with = _fid_run(module, tmp_path / "w", "m", ("kid", "pr"))
    assert fid_with == fid_plain and scores_with == scores_plain and tr.last_fid == plain.last_fid
    assert tr.loader.taken == plain.loader.taken
    assert not (tmp_path / "p" / "results" / "m" / "fid_metrics.txt").exists() and plain.last_fid_metrics is None
    lines = (tmp_path / "w" / "results" / "m" / "fid_metrics.txt").read_text().splitlines()
    assert len(lines) == 1 and len(lines[0].split(",")) == 6, lines
    step, value, kid_mean, kid_std, precision, recall = lines[0].split(",")
    assert int(step) == 1 and float(value) == tr.last_fid
    ev = tr._fid_eval
    assert ev.keep_features and tuple(ev.real_features.shape) == (16, 2048) and tuple(ev.fake_features.shape) == (16, 2048)
    assert (float(kid_mean), float(kid_std)) == fid.kid(ev.real_features, ev.fake_features) == tr.last_fid_metrics["kid"]
    assert (float(precision), float(recall)) == fid.precision_recall(ev.real_features, ev.fake_features)
    assert (tr.last_fid_metrics["precision"], tr.last_fid_metrics["recall"]) == (float(precision), float(recall))
    # the real features are cached beside the statistics: reused, then rebuilt under clear_fid_cache
    cache = tmp_path / "w" / "fid" / "m" / "real_features.npy"
    assert cache.exists() and (tmp_path / "w" / "fid" / "m" / "real_features.npy.tag").exists()
    taken, kept = tr.loader.taken, ev.real_features.clone()
    tr.calculate_fid(2)
    assert tr.loader.taken == taken and torch.equal(tr._fid_eval.real_features, kept), "the cached real features were not reused"
    tr.clear_fid_cache = True
    tr.calculate_fid(2)
    assert tr.loader.taken == taken + 2
    tr.clear_fid_cache = False
    (tmp_path / "w" / "fid" / "m" / "real_features.npy.tag").write_text("another tag")
    tr.calculate_fid(2)
    assert tr.loader.taken == taken + 4, "a mistagged feature file must not be used"
    only_kid = _trainer(module, tmp_path / "k", "m", fid_weights="random:1", fid_metrics=("kid",))
    only_kid.init_StylEx()
    only_kid.calculate_fid(2)
    assert sorted(only_kid.last_fid_metrics) == ["kid"]
    with pytest.raises(AssertionError):
        _trainer(module, tmp_path / "x", "m", fid_metrics=("fidelity",))


def _write_folder(path, n, seed):
    from PIL import Image

    path.mkdir()
    rng = np.random.RandomState(seed)
    for i in range(n):
        a = (rng.randint(0, 256, (32, 32, 3)) * (0.4 + 0.6 * seed / 3)).astype(np.uint8)
        Image.fromarray(a).save(path / ("%02d.png" % i))


def test_fid_cli_prints_the_metrics_only_when_asked(tmp_path, monkeypatch, capsys, deterministic_library):
    import fid_cli
    import fid_inception as fi

    _write_folder(tmp_path / "a", 12, 1)
    _write_folder(tmp_path / "b", 10, 2)
    net = fi.build("random:1", torch.device(DEV))
    monkeypatch.setattr(fi, "build", lambda spec, device: net)
    base = ["--real", str(tmp_path / "a"), "--fake", str(tmp_path / "b"), "--weights", "random:1", "--batch", "6"]
    v = fid_cli.main(base)
    plain = capsys.readouterr().out.splitlines()
    assert [ln for ln in plain if ln.startswith(("KID", "Precision", "Recall"))] == []
    v2 = fid_cli.main(base + ["--metrics", "kid,pr", "--kid_subsets", "4", "--kid_subset_size", "8", "--pr_k", "2"])
    out = capsys.readouterr().out.splitlines()
    assert v2 == v and [ln for ln in out if ln.startswith("FID: ")] == [ln for ln in plain if ln.startswith("FID: ")]
    tail = out[out.index([ln for ln in out if ln.startswith("FID: ")][0]) + 1:]
    assert [ln.split(":")[0] for ln in tail] == ["KID", "Precision", "Recall"], tail
    ev = fid.FIDEvaluator(net, keep_features=True)
    fid_cli.add_folder(ev.add_real, str(tmp_path / "a"), 6, torch.device(DEV))
    fid_cli.add_folder(ev.add_fake, str(tmp_path / "b"), 6, torch.device(DEV))
    mean, std = ev.kid(num_subsets=4, max_subset_size=8)
    p, r = ev.precision_recall(k=2)
    assert tail == ["KID: %s +- %s" % (mean, std), "Precision: %s" % p, "Recall: %s" % r]
    assert math.isfinite(mean) and 0.0 <= p <= 1.0 and 0.0 <= r <= 1.0
    v3 = fid_cli.main(base + ["--metrics", "kid"])
    assert v3 == v and [ln.split(":")[0] for ln in capsys.readouterr().out.splitlines() if not ln.startswith("FID")][-1:] == ["KID"]
