"""FID without a GPU: the host arithmetic of stylex/fid.py (distance, covariance from raw moments, the statistics file), the
in-repo FID Inception-v3 (layout, loader, the two pooling rules that set it apart from torchvision's) and the argument
validation of the three entry points of csrc/fid.hip."""
import ctypes

import numpy as np
import pytest
import torch

import fid
import fid_inception as fi
import hip_backend


def _features(d, n, seed):
    rng = np.random.RandomState(seed)
    a = rng.randn(d, d) / np.sqrt(d)
    return np.abs(rng.randn(n, d) @ a + rng.randn(d))


@pytest.mark.parametrize("d,n", [(64, 512), (256, 1024)])
def test_frechet_distance_matches_the_scipy_formula(d, n):
    """pytorch_fid's formula: sqrtm(s1 . s2), real part.  N >= 2 D: with N < D scipy's own square root is only good to 1e-8."""
    linalg = pytest.importorskip("scipy.linalg")
    f1, f2 = _features(d, n, 1), _features(d, n, 2)
    mu1, s1, mu2, s2 = f1.mean(0), np.cov(f1, rowvar=False), f2.mean(0), np.cov(f2, rowvar=False)
    root = linalg.sqrtm(s1.dot(s2))
    want = float((mu1 - mu2).dot(mu1 - mu2) + np.trace(s1) + np.trace(s2) - 2 * np.trace(np.real(root)))
    got = fid.frechet_distance(mu1, s1, mu2, s2)
    rel = abs(got - want) / abs(want)
    print("D = %d, N = %d: eigh %.15g, scipy %.15g, relative difference %.3g" % (d, n, got, want, rel))
    assert rel <= 1e-10
    assert abs(fid.frechet_distance(mu1, s1, mu1, s1)) <= 1e-10 * np.trace(s1)


def test_mean_cov_from_raw_moments_matches_np_cov():
    f = _features(64, 512, 3)
    gram = np.triu(f.T @ f) + np.tril(np.full((64, 64), 1e30), -1)  # whatever lies below the diagonal is not read
    mu, sigma = fid.mean_cov(len(f), f.sum(0), gram)
    want = np.cov(f, rowvar=False)
    err = np.abs(sigma - want).max() / np.abs(want).max()
    print("covariance from raw moments vs np.cov: %.3g of the largest entry" % err)
    assert err <= 1e-12 and np.array_equal(sigma, sigma.T)
    assert np.abs(mu - f.mean(0)).max() <= 1e-14 * np.abs(mu).max()


def test_statistics_file_round_trip_and_tag(tmp_path):
    f = torch.from_numpy(_features(32, 40, 4))
    st = fid.FIDStats(32, "cpu")
    st.n, st.sum, st.gram = 40, f.sum(0), torch.triu(f.T @ f)
    path = tmp_path / "fid" / "real_stats.npz"
    st.save(path, "image_size=32;weights=random:1")
    back = fid.FIDStats.load(path, "image_size=32;weights=random:1", "cpu")
    assert back.n == 40 and torch.equal(back.sum, st.sum) and torch.equal(back.gram, st.gram)
    assert all(np.array_equal(a, b) for a, b in zip(back.mean_cov(), st.mean_cov()))
    # another image size or other weights: no statistics, the caller computes them again
    assert fid.FIDStats.load(path, "image_size=64;weights=random:1", "cpu") is None
    assert fid.FIDStats.load(path, "image_size=32;weights=random:2", "cpu") is None
    assert fid.FIDStats.load(tmp_path / "absent.npz", "image_size=32;weights=random:1", "cpu") is None
    with pytest.raises(Exception):  # update() has no host path
        st.update(torch.zeros(2, 32, 1, 1))


@pytest.fixture(scope="module")
def net():
    return fi.FIDInceptionV3().init_random(1)


def test_inception_layout(net):
    sd = net.state_dict()
    for key, shape in [("Mixed_5b.branch5x5_2.conv.weight", (64, 48, 5, 5)), ("Mixed_5b.branch_pool.conv.weight", (32, 192, 1, 1)),
                       ("Mixed_6a.branch3x3.conv.weight", (384, 288, 3, 3)), ("Mixed_6b.branch7x7_2.conv.weight", (128, 128, 1, 7)),
                       ("Mixed_6b.branch7x7dbl_2.conv.weight", (128, 128, 7, 1)),
                       ("Mixed_7a.branch7x7x3_4.conv.weight", (192, 192, 3, 3)),
                       ("Mixed_7b.branch3x3_2a.conv.weight", (384, 384, 1, 3)),
                       ("Mixed_7c.branch3x3dbl_1.conv.weight", (448, 2048, 1, 1))]:
        assert tuple(sd[key].shape) == shape, key
    convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 94 and all(c.bias is None for c in convs)
    assert all(m.eps == 0.001 for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d))
    assert not any(k.startswith(("AuxLogits", "fc.")) for k in sd)
    taps = {}
    with torch.no_grad():
        y = net(torch.randn(1, 3, 299, 299, generator=torch.Generator().manual_seed(0)), taps=taps)
    assert tuple(y.shape) == (1, 2048, 8, 8) and torch.isfinite(y).all()
    assert tuple(taps["Mixed_5d"].shape) == (1, 288, 35, 35)
    assert tuple(taps["Mixed_6e"].shape) == (1, 768, 17, 17)
    assert tuple(taps["Mixed_7a"].shape) == (1, 1280, 8, 8)


def test_loader_ignores_fc_and_names_a_missing_key(net):
    sd = dict(net.state_dict())
    sd["fc.weight"], sd["fc.bias"] = torch.zeros(1008, 2048), torch.zeros(1008)
    other = fi.FIDInceptionV3()
    other.load_fid_state_dict(sd)
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in net.state_dict().items())
    gone = "Mixed_6c.branch7x7dbl_3.bn.running_var"
    del sd[gone]
    with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
        fi.FIDInceptionV3().load_fid_state_dict(sd)
    sd[gone] = net.state_dict()[gone]
    sd["Mixed_8a.conv.weight"] = torch.zeros(1)
    with pytest.raises(KeyError, match="Mixed_8a"):
        fi.FIDInceptionV3().load_fid_state_dict(sd)


def test_missing_weight_file_is_named(tmp_path, monkeypatch):
    monkeypatch.delenv("STYLEX_FID_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError, match="no_such_weights.pth"):
        fi.build(str(tmp_path / "no_such_weights.pth"))
    monkeypatch.setenv("HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match=fi.WEIGHTS_FILE):
        fi.resolve_weights(None)
    monkeypatch.setenv("STYLEX_FID_WEIGHTS", "random:3")
    assert fi.resolve_weights(None) == "random:3"


def _identity_pool_branch(block, cin):
    """Make `block.branch_pool` the identity on its first channels: 1x1 conv = selection, BatchNorm = identity."""
    layer = block.branch_pool
    with torch.no_grad():
        layer.conv.weight.zero_()
        for o in range(layer.conv.out_channels):
            layer.conv.weight[o, o, 0, 0] = 1.
        layer.bn.weight.fill_(1.)
        layer.bn.bias.zero_()
        layer.bn.running_mean.zero_()
        layer.bn.running_var.fill_(1. - layer.bn.eps)
    return layer.conv.out_channels


def test_pool_branch_of_mixed_5b_averages_without_the_padding():
    net = fi.FIDInceptionV3().init_random(2)
    n = _identity_pool_branch(net.Mixed_5b, 192)
    with torch.no_grad():
        y = net.Mixed_5b(torch.ones(1, 192, 9, 9))
    pool = y[:, -n:]
    assert torch.allclose(pool, torch.ones_like(pool), atol=1e-6)  # count_include_pad=True would give 4/9 in the corners
    assert abs(float(pool[0, 0, 0, 0]) - 1.) < 1e-6


def test_pool_branch_of_mixed_7c_is_a_max_pool_and_7b_an_average():
    net = fi.FIDInceptionV3().init_random(2)
    x = torch.zeros(1, 2048, 8, 8)
    x[0, 5, 3, 4] = 7.
    n = _identity_pool_branch(net.Mixed_7c, 2048)
    with torch.no_grad():
        pool = net.Mixed_7c(x)[:, -n:]
    want = torch.zeros(8, 8)
    want[2:5, 3:6] = 7.
    assert torch.allclose(pool[0, 5], want, atol=1e-5) and float(pool[0, 4].abs().max()) == 0.
    x = torch.zeros(1, 1280, 8, 8)
    x[0, 5, 3, 4] = 9.
    n = _identity_pool_branch(net.Mixed_7b, 1280)
    with torch.no_grad():
        pool = net.Mixed_7b(x)[:, -n:]
    assert torch.allclose(pool[0, 5], want / 7., atol=1e-5)  # 9 / 9 on the same neighbourhood: the average of interior windows


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = hip_backend.load_library()
    EINVAL = -1
    buf = (ctypes.c_double * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    sh, st = i64(2, 8, 8, 299, 299), i64(192, 64, 8, 1)
    assert lib.stylex_fid_prep(None, p, sh, st, 0, None) == EINVAL
    assert lib.stylex_fid_prep(p, None, sh, st, 0, None) == EINVAL
    assert lib.stylex_fid_prep(p, p, None, st, 0, None) == EINVAL
    assert lib.stylex_fid_prep(p, p, sh, None, 0, None) == EINVAL
    assert lib.stylex_fid_prep(p, p, i64(2, 0, 8, 299, 299), st, 0, None) == EINVAL
    assert lib.stylex_fid_prep(p, p, sh, i64(192, 64, -8, 1), 0, None) == EINVAL
    assert lib.stylex_fid_prep(p, p, i64(1 << 20, 8, 8, 299, 299), st, 0, None) == EINVAL  # output past 2^31 elements
    assert lib.stylex_fid_prep(p, p, sh, i64(1 << 31, 64, 8, 1), 1, None) == EINVAL        # input offsets past 2^31
    args = (p, p, p, None, p)
    assert lib.stylex_affine_act_nchw_slice_fwd(None, p, p, None, p, 2, 4, 16, 128, 1, None) == EINVAL
    assert lib.stylex_affine_act_nchw_slice_fwd(p, None, p, None, p, 2, 4, 16, 128, 1, None) == EINVAL
    assert lib.stylex_affine_act_nchw_slice_fwd(p, p, p, None, None, 2, 4, 16, 128, 1, None) == EINVAL
    assert lib.stylex_affine_act_nchw_slice_fwd(*args, 0, 4, 16, 128, 1, None) == EINVAL
    assert lib.stylex_affine_act_nchw_slice_fwd(*args, 2, 4, 16, 63, 1, None) == EINVAL  # rows would overlap
    assert lib.stylex_affine_act_nchw_slice_fwd(*args, 1 << 16, 4, 16, 1 << 16, 1, None) == EINVAL
    assert lib.stylex_fid_moments_acc(None, p, p, p, 4, 16, 1, None) == EINVAL
    assert lib.stylex_fid_moments_acc(p, p, None, p, 4, 16, 1, None) == EINVAL
    assert lib.stylex_fid_moments_acc(p, p, p, None, 4, 16, 1, None) == EINVAL
    assert lib.stylex_fid_moments_acc(p, p, p, p, 4, 24, 1, None) == EINVAL   # D % 16
    assert lib.stylex_fid_moments_acc(p, p, p, p, 0, 16, 1, None) == EINVAL
    assert lib.stylex_fid_moments_acc(p, p, p, p, 4, 16, 0, None) == EINVAL
    assert lib.stylex_fid_moments_acc(p, None, p, p, 4, 16, 4, None) == EINVAL  # pooled features need a buffer
    assert lib.stylex_fid_moments_acc(p, p, p, p, 1 << 20, 2048, 64, None) == EINVAL
