"""KID and precision / recall without a GPU: the subset drawing of fid.kid (its own generator, the global ones untouched),
the feature cache file, and the argument validation of every entry point of csrc/feature_metrics.hip — all of it runs before
anything is launched, so the library answers on a machine without a device."""
import ctypes
import random

import numpy as np
import pytest
import torch

import _feature_metrics_defs as fd
import fid
import hip_backend

EINVAL = -1


def test_kid_subsets_come_from_a_private_generator():
    torch.manual_seed(123)
    np.random.seed(123)
    random.seed(123)
    before = (torch.get_rng_state().clone(), np.random.get_state()[1].copy(), random.getstate())
    a = fid.kid_subsets(300, 280, num_subsets=6, max_subset_size=100, seed=4)
    b = fid.kid_subsets(300, 280, num_subsets=6, max_subset_size=100, seed=4)
    c = fid.kid_subsets(300, 280, num_subsets=6, max_subset_size=100, seed=5)
    with pytest.raises(hip_backend.StylexHipError):  # there is no host path; the draw itself has happened by then
        fid.kid(torch.zeros(40, 16), torch.zeros(30, 16), num_subsets=2)
    assert torch.equal(torch.get_rng_state(), before[0]) and np.array_equal(np.random.get_state()[1], before[1])
    assert random.getstate() == before[2]
    assert len(a) == 6 and all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a, b))
    assert not all(np.array_equal(p[0], q[0]) for p, q in zip(a, c))
    want = fd.draw_subsets(300, 280, 6, 100, seed=4)
    assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a, want))
    for ix, iy in a:  # without replacement, inside each side's range
        assert len(set(ix)) == len(ix) == 100 and len(set(iy)) == 100 and ix.max() < 300 and iy.max() < 280


@pytest.mark.parametrize("n,m,cap,s", [(300, 280, 1000, 280), (50, 70, 1000, 50), (3000, 2000, 1000, 1000), (40, 40, 16, 16)])
def test_kid_subset_size_is_the_smallest_of_the_three(n, m, cap, s):
    subsets = fid.kid_subsets(n, m, num_subsets=2, max_subset_size=cap)
    assert all(len(ix) == len(iy) == s for ix, iy in subsets)


def test_feature_cache_round_trip_and_tag(tmp_path):
    f = torch.from_numpy(fd.real_features(20, 4, 32)[0])
    path = tmp_path / "fid" / "real_features.npy"
    fid.save_features(path, f, "image_size=32;weights=random:1")
    back = fid.load_features(path, "image_size=32;weights=random:1", "cpu")
    assert back.dtype == torch.float32 and torch.equal(back, f)
    assert fid.load_features(path, "image_size=64;weights=random:1", "cpu") is None
    assert fid.load_features(tmp_path / "absent.npy", "image_size=32;weights=random:1", "cpu") is None
    (tmp_path / "fid" / "real_features.npy.tag").unlink()
    assert fid.load_features(path, "image_size=32;weights=random:1", "cpu") is None


def test_evaluator_methods_need_kept_features():
    ev = fid.FIDEvaluator(net=None)
    assert ev.keep_features is False
    for call in (ev.kid, ev.precision_recall):
        with pytest.raises(AssertionError, match="keep_features"):
            call()


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = hip_backend.load_library()
    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = ctypes.c_void_p(base)          # 16-byte aligned
    odd8 = ctypes.c_void_p(base + 8)   # 8- but not 16-byte aligned: no home for fp32 rows read four at a time
    odd4 = ctypes.c_void_p(base + 4)   # not 8-byte aligned: no home for fp64
    big = 1 << 31

    # stylex_feat_rownorm(x, out, n, D, stream)
    assert lib.stylex_feat_rownorm(None, p, 4, 16, None) == EINVAL
    assert lib.stylex_feat_rownorm(p, None, 4, 16, None) == EINVAL
    for n, d in ((0, 16), (-1, 16), (4, 0), (4, 8), (4, 24), (big, 16), (1 << 20, 1 << 12)):
        assert lib.stylex_feat_rownorm(p, p, n, d, None) == EINVAL, (n, d)
    assert lib.stylex_feat_rownorm(odd8, p, 4, 16, None) == EINVAL
    assert lib.stylex_feat_rownorm(p, odd4, 4, 16, None) == EINVAL

    # stylex_feat_poly_workspace_bytes(n, m)
    assert lib.stylex_feat_poly_workspace_bytes(17, 33) == 2 * 3 * 8
    for n, m in ((0, 4), (4, 0), (big, 4), (4, big), (1 << 20, 1 << 20)):
        assert lib.stylex_feat_poly_workspace_bytes(n, m) == -1, (n, m)

    # stylex_feat_poly_sum(x, y, n, m, D, symmetric, gamma, coef0, tile_sums_ws, out, stream)
    poly = lambda x=p, y=p, n=8, m=8, d=16, sym=0, ws=p, out=p: lib.stylex_feat_poly_sum(x, y, n, m, d, sym, 1 / 16, 1.0, ws, out, None)  # noqa: E731
    for kw in (dict(x=None), dict(y=None), dict(ws=None), dict(out=None), dict(n=0), dict(m=-3), dict(d=8), dict(d=40),
               dict(n=8, m=9, sym=1), dict(n=big), dict(n=1 << 20, d=1 << 12), dict(m=1 << 20, d=1 << 12), dict(n=1 << 20, m=1 << 20),
               dict(x=odd8), dict(y=odd8), dict(ws=odd4), dict(out=odd4)):
        assert poly(**kw) == EINVAL, kw

    # stylex_feat_dist2_block(x, y, nx, ny, row0, R, n, m, D, out_block, stream)
    dist = lambda x=p, y=p, nx=p, ny=p, row0=0, r=8, n=8, m=8, d=16, out=p: lib.stylex_feat_dist2_block(x, y, nx, ny, row0, r, n, m, d, out, None)  # noqa: E731
    for kw in (dict(x=None), dict(y=None), dict(nx=None), dict(ny=None), dict(out=None), dict(n=0), dict(m=0), dict(d=0), dict(d=17),
               dict(r=0), dict(row0=-1), dict(row0=1), dict(row0=8, r=1), dict(r=9), dict(n=1 << 20, d=1 << 12),
               dict(m=1 << 20, d=1 << 12), dict(n=1 << 16, r=1 << 16, m=1 << 16), dict(x=odd8), dict(y=odd8), dict(nx=odd4),
               dict(ny=odd4), dict(out=odd4)):
        assert dist(**kw) == EINVAL, kw

    # stylex_feat_row_kth(block, R, M, k, self0, out_r2, stream)
    kth = lambda blk=p, r=8, m=16, k=3, self0=-1, out=p: lib.stylex_feat_row_kth(blk, r, m, k, self0, out, None)  # noqa: E731
    for kw in (dict(blk=None), dict(out=None), dict(r=0), dict(m=0), dict(k=0), dict(k=9), dict(k=-1), dict(m=3, r=3, k=3, self0=0),
               dict(m=8, r=8, k=8, self0=0), dict(m=2, r=2, k=3), dict(self0=9), dict(self0=16, r=1), dict(r=1 << 16, m=1 << 16),
               dict(blk=odd4), dict(out=odd4)):
        assert kth(**kw) == EINVAL, kw

    # stylex_feat_col_any(block, r2, row0, R, M, flags, stream)
    col = lambda blk=p, r2=p, row0=0, r=8, m=16, flags=p: lib.stylex_feat_col_any(blk, r2, row0, r, m, flags, None)  # noqa: E731
    for kw in (dict(blk=None), dict(r2=None), dict(flags=None), dict(row0=-1), dict(r=0), dict(m=0), dict(r=1 << 16, m=1 << 16),
               dict(row0=big), dict(blk=odd4), dict(r2=odd4)):
        assert col(**kw) == EINVAL, kw
