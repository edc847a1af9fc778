"""The fp64 definitions of KID and precision / recall (tests/_feature_metrics_defs.py) against scipy / scikit-learn, and the
numpy model of the kernels' pass structure (fp32 inputs, fp64 accumulation, tiles of 16, tile sums, row blocks, block-wise
OR, self left out by index) held to the limits the GPU tests hold the kernels to — with one mutation per mechanism, each
of which must break them: the limits have teeth."""
import numpy as np
import pytest

import _feature_metrics_defs as fd


# ---- the definitions -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,m,d", fd.REAL_SHAPES)
def test_definitions_against_scipy_and_sklearn(n, m, d):
    from scipy.spatial.distance import cdist
    from sklearn.metrics.pairwise import polynomial_kernel
    from sklearn.neighbors import NearestNeighbors

    x, y = fd.real_features(n, m, d)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    k = polynomial_kernel(x64, y64, degree=3, gamma=1.0 / d, coef0=1)
    assert np.abs(fd.poly(x, y) - k).max() <= 1e-12 * np.abs(k).max()
    d2 = cdist(x64, y64, "sqeuclidean")
    assert np.abs(fd.dist2(x, y) - d2).max() <= 1e-12 * d2.max()
    for kk in (1, 3, 8):
        # the query point itself is its own nearest neighbour (there are no duplicates here): column kk of kk + 1
        dist, _ = NearestNeighbors(n_neighbors=kk + 1, algorithm="brute").fit(x64).kneighbors(x64)
        assert np.abs(np.sqrt(fd.radii2(x, kk)) - dist[:, kk]).max() <= 1e-6 * dist.max()
    r = np.sqrt(fd.radii2(x, 3))
    want = (np.sqrt(d2) <= r[:, None]).any(0)
    assert np.array_equal(fd.inside(x, y, 3).astype(bool), want)
    p, rec = fd.precision_recall(x, y, 3)
    assert p == want.mean() and 0 < rec < 1


def test_kid_definition():
    x, y = fd.real_features(60, 50, 16, seed=1)
    subsets = fd.draw_subsets(60, 50, 7, 20, seed=3)
    assert len(subsets) == 7 and all(len(ix) == len(iy) == 20 and len(set(ix)) == 20 for ix, iy in subsets)
    vals = []
    for ix, iy in subsets:
        a, b = x[ix].astype(np.float64), y[iy].astype(np.float64)
        kxx, kyy, kxy = [(p @ q.T / 16 + 1) ** 3 for p, q in ((a, a), (b, b), (a, b))]
        vals.append((kxx.sum() - np.trace(kxx) + kyy.sum() - np.trace(kyy)) / (20 * 19) - 2 * kxy.mean())
    mean, std = fd.kid(x, y, subsets)
    assert abs(mean - np.mean(vals)) <= 1e-12 * abs(mean) and abs(std - np.std(vals)) <= 1e-12 * abs(mean)
    same = fd.kid(x, x, [(np.arange(60), np.arange(60))])
    # identical sets: the cross term keeps its diagonal, so the estimate is below zero; one subset has no spread
    assert same[0] < 0 and same[1] == 0.0


def test_self_is_left_out_by_index_not_by_value():
    x, _ = fd.integer_features(6, 6, 16)
    x[4] = x[1]  # a duplicate is a neighbour at distance 0
    r2 = fd.radii2(x, 1)
    assert r2[1] == 0.0 and r2[4] == 0.0 and (np.delete(r2, [1, 4]) > 0).all()


# ---- the model of the pass structure, and its mutations ------------------------------------------------------------------

def test_model_is_exact_on_integers():
    for n, m in fd.INT_SHAPES:
        for d in (16, 64):
            x, y = fd.integer_features(n, m, d)
            assert fd.model_poly_sum(x, y) == fd.poly_sum(x, y) and fd.model_poly_sum(x, x, True) == fd.poly_sum(x, x, True)
            nx, ny = fd.model_rownorm(x), fd.model_rownorm(y)
            for rows in sorted({16, 17, n}):
                got = np.concatenate([fd.model_dist2_block(x, y, nx, ny, r0, min(rows, n - r0)) for r0 in range(0, n, rows)])
                assert np.array_equal(got, fd.dist2(x, y))
            if n >= 2:
                k = min(3, n - 1)
                for rb in (16, 17, n):
                    assert np.array_equal(fd.model_radii2(x, k, rb), fd.radii2(x, k))
                    assert np.array_equal(fd.model_inside(x, y, k, rb), fd.inside(x, y, k))


@pytest.mark.parametrize("n,m,d", fd.REAL_SHAPES)
def test_model_within_the_bounds_on_real_values(n, m, d):
    x, y = fd.real_features(n, m, d)
    nx, ny = fd.model_rownorm(x), fd.model_rownorm(y)
    got = np.concatenate([fd.model_dist2_block(x, y, nx, ny, r0, min(16, n - r0)) for r0 in range(0, n, 16)])
    assert (np.abs(got - fd.dist2(x, y)) <= fd.dist2_bound(x, y)).all()
    assert (np.abs(fd.model_radii2(x, 3) - fd.radii2(x, 3)) <= fd.radius_bound(x)).all()
    for a, b, sym in ((x, y, False), (x, x, True)):
        assert abs(fd.model_poly_sum(a, b, sym) - fd.poly_sum(a, b, sym)) <= fd.poly_sum_bound(a, b)
    assert fd.undecided_pairs(x, y, 3) == 0 and fd.undecided_pairs(y, x, 3) == 0
    for rb in (16, 64, 1024):
        assert fd.model_precision_recall(x, y, 3, rb) == fd.precision_recall(x, y, 3)


def _integer_case():
    return fd.integer_features(17, 33, 16)


def _breaks_flags(**mutation):
    """Does the mutated model miss the definition's flags or radii on an input of the GPU tests?"""
    out = False
    for x, y, k in ((*_integer_case(), 3), (*fd.integer_features(48, 31, 64), 3), (*fd.real_features(17, 33, 16), 3),
                    (*fd.real_features(100, 130, 64), 3)):
        out |= not np.array_equal(fd.model_inside(x, y, k, 16, **mutation), fd.inside(x, y, k))
        out |= not np.array_equal(fd.model_inside(y, x, k, 16, **mutation), fd.inside(y, x, k))
    return out


def test_mutation_diagonal_not_excluded():
    x, y = _integer_case()
    assert fd.model_poly_sum(x, x, True, keep_diag=True) != fd.poly_sum(x, x, True)
    a, b = fd.real_features(17, 33, 16)
    assert abs(fd.model_poly_sum(a, a, True, keep_diag=True) - fd.poly_sum(a, a, True)) > fd.poly_sum_bound(a, a)


def test_mutation_strict_comparison():
    """Only pairs exactly at their radius tell < from <=: the integer inputs have them, the real-valued ones do not."""
    broken = []
    for n, m, d in ((17, 33, 16), (48, 31, 64)):
        x, y = fd.integer_features(n, m, d)
        assert (fd.dist2(x, y) == fd.radii2(x, 3)[:, None]).sum() >= 10
        broken.append(not np.array_equal(fd.model_inside(x, y, 3, 16, strict=True), fd.inside(x, y, 3)))
    assert any(broken)
    a, b = fd.real_features(17, 33, 16)
    assert np.array_equal(fd.model_inside(a, b, 3, 16, strict=True), fd.inside(a, b, 3))


def test_mutation_k_off_by_one():
    assert _breaks_flags(k_off=1) and _breaks_flags(k_off=-1)
    x, _ = fd.real_features(17, 33, 16)
    assert (np.abs(fd.model_radii2(x, 3, k_off=1) - fd.radii2(x, 3)) > fd.radius_bound(x)).any()


def test_mutation_self_excluded_by_value():
    x, _ = _integer_case()
    x = x.copy()
    x[5] = x[2]  # duplicates: leaving out every column that EQUALS the own distance drops the duplicate too
    assert not np.array_equal(fd.model_radii2(x, 1, self_by_value=True), fd.radii2(x, 1))
    assert np.array_equal(fd.model_radii2(x, 1), fd.radii2(x, 1))


def test_mutation_last_ragged_tile_dropped():
    x, y = _integer_case()
    assert fd.model_poly_sum(x, y, drop_ragged=True) != fd.poly_sum(x, y)
    assert _breaks_flags(drop_ragged=True)
    a, b = fd.real_features(17, 33, 16)
    assert abs(fd.model_poly_sum(a, b, drop_ragged=True) - fd.poly_sum(a, b)) > fd.poly_sum_bound(a, b)


def test_mutation_dot_applied_once():
    x, y = _integer_case()
    nx, ny = fd.model_rownorm(x), fd.model_rownorm(y)
    assert not np.array_equal(fd.model_dist2_block(x, y, nx, ny, 0, 17, dot_once=True), fd.dist2(x, y))
    a, b = fd.real_features(17, 33, 16)
    na, nb = fd.model_rownorm(a), fd.model_rownorm(b)
    assert (np.abs(fd.model_dist2_block(a, b, na, nb, 0, 17, dot_once=True) - fd.dist2(a, b)) > fd.dist2_bound(a, b)).any()
    assert _breaks_flags(dot_once=True)


def test_mutation_std_with_ddof_1():
    x, y = fd.real_features(300, 280, 64, seed=3)
    subsets = fd.draw_subsets(300, 280, 5, 100, seed=11)
    want = fd.kid(x, y, subsets)
    good, bad = fd.model_kid(x, y, subsets), fd.model_kid(x, y, subsets, ddof=1)
    bound = max((fd.poly_sum_bound(x[ix], x[ix]) + fd.poly_sum_bound(y[iy], y[iy])) / 9900 + 2 * fd.poly_sum_bound(x[ix], y[iy]) / 1e4
                for ix, iy in subsets) + 1e-15
    print("KID %.12g +- %.12g; ddof 1: %.12g; bound %.3g" % (want + (bad[1], bound)))
    assert abs(good[0] - want[0]) <= bound and abs(good[1] - want[1]) <= bound
    assert abs(bad[1] - want[1]) > 1e3 * bound


def test_mutation_one_row_block_skipped():
    assert _breaks_flags(skip_block=0) and _breaks_flags(skip_block=1)
