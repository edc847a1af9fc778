"""Float64 definitions of the pairwise feature metrics (csrc/feature_metrics.hip; stylex/fid.py: kid, precision_recall),
written from the formulas and independent of the kernels' pass structure; a numpy model OF that pass structure (tiles of
16, tile sums, row blocks, block-wise OR, self left out by index) with switches that each break it in one way; the error
bounds both test files hold results to; and the input cases they share.

KID (Binkowski et al. 2018, as StyleGAN2-ADA computes it): k(a, b) = (a . b / D + 1)^3; per subset (ix, iy) of size s
  MMD^2_u = [sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)] / (s (s - 1)) - 2 sum_{i, j} k(x_i, y_j) / s^2;
(mean, std) over the subsets, std with ddof 0.
Improved precision / recall (Kynkaanniemi et al. 2019): d2(a, b) = max(|a|^2 + |b|^2 - 2 a . b, 0); r2_i = the k-th
smallest d2(x_i, x_j) over j != i (by index: a duplicate of x_i is a neighbour at distance 0);
inside(ref, q)_j = any_i d2(ref_i, q_j) <= r2_i(ref); precision = mean inside(real, fake), recall = mean inside(fake, real).
No square root anywhere.

Bounds (u = 2^-53; every product of two fp32 values is exact in fp64, so only the additions round): a dot product of
length D summed in any order is within (D - 1) u sum_k |x_ik y_jk| (1 + O(D u)); each norm likewise; the three further
operations of the distance add at most 3 u of the magnitudes involved.  With S_ij = |x_i|^2 + |y_j|^2 + 2 sum_k |x_ik y_jk|
every distance is within 4 (D + 4) u S_ij; a radius, being one of the distances of its row, within the largest such bound
of the row.  The cube of t = dot / D + 1 has relative error 3 (D + 1) u + 3 u <= 4 (D + 4) u against the bound's
(sum_k |x_ik y_jk| / D + 1)^3 >= |t|^3, and adding n m terms in any order costs at most n m u sum |k_ij|."""
import numpy as np

U = 2.0 ** -53


# ---- definitions -----------------------------------------------------------------------------------------------------------

def f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32 and a.ndim == 2, (a.dtype, a.shape)
    return a.astype(np.float64)


def poly(x, y):
    """k(x_i, y_j) = (x_i . y_j / D + 1)^3, [n, m]."""
    x, y = f64(x), f64(y)
    t = x @ y.T / x.shape[1] + 1.0
    return t * t * t


def poly_sum(x, y, symmetric=False):
    k = poly(x, y)
    if symmetric:
        assert k.shape[0] == k.shape[1]
        k = k - np.diag(np.diag(k))
    return float(k.sum())


def mmd2(x, y):
    """MMD^2_u of two equally sized sets."""
    s = len(x)
    assert len(y) == s and s >= 2
    return (poly_sum(x, x, True) + poly_sum(y, y, True)) / (s * (s - 1)) - 2.0 * poly_sum(x, y) / (s * s)


def draw_subsets(n, m, num_subsets=100, max_subset_size=1000, seed=0):
    """The subsets fid.kid draws: a private RandomState(seed), choice without replacement per side and per subset."""
    rng = np.random.RandomState(seed)
    s = min(n, m, max_subset_size)
    return [(rng.choice(n, s, replace=False), rng.choice(m, s, replace=False)) for _ in range(num_subsets)]


def kid(x, y, subsets, ddof=0):
    v = np.array([mmd2(np.asarray(x)[ix], np.asarray(y)[iy]) for ix, iy in subsets], dtype=np.float64)
    return float(v.mean()), float(v.std(ddof=ddof))


def dist2(x, y):
    x, y = f64(x), f64(y)
    return np.maximum((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (x @ y.T), 0.0)


def radii2(x, k=3):
    """r2_i: the k-th smallest squared distance from x_i to the other rows, self left out by index."""
    d = dist2(x, x)
    n = len(d)
    assert 1 <= k < n
    out = np.empty(n)
    for i in range(n):
        out[i] = np.sort(np.delete(d[i], i))[k - 1]
    return out


def inside(ref, q, k=3):
    """Per row of q: does it lie within the radius of any row of ref?  [m] of 0 / 1."""
    return (dist2(ref, q) <= radii2(ref, k)[:, None]).any(0).astype(np.uint8)


def precision_recall(real, fake, k=3):
    return float(inside(real, fake, k).mean()), float(inside(fake, real, k).mean())


# ---- bounds ----------------------------------------------------------------------------------------------------------------

def abs_dot(x, y):
    return np.abs(f64(x)) @ np.abs(f64(y)).T


def dist2_bound(x, y):
    """Per-entry bound 4 (D + 4) u S_ij, [n, m]."""
    x64, y64 = f64(x), f64(y)
    s = (x64 * x64).sum(1)[:, None] + (y64 * y64).sum(1)[None, :] + 2.0 * abs_dot(x, y)
    return 4.0 * (x64.shape[1] + 4) * U * s


def radius_bound(x):
    return dist2_bound(x, x).max(1)


def poly_entry_bound(x, y):
    d = np.asarray(x).shape[1]
    return 4.0 * (d + 4) * U * (abs_dot(x, y) / d + 1.0) ** 3


def poly_sum_bound(x, y):
    """Bound of any sum over (a subset of) the pairs: entry bounds plus n m u sum |k_ij|."""
    n, m = len(x), len(y)
    return float(poly_entry_bound(x, y).sum() + n * m * U * np.abs(poly(x, y)).sum())


def undecided_pairs(ref, q, k=3):
    """Pairs whose flag a result within the bounds could still turn: |d2 - r2| inside the sum of the two bounds."""
    gap = np.abs(dist2(ref, q) - radii2(ref, k)[:, None])
    return int((gap <= dist2_bound(ref, q) + radius_bound(ref)[:, None]).sum())


# ---- inputs ----------------------------------------------------------------------------------------------------------------

INT_SHAPES = [(1, 1), (4, 4), (15, 17), (16, 16), (17, 33), (48, 31)]
REAL_SHAPES = [(17, 33, 16), (100, 130, 64), (257, 255, 2048)]


def integer_features(n, m, d, seed=0):
    """x [n, d], y [m, d] with entries in {0..3}; every third row of y is a copy of a row of x, so that distance exactly 0 and
    exact ties at a radius occur."""
    rng = np.random.RandomState(1000 * seed + 7 * n + 3 * m + d)
    x = rng.randint(0, 4, size=(n, d)).astype(np.float32)
    y = rng.randint(0, 4, size=(m, d)).astype(np.float32)
    for j in range(0, m, 3):
        y[j] = x[rng.randint(0, n)]
    return x, y


def real_features(n, m, d, seed=22):
    """Rank-4 features relu(z A): z ~ N(shift, I_4), A [4, d] ~ N / 2, shift 0 for x and 0.6 for y.  With the default seed
    the definition gives precision / recall 0.91 / 0.76, 0.84 / 0.93 and 0.82 / 0.80 at REAL_SHAPES (k = 3) and no pair
    within the error bounds of its radius at k = 1, 3, 8 (smallest gap 3e-3 against bounds <= 1.9e-8); the tests assert both
    on the definition, so another generator fails loudly."""
    rng = np.random.RandomState(50 + seed)
    a = rng.randn(4, d) / 2.0
    x = np.maximum(rng.randn(n, 4) @ a, 0.0).astype(np.float32)
    y = np.maximum((rng.randn(m, 4) + 0.6) @ a, 0.0).astype(np.float32)
    return x, y


# ---- model of the pass structure -------------------------------------------------------------------------------------------
# Switches (all False / 0: the kernels' structure): keep_diag, strict (< for <=), k_off, self_by_value, drop_ragged,
# dot_once (nx + ny - dot), skip_block (index of a row block left out of the OR).

def model_dot_tiles(x, y):
    """Dot products in fp64 from fp32 rows, D walked in ascending blocks of 16 as pair_f64_kernel walks it."""
    x, y = f64(x), f64(y)
    acc = np.zeros((len(x), len(y)))
    for k0 in range(0, x.shape[1], 16):
        for q in range(4):
            acc += x[:, k0 + q:k0 + 16:4] @ y[:, k0 + q:k0 + 16:4].T
    return acc


def model_poly_tile_sums(x, y, symmetric=False, keep_diag=False, drop_ragged=False):
    """tile_sums [TI, TJ] of the POLY pass: each 16 x 16 tile's valid entries, i == j left out when symmetric."""
    n, m, d = len(x), len(y), np.asarray(x).shape[1]
    t = model_dot_tiles(x, y) * (1.0 / d) + 1.0
    k = t * t * t
    if symmetric and not keep_diag:
        k[np.arange(n)[:, None] == np.arange(m)[None, :]] = 0.0
    ti, tj = (n + 15) // 16, (m + 15) // 16
    sums = np.zeros((ti, tj))
    for a in range(ti):
        for b in range(tj):
            if drop_ragged and ((a + 1) * 16 > n or (b + 1) * 16 > m):
                continue
            sums[a, b] = k[a * 16:(a + 1) * 16, b * 16:(b + 1) * 16].sum()
    return sums


def model_poly_sum(x, y, symmetric=False, **kw):
    return float(model_poly_tile_sums(x, y, symmetric, **kw).ravel().sum())


def model_mmd2(x, y, **kw):
    s = len(x)
    return (model_poly_sum(x, x, True, **kw) + model_poly_sum(y, y, True, **kw)) / (s * (s - 1)) - 2.0 * model_poly_sum(x, y, **kw) / (s * s)


def model_kid(x, y, subsets, ddof=0, **kw):
    v = np.array([model_mmd2(np.asarray(x)[ix], np.asarray(y)[iy], **kw) for ix, iy in subsets])
    return float(v.mean()), float(v.std(ddof=ddof))


def model_rownorm(x):
    x = f64(x)
    return (x * x).sum(1)


def model_dist2_block(x, y, nx, ny, row0, rows, dot_once=False, drop_ragged=False):
    dot = model_dot_tiles(np.asarray(x)[row0:row0 + rows], y)
    out = np.maximum((nx[row0:row0 + rows, None] + ny[None, :]) - (1.0 if dot_once else 2.0) * dot, 0.0)
    if drop_ragged:
        out[(rows // 16) * 16:, :] = np.inf
        out[:, (len(y) // 16) * 16:] = np.inf
    return out


def model_row_kth(block, k, self0=-1, self_by_value=False, k_off=0):
    out = np.empty(len(block))
    for i, row in enumerate(block):
        if self0 >= 0:
            row = row[row != row[self0 + i]] if self_by_value else np.delete(row, self0 + i)
        row = np.sort(row)
        out[i] = row[min(k - 1 + k_off, len(row) - 1)] if len(row) else np.inf
    return out


def model_radii2(x, k=3, row_block=16, **kw):
    kth = {a: kw.pop(a) for a in ("self_by_value", "k_off") if a in kw}
    nx = model_rownorm(x)
    out = np.empty(len(x))
    for r0 in range(0, len(x), row_block):
        rows = min(row_block, len(x) - r0)
        out[r0:r0 + rows] = model_row_kth(model_dist2_block(x, x, nx, nx, r0, rows, **kw), k, r0, **kth)
    return out


def model_inside(ref, q, k=3, row_block=16, strict=False, skip_block=None, **kw):
    r2 = model_radii2(ref, k, row_block, **kw)
    for a in ("self_by_value", "k_off"):
        kw.pop(a, None)
    nr, nq = model_rownorm(ref), model_rownorm(q)
    flags = np.zeros(len(q), dtype=np.uint8)
    for b, r0 in enumerate(range(0, len(ref), row_block)):
        if b == skip_block:
            continue
        rows = min(row_block, len(ref) - r0)
        blk = model_dist2_block(ref, q, nr, nq, r0, rows, **kw)
        hit = blk < r2[r0:r0 + rows, None] if strict else blk <= r2[r0:r0 + rows, None]
        flags |= hit.any(0).astype(np.uint8)
    return flags


def model_precision_recall(real, fake, k=3, row_block=16, **kw):
    return float(model_inside(real, fake, k, row_block, **kw).mean()), float(model_inside(fake, real, k, row_block, **kw).mean())
