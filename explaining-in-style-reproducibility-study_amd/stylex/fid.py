"""Frechet Inception Distance without image files (reference stylex/stylex_train.py:1577-1622 writes PNG / JPEG folders
and calls pytorch_fid on them): real and generated batches go from the loader / generator through ``stylex_fid_prep``,
the Inception network (fid_inception.py) and ``stylex_fid_moments_acc`` without leaving the GPU; only the two raw moments
(count, sum, upper triangle of the Gram matrix, fp64) come back to the host, where mean, covariance and the distance
are computed in fp64.  The reference's generated images are .jpg files: ``add_fake(batch, jpeg_quality=75)`` applies that
round trip on the device (``stylex_jpeg_roundtrip``) in front of the network.

Beside FID, from the same pooled features (``FIDEvaluator(keep_features=True)`` keeps them on the device): ``kid`` (kernel
inception distance, unbiased for small sample counts) and ``precision_recall`` (improved precision and recall, Kynkaanniemi
et al. 2019), both on the fp64 pairwise kernels of csrc/feature_metrics.hip; definitions and rounding contract in DESIGN §15.
"""
import os

import numpy as np
import torch


class FIDStats:
    """Running raw moments of the pooled features: n, sum [D] and the upper triangle of gram [D, D] (fp64, on the device)."""

    def __init__(self, dim, device):
        assert dim % 16 == 0, "the moments kernel works on 16 x 16 tiles: feature width %d" % dim
        self.dim, self.device, self.n = int(dim), torch.device(device), 0
        self.sum = torch.zeros(dim, dtype=torch.float64, device=device)
        self.gram = torch.zeros(dim, dim, dtype=torch.float64, device=device)

    def update(self, feature_map):
        """feature_map [B, D, h, w], dense fp32 on the GPU: pools it and accumulates; returns the pooled features [B, D]."""
        import hip_backend as hb

        assert feature_map.dim() == 4 and feature_map.shape[1] == self.dim, tuple(feature_map.shape)
        feat = hb.fid_moments_acc(feature_map.contiguous(), self.sum, self.gram)
        self.n += int(feature_map.shape[0])
        return feat

    def mean_cov(self):
        """(mu [D], sigma [D, D]) as fp64 numpy arrays: mu = sum / n, sigma = (gram - n mu mu^T) / (n - 1), the unbiased
        covariance np.cov gives; gram is symmetrised from its upper triangle."""
        return mean_cov(self.n, self.sum.cpu().numpy(), self.gram.cpu().numpy())

    def save(self, path, tag):
        os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
        np.savez(str(path), n=np.int64(self.n), sum=self.sum.cpu().numpy(), gram=np.triu(self.gram.cpu().numpy()),
                 tag=np.array(str(tag)))

    @classmethod
    def load(cls, path, tag, device):
        """The statistics saved under `tag`, or None when there is no file or it was saved under another tag."""
        path = str(path)
        if not os.path.isfile(path):
            return None
        with np.load(path, allow_pickle=False) as z:
            if str(z["tag"]) != str(tag):
                return None
            st = cls(int(z["sum"].shape[0]), device)
            st.n = int(z["n"])
            st.sum.copy_(torch.from_numpy(z["sum"]))
            st.gram.copy_(torch.from_numpy(z["gram"]))
        return st


def mean_cov(n, total, gram):
    """Mean and unbiased covariance from raw moments (fp64 numpy; only gram's upper triangle is read)."""
    assert n >= 2, "a covariance needs at least two samples (got %d)" % n
    total, gram = np.asarray(total, dtype=np.float64), np.asarray(gram, dtype=np.float64)
    up = np.triu(gram)
    full = up + np.triu(gram, 1).T
    mu = total / n
    return mu, (full - n * np.outer(mu, mu)) / (n - 1)


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), fp64 on the host.  S1 S2 is similar to the symmetric positive
    semi-definite S1^(1/2) S2 S1^(1/2), so tr sqrt(S1 S2) = sum_i sqrt(max(lambda_i, 0)) over its eigenvalues: two
    symmetric eigendecompositions (torch.linalg.eigh) instead of scipy's general matrix square root."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)  # noqa: E731
    mu1, mu2, s1, s2 = t(mu1), t(mu2), t(sigma1), t(sigma2)
    lam, vec = torch.linalg.eigh((s1 + s1.T) / 2)
    root = (vec * lam.clamp_min(0).sqrt()) @ vec.T
    m = root @ s2 @ root
    tr = torch.linalg.eigvalsh((m + m.T) / 2).clamp_min(0).sqrt().sum()
    d = mu1 - mu2
    return float(d @ d + torch.trace(s1) + torch.trace(s2) - 2 * tr)


class FIDEvaluator:
    """FID between the images given to add_real and to add_fake.  `net` maps the prepared batch [B, 3, 299, 299] (fp32 in
    [-1, 1]) to a feature map [B, D, h, w] whose spatial mean is the feature (FIDInceptionV3, or any module for tests)."""

    def __init__(self, net, input_size=299, keep_features=False):
        self.net, self.input_size = net, int(input_size)
        self.real = self.fake = None
        # keep_features: the pooled features [B, D] FIDStats.update returns are kept (on the device) for kid /
        # precision_recall; off, nothing is kept and nothing extra is allocated or launched
        self.keep_features = bool(keep_features)
        self._feats = {"real": [], "fake": []}

    def features(self, batch, jpeg_quality=None):
        """Image batch [B, >= 3, H, W] in [0, 1] (fp32 or bf16, any layout) -> the network's last feature map.  With
        `jpeg_quality` the images first go through the JPEG round trip an image folder of .jpg files applies (the decoded
        bytes of hip_backend.jpeg_roundtrip); None keeps the lossless (PNG) path."""
        import hip_backend as hb

        with torch.no_grad():
            if jpeg_quality is None:
                prepared = hb.fid_prep(batch, self.input_size)
            else:
                prepared = hb.fid_prep_u8(hb.jpeg_roundtrip(batch, int(jpeg_quality)), self.input_size)
            fm = self.net(prepared)
        assert fm.dim() == 4 and fm.dtype == torch.float32, (tuple(fm.shape), fm.dtype)
        return fm

    def _add(self, stats, batch, jpeg_quality=None, side=None):
        fm = self.features(batch, jpeg_quality)
        if stats is None:
            stats = FIDStats(fm.shape[1], fm.device)
            if self.keep_features:
                self._feats[side] = []
        feat = stats.update(fm)
        if self.keep_features:
            self._feats[side].append(feat)
        return stats

    def add_real(self, batch):
        self.real = self._add(self.real, batch, side="real")

    def add_fake(self, batch, jpeg_quality=None):
        self.fake = self._add(self.fake, batch, jpeg_quality, side="fake")

    def _kept(self, side):
        assert self.keep_features, "build the evaluator with keep_features=True"
        parts = self._feats[side]
        assert parts, "no %s features: add_%s first (or set_real_features from the cache)" % (side, side)
        if len(parts) > 1:  # concatenated at the first use, once
            parts[:] = [torch.cat(parts)]
        return parts[0]

    @property
    def real_features(self):
        """The real features kept so far, fp32 [n, D] on the device."""
        return self._kept("real")

    @property
    def fake_features(self):
        return self._kept("fake")

    def set_real_features(self, feats):
        """Real features from a cache file (load_features) in place of add_real calls."""
        assert self.keep_features
        self._feats["real"] = [feats]

    def kid(self, **kw):
        """kid() of the kept real and generated features."""
        return kid(self.real_features, self.fake_features, **kw)

    def precision_recall(self, **kw):
        """precision_recall() of the kept real and generated features."""
        return precision_recall(self.real_features, self.fake_features, **kw)

    def value(self):
        assert self.real is not None and self.fake is not None, "add_real and add_fake first"
        return frechet_distance(*self.real.mean_cov(), *self.fake.mean_cov())


# ---- KID and precision / recall on the pooled features (csrc/feature_metrics.hip) ------------------------------

def _dev_features(f):
    f = torch.as_tensor(f)
    assert f.dim() == 2 and f.dtype == torch.float32, (tuple(f.shape), f.dtype)
    return f.contiguous()


def kid_subsets(n, m, num_subsets=100, max_subset_size=1000, seed=0):
    """The index subsets of kid(): s = min(n, m, max_subset_size) indices without replacement per side and per subset from a
    private np.random.RandomState(seed) — no global generator (numpy's or torch's) is read or advanced."""
    rng = np.random.RandomState(seed)
    s = min(int(n), int(m), int(max_subset_size))
    return [(rng.choice(int(n), s, replace=False), rng.choice(int(m), s, replace=False)) for _ in range(int(num_subsets))]


def kid(fx, fy, num_subsets=100, max_subset_size=1000, seed=0, subsets=None):
    """Kernel inception distance (mean, std over the subsets; std with ddof 0) between the feature sets fx [n, D] and fy
    [m, D] (fp32 on the GPU), defaults of StyleGAN2-ADA.  Kernel k(a, b) = (a . b / D + 1)^3; per subset of size s,
    MMD^2_u = [sum_{i != j} k(x_i, x_j) + sum_{i != j} k(y_i, y_j)] / (s (s - 1)) - 2 sum_{i, j} k(x_i, y_j) / s^2.
    `subsets`: explicit [(ix, iy), ...] in place of the drawn ones.  Per subset three stylex_feat_poly_sum calls leave three
    fp64 scalars on the device; all subsets are queued, one transfer brings the scalars back, the rest is host fp64."""
    import hip_backend as hb

    fx, fy = _dev_features(fx), _dev_features(fy)
    if subsets is None:
        subsets = kid_subsets(fx.shape[0], fy.shape[0], num_subsets, max_subset_size, seed)
    assert len(subsets) >= 1
    sums = torch.empty((len(subsets), 3), dtype=torch.float64, device=fx.device)
    ws = None
    sizes = []
    for q, (ix, iy) in enumerate(subsets):
        ix, iy = np.asarray(ix, dtype=np.int64), np.asarray(iy, dtype=np.int64)
        s = len(ix)
        assert len(iy) == s and s >= 2, "a KID subset needs at least two samples per side (got %d, %d)" % (len(ix), len(iy))
        sizes.append(s)
        x = fx.index_select(0, torch.from_numpy(ix).to(fx.device))
        y = fy.index_select(0, torch.from_numpy(iy).to(fy.device))
        if ws is None or ws.numel() != hb.feat_poly_tiles(s, s):
            ws = torch.empty(hb.feat_poly_tiles(s, s), dtype=torch.float64, device=fx.device)
        hb.feat_poly_sum(x, x, symmetric=True, out=sums[q, 0:1], ws=ws)
        hb.feat_poly_sum(y, y, symmetric=True, out=sums[q, 1:2], ws=ws)
        hb.feat_poly_sum(x, y, symmetric=False, out=sums[q, 2:3], ws=ws)
    host = sums.cpu().numpy()
    s = np.asarray(sizes, dtype=np.float64)
    v = (host[:, 0] + host[:, 1]) / (s * (s - 1.0)) - 2.0 * host[:, 2] / (s * s)
    return float(v.mean()), float(v.std())


def _radii2(f, nf, k, row_block, block):
    import hip_backend as hb

    n = f.shape[0]
    r2 = torch.empty(n, dtype=torch.float64, device=f.device)
    for r0 in range(0, n, row_block):
        rows = min(row_block, n - r0)
        blk = block[:rows * n].view(rows, n)
        hb.feat_dist2_block(f, f, nf, nf, r0, rows, out=blk)
        hb.feat_row_kth(blk, k, self0=r0, out=r2[r0:r0 + rows])
    return r2


def _inside(ref, nref, r2, q, nq, row_block, block, flags):
    import hip_backend as hb

    n, m = ref.shape[0], q.shape[0]
    for r0 in range(0, n, row_block):
        rows = min(row_block, n - r0)
        blk = block[:rows * m].view(rows, m)
        hb.feat_dist2_block(ref, q, nref, nq, r0, rows, out=blk)
        hb.feat_col_any(blk, r2, r0, flags)
    return flags


def precision_recall(f_real, f_fake, k=3, row_block=1024):
    """Improved precision and recall (Kynkaanniemi et al. 2019) of the generated features f_fake [m, D] against the real
    ones f_real [n, D] (fp32 on the GPU).  d2(a, b) = max(|a|^2 + |b|^2 - 2 a . b, 0) in fp64; r2_i = the k-th smallest
    d2 from row i to the other rows of its own set (self left out by index); a point is inside a set when it lies within
    r2_i of any row i (<=, squared distances throughout).  precision = the fraction of generated points inside the real
    set, recall = the fraction of real points inside the generated set.
    Row blocks of `row_block` rows go through one fp64 buffer [row_block, max(n, m)] that every pass reuses: the peak extra
    memory is that one block (105 MB at 12800 features and the default 1024 rows) plus norms, radii and flags; no n x m
    matrix exists at any time.  The flags of both passes come back in one copy."""
    import hip_backend as hb

    fr, ff = _dev_features(f_real), _dev_features(f_fake)
    n, m = fr.shape[0], ff.shape[0]
    k, row_block = int(k), int(row_block)
    assert row_block >= 1
    if not (1 <= k <= 8 and k < n and k < m):
        raise hb.StylexHipError("precision_recall: k = %d needs 1 <= k <= 8 and k below both set sizes (%d, %d)" % (k, n, m))
    row_block = min(row_block, max(n, m))
    block = torch.empty(row_block * max(n, m), dtype=torch.float64, device=fr.device)
    nr, nf = hb.feat_rownorm(fr), hb.feat_rownorm(ff)
    r2r = _radii2(fr, nr, k, row_block, block)
    r2f = _radii2(ff, nf, k, row_block, block)
    flags = torch.zeros(m + n, dtype=torch.uint8, device=fr.device)
    _inside(fr, nr, r2r, ff, nf, row_block, block, flags[:m])
    _inside(ff, nf, r2f, fr, nr, row_block, block, flags[m:])
    host = flags.cpu().numpy()
    return float(host[:m].mean(dtype=np.float64)), float(host[m:].mean(dtype=np.float64))


def save_features(path, feats, tag):
    """Real features beside real_stats.npz: `path` (.npy, fp32 [n, D]) and the tag in the sidecar `path`.tag."""
    path = str(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.save(path, feats.detach().cpu().numpy())
    with open(path + ".tag", "w") as f:
        f.write(str(tag))


def load_features(path, tag, device):
    """The features saved under `tag`, or None when a file is missing or was saved under another tag."""
    path = str(path)
    if not (os.path.isfile(path) and os.path.isfile(path + ".tag")):
        return None
    with open(path + ".tag") as f:
        if f.read() != str(tag):
            return None
    a = np.load(path, allow_pickle=False)
    if a.ndim != 2 or a.dtype != np.float32:
        return None
    return torch.from_numpy(a).to(device)
