"""Frechet Inception Distance without image files (reference stylex/stylex_train.py:1577-1622 writes PNG / JPEG folders
and calls pytorch_fid on them): real and generated batches go from the loader / generator through ``stylex_fid_prep``,
the Inception network (fid_inception.py) and ``stylex_fid_moments_acc`` without leaving the GPU; only the two raw moments
(count, sum, upper triangle of the Gram matrix, fp64) come back to the host, where mean, covariance and the distance
are computed in fp64.  The reference's generated images are .jpg files: ``add_fake(batch, jpeg_quality=75)`` applies that
round trip on the device (``stylex_jpeg_roundtrip``) in front of the network.
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

    def __init__(self, net, input_size=299):
        self.net, self.input_size = net, int(input_size)
        self.real = self.fake = None

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

    def _add(self, stats, batch, jpeg_quality=None):
        fm = self.features(batch, jpeg_quality)
        if stats is None:
            stats = FIDStats(fm.shape[1], fm.device)
        stats.update(fm)
        return stats

    def add_real(self, batch):
        self.real = self._add(self.real, batch)

    def add_fake(self, batch, jpeg_quality=None):
        self.fake = self._add(self.fake, batch, jpeg_quality)

    def value(self):
        assert self.real is not None and self.fake is not None, "add_real and add_fake first"
        return frechet_distance(*self.real.mean_cov(), *self.fake.mean_cov())
