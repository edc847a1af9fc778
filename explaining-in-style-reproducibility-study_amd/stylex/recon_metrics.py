"""Reconstruction fidelity of a StylEx checkpoint on held-out images: how far G(encoder(x), classifier(x)) is from x, as an
image (MAE, MSE, PSNR, SSIM, LPIPS) and as a decision (classifier KL, agreement, probability shift).  AttFind and the
counterfactual sweep explain the reconstruction, so these are the numbers that say whether they explain x.  The reference
has no such report (its training loop minimises L1, LPIPS and the KL, its evaluate() saves the `from_encoder` grid).

The image-pair metrics come from one fused kernel per batch (hip_backend.image_pair_stats, csrc/image_metrics.hip, DESIGN
§14); LPIPS and the classifier are the Trainer's own frozen networks.  summary() is a pure function of the per-image
arrays."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import hip_backend as hb

METRICS = ("mae", "mse", "psnr", "ssim", "lpips", "kl", "dp")  # per-image arrays, besides the boolean `agree`


class ReconEvaluator:
    """add(real_batch) reconstructs the batch through the EMA generator as Trainer.evaluate(encoder_input=True) builds w —
    encoder output with the classifier logits (default architecture) or with the soft-max probabilities (conditional
    one) for every layer — at truncation 1 with one fixed noise plane, and collects the per-image metrics."""

    def __init__(self, stylex, classifier, lpips, new_architecture=False, quantise=True, noise_seed=0):
        self.stylex, self.classifier, self.lpips = stylex, classifier, lpips
        self.new_architecture, self.quantise = bool(new_architecture), bool(quantise)
        self.noise_seed = int(noise_seed)
        self._noise = None
        self.arrays = {k: [] for k in METRICS + ("agree",)}

    def _noise_plane(self, n, device):
        if self._noise is None:
            size = self.stylex.G.image_size
            g = torch.Generator().manual_seed(self.noise_seed)
            self._noise = torch.rand(1, size, size, 1, generator=g).to(device)
        return self._noise.expand(n, -1, -1, -1)

    @torch.no_grad()
    def reconstruct(self, real, logits=None):
        m = self.stylex
        if logits is None:
            logits = self.classifier.classify_images(real)
        cond = F.softmax(logits, dim=1) if self.new_architecture else logits
        w = torch.cat((m.encoder(real), cond), dim=1)
        styles = w[:, None, :].expand(-1, m.G.num_layers, -1)
        return m.GE(styles, self._noise_plane(real.shape[0], real.device)).clamp_(0., 1.)

    @torch.no_grad()
    def add(self, real):
        from stylex_train import _frozen_layout, lpips_normalize

        self.stylex.eval()
        real_logits = self.classifier.classify_images(real)
        rec = self.reconstruct(real, real_logits)
        pair = hb.image_pair_stats(real, rec, channels=min(3, real.shape[1]), quantise=self.quantise)
        lp = self.lpips(_frozen_layout(lpips_normalize(real)), _frozen_layout(lpips_normalize(rec))).reshape(-1)
        terms = classifier_terms(real_logits, self.classifier.classify_images(rec))
        for k in ("mae", "mse", "psnr", "ssim"):
            self.arrays[k].append(getattr(pair, k).cpu().numpy())
        self.arrays["lpips"].append(lp.double().cpu().numpy())
        for k in ("kl", "dp", "agree"):
            self.arrays[k].append(terms[k].cpu().numpy())
        return rec

    def per_image(self):
        return {k: (np.concatenate(v) if v else np.zeros(0, dtype=bool if k == "agree" else np.float64))
                for k, v in self.arrays.items()}

    def summary(self):
        return summary(self.per_image())


def classifier_terms(real_logits, rec_logits):
    """Per image: kl — the training loss's term (ops._KLLogits: KLDivLoss(log_target=True)(log_softmax(rec),
    log_softmax(real)), i.e. sum_k p_real (log p_real - log p_rec)) before its batch mean; agree — the arg-max classes
    match; dp — |p_real - p_rec| at the real image's top class."""
    lr, lf = F.log_softmax(real_logits.float(), dim=1), F.log_softmax(rec_logits.float(), dim=1)
    kl = F.kl_div(lf, lr, reduction="none", log_target=True).sum(dim=1)
    top = lr.argmax(dim=1)
    dp = (lr.exp() - lf.exp()).abs().gather(1, top[:, None])[:, 0]
    return dict(kl=kl.double(), dp=dp.double(), agree=top == lf.argmax(dim=1))


def summary(per_image):
    """{metric: {mean, std, count}} for every per-image metric (population standard deviation), `agreement` (the rate of
    matching classifier decisions) and `psnr_infinite` (images reconstructed exactly: their infinite PSNR is left out of
    the PSNR mean, standard deviation and count, and reported here instead)."""
    out = {}
    for k in METRICS:
        v = np.asarray(per_image[k], dtype=np.float64)
        if k == "psnr":
            out["psnr_infinite"] = int(np.isinf(v).sum())
            v = v[~np.isinf(v)]
        out[k] = dict(mean=float(v.mean()) if v.size else math.nan, std=float(v.std()) if v.size else math.nan,
                      count=int(v.size))
    agree = np.asarray(per_image["agree"], dtype=bool)
    out["agreement"] = float(agree.mean()) if agree.size else math.nan
    out["images"] = int(agree.size)
    return out


def pair_summary(per_image):
    """summary() for the image-pair metrics alone (recon_cli.py --a DIR --b DIR: no model, no classifier)."""
    full = dict({k: np.zeros(0) for k in METRICS}, agree=np.zeros(0, dtype=bool), **per_image)
    s = summary(full)
    return dict({k: s[k] for k in ("mae", "mse", "psnr", "ssim", "psnr_infinite")}, images=int(len(per_image["mse"])))
