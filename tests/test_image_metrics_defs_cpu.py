"""CPU checks of the image-pair statistics' definitions (tests/_image_metrics_defs.py): the fp64 definition against its own
separable form, closed forms and (where installed) scikit-image; the fp32 model of the kernel's passes, whose measured error
sets the SSIM limit of tests/test_image_metrics_gpu.py, and the mutations that limit tells apart; the derived bounds of the
|d| and d^2 sums; recon_metrics.summary on hand-made arrays."""
import math
import os

import numpy as np
import pytest
import torch

import _image_metrics_defs as D
import hip_backend as hb
import recon_metrics


def _tile():
    return hb.image_pair_tile()  # the built library's output tile extent (needs no device)


def _record(lines):
    """Print measured figures, and append them to $STYLEX_PROFILE_DIR/image_metrics_errors.txt where that variable names a
    folder (profiles/image_metrics_errors.txt is the record of one such run)."""
    out = os.environ.get("STYLEX_PROFILE_DIR")
    if out and os.path.isdir(out):
        with open(os.path.join(out, "image_metrics_errors.txt"), "a") as f:
            for line in lines:
                f.write(line + "\n")
    for line in lines:
        print(line)


# ---- the definition ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (2, 3, 20, 23), (1, 2, 37, 12)])
def test_separable_and_direct_forms_agree(shape):
    x, y = D.family_pair("noise", shape, 1)
    a, b = D.clamp_rule(x.numpy()), D.clamp_rule(y.numpy())
    direct, separable = D.ssim_map_direct(a, b), D.ssim_map_separable(a, b)
    assert direct.shape == shape[:2] + (shape[2] - 10, shape[3] - 10)
    assert float(np.abs(direct - separable).max()) <= 1e-12


def test_window_is_normalised_and_symmetric():
    g = D.gaussian()
    assert g.shape == (11,) and abs(g.sum() - 1.0) <= 1e-15 and np.array_equal(g, g[::-1])
    assert abs(g[5] / g[4] - math.exp(1.0 / (2 * 1.5 ** 2))) <= 1e-14


@pytest.mark.parametrize("quantise", [True, False])
def test_identical_images(quantise):
    x, _ = D.family_pair("outside", (3, 3, 17, 19), 2)
    s = D.pair_stats(x, x, 3, quantise)
    assert np.array_equal(s["ssim"], np.ones(3)) and np.array_equal(s["mse"], np.zeros(3)) and np.array_equal(s["mae"], np.zeros(3))
    assert np.all(np.isinf(s["psnr"])) and np.all(s["psnr"] > 0)


def test_constant_offset_closed_form():
    """Two constant images a and b: every (co)variance is 0, SSIM = (2 a b + C1) / (a^2 + b^2 + C1) at every position."""
    a, b = 0.25, 0.75  # exact in fp32; the clamp rule keeps them
    s = D.pair_stats(torch.full((2, 3, 15, 13), a), torch.full((2, 3, 15, 13), b), 3, quantise=False)
    want = (2 * a * b + D.C1) / (a * a + b * b + D.C1)
    assert float(np.abs(s["ssim"] - want).max()) <= 1e-12
    assert float(np.abs(s["mse"] - 0.25).max()) <= 1e-15 and float(np.abs(s["mae"] - 0.5).max()) <= 1e-15
    assert float(np.abs(s["psnr"] - 10 * math.log10(4.0)).max()) <= 1e-12


def test_byte_rule():
    v = np.array([-0.2, 0.0, 0.5 / 255, 0.499 / 255, 1.0, 1.3, 127.4 / 255, 127.6 / 255], dtype=np.float32)
    assert D.byte_rule(v).tolist() == [0.0, 0.0, 1.0, 0.0, 255.0, 255.0, 127.0, 128.0]
    assert D.clamp_rule(np.array([-1.0, 0.25, 2.0], dtype=np.float32)).tolist() == [0.0, 0.25, 1.0]


def test_against_scikit_image():
    metrics = pytest.importorskip("skimage.metrics")  # pinned only where the package is installed; nothing is installed for it
    x, y = D.family_pair("noise", (2, 3, 24, 31), 3)
    a, b = D.clamp_rule(x.numpy()), D.clamp_rule(y.numpy())
    want = D.ssim_map_direct(a, b).mean((1, 2, 3))
    for i in range(2):
        per_channel = []
        for c in range(3):
            _, full = metrics.structural_similarity(a[i, c], b[i, c], gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
                                                    data_range=1, full=True)
            per_channel.append(full[5:-5, 5:-5].mean())  # the package averages the same valid positions
        assert abs(np.mean(per_channel) - want[i]) <= 1e-9


# ---- the fp32 model and the SSIM limit ----------------------------------------------------------------------------------------

def test_model_error_sets_the_limit():
    tile = _tile()
    errors, limit = D.model_errors(tile), D.ssim_limit(tile)
    _record(["# tests/test_image_metrics_defs_cpu.py::test_model_error_sets_the_limit (tile %d, %d cases): worst per-image "
             "|SSIM of the fp32 model of the kernel's passes - SSIM of the fp64 definition|" % (tile, len(D.cases(tile)))]
            + ["model %-8s %.4g" % (f, errors[f]) for f in D.FAMILIES]
            + ["SSIM limit of the GPU test = 4 x the worst of them: %.4g" % limit,
               "derived: quantise = 0 sums of |d| and d^2 within relative 2^-22 = %.4g; quantise = 1 sums exact" % D.SUM_REL_BOUND])
    assert limit == 4.0 * max(errors.values()) and limit > 0.0
    # the cancellation in E[x^2] - mu^2 is a few ulps of 0.25 (1e-7) against C2 = 9e-4: an error above 1e-4 per image would
    # mean the model is not the definition's computation any more
    assert limit < 1e-4


def test_model_is_exact_on_identical_images():
    x, _ = D.family_pair("ramp", (2, 3, 27, 29), 4)
    for quantise in (True, False):
        assert np.array_equal(D.ssim_model_fp32(x, x, 3, quantise), np.ones(2))


@pytest.mark.parametrize("mutation", D.MUTATIONS)
def test_mutations_exceed_the_limit(mutation):
    tile = _tile()
    limit, worst = D.ssim_limit(tile), 0.0
    for _, _, quantise, channels, x, y in D.cases(tile):
        want = D.pair_stats(x, y, channels, quantise)["ssim"]
        got = D.ssim_model_fp32(x, y, channels, quantise, tile, mutation=mutation)
        worst = max(worst, float(np.abs(got - want).max()))
    print("%s: worst error %.4g, limit %.4g" % (mutation, worst, limit))
    assert worst > limit


# ---- derived bounds of the difference sums --------------------------------------------------------------------------------------

def test_sum_bounds():
    """quantise = 0: d = x - y, |d| and d * d in fp32 (one rounding in |d|, three in d^2: (1 + e)^2 (1 + e')), added in fp64:
    within relative 2^-22 of the definition, every term being non-negative.  quantise = 1: the byte differences and their
    squares (below 2^16) are exact in fp32."""
    for _, _, quantise, channels, x, y in D.cases(_tile()):
        a, b = D._f32(x, channels), D._f32(y, channels)
        want = D.pair_stats(x, y, channels, quantise)
        if quantise:
            d = D.byte_rule(a).astype(np.float32) - D.byte_rule(b).astype(np.float32)
        else:
            d = D.clamp_rule(a).astype(np.float32) - D.clamp_rule(b).astype(np.float32)
        assert d.dtype == np.float32
        got_abs, got_sq = np.abs(d).astype(np.float64).sum((1, 2, 3)), (d * d).astype(np.float64).sum((1, 2, 3))
        if quantise:
            assert np.array_equal(got_abs, want["sum_abs"]) and np.array_equal(got_sq, want["sum_sq"])
        else:
            assert np.all(np.abs(got_abs - want["sum_abs"]) <= D.SUM_REL_BOUND * want["sum_abs"])
            assert np.all(np.abs(got_sq - want["sum_sq"]) <= D.SUM_REL_BOUND * want["sum_sq"])


# ---- recon_metrics.summary --------------------------------------------------------------------------------------------------

def test_summary_of_hand_made_arrays():
    per_image = dict(mae=[0.1, 0.2, 0.0, 0.3], mse=[0.01, 0.04, 0.0, 0.09], psnr=[20.0, 14.0, math.inf, 11.0],
                     ssim=[0.9, 0.8, 1.0, 0.5], lpips=[0.2, 0.4, 0.0, 0.6], kl=[0.0, 0.1, 0.0, 0.3], dp=[0.0, 0.05, 0.0, 0.55],
                     agree=[True, True, True, False])
    s = recon_metrics.summary(per_image)
    assert s["images"] == 4 and s["agreement"] == 0.75 and s["psnr_infinite"] == 1
    assert s["psnr"]["count"] == 3 and s["psnr"]["mean"] == pytest.approx(15.0) and math.isfinite(s["psnr"]["std"])
    assert s["psnr"]["std"] == pytest.approx(np.std([20.0, 14.0, 11.0]))
    assert s["ssim"] == dict(mean=pytest.approx(0.8), std=pytest.approx(np.std([0.9, 0.8, 1.0, 0.5])), count=4)
    assert s["mse"]["mean"] == pytest.approx(0.035) and s["mae"]["mean"] == pytest.approx(0.15)
    assert s["lpips"]["mean"] == pytest.approx(0.3) and s["kl"]["mean"] == pytest.approx(0.1) and s["dp"]["count"] == 4


def test_summary_when_every_psnr_is_infinite():
    per_image = {k: [0.0, 0.0] for k in recon_metrics.METRICS}
    per_image.update(psnr=[math.inf, math.inf], ssim=[1.0, 1.0], agree=[True, True])
    s = recon_metrics.summary(per_image)
    assert s["psnr_infinite"] == 2 and s["psnr"]["count"] == 0 and math.isnan(s["psnr"]["mean"])
    assert s["agreement"] == 1.0 and s["ssim"]["mean"] == 1.0
    p = recon_metrics.pair_summary(dict(mae=[0.0], mse=[0.0], psnr=[math.inf], ssim=[1.0]))
    assert p["images"] == 1 and p["psnr_infinite"] == 1 and p["ssim"]["mean"] == 1.0 and set(p) == {"mae", "mse", "psnr", "ssim",
                                                                                                   "psnr_infinite", "images"}


def test_classifier_terms_follow_the_training_loss():
    """kl: the per-image term of ops.kl_logits' composition (its batch mean is the loss); agree and dp by hand."""
    import torch.nn.functional as F

    real = torch.tensor([[2.0, 0.0], [0.0, 1.0], [0.3, 0.1]])
    rec = torch.tensor([[1.0, 0.0], [0.5, 0.0], [0.3, 0.1]])
    t = recon_metrics.classifier_terms(real, rec)
    loss = F.kl_div(F.log_softmax(rec, dim=1), F.log_softmax(real, dim=1), reduction="batchmean", log_target=True)
    assert float(t["kl"].mean()) == pytest.approx(float(loss), rel=1e-6)
    assert t["agree"].tolist() == [True, False, True]
    p_real, p_rec = F.softmax(real, dim=1), F.softmax(rec, dim=1)
    want = [abs(float(p_real[0, 0] - p_rec[0, 0])), abs(float(p_real[1, 1] - p_rec[1, 1])), 0.0]
    assert t["dp"].tolist() == pytest.approx(want, abs=1e-6)
    assert float(t["kl"][2]) == 0.0


# ---- recon_cli: pairing by name -------------------------------------------------------------------------------------------------

def test_recon_cli_pairs_by_name_and_lists_unpaired(tmp_path):
    import recon_cli

    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    for name in ("1.png", "2.png", "only_a.png", "notes.txt"):
        (a / name).write_bytes(b"")
    for name in ("1.jpg", "2.png", "only_b.bmp", "other_b.png"):
        (b / name).write_bytes(b"")
    with pytest.raises(SystemExit) as err:
        recon_cli.paired_files(str(a), str(b))
    assert all(n in str(err.value) for n in ("only_a", "only_b", "other_b")) and "notes" not in str(err.value)
    (a / "only_a.png").unlink()
    (b / "only_b.bmp").unlink()
    (b / "other_b.png").unlink()
    assert recon_cli.paired_files(str(a), str(b)) == [(str(a / "1.png"), str(b / "1.jpg")), (str(a / "2.png"), str(b / "2.png"))]
    with pytest.raises(SystemExit, match="--a and --b"):
        recon_cli.main(["--a", str(a)])
