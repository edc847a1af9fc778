"""-m gpu: the image-pair statistics kernel (csrc/image_metrics.hip, hip_backend.image_pair_stats) against its fp64
definition (tests/_image_metrics_defs.py) evaluated on the same input tensors — exact cases bit for bit, SSIM within 4 x the
measured error of the fp32 model of the kernel's passes (measured against the definition on the CPU, never against the
kernel), the quantise = 0 sums within the derived 2^-22 — then its refusals, Trainer.evaluate_reconstruction end to end and
recon_cli.py on a folder against itself.  One run on an MI355X (profiles/image_metrics_errors.txt): worst SSIM error 8.5e-7
(noise), 1.9e-6 (ramp), 2.6e-7 (outside) — the model's own figures — against the limit 7.5e-6; quantise = 0 d^2 sums within
7.2e-9 of the definition (bound 2.4e-7), |d| sums and all byte sums exact."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _image_metrics_defs as D  # noqa: E402
import hip_backend as hb  # noqa: E402
import recon_metrics  # noqa: E402

DEV = "cuda:0"


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


def _on_device(t):
    """The CPU tensor on the device with the same sizes, strides and storage offset (a plain .to() would make a sliced view
    dense)."""
    n = t.untyped_storage().nbytes() // t.element_size()
    out = torch.zeros(n, dtype=t.dtype, device=DEV).as_strided(t.shape, t.stride(), t.storage_offset())
    out.copy_(t)
    assert out.stride() == t.stride() and out.storage_offset() == t.storage_offset()
    return out


def _stats(x, y, channels, quantise):
    sums = hb.image_pair_sums(x, y, channels, quantise)
    assert sums.shape == (x.shape[0], 3) and sums.dtype == torch.float64 and sums.is_contiguous()
    pair = hb.image_pair_stats(x, y, channels, quantise)
    return sums.cpu().numpy(), {k: getattr(pair, k).cpu().numpy() for k in pair._fields}


# ---- per-element cases --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", D.FAMILIES)
def test_against_the_definition(family):
    tile = hb.image_pair_tile()
    limit = D.ssim_limit(tile)
    worst_ssim, worst_abs, worst_sq, seen = 0.0, 0.0, 0.0, set()
    for fam, kind, quantise, channels, x, y in D.cases(tile):
        if fam != family:
            continue
        want = D.pair_stats(x, y, channels, quantise)
        xd, yd = _on_device(x), _on_device(y)
        if kind == "sliced":
            # a view of every second image and planes 1.. of a larger tensor: offset, batch stride twice the parent's
            assert xd.storage_offset() > 0 and xd.stride(0) == 2 * (xd.shape[1] + 1) * xd.stride(1)
            assert xd.shape[0] == 1 or not xd.is_contiguous()
        if kind == "f32_bf16cl":
            assert yd.dtype == torch.bfloat16 and xd.dtype == torch.float32 and (yd.stride(1) == 1 or yd.shape[1] == 1)
        sums, got = _stats(xd, yd, channels, quantise)
        seen.add((tuple(x.shape), channels, kind, quantise))
        e_ssim = float(np.abs(got["ssim"] - want["ssim"]).max())
        rel = lambda a, b: float((np.abs(a - b) / np.where(b > 0, b, 1.0)).max())  # noqa: E731
        e_abs, e_sq = rel(sums[:, 0], want["sum_abs"]), rel(sums[:, 1], want["sum_sq"])
        print("%-7s %-10s quantise %d %s channels %d: SSIM error %.3g (limit %.3g), sum |d| rel %.3g, sum d^2 rel %.3g"
              % (family, kind, quantise, tuple(x.shape), channels, e_ssim, limit, e_abs, e_sq))
        worst_ssim = max(worst_ssim, e_ssim)
        if quantise:
            assert np.array_equal(sums[:, 0], want["sum_abs"]) and np.array_equal(sums[:, 1], want["sum_sq"])
        else:
            worst_abs, worst_sq = max(worst_abs, e_abs), max(worst_sq, e_sq)
            assert e_abs <= D.SUM_REL_BOUND and e_sq <= D.SUM_REL_BOUND
        assert e_ssim <= limit
        # the record's other fields follow from the sums on the host, in fp64
        assert np.allclose(got["mae"], want["mae"], rtol=1e-6, atol=0) and np.allclose(got["mse"], want["mse"], rtol=1e-6, atol=0)
        assert np.allclose(got["psnr"], want["psnr"], rtol=0, atol=1e-5)
    assert len(seen) == 16  # five small shapes in one operand form each, 64 px in all three; both value rules
    _record(["# tests/test_image_metrics_gpu.py::test_against_the_definition[%s]: worst over %d cases" % (family, len(seen)),
             "gpu   %-8s SSIM error %.4g (limit %.4g); quantise = 0: sum |d| rel %.4g, sum d^2 rel %.4g (bound %.4g)"
             % (family, worst_ssim, limit, worst_abs, worst_sq, D.SUM_REL_BOUND)])


# ---- exact cases ----------------------------------------------------------------------------------------------------------------

def _byte_images(shape, seed):
    """Images whose bytes do not depend on how x * 255 + 0.5 is rounded: every value sits in the middle half of its cell."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, shape, generator=g).float()
    return (q + (torch.rand(shape, generator=g) - 0.5) * 0.5) / 255, q


@pytest.mark.parametrize("shape", [(1, 3, 11, 11), (5, 3, 25, 27), (2, 4, 43, 11), (1, 3, 64, 64)])
def test_byte_sums_are_exact(shape):
    (x, qx), (y, qy) = _byte_images(shape, 1), _byte_images(shape, 2)
    channels = min(shape[1], 3)
    d = (qx - qy)[:, :channels].double()
    sums = hb.image_pair_sums(x.to(DEV), y.to(DEV), channels, quantise=True).cpu()
    assert torch.equal(sums[:, 0], d.abs().sum((1, 2, 3))) and torch.equal(sums[:, 1], (d * d).sum((1, 2, 3)))
    want = D.pair_stats(x, y, channels, True)
    assert torch.equal(sums[:, 0], torch.from_numpy(want["sum_abs"])) and torch.equal(sums[:, 1], torch.from_numpy(want["sum_sq"]))


@pytest.mark.parametrize("quantise", [True, False])
@pytest.mark.parametrize("shape", [(1, 1, 11, 12), (5, 3, 11, 26), (1, 4, 25, 27), (2, 3, 64, 64)])
def test_identical_operands_give_exactly_one(shape, quantise):
    x = D.family_pair("outside", shape, 7)[0].to(DEV)
    sums, got = _stats(x, x, shape[1], quantise)
    assert np.array_equal(sums[:, :2], np.zeros((shape[0], 2)))
    assert np.array_equal(sums[:, 2], np.full(shape[0], float(shape[1] * (shape[2] - 10) * (shape[3] - 10))))
    assert np.array_equal(got["ssim"], np.ones(shape[0])) and np.array_equal(got["mse"], np.zeros(shape[0]))
    assert np.all(np.isinf(got["psnr"])) and np.all(got["psnr"] > 0)


def test_bf16_copy_with_the_same_bytes_gives_exactly_one():
    x = D.family_pair("noise", (3, 3, 30, 41), 8)[0].bfloat16().float()  # fp32 holding values a bf16 copy keeps
    y = x.bfloat16().contiguous(memory_format=torch.channels_last)
    assert np.array_equal(D.byte_rule(x.numpy()), D.byte_rule(y.float().numpy()))
    _, got = _stats(_on_device(x), _on_device(y), 3, True)
    assert np.array_equal(got["ssim"], np.ones(3)) and np.array_equal(got["mse"], np.zeros(3))


def test_two_launches_are_bit_identical():
    x, y = D.family_pair("noise", (5, 3, 64, 64), 9)
    x, y = x.to(DEV), y.to(DEV).bfloat16().contiguous(memory_format=torch.channels_last)
    for quantise in (True, False):
        a = hb.image_pair_sums(x, y, 3, quantise)
        other = hb.image_pair_sums(y, x, 3, not quantise)  # other work in between
        b = hb.image_pair_sums(x, y, 3, quantise)
        assert torch.equal(a, b) and not torch.equal(a, other)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals():
    lib = hb.load_library()
    x = torch.rand(2, 3, 16, 16, device=DEV)
    with pytest.raises(hb.StylexHipError, match="at least 11"):
        hb.image_pair_stats(x[:, :, :10], x[:, :, :10])
    with pytest.raises(hb.StylexHipError, match="at least 11"):
        hb.image_pair_stats(x[:, :, :, :10], x[:, :, :, :10])
    with pytest.raises(hb.StylexHipError, match="channels"):
        hb.image_pair_stats(torch.rand(2, 5, 16, 16, device=DEV), torch.rand(2, 5, 16, 16, device=DEV), channels=5)
    with pytest.raises(hb.StylexHipError, match="channels"):
        hb.image_pair_stats(x, x, channels=4)  # more than the operands hold
    with pytest.raises(hb.StylexHipError, match="batch"):
        hb.image_pair_stats(x, x[:1])
    with pytest.raises(hb.StylexHipError, match="GPU tensor"):
        hb.image_pair_stats(x.cpu(), x.cpu())
    with pytest.raises(hb.StylexHipError, match="GPU tensor"):
        hb.image_pair_stats(x, x.cpu())
    # the C entry points themselves: the query and the call refuse before anything is launched
    assert lib.stylex_image_pair_stats_workspace_bytes(2, 3, 10, 16) == -1
    assert lib.stylex_image_pair_stats_workspace_bytes(2, 5, 16, 16) == -1
    assert lib.stylex_image_pair_stats_workspace_bytes(2, 3, 16, 16) == 2 * 3 * 1 * 3 * 8
    out = torch.full((2, 3), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(64, dtype=torch.float64, device=DEV)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    st = i64(*x.stride())
    call = lambda sh, nbytes: lib.stylex_image_pair_stats(x.data_ptr(), x.data_ptr(), out.data_ptr(), sh, st, st, 0, 0, 1,  # noqa: E731
                                                          ws.data_ptr(), nbytes, None)
    assert call(i64(2, 3, 10, 16), 512) == -1 and call(i64(2, 5, 16, 16), 512) == -1 and call(i64(2, 3, 16, 16), 8) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---- end to end -----------------------------------------------------------------------------------------------------------------

class _Loader:
    def __init__(self, batches):
        self.batches, self.taken = batches, 0

    def __iter__(self):
        return self

    def __next__(self):
        self.taken += 1
        return self.batches[(self.taken - 1) % len(self.batches)]


def _trainer(module, tmp_path, name):
    from lpips_standin import LPIPSStandIn
    from standins import TinyClassifier

    dev = torch.device(DEV)
    tr = module.Trainer(name=name, base_dir=str(tmp_path), image_size=32, network_capacity=4, fmap_max=64, batch_size=4,
                        gradient_accumulate_every=1, classifier=TinyClassifier(seed=99).to(dev),
                        lpips_fn=LPIPSStandIn(seed=4242).to(dev), classifier_name="resnet", evaluate_every=10 ** 9,
                        save_every=10 ** 9, device=dev, tensorboard_dir=None)
    gen = torch.Generator().manual_seed(5)
    tr.loader = _Loader([torch.rand(4, 3, 32, 32, generator=gen) for _ in range(2)])
    return tr


@pytest.mark.parametrize("arch", ["default", "conditional"])
def test_trainer_evaluate_reconstruction(tmp_path, monkeypatch, arch):
    import importlib

    module = importlib.import_module("stylex_train" if arch == "default" else "stylex_train_new")
    torch.manual_seed(0)
    tr = _trainer(module, tmp_path, "r")
    tr.init_StylEx()
    pairs, add = [], recon_metrics.ReconEvaluator.add

    def recording_add(self, real):
        rec = add(self, real)
        pairs.append((real.clone(), rec.clone()))
        return rec

    monkeypatch.setattr(recon_metrics.ReconEvaluator, "add", recording_add)
    s = tr.evaluate_reconstruction(1)
    assert tr.loader.taken == 1 and len(pairs) == 1 and s["images"] == 4
    for k in recon_metrics.METRICS:
        assert s[k]["count"] + (s["psnr_infinite"] if k == "psnr" else 0) == 4
        assert math.isfinite(s[k]["mean"]) and math.isfinite(s[k]["std"]), k
    assert 0.0 <= s["agreement"] <= 1.0 and s["kl"]["mean"] >= 0.0 and -1.0 <= s["ssim"]["mean"] <= 1.0
    folder = tmp_path / "results" / "r"
    lines = (folder / "recon_scores.txt").read_text().splitlines()
    assert len(lines) == 1 and lines[0].startswith("0,") and json.loads(lines[0].split(",", 1)[1]) == s
    arrays = np.load(str(folder / "recon_0.npz"))
    assert set(arrays.files) == set(recon_metrics.METRICS) | {"agree"} and all(arrays[k].shape == (4,) for k in arrays.files)
    real, rec = pairs[0]
    assert rec.shape == real.shape and float(rec.min()) >= 0.0 and float(rec.max()) <= 1.0
    direct = hb.image_pair_stats(real, rec, channels=3, quantise=True)
    assert np.array_equal(arrays["ssim"], direct.ssim.cpu().numpy()) and np.array_equal(arrays["mse"], direct.mse.cpu().numpy())
    want = D.pair_stats(real, rec, 3, True)  # and the definition, on the bytes of both batches
    assert np.array_equal(arrays["mse"], want["mse"])
    assert float(np.abs(arrays["ssim"] - want["ssim"]).max()) <= D.ssim_limit(hb.image_pair_tile())
    assert s["ssim"]["mean"] == pytest.approx(float(arrays["ssim"].mean()), rel=1e-12)
    tr.evaluate_reconstruction(1, quantise=False)  # a second call appends a second line
    assert len((folder / "recon_scores.txt").read_text().splitlines()) == 2


def test_recon_cli_folder_against_itself(tmp_path, capsys):
    from PIL import Image

    import recon_cli

    d = tmp_path / "d"
    d.mkdir()
    rng = np.random.RandomState(3)
    for i, (h, w) in enumerate(((24, 32), (24, 32), (32, 32), (32, 32))):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(d / ("%02d.png" % i))
    (d / "notes.txt").write_text("not an image")
    out = recon_cli.main(["--a", str(d), "--b", str(d), "--batch", "3", "--out", str(tmp_path / "same.json")])
    assert out["images"] == 4 and out["psnr_infinite"] == 4 and out["psnr"]["count"] == 0
    assert out["ssim"] == dict(mean=1.0, std=0.0, count=4)
    assert out["mse"] == dict(mean=0.0, std=0.0, count=4) and out["mae"] == dict(mean=0.0, std=0.0, count=4)
    assert json.loads((tmp_path / "same.json").read_text())["ssim"]["mean"] == 1.0
    # against a darker copy (saved under other extensions' stems): the definition on the decoded bytes
    e = tmp_path / "e"
    e.mkdir()
    for f in sorted(os.listdir(d)):
        if f.endswith(".png"):
            with Image.open(d / f) as im:
                Image.fromarray((np.asarray(im) * 0.8).astype(np.uint8)).save(e / f.replace(".png", ".bmp"))
    per_image = recon_cli.folder_pair_metrics(str(d), str(e), batch=4)
    for i, f in enumerate(sorted(x for x in os.listdir(d) if x.endswith(".png"))):
        with Image.open(d / f) as im:
            a = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1)[None].float() / 255
        with Image.open(e / f.replace(".png", ".bmp")) as im:
            b = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1)[None].float() / 255
        want = D.pair_stats(a, b, 3, True)
        assert per_image["mse"][i] == want["mse"][0]
        assert abs(per_image["ssim"][i] - want["ssim"][0]) <= D.ssim_limit(hb.image_pair_tile())
    (e / "extra.png").write_bytes((d / "00.png").read_bytes())
    with pytest.raises(SystemExit, match="extra"):
        recon_cli.main(["--a", str(d), "--b", str(e)])
