"""-m gpu: the device JPEG round trip (csrc/jpeg_rt.hip) bit for bit against its numpy definition (tests/_jpeg_defs.py, which
tests/test_jpeg_defs_cpu.py holds to Pillow's output), the byte-reading FID prep, FIDEvaluator's jpeg_quality and
Trainer.calculate_fid / cli.py with fid_jpeg."""
import functools
import itertools
import math
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

import _jpeg_defs as jd  # noqa: E402
import fid  # noqa: E402
import hip_backend as hb  # noqa: E402

DEV = "cuda:0"
LAYOUTS = ("f32_nchw", "bf16_channels_last", "four_channel_view")


@functools.lru_cache(maxsize=None)
def _float_images(B, h, w, kind, layout):
    """A float image batch on the host whose bytes are those of jd.content(kind): every value sits inside its quantisation
    cell, `saturated` images reach past [0, 1] (the clamp).  Returned in the layout's dtype with the layout's channels."""
    rng = np.random.RandomState(B * 7919 + h * 131 + w + len(kind))
    q = np.stack([jd.content(kind, h, w, seed=B * 1000 + h * 31 + w + i).transpose(2, 0, 1) for i in range(B)]).astype(np.float32)
    x = (q + (rng.rand(*q.shape).astype(np.float32) - 0.5) * 0.5) / 255
    if kind == "saturated":
        x = x * 1.2 - 0.1
    x = torch.from_numpy(x)
    if layout == "four_channel_view":  # four channels out of six, at a storage offset: only the first three are read
        x = torch.cat([torch.rand(B, 1, h, w), x, torch.rand(B, 2, h, w)], 1)
    elif layout == "bf16_channels_last":
        x = x.bfloat16()
    return x


def _on_device(x, layout):
    x = x.to(DEV)
    if layout == "four_channel_view":
        x = x[:, 1:5]
        assert x.shape[1] == 4 and x.storage_offset() > 0
    elif layout == "bf16_channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    return x


@functools.lru_cache(maxsize=None)
def _want(B, h, w, kind, layout, quality):
    x = _float_images(B, h, w, kind, layout)
    x = x[:, 1:4] if layout == "four_channel_view" else x
    return torch.from_numpy(jd.roundtrip_batch(jd.to_byte(x.float().numpy()), quality))


@pytest.mark.parametrize("h,w", [(8, 8), (16, 16), (24, 40), (19, 21), (33, 17), (18, 22), (64, 64)])
def test_roundtrip_equals_the_definition(h, w):
    checked = 0
    for B in (1, 3):
        for layout in LAYOUTS:
            for quality in (75, 10, 100):
                for kind in jd.KINDS:
                    got = hb.jpeg_roundtrip(_on_device(_float_images(B, h, w, kind, layout), layout), quality)
                    assert got.dtype == torch.uint8 and got.shape == (B, 3, h, w) and got.is_contiguous()
                    want = _want(B, h, w, kind, layout, quality)
                    assert torch.equal(got.cpu(), want), (B, layout, quality, kind, int((got.cpu() != want).sum()))
                    checked += 1
    assert checked == 54


@pytest.mark.parametrize("layout", LAYOUTS)
def test_roundtrip_equals_the_definition_at_256(layout):
    for kind, quality in (("noise", 75), ("smooth", 75), ("saturated", 100), ("smooth", 10)):
        got = hb.jpeg_roundtrip(_on_device(_float_images(2, 256, 256, kind, layout), layout), quality)
        assert torch.equal(got.cpu(), _want(2, 256, 256, kind, layout, quality)), (kind, quality)


def test_roundtrip_is_not_a_copy_and_repeats_bit_for_bit():
    x = _on_device(_float_images(3, 33, 17, "noise", "f32_nchw"), "f32_nchw")
    a, b = hb.jpeg_roundtrip(x, 75), hb.jpeg_roundtrip(x, 75)
    assert torch.equal(a, b)
    q = torch.from_numpy(jd.to_byte(x.cpu().numpy()))
    assert float((a.cpu() != q).float().mean()) > 0.9
    big = _on_device(_float_images(2, 256, 256, "smooth", "bf16_channels_last"), "bf16_channels_last")
    assert torch.equal(hb.jpeg_roundtrip(big, 75), hb.jpeg_roundtrip(big, 75))


@pytest.mark.parametrize("offset", [0, 1, 4])
def test_roundtrip_writes_between_its_guard_bands(offset):
    """19 x 21: ragged in both directions, the byte-store path; the output view starts `offset` bytes into its buffer."""
    B, h, w, band = 3, 19, 21, 512
    n = B * 3 * h * w
    buf = torch.full((band + offset + n + band,), 0xA5, dtype=torch.uint8, device=DEV)
    out = buf[band + offset:band + offset + n].view(B, 3, h, w)
    x = _on_device(_float_images(B, h, w, "noise", "f32_nchw"), "f32_nchw")
    hb.jpeg_roundtrip(x, 75, out=out)
    assert torch.equal(out.cpu(), _want(B, h, w, "noise", "f32_nchw", 75))
    host = buf.cpu()
    assert bool((host[:band + offset] == 0xA5).all()) and bool((host[band + offset + n:] == 0xA5).all())


def test_roundtrip_rejects_small_planes():
    with pytest.raises(hb.StylexHipError):
        hb.jpeg_roundtrip(torch.rand(1, 3, 4, 16, device=DEV))
    with pytest.raises(hb.StylexHipError):
        hb.jpeg_roundtrip(torch.rand(1, 3, 16, 16, device=DEV), quality=0)


@pytest.mark.parametrize("B,h,w", [(2, 8, 8), (3, 19, 21), (2, 64, 64), (1, 256, 256), (1, 320, 300)])
def test_prep_u8_equals_prep_of_the_float_image(B, h, w):
    """floor(fl(fl(q / 255) * 255) + 0.5) = q for every byte, so fid_prep of q / 255 sees the same bytes."""
    q = torch.randint(0, 256, (B, 3, h, w), generator=torch.Generator().manual_seed(h), dtype=torch.uint8)
    if (h, w) == (8, 8):
        q.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)  # every byte value
    q = q.to(DEV)
    got, want = hb.fid_prep_u8(q), hb.fid_prep(q.float() / 255)
    assert got.shape == (B, 3, 299, 299) and got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(hb.fid_prep_u8(q, 64), hb.fid_prep(q.float() / 255, 64))


# ---- FIDEvaluator ---------------------------------------------------------------------------------------------------------

class _StandIn(nn.Module):
    """Two conv layers: [B, 3, 299, 299] -> [B, 32, 36, 36]."""

    def __init__(self, seed=11):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.c1, self.c2 = nn.Conv2d(3, 16, 7, 4), nn.Conv2d(16, 32, 3, 2)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 / math.sqrt(max(p[0].numel(), 1))))
                p.requires_grad_(False)

    def forward(self, x):
        return F.relu(self.c2(F.relu(self.c1(x))))


def _decoded(x, quality=75):
    """The definition's decoded images of a float batch, as a float batch on the device."""
    q = jd.roundtrip_batch(jd.to_byte(x[:, :3].float().cpu().numpy()), quality)
    return (torch.from_numpy(q).float() / 255).to(DEV)


def test_evaluator_jpeg_quality():
    net = _StandIn().to(DEV)
    batches = [_on_device(_float_images(3, 24, 40, kind, "f32_nchw"), "f32_nchw") for kind in ("noise", "smooth")]
    a, b, plain, before = (fid.FIDEvaluator(net) for _ in range(4))
    for x in batches:
        a.add_fake(x, jpeg_quality=75)
        b.add_fake(_decoded(x, 75))
        plain.add_fake(x, jpeg_quality=None)
        before.add_fake(x)
        assert torch.equal(a.features(x, jpeg_quality=75), b.features(_decoded(x, 75)))
    assert a.fake.n == b.fake.n == 6
    assert torch.equal(a.fake.sum, b.fake.sum) and torch.equal(a.fake.gram, b.fake.gram)
    assert torch.equal(plain.fake.sum, before.fake.sum) and torch.equal(plain.fake.gram, before.fake.gram)
    assert not torch.equal(a.fake.sum, plain.fake.sum)
    # today's path is fid_prep, the network, the moments: nothing else
    want = fid.FIDStats(32, DEV)
    with torch.no_grad():
        for x in batches:
            want.update(net(hb.fid_prep(x, 299)))
    assert torch.equal(plain.fake.sum, want.sum) and torch.equal(plain.fake.gram, want.gram)


# ---- Trainer.calculate_fid, cli.py ------------------------------------------------------------------------------------------

@pytest.fixture
def deterministic_library(monkeypatch):
    """Two evaluations of one batch are compared bit for bit below.  The Inception convolutions run on the stock library,
    whose default algorithm choice is not reproducible run to run (the one noise source stylex_train.py names); cli.py's
    set_seed pins it as the reference does (cli.py:37), and so does this fixture for the duration of a test."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)


def _trainer(module, tmp_path, name, channels=3, **kw):
    from lpips_standin import LPIPSStandIn
    from standins import TinyClassifier

    dev = torch.device(DEV)
    tr = module.Trainer(name=name, base_dir=str(tmp_path), image_size=32, network_capacity=4, fmap_max=64, batch_size=8,
                        gradient_accumulate_every=1, classifier=TinyClassifier(seed=99).to(dev),
                        lpips_fn=LPIPSStandIn(seed=4242).to(dev), classifier_name="resnet", evaluate_every=10 ** 9,
                        save_every=10 ** 9, device=dev, tensorboard_dir=None, fid_weights="random:1", **kw)
    gen = torch.Generator().manual_seed(5)
    batches = [torch.rand(8, channels, 32, 32, generator=gen) for _ in range(2)]
    tr.loader = itertools.cycle(batches)
    tr.init_StylEx()
    return tr


def _fid_with_recorded_fakes(tr, seed):
    """calculate_fid(2) under `seed`, and the generated batches it scored."""
    rec, orig = [], tr.generate_truncated

    def spy(*a, **k):
        out = orig(*a, **k)
        rec.append(out.clone())
        return out

    tr.generate_truncated = spy
    try:
        torch.manual_seed(seed)
        value = tr.calculate_fid(2)
    finally:
        del tr.generate_truncated
    assert len(rec) == 2
    return value, rec


@pytest.mark.parametrize("arch", ["old", "new"])
def test_trainer_fid_jpeg(tmp_path, arch, deterministic_library):
    import stylex_train as st
    import stylex_train_new as stn

    torch.manual_seed(0)
    tr = _trainer(st if arch == "old" else stn, tmp_path, "j" + arch, fid_jpeg=True)
    assert tr.fid_jpeg is True and tr.image_extension == "jpg"
    assert math.isfinite(tr.calculate_fid(2))  # the real statistics and the truncation mean exist from here on
    v_on, fakes_on = _fid_with_recorded_fakes(tr, 3)
    tr.fid_jpeg = False
    v_off, fakes_off = _fid_with_recorded_fakes(tr, 3)
    assert all(torch.equal(a, b) for a, b in zip(fakes_on, fakes_off)), "the same seed did not give the same images"
    print("FID with the JPEG round trip %.10g, without %.10g" % (v_on, v_off))
    assert math.isfinite(v_on) and math.isfinite(v_off) and v_on != v_off
    ev = fid.FIDEvaluator(tr._fid_eval.net)
    ev.real = tr._fid_eval.real
    for x in fakes_on:
        assert x.shape == (8, 3, 32, 32)
        ev.add_fake(_decoded(x, 75))
    assert ev.value() == v_on


def test_trainer_fid_jpeg_leaves_transparent_models_alone(tmp_path, deterministic_library):
    import stylex_train as st

    torch.manual_seed(0)
    tr = _trainer(st, tmp_path, "t", channels=4, transparent=True, fid_jpeg=True)
    assert tr.image_extension == "png"
    assert math.isfinite(tr.calculate_fid(2))
    v_on, fakes_on = _fid_with_recorded_fakes(tr, 3)
    tr.fid_jpeg = False
    v_off, fakes_off = _fid_with_recorded_fakes(tr, 3)
    assert fakes_on[0].shape[1] == 4 and all(torch.equal(a, b) for a, b in zip(fakes_on, fakes_off))
    assert v_on == v_off


def test_cli_fid_jpeg_flag(tmp_path, monkeypatch):
    from PIL import Image

    import cli
    import ops

    data = tmp_path / "imgs"
    data.mkdir()
    rng = np.random.RandomState(0)
    for i in range(8):
        Image.fromarray(rng.randint(0, 255, (40, 40, 3), dtype=np.uint8)).save(data / f"{i}.png")
    made = []

    class Recording(cli.Trainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(cli, "Trainer", Recording)
    monkeypatch.setattr(sys, "argv", ["cli.py", "--data", str(data), "--results_dir", str(tmp_path / "results"), "--models_dir",
                                      str(tmp_path / "models"), "--name", "c", "--new", "--image_size", "32",
                                      "--network_capacity", "4", "--fmap_max", "64", "--batch_size", "4",
                                      "--gradient_accumulate_every", "1", "--num_train_steps", "2", "--num_workers", "0",
                                      "--save_every", "1000000", "--evaluate_every", "1000000", "--tensorboard_dir", "None",
                                      "--classifier_path", "None", "--calculate_fid_every", "1", "--calculate_fid_num_images", "8",
                                      "--fid_weights", "random:1", "--fid_jpeg"])
    try:
        cli.main()
    finally:
        ops.set_precision("fp32")
    assert len(made) == 1 and made[0].fid_jpeg is True
    lines = (tmp_path / "results" / "c" / "fid_scores.txt").read_text().splitlines()
    assert len(lines) == 1 and lines[0].startswith("1,") and math.isfinite(float(lines[0].split(",")[1]))
    assert cli.DEFAULTS["fid_jpeg"] is False
