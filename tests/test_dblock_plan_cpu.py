"""ops._dblock_plan: the one place that decides how a fused DiscriminatorBlock runs, against the rules written out here
case by case (not imported from the code under test).  No GPU and no kernel library: the two library probes are stubs."""
import glob
import math
import os

import pytest
import torch

import hip_backend as hb
import ops

SWITCHES = ("STYLEX_PAD_RGB", "STYLEX_RES_GEMM", "STYLEX_RES_FOLD", "STYLEX_GATE_MASK", "STYLEX_GATE_MASK_MIN_PIXELS",
            "STYLEX_WGRAD_BIAS")
B = 3
# (cin, cout, pixels, downsample) -> space-to-depth tail in the bf16 modes: 64 | cout, even size, at least 16 px after
# the stride.  The fp32 mode never takes it.
CASES = {(3, 64, 64, True): True, (64, 64, 64, True): True, (64, 128, 32, True): True,
         (32, 48, 16, True): False,   # 48 is no multiple of 64
         (64, 64, 8, True): False,    # 4 px after the stride
         (64, 64, 2, False): False}   # no stride-2 tail at all


def yes(*a):
    return True


def no(*a):
    return False


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def plan(case, prec, probe=yes, blur=yes, cuda=True, dtype=torch.float32):
    cin, cout, px, down = case
    shapes = [(cout, cin, 1, 1), (cout, cin, 3, 3), (cout, cout, 3, 3), (cout, cout, 3, 3) if down else None]
    return ops._dblock_plan((B, cin, px, px), dtype, cuda, shapes, down, prec, probe, blur)


@pytest.mark.parametrize("prec", [hb.BF16_ACT, hb.BF16, hb.F32])
@pytest.mark.parametrize("case", list(CASES))
def test_plan_against_the_rules_case_by_case(case, prec):
    cin, cout, px, down = case
    p = plan(case, prec)
    bf16 = prec == hb.BF16_ACT
    s2d = CASES[case] and prec != hb.F32
    assert (p.cin, p.downsample, p.prec) == (cin, down, prec)
    assert p.c == 1 / math.sqrt(2)
    assert p.s2d == s2d
    assert p.alg == (down and prec != hb.F32)
    assert p.res_gemm == bf16                       # hipBLASLt GEMM: the bf16-activation mode only
    assert p.wgrad_bias is True
    assert p.mask1 is False and p.mask2 is False    # every case is below 128^2
    # RGB: one 16-byte slot = 8 bf16 or 4 fp32 channels; the one-pass kernel serves the bf16-activation mode
    want_pad = (None, 0) if cin != 3 else (("pad_rgb8", 5) if bf16 else ("_pad_rgb", 1))
    assert (p.pad, p.extra) == want_pad
    # with a probe that accepts everything the fold is decided by the block alone: s2d tail, GEMM residual, and the
    # (padded) input channels a multiple of 8 — true of every listed case
    assert p.fold_res == (s2d and bf16)
    assert not p.fold_res or p.s2d


def test_fold_res_implies_s2d_where_the_probe_alone_would_accept():
    """64 -> 64 at 8 px, bf16: even size, 64 | cout, 8 | cin, GEMM residual — everything the fold used to ask for — but
    no space-to-depth tail to consume it; the probe is not even asked."""
    asked = []
    p = plan((64, 64, 8, True), hb.BF16_ACT, probe=lambda *a: asked.append(a) or True)
    assert not p.s2d and not p.fold_res and not asked


def test_probe_sees_the_space_to_depth_shape_and_can_refuse():
    asked = []
    p = plan((3, 64, 64, True), hb.BF16_ACT, probe=lambda *a: asked.append(a) or True)
    assert p.fold_res and asked == [((B, 4 * 64, 32, 32), 64, 64, 8)]  # (xb shape, N of conv_res, C of y2, padded cin)
    assert not plan((3, 64, 64, True), hb.BF16_ACT, probe=no).fold_res


@pytest.mark.parametrize("switch,field,case", [("STYLEX_RES_GEMM", "res_gemm", (64, 64, 64, True)),
                                               ("STYLEX_RES_GEMM", "fold_res", (64, 64, 64, True)),
                                               ("STYLEX_RES_FOLD", "fold_res", (64, 64, 64, True)),
                                               ("STYLEX_GATE_MASK", "mask1", (64, 64, 128, True)),
                                               ("STYLEX_GATE_MASK", "mask2", (64, 64, 128, True)),
                                               ("STYLEX_WGRAD_BIAS", "wgrad_bias", (64, 64, 64, True))])
def test_switch_set_to_0_turns_its_field_off(switch, field, case, monkeypatch):
    assert getattr(plan(case, hb.BF16_ACT), field) is True
    monkeypatch.setenv(switch, "0")
    assert getattr(plan(case, hb.BF16_ACT), field) is False
    monkeypatch.setenv(switch, "1")
    assert getattr(plan(case, hb.BF16_ACT), field) is True


def test_rgb_padding_routes(monkeypatch):
    rgb = (3, 64, 64, True)
    assert plan(rgb, hb.BF16_ACT).pad == "pad_rgb8"
    assert plan(rgb, hb.BF16_ACT, dtype=torch.bfloat16).pad == "pad_rgb8"
    for kw in (dict(cuda=False), dict(dtype=torch.float16)):  # what the one-pass kernel does not read
        p = plan(rgb, hb.BF16_ACT, **kw)
        assert (p.pad, p.extra) == ("_pad_rgb", 5)
    monkeypatch.setenv("STYLEX_PAD_RGB", "0")
    p = plan(rgb, hb.BF16_ACT)
    assert (p.pad, p.extra) == ("_pad_rgb", 5) and p.fold_res  # same 8 channels either way


def test_masks(monkeypatch):
    c64, c128 = (64, 64, 64, True), (64, 64, 128, True)
    assert not plan(c64, hb.BF16_ACT).mask1 and plan(c128, hb.BF16_ACT).mask1  # from 128^2 up by default
    assert not plan(c128, hb.F32).mask1 and not plan(c128, hb.BF16).mask1       # bf16 activations only
    monkeypatch.setenv("STYLEX_GATE_MASK_MIN_PIXELS", "0")
    p = plan(c64, hb.BF16_ACT)
    assert p.mask1 and p.mask2
    # mask2: the blur adjoint must be able to read it (asked with y2's shape and dtype), and only the s2d tail does
    asked = []
    assert not plan(c64, hb.BF16_ACT, blur=lambda *a: asked.append(a) and False).mask2
    assert asked == [((B, 64, 64, 64), torch.bfloat16)]
    for case in ((32, 48, 16, True), (64, 64, 8, True), (64, 64, 2, False)):
        p = plan(case, hb.BF16_ACT)
        assert p.mask1 and not p.s2d and not p.mask2


def test_probes_default_to_the_backend():
    d = ops._dblock_plan.__defaults__
    assert d == (hb.s2d_res_supported, hb.blur_mask_ok)


def test_companion_stream_switch_is_gone():
    here = os.path.dirname(os.path.abspath(ops.__file__))
    for path in glob.glob(os.path.join(here, "**", "*.py"), recursive=True):
        with open(path) as f:
            assert "STYLEX_DBLOCK_SIDE" not in f.read(), path
