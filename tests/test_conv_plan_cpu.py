"""ops._conv_plan: the one place that decides how a plain conv call (ops.conv2d, ops.blur_down) runs, against the rules
written out here case by case (not imported from the code under test).  No GPU and no kernel library."""
import inspect
import re

import pytest
import torch

import hip_backend as hb
import ops

SWITCHES = ("STYLEX_RES_GEMM", "STYLEX_RES_GEMM_DD")
PRECS = [hb.F32, hb.BF16, hb.BF16_ACT]
ADT = {hb.F32: torch.float32, hb.BF16: torch.float32, hb.BF16_ACT: torch.bfloat16}   # activation dtype of each mode
# blur_down form (B, C, N, H, W) -> (the rule it shares with the fused block: 64 | C, even size, at least 16 px after the
# stride; this form's own 4 | N).  Space-to-depth where both hold, outside the fp32 mode.
BLUR_CASES = {(1, 64, 64, 32, 32): (True, True),
              (2, 64, 64, 16, 16): (False, True),    # half-resolution side 8 < 16
              (1, 96, 64, 32, 32): (False, True),    # 96 is no multiple of 64
              (1, 64, 66, 32, 32): (True, False),    # N = 66
              (1, 128, 64, 48, 80): (True, True),
              (1, 64, 64, 33, 32): (False, True)}    # odd height


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def plan(case, k, stride, pad, prec, fast, blurred=False):
    B, C, N, H, W = case
    return ops._conv_plan((B, C, H, W), ADT[prec], (N, C, k, k), stride, pad, prec, fast, blurred)


def launch(stride, pad, s2d=0, gemm=False):
    return (stride, pad, s2d, gemm)


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("prec", PRECS)
def test_conv3x3_takes_the_fused_or_the_composable_function(prec, fast):
    p = plan((2, 16, 16, 9, 9), 3, 1, 1, prec, fast)       # the bias + lrelu layer of a block
    assert p == (0, False, False, "fused" if fast else "composable", launch(1, 1))
    assert len(p) == 5 and len(p.launch) == 4              # every field is asserted above


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("prec", PRECS)
def test_conv1x1_is_a_gemm_only_on_the_composable_route_in_the_bf16_mode(prec, fast, monkeypatch):
    gemm = prec == hb.BF16_ACT and not fast
    p = plan((2, 16, 32, 8, 8), 1, 1, 0, prec, fast)
    assert p == (0, False, False, "fused" if fast else "composable", launch(1, 0, gemm=gemm))
    assert not (p.route == "fused" and p.launch.gemm)
    assert not plan((2, 16, 32, 8, 8), 1, 1, 1, prec, fast).launch.gemm      # padded 1x1: no plain GEMM
    for switch in SWITCHES:                                 # each switch alone turns it off, and nothing else
        monkeypatch.setenv(switch, "0")
        assert plan((2, 16, 32, 8, 8), 1, 1, 0, prec, fast) == p._replace(launch=p.launch._replace(gemm=False))
        monkeypatch.setenv(switch, "1")
        assert plan((2, 16, 32, 8, 8), 1, 1, 0, prec, fast) == p
        monkeypatch.delenv(switch)


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("prec", PRECS)
def test_conv1x1_stride2_gathers_the_even_pixels_first(prec, fast):
    route = "fused" if fast else "composable"
    gemm = prec == hb.BF16_ACT and not fast                 # the stride-1 conv that remains is the GEMM form
    assert plan((2, 16, 32, 12, 12), 1, 2, 0, prec, fast) == (0, False, True, route, launch(1, 0, gemm=gemm))
    # C = 6 is no multiple of 4: the strided conv itself
    assert plan((2, 6, 32, 12, 12), 1, 2, 0, prec, fast) == (0, False, False, route, launch(2, 0))
    assert not plan((2, 16, 32, 12, 12), 3, 2, 1, prec, fast).subsample      # 3x3 / stride 2
    assert not plan((2, 16, 32, 12, 12), 1, 2, 1, prec, fast).subsample      # padded


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("prec", PRECS)
def test_rgb_input_is_padded_to_one_16_byte_slot(prec, fast):
    extra = 5 if prec == hb.BF16_ACT else 1                 # 8 bf16 or 4 fp32 channels
    assert plan((2, 3, 16, 8, 8), 3, 1, 1, prec, fast) == (extra, False, False, "fused" if fast else "composable", launch(1, 1))
    # the padded input has a multiple of 4 channels: an RGB 1x1 / stride-2 conv gathers
    assert plan((2, 3, 16, 8, 8), 1, 2, 0, prec, fast).subsample


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("prec", PRECS)
def test_three_outputs_run_as_four_on_the_triad_whatever_fast_is(prec, fast):
    gemm = prec == hb.BF16_ACT                              # the triad is composable: GEMM in the fast mode too
    assert plan((2, 16, 3, 8, 8), 1, 1, 0, prec, fast) == (0, True, False, "triad", launch(1, 0, gemm=gemm))
    assert plan((2, 16, 3, 8, 8), 3, 1, 1, prec, fast) == (0, True, False, "triad", launch(1, 1))


@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", list(BLUR_CASES))
def test_blur_down_form_and_the_fused_block_share_the_space_to_depth_rule(case, prec, fast):
    B, C, N, H, W = case
    shared, own = BLUR_CASES[case]
    s2d = shared and own and prec != hb.F32
    p = plan(case, 3, 2, 1, prec, fast, blurred=True)
    route = "fused" if fast else "composable"
    assert p == (0, False, False, route, launch(1, 1, s2d=C) if s2d else launch(2, 1))
    assert plan(case, 3, 2, 1, prec, fast).launch == launch(2, 1)             # ops.conv2d never takes the form
    # the fused DiscriminatorBlock whose stride-2 tail reads C channels at H x W answers by the shared rule alone
    shapes = [(C, C, 1, 1), (C, C, 3, 3), (C, C, 3, 3), (N, C, 3, 3)]
    block = ops._dblock_plan((B, C, H, W), ADT[prec], True, shapes, True, prec, lambda *a: True, lambda *a: True)
    assert block.s2d == (shared and prec != hb.F32) == ops._s2d_eligible(C, H, W, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_blur_down_form_wants_a_3x3_kernel(prec):
    assert plan((1, 64, 64, 32, 32), 1, 2, 1, prec, True, blurred=True).launch.s2d == 0
    assert plan((1, 64, 64, 32, 32), 5, 2, 1, prec, True, blurred=True).launch.s2d == 0


@pytest.mark.parametrize("prec", PRECS)
def test_rgb_slot_is_one_rule_for_the_plain_conv_and_the_fused_block(prec):
    want = 5 if prec == hb.BF16_ACT else 1
    assert ops._rgb_extra(ADT[prec]) == want
    assert plan((2, 3, 64, 64, 64), 3, 1, 1, prec, True).extra_in == want
    shapes = [(64, 3, 1, 1), (64, 3, 3, 3), (64, 64, 3, 3), (64, 64, 3, 3)]
    for cuda in (True, False):                              # the one-pass kernel and the concatenation pad alike
        block = ops._dblock_plan((2, 3, 64, 64), torch.float32, cuda, shapes, True, prec, lambda *a: True, lambda *a: True)
        assert block.extra == want


def test_only_the_plan_reads_the_gemm_switches():
    """STYLEX_RES_GEMM_DD belongs to this path alone; STYLEX_RES_GEMM is also read by _dblock_plan, for the fused block."""
    src = inspect.getsource(ops)
    plan_src = inspect.getsource(ops._conv_plan)
    dd = "STYLEX_RES_GEMM_DD"
    assert plan_src.count(dd) >= 1 and src.count(dd) == plan_src.count(dd)
    both = plan_src.count("STYLEX_RES_GEMM") + inspect.getsource(ops._dblock_plan).count("STYLEX_RES_GEMM")
    assert src.count("STYLEX_RES_GEMM") == both
    for fn in (ops._gemm_1x1, ops._fwd, ops._bwd_data, ops._bwd_weight, ops._conv_forward, ops._conv_backward, ops._conv_apply,
               ops._Conv, ops._Dgrad, ops._Wgrad, ops._ConvBiasActFast, ops._ConvBiasActDD):
        assert not re.search(r"environ|getenv", inspect.getsource(fn)), fn


def test_space_to_depth_weight_shape_is_spelled_in_the_backend_only():
    assert not re.search(r"4 \* \w+, 3, 3\)", inspect.getsource(ops))
    assert "pack_weight_s2d" not in inspect.getsource(ops._fwd) + inspect.getsource(ops._bwd_data)
    assert not hasattr(ops, "_DownS2DFast")
