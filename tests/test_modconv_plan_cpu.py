"""ops._modconv_plan: the one place that decides how a fused modulated conv (Conv2DMod + noise + LeakyReLU) runs, against
the rules written out here case by case (not imported from the code under test).  No GPU and no kernel library: the
library probe is a stub."""
import inspect
import re

import pytest

import hip_backend as hb
import ops

SWITCHES = ("STYLEX_FOLD_D", "STYLEX_NOISE_NAT")
# MODCONV_CASES of test_bwd_glue_gpu.py (B, Cin, Cout, H, W, side of the noise plane) -> what the rules give:
#   pre:     bf16 activations, H*W <= 64, 64 | Cin
#   natural: the forward reads the natural-order plane: 4 | side
#   reduce:  hb.scale_reduce for the input gradient: 4 | Cin, Cin <= 1024
CASES = {(3, 12, 12, 9, 9, 12): dict(pre=False, natural=True, reduce=True),
         (2, 40, 40, 10, 13, 16): dict(pre=False, natural=True, reduce=True),    # 130 px; 40 is no multiple of 64
         (2, 64, 40, 8, 8, 8): dict(pre=True, natural=True, reduce=True),
         (2, 6, 12, 9, 9, 9): dict(pre=False, natural=False, reduce=False),     # side 9, Cin = 6
         (16, 512, 512, 4, 4, 4): dict(pre=True, natural=True, reduce=True)}
SMALL = (2, 64, 40, 8, 8, 8)
ODD = (2, 6, 12, 9, 9, 9)


def yes(name):
    return True


def no(name):
    return False


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def plan(case, prec, probe=yes, cuda=True, d=True, style=True, noise=True, nat=True, lrelu=True, pad=1):
    B, ci, co, H, W, side = case
    return ops._modconv_plan((B, ci, H, W), (co, ci, 3, 3), cuda, d, style, noise, nat, side, pad, lrelu, prec, probe)


@pytest.mark.parametrize("prec", [hb.BF16_ACT, hb.BF16, hb.F32])
@pytest.mark.parametrize("case", list(CASES))
def test_plan_against_the_rules_case_by_case(case, prec):
    want = CASES[case]
    p = plan(case, prec)
    pre = want["pre"] and prec == hb.BF16_ACT
    fold = prec != hb.F32               # every case has d, 4 | Cout <= 1024 and the switch at its default
    assert (p.prec, p.pad, p.lrelu) == (prec, 1, True)
    assert p.pre is pre
    assert p.nat is True
    assert p.fwd_noise == ("natural" if want["natural"] else "transposed")
    assert p.bwd_noise == "natural"     # at any side
    assert p.prep is True and p.prep_ok is True
    assert p.fold is fold
    assert p.dgrad == ("folded" if fold else "in_scale")  # fp32 has no `pre`, so never "prescaled"
    assert p.scale_reduce is want["reduce"]
    assert len(p) == 12                 # every field is asserted above


def test_small_layer_takes_pre_and_each_data_gradient_form(monkeypatch):
    p = plan(SMALL, hb.BF16_ACT)
    assert p.pre and p.fold and p.dgrad == "folded"
    assert plan(SMALL, hb.F32).dgrad == "in_scale" and not plan(SMALL, hb.F32).pre
    monkeypatch.setenv("STYLEX_FOLD_D", "0")
    p = plan(SMALL, hb.BF16_ACT)
    assert p.pre and not p.fold and p.dgrad == "prescaled"
    assert plan(SMALL, hb.BF16_ACT, d=False).dgrad == "in_scale"      # nothing to pre-scale by
    p = plan(SMALL, hb.BF16)                                          # bf16 operands, fp32 activations: no `pre`
    assert not p.pre and p.dgrad == "in_scale"
    assert not plan(SMALL, hb.BF16_ACT, style=False).pre


def test_forward_and_backward_noise_reads_may_differ():
    p = plan(ODD, hb.BF16_ACT)
    assert (p.fwd_noise, p.bwd_noise) == ("transposed", "natural")
    assert p.scale_reduce is False                                    # the two ATen expressions
    assert not plan((2, 40, 40, 10, 13, 16), hb.BF16_ACT).pre
    assert not plan((2, 1028, 12, 4, 4, 4), hb.F32).scale_reduce      # 4 | Cin but above 1024


@pytest.mark.parametrize("switch,field,off", [("STYLEX_FOLD_D", "fold", False), ("STYLEX_NOISE_NAT", "nat", False),
                                              ("STYLEX_NOISE_NAT", "fwd_noise", "transposed"),
                                              ("STYLEX_NOISE_NAT", "bwd_noise", "transposed")])
def test_switch_set_to_0_turns_its_field_off(switch, field, off, monkeypatch):
    on = getattr(plan(SMALL, hb.BF16_ACT), field)
    assert on in (True, "natural")
    monkeypatch.setenv(switch, "0")
    assert getattr(plan(SMALL, hb.BF16_ACT), field) == off
    monkeypatch.setenv(switch, "1")
    assert getattr(plan(SMALL, hb.BF16_ACT), field) == on


def test_natural_plane_needs_a_device_input_and_a_plane():
    for kw in (dict(cuda=False), dict(nat=False)):
        p = plan(SMALL, hb.BF16_ACT, **kw)
        assert (p.nat, p.fwd_noise, p.bwd_noise) == (False, "transposed", "transposed")


def test_probe_refusing_moves_only_the_backward_read():
    asked = []
    p = plan(SMALL, hb.BF16_ACT, probe=lambda name: asked.append(name) and False)
    assert asked == ["stylex_modconv_bwd_prep_nat"]
    assert (p.nat, p.fwd_noise, p.bwd_noise) == (True, "natural", "transposed")
    assert p == plan(SMALL, hb.BF16_ACT)._replace(bwd_noise="transposed")


def test_probe_is_not_asked_without_a_natural_plane():
    """A host tensor never reaches the library."""
    asked = []
    plan(SMALL, hb.F32, probe=lambda name: asked.append(name) or True, cuda=False)
    assert not asked


@pytest.mark.parametrize("prec", [hb.BF16_ACT, hb.F32])
def test_plain_modulated_conv_has_no_prep_pass(prec):
    """No noise, no LeakyReLU, no demodulation (the padded to-RGB route): y is not saved, the gradient goes in unscaled."""
    p = plan((2, 16, 4, 8, 8, 0), prec, d=False, noise=False, nat=False, lrelu=False, pad=0)
    assert (p.prep, p.fold, p.dgrad, p.fwd_noise, p.bwd_noise) == (False, False, "in_scale", "none", "transposed")
    assert p.pad == 0 and p.lrelu is False
    for kw in (dict(lrelu=True), dict(d=True), dict(noise=True)):     # each of the three alone asks for the pass
        assert plan((2, 16, 4, 8, 8, 8), prec, **{**dict(d=False, noise=False, nat=False, lrelu=False), **kw}).prep


def test_six_output_channels_are_recorded_not_raised():
    """The backward raises for them; a forward under no_grad must keep working, so the plan only records it."""
    p = plan((2, 12, 6, 9, 9, 12), hb.BF16_ACT)
    assert p.prep and not p.prep_ok and not p.fold and p.dgrad == "in_scale"
    assert not plan((2, 12, 1028, 4, 4, 4), hb.BF16_ACT).prep_ok      # 4 | Cout but above 1024


def test_probe_defaults_to_the_backend():
    assert ops._modconv_plan.__defaults__ == (hb.has_symbol,)


def test_only_the_plan_reads_the_switches_and_the_library():
    src = inspect.getsource(ops)
    plan_src = inspect.getsource(ops._modconv_plan)
    for name in SWITCHES:
        assert plan_src.count(name) >= 1 and src.count(name) == plan_src.count(name), name
    for fn in (ops._modconv_forward, ops._modconv_backward, ops._ModConvFast):
        assert not re.search(r"environ|has_symbol", inspect.getsource(fn)), fn
