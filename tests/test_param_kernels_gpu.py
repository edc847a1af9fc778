"""-m gpu: the kernels that touch parameters, csrc/adam_pack.hip (the Adam step and every operand copy it refreshes),
csrc/style_coeffs.hip (wsq, modcoeff forward, both backward kernels) and csrc/initial_block.hip (forward, data gradient, weight
gradient), against their float64 definitions (tests/_param_defs.py), element by element.  Run this file before any change to
one of the three.

Method and helpers are those of tests/test_ew_torgb_gpu.py and tests/test_linattn_gpu.py (read their docstrings first): the hb
wrappers are called directly on seeded inputs; the references are taken in float64 from the values the kernel receives; every
call runs twice and must give the same bits.  Inputs, chain counts, limits and the comparison itself are those of
tests/test_param_defs_cpu.py, which holds an fp32 model of each kernel's pass structure to them on the CPU and shows that
mutations of the model break them; nothing here is tuned against the kernels.  The backward kernels of style_coeffs.hip are
functions of their saved operands: they are handed the definition's d and s1 rounded to fp32, and the reference is taken
from those.

EXACT class: the result must EQUAL float32(definition), or bfloat16(float32(definition)).
  operand copies   every bf16 copy the Adam launch refreshes equals bfloat16(float32(scale) * w) of the parameter the step left
                   behind, in the layout defined on the host: no tolerance.
  style coeffs     integer weights in [-4, 4], styles multiples of 1/2, handed-in d in {1/2, 1}, integer gd and gs1: wsq, s1,
                   gstyle, gw are exact (the sums, in units of their granule, are asserted below 2^24).  The forward d goes through
                   rsqrtf and stays in the GAUSS class.
  initial block    integer styles equal across the L layers (the mean is exact for any L), integer weights in [-4, 4] (exact in
                   bf16), integer gx: x and dW are exact; dstyles is exact for L a power of two, otherwise within the two
                   roundings of s * (1.f / L): 2 * 2^-24 |want|.

GAUSS class: per element  |got - want| <= EW |want| + 2^-24 (N abs_terms + arg_terms),  EW = 2^-22 (fp32) / 2^-8 (bf16); where
the limit is 0 the result must be 0.  arg_terms: see _param_defs.  N = fp32 roundings on the longest path of a term, read from
the code and counted without contraction (an fmaf counts as its product and its addition); division and square root round once
(no fast-math in the build); rsqrtf counts as its documented bound of 2 ulp = 4 * 2^-24 of the value; the pow and sqrt of the bias
corrections run in double and count as the one conversion to float.
  Adam exp_avg        N = 3    1.f - beta1, the product with g, the fma's addition (the m term: float(beta1) and the addition);
                               arg_terms beta1 |g|: float(beta1) seen through 1 - beta1
       exp_avg_sq     N = 4    1.f - beta2, two products with g, the addition; arg_terms beta2 g^2
       p              N = 13   exp_avg 3; step_size = float(lr / bc1) 1; step_size * m 1; the denominator 6 = half of the 4 of
                               exp_avg_sq under the square root, sqrt, float(sqrt(bc2)), the division, + eps; the division; the
                               subtraction.  abs_terms |p| + step_size / denom * abs_terms(exp_avg); arg_terms those of exp_avg
                               scaled alike, and half the relative arg_terms of exp_avg_sq on the update
  wsq (tap sum)       N = T + 1         the square and T additions, in the Adam launch and in wsq_kernel
  s1                  N = 0             one addition: EW |want| alone
  d                   EW d + 2^-24 (4 d + N_acc d / 2),  N_acc = 3 + ceil(C / 16) + 4 + 1: style + 1, s * s, the product with wsq,
                               the lane's additions, four shuffle additions, + eps; every term of the argument is positive, so
                               one rounding on its chain moves d by at most d / 2
  gstyle              N = 8 + ceil(O / 4)   dq = -0.5 gd d d d 3, the product with wsq, ceil(O / 4) additions, 2 of the LDS tree,
                               the product with 2 s1, + gs1
  gw                  N = 6 + B        dq 3, s1 * s1, their product, B additions, the product with 2 w
  initial block x     N = L + D + 2    the L additions and the division of the mean, the product, D additions; in bf16 the weight
                               operand is rounded first and the store is one round-to-nearest-even (EW = 2^-8)
       dstyles        N = 16 ceil(C / 64) + 9   the product, the lane's additions, six shuffle additions, 1.f / L, the product
       dW             N = L + B + 2    the mean, the product, B additions; in bf16 gx is rounded first

Branches and the cases that enter them (ADAM_TENSORS, STYLE_SHAPES, IB_SHAPES of test_param_defs_cpu.py).
adam_pack_kernel, all in both placements (p and grad 16-byte aligned / at a 4-byte offset into a larger buffer, which turns
every float4 branch into its scalar twin; the two placements must give identical bits):
  flat float4 block                flat4608 (exactly one), flat9221 (two)        flat scalar tail      flat9221 (5), flat1, linear
  slab float4 rows                 w16x64x9, w5x7x4, w24x40x1, initw*, five      slab scalar rows      w16x130x9 (C T % 4 != 0),
                                                                                                        w12x33x9, w8x75x9, w4x6x9
  N % 8 != 0 / N < 8               w12x33x9 (8 + 4), initw18x24 (8 + 8 + 2) / w4x6x9, w5x7x4, initw3x512
  odd C / ragged last slab         w12x33x9, w5x7x4 / w16x130x9 (2, even), w8x75x9 (11, odd);  T in {1, 4, 9}: w24x40x1, initw*; w5x7x4; the rest
  pack   even_c / !even_c          w16x64x9, w16x130x9, w4x6x9, w24x40x1 / w12x33x9, w8x75x9, w5x7x4
         full_n / !full_n          w16x64x9, w16x130x9, w8x75x9, w24x40x1 / w12x33x9, w4x6x9, w5x7x4
  s2d    even_c+full_n, even_c+!full_n, !even_c+full_n, !even_c+!full_n     w16x64x9 and w16x130x9, w4x6x9, w8x75x9, w12x33x9
  scaled pack / scaled s2d / bf16 matrix (plain, scaled) / wsq / initw      w16x64x9 / w16x64x9, w4x6x9 / w24x40x1 / w16x130x9,
                                                                             w12x33x9, w5x7x4 / initw18x24 (6 slabs), initw3x512 (128)
  more than four copies: "five" (four refreshed, the fifth re-packed lazily);  no gradient: "frozen" (untouched, its pack served)
  steps 2, 3, 10001; lr changed before every call; two groups with different lr, betas and eps.
style_coeffs.hip (B, C, O, K): C < 16 (1x1x1x1, 3x3x5x9, 2x15x3x9), O < 4 (1x1x1x1, 2x15x3x9), O % 16 != 0 and O % 4 != 0 (3x65x17x9,
  7x130x77x1), C % 64 != 0 with more than one block (7x130x77x1, 3x65x17x9), K = 1, the real width 2x512x512x9; gs1 present / absent.
initial_block.hip (B, L, D, C): n >= N guards 3x7x18x24 (N = 384) and 1x1x1x1, 3x2x514x80, 130x2x18x40; the weight gradient's
  second / third sample tile 65x4x33x16 / 130x2x18x40; forward's ragged last tile of samples the same two, 3x*, 9x*; dgrad's
  grid.y of 3 (65x*), 5 (130x*); L = 1, L = 64; D = 1, D = 1024; the ragged second channel chunk 3x2x514x80; 9x7x514x512.
Not reachable through the wrappers: none of the branches listed in the kernels is; the descriptor's fallback N = C = T = 0 for a
weight with kh * kw > 9 that has copies other than initw is host logic and has no kernel branch of its own.

With STYLEX_PARAM_RECORD=<file> every case leaves one line in that file: its worst error / limit
(profiles/param_kernels_errors.txt is the record of one run)."""
import functools
import os
import warnings

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.against_definition]

import _param_defs as P  # noqa: E402
import hip_backend as hb  # noqa: E402
import ops  # noqa: E402
import test_param_defs_cpu as T  # noqa: E402
from test_ew_torgb_gpu import DEV, DT, Recorder, hip_impl, sid, twice  # noqa: E402,F401
from test_linattn_defs_cpu import limit, worst  # noqa: E402

NAN = float("nan")
BAND = 8192
_LINES = []


@pytest.fixture
def rec(request):
    r = Recorder()
    yield r
    name = request.node.nodeid.split("::", 1)[-1]
    tail = "".join("  [%s]" % e for e in r.each) + ("  [%d exact comparisons]" % r.exact if r.exact else "")
    _LINES.append("%-64s %8.4f  %s%s" % (name, r.worst, r.what or "-", tail))


HEADER = """# tests/test_param_kernels_gpu.py: per test case, the worst observed error / limit (<= 1 passes) of its Gauss-class quantities and
# the quantity that gave it, then [every quantity]; exact-class quantities (the bf16 operand copies, the integer classes) assert
# equality with the rounded float64 definition and are counted.  Limit per element: EW * |want| + 2^-24 * (N * abs_terms + arg_terms),
# EW = 2^-22 (fp32) / 2^-8 (bf16), N per kernel as in the file's docstring.  Adam quantities are named <quantity>@<step count>.
# Ratios above 0.5 are the bf16 x of the initial block: the one round-to-nearest-even store (up to 2^-8 / (1 + 2^-8) = 0.9961 of
# EW * |want| legitimately), and the dstyles of its exact class at L = 3, 7: held to the two roundings of s * (1.f / L) alone.
# In the other fp32 rows a ratio far below 1 is expected; one above 1 is a finding.
"""


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    out = os.environ.get("STYLEX_PARAM_RECORD")
    if out and _LINES:
        with open(out, "w") as f:
            f.write(HEADER + "\n".join(_LINES) + "\n")


def record(rec, res):
    for name, v in res.items():
        if isinstance(v, bool):
            assert v, "%s (exact class) differs from the rounded definition" % name
            rec.equal()
        else:
            rec.ratio(v, name)


# ---- guard bands ---------------------------------------------------------------------------------------------------------------
def guarded(t, off=0):
    """(allocation, view): a device copy of `t` (same strides) between two NaN bands of its own allocation, `off` elements
    further in (off = 1: a 4-byte-aligned fp32 pointer that is not 16-byte aligned)."""
    flat = torch.full((t.numel() + 2 * BAND + off,), NAN, dtype=t.dtype, device=DEV)
    view = flat.as_strided(t.shape, t.stride(), BAND + off)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * off) % 16 or t.dtype != torch.float32
    return flat, view


def intact(flat, numel, off=0):
    return bool(torch.isnan(flat[:BAND + off].float()).all()) and bool(torch.isnan(flat[BAND + off + numel:].float()).all())


def own_bands_intact(t):
    """A tensor hb allocated under _POISON / _GUARD: its storage is the tensor between two NaN bands."""
    store = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())
    return store.numel() == t.numel() + 2 * BAND and t.storage_offset() == BAND and intact(store, t.numel())


@pytest.fixture
def guards(monkeypatch):
    monkeypatch.setattr(hb, "_POISON", True)
    monkeypatch.setattr(hb, "_GUARD", BAND)


# ================================================================ Adam and the copies =========================================
FROZEN = (8, 8, 3, 3)


def _register(p, kind, scale):
    """The cache entry a training step would have created; returns (getter of the served value, allocations to watch)."""
    if kind == "pack":
        get = lambda: hb.pack_weight(p, True, True, hb.BF16_ACT)
    elif kind == "pack_b":
        get = lambda: hb.pack_weight(p, False, True, hb.BF16_ACT, scale=scale)
    elif kind == "s2d":
        get = lambda: hb.pack_weight_s2d(p, scale=scale)
    elif kind == "wsq":
        get = lambda: (hb.weight_sumsq(p), None)
    else:  # bf16mat, initw: torch builds them; registered as _bf16_matrix / _initial_block_operand do, between guard bands
        flat, view = guarded(torch.zeros(p.shape[0], p.numel() // p.shape[0], dtype=torch.bfloat16))
        if kind == "bf16mat":
            hb.packs.put((p,), "bf16mat", (view,), None, scale=scale, derived=False, extra=None)
            get = lambda: (hb._bf16_matrix(p, scale), None)
        else:
            hb.packs.put((p,), "initw", (view,), None)
            get = lambda: (hb._initial_block_operand(p, hb.BF16_ACT)[0], None)
        assert get()[0].data_ptr() == view.data_ptr()
        return get, [(flat, view.numel())]
    return get, None


@functools.lru_cache(maxsize=None)
def adam_run(place):
    """All tensors of T.ADAM_TENSORS through the three calls of T.ADAM_CALLS in one optimiser, p and grad at offset `place` (0 or
    1 element) behind their guard band.  Every call writes p, grad, exp_avg, exp_avg_sq and step in place (the plan's pointers
    stay valid), runs hb.adam_pack_step twice from that state and keeps the results on the CPU."""
    off = {"aligned": 0, "offset": 1}[place]
    prev = hb._POISON, hb._GUARD
    hb._POISON, hb._GUARD = True, BAND
    hb.pack_cache_clear()
    hb.adam_forget()
    out, watch = {}, []  # watch: (what, allocation, numel, off)
    try:
        params, groups = {}, ([], [])
        for name, spec in T.ADAM_TENSORS.items():
            p0, g0, _, _ = T.adam_inputs(name, 0)
            pf, pv = guarded(p0, off)
            gf, gv = guarded(g0, off)
            p = torch.nn.Parameter(pv)
            p.grad = gv
            assert p.data_ptr() == pv.data_ptr() and p.grad.data_ptr() == gv.data_ptr() and p.is_contiguous()
            watch += [(name + ".p", pf, p0.numel(), off), (name + ".grad", gf, p0.numel(), off)]
            params[name] = p
            groups[spec.group].append(p)
        frozen = torch.nn.Parameter(torch.randn(FROZEN, generator=T.gen("frozen")).to(DEV))  # never gets a gradient
        groups[0].append(frozen)
        opt = torch.optim.Adam([dict(params=groups[i], **T.ADAM_GROUPS[i]) for i in (0, 1)], fused=True)
        assert hb.adam_pack_step(opt) is False, "the first step initialises torch's state: must fall back"
        opt.step()
        for name, p in params.items():  # the moments between guard bands too: installed before the first plan is made
            st = opt.state[p]
            for key in ("exp_avg", "exp_avg_sq"):
                flat, view = guarded(st[key].cpu())
                st[key] = view
                watch.append((name + "." + key, flat, view.numel(), 0))
        getters = {}
        for name, spec in T.ADAM_TENSORS.items():
            getters[name] = []
            for kind, scale in spec.copies:
                get, own = _register(params[name], kind, scale)
                served = get()
                getters[name].append((kind, scale, get, served))
                for j, t in enumerate(served):
                    if t is not None and own is None:
                        assert own_bands_intact(t), (name, kind, "not between guard bands")
                for flat, n in own or ():
                    watch.append(("%s.%s" % (name, kind), flat, n, 0))
        frozen_get = lambda: hb.pack_weight(frozen, True, True, hb.BF16_ACT)
        frozen_before = (frozen.detach().clone(), [t.clone() for t in frozen_get()], [t.data_ptr() for t in frozen_get()])

        for call, (step, f) in enumerate(T.ADAM_CALLS):
            for i, grp in enumerate(opt.param_groups):
                grp["lr"] = T.ADAM_GROUPS[i]["lr"] * f
            runs = []
            for _ in range(2):
                with torch.no_grad():
                    for name, p in params.items():
                        p0, g0, m0, v0 = T.adam_inputs(name, call)
                        st = opt.state[p]
                        p.copy_(p0), p.grad.copy_(g0), st["exp_avg"].copy_(m0), st["exp_avg_sq"].copy_(v0), st["step"].fill_(step - 1)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # "five": one copy more than the descriptor has slots
                    assert hb.adam_pack_step(opt) is True
                torch.cuda.synchronize()
                res = {}
                for name, p in params.items():
                    st = opt.state[p]
                    assert float(st["step"]) == step
                    copies = []
                    for kind, scale, get, served in getters[name]:
                        now = get()
                        same = all((a is None) == (b is None) and (a is None or a.data_ptr() == b.data_ptr()) for a, b in zip(now, served))
                        copies.append((kind, scale, same, [None if t is None else t.detach().cpu().clone() for t in now],
                                       all(t is None or own_bands_intact(t) for t in now) if kind in ("pack", "pack_b", "s2d", "wsq") else True))
                    res[name] = dict(p=p.detach().cpu().clone(), m=st["exp_avg"].cpu().clone(), v=st["exp_avg_sq"].cpu().clone(), copies=copies)
                runs.append(res)
            for name in params:
                a, b = runs
                assert all(torch.equal(a[name][k], b[name][k]) for k in "pmv"), (name, call, "second call differs")
                for ca, cb in zip(a[name]["copies"], b[name]["copies"]):
                    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(ca[3], cb[3])), (name, call, ca[0], "second call differs")
            out[call] = runs[0]
        now = frozen_get()
        out["frozen"] = (torch.equal(frozen.detach(), frozen_before[0]) and all(torch.equal(a, b) for a, b in zip(now, frozen_before[1]))
                         and [t.data_ptr() for t in now] == frozen_before[2])
        out["bands"] = [what for what, flat, n, o in watch if not intact(flat, n, o)]
    finally:
        hb._POISON, hb._GUARD = prev
        hb.pack_cache_clear()
        hb.adam_forget()
    return out


@pytest.mark.parametrize("name", list(T.ADAM_TENSORS))
@pytest.mark.parametrize("place", ("aligned", "offset"))
def test_adam_step_and_copies(place, name, rec):
    """p, exp_avg, exp_avg_sq within their per-element limits of the float64 step at steps 2, 3, 10001 (lr changed before each);
    every registered copy served from the cache afterwards and equal to the host definition taken from the resulting p."""
    run = adam_run(place)
    for call, (step, _) in enumerate(T.ADAM_CALLS):
        got = run[call][name]
        want = P.adam(*T.adam_inputs(name, call), **T.adam_hyper(name, call))
        for k, r in T.adam_ratios(want, got["p"], got["m"], got["v"]).items():
            rec.ratio(r, "%s@%d" % (k, step))
        fresh = 0
        for kind, scale, same, value, banded in got["copies"]:
            assert banded, (kind, "a guard band of the copy was written")
            fresh += not same
            if kind == "wsq":
                q = P.wsq(got["p"])
                rec.ratio(worst(value[0], q.value, limit(q, T.wsq_n(got["p"][0, 0].numel()), "fp32")), "wsq@%d" % step)
                continue
            for have, expect, side in zip(value, T.copy_definitions(kind, got["p"], scale), "ab"):
                assert (have is None) == (expect is None), (kind, side)
                if have is not None:
                    assert have.dtype == torch.bfloat16 and have.numel() == expect.numel()
                    assert torch.equal(have.view(-1), expect.view(-1)), "%s %s (scale %r) at step %d differs from its definition: %d elements" % (
                        kind, side, scale, step, int((have.view(-1) != expect.view(-1)).sum()))
                    rec.equal()
        # four slots: a parameter with five copies has four rewritten in place and one re-packed on its next use
        assert fresh == (1 if name == "five" else 0), (name, fresh, "copies not served from the refreshed cache entries")


@pytest.mark.parametrize("place", ("aligned", "offset"))
def test_adam_guard_bands_and_the_parameter_without_a_gradient(place):
    run = adam_run(place)
    assert run["bands"] == [], "guard bands written: %s" % run["bands"]
    assert run["frozen"], "a parameter without a gradient changed, or its pack was rebuilt"


def test_adam_placements_give_identical_bits():
    """The invariant adam_update's comment promises: p and grad as 4-byte-aligned views of a larger buffer (the scalar branches)
    and as 16-byte-aligned tensors (the float4 branches) give the same p, exp_avg, exp_avg_sq, and so the same copies."""
    a, b = adam_run("aligned"), adam_run("offset")
    for call in range(len(T.ADAM_CALLS)):
        for name in T.ADAM_TENSORS:
            for k in "pmv":
                assert torch.equal(a[call][name][k], b[call][name][k]), (name, call, k)
            for ca, cb in zip(a[call][name]["copies"], b[call][name]["copies"]):
                assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(ca[3], cb[3])), (name, call, ca[0])


# ================================================================ style coefficients ==========================================
def banded(*outs):
    """Results allocated under the `guards` fixture: their own NaN bands are intact."""
    torch.cuda.synchronize()
    assert all(own_bands_intact(t) for t in outs), "a guard band of a result was written"
    return outs[0] if len(outs) == 1 else outs


def style_kernels():
    dev = lambda t: None if t is None else t.to(DEV).contiguous()

    def wsq_fn(w):
        wd = dev(w)
        return banded(twice(lambda: hb.weight_sumsq(wd)))

    def fwd_fn(style, wsq32, eps):
        sd, qd = dev(style), dev(wsq32)
        return banded(*twice(lambda: hb.modcoeff_fwd(sd, qd, eps)))

    def bwd_fn(gd, d, s1, wsq32, w, gs1):
        a = [dev(t) for t in (gd, d, s1, wsq32, w, gs1)]
        gs, gw = twice(lambda: hb.modcoeff_bwd(*a, True, True))
        only_s, none_w = hb.modcoeff_bwd(*a, True, False)
        none_s, only_w = hb.modcoeff_bwd(*a, False, True)
        assert none_w is None and none_s is None and torch.equal(only_s, gs) and torch.equal(only_w, gw), "a gradient depends on the other's launch"
        return banded(gs, gw)

    return wsq_fn, fwd_fn, bwd_fn


@pytest.mark.parametrize("eps", T.STYLE_EPS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("shape", T.STYLE_SHAPES, ids=[sid(s) for s in T.STYLE_SHAPES])
def test_style_coefficients(shape, cls, eps, rec, guards):
    record(rec, T.style_ratios(shape, cls, eps, *style_kernels()))


def test_mod_coeffs_entry_point_runs_the_fused_node(rec):
    """ops.mod_coeffs on the fast path: the fused node serves it; its d comes from the kernel's own wsq (the argument carries the
    wsq chain as well), and its backward is held to the definition at the saved s1 and d it returned."""
    shape, eps = (5, 24, 40, 9), 1e-8
    inp, cnt = T.style_inputs(shape, "gauss", eps), T.style_counts(*shape)
    sd, wd = inp.style.to(DEV).requires_grad_(), torch.nn.Parameter(inp.w.to(DEV))
    prev = ops.set_fast(True)
    try:
        s1, d = ops.mod_coeffs(sd, wd, True, eps)
        assert type(s1.grad_fn).__name__.startswith("_ModCoeffs"), "the fused kernels must serve the fast path"
        ((s1 * inp.gs1.to(DEV)).sum() + (d * inp.gd.to(DEV)).sum()).backward()
        wsq = hb.weight_sumsq(wd).cpu()
    finally:
        ops.set_fast(prev)
        hb.pack_cache_clear()
    q, dw = P.wsq(inp.w), P.demod(inp.style, P.wsq(inp.w).value, eps)
    rec.ratio(worst(wsq, q.value, limit(q, cnt["wsq"], "fp32")), "wsq")
    rec.ratio(worst(d.detach().cpu(), dw.value, T.d_limit(dw, cnt["acc"] + cnt["wsq"])), "d")
    want = P.modcoeff_bwd(inp.gd, d.detach().cpu(), s1.detach().cpu(), wsq, inp.w, inp.gs1)
    rec.ratio(worst(sd.grad.cpu(), want.gstyle.value, limit(want.gstyle, cnt["gs"], "fp32")), "gstyle")
    rec.ratio(worst(wd.grad.cpu(), want.gw.value, limit(want.gw, cnt["gw"], "fp32")), "gw")


# ================================================================ initial block ===============================================
def ib_kernels(prec):
    """The three wrappers on operands between guard bands (the bf16 weight operand registered as hb._initial_block_operand does);
    the results, allocated under hb._GUARD, must leave their own bands intact."""
    mode = hb.F32 if prec == "fp32" else hb.BF16_ACT
    kept = []

    def put(t):
        flat, view = guarded(t)
        kept.append((flat, t.numel()))
        return view

    def weight(w):
        if prec == "fp32":
            return put(w)
        wp = torch.nn.Parameter(put(w))
        op = put(P.matrix(w))
        assert torch.equal(op.float().cpu(), w.reshape(w.shape[0], -1)), "the bf16 class hands in bf16 values"
        hb.packs.put((wp,), "initw", (op,), None)
        assert hb._initial_block_operand(wp, mode)[0].data_ptr() == op.data_ptr()
        return wp

    def act(gx):
        return put(gx.to(DT[prec]).contiguous(memory_format=torch.channels_last))

    def done(*outs):
        torch.cuda.synchronize()
        for t in outs:
            assert own_bands_intact(t), "a guard band of a result was written"
        assert all(intact(flat, n) for flat, n in kept), "a guard band of an operand was written"
        return outs[0]

    def fwd(styles, w):
        sd, wd = put(styles), weight(w)
        x = twice(lambda: hb.initial_block_fwd(sd, wd, mode, DT[prec]))
        assert hb.is_cl(x)
        return done(x)

    def dgrad(gx, w, L):
        gd, wd = act(gx), weight(w)
        return done(twice(lambda: hb.initial_block_bwd_data(gd, wd, L, mode)))

    def wgrad(styles, gx):
        sd, gd = put(styles), act(gx)
        return done(twice(lambda: hb.initial_block_bwd_weight(sd, gd)))

    return fwd, dgrad, wgrad


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("case", T.IB_SHAPES, ids=[sid(s) for s in T.IB_SHAPES])
def test_initial_block(case, cls, prec, rec, guards):
    assert hb.initial_block_supported(*case)
    try:
        record(rec, T.ib_ratios(case, cls, prec, *ib_kernels(prec)))
    finally:
        hb.pack_cache_clear()


def test_initial_block_limits_are_rejected_just_outside():
    for case in T.IB_OUTSIDE:
        assert not hb.initial_block_supported(*case), case
    assert hb.initial_block_supported(2, 64, 1024, 512)
