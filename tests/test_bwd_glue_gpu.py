"""-m gpu: the backward glue kernels against their float64 definitions (tests/_bwd_glue_defs.py) — the contract of
csrc/fused_bwd.hip (act_bwd_reduce, modconv_bwd_prep[_scaled], scale_reduce) and of the resampling copies of
csrc/elementwise.hip (subsample2_fwd/bwd, add_at_even).  Run this file before any change to fused_bwd.hip.

Kernel level: the hb wrappers on given inputs (seeded, rounded to the activation dtype first; the reference is computed from the
rounded values), at the edges of make_geo's lane / chunk geometry.  Tolerances are derived, not tuned:
  * elementwise outputs, fp32: a product of at most three factors, two of them rounded constants (the fp32 scale argument,
    0.2f): <= 3.25 * 2^-24 relative, asserted as 2^-22 * |want|;
  * elementwise outputs, bf16: ONE round-to-nearest-even store (act_pack2) of such a product: half a spacing of 2^-7, at most
    2^-8 / (1 + 2^-8) of the value (+ the above), asserted as 2^-8 * |want| — ratios up to 0.9962 are this bound being tight;
  * sums: fp32 accumulation in a fixed order, per entry |got - want| <= TOL32 * sum|terms| (TOL32 = 2e-5 = 335 * 2^-24 covers
    the longest chain here, 16 + 16 + 128 additions); sum|terms| comes from the reference alone.  A dropped pixel moves a sum
    by about sum|terms| / HW >= 1e-4 * sum|terms| at every shape below: it cannot hide;
  * a second call is bit-identical.
Function level (`against_definition`): ops.modconv_noise_act and ops.conv2d on the fast path at the same edge shapes against
float64 autograd of their docstring formulas, in the project's bands (TOL32 / TOLBF of the reference's max-abs).

With STYLEX_BWD_GLUE_RECORD=<file> every test case leaves one line in that file: its worst error / tolerance
(profiles/bwd_glue_errors.txt is the record of one run)."""
import ctypes
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _bwd_glue_defs as D  # noqa: E402
import hip_backend as hb  # noqa: E402
import ops  # noqa: E402

DEV = "cuda:0"
TOL32, TOLBF = 2e-5, 4e-2
EW = {"fp32": 2.0 ** -22, "bf16": 2.0 ** -8}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
RSQRT2 = 2 ** -0.5


@pytest.fixture(autouse=True)
def hip_impl():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    prev = ops.use_impl(ops.HipOps)
    ops.set_precision("fp32")
    hb.load_library()  # fails loudly if the extension is missing
    yield
    ops.set_precision("fp32")
    ops.use_impl(prev)


# ---- bookkeeping: worst error / tolerance per test case ---------------------------------------------------------------
_LINES = []
_INPUTS = {}


class Recorder:
    def __init__(self):
        self.worst, self.what, self.notes, self.each = 0.0, "", [], None

    def ratio(self, r, what):
        """Record err / tol of one quantity, then assert it."""
        r = float(r)
        if not r <= self.worst:  # also true for NaN
            self.worst, self.what = r, what
        if self.each is not None:
            self.each.append("%s %.4f" % (what, r))
        assert r <= 1.0, "%s: error / tolerance = %.4g" % (what, r)

    def note(self, s):
        self.notes.append(s)


@pytest.fixture
def rec(request):
    r = Recorder()
    yield r
    name = request.node.nodeid.split("::", 1)[-1]
    _LINES.append("%-118s %8.4f  %s%s" % (name, r.worst, r.what, "".join("  [%s]" % n for n in r.notes + (r.each or []))))


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    _INPUTS.clear()
    out = os.environ.get("STYLEX_BWD_GLUE_RECORD")
    if out and _LINES:
        with open(out, "w") as f:
            f.write("# tests/test_bwd_glue_gpu.py: per test case, the worst observed error / tolerance (<= 1 passes) and the quantity\n"
                    "# that gave it; function level: [every quantity].  Kernel-level tolerances: 2^-22 |want| (fp32) / 2^-8 |want|\n"
                    "# (bf16; 0.9961 = a value just above a power of two rounded at a tie) elementwise, 2e-5 * sum|terms| for sums;\n"
                    "# function level: 2e-5 (fp32) / 4e-2 (bf16) of the reference's max-abs.\n")
            f.write("\n".join(_LINES) + "\n")


def _worst(got, want, lim):
    """max |got - want| / lim; where lim == 0 (want == 0, or a sum without terms) the result must be exactly zero."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    if not torch.isfinite(got).all() or (err[lim == 0] != 0).any():
        return float("inf")
    nz = lim > 0
    return (err[nz] / lim[nz]).max().item() if nz.any() else 0.0


def ew_ratio(got, want, prec):
    return _worst(got, want, EW[prec] * want.detach().double().cpu().abs())


def sum_ratio(got, want, abs_terms):
    return _worst(got, want, TOL32 * abs_terms.double())


def dev_cl(t):
    t = t.to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


# ---- kernel level ----------------------------------------------------------------------------------------------------
SHAPES = [
    (1, 4, 2, 2),       # one channel vector, 256 pixel rows against 4 pixels
    (3, 12, 9, 9),      # 3 vectors, 85 rows, one idle lane; 81 px -> chunks of 41 and 40
    (2, 40, 10, 13),    # 10 vectors, 25 rows, 6 idle lanes; 130 px -> 44 / 44 / 42; ns = 16: ns, H and W all differ
    (2, 516, 5, 5),     # 129 vectors, one row, 127 idle lanes
    (2, 1024, 4, 4),    # the channel limit
    (64, 512, 4, 4),    # the real 4 px tail; flat path over 1024 pixels
    (5, 64, 24, 40),    # flat: reduce_chunks says 75, the wrapper clamps to 64 -> ranges of 75 px cross images; per sample: 15 chunks
    (8, 64, 64, 64),    # fp32 only: flat path on the byte-count branch of the clamp (512 -> 128)
]
SHAPE_PREC = [(s, p) for s in SHAPES for p in ("fp32", "bf16") if not (s == (8, 64, 64, 64) and p == "bf16")]
SP_IDS = ["%s-%s" % ("x".join(map(str, s)), p) for s, p in SHAPE_PREC]


def inputs(shape, prec):
    """Seeded inputs of one (shape, precision), rounded to the activation dtype; device copies (channels_last) and the same
    values on the CPU.  About 1 % of y is exactly +0.0 or -0.0.  Shared by the tests of the shape and never written."""
    key = (shape, prec)
    if key in _INPUTS:
        return _INPUTS[key]
    B, C, H, W = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    dt = DT[prec]
    r = {}
    for name in ("dy", "y", "x", "t"):
        r[name] = torch.randn(B, C, H, W, generator=g).to(dt)
    yf = r["y"].view(-1)
    u = torch.rand(yf.numel(), generator=g)
    yf[u < 0.005] = 0.0
    yf[(u >= 0.005) & (u < 0.01)] = -0.0
    yf[0], yf[yf.numel() - 1] = 0.0, -0.0  # also at the smallest shape
    for extra in (0, 3):
        ns = max(H, W) + extra
        r["noise%d" % extra] = torch.rand(B, ns, ns, generator=g)
    r["nw"], r["nb"] = torch.randn(C, generator=g), torch.randn(C, generator=g)
    r["d"] = torch.rand(B, C, generator=g) + 0.5
    r["dev"] = {k: dev_cl(v) for k, v in r.items()}
    _INPUTS[key] = r
    return r


ACT_MODES = {
    # name: (lrelu, scale, want_dx, want_sum, per_sample, pass y)
    "lrelu": (True, 1.0, True, True, False, True),
    "lrelu-rsqrt2": (True, RSQRT2, True, True, False, True),
    "none-rsqrt2": (False, RSQRT2, True, True, False, False),
    "relu": ("relu", 1.0, True, True, False, True),
    "sum-only-per-sample": (False, 1.0, False, True, True, False),   # gp_tangent's call
    "sum-only-rsqrt2-flat": (False, RSQRT2, False, True, False, False),  # ops._channel_sum's call
    "lrelu-no-sum": (True, 1.0, True, False, False, True),
}


def test_wrapper_chunk_counts_are_the_ones_the_shapes_are_named_for():
    """The geometry the shape table relies on (stylex_reduce_chunks and the flat clamp of hb.act_bwd_reduce)."""
    lib = hb.load_library()
    chunks = lambda b, h, w, c: lib.stylex_reduce_chunks(hb._shape(b, h, w, c))
    assert chunks(3, 9, 9, 12) == 2 and chunks(2, 10, 13, 40) == 3 and chunks(5, 24, 40, 64) == 15
    assert chunks(1, 5 * 24, 40, 64) == 75 and chunks(1, 8 * 64, 64, 64) == 512 and chunks(1, 64 * 4, 4, 512) == 16


@pytest.mark.parametrize("mode", list(ACT_MODES))
@pytest.mark.parametrize("shape,prec", SHAPE_PREC, ids=SP_IDS)
def test_act_bwd_reduce(shape, prec, mode, rec):
    lrelu, scale, want_dx, want_sum, per_sample, with_y = ACT_MODES[mode]
    a = inputs(shape, prec)
    dy, y = a["dev"]["dy"], a["dev"]["y"] if with_y else None
    want = D.act_bwd(a["dy"], a["y"] if with_y else None, lrelu, scale)
    dx, s = hb.act_bwd_reduce(dy, y, lrelu, scale, want_dx=want_dx, want_sum=want_sum, per_sample=per_sample)
    dx2, s2 = hb.act_bwd_reduce(dy, y, lrelu, scale, want_dx=want_dx, want_sum=want_sum, per_sample=per_sample)
    assert (dx is not None) == want_dx and (s is not None) == want_sum
    if want_dx:
        assert dx.dtype == dy.dtype and dx.shape == dy.shape and hb.is_cl(dx)
        assert torch.equal(dx, dx2), "second call differs (dx)"
        rec.ratio(ew_ratio(dx, want.dx, prec), "dx")
    if want_sum:
        assert s.dtype == torch.float32 and torch.equal(s, s2), "second call differs (sum)"
        if per_sample:
            rec.ratio(sum_ratio(s, want.sum_hw, want.abs_hw), "sum over (h,w)")
        else:
            rec.ratio(sum_ratio(s, want.sum_bhw, want.abs_bhw), "sum over (b,h,w)")


PREP_CASES = {
    # name: (noise key or None, gz_scale, lrelu)
    "ns=max": ("noise0", False, True),
    "ns=max-scaled": ("noise0", True, True),
    "ns=max+3": ("noise3", False, True),
    "ns=max+3-scaled": ("noise3", True, True),
    "no-noise": (None, False, True),
    "no-noise-scaled": (None, True, True),
    "linear-ns=max+3-scaled": ("noise3", True, False),
}


@pytest.mark.parametrize("case", list(PREP_CASES))
@pytest.mark.parametrize("shape,prec", SHAPE_PREC, ids=SP_IDS)
def test_modconv_bwd_prep(shape, prec, case, rec):
    nkey, scaled, lrelu = PREP_CASES[case]
    a = inputs(shape, prec)
    dv = a["dev"]
    noise, nw, nb = (dv[nkey], dv["nw"], dv["nb"]) if nkey else (None, None, None)
    want = D.modconv_prep(a["dy"], a["y"], a[nkey] if nkey else None, a["nw"], a["nb"], lrelu, a["d"] if scaled else None)
    run = lambda: hb.modconv_bwd_prep(dv["dy"], dv["y"], noise, nw, nb, lrelu, gz_scale=dv["d"] if scaled else None)
    gz, S = run()
    gz2, S2 = run()
    assert gz.dtype == dv["dy"].dtype and hb.is_cl(gz) and S.dtype == torch.float32 and tuple(S.shape) == (shape[0], 3, shape[1])
    assert torch.equal(gz, gz2) and torch.equal(S, S2), "second call differs"
    rec.ratio(ew_ratio(gz, want.gz, prec), "gz")
    for k, name in enumerate(("S0 = sum gz*(t - noise)", "S1 = sum gz*plane", "S2 = sum gz")):
        rec.ratio(sum_ratio(S[:, k], want.S[:, k], want.abs_S[:, k]), name)


@pytest.mark.parametrize("want_gx", [True, False], ids=["gx", "no-gx"])
@pytest.mark.parametrize("shape,prec", SHAPE_PREC, ids=SP_IDS)
def test_scale_reduce(shape, prec, want_gx, rec):
    a = inputs(shape, prec)
    dv = a["dev"]
    want = D.scale_reduce(a["x"], a["t"], a["d"])
    gx, s = hb.scale_reduce(dv["x"], dv["t"], dv["d"], want_gx=want_gx)
    gx2, s2 = hb.scale_reduce(dv["x"], dv["t"], dv["d"], want_gx=want_gx)
    assert (gx is not None) == want_gx and torch.equal(s, s2), "second call differs (sum)"
    if want_gx:
        assert gx.dtype == dv["t"].dtype and hb.is_cl(gx) and torch.equal(gx, gx2), "second call differs (gx)"
        rec.ratio(ew_ratio(gx, want.gx, prec), "gx")
    rec.ratio(sum_ratio(s, want.sum_hw, want.abs_hw), "sum x*t")


# ---- the C entry points with a caller-chosen chunk count ----------------------------------------------------------------
# (2, 8, 3, 3): 9 pixels.  4 chunks of ceil(9 / 4) = 3 px leave the fourth empty, 12 chunks exceed the pixel count.  In bounds
# by make_geo: p_end is clipped to HW, p_begin >= HW then runs no iteration, and partial has nchunks rows.
CAPI_SHAPE = (2, 8, 3, 3)


def _written_and_empty_rows_zero(partial, nch, hw):
    assert not torch.isnan(partial).any(), "rows of partial left unwritten"
    per = -(-hw // nch)
    for chunk in range(nch):
        if chunk * per >= hw:
            assert (partial[:, chunk] == 0).all(), "an empty pixel range must write zeros (chunk %d)" % chunk


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("nch", [1, 4, 9, 12])
def test_act_bwd_reduce_capi_with_given_nchunks(nch, prec, rec):
    B, C, H, W = CAPI_SHAPE
    a = inputs(CAPI_SHAPE, prec)
    dy, y = a["dev"]["dy"], a["dev"]["y"]
    lib = hb._ensure_device(dy)
    want = D.act_bwd(a["dy"], a["y"], True, RSQRT2)
    outs = []
    for _ in range(2):
        partial = torch.full((B, nch, C), float("nan"), device=DEV)
        dx = hb.empty_cl(tuple(dy.shape), dy)
        rc = lib.stylex_act_bwd_reduce(hb._ptr(dy), hb._ptr(y), hb._ptr(dx), hb._ptr(partial), hb._shape(B, H, W, C), nch, 1,
                                       ctypes.c_float(RSQRT2), hb._adt(dy), hb._stream())
        assert rc == 0
        outs.append((dx, partial))
    (dx, partial), (dx2, partial2) = outs
    _written_and_empty_rows_zero(partial, nch, H * W)
    assert torch.equal(dx, dx2) and torch.equal(partial, partial2)
    rec.ratio(ew_ratio(dx, want.dx, prec), "dx")
    rec.ratio(sum_ratio(partial.sum(dim=1), want.sum_hw, want.abs_hw), "sum over chunks")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("nch", [1, 4, 9, 12])
def test_modconv_bwd_prep_capi_with_given_nchunks(nch, prec, rec):
    B, C, H, W = CAPI_SHAPE
    a = inputs(CAPI_SHAPE, prec)
    dv = a["dev"]
    gy, y, noise = dv["dy"], dv["y"], dv["noise3"]
    lib = hb._ensure_device(gy)
    want = D.modconv_prep(a["dy"], a["y"], a["noise3"], a["nw"], a["nb"], True, None)
    outs = []
    for _ in range(2):
        partial = torch.full((B, nch, 3, C), float("nan"), device=DEV)
        gz = hb.empty_cl(tuple(gy.shape), gy)
        rc = lib.stylex_modconv_bwd_prep(hb._ptr(gy), hb._ptr(y), hb._ptr(noise), noise.shape[1], hb._ptr(dv["nw"]), hb._ptr(dv["nb"]),
                                         hb._ptr(gz), hb._ptr(partial), hb._shape(B, H, W, C), nch, 1, hb._adt(gy), hb._stream())
        assert rc == 0
        outs.append((gz, partial))
    (gz, partial), (gz2, partial2) = outs
    _written_and_empty_rows_zero(partial, nch, H * W)
    assert torch.equal(gz, gz2) and torch.equal(partial, partial2)
    rec.ratio(ew_ratio(gz, want.gz, prec), "gz")
    S = partial.sum(dim=1)
    for k in range(3):
        rec.ratio(sum_ratio(S[:, k], want.S[:, k], want.abs_S[:, k]), "S%d over chunks" % k)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_modconv_bwd_prep_refuses_relu(prec):
    """The prologue needs the pre-activation, which a ReLU output of 0 does not determine: mode "relu" (2) is an error, for
    both entry points, and nothing is launched (the NaN-filled outputs stay NaN)."""
    a = inputs(CAPI_SHAPE, prec)
    dv = a["dev"]
    gy, y = dv["dy"], dv["y"]
    B, C, H, W = CAPI_SHAPE
    with pytest.raises(hb.StylexHipError):
        hb.modconv_bwd_prep(gy, y, None, None, None, "relu")
    with pytest.raises(hb.StylexHipError):
        hb.modconv_bwd_prep(gy, y, dv["noise0"], dv["nw"], dv["nb"], "relu", gz_scale=dv["d"])
    lib = hb._ensure_device(gy)
    nan = float("nan")
    partial = torch.full((B, 1, 3, C), nan, device=DEV)
    gz = torch.full(tuple(gy.shape), nan, device=DEV, dtype=gy.dtype).contiguous(memory_format=torch.channels_last)
    for lrelu in (2, -1, 3):
        assert lib.stylex_modconv_bwd_prep(hb._ptr(gy), hb._ptr(y), None, 0, None, None, hb._ptr(gz), hb._ptr(partial),
                                           hb._shape(B, H, W, C), 1, lrelu, hb._adt(gy), hb._stream()) == -1  # STYLEX_EINVAL
        assert lib.stylex_modconv_bwd_prep_scaled(hb._ptr(gy), hb._ptr(y), None, 0, None, None, hb._ptr(dv["d"]), hb._ptr(gz),
                                                  hb._ptr(partial), hb._shape(B, H, W, C), 1, lrelu, hb._adt(gy), hb._stream()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(partial).all() and torch.isnan(gz).all()


# ---- resampling copies ------------------------------------------------------------------------------------------------
RESAMPLE_SHAPES = [(2, 8, 5, 7), (1, 6, 6, 6), (2, 4, 3, 3)]  # 16-byte vectors (8 x bf16 / 4 x fp32), scalar (C % 4 != 0), 4-vectors


def _resample_inputs(shape, prec, view):
    """x [B,C,H,W] and a half-resolution tensor, channels_last on the device.  view: both are the batch slice [1:] of a tensor
    with one more sample — in bf16 at (*, 4, 3, 3) the slice starts 72 bytes in: 8-byte aligned only, LAUNCH_EW's scalar fallback."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, prec, view)).encode()))
    nb = B + 1 if view else B
    big = dev_cl(torch.randn(nb, C, H, W, generator=g).to(DT[prec]))
    half = dev_cl(torch.randn(nb, C, (H + 1) // 2, (W + 1) // 2, generator=g).to(DT[prec]))
    if view:
        x, s = big[1:], half[1:]
        assert hb.is_cl(x) and hb.is_cl(s)
        if prec == "bf16" and shape == (2, 4, 3, 3):
            assert x.data_ptr() % 16 == 8
        return big, x, s
    return big, big, half


RESAMPLE_CASES = [(s, p, False) for s in RESAMPLE_SHAPES for p in ("fp32", "bf16")] + [((2, 4, 3, 3), "bf16", True)]
RESAMPLE_IDS = ["%s-%s%s" % ("x".join(map(str, s)), p, "-view" if v else "") for s, p, v in RESAMPLE_CASES]


@pytest.mark.parametrize("shape,prec,view", RESAMPLE_CASES, ids=RESAMPLE_IDS)
def test_subsample2_and_its_adjoint_are_exact_copies(shape, prec, view, rec):
    _, x, s = _resample_inputs(shape, prec, view)
    B, C, H, W = shape
    y = hb.subsample2_fwd(x)
    assert torch.equal(y.cpu(), x.cpu()[:, :, ::2, ::2])
    want = torch.zeros(B, C, H, W, dtype=x.dtype)
    want[:, :, ::2, ::2] = s.cpu()
    dx = hb.subsample2_bwd(s, (H, W))
    assert tuple(dx.shape) == (B, C, H, W) and hb.is_cl(dx)
    assert torch.equal(dx.cpu(), want)  # (+0.0 == -0.0: the inserted zeros may carry either sign)
    if view:  # the half-resolution slice is 16-byte aligned; the misaligned full-size slice as the INPUT of the adjoint
        for hw in ((2 * H - 1, 2 * W), (2 * H, 2 * W - 1)):
            want = torch.zeros(B, C, *hw, dtype=x.dtype)
            want[:, :, ::2, ::2] = x.cpu()
            assert torch.equal(hb.subsample2_bwd(x, hw).cpu(), want)
    rec.ratio(0.0, "exact")


@pytest.mark.parametrize("shape,prec,view", RESAMPLE_CASES, ids=RESAMPLE_IDS)
def test_add_at_even(shape, prec, view, rec):
    big, x, s = _resample_inputs(shape, prec, view)
    before_big, before, src = big.cpu().clone(), x.cpu().clone(), s.cpu().clone()
    out = hb.add_at_even_(x, s)
    assert out is x
    got = x.cpu()
    odd = torch.ones(got.shape, dtype=torch.bool)
    odd[:, :, ::2, ::2] = False
    assert torch.equal(got[odd], before[odd]), "pixels off the even grid changed"
    if view:
        assert torch.equal(big.cpu()[0], before_big[0]), "the sample before the view changed"
    want64 = before[:, :, ::2, ::2].double() + src.double()
    if prec == "fp32":  # one IEEE addition: the correctly rounded sum
        assert torch.equal(got[:, :, ::2, ::2], before[:, :, ::2, ::2] + src)
    rec.ratio(ew_ratio(got[:, :, ::2, ::2], want64, prec), "dst + src")


# ---- function level: the fast-path Functions against float64 autograd of their formulas ----------------------------------
def close_ratio(got, want, tol):
    """close() of test_hip_parity.py as a ratio: max error / (tol * max(1e-3, max|want|))."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    return (got - want).abs().max().item() / (tol * max(1e-3, want.abs().max().item()))


def lrelu_by_saved_output(pre, y_gpu, tol_fwd, rec):
    """LeakyReLU of the float64 pre-activation with the branch taken from the kernel's OUTPUT (the backward's contract is in
    terms of the saved y; a pre-activation near zero may round to the other sign).  Condition, asserted: every element whose
    branch differs from sign(pre) has |pre| <= tol_fwd * max|pre|, and they are at most 1e-3 of the tensor."""
    rec.each = []  # function level: every quantity's ratio goes into the record, not only the worst
    pos = y_gpu.detach().cpu() > 0
    p = pre.detach()
    flip = pos != (p > 0)
    n = int(flip.sum())
    rec.note("%d of %d branches differ" % (n, p.numel()))
    if n:
        rec.ratio(p[flip].abs().max().item() / (tol_fwd * p.abs().max().item()), "|pre| where the branch differs")
        rec.ratio(n / (1e-3 * p.numel()), "fraction of differing branches / 1e-3")
    return torch.where(pos, pre, 0.2 * pre)


def rounded(t, prec):
    return t.to(DT[prec]).float()


MODCONV_CASES = [
    # B, Cin, Cout, H, W, ns
    (3, 12, 12, 9, 9, 12),       # the small geometry of the kernel tests (natural-order noise plane)
    (2, 40, 40, 10, 13, 16),     # non-square
    (2, 64, 40, 8, 8, 8),        # bf16: the `pre` branch (modulation applied up front), with the fold
    (2, 6, 12, 9, 9, 9),         # Cin % 4 != 0: the ATen branch beside scale_reduce; transposed-read noise plane
    (16, 512, 512, 4, 4, 4),     # the 4 px tail at real width
]
MODCONV_PARAMS = [(c, "fp32", "1") for c in MODCONV_CASES] + [(c, "bf16", f) for c in MODCONV_CASES for f in ("1", "0")]
MODCONV_IDS = ["%s-%s-fold%s" % ("x".join(map(str, c[:5])), p, f) for c, p, f in MODCONV_PARAMS]


@pytest.mark.against_definition
@pytest.mark.parametrize("case,prec,fold", MODCONV_PARAMS, ids=MODCONV_IDS)
def test_modconv_noise_act_fast_path_vs_float64(case, prec, fold, rec, monkeypatch):
    """y = lrelu(d[b,o] * conv(x * (style+1)[b,i], W) + inoise[b,w,h] * nw[o] + nb[o]),  d = rsqrt(((style+1)^2) @ sum_k W^2 + eps)
    (HipOps.modulated_conv2d's docstring plus the noise plane) and the gradients of sum(y * r) with respect to x, style, W, nw, nb."""
    B, Ci, Co, H, W, ns = case
    monkeypatch.setenv("STYLEX_FOLD_D", fold)
    tol = TOL32 if prec == "fp32" else TOLBF
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    x = rounded(torch.randn(B, Ci, H, W, generator=g), prec)
    style = torch.randn(B, Ci, generator=g) * 0.5
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5
    nw, nb = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    inoise = torch.rand(B, ns, ns, 1, generator=g)
    r = rounded(torch.randn(B, Co, H, W, generator=g), prec)

    ops.set_precision(prec)
    prev = ops.set_fast(True)
    try:
        leaves = [dev_cl(x).requires_grad_()] + [t.to(DEV).requires_grad_() for t in (style, w, nw, nb)]
        y = ops.modconv_noise_act(leaves[0], leaves[1], leaves[2], inoise.to(DEV), leaves[3], leaves[4])
        assert y.dtype == DT[prec] and "ModConvFast" in type(y.grad_fn).__name__
        (y.float() * dev_cl(r)).sum().backward()
        grads = [t.grad for t in leaves]
    finally:
        ops.set_fast(prev)

    ref = [t.double().requires_grad_() for t in (x, style, w, nw, nb)]
    xr, sr, wr, nwr, nbr = ref
    s1 = sr + 1
    d = torch.rsqrt((s1 * s1) @ wr.pow(2).sum(dim=(2, 3)).t() + 1e-8)
    plane = D.noise_plane(inoise[:, :, :, 0], H, W)[:, None]
    pre = d[:, :, None, None] * F.conv2d(xr * s1[:, :, None, None], wr, None, 1, 1) + plane * nwr.view(1, -1, 1, 1) + nbr.view(1, -1, 1, 1)
    y_ref = lrelu_by_saved_output(pre, y, tol, rec)
    (y_ref * r.double()).sum().backward()
    rec.ratio(close_ratio(y, y_ref, tol), "y")
    for name, got, want in zip(("x", "style", "weight", "noise_w", "noise_b"), grads, ref):
        assert got is not None, name
        rec.ratio(close_ratio(got, want.grad, tol), "grad " + name)


def test_modconv_backward_follows_the_forward_plan_not_the_environment(monkeypatch):
    """STYLEX_FOLD_D is read once, when the forward builds the plan: flipping it before .backward() changes no bit of the
    five gradients, whichever way round (2x64x40x8x8, side 8, bf16: the `pre` layer, "folded" against "prescaled")."""
    B, Ci, Co, H, W, ns = 2, 64, 40, 8, 8, 8
    g = torch.Generator().manual_seed(5)
    x = rounded(torch.randn(B, Ci, H, W, generator=g), "bf16")
    style = torch.randn(B, Ci, generator=g) * 0.5
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5
    nw, nb = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    inoise = torch.rand(B, ns, ns, 1, generator=g).to(DEV)
    r = dev_cl(rounded(torch.randn(B, Co, H, W, generator=g), "bf16"))

    def grads(fold_fwd, fold_bwd):
        monkeypatch.setenv("STYLEX_FOLD_D", fold_fwd)
        leaves = [dev_cl(x).requires_grad_()] + [t.to(DEV).requires_grad_() for t in (style, w, nw, nb)]
        y = ops.modconv_noise_act(leaves[0], leaves[1], leaves[2], inoise, leaves[3], leaves[4])
        assert "ModConvFast" in type(y.grad_fn).__name__
        assert y.grad_fn.plan.dgrad == ("folded" if fold_fwd == "1" else "prescaled")
        monkeypatch.setenv("STYLEX_FOLD_D", fold_bwd)
        (y.float() * r).sum().backward()
        return [t.grad for t in leaves]

    ops.set_precision("bf16")
    prev = ops.set_fast(True)
    try:
        for fwd, bwd in (("0", "1"), ("1", "0")):
            for name, got, want in zip(("x", "style", "weight", "noise_w", "noise_b"), grads(fwd, bwd), grads(fwd, fwd)):
                assert got is not None and torch.equal(got, want), (fwd, bwd, name)
    finally:
        ops.set_fast(prev)


def test_conv_double_backward_follows_the_forward_plan_not_the_environment(monkeypatch):
    """STYLEX_RES_GEMM_DD is read once, when ops.conv2d builds the plan: the nodes that the gradient penalty's two backward
    passes create take the launch record of their forward, so setting the switch to 0 after the forward changes no bit of
    the gradients (2x16x8x8, bf16: a 1x1 conv with bias on the GEMM route, then a 3x3 conv with LeakyReLU, composable
    Functions).  The penalty of a piecewise-linear network does not depend on x: its gradient is None in either run.
    Not asserted: that a run with the switch off from the start differs.  At this shape (K = 16) hipBLASLt and the
    project's kernel give the same bits (tools/conv_bits.py: the hashes with STYLEX_RES_GEMM_DD=0 equal the default's)."""
    import stylex_train as st

    g = torch.Generator().manual_seed(17)
    x = rounded(torch.randn(2, 16, 8, 8, generator=g), "bf16")
    w1, b1 = torch.randn(16, 16, 1, 1, generator=g) / 4, torch.randn(16, generator=g)
    w2 = torch.randn(16, 16, 3, 3, generator=g) / 12

    def grads(dd_forward, dd_backward):
        """Gradients of x, w1, w2 with the switch at `dd_forward` (None: unset) in the forward and `dd_backward` after it."""
        monkeypatch.delenv("STYLEX_RES_GEMM_DD", raising=False)
        if dd_forward is not None:
            monkeypatch.setenv("STYLEX_RES_GEMM_DD", dd_forward)
        xd, w1d, b1d, w2d = [t.to(DEV).requires_grad_() for t in (x, w1, b1, w2)]
        y = ops.conv2d(ops.conv2d(xd, w1d, b1d), w2d, None, 1, 1, lrelu=True)
        assert "ConvBiasActDD" in type(y.grad_fn).__name__
        first = y.grad_fn.next_functions[0][0]
        assert "ConvBiasActDD" in type(first).__name__ and first.epi.launch.gemm is (dd_forward != "0")
        if dd_backward is not None:
            monkeypatch.setenv("STYLEX_RES_GEMM_DD", dd_backward)
        st.gradient_norms(xd, y).mean().backward()
        return [xd.grad, w1d.grad, w2d.grad]

    ops.set_precision("bf16")
    prev = ops.set_fast(False)
    try:
        untouched, flipped = grads(None, None), grads(None, "0")
    finally:
        ops.set_fast(prev)
    assert untouched[0] is None and flipped[0] is None
    for name, a, b in zip(("w1", "w2"), untouched[1:], flipped[1:]):
        assert a is not None and torch.equal(a, b), name


@pytest.mark.against_definition
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", [(3, 12, 12, 9, 9), (5, 64, 64, 24, 40)], ids=["3x12x12x9x9", "5x64x64x24x40"])
def test_conv_residual_lrelu_fast_path_vs_float64(case, prec, rec):
    """y = lrelu((conv(x, W) + b + res) * 2^-0.5) and the gradients of sum(y * r) with respect to x, W, b, res: the
    flat act_bwd_reduce (activation derivative, scale, bias sum) between the conv launches."""
    B, Ci, Co, H, W = case
    tol = TOL32 if prec == "fp32" else TOLBF
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    x = rounded(torch.randn(B, Ci, H, W, generator=g), prec)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5
    b = torch.randn(Co, generator=g)
    res = rounded(torch.randn(B, Co, H, W, generator=g), prec)
    r = rounded(torch.randn(B, Co, H, W, generator=g), prec)

    ops.set_precision(prec)
    prev = ops.set_fast(True)
    try:
        leaves = [dev_cl(x).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_(), dev_cl(res).requires_grad_()]
        y = ops.conv2d(leaves[0], leaves[1], leaves[2], 1, 1, lrelu=True, residual=leaves[3], res_scale=RSQRT2)
        assert y.dtype == DT[prec] and "ConvBiasActFast" in type(y.grad_fn).__name__
        (y.float() * dev_cl(r)).sum().backward()
        grads = [t.grad for t in leaves]
    finally:
        ops.set_fast(prev)

    ref = [t.double().requires_grad_() for t in (x, w, b, res)]
    xr, wr, br, rr = ref
    pre = (F.conv2d(xr, wr, br, 1, 1) + rr) * RSQRT2
    y_ref = lrelu_by_saved_output(pre, y, tol, rec)
    (y_ref * r.double()).sum().backward()
    rec.ratio(close_ratio(y, y_ref, tol), "y")
    for name, got, want in zip(("x", "weight", "bias", "res"), grads, ref):
        assert got is not None, name
        rec.ratio(close_ratio(got, want.grad, tol), "grad " + name)
