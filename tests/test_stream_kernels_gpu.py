"""-m gpu: the streaming kernels with 16-byte lanes — the strip forms of the bilinear x2 pair (csrc/elementwise.hip) and the
8-channel lanes of the backward glue reductions modconv_bwd_prep and scale_reduce (csrc/fused_bwd.hip; act_bwd_reduce has
no such form: tests/test_bwd_glue_gpu.py is its contract) — against the kernels they stand in for and against
float64 definitions.  bf16 throughout (the only mode that takes them).

Bounds, none of them tuned:
  * a strip / wide kernel and its generic form run the same fma / product sequence per element: elementwise outputs are
    compared with torch.equal;
  * against float64: ONE round-to-nearest-even bf16 store of a value whose fp32 evaluation is exact to 2^-22, asserted as
    2^-8 * |want| (the bound of tests/test_bwd_glue_gpu.py); where want == 0 the result must be zero;
  * sums: |got - want| <= 2e-5 * sum|terms| (TOL32 of tests/test_bwd_glue_gpu.py: chains of up to 335 fp32 additions), and
    torch.equal between the 8- and the 4-channel lanes: a wide lane adds, per channel, the pixels of the 4-channel lane of
    that channel in its order, and the block's LDS pass adds the same rows in the same order (a training run must not depend
    on the lane width: the untrained GAN amplifies a last-bit difference of a gradient sum within a few steps);
  * a second call is bit-identical;
  * the comparisons are between forms built to agree, so one test reads the kernel names from the profiler: the strip / wide
    kernels are the ones launched at the default settings, the direct / 4-channel ones under the switches and for C % 8 != 0."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import _bwd_glue_defs as D  # noqa: E402
import hip_backend as hb  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
EW_TOL, SUM_TOL = 2.0 ** -8, 2e-5


@pytest.fixture(autouse=True)
def _lib():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    hb.load_library()


def dev_cl(t):
    t = t.to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def worst(got, want, lim):
    """max |got - want| / lim; where lim == 0 the result must be exactly zero."""
    got, want, lim = got.detach().double().cpu(), want.detach().double().cpu(), lim.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs()
    if not torch.isfinite(got).all() or (err[lim == 0] != 0).any():
        return float("inf")
    nz = lim > 0
    return (err[nz] / lim[nz]).max().item() if nz.any() else 0.0


def check(ratio, what):
    print("%s: error / tolerance = %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: error / tolerance = %.4g" % (what, ratio)


# ---- bilinear x2 ------------------------------------------------------------------------------------------------------
# one strip is 8 input rows: (2,8,2,2) less than one (the generic kernels serve it under both settings), (1,24,9,5) one and
# a ragged second of one row, (2,40,17,16) two and a ragged third, (1,8,8,33) exactly one; W = 2 / 5 clamp both borders in
# neighbouring columns; 24 and 40 channels are 3 and 5 vectors per pixel.
UP_SHAPES = [(2, 8, 2, 2), (1, 24, 9, 5), (2, 40, 17, 16), (1, 8, 8, 33)]
UP_IDS = ["x".join(map(str, s)) for s in UP_SHAPES]
_UP = {}


def up_matrix(n):
    """U [2n, n] of the index rule: out[2k] = .25 in[k-1] + .75 in[k], out[2k+1] = .75 in[k] + .25 in[k+1], clamped."""
    u = torch.zeros(2 * n, n, dtype=F64)
    for k in range(n):
        u[2 * k, max(k - 1, 0)] += 0.25
        u[2 * k, k] += 0.75
        u[2 * k + 1, k] += 0.75
        u[2 * k + 1, min(k + 1, n - 1)] += 0.25
    return u


def up_fwd64(x):
    return torch.einsum("ph,bchw,qw->bcpq", up_matrix(x.shape[2]), x.double(), up_matrix(x.shape[3]))


def up_bwd64(dy):
    return torch.einsum("ph,bcpq,qw->bchw", up_matrix(dy.shape[2] // 2), dy.double(), up_matrix(dy.shape[3] // 2))


def up_inputs(shape):
    if shape not in _UP:
        B, C, H, W = shape
        g = gen("up", shape)
        x = torch.randn(B, C, H, W, generator=g).to(BF)
        dy = torch.randn(B, C, 2 * H, 2 * W, generator=g).to(BF)
        _UP[shape] = dict(x=x, dy=dy, xd=dev_cl(x), dyd=dev_cl(dy), fwd=up_fwd64(x), bwd=up_bwd64(dy))
    return _UP[shape]


@pytest.mark.parametrize("shape", UP_SHAPES, ids=UP_IDS)
def test_upsample_strip_forward(shape, monkeypatch):
    a = up_inputs(shape)
    y = hb.upsample2x_fwd(a["xd"])
    y2 = hb.upsample2x_fwd(a["xd"])
    monkeypatch.setenv("STYLEX_UPSAMPLE_STRIP", "0")
    y_generic = hb.upsample2x_fwd(a["xd"])
    assert y.dtype == BF and hb.is_cl(y) and tuple(y.shape) == (shape[0], shape[1], 2 * shape[2], 2 * shape[3])
    assert torch.equal(y, y_generic), "strip and generic kernels differ"
    assert torch.equal(y, y2), "second call differs"
    check(worst(y, a["fwd"], EW_TOL * a["fwd"].abs()), "upsample2x_fwd vs the float64 index rule")


@pytest.mark.parametrize("shape", UP_SHAPES, ids=UP_IDS)
def test_upsample_strip_adjoint(shape, monkeypatch):
    a = up_inputs(shape)
    B, C, H, W = shape
    probes = []
    for (p, q) in ((0, 0), (0, 2 * W - 1), (2 * H - 1, 0), (2 * H - 1, 2 * W - 1)):
        t = torch.zeros(B, C, 2 * H, 2 * W, dtype=BF)
        t[:, :, p, q] = 1.0
        probes.append(t)
    dx = hb.upsample2x_bwd(a["dyd"])
    dx2 = hb.upsample2x_bwd(a["dyd"])
    got_probes = [hb.upsample2x_bwd(dev_cl(t)) for t in probes]
    monkeypatch.setenv("STYLEX_UPSAMPLE_STRIP", "0")
    dx_generic = hb.upsample2x_bwd(a["dyd"])
    assert dx.dtype == BF and hb.is_cl(dx) and tuple(dx.shape) == shape
    assert torch.equal(dx, dx_generic), "strip and generic kernels differ"
    assert torch.equal(dx, dx2), "second call differs"
    check(worst(dx, a["bwd"], EW_TOL * a["bwd"].abs()), "upsample2x_bwd vs the float64 adjoint")
    for t, got in zip(probes, got_probes):  # every coefficient (1, 3/4, 1/4 and their products) is a bf16 number: exact
        assert torch.equal(got.cpu().double(), up_bwd64(t)), "one-hot probe at a corner"
        assert torch.equal(got, hb.upsample2x_bwd(dev_cl(t))), "one-hot probe: strip and generic kernels differ"


# ---- glue reductions --------------------------------------------------------------------------------------------------
# (2,8,3,5): one vector per pixel, 15 pixels against 128 pixel rows; (3,24,7,9): 3 vectors, 42 rows, two idle lanes, an odd
# pixel count (the two-pixel loop ends on a single); (1,40,16,16): 4 chunks of 64 px, 25 rows; (2,512,4,4): 64 vectors,
# 2 rows, four passes of the loop; (2,12,3,5): C % 8 != 0, the 4-channel lanes under both settings.
GLUE_SHAPES = [(2, 8, 3, 5), (3, 24, 7, 9), (1, 40, 16, 16), (2, 512, 4, 4), (2, 12, 3, 5)]
GLUE_IDS = ["x".join(map(str, s)) for s in GLUE_SHAPES]
_GLUE = {}


def glue_inputs(shape):
    """Seeded bf16 inputs; about 1 % of y is +0.0 or -0.0.  Shared by the tests of the shape and never written."""
    if shape in _GLUE:
        return _GLUE[shape]
    B, C, H, W = shape
    g = gen("glue", shape)
    r = {name: torch.randn(B, C, H, W, generator=g).to(BF) for name in ("dy", "y", "x", "t")}
    yf = r["y"].view(-1)
    u = torch.rand(yf.numel(), generator=g)
    yf[u < 0.005] = 0.0
    yf[(u >= 0.005) & (u < 0.01)] = -0.0
    yf[0], yf[yf.numel() - 1] = 0.0, -0.0
    ns = max(H, W) + 3
    r["noise"] = torch.rand(B, ns, ns, generator=g)  # transposed read: plane[b,h,w] = noise[b,w,h]
    r["nat"] = r["noise"].transpose(1, 2).contiguous()
    r["nw"], r["nb"] = torch.randn(C, generator=g), torch.randn(C, generator=g)
    r["d"] = torch.rand(B, C, generator=g) + 0.5
    r["dev"] = {k: dev_cl(v) for k, v in r.items()}
    _GLUE[shape] = r
    return r


def both_lanes(monkeypatch, run):
    """run() twice with the default lanes and once with STYLEX_GLUE_WIDE=0."""
    first, second = run(), run()
    monkeypatch.setenv("STYLEX_GLUE_WIDE", "0")
    narrow = run()
    monkeypatch.delenv("STYLEX_GLUE_WIDE")
    return first, second, narrow


ACT_MODES = {
    # name: (lrelu, scale, want_dx, per_sample, pass y)
    "lrelu-flat": (True, 1.0, True, False, True),
    "relu-rsqrt2-flat": ("relu", 2 ** -0.5, True, False, True),
    "none-rsqrt2-per-sample": (False, 2 ** -0.5, True, True, False),
    "sum-only-per-sample": (False, 1.0, False, True, False),
}


@pytest.mark.parametrize("mode", list(ACT_MODES))
@pytest.mark.parametrize("shape", GLUE_SHAPES, ids=GLUE_IDS)
def test_act_bwd_reduce_lanes(shape, mode, monkeypatch):
    """act_bwd_reduce has 4-channel lanes only: the switch must not change it, and the shapes of this file hold its bounds."""
    lrelu, scale, want_dx, per_sample, with_y = ACT_MODES[mode]
    a = glue_inputs(shape)
    dy, y = a["dev"]["dy"], a["dev"]["y"] if with_y else None
    want = D.act_bwd(a["dy"], a["y"] if with_y else None, lrelu, scale)
    run = lambda: hb.act_bwd_reduce(dy, y, lrelu, scale, want_dx=want_dx, want_sum=True, per_sample=per_sample)
    (dx, s), (dx2, s2), (dx4, s4) = both_lanes(monkeypatch, run)
    assert torch.equal(s, s2), "second call differs (sum)"
    if want_dx:
        assert torch.equal(dx, dx2), "second call differs (dx)"
        assert torch.equal(dx, dx4), "dx depends on STYLEX_GLUE_WIDE"
        check(worst(dx, want.dx, EW_TOL * want.dx.abs()), "dx")
    else:
        assert dx is None
    ref, terms = (want.sum_hw, want.abs_hw) if per_sample else (want.sum_bhw, want.abs_bhw)
    check(worst(s, ref, SUM_TOL * terms), "sum")
    check(worst(s4, ref, SUM_TOL * terms), "sum, 4-channel lanes")
    assert torch.equal(s, s4), "the sum depends on STYLEX_GLUE_WIDE"


PREP_CASES = {
    # name: (noise, gz_scale, lrelu)
    "noise": (True, False, True),
    "noise-scaled": (True, True, True),
    "no-noise": (False, False, True),
    "no-noise-scaled": (False, True, True),
    "linear-noise-scaled": (True, True, False),
}


@pytest.mark.parametrize("case", list(PREP_CASES))
@pytest.mark.parametrize("shape", GLUE_SHAPES, ids=GLUE_IDS)
def test_modconv_bwd_prep_lanes(shape, case, monkeypatch):
    noise, scaled, lrelu = PREP_CASES[case]
    a = glue_inputs(shape)
    dv = a["dev"]
    d = dv["d"] if scaled else None
    want = D.modconv_prep(a["dy"], a["y"], a["noise"] if noise else None, a["nw"], a["nb"], lrelu, a["d"] if scaled else None)
    if noise:
        run = lambda: hb.modconv_bwd_prep(dv["dy"], dv["y"], dv["noise"], dv["nw"], dv["nb"], lrelu, gz_scale=d)
        run_nat = lambda: hb.modconv_bwd_prep(dv["dy"], dv["y"], dv["nat"], dv["nw"], dv["nb"], lrelu, gz_scale=d, noise_natural=True)
    else:
        run = lambda: hb.modconv_bwd_prep(dv["dy"], dv["y"], None, None, None, lrelu, gz_scale=d)
        run_nat = None
    (gz, S), (gz2, S2), (gz4, S4) = both_lanes(monkeypatch, run)
    assert gz.dtype == BF and hb.is_cl(gz) and tuple(S.shape) == (shape[0], 3, shape[1])
    assert torch.equal(gz, gz2) and torch.equal(S, S2), "second call differs"
    assert torch.equal(gz, gz4), "gz differs between the 8- and the 4-channel lanes"
    check(worst(gz, want.gz, EW_TOL * want.gz.abs()), "gz")
    for k in range(3):
        check(worst(S[:, k], want.S[:, k], SUM_TOL * want.abs_S[:, k]), "S%d" % k)
        check(worst(S4[:, k], want.S[:, k], SUM_TOL * want.abs_S[:, k]), "S%d, 4-channel lanes" % k)
    assert torch.equal(S, S4), "sums differ between the 8- and the 4-channel lanes"
    if run_nat is not None:  # the same values in the same order: the natural plane changes addresses only
        (gzn, Sn), _, (gzn4, Sn4) = both_lanes(monkeypatch, run_nat)
        assert torch.equal(gzn, gz) and torch.equal(Sn, S), "natural and transposed plane differ"
        assert torch.equal(gzn4, gz4) and torch.equal(Sn4, S4), "natural and transposed plane differ (4-channel lanes)"


@pytest.mark.parametrize("want_gx", [True, False], ids=["gx", "no-gx"])
@pytest.mark.parametrize("shape", GLUE_SHAPES, ids=GLUE_IDS)
def test_scale_reduce_lanes(shape, want_gx, monkeypatch):
    a = glue_inputs(shape)
    dv = a["dev"]
    want = D.scale_reduce(a["x"], a["t"], a["d"])
    run = lambda: hb.scale_reduce(dv["x"], dv["t"], dv["d"], want_gx=want_gx)
    (gx, s), (gx2, s2), (gx4, s4) = both_lanes(monkeypatch, run)
    assert torch.equal(s, s2), "second call differs (sum)"
    if want_gx:
        assert gx.dtype == BF and hb.is_cl(gx) and torch.equal(gx, gx2), "second call differs (gx)"
        assert torch.equal(gx, gx4), "gx differs between the 8- and the 4-channel lanes"
        check(worst(gx, want.gx, EW_TOL * want.gx.abs()), "gx")
    else:
        assert gx is None
    check(worst(s, want.sum_hw, SUM_TOL * want.abs_hw), "sum x*t")
    check(worst(s4, want.sum_hw, SUM_TOL * want.abs_hw), "sum x*t, 4-channel lanes")
    assert torch.equal(s, s4), "sums differ between the 8- and the 4-channel lanes"


def test_natural_plane_entry_point_refuses_a_missing_plane():
    """stylex_modconv_bwd_prep_nat without a plane is an error before any launch (the outputs stay NaN)."""
    a = glue_inputs((2, 8, 3, 5))
    dv = a["dev"]
    B, C, H, W = 2, 8, 3, 5
    lib = hb._ensure_device(dv["dy"])
    partial = torch.full((B, 1, 3, C), float("nan"), device=DEV)
    gz = torch.full((B, C, H, W), float("nan"), device=DEV, dtype=BF).contiguous(memory_format=torch.channels_last)
    rc = lib.stylex_modconv_bwd_prep_nat(hb._ptr(dv["dy"]), hb._ptr(dv["y"]), None, 0, None, None, None, hb._ptr(gz),
                                         hb._ptr(partial), hb._shape(B, H, W, C), 1, 1, hb._adt(dv["dy"]), hb._stream())
    assert rc == -1  # STYLEX_EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(partial).all() and torch.isnan(gz).all()


def _kernels_of(fn):
    """Names of the GPU kernels fn() launches."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    assert names, "the profiler recorded no GPU kernel"
    return " ".join(names)


def test_default_settings_launch_the_strip_and_wide_kernels(monkeypatch):
    up = up_inputs((2, 40, 17, 16))
    small = up_inputs((2, 8, 2, 2))
    a, odd = glue_inputs((3, 24, 7, 9))["dev"], glue_inputs((2, 12, 3, 5))["dev"]
    prep = lambda v, **kw: hb.modconv_bwd_prep(v["dy"], v["y"], v["nat"], v["nw"], v["nb"], True, gz_scale=v["d"], noise_natural=True)
    scale = lambda v: hb.scale_reduce(v["x"], v["t"], v["d"])
    assert "upsample2x_fwd_strip_kernel" in _kernels_of(lambda: hb.upsample2x_fwd(up["xd"]))
    assert "upsample2x_bwd_strip_kernel" in _kernels_of(lambda: hb.upsample2x_bwd(up["dyd"]))
    assert "strip" not in _kernels_of(lambda: hb.upsample2x_fwd(small["xd"]))  # H < 8: less than one strip
    assert "modconv_bwd_prep_wide_kernel" in _kernels_of(lambda: prep(a))
    assert "scale_reduce_wide_kernel" in _kernels_of(lambda: scale(a))
    assert "wide" not in _kernels_of(lambda: prep(odd)) and "wide" not in _kernels_of(lambda: scale(odd))  # C = 12
    monkeypatch.setenv("STYLEX_UPSAMPLE_STRIP", "0")
    monkeypatch.setenv("STYLEX_GLUE_WIDE", "0")
    assert "strip" not in _kernels_of(lambda: hb.upsample2x_fwd(up["xd"]))
    assert "strip" not in _kernels_of(lambda: hb.upsample2x_bwd(up["dyd"]))
    assert "wide" not in _kernels_of(lambda: prep(a)) and "wide" not in _kernels_of(lambda: scale(a))
