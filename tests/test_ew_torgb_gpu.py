"""-m gpu: the streaming kernels of csrc/elementwise.hip (3x3 reflect blur and its adjoint in every form, the fused RGB tail,
bias (+ noise) + LeakyReLU and its gradient, rowwise_sumsq) and of csrc/torgb.hip (to-RGB forward, input gradient and the
pixel reduction T) against their float64 definitions (tests/_ew_defs.py), element by element.
Run this file before any change to elementwise.hip or torgb.hip.

The hb wrappers are called directly on seeded inputs (keyed by zlib.crc32 of the case), rounded to the activation dtype first;
the reference is computed from the rounded values; a second call must be bit-identical.  Every case runs in two input classes.

EXACT class.  Integer operands in [-4, 4] (gates and saved outputs from {-2, -1, -0.0, +0.0, 1, 2}, noise planes from
{0, 0.5, 1}).  The coefficients are dyadic (k/16 for the blur, k/256 for the RGB tail; to-RGB and T are plain products and
sums), so every fp32 intermediate is exact in any order, with or without FMA contraction, as long as the sums stay below
2^24 (asserted from abs_terms before the comparison).  Then an fp32 result must EQUAL float32(definition) and a bf16 result
bfloat16(float32(definition)).  The one inexact operation is the product with the fp32 constant 0.2f on the negative branch
of a LeakyReLU (bias_act fwd / bwd, the gated blur adjoints): the definitions use double(0.2f), t is exact and short, so the
double product is exact and float32(definition) is the kernel's single rounding — the same two asserts cover it.

GAUSS class.  randn operands, per element  |got - want| <= EW[prec] * |want| + N * 2^-24 * abs_terms,  EW = 2^-22 (fp32) /
2^-8 (bf16: one round-to-nearest-even store, as tests/test_bwd_glue_gpu.py); where the limit is 0 the result must be 0.
N = fp32 roundings on the longest path of a term through the kernel, read from the code (not tuned):
  direct blur (blur3x3_fwd/bwd_kernel)      9   nine fmas onto one accumulator, coefficients exact
  strip blur (blur3x3_strip_kernel)         6   three fmas per filtered row + three down the window
  gated adjoints                           +1   the product with the slope
  RGB tail forward                         10   rgb + prev, then nine fmas
  RGB tail adjoint                         36   6 x 6 fmas
  bias_act forward                          4   x + bias, fma(noise, nw, nb), their sum, 0.2f * t
  bias_act backward                         1   0.2f * dy
  to-RGB forward            2 (8 + log2(C/8))   W * s1, the product with x, 8 additions in the lane, log2(C/8) shuffle adds,
                                                 counted without contraction (every product and every addition rounds)
  to-RGB gx                                 5   W * s1, g * m and two additions: 4 on the path of a term, 5 bounds it
  T, rowwise_sumsq           335 (TOL32 = 2e-5)  the chain is computed per shape and asserted to be shorter: T adds 2 roundings
                                                 per pixel of a lane (ceil(px_per_block / (2048 / C)) <= 9 pixels), log2(512 / C)
                                                 shuffle adds, 3 LDS adds and the chunks (t_chain: at most 56 here); rowwise_sumsq
                                                 <= 16 fmas + 6 shuffle adds + 16 LDS adds (sumsq_chain)
A dropped tap moves an element by >= |x| / 16 and a dropped pixel a sum by abs_terms / HW: far above these limits.

Not reachable by a test that takes seconds, and so not chased: the strip kernels' grid-stride loop wraps only above 2^28
elements, and the 64-bit branch of decomp_index needs a flat index of 2^31.  The direct kernels' loop (grid_for: 2048 blocks
of 256 lanes) does wrap, at the two grid-wrap shapes below.

With STYLEX_EW_RECORD=<file> every case leaves one line in that file: its worst error / limit
(profiles/ew_torgb_errors.txt is the record of one run)."""
import math
import os
import re
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import _ew_defs as D  # noqa: E402
import hip_backend as hb  # noqa: E402
import ops  # noqa: E402
from test_stream_kernels_gpu import _kernels_of  # noqa: E402

DEV = "cuda:0"
F64 = torch.float64
TOL32 = 2e-5  # = 335 * 2^-24
U = 2.0 ** -24
EW = {"fp32": 2.0 ** -22, "bf16": 2.0 ** -8}
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
CLASSES = ("exact", "gauss")
SLOPE = 0.2  # the wrappers' default; reaches the kernel as 0.2f = D.SLOPE


@pytest.fixture(autouse=True)
def hip_impl():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    prev = ops.use_impl(ops.HipOps)
    ops.set_precision("fp32")
    hb.load_library()  # fails loudly if the extension is missing
    yield
    ops.set_precision("fp32")
    ops.use_impl(prev)


# ---- bookkeeping: worst error / limit per test case ---------------------------------------------------------------------
_LINES = []


class Recorder:
    def __init__(self):
        self.worst, self.what, self.exact, self.each = 0.0, "", 0, []

    def ratio(self, r, what):
        """Record err / limit of one quantity, then assert it."""
        r = float(r)
        self.each.append("%s %.4f" % (what, r))
        if not r <= self.worst:  # also true for NaN
            self.worst, self.what = r, what
        assert r <= 1.0, "%s: error / limit = %.4g" % (what, r)

    def equal(self):
        self.exact += 1


@pytest.fixture
def rec(request):
    r = Recorder()
    yield r
    name = request.node.nodeid.split("::", 1)[-1]
    tail = "  [%d exact comparisons]" % r.exact if r.exact else "".join("  [%s]" % e for e in r.each if len(r.each) > 1)
    _LINES.append("%-86s %8.4f  %s%s" % (name, r.worst, r.what or "-", tail))


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    out = os.environ.get("STYLEX_EW_RECORD")
    if out and _LINES:
        with open(out, "w") as f:
            f.write("# tests/test_ew_torgb_gpu.py: per test case, the worst observed error / limit (<= 1 passes) of its Gauss-class\n"
                    "# quantities and the quantity that gave it, then [every quantity]; exact-class cases assert equality with the rounded float64\n"
                    "# definition and report the number of such comparisons.  Limit per element:\n"
                    "# EW * |want| + N * 2^-24 * abs_terms, EW = 2^-22 (fp32) / 2^-8 (bf16), N per kernel as in the file's docstring;\n"
                    "# T and rowwise_sumsq: 2e-5 * abs_terms.\n"
                    "# Ratios above 0.5 are all bf16 outputs and all the same thing: the one round-to-nearest-even store.  Half a\n"
                    "# bf16 spacing is 2^-8 of the power of two below the value, so a value just above a power of two that lands\n"
                    "# near a tie reaches 2^-8 / (1 + 2^-8) = 0.9961 of EW * |want| legitimately; the fp32 part of the error is\n"
                    "# the 0.05 - 0.25 of the fp32 rows.  bias_act_bwd in bf16 stops at 0.7901: the worst of\n"
                    "# 0.2f * dy over the 128 mantissas a bf16 dy can have.\n")
            f.write("\n".join(_LINES) + "\n")


def _worst(got, want, lim):
    """max |got - want| / lim; where lim == 0 (want == 0 and no terms) the result must be exactly zero."""
    got, want, lim = got.detach().double().cpu(), want.detach().double().cpu(), lim.detach().double().cpu()
    assert got.shape == want.shape == lim.shape, (got.shape, want.shape, lim.shape)
    err = (got - want).abs()
    if not torch.isfinite(got).all() or (err[lim == 0] != 0).any():
        return float("inf")
    nz = lim > 0
    return (err[nz] / lim[nz]).max().item() if nz.any() else 0.0


def first_diff(got, want):
    d = (got != want).nonzero()
    i = tuple(d[0].tolist())
    return "%d elements differ, first at %s: got %r, want %r" % (d.shape[0], i, got[i].item(), want[i].item())


def check(rec, cls, prec, got, want, abs_terms, n, what, out_prec=None):
    """The contract of one output.  exact: equality with the rounded definition (sums below 2^24, so fp32 is exact).
    gauss: per element EW * |want| + n * 2^-24 * abs_terms, or TOL32 * abs_terms for n = "sum" (T, rowwise_sumsq).
    out_prec: the output's dtype when it is not the activations'."""
    out_prec = out_prec or prec
    got = got.detach().cpu()
    assert got.dtype == DT[out_prec] and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.shape)
    if cls == "exact":
        assert float(abs_terms.max()) < 2 ** 24, "%s: a sum of the exact class reaches 2^24" % what
        expect = want.float() if out_prec == "fp32" else want.float().bfloat16()
        assert torch.equal(got, expect), "%s (exact class): %s" % (what, first_diff(got, expect))
        rec.equal()
    else:
        lim = TOL32 * abs_terms if n == "sum" else EW[out_prec] * want.abs() + n * U * abs_terms
        rec.ratio(_worst(got, want, lim), what)


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def dev_cl(t):
    t = t.to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def draw(g, shape, cls, prec, lim=4):
    """An operand: integers in [-lim, lim] (exact class) or randn, rounded to the activation dtype."""
    if cls == "exact":
        return torch.randint(-lim, lim + 1, tuple(shape), generator=g).float().to(DT[prec])
    return torch.randn(*shape, generator=g).to(DT[prec])


def draw_gate(g, shape, cls, prec):
    """A gate / saved output: exact class from {-2, -1, -0.0, +0.0, 1, 2}; gauss class randn with about 1 % of +0.0 / -0.0.
    The first and the last element are zeros of either sign in both."""
    if cls == "exact":
        t = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0])[torch.randint(0, 6, tuple(shape), generator=g)]
    else:
        t = torch.randn(*shape, generator=g)
        u = torch.rand(t.numel(), generator=g).view(t.shape)
        t[u < 0.005] = 0.0
        t[(u >= 0.005) & (u < 0.01)] = -0.0
    t = t.to(DT[prec]).contiguous()
    f = t.view(-1)
    f[0], f[f.numel() - 1] = 0.0, -0.0
    return t


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), "second call differs"
    return a


def sid(shape):
    return "x".join(map(str, shape))


# ---- blur ----------------------------------------------------------------------------------------------------------------
# The launcher's conditions (LAUNCH_EW, blur_strip_ok): bf16, C % 8 == 0 and H >= 8 take blur3x3_strip_kernel; otherwise the
# direct blur3x3_fwd / bwd_kernel in lanes of <8> (bf16, C % 8 == 0), <4> (C % 4 == 0) or <1> channels.  All pointers here are
# fresh allocations (16-byte aligned); the misaligned fallback is the unaligned table further down.
BLUR_TABLE = [
    # shape, precision, kernel, lane
    ((1, 4, 2, 2), "fp32", "direct", 4),     # the smallest: every tap of every pixel is a border tap, one vector
    ((2, 8, 4, 4), "fp32", "direct", 4),     # two vectors per pixel, even: s2d forms
    ((2, 12, 9, 7), "fp32", "direct", 4),    # odd sizes, 3 vectors, 378 lanes = two blocks
    ((2, 3, 5, 7), "fp32", "direct", 1),     # C % 4 != 0
    ((1, 6, 2, 3), "fp32", "direct", 1),     # H = 2: both row reflects land on the other row
    ((2, 8, 4, 4), "bf16", "direct", 8),     # the 4 px layers: H < 8 keeps bf16 off the strip kernel
    ((1, 16, 2, 2), "bf16", "direct", 8),    # 2 x 2, two vectors
    ((2, 512, 4, 4), "bf16", "direct", 8),   # the real 4 px width: 2048 lanes = 8 blocks
    ((1, 8, 6, 4), "bf16", "direct", 8),     # H = 6 < 8, non-square
    ((2, 12, 6, 10), "bf16", "direct", 4),   # bf16, C % 8 != 0
    ((2, 3, 8, 8), "bf16", "direct", 1),     # bf16, C % 4 != 0 (H >= 8, but no whole vectors: no strips)
    ((1, 8, 8, 2), "bf16", "strip", 8),      # W = 2: both borders are neighbours; exactly one strip
    ((1, 16, 9, 3), "bf16", "strip", 8),     # a ragged second strip of one row
    ((2, 24, 17, 5), "bf16", "strip", 8),    # two strips and a ragged third, 3 vectors
    ((2, 8, 16, 6), "bf16", "strip", 8),     # two whole strips, even: s2d, gate and mask forms
    ((1, 40, 10, 12), "bf16", "strip", 8),   # 5 vectors, even, a ragged strip of two rows: s2d, gate and mask forms
]
BLUR_IDS = ["%s-%s-%s%d" % (sid(s), p, k, v) for s, p, k, v in BLUR_TABLE]


def blur_n(kernel):
    return 6 if kernel == "strip" else 9


def gate_mask(gate_cpu):
    """The bit mask conv2d_fwd(want_mask=True) writes: bit e of byte (pixel * C + c) / 8 is set when gate[c + e] > 0 (NHWC)."""
    bits = (gate_cpu.permute(0, 2, 3, 1).reshape(-1, 8) > 0).to(torch.int32)
    return (bits * (2 ** torch.arange(8, dtype=torch.int32))).sum(dim=1).to(torch.uint8)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape,prec,kernel,lane", BLUR_TABLE, ids=BLUR_IDS)
def test_blur_forms(shape, prec, kernel, lane, cls, rec):
    B, C, H, W = shape
    g = gen("blur", shape, prec, cls)
    x, dy, gt = draw(g, shape, cls, prec), draw(g, shape, cls, prec), draw_gate(g, shape, cls, prec)
    xd, dyd, gtd = dev_cl(x), dev_cl(dy), dev_cl(gt)
    n = blur_n(kernel)
    fwd, adj = D.blur(x), D.blur_adj(dy)
    y = twice(lambda: hb.blur3x3_fwd(xd))
    assert hb.is_cl(y)
    check(rec, cls, prec, y, fwd.value, fwd.abs_terms, n, "blur3x3_fwd")
    dx = twice(lambda: hb.blur3x3_bwd(dyd))
    assert hb.is_cl(dx)
    check(rec, cls, prec, dx, adj.value, adj.abs_terms, n, "blur3x3_bwd")
    gated = D.gate(adj.value, gt, D.SLOPE)
    dxg = twice(lambda: hb.blur3x3_bwd_gate(dyd, gtd, SLOPE))
    check(rec, cls, prec, dxg, gated, adj.abs_terms, n + 1, "blur3x3_bwd_gate")
    if H % 2 or W % 2:
        return
    y2 = twice(lambda: hb.blur3x3_s2d_fwd(xd))
    assert tuple(y2.shape) == (B, 4 * C, H // 2, W // 2) and hb.is_cl(y2)
    check(rec, cls, prec, y2, D.to_s2d(fwd.value), D.to_s2d(fwd.abs_terms), n, "blur3x3_s2d_fwd")
    dy2 = dev_cl(D.to_s2d(dy))
    dx2 = twice(lambda: hb.blur3x3_s2d_bwd(dy2))
    check(rec, cls, prec, dx2, adj.value, adj.abs_terms, n, "blur3x3_s2d_bwd")
    dx2g = twice(lambda: hb.blur3x3_s2d_bwd(dy2, gate=gtd, slope=SLOPE))
    check(rec, cls, prec, dx2g, gated, adj.abs_terms, n + 1, "blur3x3_s2d_bwd(gate)")
    assert hb.blur_mask_ok(shape, DT[prec]) == (kernel == "strip")
    if hb.blur_mask_ok(shape, DT[prec]):
        mask = gate_mask(gt).to(DEV)
        dx2m = twice(lambda: hb.blur3x3_s2d_bwd(dy2, gate_mask=mask, slope=SLOPE))
        check(rec, cls, prec, dx2m, gated, adj.abs_terms, n + 1, "blur3x3_s2d_bwd(gate_mask)")
        assert torch.equal(dx2m, dx2g), "mask and gate forms differ"


@pytest.mark.parametrize("shape,prec,kernel,lane", BLUR_TABLE, ids=BLUR_IDS)
def test_blur_one_hot_probes_at_the_corners(shape, prec, kernel, lane):
    """A single 1 at each corner of (B, C, H, W): forward and adjoint must be the definition's column / row of k/16 exactly
    (each is a bf16 number), and zero everywhere else — a tap that reads or writes across a sample, channel or border shows."""
    B, C, H, W = shape
    for idx in ((0, 0, 0, 0), (0, C - 1, 0, W - 1), (B - 1, 0, H - 1, 0), (B - 1, C - 1, H - 1, W - 1)):
        t = torch.zeros(shape, dtype=DT[prec])
        t[idx] = 1.0
        td = dev_cl(t)
        for name, fn, ref in (("fwd", hb.blur3x3_fwd, D.blur), ("bwd", hb.blur3x3_bwd, D.blur_adj)):
            got, want = fn(td).cpu().double(), ref(t).value
            assert torch.equal(got, want), "one-hot at %s, %s: %s" % (idx, name, first_diff(got, want))


def lane_of(names, kernel):
    """The template argument V of `kernel<V>` in the profiler's kernel names."""
    m = re.search(re.escape(kernel) + r"<(\d+)>", names)
    assert m, "the profiler printed no template argument for %s: the lane cannot be checked (%s)" % (kernel, names)
    return int(m.group(1))


LANE_ROWS = {}
for _row in BLUR_TABLE:
    LANE_ROWS.setdefault((_row[1], _row[2], _row[3]), _row)  # the first row of every (precision, kernel, lane)


@pytest.mark.parametrize("row", list(LANE_ROWS.values()), ids=["%s-%s%d" % k for k in LANE_ROWS])
def test_blur_rows_launch_the_kernel_they_are_named_for(row):
    """Strip against direct from the kernel's name, and the <8> / <4> / <1> lane from its template argument.  The profiler
    prints template arguments ("blur3x3_fwd_kernel<4>(void const*, ...)"); should a later one stop, lane_of fails here and
    says so: the lane check must not turn into strip-against-direct without a trace."""
    shape, prec, kernel, lane = row
    t = dev_cl(torch.ones(shape, dtype=DT[prec]))
    for fn, direct in ((hb.blur3x3_fwd, "blur3x3_fwd_kernel"), (hb.blur3x3_bwd, "blur3x3_bwd_kernel")):
        names = _kernels_of(lambda: fn(t))
        if kernel == "strip":
            assert "blur3x3_strip_kernel" in names and direct not in names, names
        else:
            assert direct in names and "blur3x3_strip_kernel" not in names, names
            assert lane_of(names, direct) == lane, names


# ---- grid wrap: the direct kernels' grid-stride loop (grid_for caps the grid at 2048 x 256 lanes) ---------------------------
WRAP = [((2, 64, 128, 132), 4),   # fp32 <4>: 540,672 lanes > 524,288
        ((1, 3, 420, 420), 1)]    # fp32 <1>: 529,200 lanes


@pytest.mark.parametrize("shape,lane", WRAP, ids=[sid(s) for s, _ in WRAP])
def test_grid_stride_loops_wrap(shape, lane, rec):
    B, C, H, W = shape
    assert B * C * H * W // lane > 2048 * 256
    g = gen("wrap", shape)
    x = draw(g, shape, "exact", "fp32")
    xd = dev_cl(x)
    fwd, adj = D.blur(x), D.blur_adj(x)
    check(rec, "exact", "fp32", hb.blur3x3_fwd(xd), fwd.value, fwd.abs_terms, 9, "blur3x3_fwd")
    check(rec, "exact", "fp32", hb.blur3x3_bwd(xd), adj.value, adj.abs_terms, 9, "blur3x3_bwd")
    ns = max(H, W)
    bias, nw, nb = (torch.randint(-4, 5, (C,), generator=g).float() for _ in range(3))
    noise = torch.randint(0, 3, (B, ns, ns), generator=g).float() / 2
    want = D.bias_act(x, bias, noise, nw, nb)
    y = hb.bias_act_fwd(xd, bias.to(DEV), noise.to(DEV), nw.to(DEV), nb.to(DEV))
    check(rec, "exact", "fp32", y, want.value, want.abs_terms, 4, "bias_act_fwd")


# ---- RGB tail ------------------------------------------------------------------------------------------------------------
TAIL_SHAPES = [
    (1, 8, 1, 1),    # one input pixel: every clamp and reflect at once; the adjoint's <8> lane in bf16 (the forward has none)
    (3, 4, 4, 4),    # the network's 4-channel RGB storage
    (2, 3, 5, 7),    # C = 3: the scalar lane, odd sizes
    (2, 4, 8, 16),   # 2048 output pixels, two blocks
    (1, 4, 2, 1),    # one column: both clamps and both reflects on one pixel
]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("with_prev", [True, False], ids=["prev", "no-prev"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=[sid(s) for s in TAIL_SHAPES])
def test_rgb_tail(shape, prec, with_prev, cls, rec):
    B, C, H, W = shape
    g = gen("tail", shape, prec, cls)
    rgb, prev, dy = draw(g, shape, cls, prec), draw(g, shape, cls, prec), draw(g, (B, C, 2 * H, 2 * W), cls, prec)
    rd, pd, dyd = dev_cl(rgb), dev_cl(prev) if with_prev else None, dev_cl(dy)
    want = D.rgb_tail(rgb, prev if with_prev else None)
    y = twice(lambda: hb.rgb_up_blur_add_fwd(rd, pd))
    assert hb.is_cl(y)
    check(rec, cls, prec, y, want.value, want.abs_terms, 10, "rgb_up_blur_add_fwd")
    if with_prev:  # the adjoint does not depend on prev: once per shape
        adj = D.rgb_tail_adj(dy)
        dx = twice(lambda: hb.rgb_up_blur_add_bwd(dyd))
        assert hb.is_cl(dx)
        check(rec, cls, prec, dx, adj.value, adj.abs_terms, 36, "rgb_up_blur_add_bwd")


# ---- bias (+ noise) + LeakyReLU -----------------------------------------------------------------------------------------------
# The lanes named here are the FORWARD's (LAUNCH_EW: <8> for bf16 with C % 8 == 0, <4> for C % 4 == 0, else <1>).
BIAS_ACT = [
    ((1, 4, 2, 2), "fp32"), ((1, 4, 2, 2), "bf16"),      # one vector per pixel; bf16: the <4> lane
    ((2, 12, 5, 7), "fp32"), ((2, 12, 5, 7), "bf16"),    # non-square (a transposed read shows), 3 vectors, <4>
    ((2, 3, 5, 7), "fp32"), ((2, 3, 5, 7), "bf16"),      # the scalar lane
    ((2, 8, 4, 4), "bf16"),                              # bf16 <8>
    ((2, 12, 8, 8), "bf16"),                             # bf16 <4> on a square plane
]
# The backward is flat over n = B * C * H * W elements and has no <8> lane: <4> when n % 4 == 0 (and dy, y, dx are 16-byte
# aligned), else <1>.  Of the rows above only (2, 3, 5, 7) has n % 4 != 0 (210): <1>; all others, bf16 included, take <4>.
# (1, 3, 3, 3) is a second <1> row, of 27 elements: fewer than one block, an odd count.
BIAS_ACT_BWD = BIAS_ACT + [((1, 3, 3, 3), "fp32"), ((1, 3, 3, 3), "bf16")]
FORMS = {"bias": (True, None), "noise": (False, 0), "bias+noise-ns=max": (True, 0), "bias+noise-ns=max+3": (True, 3)}


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape,prec", BIAS_ACT, ids=["%s-%s" % (sid(s), p) for s, p in BIAS_ACT])
def test_bias_act_fwd(shape, prec, form, cls, rec):
    B, C, H, W = shape
    with_bias, extra = FORMS[form]
    g = gen("bias_act", shape, prec, cls, form)
    x = draw(g, shape, cls, prec)
    bias = draw(g, (C,), cls, "fp32") if with_bias else None
    noise = nw = nb = None
    if extra is not None:
        ns = max(H, W) + extra
        noise = torch.randint(0, 3, (B, ns, ns), generator=g).float() / 2 if cls == "exact" else torch.rand(B, ns, ns, generator=g)
        nw, nb = draw(g, (C,), cls, "fp32"), draw(g, (C,), cls, "fp32")
    to = lambda t: None if t is None else t.to(DEV)
    xd = dev_cl(x)
    want = D.bias_act(x, bias, noise, nw, nb)
    y = twice(lambda: hb.bias_act_fwd(xd, to(bias), to(noise), to(nw), to(nb)))
    assert hb.is_cl(y)
    check(rec, cls, prec, y, want.value, want.abs_terms, 4, "bias_act_fwd")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape,prec", BIAS_ACT_BWD, ids=["%s-%s" % (sid(s), p) for s, p in BIAS_ACT_BWD])
def test_bias_act_bwd(shape, prec, cls, rec):
    g = gen("bias_act_bwd", shape, prec, cls)
    dy, y = draw(g, shape, cls, prec), draw_gate(g, shape, cls, prec)
    dyd, yd = dev_cl(dy), dev_cl(y)
    want = D.bias_act_bwd(dy, y)
    dx = twice(lambda: hb.bias_act_bwd(dyd, yd))
    assert hb.is_cl(dx)
    check(rec, cls, prec, dx, want, want.abs(), 1, "bias_act_bwd")


# ---- the fallback for pointers that are not 16-byte aligned ------------------------------------------------------------------
# LAUNCH_EW / vec_ok test the two activation pointers it is given (input and output), stylex_rgb_up_blur_add_fwd also prev,
# stylex_bias_act_bwd all three; bias, noise and the mask are not tested and stay aligned.  A channels-last view one element
# into a larger buffer is 2 (bf16) or 4 (fp32) bytes off: the <1> lanes.  The wrappers' `out=` lets the OUTPUT be such a
# view too; the buffer's elements around the view must stay untouched.
UNALIGNED_SHAPE = (2, 8, 4, 6)


def off_view(shape, dtype, fill=None):
    """A channels-last [B, C, H, W] view at a storage offset of one element into a buffer 8 elements larger (NaN around it)."""
    B, C, H, W = shape
    n = B * C * H * W
    buf = torch.full((n + 8,), float("nan"), dtype=dtype, device=DEV)
    v = buf[1:1 + n].view(B, H, W, C).permute(0, 3, 1, 2)
    if fill is not None:
        v.copy_(fill)
    assert hb.is_cl(v) and v.data_ptr() % 16 == v.element_size()
    return buf, v


UNALIGNED_OPS = ["blur3x3_fwd", "blur3x3_bwd", "rgb_up_blur_add_fwd", "rgb_up_blur_add_bwd", "bias_act_fwd", "bias_act_bwd"]


@pytest.mark.parametrize("where", ["in", "out", "both"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("op", UNALIGNED_OPS)
def test_unaligned_pointers_take_the_scalar_lanes(op, prec, where, rec):
    """Exact class at (2, 8, 4, 6): the result must equal the aligned call's bit for bit, and the definition's."""
    shape = UNALIGNED_SHAPE
    B, C, H, W = shape
    dt = DT[prec]
    g = gen("unaligned", op, prec)
    up = (B, C, 2 * H, 2 * W)
    a, b = draw(g, shape, "exact", prec), draw(g, shape, "exact", prec)
    if op == "blur3x3_fwd":
        ins, out_shape, want, call = [a], shape, D.blur(a), lambda i, o: hb.blur3x3_fwd(*i, out=o)
    elif op == "blur3x3_bwd":
        ins, out_shape, want, call = [a], shape, D.blur_adj(a), lambda i, o: hb.blur3x3_bwd(*i, out=o)
    elif op == "rgb_up_blur_add_fwd":
        ins, out_shape, want, call = [a, b], up, D.rgb_tail(a, b), lambda i, o: hb.rgb_up_blur_add_fwd(*i, out=o)
    elif op == "rgb_up_blur_add_bwd":
        big = draw(g, up, "exact", prec)
        ins, out_shape, want, call = [big], shape, D.rgb_tail_adj(big), lambda i, o: hb.rgb_up_blur_add_bwd(*i, out=o)
    elif op == "bias_act_fwd":
        ns = max(H, W) + 3
        bias, nw, nb = (torch.randint(-4, 5, (C,), generator=g).float() for _ in range(3))
        noise = torch.randint(0, 3, (B, ns, ns), generator=g).float() / 2
        extra = tuple(t.to(DEV) for t in (bias, noise, nw, nb))
        assert all(t.data_ptr() % 16 == 0 for t in extra)
        ins, out_shape, want, call = [a], shape, D.bias_act(a, bias, noise, nw, nb), lambda i, o: hb.bias_act_fwd(i[0], *extra, out=o)
    else:
        y = draw_gate(g, shape, "exact", prec)
        v = D.bias_act_bwd(a, y)
        ins, out_shape, want, call = [a, y], shape, D.Sum(v, v.abs()), lambda i, o: hb.bias_act_bwd(*i, out=o)
    ref = call([dev_cl(t) for t in ins], None)
    if where in ("in", "both"):
        dins = [off_view(tuple(t.shape), dt, t.to(DEV))[1] for t in ins]
    else:
        dins = [dev_cl(t) for t in ins]
    if where in ("out", "both"):
        buf, out = off_view(out_shape, dt)
    else:
        out = torch.full(out_shape, float("nan"), dtype=dt, device=DEV).contiguous(memory_format=torch.channels_last)
        buf = None
    assert all((t.data_ptr() % 16 != 0) == (where in ("in", "both")) for t in dins)
    assert (out.data_ptr() % 16 != 0) == (where in ("out", "both"))
    assert call(dins, out) is out
    torch.cuda.synchronize()
    assert torch.equal(out, ref), "the scalar lane and the vector lane differ: %s" % first_diff(out.cpu(), ref.cpu())
    check(rec, "exact", prec, out, want.value, want.abs_terms, 0, op)
    if buf is not None:
        n = out.numel()
        assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + n:]).all(), "a write outside the view"


def test_unaligned_pointers_launch_the_scalar_kernels():
    a = draw(gen("unaligned-names"), UNALIGNED_SHAPE, "exact", "bf16")
    _, v = off_view(UNALIGNED_SHAPE, torch.bfloat16, a.to(DEV))
    for fn, name in ((hb.blur3x3_fwd, "blur3x3_fwd_kernel"), (hb.blur3x3_bwd, "blur3x3_bwd_kernel"),
                     (hb.rgb_up_blur_add_bwd, "rgb_up_blur_add_bwd_kernel"), (hb.bias_act_fwd, "bias_act_fwd_kernel")):
        names = _kernels_of(lambda: fn(v))
        assert name in names and lane_of(names, name) == 1, names


# ---- rowwise_sumsq -----------------------------------------------------------------------------------------------------------
ROWS_COLS = [
    (1, 1), (3, 3),   # scalar lane, fewer columns than threads
    (5, 4),           # vector lane, one float4: 1023 idle threads
    (2, 1023),        # scalar, one short of the block
    (4, 4096),        # vector, one float4 per thread
    (3, 4100),        # vector, a ragged second pass of one float4
    (5, 12291),       # scalar, 13 passes, ragged; rows at odd offsets
    (2, 16384),       # vector, four full passes
]


def sumsq_chain(cols):
    per_thread = -(-cols // 4096) * 4 if cols % 4 == 0 else -(-cols // 1024)
    return per_thread + 6 + 16  # fmas of a thread, shuffle adds of a wave, the 16 waves through LDS


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("rows,cols", ROWS_COLS, ids=["%dx%d" % rc for rc in ROWS_COLS])
def test_rowwise_sumsq(rows, cols, cls, rec):
    assert sumsq_chain(cols) < 335
    x = draw(gen("sumsq", rows, cols, cls), (rows, cols), cls, "fp32", lim=3)
    xd = x.to(DEV)
    want = D.rowwise_sumsq(x)
    s = twice(lambda: hb.rowwise_sumsq(xd))
    check(rec, cls, "fp32", s, want.value, want.abs_terms, "sum", "rowwise_sumsq")


# ---- to-RGB ------------------------------------------------------------------------------------------------------------------
TORGB_SHAPES = [
    (2, 8, 16, 16),     # LP = 1: a lane owns a whole pixel, no shuffle in the forward, six in T's reduction
    (3, 16, 5, 7),      # odd pixel count (35 against 128 pixel rows): a ragged, single pass
    (2, 64, 33, 7),     # 231 px against 32 rows: 8 passes, the last ragged
    (1, 128, 64, 64),   # 32 chunks
    (2, 256, 40, 40),   # 25 chunks of 64 px
    (2, 512, 4, 4),     # LP = 64: a pixel is a whole wave, no in-wave reduction of T
    (5, 32, 1, 1),      # one pixel: 255 idle lanes, 63 idle pixel rows
    (1, 128, 9, 15),    # 135 px in 2 chunks: px_per_block = 68 rounds UP, the second chunk is ragged
]
TORGB_IDS = [sid(s) for s in TORGB_SHAPES]
_TORGB = {}


def torgb_geo(shape):
    B, C, H, W = shape
    nch = hb.load_library().stylex_torgb_chunks(hb._shape(B, H, W, C))
    ppb = -(-H * W // nch)
    return nch, ppb


def t_chain(shape):
    """fp32 roundings on the longest path of a term of T: a product and an addition per pixel of the lane, the shuffle adds
    over the lanes of a wave that share a channel group, three LDS additions, and the sum over the chunks."""
    B, C, H, W = shape
    nch, ppb = torgb_geo(shape)
    lp = C // 8
    return 2 * -(-ppb // (256 // lp)) + int(math.log2(64 // lp)) + 3 + (nch - 1)


def torgb_inputs(shape, cls):
    """x, gy (4-channel storage whose channel 3 holds values the kernel must ignore), s1, w and the definitions; shared, never
    written."""
    key = (shape, cls)
    if key not in _TORGB:
        B, C, H, W = shape
        g = gen("torgb", shape, cls)
        x, gy4 = draw(g, shape, cls, "bf16"), draw(g, (B, 4, H, W), cls, "bf16")
        s1, w = draw(g, (B, C), cls, "fp32"), draw(g, (3, C, 1, 1), cls, "fp32")
        r = dict(x=x, gy4=gy4, s1=s1, w=w, xd=dev_cl(x), gyd=dev_cl(gy4), s1d=s1.to(DEV), wd=w.to(DEV))
        r["fwd"], r["bwd"] = D.torgb(x, s1, w), D.torgb_bwd(x, gy4[:, :3], s1, w)
        _TORGB[key] = r
    return _TORGB[key]


def check_t(rec, cls, shape, T, bwd, what):
    assert t_chain(shape) < 335, (shape, t_chain(shape))
    check(rec, cls, "bf16", T, bwd.T, bwd.abs_T, "sum", what, out_prec="fp32")


def test_torgb_geometry_is_the_one_the_shapes_are_named_for():
    geo = {s: torgb_geo(s) for s in TORGB_SHAPES}
    assert geo[(2, 8, 16, 16)] == (1, 256) and geo[(3, 16, 5, 7)] == (1, 35) and geo[(2, 64, 33, 7)] == (1, 231)
    assert geo[(1, 128, 64, 64)] == (32, 128) and geo[(2, 256, 40, 40)] == (25, 64) and geo[(2, 512, 4, 4)] == (1, 16)
    assert geo[(5, 32, 1, 1)] == (1, 1) and geo[(1, 128, 9, 15)] == (2, 68)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", TORGB_SHAPES, ids=TORGB_IDS)
def test_torgb_fwd(shape, cls, rec):
    B, C, H, W = shape
    a = torgb_inputs(shape, cls)
    y = twice(lambda: hb.torgb_fwd(a["xd"], a["s1d"], a["wd"]))
    assert tuple(y.shape) == (B, 4, H, W) and y.dtype == torch.bfloat16 and hb.is_cl(y)
    assert (y[:, 3].contiguous().view(torch.int16) == 0).all(), "channel 3 of the storage is not +0"
    check(rec, cls, "bf16", y[:, :3], a["fwd"].value, a["fwd"].abs_terms, 2 * (8 + int(math.log2(C // 8))), "torgb_fwd")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", TORGB_SHAPES, ids=TORGB_IDS)
def test_torgb_bwd(shape, cls, rec):
    B, C, H, W = shape
    a = torgb_inputs(shape, cls)
    gx, T = twice(lambda: hb.torgb_bwd(a["xd"], a["gyd"], a["s1d"], a["wd"], want_gx=True))
    none, T2 = twice(lambda: hb.torgb_bwd(a["xd"], a["gyd"], a["s1d"], a["wd"], want_gx=False))
    assert none is None and torch.equal(T, T2), "T depends on want_gx"
    assert hb.is_cl(gx) and tuple(T.shape) == (B, 3, C)
    check(rec, cls, "bf16", gx, a["bwd"].gx, a["bwd"].abs_gx, 5, "torgb_bwd gx")
    check_t(rec, cls, shape, T, a["bwd"], "torgb_bwd T")


# Empty trailing chunks.  A block whose range starts at or past HW, (n - 1) * ceil(HW / n) >= HW, gets no pixel and must write
# zeros into its row of `partial`.  Uncapped, stylex_torgb_chunks gives n = ceil(HW / P), P = 8 * (2048 / C) pixels, hence
# P (n - 1) < HW and ceil(HW / n) <= P: no block is empty.  The cap n <= 4096 / B changes that: a lowered n raises
# px_per_block = ceil(HW / n) above P, and its rounding up can leave the last block(s) nothing, e.g. B = 120, C = 512,
# HW = 1089: n = 35 capped to 34, 33 px per block, 33 * 33 = 1089, block 33 is empty; or B = 1, C = 512, HW = 131073:
# n = 4096, 33 px, blocks 3972 .. 4095 are empty.  The cap binds only when B * ceil(HW / P) > 4096, that is from about
# 4096 * P * C = 6.7e7 input elements (134 MB) at any C, so no shape under 64 KB has one and a search there finds nothing.
# The case is run at (120, 512, 33, 33) instead; to keep the float64 reference at one sample (557,568 elements), every
# sample holds the same x and s1, and gy alternates in sign with the sample, so T[b] = +-T[0] and y[b] = y[0].
EMPTY_CHUNK_SHAPE = (120, 512, 33, 33)


def test_torgb_empty_trailing_chunk_writes_zeros(rec):
    B, C, H, W = EMPTY_CHUNK_SHAPE
    HW = H * W
    lib = hb.load_library()
    nch, ppb = torgb_geo(EMPTY_CHUNK_SHAPE)
    empty = [k for k in range(nch) if k * ppb >= HW]
    assert (nch, ppb) == (34, 33) and empty == [33], "the chunk rule changed: pick a shape with an empty trailing chunk again"
    one = (1, C, H, W)
    g = gen("torgb-empty", EMPTY_CHUNK_SHAPE)
    x0, gy0 = draw(g, one, "exact", "bf16"), draw(g, (1, 4, H, W), "exact", "bf16")
    s0, w = draw(g, (1, C), "exact", "fp32"), draw(g, (3, C, 1, 1), "exact", "fp32")
    sgn = 1.0 - 2.0 * (torch.arange(B) % 2).float()  # +1, -1, +1, ...
    cl = torch.channels_last
    xd = dev_cl(x0).expand(B, -1, -1, -1).contiguous(memory_format=cl)
    gyd = (dev_cl(gy0) * sgn.to(DEV).view(B, 1, 1, 1)).to(torch.bfloat16).contiguous(memory_format=cl)
    s1d, wd = s0.to(DEV).expand(B, -1).contiguous(), w.to(DEV)
    assert hb.is_cl(xd) and hb.is_cl(gyd) and tuple(xd.shape) == EMPTY_CHUNK_SHAPE and tuple(gyd.shape) == (B, 4, H, W)
    fwd, bwd = D.torgb(x0, s0, w), D.torgb_bwd(x0, gy0[:, :3], s0, w)
    assert float(fwd.abs_terms.max()) < 2 ** 24 and float(bwd.abs_T.max()) < 2 ** 24
    # the C entry point, so that the rows of `partial` can be looked at: NaN before the launch
    hb._ensure_device(xd)
    partial = torch.full((B, nch, 3, C), float("nan"), device=DEV)
    rc = lib.stylex_torgb_bwd(hb._ptr(xd), hb._ptr(gyd), hb._ptr(s1d), hb._ptr(wd), None, hb._ptr(partial),
                              hb._shape(B, H, W, C), hb._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not torch.isnan(partial).any(), "rows of partial left unwritten"
    assert (partial[:, empty] == 0).all(), "the empty chunk did not write zeros"
    want_T = sgn.view(B, 1, 1) * bwd.T.float()
    T = partial.sum(dim=1).cpu()
    assert torch.equal(T, want_T), "T with an empty trailing chunk: %s" % first_diff(T, want_T)
    rec.equal()
    none, T2 = hb.torgb_bwd(xd, gyd, s1d, wd, want_gx=False)
    assert none is None and torch.equal(T2.cpu(), want_T), "hb.torgb_bwd with an empty trailing chunk"
    rec.equal()
    # the forward splits the pixels the same way: its last block has nothing to write
    y = hb.torgb_fwd(xd, s1d, wd)
    want_y = fwd.value.float().bfloat16().expand(B, -1, -1, -1)
    assert (y[:, 3].contiguous().view(torch.int16) == 0).all() and torch.equal(y[:, :3].cpu(), want_y), "torgb_fwd"
    rec.equal()


FN_ROWS = [(2, 8, 16, 16), (3, 16, 5, 7), (5, 32, 1, 1), (2, 64, 33, 7), (1, 128, 9, 15), (2, 256, 40, 40), (2, 512, 4, 4)]


@pytest.mark.against_definition
@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", FN_ROWS, ids=[sid(s) for s in FN_ROWS])
def test_modulated_conv2d_to_rgb_uses_T_as_defined(shape, cls, rec):
    """ops.modulated_conv2d(x, style, w, demod=False) on the fast path in bf16, one row per channel count: the fused node runs,
    and output, gx, gstyle = sum_n W T and gw = sum_b (style + 1) T meet the definitions per element.  gstyle and gw are fp32
    contractions of T done by the caller: a product and 2 (gstyle) or B - 1 (gw) additions on top of T's chain."""
    B, C, H, W = shape
    g = gen("torgb-fn", shape, cls)
    x, r = draw(g, shape, cls, "bf16"), draw(g, (B, 3, H, W), cls, "bf16")
    style, w = draw(g, (B, C), cls, "fp32"), draw(g, (3, C, 1, 1), cls, "fp32")
    s1 = style + 1  # fp32, one rounding: the same IEEE addition as the device's
    ops.set_precision("bf16")
    prev = ops.set_fast(True)
    try:
        xd, sd, wd = dev_cl(x).requires_grad_(), style.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
        assert hb.torgb_ok(ops._act(xd))
        y = ops.modulated_conv2d(xd, sd, wd, demod=False)
        node = y.grad_fn.next_functions[0][0]
        assert "_ToRGBFast" in type(node).__name__, (y.grad_fn, node)
        (y.float() * dev_cl(r).float()).sum().backward()
    finally:
        ops.set_fast(prev)
        ops.set_precision("fp32")
    fwd, bwd = D.torgb(x, s1, w), D.torgb_bwd(x, r, s1, w)
    ds, dw = D.torgb_dstyle(bwd.T, w, bwd.abs_T), D.torgb_dw(bwd.T, s1, bwd.abs_T)
    assert tuple(y.shape) == (B, 3, H, W)
    nT = TOL32 / U  # T's own bound, as a count of roundings
    assert t_chain(shape) < 335
    check(rec, cls, "bf16", y, fwd.value, fwd.abs_terms, 2 * (8 + int(math.log2(C // 8))), "output")
    check(rec, cls, "bf16", xd.grad, bwd.gx, bwd.abs_gx, 5, "gx")
    check(rec, cls, "bf16", sd.grad, ds.value, ds.abs_terms, nT + 3, "gstyle", out_prec="fp32")
    check(rec, cls, "bf16", wd.grad, dw.value.reshape(3, C, 1, 1), dw.abs_terms.reshape(3, C, 1, 1), nT + B, "gw", out_prec="fp32")
