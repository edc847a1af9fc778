"""-m gpu: the kernels of csrc/frozen_ew.hip (the elementwise tails of the frozen classifier, its input resize, the LPIPS tap in
both layouts, the layout bridges, relu_gate_add, the bf16 max-pool and the image gradient of a stem convolution) against their
float64 definitions (tests/_frozen_defs.py), element by element.  Run this file before any change to frozen_ew.hip.

Method and helpers are those of tests/test_ew_torgb_gpu.py (read its docstring first): the hb wrappers are called directly on
seeded inputs; a second call must be bit-identical; outputs lie between NaN guard bands (the wrappers' `out=`); the
instantiation that ran is read from the profiler's kernel names, template arguments included.  Every case runs in an EXACT
class where one exists and in a GAUSS class.

EXACT class.  Integer operands in [-4, 4], dyadic scales and shifts (k / 4, a negative scale among them), std a power of two,
gates and saved outputs from {-2, -1, -0.0, +0.0, 1, 2}, resize pairs with power-of-two ratios (32 -> 64, 64 -> 32, 8 -> 32)
and the identity: every fp32 intermediate is exact in any order while the sums stay below 2^24 (asserted), so the result must
EQUAL float32(definition) or bfloat16(float32(definition)).  All of conv_image_grad is in this class; the pooling index planes,
the bridges, relu_gate_add and the bf16 max-pool are exact in both classes (a comparison, a copy, one correctly rounded sum).

GAUSS class.  Per element  |got - want| <= EW * |want| + N * 2^-24 * abs_terms,  EW = 2^-22 (fp32) / 2^-8 (bf16); where the
limit is 0 the result must be 0.  N = fp32 roundings on the longest path of a term, read from the code and counted without
contraction (an explicit fmaf is one rounding):
  affine_act fwd          1 + residual   fmaf(x, s, t); + r
  affine_act bwd gx       1              g * s; gres must equal gy or 0 exactly
  pool fwd                1              fmaf(x, s, t), then comparisons
  pool bwd                4              0 + g is exact, three further additions, * s
  resize fwd              6 (+ 2)        l0 = 1 - l1, w * p, +, l0 of the rows, h * r, +   (- mean, / std)
  resize adjoint          kx + ky + 6 (+ 1)   per axis: the weight (1 - l1, and l0 + l1 at the clamped border: 2), the product,
                                         one addition per output that names the pixel (kx, ky: counted from the matrices);  / std
  relu_gate_add           1              a + b in fp32 (the exact and the gauss class both compare bit for bit: the float64 sum
                                         of two bf16 numbers is exact and its float32 rounding is the kernel's)
  maxpool3s2 bwd          3              0 + g exact, three further additions
  LPIPS (SL waves or 8 lanes share a pixel; L = fmas of a lane, X = additions of the cross-wave / octet reduction:
         NCHW  L = ceil(C / SL), X = 2 + SL / 4;  NHWC  L = 8 ceil(C / 64), X = 3)
    sum of squares        Ns = 2 L + X
    norms                 En = Ns / 2 + 1             the square root halves the relative error and rounds once
    distance              2 (En + 4) + 2 + L + X + R  t = x / A - y / B carries En + 4 (+ eps, 1 / ., two products, -), the term
                                                      lin t t twice that + 2; R = 6 shuffle adds + / HW + the sum over the blocks
                                                      (NHWC: 3 + 2 + 1 + blocks), on abs_dist
    gradients             own * (2 En + 11) + cross * (Edot + 3 En + 9),  Edot = En + 6 + L + X:
                          first-order propagation from the saved fp32 norms (En each) through t, lin t, the dot products
                          (abs_dot0 / abs_dot1), k = 2 dot / (A A r) and the element's two terms, own = |gs| 2 lin T / A and
                          cross = |gs| 2 abs_dot / (A^2 r) |f|; bf16 gradients add 2^-8 |want|
resize_norm carries one more term, because its weights are themselves fp32 results: 3 * 2^-24 * (Hi * dy_terms + Wi * dx_terms),
dy_terms / dx_terms the |tap difference| sums of the definition (for the adjoint |gy| through the |derivative| of one axis's
weights and the other axis's weights); the constant 3 and the cell i0 are asserted for every (in, out) pair used here by
tests/test_frozen_defs_cpu.py.  A dropped tap or term moves an element by a whole term: far above these limits.

Grid-stride wrap.  grid_for caps a launch at 16384 blocks of 256 lanes; the five wrap shapes have just over 4,194,304 lanes
and take their reference in float64 on the device.  relu_gate_add's launcher caps its grid the same way: (8, 64, 257, 256).
Not chased: maxpool3s2_nhwc wraps only above 1.3e8 input elements, 32 times the workload.

With STYLEX_FROZEN_RECORD=<file> every case leaves one line in that file: its worst error / limit
(profiles/frozen_ew_errors.txt is the record of one run)."""
import math
import os
import re

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.against_definition]

import _frozen_defs as D  # noqa: E402
import hip_backend as hb  # noqa: E402
from test_ew_torgb_gpu import DEV, DT, EW, U, Recorder, _worst, check, draw, draw_gate, first_diff, gen, hip_impl, sid, twice  # noqa: E402,F401
from test_frozen_defs_cpu import EXACT_PAIRS, GAUSS_PAIRS, LPIPS_SHAPES, POOL_SHAPES, lpips_inputs, pool_inputs  # noqa: E402
from test_stream_kernels_gpu import _kernels_of  # noqa: E402

F64 = torch.float64
CLASSES = ("exact", "gauss")
NAN = float("nan")
G = 64  # elements of guard band on either side of an output
CAP = 16384 * 256  # grid_for: lanes of one pass of the grid-stride loops

_LINES = []


@pytest.fixture
def rec(request):
    r = Recorder()
    yield r
    name = request.node.nodeid.split("::", 1)[-1]
    tail = "  [%d exact comparisons]" % r.exact if r.exact and not r.each else "".join("  [%s]" % e for e in r.each if len(r.each) > 1)
    _LINES.append("%-92s %8.4f  %s%s" % (name, r.worst, r.what or "-", tail))


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    out = os.environ.get("STYLEX_FROZEN_RECORD")
    if out and _LINES:
        with open(out, "w") as f:
            f.write("# tests/test_frozen_ew_gpu.py: per test case, the worst observed error / limit (<= 1 passes) of its Gauss-class\n"
                    "# quantities and the quantity that gave it, then [every quantity]; exact-class cases assert equality with the rounded\n"
                    "# float64 definition and report the number of such comparisons.  Limit per element:\n"
                    "# EW * |want| + N * 2^-24 * abs_terms (+ the coordinate term of resize_norm), EW = 2^-22 (fp32) / 2^-8 (bf16),\n"
                    "# N per kernel as in the file's docstring.\n")
            f.write("\n".join(_LINES) + "\n")


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def guarded(shape, dtype, cl=False, off=0):
    """(buffer, view): a dense output of `shape` (channels_last when cl) `off` elements past the first guard band of a flat
    buffer filled with NaN (bytes: 171)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * G + off,), 171 if dtype == torch.uint8 else NAN, dtype=dtype, device=DEV)
    v = buf[G + off:G + off + n]
    if cl:
        B, C, H, W = shape
        v = v.view(B, H, W, C).permute(0, 3, 1, 2)
        assert hb.is_cl(v)
    else:
        v = v.view(shape)
    return buf, v


def untouched(t):
    return bool((t == 171).all()) if t.dtype == torch.uint8 else bool(torch.isnan(t).all())


def bands_ok(buf, v):
    a, n = v.storage_offset(), v.numel()
    assert untouched(buf[:a]) and untouched(buf[a + n:]), "a write outside the output"


def into(fn, *specs):
    """fn(*outs) on fresh guarded outputs (spec: shape, dtype[, cl[, off]]); the bands are checked after the call."""
    made = [guarded(*s) for s in specs]
    res = fn(*[v for _, v in made])
    torch.cuda.synchronize()
    for buf, v in made:
        bands_ok(buf, v)
    return res


def off4(t):
    """A dense copy of the fp32 tensor t whose pointer is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def targs(names, kernel):
    """The template arguments of `kernel<...>` in the profiler's kernel names."""
    m = re.search(re.escape(kernel) + r"<([\d, ]+)>", names)
    assert m, "the profiler printed no template argument for %s: the instantiation cannot be checked (%s)" % (kernel, names)
    return tuple(int(v) for v in m.group(1).split(","))


def cpu(*ts):
    return tuple(None if t is None else t.detach().cpu() for t in ts)


def affine_params(g, c, cls, dev="cpu"):
    if cls == "exact":
        s, t = torch.randint(-8, 9, (c,), generator=g).float() / 4, torch.randint(-8, 9, (c,), generator=g).float() / 4
        s[0] = -0.75
    else:
        s, t = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
        s[0] = -s[0]
    return s.to(dev), t.to(dev)


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


# ---- affine (+ residual) (+ ReLU) ---------------------------------------------------------------------------------------------
AFFINE = [  # shape, the operand given a 4-byte-offset pointer, lane forward, lane backward
    ((2, 5, 6, 6), None, 4, 4),
    ((3, 5, 7, 7), None, 1, 1),   # HW % 4 != 0
    ((2, 5, 6, 6), "x", 1, 4),
    ((2, 5, 6, 6), "r", 1, 4),
    ((2, 5, 6, 6), "gy", 4, 1),
    ((2, 5, 6, 6), "y", 4, 1),
    ((2, 5, 6, 6), "out", 1, 1),  # the outputs themselves (y forward, gx backward)
    ((1, 1, 1, 1), None, 1, 1),
]
AFFINE_IDS = ["%s-%s" % (sid(s), m or "aligned") for s, m, _, _ in AFFINE]


def affine_case(shape, mis, res, relu, cls, key="affine"):
    B, C, H, W = shape
    g = gen(key, shape, mis, res, relu, cls)
    x, r, gy, y = draw(g, shape, cls, "fp32"), draw(g, shape, cls, "fp32"), draw(g, shape, cls, "fp32"), draw_gate(g, shape, cls, "fp32")
    s, t = affine_params(g, C, cls)
    put = lambda name, v: off4(v.to(DEV)) if mis == name else v.to(DEV)
    d = dict(x=x, r=r if res else None, gy=gy, y=y, s=s, t=t, xd=put("x", x), rd=put("r", r) if res else None, gyd=put("gy", gy),
             yd=put("y", y), sd=s.to(DEV), td=t.to(DEV), off=1 if mis == "out" else 0)
    return d


def affine_calls(d, shape, res, relu):
    o = d["off"]
    fwd = lambda: into(lambda out: hb.affine_act_fwd(d["xd"], d["sd"], d["td"], d["rd"], relu, out=out), (shape, torch.float32, False, o))
    bwd = lambda: into(lambda out, out_res: hb.affine_act_bwd(d["gyd"], d["yd"], d["sd"], relu, want_res=res, out=out, out_res=out_res),
                       (shape, torch.float32, False, o), (shape, torch.float32))
    return fwd, bwd


# the kernel is handed r only with a residual and y only with the ReLU: the offset rows of the two run in those forms alone
AFFINE_FORMS = [(s, m, res, relu) for s, m, _, _ in AFFINE for res in (True, False) for relu in (True, False)
                if not (m == "r" and not res) and not (m == "y" and not relu)]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape,mis,res,relu", AFFINE_FORMS,
                         ids=["%s-%s-%s-%s" % (sid(s), m or "aligned", "res" if r else "no-res", "relu" if a else "linear") for s, m, r, a in AFFINE_FORMS])
def test_affine_act(shape, mis, res, relu, cls, rec):
    d = affine_case(shape, mis, res, relu, cls)
    fwd, bwd = affine_calls(d, shape, res, relu)
    want = D.affine_act(d["x"], d["s"], d["t"], d["r"], relu)
    check(rec, cls, "fp32", twice(fwd), want.value, want.abs_terms, 2 if res else 1, "affine_act_fwd")
    wgx, wgres = D.affine_act_bwd(d["gy"], d["y"], d["s"], relu)
    gx, gres = twice(bwd)
    check(rec, cls, "fp32", gx, wgx.value, wgx.abs_terms, 1, "affine_act_bwd gx")
    assert (gres is None) == (not res)
    if res:
        assert torch.equal(gres.cpu(), wgres.float()), "gres is not gy or 0: %s" % first_diff(gres.cpu(), wgres.float())
        rec.equal()


@pytest.mark.parametrize("shape,mis,lf,lb", AFFINE, ids=AFFINE_IDS)
def test_affine_act_rows_launch_the_lane_they_are_named_for(shape, mis, lf, lb):
    d = affine_case(shape, mis, True, True, "exact")
    fwd, bwd = affine_calls(d, shape, True, True)
    assert targs(_kernels_of(fwd), "affine_act_fwd_kernel") == (lf,)
    assert targs(_kernels_of(bwd), "affine_act_bwd_kernel") == (lb,)


AFFINE_WRAP = [((2, 33, 253, 255), 1), ((4, 66, 256, 252), 4)]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape,lane", AFFINE_WRAP, ids=[sid(s) for s, _ in AFFINE_WRAP])
def test_affine_act_grid_stride_loop_wraps(shape, lane, cls, rec):
    B, C, H, W = shape
    assert B * C * H * W // lane > CAP and (H * W % 4 == 0) == (lane == 4)
    g = torch.Generator(device=DEV).manual_seed(71 + lane)
    mk = (lambda: torch.randint(-4, 5, shape, device=DEV, generator=g).float()) if cls == "exact" else (lambda: torch.randn(shape, device=DEV, generator=g))
    x, r, gy = mk(), mk(), mk()
    s, t = affine_params(gen("affine-wrap", shape, cls), C, cls, DEV)
    want = D.affine_act(x, s, t, r, True)
    fwd = lambda: into(lambda out: hb.affine_act_fwd(x, s, t, r, True, out=out), (shape, torch.float32))
    assert targs(_kernels_of(fwd), "affine_act_fwd_kernel") == (lane,)
    y = fwd()
    check(rec, cls, "fp32", y, *cpu(want.value, want.abs_terms), 2, "affine_act_fwd")
    wgx, wgres = D.affine_act_bwd(gy, y, s, True)
    bwd = lambda: into(lambda out, out_res: hb.affine_act_bwd(gy, y, s, True, want_res=True, out=out, out_res=out_res),
                       (shape, torch.float32), (shape, torch.float32))
    assert targs(_kernels_of(bwd), "affine_act_bwd_kernel") == (lane,)
    gx, gres = bwd()
    check(rec, cls, "fp32", gx, *cpu(wgx.value, wgx.abs_terms), 1, "affine_act_bwd gx")
    assert torch.equal(gres, wgres.float()), "gres"
    rec.equal()


# ---- BatchNorm -> ReLU -> MaxPool2d(3, 2, 1) --------------------------------------------------------------------------------------
POOL_KINDS = ("exact", "gauss", "ties", "negative")


def pool_check(rec, kind, x, s, t, gy, shape):
    """x, s, t, gy on any device; the kernels run on the device copies."""
    B, C, H, W = shape
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    cls = "exact" if kind == "exact" else "gauss"
    xd, sd, td, gyd = x.to(DEV), s.to(DEV), t.to(DEV), gy.to(DEV)
    d = D.affine_relu_maxpool(x, s, t)
    oshape = (B, C, ho, wo)
    y, idx = twice(lambda: into(lambda o, oi: hb.affine_relu_maxpool_fwd(xd, sd, td, True, out=o, out_idx=oi), (oshape, torch.float32),
                                (oshape, torch.uint8)))
    check(rec, cls, "fp32", y, *cpu(d.y, d.abs_terms), 1, "affine_relu_maxpool_fwd")
    assert idx.dtype == torch.uint8
    share = d.near_tie.float().mean().item()
    assert share <= 1e-3 and (cls != "exact" or share == 0), "near ties: %g of the windows" % share
    same = (idx.to(d.idx.device) == d.idx) | d.near_tie
    assert bool(same.all()), "index plane: %d windows differ, first at %s" % (int((~same).sum()), (~same).nonzero()[0].tolist())
    rec.equal()
    y2, none = into(lambda o: hb.affine_relu_maxpool_fwd(xd, sd, td, False, out=o), (oshape, torch.float32))
    assert none is None and torch.equal(y2, y), "want_idx=False changes the values"
    # the scatter, by the DEFINITION's index plane
    bw = D.affine_relu_maxpool_bwd(gy, d.idx, s, (H, W))
    idxd = d.idx.to(DEV).contiguous()
    gx = twice(lambda: into(lambda o: hb.affine_relu_maxpool_bwd(gyd, idxd, sd, (H, W), out=o), (shape, torch.float32)))
    check(rec, cls, "fp32", gx, *cpu(bw.value, bw.abs_terms), 4, "affine_relu_maxpool_bwd")
    return d


@pytest.mark.parametrize("kind", POOL_KINDS)
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=[sid(s) for s in POOL_SHAPES])
def test_affine_relu_maxpool(shape, kind, rec):
    B, C, H, W = shape
    g = gen("pool", shape, kind)
    if kind == "exact":
        x = draw(g, shape, "exact", "fp32")
        s, t = affine_params(g, C, "exact")
    else:
        x, s, t = pool_inputs(shape, kind)  # the inputs whose near-tie share tests/test_frozen_defs_cpu.py asserts
    gy = draw(g, (B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1), "exact" if kind == "exact" else "gauss", "fp32")
    d = pool_check(rec, kind, x, s, t, gy, shape)
    if kind == "negative":
        assert bool((d.idx == 255).all())


POOL_WRAP = (2, 33, 509, 511)


@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_affine_relu_maxpool_grid_stride_loops_wrap(kind, rec):
    B, C, H, W = POOL_WRAP
    ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert B * C * ho * wo == 4308480 > CAP and B * C * H * W > 4 * CAP
    g = torch.Generator(device=DEV).manual_seed(73)
    mk = (lambda sh: torch.randint(-4, 5, sh, device=DEV, generator=g).float()) if kind == "exact" else (lambda sh: torch.randn(sh, device=DEV, generator=g))
    x, gy = mk(POOL_WRAP), mk((B, C, ho, wo))
    s, t = affine_params(gen("pool-wrap", kind), C, kind, DEV)
    pool_check(rec, kind, x, s, t, gy, POOL_WRAP)


# ---- resize + normalise ----------------------------------------------------------------------------------------------------------
RESIZE_GAUSS = [(4, 3, 256, 256, 224, 224, "nchw"), (4, 3, 256, 256, 224, 224, "nhwc"), (2, 3, 32, 32, 224, 224, "nchw"),
                (2, 3, 64, 64, 224, 224, "nhwc"), (2, 4, 40, 56, 33, 97, "nchw"), (1, 3, 224, 224, 224, 224, "nchw"),
                (3, 1, 7, 5, 3, 11, "slice"), (1, 1, 1, 1, 3, 3, "nchw"), (2, 3, 5, 7, 1, 1, "nchw")]
RESIZE_EXACT = [(2, 3, 32, 32, 64, 64, "nchw"), (2, 3, 64, 64, 32, 32, "nhwc"), (1, 4, 8, 8, 32, 32, "slice"), (2, 3, 16, 16, 16, 16, "nchw"),
                (1, 2, 32, 8, 64, 32, "nchw")]
RESIZE_WRAP = (28, 3, 256, 256, 224, 224, "nchw")
for _c in RESIZE_GAUSS + [RESIZE_WRAP]:
    assert (_c[2], _c[4]) in GAUSS_PAIRS and (_c[3], _c[5]) in GAUSS_PAIRS, _c  # the index rule is asserted for these pairs
for _c in RESIZE_EXACT:
    assert (_c[2], _c[4]) in EXACT_PAIRS and (_c[3], _c[5]) in EXACT_PAIRS, _c


def layout_of(x, layout, g):
    """x [B, C, H, W] on the device in the layout named: dense, channels_last, or a channel slice of a wider tensor."""
    if layout == "nhwc":
        return x.contiguous(memory_format=torch.channels_last)
    if layout == "slice":
        B, C, H, W = x.shape
        wide = torch.full((B, C + 2, H, W), NAN, device=DEV)
        wide[:, 1:1 + C] = x
        return wide[:, 1:1 + C]
    return x


def resize_check(rec, case, cls, norm):
    B, C, H, W, Ho, Wo, layout = case
    g = torch.Generator(device=DEV).manual_seed(61 + H * 3 + Wo)
    mk = (lambda sh: torch.randint(-4, 5, sh, device=DEV, generator=g).float()) if cls == "exact" else (lambda sh: torch.randn(sh, device=DEV, generator=g))
    x, gy = mk((B, C, H, W)), mk((B, C, Ho, Wo))
    mean = std = None
    if norm:
        if cls == "exact":
            mean = torch.randint(-4, 5, (C,), device=DEV, generator=g).float()
            std = torch.tensor([0.5, 2.0, 0.25, 4.0], device=DEV)[:C].contiguous()
        else:
            mean, std = torch.randn(C, device=DEV, generator=g), torch.rand(C, device=DEV, generator=g) + 0.5
    xl = layout_of(x, layout, g)
    d = D.resize_norm(x, (Ho, Wo), mean, std)
    n = 8 if norm else 6
    y = twice(lambda: into(lambda o: hb.resize_norm_fwd(xl, (Ho, Wo), mean, std, out=o), ((B, C, Ho, Wo), torch.float32)))
    check(rec, cls, "fp32", y, *cpu(d.value, d.abs_terms + 3.0 / n * (H * d.dy_terms + W * d.dx_terms)), n, "resize_norm_fwd")
    a = D.resize_norm_adj(gy, (H, W), std)
    ky = int((D.resize_matrices(H, Ho)[0] != 0).sum(dim=0).max())
    kx = int((D.resize_matrices(W, Wo)[0] != 0).sum(dim=0).max())
    n = kx + ky + 6 + (1 if norm else 0)
    gx = twice(lambda: into(lambda o: hb.resize_norm_bwd(gy, (H, W), std, out=o), ((B, C, H, W), torch.float32)))
    check(rec, cls, "fp32", gx, *cpu(a.value, a.abs_terms + 3.0 / n * (H * a.dy_terms + W * a.dx_terms)), n, "resize_norm_bwd")


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("case", RESIZE_GAUSS, ids=lambda c: "-".join(map(str, c)))
def test_resize_norm_gauss(case, norm, rec):
    resize_check(rec, case, "gauss", norm)


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "plain"])
@pytest.mark.parametrize("case", RESIZE_EXACT, ids=lambda c: "-".join(map(str, c)))
def test_resize_norm_exact(case, norm, rec):
    resize_check(rec, case, "exact", norm)


def test_resize_norm_grid_stride_loops_wrap(rec):
    B, C, H, W, Ho, Wo, _ = RESIZE_WRAP
    assert B * C * Ho * Wo == 4214784 > CAP and B * C * H * W > CAP
    resize_check(rec, RESIZE_WRAP, "gauss", True)


# ---- the LPIPS tap, fp32 NCHW ----------------------------------------------------------------------------------------------------
LP16 = [(2, 192, 5, 7), (2, 384, 3, 5), (1, 256, 1, 1), (2, 130, 8, 8), (2, 129, 5, 13)]
LP4 = [(3, 64, 9, 9), (2, 1, 5, 5), (2, 35, 8, 9), (2, 72, 1, 65), (17, 128, 64, 64)]
assert set(LP16 + LP4[:-1]) == set(LPIPS_SHAPES)  # the shapes whose inputs tests/test_frozen_defs_cpu.py looks at


def lp_units(C, nblk, sl):
    """The chain lengths of the docstring, in units of 2^-24: (En, N of the distance, factor of own, factor of cross).  nblk: the
    partial sums the caller adds up; sl: the waves that share a pixel (NCHW), 0 for the NHWC kernels."""
    if sl:
        L, X, R = -(-C // sl), 2 + sl // 4, 6 + 1 + nblk
    else:
        L, X, R = 8 * -(-C // 64), 3, 3 + 2 + 1 + nblk
    en = (2 * L + X) / 2 + 1
    return en, 2 * (en + 4) + 2 + L + X + R, 2 * en + 11, (en + 6 + L + X) + 3 * en + 9


def lp_grad_check(rec, got, want, own, cross, units, prec, what):
    lim = EW[prec] * want.abs() + U * (own * units[2] + cross * units[3])
    assert got.dtype == DT[prec] and tuple(got.shape) == tuple(want.shape)
    rec.ratio(_worst(got, want, lim), what)


def lpips_case(shape, bf16=False):
    f0, f1, lin, gout = lpips_inputs(shape)
    if bf16:
        f0, f1 = f0.bfloat16(), f1.bfloat16()
        return cl(f0), cl(f1), lin.to(DEV), gout.to(DEV)
    return f0.to(DEV), f1.to(DEV), lin.to(DEV), gout.to(DEV)


@pytest.mark.parametrize("shape,sl", [(s, 16) for s in LP16] + [(s, 4) for s in LP4], ids=lambda v: sid(v) if isinstance(v, tuple) else "sl%d" % v)
def test_lpips_tap_nchw(shape, sl, rec):
    B, C, H, W = shape
    HW, blocks = H * W, -(-H * W // 64)
    assert (blocks * B < 1024 and C >= 128) == (sl == 16)
    f0, f1, lin, gout = lpips_case(shape)
    d = D.lpips_tap(f0, f1, lin, gout)
    units = lp_units(C, blocks, sl)
    fwd = lambda: into(lambda a, b: hb.lpips_taps_fwd([f0], [f1], [lin], keep_norms=True, out_norms=[(a, b)]), ((B, HW), torch.float32),
                       ((B, HW), torch.float32))
    assert targs(_kernels_of(fwd), "lpips_tap_fwd_kernel") == (sl,)
    dist, norms = fwd()
    dist2, norms2 = fwd()
    assert torch.equal(dist, dist2) and torch.equal(norms[0][0], norms2[0][0]) and torch.equal(norms[0][1], norms2[0][1]), "second call differs"
    r0, r1 = norms[0]
    check(rec, "gauss", "fp32", dist, *cpu(d.dist, d.abs_dist), units[1], "distance")
    check(rec, "gauss", "fp32", r0, *cpu(d.r0, d.r0), units[0], "norms of f0")
    check(rec, "gauss", "fp32", r1, *cpu(d.r1, d.r1), units[0], "norms of f1")
    dist3, none = hb.lpips_taps_fwd([f0], [f1], [lin], keep_norms=False)
    assert none == [(None, None)] and torch.equal(dist3, dist), "keep_norms=False changes the distance"
    bwd = lambda w0, w1: into(lambda o0, o1: hb.lpips_tap_bwd(f0, f1, lin, r0, r1, gout, w0, w1, out0=o0, out1=o1), (shape, torch.float32),
                              (shape, torch.float32))
    assert targs(_kernels_of(lambda: bwd(True, True)), "lpips_tap_bwd_kernel") == (sl,)
    g0, g1 = twice(lambda: bwd(True, True))
    lp_grad_check(rec, g0, d.g0, d.own0, d.cross0, units, "fp32", "gradient to f0")
    lp_grad_check(rec, g1, d.g1, d.own1, d.cross1, units, "fp32", "gradient to f1")
    only0, only1 = bwd(True, False), bwd(False, True)
    assert only0[1] is None and only1[0] is None and torch.equal(only0[0], g0) and torch.equal(only1[1], g1), "want0 / want1 singly"


LP_MULTI = [(2, 192, 5, 7), (2, 35, 8, 9), (2, 72, 1, 65), (2, 130, 8, 8)]  # 1 + 2 + 2 + 1 blocks: partial_stride 6 > every tap's own


def test_lpips_several_taps_in_one_call(rec):
    taps = [lpips_case(s) for s in LP_MULTI]
    nblk = sum(-(-s[2] * s[3] // 64) for s in LP_MULTI)
    assert nblk == 6
    dist = twice(lambda: hb.lpips_taps_fwd([t[0] for t in taps], [t[1] for t in taps], [t[2] for t in taps], keep_norms=True)[0])
    want = lim_terms = alone = 0
    for s, t in zip(LP_MULTI, taps):
        d = D.lpips_tap(t[0], t[1], t[2])
        sl = 16 if s[1] >= 128 and 2 * -(-s[2] * s[3] // 64) < 1024 else 4
        want, lim_terms = want + d.dist, lim_terms + lp_units(s[1], nblk, sl)[1] * d.abs_dist
        alone = alone + hb.lpips_taps_fwd([t[0]], [t[1]], [t[2]], keep_norms=False)[0].double()  # partial_stride = its own blocks
    check(rec, "gauss", "fp32", dist, *cpu(want, lim_terms), 1, "distance over four taps")
    # the same partial sums through other offsets and strides: they differ by the order of one fp32 sum of six numbers
    assert bool(((dist.double() - alone).abs() <= nblk * U * alone.abs()).all()), (dist, alone)


# ---- the LPIPS tap, bf16 NHWC --------------------------------------------------------------------------------------------------------
LPN = [(3, 64, 63, 63), (2, 192, 31, 31), (4, 384, 15, 15), (2, 256, 15, 15), (1, 8, 1, 1), (2, 72, 5, 7), (2, 8, 1, 31), (2, 8, 4, 8), (2, 8, 3, 11)]


@pytest.mark.parametrize("shape", LPN, ids=[sid(s) for s in LPN])
def test_lpips_tap_nhwc(shape, rec):
    B, C, H, W = shape
    HW, blocks = H * W, -(-H * W // 32)
    f0, f1, lin, gout = lpips_case(shape, bf16=True)
    assert bool((f0.float().abs().sum(1) > 0).all()) and bool((f1.float().abs().sum(1) > 0).all()), "an all-zero pixel"
    d = D.lpips_tap(f0, f1, lin, gout)
    units = lp_units(C, blocks, 0)
    fwd = lambda: into(lambda a, b: hb.lpips_taps_nhwc_fwd([f0], [f1], [lin], keep_norms=True, out_norms=[(a, b)]), ((B, HW), torch.float32),
                       ((B, HW), torch.float32))
    dist, norms = fwd()
    dist2, norms2 = fwd()
    assert torch.equal(dist, dist2) and torch.equal(norms[0][0], norms2[0][0]) and torch.equal(norms[0][1], norms2[0][1]), "second call differs"
    r0, r1 = norms[0]
    check(rec, "gauss", "fp32", dist, *cpu(d.dist, d.abs_dist), units[1], "distance")
    check(rec, "gauss", "fp32", r0, *cpu(d.r0, d.r0), units[0], "norms of f0")
    check(rec, "gauss", "fp32", r1, *cpu(d.r1, d.r1), units[0], "norms of f1")
    dist3, none = hb.lpips_taps_nhwc_fwd([f0], [f1], [lin], keep_norms=False)
    assert none == [(None, None)] and torch.equal(dist3, dist)
    bwd = lambda w0, w1: into(lambda o0, o1: hb.lpips_tap_nhwc_bwd(f0, f1, lin, r0, r1, gout, w0, w1, out0=o0, out1=o1),
                              (shape, torch.bfloat16, True), (shape, torch.bfloat16, True))
    g0, g1 = twice(lambda: bwd(True, True))
    assert hb.is_cl(g0) and hb.is_cl(g1)
    lp_grad_check(rec, g0, d.g0, d.own0, d.cross0, units, "bf16", "gradient to f0")
    lp_grad_check(rec, g1, d.g1, d.own1, d.cross1, units, "bf16", "gradient to f1")
    only0, only1 = bwd(True, False), bwd(False, True)
    assert only0[1] is None and only1[0] is None and torch.equal(only0[0], g0) and torch.equal(only1[1], g1), "want0 / want1 singly"


# ---- layout bridges, relu_gate_add ---------------------------------------------------------------------------------------------------
BRIDGE = [(2, c, h, w) for c in (8, 72, 136) for h, w in ((1, 1), (7, 9), (8, 8), (5, 13))]  # HW = 1, 63, 64, 65


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", BRIDGE, ids=[sid(s) for s in BRIDGE])
def test_bridges_and_relu_gate_add(shape, cls, rec):
    g = gen("bridge", shape, cls)
    x = draw(g, shape, cls, "fp32")
    xd = x.to(DEV)
    for relu in (False, True):
        y = twice(lambda: into(lambda o: hb.nchw_to_cl_bf16(xd, relu=relu, out=o), (shape, torch.bfloat16, True)))
        v = D.bridge_fwd(x, relu)
        check(rec, "exact", "bf16", y, v, v.abs(), 0, "nchw_to_cl_bf16(relu=%s)" % relu)
    a, b, gate = draw(g, shape, cls, "bf16"), draw(g, shape, cls, "bf16"), draw_gate(g, shape, cls, "bf16")
    ad, bd, gd = cl(a), cl(b), cl(gate)
    for gt, gtd in ((None, None), (gate, gd)):
        got = twice(lambda: into(lambda o: hb.cl_bf16_to_nchw(ad, gate=gtd, out=o), (shape, torch.float32)))
        v = D.bridge_bwd(a, gt)
        assert got.is_contiguous()
        check(rec, "exact", "bf16", got, v, v.abs(), 0, "cl_bf16_to_nchw(gate=%s)" % (gt is not None), out_prec="fp32")
    for other, od in ((b, bd), (None, None)):
        got = twice(lambda: into(lambda o: hb.relu_gate_add(ad, od, gd, out=o), (shape, torch.bfloat16, True)))
        v = D.relu_gate_add(a, other, gate)
        check(rec, "exact", "bf16", got, v.value, v.abs_terms, 1, "relu_gate_add(b=%s)" % (other is not None))


def test_relu_gate_add_grid_stride_loop_wraps(rec):
    shape = (8, 64, 257, 256)
    assert math.prod(shape) // 8 > CAP
    g = torch.Generator(device=DEV).manual_seed(77)
    mk = lambda: torch.randn(shape, device=DEV, generator=g).bfloat16().contiguous(memory_format=torch.channels_last)
    a, b, y = mk(), mk(), mk()
    got = into(lambda o: hb.relu_gate_add(a, b, y, out=o), (shape, torch.bfloat16, True))
    want = torch.where(y.float() > 0, (a.double() + b.double()).float(), torch.zeros((), device=DEV)).bfloat16()
    assert torch.equal(got, want), "relu_gate_add beyond one pass of the grid"
    rec.equal()


# ---- MaxPool2d(3, 2) on bf16 NHWC ---------------------------------------------------------------------------------------------------------
MAXPOOL = [(2, 64, 63, 63), (3, 192, 31, 31), (1, 8, 3, 3), (2, 16, 8, 11), (1, 24, 4, 7), (1, 8, 3, 4), (1, 8, 4, 3), (2, 16, 5, 6)]


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("shape", MAXPOOL, ids=[sid(s) for s in MAXPOOL])
def test_maxpool3s2_nhwc(shape, cls, rec):
    B, C, H, W = shape
    ho, wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    g = gen("maxpool", shape, cls)
    if cls == "exact":
        x = draw(g, shape, "exact", "bf16", lim=2)
    else:
        x = ((torch.randn(shape, generator=g).relu() * 4).round() / 4).bfloat16()  # ties at zero and among the positive values
        if H * W > 20:
            x[0, 0, 1, 1] = NAN
            x[-1, -1, H - 2, W - 2] = NAN
    gy = draw(g, (B, C, ho, wo), cls, "bf16")
    xd, gyd = cl(x), cl(gy)
    d = D.maxpool3s2(x)
    fwd = lambda: into(lambda o, oi: hb.maxpool3s2_cl_fwd(xd, out=o, out_idx=oi), ((B, C, ho, wo), torch.bfloat16, True),
                       ((B, ho, wo, C), torch.uint8))
    (y, idx), (y2, idx2) = fwd(), fwd()
    bits = lambda t: t.permute(0, 2, 3, 1).view(torch.int16)  # NaNs compare by their bit pattern
    assert torch.equal(bits(y), bits(y2)) and torch.equal(idx, idx2), "second call differs"
    assert y.dtype == torch.bfloat16 and hb.is_cl(y)
    assert torch.equal(torch.nan_to_num(y.cpu().double(), nan=-7.0), torch.nan_to_num(d.y, nan=-7.0)), "maxima"
    assert torch.equal(idx.cpu().permute(0, 3, 1, 2), d.pos), "window positions"
    rec.equal()
    bw = D.maxpool3s2_bwd(gy, d.pos, (H, W))
    posd = d.pos.permute(0, 2, 3, 1).contiguous().to(DEV)
    gx = twice(lambda: into(lambda o: hb.maxpool3s2_cl_bwd(gyd, posd, (H, W), out=o), (shape, torch.bfloat16, True)))
    check(rec, cls, "bf16", gx, bw.value, bw.abs_terms, 3, "maxpool3s2_cl_bwd")


# ---- image gradient of the stems -------------------------------------------------------------------------------------------------------
IMG_GRAD = [  # (B, N, C, K, S, pad, Hi, Wi), kernel, template arguments
    ((2, 5, 3, 11, 4, 2, 37, 45), "rt", (4, 3)),
    ((1, 13, 3, 13, 4, 6, 21, 70), "rt", (4, 4)),      # nt = 4; pad > S
    ((1, 8, 1, 5, 4, 0, 21, 17), "rt", (4, 4)),        # nt = 2; pad = 0; C = 1
    ((2, 5, 3, 7, 2, 3, 33, 130), "rt", (2, 4)),       # 65 class columns and 17 class rows: a second tile in both axes
    ((2, 13, 2, 5, 2, 2, 19, 23), "rt", (2, 3)),
    ((1, 5, 4, 3, 1, 1, 9, 70), "rt", (1, 3)),
    ((1, 6, 3, 4, 1, 2, 9, 11), "rt", (1, 4)),
    ((1, 3, 2, 2, 1, 0, 6, 7), "rt", (1, 4)),          # nt = 2 on the four-tap tile
    ((1, 384, 3, 3, 1, 1, 9, 9), "generic", (1,)),     # the register tile's LDS exceeds 64 KB
    ((1, 7, 3, 1, 1, 0, 5, 5), "generic", (1,)),       # K = 1: a single tap
    ((1, 5, 3, 9, 2, 4, 23, 21), "generic", (2,)),     # five taps per axis
    ((1, 344, 3, 11, 4, 2, 21, 25), "generic", (4,)),  # register-tile LDS 66,048 bytes
]


@pytest.mark.parametrize("case,kernel,args", IMG_GRAD, ids=["-".join(map(str, c)) for c, _, _ in IMG_GRAD])
def test_conv_image_grad_exact(case, kernel, args, rec):
    B, N, C, K, S, pad, H, W = case
    Ho, Wo = (H + 2 * pad - K) // S + 1, (W + 2 * pad - K) // S + 1
    g = gen("img-grad", case)
    dy, w = draw(g, (B, N, Ho, Wo), "exact", "fp32"), draw(g, (N, C, K, K), "exact", "fp32")
    dyd, wd = dy.to(DEV), w.to(DEV)
    want = D.conv_image_grad(dy, w, (H, W), S, pad)
    call = lambda: into(lambda o: hb.conv_image_grad(dyd, wd, (H, W), S, pad, out=o), ((B, C, H, W), torch.float32))
    names = _kernels_of(call)
    rt, gen_ = "conv_image_grad_rt_kernel", "conv_image_grad_kernel"
    if kernel == "rt":
        assert targs(names, rt) == args and gen_ + "<" not in names, names
    else:
        assert targs(names, gen_) == args and rt not in names, names
    check(rec, "exact", "fp32", twice(call), want.value, want.abs_terms, 0, "conv_image_grad")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _bf(shape, off=0):
    """A bf16 channels_last tensor of ones whose pointer is `off` elements past a 16-byte boundary."""
    B, C, H, W = shape
    buf = torch.ones(B * C * H * W + 8, dtype=torch.bfloat16, device=DEV)
    return buf[off:off + B * C * H * W].view(B, H, W, C).permute(0, 3, 1, 2)


def _f(*shape):
    return torch.ones(shape, device=DEV)


REFUSALS = {
    "bridge-fwd-C12": (lambda o: hb.nchw_to_cl_bf16(_f(1, 12, 2, 2), out=o), ((1, 12, 2, 2), torch.bfloat16, True)),
    "bridge-bwd-offset": (lambda o: hb.cl_bf16_to_nchw(_bf((1, 8, 2, 2), 2), out=o), ((1, 8, 2, 2), torch.float32)),
    "bridge-bwd-gate-offset": (lambda o: hb.cl_bf16_to_nchw(_bf((1, 8, 2, 2)), gate=_bf((1, 8, 2, 2), 2), out=o), ((1, 8, 2, 2), torch.float32)),
    "relu-gate-add-C12": (lambda o: hb.relu_gate_add(_bf((1, 12, 1, 1)), None, _bf((1, 12, 1, 1)), out=o), ((1, 12, 1, 1), torch.bfloat16, True)),
    "relu-gate-add-offset": (lambda o: hb.relu_gate_add(_bf((1, 8, 2, 2), 2), None, _bf((1, 8, 2, 2)), out=o), ((1, 8, 2, 2), torch.bfloat16, True)),
    "maxpool-offset": (lambda o: hb.maxpool3s2_cl_fwd(_bf((1, 8, 3, 3), 2), out=o), ((1, 8, 1, 1), torch.bfloat16, True)),
    "maxpool-bwd-offset": (lambda o: hb.maxpool3s2_cl_bwd(_bf((1, 8, 1, 1), 2), torch.zeros(1, 1, 1, 8, dtype=torch.uint8, device=DEV), (3, 3), out=o),
                           ((1, 8, 3, 3), torch.bfloat16, True)),
    "lpips-nhwc-bwd-C12": (lambda o: hb.lpips_tap_nhwc_bwd(_bf((1, 12, 2, 2)), _bf((1, 12, 2, 2)), _f(12), _f(1, 4), _f(1, 4), _f(1), True, False, out0=o),
                           ((1, 12, 2, 2), torch.bfloat16, True)),
    "lpips-nhwc-bwd-offset": (lambda o: hb.lpips_tap_nhwc_bwd(_bf((1, 8, 2, 2), 2), _bf((1, 8, 2, 2)), _f(8), _f(1, 4), _f(1, 4), _f(1), True, False, out0=o),
                              ((1, 8, 2, 2), torch.bfloat16, True)),
    "img-grad-pad>=K": (lambda o: hb.conv_image_grad(_f(1, 2, 8, 8), _f(2, 3, 3, 3), (6, 6), 1, 3, out=o), ((1, 3, 6, 6), torch.float32)),
    "img-grad-S3": (lambda o: hb.conv_image_grad(_f(1, 2, 2, 2), _f(2, 3, 3, 3), (6, 6), 3, 1, out=o), ((1, 3, 6, 6), torch.float32)),
    "img-grad-C5": (lambda o: hb.conv_image_grad(_f(1, 2, 6, 6), _f(2, 5, 3, 3), (6, 6), 1, 1, out=o), ((1, 5, 6, 6), torch.float32)),
    "img-grad-Ho": (lambda o: hb.conv_image_grad(_f(1, 2, 5, 6), _f(2, 3, 3, 3), (6, 6), 1, 1, out=o), ((1, 3, 6, 6), torch.float32)),
    "resize-mean-without-std": (lambda o: hb.resize_norm_fwd(_f(1, 3, 4, 4), (5, 5), mean=_f(3), std=None, out=o), ((1, 3, 5, 5), torch.float32)),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_launchers_refuse_what_they_document(name):
    fn, spec = REFUSALS[name]
    buf, out = guarded(*spec)
    with pytest.raises(hb.StylexHipError):
        fn(out)
    torch.cuda.synchronize()
    assert untouched(buf), "a refused call wrote to its output"


def test_lpips_nhwc_forward_refuses_ragged_channels_and_offset_pointers():
    for f0, c in ((_bf((1, 12, 2, 2)), 12), (_bf((1, 8, 2, 2), 2), 8)):
        with pytest.raises(hb.StylexHipError):
            hb.lpips_taps_nhwc_fwd([f0], [_bf((1, c, 2, 2))], [_f(c)], keep_norms=False)
