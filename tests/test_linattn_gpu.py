"""-m gpu: the eleven kernels of csrc/linattn.hip (attention core forward and backward, ChanNorm forward and backward, the
depthwise 3x3 and its weight gradient, the slice reduction) against their float64 definitions (tests/_linattn_defs.py), element
by element.  Run this file before any change to linattn.hip.

Method and helpers are those of tests/test_ew_torgb_gpu.py and tests/test_frozen_ew_gpu.py (read their docstrings first): the hb
wrappers are called directly on seeded inputs rounded to the activation dtype first; the references are taken in float64 from
the rounded values; a second call must be bit-identical; the instantiation that ran, <true> (bf16) or <false> (fp32), is read
from the profiler's kernel names.  Every output of every entry point is checked, the saved ones (pre, context, lse, mean, std)
included.  Inputs, plans, chain counts, limits and the comparison itself are those of tests/test_linattn_defs_cpu.py, which
holds an fp32 model of the pass structure to them on the CPU and shows that mutations of the model break them; nothing here is
tuned against the kernels.  The backward entry points are functions of their saved operands: they are handed the definition's
pre (rounded to the activation dtype: in bf16 the stored value), context and lse (rounded to fp32), and the reference is taken
from those.

EXACT class: the result must EQUAL float32(definition), or bfloat16(float32(definition)).
  depthwise        integer operands in [-4, 4], weights k / 4; the sums are below 2^24 (asserted from abs_terms).
  ChanNorm         eps = 0; every pixel is m +- s, half the channels on either side, m an integer, s in {1/2, 1}, per pixel; g, b
                   multiples of 1/2: mean, std, y, gx, dg, db are exact.  The reference's formula is 0 / 0 at a pixel of std 0 with
                   eps = 0, so that pixel runs in a second call: s = 1/2 everywhere, eps = 1/2 (std + eps = 1), pixel 0 with all
                   channels equal: std = 0, y = b, and gx without its second term (the kernel's documented convention).
  attention fwd    k is 0 on a pixel set S_d and -128 elsewhere, |S_d| a power of two, S_d seeded per (sample, head, channel);
                   S_0 lies in the last tile of chunk 0 (the rescale by exp(-128 - 0) = 0 wipes the accumulator of the earlier
                   tiles, whose exp(k - max) were all 1), S_1 in the last chunk, and every chunk but one has no member of
                   columns 0 and 1.  q rows are 0 on 2^j channels, j in [0, 3], -128 elsewhere; v integers in [-4, 4].  exp(-128) is 0
                   in fp32, so K is 0 or 1 / |S_d| and Q is 0 or 2^(-3-j): pre and context are exact.  lse and y go through
                   logf / erff and are held to the Gauss bound, y as gelu_erf of the fp32 pre just shown to be exact (the float64
                   definition keeps exp(-128) = 2.6e-56, which no fp32 result can follow).
  attention bwd    pre = 0 (gelu' = 1/2), context k / 4, lse = 0 with k in {0, -128}, q as above, v integers, gy even integers:
                   dq, dk, dv equal the closed form.

GAUSS class: per element  |got - want| <= EW |want| + 2^-24 (N abs_terms + arg_terms),  EW = 2^-22 (fp32) / 2^-8 (bf16); where
the limit is 0 the result must be 0.  arg_terms: see _linattn_defs.  N = fp32 roundings on the longest path of a term, counted
without contraction; a library call counts as its OpenCL full-profile bound (exp 3, log 3, erf 16 ulp; these are the documented
bounds, not measured ones: the record shows how much of each limit a run uses); division and square root round once (no
fast-math in the build).  T = tiles per chunk, nch = chunks (attn_counts), lp = log2(C / 4), PPB = 256 >> lp pixels per pass,
passes / blocks of the pixel stream (norm_counts):
  Q (row soft-max)     N_Q = 15            expf 3, e * s, and s = 0.125 / sum: expf 3, 3 lane adds, 4 shuffle adds, the division
  column sum S         19 + 5 (T - 1) + nch    expf 3, 8 + 3 LDS adds, s_run * al + .; per further tile expf(al) 3, *, +; combine: expf 3, *, nch adds
  context              36 T + 5 + nch + 1 + N_S    per tile expf 3, e * v, 32 adds (further tiles: expf(al) 3, acc * al, 32 adds);
                                           combine expf 3, *, nch adds, * invS; invS = 1 / S carries N_S
  lse                  3 |log S| + N_S + sum_n K |k - max|  (in 2^-24), + EW |lse| for the final sum
  pre                  N_context + N_Q + 1 + 64
  y                    (16 / 2 + 3) |pre| + 1.13 (N_pre abs_pre + arg_pre): erff at the half-weight, x * c, 1 + ., two products;
                       1.13 bounds |gelu'|
  G = gy gelu'(pre)    N_G = 28            erff 16, its argument, 1 + ., 0.5 *; x * x, expf 3, two products; the sum; * gy
  dq                   N_Q + (N_G + 1 + 64) + (N_Q + 1 + 3 + 4) + 2    Q; dQ = G C^T; the row dot product; a - dot; Q * .
  dC                   N_Q + N_G + 1 + 32 T + nch
  dv                   3 + N_dC + 1 + 64   K = expf(k - lse)
  dk                   3 + N_dC + 1 + 64 + 2
  ChanNorm mean        3 + lp              1 / C is a power of two
           std         N_mean + 1 + (4 + lp) / 2 + 1     on abs_terms = std + mean|x|: the mean's error is an absolute error of x - mean
           y           (N_mean + 1) + (N_std + 2) + 3    on |g| inv (|x| + mean|x|) (1 + |d| inv) + |b|
           gx          18 + lp
           dg, db      5 + passes + PPB + blocks,  passes + PPB + blocks
  depthwise fwd        10                  a product and nine additions
  depthwise dw         1 + passes + PPB + blocks

Plans, asserted against stylex_linattn_chunks and the re-stated plan_of ((B, heads, H, W): chunks x pixels, tiles per chunk):
  (1, 1, 1, 1)        1 x 32, 1    one pixel
  (3, 2, 3, 11)       2 x 32, 1    the last chunk of 1 pixel
  (1, 1, 32, 64)      64 x 32, 1   the MAXCHUNK cap, every tile full
  (1, 1, 45, 47)      34 x 64, 2   the last chunk of 3 pixels
  (1, 1, 50, 82)      43 x 96, 3   the last chunk with tiles 32 / 32 / 4
  (128, 8, 7, 10)     2 x 64, 2    the second chunk of 6 pixels
  (256, 8, 5, 8)      1 x 64, 2    nch = 1, tiles 32 + 8
The small shapes also run with k and v as separate dense tensors and with q as a channel slice of a wider tensor (the default is
k, v as the two channel halves of one NHWC tensor, as LinearAttention passes them).  ChanNorm and depthwise run at every host width
4 .. 256 on (2, C, 5, 7), (3, C, 1, 1), (3, C, 1, 9), (3, C, 6, 1); the depthwise forward also at C = 12; at C = 4 and C = 256 the
ChanNorm forward runs just over 4096 blocks and the ChanNorm backward and the depthwise weight gradient just over 1024 blocks of
8 passes (references in float64 on the device).

With STYLEX_LINATTN_RECORD=<file> every case leaves one line in that file: its worst error / limit
(profiles/linattn_errors.txt is the record of one run)."""
import os
import re

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.against_definition]

import _linattn_defs as D  # noqa: E402
import hip_backend as hb  # noqa: E402
import test_linattn_defs_cpu as T  # noqa: E402
from test_ew_torgb_gpu import DEV, DT, Recorder, hip_impl, sid, twice  # noqa: E402,F401
from test_stream_kernels_gpu import _kernels_of  # noqa: E402

NAN = float("nan")
_LINES = []


@pytest.fixture
def rec(request):
    r = Recorder()
    yield r
    name = request.node.nodeid.split("::", 1)[-1]
    tail = "".join("  [%s]" % e for e in r.each) + ("  [%d exact comparisons]" % r.exact if r.exact else "")
    _LINES.append("%-64s %8.4f  %s%s" % (name, r.worst, r.what or "-", tail))


HEADER = """# tests/test_linattn_gpu.py: per test case, the worst observed error / limit (<= 1 passes) of its Gauss-class quantities and the
# quantity that gave it, then [every quantity]; exact-class quantities assert equality with the rounded float64 definition and
# are counted.  Limit per element: EW * |want| + 2^-24 * (N * abs_terms + arg_terms), EW = 2^-22 (fp32) / 2^-8 (bf16), N per
# kernel and plan as in the file's docstring.
# Ratios above 0.5 are bf16 outputs (pre, y, dq, dk, dv, ChanNorm y / gx, depthwise y): the one round-to-nearest-even store.  Half
# a bf16 spacing is 2^-8 of the power of two below the value, so a value just above a power of two that lands near a tie
# reaches 2^-8 / (1 + 2^-8) = 0.9961 of EW * |want| legitimately; the fp32 part of the error is what the fp32 rows show.
"""


@pytest.fixture(scope="module", autouse=True)
def _write_errors():
    yield
    out = os.environ.get("STYLEX_LINATTN_RECORD")
    if out and _LINES:
        with open(out, "w") as f:
            f.write(HEADER + "\n".join(_LINES) + "\n")


# ---- helpers -----------------------------------------------------------------------------------------------------------------
def act(t, prec):
    return t.to(DEV).to(DT[prec]).contiguous(memory_format=torch.channels_last)


def ran(fn, kernels, prec):
    """fn() once under the profiler: each of `kernels` ran in the instantiation of `prec` and in no other."""
    names = _kernels_of(fn)
    for k in kernels:
        found = set(re.findall(re.escape(k) + r"<(true|false)>", names))
        assert found == {"true" if prec == "bf16" else "false"}, (k, found, names)


def record(rec, cls, res):
    for name, v in res.items():
        if isinstance(v, bool):
            assert v, "%s (exact class) differs from the rounded definition" % name
            rec.equal()
        else:
            rec.ratio(v, name)


def laid_out(q, k, v, prec, layout):
    """Device operands in the layout named; the attention wrappers must address them in place."""
    if layout == "dense":
        return act(q, prec), act(k, prec), act(v, prec)
    kd, vd = act(torch.cat([k, v], dim=1), prec).chunk(2, dim=1)
    qd = act(q, prec)
    if layout == "qslice":
        B, C, H, W = q.shape
        wide = torch.full((B, H, W, C + 8), NAN, dtype=DT[prec], device=DEV).permute(0, 3, 1, 2)
        wide[:, 4:4 + C] = qd
        qd = wide[:, 4:4 + C]
        assert hb._nhwc_view(qd)[0] is qd
    assert hb._nhwc_view(kd)[0] is kd and hb._nhwc_view(vd)[0] is vd
    return qd, kd, vd


def attn_pair(heads, prec, layout):
    def fwd(q, k, v):
        qd, kd, vd = laid_out(q, k, v, prec, layout)
        call = lambda: hb.linattn_fwd(qd, kd, vd, heads)
        ran(call, ("linattn_ctx_partial", "linattn_out"), prec)
        return twice(call)

    def bwd(q, k, v, pre, gy, context, lse):
        qd, kd, vd = laid_out(q, k, v, prec, layout)
        pd, gd, cd, ld = act(pre, prec), act(gy, prec), context.to(DEV).contiguous(), lse.to(DEV).contiguous()
        call = lambda: hb.linattn_bwd(qd, kd, vd, pd, cd, ld, gd, heads)
        ran(call, ("linattn_bwd_q", "linattn_bwd_kv"), prec)
        return twice(call)

    return fwd, bwd


# ---- attention core ------------------------------------------------------------------------------------------------------------
SMALL = [(1, 1, 1, 1), (3, 2, 3, 11)]
ATTN_GAUSS = [(c, k, "kv") for c, k in T.GAUSS_CORE] + [(c, "plain", lay) for c in SMALL for lay in ("dense", "qslice")]
ATTN_EXACT = [(c, "kv") for c in T.CORE] + [(c, lay) for c in SMALL for lay in ("dense", "qslice")]


def test_the_library_plans_the_chunks_listed():
    lib = hb.load_library()
    for (B, heads, H, W), pl in T.CORE.items():
        assert lib.stylex_linattn_chunks(hb._shape(B, H * W, heads)) == pl.nch == T.plan_of(B, heads, H * W).nch, (B, heads, H, W)
    for shape in NORM_BWD_CAP:
        B, C, H, W = shape
        st = T.stream_of(B * H * W, C)
        assert lib.stylex_chan_norm_bwd_blocks(hb._shape(B * H * W, C)) == st.blocks == 1024 and st.passes == 9
        assert lib.stylex_dwconv3x3_wgrad_blocks(hb._shape(B, H, W, C)) == 1024


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("case,kind,layout", ATTN_GAUSS, ids=["%s-%s-%s" % (sid(c), k, lay) for c, k, lay in ATTN_GAUSS])
def test_attention_gauss(case, kind, layout, prec, rec):
    record(rec, "gauss", T.attn_gauss_ratios(case, kind, prec, *attn_pair(case[1], prec, layout)))


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("case,layout", ATTN_EXACT, ids=["%s-%s" % (sid(c), lay) for c, lay in ATTN_EXACT])
def test_attention_exact(case, layout, prec, rec):
    res, (d, y, lse) = T.attn_exact_results(case, prec, *attn_pair(case[1], prec, layout))
    record(rec, "exact", res)
    want, lim, _ = T.fwd_limits(d, T.attn_counts(T.plan_of(case[0], case[1], case[2] * case[3])), prec)["lse"]
    assert lse.dtype == torch.float32 and y.dtype == DT[prec]
    rec.ratio(T.worst(lse, want, lim), "lse")
    rec.ratio(T.worst(y, *T.exact_y_limit(d, prec)), "y")


# ---- ChanNorm, depthwise -------------------------------------------------------------------------------------------------------
def norm_pair(prec):
    def fwd(x, g, b, eps):
        xd, gd, bd = act(x, prec), g.to(DEV), b.to(DEV)
        call = lambda: hb.chan_norm_fwd(xd, gd, bd, eps)
        ran(call, ("chan_norm_fwd_kernel",), prec)
        return twice(call)

    def bwd(x, gy, g, mean, std, eps):
        xd, gyd, gd, md, sd = act(x, prec), act(gy, prec), g.to(DEV), mean.to(DEV).contiguous(), std.to(DEV).contiguous()
        call = lambda: hb.chan_norm_bwd(xd, gyd, gd, md, sd, eps)
        ran(call, ("chan_norm_bwd_kernel",), prec)
        gx, dg, db = twice(call)
        only = hb.chan_norm_bwd(xd, gyd, gd, md, sd, eps, want_params=False)
        assert only[1] is None and only[2] is None and torch.equal(only[0], gx), "want_params=False changes gx"
        return gx, dg, db

    return fwd, bwd


def conv_pair(prec, wgrad=True):
    def conv(x, w):
        xd, wd = act(x, prec), w.to(DEV)
        call = lambda: hb.dwconv3x3_fwd(xd, wd)
        ran(call, ("dwconv3x3_kernel",), prec)
        return twice(call)

    def wg(x, gy):
        xd, gyd = act(x, prec), act(gy, prec)
        call = lambda: hb.dwconv3x3_bwd_weight(xd, gyd)
        ran(call, ("dwconv3x3_wgrad_kernel",), prec)
        return twice(call)

    return conv, (wg if wgrad else None)


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("shape", T.HOST, ids=[sid(s) for s in T.HOST])
def test_chan_norm(shape, cls, prec, rec):
    assert hb.chan_norm_supported(shape[1])
    record(rec, cls, T.norm_ratios(shape, cls, prec, *norm_pair(prec)))
    if cls == "exact":
        x, gy, g, b, eps = T.norm_flat_inputs(shape)
        record(rec, cls, T.norm_ratios(shape, cls, prec, *norm_pair(prec), inputs=(x, gy, g, b, eps)))
        y, _, std = hb.chan_norm_fwd(act(x, prec), g.to(DEV), b.to(DEV), eps)
        assert float(std[0]) == 0.0 and torch.equal(y[0, :, 0, 0].float().cpu(), b.to(DT[prec]).float()), "the pixel of std 0: y = b"


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("shape", T.HOST + [(2, 12, 5, 7)], ids=[sid(s) for s in T.HOST + [(2, 12, 5, 7)]])
def test_depthwise(shape, cls, prec, rec):
    """C = 12: a multiple of 4 that is no power of two; the forward kernel accepts it (dwconv3x3_supported does not route it there)."""
    pow2 = hb.dwconv3x3_supported(shape[1])
    assert pow2 == (shape[1] != 12)
    record(rec, cls, T.conv_ratios(shape, cls, prec, *conv_pair(prec, wgrad=pow2)))


# ---- the grid-stride wrap of the ChanNorm forward, the 1024-block cap of the pixel streams ---------------------------------------
NORM_FWD_WRAP = [(1, 256, 129, 128), (1, 4, 1025, 1024)]   # just over 4096 blocks of 4 / 256 pixels
NORM_BWD_CAP = [(1, 256, 129, 256), (1, 4, 1025, 2048)]    # just over 1024 blocks x 8 passes of 4 / 256 pixels


def test_wrap_shapes_are_just_over_the_caps():
    for (B, C, H, W), (B2, C2, H2, W2) in zip(NORM_FWD_WRAP, NORM_BWD_CAP):
        ppb = T.NT // (C // 4)
        assert 4096 * ppb < B * H * W <= 4096 * ppb * 1.01 and 1024 * 8 * ppb < B2 * H2 * W2 <= 1024 * 8 * ppb * 1.01 and C == C2


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("shape", NORM_FWD_WRAP, ids=[sid(s) for s in NORM_FWD_WRAP])
def test_chan_norm_forward_grid_stride_loop_wraps(shape, cls, prec, rec):
    inputs = T.norm_inputs(shape, cls, prec, dev=DEV)
    res = T.norm_ratios(shape, cls, prec, norm_pair(prec)[0], lambda *a: (None,) * 3, inputs=inputs, only=("y", "mean", "std"))
    record(rec, cls, res)


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("shape", NORM_BWD_CAP, ids=[sid(s) for s in NORM_BWD_CAP])
def test_chan_norm_backward_at_the_block_cap(shape, cls, prec, rec):
    inputs = T.norm_inputs(shape, cls, prec, dev=DEV)
    res = T.norm_ratios(shape, cls, prec, lambda *a: (None,) * 3, norm_pair(prec)[1], inputs=inputs, only=("gx", "dg", "db"))
    record(rec, cls, res)


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("shape", NORM_BWD_CAP, ids=[sid(s) for s in NORM_BWD_CAP])
def test_depthwise_weight_gradient_at_the_block_cap(shape, cls, prec, rec):
    inputs = T.conv_inputs(shape, cls, prec, dev=DEV)
    record(rec, cls, T.conv_ratios(shape, cls, prec, None, conv_pair(prec)[1], inputs=inputs))
