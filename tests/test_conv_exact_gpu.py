"""-m gpu: every conv kernel instantiation against its definition (tests/_conv_exact_defs.py), BIT FOR BIT.

The MFMA kernels multiply bf16 by bf16, accumulate in fp32 and store once (round to nearest even).  On small-integer operands
every product and every partial sum is an exact fp32 number whatever the summation order, tile shape, K chunking or split-K
plan (the definitions assert sum|terms| / grid < 2^24), so a kernel must return the definition exactly: one lost, duplicated or
misplaced product anywhere fails torch.equal (tests/test_conv_exact_defs_cpu.py: >= 90 % of the outputs a product belongs to
move).  Run this file before any change to a conv kernel or to a selector.

ROWS is one table: the call, the shape (B, C, N, H, W of the conv; the space-to-depth calls give the HALF-resolution H, W),
the epilogue form, the environment switches and the (class, kernel instantiation) the row is written for, in the spelling of
stylex_note_kernel.  Every row asserts that the timing hook reports that instantiation, torch.equal for every output (masks
and bias sums included) and that a second call is bit-identical.  EXACT_KERNELS collects (class, name) -> row ids for
tests/test_zz_kernel_coverage_gpu.py.

Second layer (GAUSS): one case per family with normal operands rounded to bf16, per element
    |got - want| <= r * 2^-8 * |want| + TOL32 * A,
r = 1 bf16 rounding on every path here (the per-sample scales are powers of two, the gate slope is 0.25: neither rounds), A = the
definition's sum|terms|: RNE on non-integers and the 0.2f paths.  With STYLEX_CONV_EXACT_RECORD=<file> every case leaves its
worst error / bound in that file (profiles/conv_exact_errors.txt is the record of one run)."""
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.against_definition]

import _conv_exact_defs as D  # noqa: E402
import hip_backend as hb  # noqa: E402
import ops  # noqa: E402

DEV = "cuda:0"
TOL32 = 2e-5
EXACT_KERNELS = {}  # (cls, kernel) -> set of row ids that launched it and passed
_LINES = []


@pytest.fixture(autouse=True)
def hip_impl():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    prev = ops.use_impl(ops.HipOps)
    hb.load_library()
    _clear_shape_caches()
    yield
    _clear_shape_caches()
    ops.set_precision("fp32")
    ops.use_impl(prev)


def _clear_shape_caches():
    # answers cached per shape by hip_backend depend on the switches a row sets
    hb._MASK_OK.clear()
    hb._S2D_RES_OK.clear()
    hb._S2D_WGRAD_OK.clear()


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("STYLEX_CONV_EXACT_RECORD")
    if out and _LINES:
        with open(out, "w") as f:
            f.write("# tests/test_conv_exact_gpu.py.  exact rows: the instantiations the row launched (all outputs bit-identical to the\n"
                    "# definition).  gauss rows: the worst |got - want| / (2^-8 |want| + 2e-5 A) over all outputs (<= 1 passes), the output\n"
                    "# that gave it and the share of the 2e-5 A term in the bound at that element (> 0.5: the fp32 term binds there).\n")
            f.write("\n".join(_LINES) + "\n")


def cl(t, dtype):
    t = t.to(DEV).to(dtype)
    return t.contiguous(memory_format=torch.channels_last) if t.dim() == 4 else t.contiguous()


def dv(t):
    return None if t is None else t.to(DEV).contiguous()


# ---- the calls ---------------------------------------------------------------------------------------------------------
# Each returns a list of (name, got, want, A): got on the device, want / A float tensors on the CPU in logical layout.
def _geometry(row):
    B, C, N, H, W = row["shape"]
    return B, C, N, H, W, row.get("k", 3), row.get("stride", 1), row.get("pad", 1)


def call_fwd(row, o, P, adt, kw):
    B, C, N, H, W, k, s, p = _geometry(row)
    form = row["form"]
    x = o["x"].clone()
    if form.startswith("rgb"):  # the padded RGB slot: channels 3..7 are zero
        x[:, 3:] = 0
    a = dict(bias=None, lrelu=False)
    d = dict(act=None)
    if "bias" in form or form.startswith("rgb") or form == "full":
        a["bias"], d["bias"] = dv(o["bias"]), o["bias"]
    if "lrelu" in form or form.startswith("rgb") or form in ("full", "mod-noise", "mod-noise-nat"):
        a["lrelu"], d["act"] = True, "lrelu"
    if "relu" in form and "lrelu" not in form:
        a["lrelu"], d["act"] = "relu", "relu"
    if form in ("full", "mod-noise", "mod-noise-nat", "mod"):
        a.update(in_scale=dv(o["s_c"]), out_scale=dv(o["s_n"]))
        d.update(in_scale=o["s_c"], out_scale=o["s_n"])
    if form in ("full", "mod-noise", "mod-noise-nat"):
        nat = form.endswith("nat")
        plane = o["noise"].transpose(1, 2).contiguous() if nat else o["noise"]  # natural order: [b, h, w] = noise[b, w, h]
        a.update(noise=dv(plane), noise_w=dv(o["nw"]), noise_b=dv(o["nb"]), noise_natural=nat)
        d.update(noise=o["noise"], noise_w=o["nw"], noise_b=o["nb"])
    if form in ("full", "bias-res"):
        a.update(residual=cl(o["res"], adt), res_scale=0.5)
        d.update(residual=o["res"], res_scale=0.5)
    want_mask = "mask" in form
    got = hb.conv2d_fwd(cl(x, adt), dv(o["w"]), s, p, P, want_mask=want_mask, **a)
    if row.get("ref_dev", False) and not kw:  # many tiles: the exact reference as a float64 matmul on the device
        ref = D.forward(x.to(DEV), o["w"].to(DEV), s, p, dt=torch.float64, **{k_: (v.to(DEV) if torch.is_tensor(v) else v) for k_, v in d.items()})
        ref = D.Out(ref.y.cpu(), ref.A.cpu())
    else:
        ref = D.forward(x, o["w"], s, p, **d, **kw)
    outs = []
    if want_mask:
        got, mask = got
        assert mask is not None, "this launch was expected to write the activation bit mask"
        outs.append(("mask", mask, None, None))
    outs.insert(0, ("y", got, ref.y, ref.A))
    return outs


def call_dgrad(row, o, P, adt, kw):
    B, C, N, H, W, k, s, p = _geometry(row)
    form = row["form"]
    a, d = {}, {}
    if "scaled" in form:
        a.update(in_scale=dv(o["s_n"]), out_scale=dv(o["s_c"]))
        d.update(in_scale=o["s_n"], out_scale=o["s_c"])
    if "gate" in form:
        a.update(gate=cl(o["gate_in"], adt), gate_slope=D.GATE_SLOPE)
        d.update(gate=o["gate_in"])
    if "mask" in form:
        sh = hb.conv_shape((B, C, H, W), (N, C, k, k), s, p)
        assert hb.conv_mask_supported(sh, 1, hb.EPI_GATE_MASK, P), "this launch was expected to read the gate as a bit mask"
        a.update(gate_mask=D.pack_mask(o["gate_in"]).to(DEV), gate_slope=D.GATE_SLOPE)
        d.update(gate=o["gate_in"])
    got = hb.conv2d_bwd_data(cl(o["dy"], adt), dv(o["w"]), (B, C, H, W), s, p, P, **a)
    if row.get("ref_dev", False) and not kw:
        ref = D.dgrad(o["dy"].to(DEV), o["w"].to(DEV), (B, C, H, W), s, p, dt=torch.float64,
                      **{k_: (v.to(DEV) if torch.is_tensor(v) else v) for k_, v in d.items()})
        ref = D.Out(ref.y.cpu(), ref.A.cpu())
    else:
        ref = D.dgrad(o["dy"], o["w"], (B, C, H, W), s, p, **d, **kw)
    return [("dx", got, ref.y, ref.A)]


def call_wgrad(row, o, P, adt, kw):
    B, C, N, H, W, k, s, p = _geometry(row)
    form = row["form"]
    a, d = {}, {}
    if form in ("mod", "scaled"):
        a["x_scale"], d["x_scale"] = dv(o["s_c"]), o["s_c"]
    if form == "scaled":
        a["dy_scale"], d["dy_scale"] = dv(o["s_n"]), o["s_n"]
    if form == "stage":
        a.update(out_scale=0.5, accumulate_into=dv(o["acc"]).clone(), accumulate_bias_into=dv(o["acc_b"]).clone(), want_bias_sum=True)
        d.update(out_scale=0.5, acc=o["acc"], acc_b=o["acc_b"])
    if form == "bias":
        a["want_bias_sum"] = True
    got = hb.conv2d_bwd_weight(cl(o["x"], adt), cl(o["dy"], adt), (N, C, k, k), s, p, P, **a)
    ref = D.wgrad(o["x"], o["dy"], (N, C, k, k), s, p, **d, **kw)
    if form in ("bias", "stage"):
        dw, db = got
        if form == "bias" or row.get("bias_sum", False):
            assert db is not None, "this launch was expected to produce the bias sums"
        outs = [("dw", dw, ref.dw, ref.A)]
        if db is not None:
            outs.append(("db", a["accumulate_bias_into"] if db is True else db, ref.db, ref.A_db))
        return outs
    return [("dw", got, ref.dw, ref.A)]


def _s2d_operands(row, o, adt):
    B, C, N, H, W = row["shape"]
    wf2, wb2 = hb.pack_weight_s2d(dv(o["w"]))
    return cl(D.s2d(o["x"]), adt), wf2, wb2


def call_s2d_fwd(row, o, P, adt, kw):
    """All three forms of the stride-2 forward on one row: the same instantiation serves them."""
    B, C, N, H, W = row["shape"]
    x2, wf2, _ = _s2d_operands(row, o, adt)
    ws, bias = (N, 4 * C, 3, 3), dv(o["bias"])
    outs = []
    got = hb.conv2d_fwd(x2, None, 1, 1, P, bias=bias, packed=wf2, w_shape=ws, s2d_c=C)
    ref = D.s2d_forward(o["x"], o["w"], bias=o["bias"], **kw)
    outs.append(("bias", got, ref.y, ref.A))
    got = hb.conv2d_fwd(x2, None, 1, 1, P, bias=bias, residual=cl(o["res"], adt), res_scale=0.5, packed=wf2, w_shape=ws, s2d_c=C)
    ref = D.s2d_forward(o["x"], o["w"], bias=o["bias"], residual=o["res"], res_scale=0.5, **kw)
    outs.append(("residual", got, ref.y, ref.A))
    if row.get("merged", True):
        cr = o["xs"].shape[1]
        assert hb.s2d_res_supported(tuple(x2.shape), N, C, cr), "the one-launch block tail was expected to take this shape"
        got = hb.conv2d_s2d_res_fwd(x2, wf2, cl(o["xs"], adt), dv(o["w_res"]).to(adt), bias, N, C, 0.5)
        ref = D.s2d_forward(o["x"], o["w"], bias=o["bias"], second=(o["xs"], o["w_res"]), res_scale=0.5, **kw)
        outs.append(("merged", got, ref.y, ref.A))
    return outs


def call_s2d_dgrad(row, o, P, adt, kw):
    B, C, N, H, W = row["shape"]
    _, _, wb2 = _s2d_operands(row, o, adt)
    got = hb.conv2d_bwd_data(cl(o["dy"], adt), None, (B, 4 * C, H, W), 1, 1, P, packed=wb2, w_shape=(N, 4 * C, 3, 3), s2d_c=C)
    ref = D.s2d_dgrad(o["dy"], o["w"], **kw)
    return [("dx2", got, ref.y, ref.A)]


def call_s2d_wgrad(row, o, P, adt, kw):
    B, C, N, H, W = row["shape"]
    x2 = cl(D.s2d(o["x"]), adt)
    if row["form"] == "stage":
        got = hb.conv2d_bwd_weight_s2d(x2, cl(o["dy"], adt), (N, C, 3, 3), P, out_scale=0.5, accumulate_into=dv(o["acc"]).clone())
        ref = D.s2d_wgrad(o["x"], o["dy"], (N, C, 3, 3), out_scale=0.5, acc=o["acc"], **kw)
    else:
        got = hb.conv2d_bwd_weight_s2d(x2, cl(o["dy"], adt), (N, C, 3, 3), P)
        ref = D.s2d_wgrad(o["x"], o["dy"], (N, C, 3, 3), **kw)
    return [("dw", got, ref.dw, ref.A)]


def call_torgb_fwd(row, o, P, adt, kw):
    got = hb.torgb_fwd(cl(o["x"], adt), dv(o["s_c"]), dv(o["w"]))
    ref = D.torgb_fwd(o["x"], o["s_c"], o["w"], **kw)
    return [("y", got, ref.y, ref.A)]


def call_torgb_bwd(row, o, P, adt, kw):
    gy = torch.cat([o["dy"], torch.zeros_like(o["dy"][:, :1])], dim=1)
    gx, T = hb.torgb_bwd(cl(o["x"], adt), cl(gy, adt), dv(o["s_c"]), dv(o["w"]))
    ref = D.torgb_bwd(o["x"], gy, o["s_c"], o["w"], **kw)
    return [("gx", gx, ref.gx, ref.A_gx), ("T", T, ref.T, ref.A_T)]


CALLS = {"fwd": call_fwd, "dgrad": call_dgrad, "wgrad": call_wgrad, "s2d_fwd": call_s2d_fwd, "s2d_dgrad": call_s2d_dgrad,
         "s2d_wgrad": call_s2d_wgrad, "torgb_fwd": call_torgb_fwd, "torgb_bwd": call_torgb_bwd}
CLS = {"fwd": "fwd", "dgrad": "bwd_data", "wgrad": "bwd_weight", "s2d_fwd": "fwd", "s2d_dgrad": "bwd_data", "s2d_wgrad": "bwd_weight"}


def _operands(row, gaussian):
    B, C, N, H, W = row["shape"]
    call = row["call"]
    if call.startswith("s2d"):
        return D.operands(row["id"], B, C, N, 2 * H, 2 * W, 3, 2, 1, c_res=row.get("c_res", 8), gaussian=gaussian)
    if call.startswith("torgb"):
        return D.operands(row["id"], B, C, 3, H, W, 1, 1, 0, gaussian=gaussian)
    return D.operands(row["id"], B, C, N, H, W, row.get("k", 3), row.get("stride", 1), row.get("pad", 1), gaussian=gaussian)


def run_row(row, monkeypatch, gaussian):
    """-> (outputs of the first call with their references, the same of a second call, the (cls, kernel) pairs that ran)."""
    for name, value in row.get("env", {}).items():
        monkeypatch.setenv(name, value)
    _clear_shape_caches()
    prec = row.get("prec", "bf16")
    ops.set_precision(prec)
    P = hb.BF16_ACT if prec == "bf16" else hb.F32
    adt = hb.act_dtype(P)
    o = _operands(row, gaussian)
    kw = dict(dt=torch.float64, exact=False) if gaussian else {}
    fn = CALLS[row["call"]]
    hb.timing_enable(1)
    try:
        first = fn(row, o, P, adt, kw)
        second = fn(row, o, P, adt, kw)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "illegal memory" in str(e) or "hipError" in str(e) or "HIP error" in str(e):
            pytest.exit("GPU fault in row %s: %s" % (row["id"], e), returncode=3)  # nothing more runs on a faulted device
        raise
    ran = {(r["cls"], r["kernel"]) for r in hb.timing_kernels() if r["kernel"]}
    return first, second, ran, prec


# ---- the table ---------------------------------------------------------------------------------------------------------
def R(id, call, shape, form, kernel, env=None, gauss=False, **kw):
    return dict(id=id, call=call, shape=shape, form=form, kernel=kernel, env=env or {}, gauss=gauss, **kw)


PIPE6, PIPE0, LINE0 = {"STYLEX_CONV_PIPE": "6"}, {"STYLEX_CONV_PIPE": "0"}, {"STYLEX_CONV_LINE64": "0"}
HALO = "conv3x3_halo_bf16_kernel<%s>"
PIPE, DMA, LINE = "conv3x3_pipe_kernel<%s>", "conv3x3_halo_dma_kernel<%s>", "conv3x3_line64_kernel<%s>"
GATHER, RGB = "conv_gather_line_kernel", "conv3x3_rgb_kernel"
SF, SD, WGP = "conv_s2d_fwd_kernel<%s>", "conv_s2d_dgrad_kernel<%s>", "conv3x3_wgrad_pipe_kernel<%s>"
TR, TRDMA, WG, IG = "conv_wgrad_tr_kernel<%s>", "conv_wgrad_tr_dma_kernel", "conv_wgrad_kernel<%s>", "conv_igemm_kernel<%s>"
NP1, NP2 = {"STYLEX_WGRAD_PIPE_NP": "1"}, {"STYLEX_WGRAD_PIPE_NP": "2"}


def _pipe_rows():
    rows = []
    # <128, *>: one whole tile; ragged rows and columns with a 32-channel tail chunk; 32 chunks; 272 tiles on 256 blocks (a
    # block walks several tiles across the ring boundary; ragged rows)
    for tag, shape in (("one-tile", (1, 64, 128, 16, 32)), ("ragged", (1, 96, 128, 24, 40)), ("32-chunks", (1, 512, 128, 16, 32)),
                       ("272-tiles", (1, 64, 128, 264, 512))):
        dev = tag == "272-tiles"
        rows.append(R("pipe128-fwd-" + tag, "fwd", shape, "bias-lrelu-mask", PIPE % "128, 0", gauss=tag == "ragged", ref_dev=dev))
        B, C, N, H, W = shape
        dshape = (B, N, C, H, W)  # the data gradient INTO 128 channels
        if tag != "272-tiles":
            rows.append(R("pipe128-dgrad-" + tag, "dgrad", dshape, "plain", PIPE % "128, 0"))
            rows.append(R("pipe128-dgrad-gate-" + tag, "dgrad", dshape, "gate", PIPE % "128, 1", gauss=tag == "ragged"))
        rows.append(R("pipe128-dgrad-mask-" + tag, "dgrad", dshape, "mask", PIPE % "128, 2", ref_dev=dev))
    # <64, *>: 32 x 32 pixel tiles, Ho >= 32
    rows.append(R("pipe64-fwd", "fwd", (1, 64, 64, 32, 32), "bias-lrelu-mask", PIPE % "64, 0"))
    rows.append(R("pipe64-fwd-ragged", "fwd", (2, 96, 64, 40, 72), "bias-relu", PIPE % "64, 0"))
    rows.append(R("pipe64-dgrad-128to64", "dgrad", (1, 64, 128, 32, 32), "plain", PIPE % "64, 0"))
    rows.append(R("pipe64-dgrad-64to64", "dgrad", (1, 64, 64, 32, 32), "plain", PIPE % "64, 0", env=PIPE6))
    rows.append(R("pipe64-dgrad-mask", "dgrad", (2, 64, 64, 40, 72), "mask", PIPE % "64, 2", env=PIPE6))
    return rows


def _dma_line_rows():
    rows = [
        R("dma1-dgrad-64to8", "dgrad", (2, 8, 64, 16, 32), "plain", DMA % "1, false", gauss=True),
        R("dma1-dgrad-64to8-ragged", "dgrad", (1, 8, 64, 24, 40), "plain", DMA % "1, false"),
        R("dma2-fwd", "fwd", (1, 64, 64, 16, 32), "bias-lrelu-mask", DMA % "2, false", env=PIPE0),
        R("dma2-fwd-ragged", "fwd", (1, 136, 64, 20, 40), "bias-relu", DMA % "2, false", env=PIPE0),
        R("dma2-dgrad-gate", "dgrad", (1, 64, 128, 24, 64), "gate", DMA % "2, false", env=PIPE0),
        R("dma2-dgrad-mask", "dgrad", (1, 64, 128, 24, 64), "mask", DMA % "2, false", env=PIPE0),
        R("dma4-fwd-n160", "fwd", (1, 128, 160, 16, 40), "bias-lrelu-mask", DMA % "4, false", gauss=True),
        R("dma4-dgrad-n160", "dgrad", (1, 160, 128, 16, 32), "gate", DMA % "4, false"),
        R("dma2s2d-fwd", "s2d_fwd", (1, 64, 64, 16, 32), "all", DMA % "2, true", env={"STYLEX_S2D_FWD": "0"}, merged=False),
        R("dma2s2d-dgrad", "s2d_dgrad", (1, 64, 64, 16, 32), "plain", DMA % "2, true", env={"STYLEX_S2D_DGRAD": "0"}),
    ]
    for tag, shape in (("128sq", (1, 64, 64, 128, 128)), ("64x256", (1, 64, 64, 64, 256))):
        rows.append(R("line64-fwd-" + tag, "fwd", shape, "bias-lrelu-mask", LINE % "0", gauss=tag == "64x256"))
        rows.append(R("line64-dgrad-" + tag, "dgrad", shape, "plain", LINE % "0"))
        rows.append(R("line64-dgrad-mask-" + tag, "dgrad", shape, "mask", LINE % "2", gauss=tag == "64x256"))
    return rows


def _small_rows():
    rows = []
    for shape in ((5, 128, 192, 8, 8), (3, 64, 64, 4, 4), (5, 64, 72, 2, 2)):
        tag = "%dpx-%dx%dx%d" % (shape[3], shape[0], shape[1], shape[2])
        rows.append(R("gather-fwd-" + tag, "fwd", shape, "bias-lrelu", GATHER, gauss=shape[3] == 8))
        B, C, N, H, W = shape
        if N % 64 == 0:
            rows.append(R("gather-dgrad-" + tag, "dgrad", (B, N, C, H, W), "plain", GATHER))
            rows.append(R("gather-dgrad-gate-" + tag, "dgrad", (B, N, C, H, W), "gate", GATHER))
    rows.append(R("gather-fwd-1x1", "fwd", (5, 128, 192, 8, 8), "bias-lrelu", GATHER, k=1, pad=0))
    rows.append(R("gather-dgrad-1x1", "dgrad", (5, 192, 128, 8, 8), "plain", GATHER, k=1, pad=0))
    rows.append(R("gather-fwd-stride2", "fwd", (3, 64, 64, 4, 12), "bias-res", GATHER, stride=2))
    rows.append(R("gather-dgrad-stride2", "dgrad", (3, 64, 64, 4, 12), "plain", GATHER, stride=2, gauss=True))
    rows.append(R("rgb-fwd", "fwd", (2, 8, 64, 40, 72), "rgb-mask", RGB, gauss=True))
    return rows


def _halo_rows():
    """The register-staged kernel: the modulated generator convs (per-sample scales, noise plane in both orders) and their scaled
    data gradients, 16- and 32-wide tiles, the smallest image (12 x 13) and a 15 x 15 partial tile."""
    rows = []
    for tag, shape, tw in (("12x13", (2, 64, 64, 12, 13), 16), ("15x15", (1, 192, 64, 15, 15), 16), ("16x32", (2, 64, 64, 16, 32), 32),
                           ("24x40", (1, 40, 96, 24, 40), 32)):
        B, C, N, H, W = shape
        rows.append(R("halo-fwd-plain-" + tag, "fwd", shape, "mod", HALO % ("%d, 2, true, false, false" % tw)))
        rows.append(R("halo-fwd-noise-" + tag, "fwd", shape, "mod-noise", HALO % ("%d, 2, true, false, true" % tw), gauss=tag == "24x40"))
        rows.append(R("halo-fwd-noise-nat-" + tag, "fwd", shape, "mod-noise-nat", HALO % ("%d, 2, true, false, true" % tw)))
        rows.append(R("halo-fwd-full-" + tag, "fwd", shape, "full", HALO % ("%d, 2, true, false, true" % tw)))
        rows.append(R("halo-dgrad-scaled-" + tag, "dgrad", (B, N, C, H, W), "scaled", HALO % ("%d, 2, true, false, false" % tw),
                      gauss=tag == "12x13"))
        rows.append(R("halo-dgrad-scaled-gate-" + tag, "dgrad", (B, N, C, H, W), "scaled-gate", HALO % ("%d, 2, true, false, true" % tw)))
    rows.append(R("halo-fwd-12x13-unscaled", "fwd", (2, 64, 64, 12, 13), "bias-lrelu", HALO % "16, 2, true, false, false"))
    rows.append(R("halo-dgrad-12x13-unscaled", "dgrad", (2, 64, 64, 12, 13), "plain", HALO % "16, 2, true, false, false"))
    rows.append(R("halo-dgrad-12x13-gate", "dgrad", (2, 64, 64, 12, 13), "gate", HALO % "16, 2, true, false, true"))
    # one 32-channel output sub-tile: the generator's last block (64 -> 32 -> 32)
    rows.append(R("halo-fwd-noise-n32", "fwd", (2, 64, 32, 16, 32), "mod-noise", HALO % "32, 1, true, false, true"))
    rows.append(R("halo-fwd-noise-nat-n32", "fwd", (2, 32, 32, 24, 40), "mod-noise-nat", HALO % "32, 1, true, false, true"))
    rows.append(R("halo-dgrad-scaled-n32", "dgrad", (2, 32, 64, 16, 32), "scaled", HALO % "32, 1, true, false, false"))
    rows.append(R("halo-fwd-n32-12x13", "fwd", (2, 64, 32, 12, 13), "bias-lrelu", HALO % "16, 1, true, false, false"))
    rows.append(R("halo-fwd-noise-n32-12x13", "fwd", (2, 64, 32, 12, 13), "mod-noise", HALO % "16, 1, true, false, true"))
    return rows


def _s2d_rows():
    rows = []
    # (B, C_res, C = N, half-res H, W) of test_s2d_forward_pipelined_kernel, B <= 3
    for (B, CR, C, H, W), tile, inst in (((3, 64, 128, 24, 64), "0", "32, 128, 8, 2"), ((3, 64, 128, 24, 64), "2", "32, 128, 4, 4"),
                                         ((1, 128, 256, 32, 32), "0", "32, 128, 8, 2"), ((1, 128, 256, 32, 32), "1", "32, 256, 8, 4"),
                                         ((3, 32, 256, 16, 16), "0", "16, 128, 8, 2"), ((3, 32, 256, 16, 16), "2", "16, 128, 4, 4"),
                                         ((3, 32, 256, 16, 16), "1", "16, 256, 8, 4"), ((3, 8, 64, 16, 64), "0", "32, 64, 4, 2"),
                                         ((2, 40, 64, 16, 16), "0", "16, 64, 4, 2"), ((1, 64, 128, 16, 32), "1", "32, 128, 8, 4")):
        rows.append(R("s2d-fwd-%dx%dx%dx%d-tile%s" % (B, C, H, W, tile), "s2d_fwd", (B, C, C, H, W), "all", SF % inst,
                      env={"STYLEX_S2D_FWD_TILE": tile}, c_res=CR, gauss=(C, tile) == (128, "2")))
    # (B, C, N, half-res H, W) of test_s2d_data_gradient_all_subpositions_kernel
    for shape in ((3, 64, 64, 24, 64), (1, 128, 128, 32, 32), (2, 64, 256, 8, 96), (3, 192, 64, 16, 32), (3, 128, 128, 16, 16),
                  (1, 64, 64, 32, 48)):
        tw = 32 if shape[4] % 32 == 0 and shape[3] % 8 == 0 else 16
        for tile, nw in (("0", 4), ("1", 8)):
            rows.append(R("s2d-dgrad-%s-tile%s" % ("x".join(map(str, shape)), tile), "s2d_dgrad", shape, "plain", SD % ("%d, %d" % (tw, nw)),
                          env={"STYLEX_S2D_DGRAD_TILE": tile}, gauss=(shape[0], tile) == (2, "0")))
    return rows


def _wgrad_rows():
    rows = []
    for env, np_ in ((NP1, 1), (NP2, 2)):
        for shape, form in (((3, 128, 128, 32, 32), "plain"), ((3, 128, 128, 32, 32), "bias"), ((2, 64, 256, 16, 16), "bias"),
                            ((5, 192, 128, 8, 16), "plain"), ((4, 64, 128, 32, 32), "mod"), ((6, 128, 128, 16, 16), "mod"),
                            ((2, 64, 256, 16, 16), "stage")):
            tw = 32 if shape[4] >= 32 else 16
            inst = "%d, %d, %s, false" % (np_, tw, "true" if form in ("bias", "stage") else "false")
            rows.append(R("wgpipe-np%d-%s-%s" % (np_, "x".join(map(str, shape)), form), "wgrad", shape, form, WGP % inst, env=env,
                          bias_sum=True, gauss=(np_, form, tw) == (2, "bias", 32)))
        for shape, form in (((2, 64, 128, 32, 32), "plain"), ((3, 128, 128, 16, 16), "plain"), ((1, 64, 256, 8, 32), "stage")):
            tw = 32 if shape[4] >= 32 else 16
            rows.append(R("wgpipe-np%d-s2d-%s-%s" % (np_, "x".join(map(str, shape)), form), "s2d_wgrad", shape, form,
                          WGP % ("%d, %d, false, true" % (np_, tw)), env=env, gauss=(np_, tw, form) == (1, 32, "plain")))
    # 40 tiles of 8 per image on 16 output tiles (256 CUs): 3 tiles per split, so splits end inside an image and run on into
    # the next; with x_scale the plan takes 2, the largest divisor of 8: every split ends on an image boundary or inside one image
    rows.append(R("wgpipe-split-inside-image", "wgrad", (5, 256, 256, 32, 32), "plain", WGP % "1, 32, false, false", env=NP1))
    rows.append(R("wgpipe-split-on-image-boundary", "wgrad", (5, 256, 256, 32, 32), "mod", WGP % "1, 32, false, false", env=NP1))
    # exactly 32 channels on either side (the generator's last block): half-filled 64-channel tiles
    rows.append(R("wgpipe-32to32-mod", "wgrad", (2, 32, 32, 32, 32), "mod", WGP % "1, 32, false, false"))
    rows.append(R("wgpipe-64to32-mod", "wgrad", (2, 64, 32, 16, 16), "mod", WGP % "1, 16, false, false"))
    rows.append(R("wgpipe-32to64-bias", "wgrad", (3, 32, 64, 32, 32), "bias", WGP % "1, 32, true, false", bias_sum=True))
    # the selector's own choice (>= 48 stages per block -> the 128-channel tile) is left to the benchmark step's shapes
    for shape, k, s, p in (((4, 128, 128, 8, 8), 3, 1, 1), ((3, 256, 128, 16, 16), 3, 2, 1), ((2, 128, 256, 32, 32), 1, 1, 0),
                           ((3, 128, 128, 2, 2), 3, 1, 1), ((5, 128, 128, 4, 8), 3, 1, 1)):
        rows.append(R("wgtrdma-%s-k%ds%d" % ("x".join(map(str, shape)), k, s), "wgrad", shape, "plain", TRDMA, k=k, stride=s, pad=p,
                      gauss=shape[0] == 5))
    rows.append(R("wgtr-64x64-8px", "wgrad", (2, 64, 64, 8, 8), "scaled", TR % "1, 1, false", gauss=True))
    rows.append(R("wgtr-40x72-ragged", "wgrad", (2, 40, 72, 10, 10), "plain", TR % "1, 1, false"))
    rows.append(R("wgtr-rgb-slot", "wgrad", (2, 8, 64, 16, 32), "plain", TR % "1, 2, true"))
    rows.append(R("wgtr-256x136", "wgrad", (2, 256, 136, 8, 8), "scaled", TR % "2, 2, false"))
    rows.append(R("wgtr-1x1-stride2", "wgrad", (2, 64, 128, 16, 16), "stage", TR % "1, 1, false", k=1, stride=2, pad=0))
    return rows


def _generic_rows():
    """conv_igemm_kernel / conv_wgrad_kernel on the small cases of CONV_CASES (odd sizes, C % 4 != 0, 1x1 stride 2, 5x5), in the
    fp32 and the bf16 precision."""
    rows = []
    for tag, shape, k, s, p in (("odd", (3, 6, 10, 9, 7), 3, 1, 1), ("1x1s2", (2, 8, 12, 8, 8), 1, 2, 0), ("5x5", (1, 8, 12, 9, 7), 5, 1, 2),
                                ("16to24", (2, 16, 24, 8, 8), 3, 1, 1), ("ragged", (2, 40, 72, 10, 10), 3, 1, 1),
                                ("128to160", (1, 128, 160, 12, 12), 3, 1, 1), ("s2-odd", (3, 72, 64, 5, 7), 3, 2, 1)):
        for prec in ("fp32", "bf16"):
            if (tag, prec) == ("128to160", "bf16"):
                continue  # 12 x 12 at C % 8 == 0: the register-staged halo kernel's shape in bf16
            kw = dict(prec=prec, k=k, stride=s, pad=p)
            name = IGEMM_OF[tag, prec]
            rows.append(R("igemm-fwd-%s-%s" % (tag, prec), "fwd", shape, "full", IG % name[0], gauss=(tag, prec) == ("ragged", "bf16"), **kw))
            rows.append(R("igemm-dgrad-%s-%s" % (tag, prec), "dgrad", shape, "scaled-gate", IG % name[1], **kw))
            rows.append(R("generic-wgrad-%s-%s" % (tag, prec), "wgrad", shape, "scaled", WGRAD_OF[tag, prec], gauss=(tag, prec) == ("odd", "fp32"), **kw))
    # 4096 rows on at most 256 tiles of 128 x 128 (the 8 x 8 px layers at B = 64 without the gather kernel): the 64 x 64 tile
    rows.append(R("igemm-small-tile", "fwd", (64, 128, 128, 8, 8), "bias-lrelu", IG % "2, 2, 1, 1, true, true, 64, true",
                  env={"STYLEX_CONV_GATHER": "0"}))
    return rows


# The instantiations of the generic kernels per (case, precision): (forward, data gradient); weight gradient.  dispatch_igemm
# picks the tile by the output-channel count of the launch (<= 32: <4, 1, 2, 1>, <= 64: <4, 1, 2, 2>, else <2, 2, 2, 2>), VEC4 by
# C % 4 == 0, then the operand type, the K tile and the bf16 activation flag; the bf16 weight gradient of 8-channel-aligned
# shapes belongs to conv_wgrad_tr.hip.
_F32V, _F32S = "true, false, 32, false", "false, false, 32, false"
IGEMM_OF = {
    ("odd", "fp32"): ("4, 1, 2, 1, " + _F32S, "4, 1, 2, 1, " + _F32S),
    ("odd", "bf16"): ("4, 1, 2, 1, false, true, 32, false", "4, 1, 2, 1, false, true, 32, false"),
    ("1x1s2", "fp32"): ("4, 1, 2, 1, " + _F32V, "4, 1, 2, 1, " + _F32V),
    ("1x1s2", "bf16"): ("4, 1, 2, 1, true, true, 32, true", "4, 1, 2, 1, true, true, 32, false"),
    ("5x5", "fp32"): ("4, 1, 2, 1, " + _F32V, "4, 1, 2, 1, " + _F32V),
    ("5x5", "bf16"): ("4, 1, 2, 1, true, true, 32, true", "4, 1, 2, 1, true, true, 32, false"),
    ("16to24", "fp32"): ("4, 1, 2, 1, " + _F32V, "4, 1, 2, 1, " + _F32V),
    ("16to24", "bf16"): ("4, 1, 2, 1, true, true, 32, true", "4, 1, 2, 1, true, true, 32, true"),
    ("ragged", "fp32"): ("2, 2, 2, 2, " + _F32V, "4, 1, 2, 2, " + _F32V),
    ("ragged", "bf16"): ("2, 2, 2, 2, true, true, 64, true", "4, 1, 2, 2, true, true, 32, true"),
    ("128to160", "fp32"): ("2, 2, 2, 2, " + _F32V, "2, 2, 2, 2, " + _F32V),
    ("s2-odd", "fp32"): ("4, 1, 2, 2, " + _F32V, "2, 2, 2, 2, " + _F32V),
    ("s2-odd", "bf16"): ("4, 1, 2, 2, true, true, 32, true", "2, 2, 2, 2, true, true, 64, true"),
}
WGRAD_OF = {
    ("odd", "fp32"): WG % "1, 1, false, false", ("odd", "bf16"): WG % "1, 1, false, true",
    ("1x1s2", "fp32"): WG % "1, 1, true, false", ("1x1s2", "bf16"): WG % "1, 1, true, true",
    ("5x5", "fp32"): WG % "1, 1, true, false", ("5x5", "bf16"): WG % "1, 1, true, true",
    ("16to24", "fp32"): WG % "1, 1, true, false", ("16to24", "bf16"): TR % "1, 1, false",
    ("ragged", "fp32"): WG % "1, 1, true, false", ("ragged", "bf16"): TR % "1, 1, false",
    ("128to160", "fp32"): WG % "2, 2, true, false",
    ("s2-odd", "fp32"): WG % "1, 1, true, false", ("s2-odd", "bf16"): TR % "1, 1, false",
}

ROWS = _pipe_rows() + _dma_line_rows() + _small_rows() + _halo_rows() + _s2d_rows() + _wgrad_rows() + _generic_rows()
for shape in ((3, 32, 3, 20, 12), (2, 512, 3, 4, 4), (2, 64, 3, 33, 7), (2, 8, 3, 16, 16), (1, 128, 3, 64, 64), (2, 256, 3, 40, 40)):
    tag = "x".join(map(str, (shape[0], shape[1], shape[3], shape[4])))
    ROWS.append(R("torgb-fwd-" + tag, "torgb_fwd", shape, "plain", None, gauss=shape[1] == 64))
    ROWS.append(R("torgb-bwd-" + tag, "torgb_bwd", shape, "plain", None, gauss=shape[1] == 64))
assert len({r["id"] for r in ROWS}) == len(ROWS)
GAUSS = [r for r in ROWS if r["gauss"]]


def _expected(row):
    return (CLS[row["call"]], row["kernel"]) if row["kernel"] else None


@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_exact(row, monkeypatch):
    first, second, ran, prec = run_row(row, monkeypatch, gaussian=False)
    want_kernel = _expected(row)
    _LINES.append("exact %-52s %s" % (row["id"], ", ".join("%s %s" % k for k in sorted(ran)) or "(no conv launch noted)"))
    if row["call"].startswith("torgb"):
        assert not ran  # the streaming to-RGB kernels are no conv launches: nothing to name
    else:
        assert want_kernel in ran, "row written for %s, the launch ran %s" % (want_kernel, sorted(ran))
    for (name, got, want, _), (_, again, _, _) in zip(first, second):
        if name == "mask":
            y = first[0][1]
            assert torch.equal(got.cpu(), D.pack_mask(y.float().cpu())), "mask is not the sign of the stored output"
        else:
            ref = D.store(want, prec if got.dtype == torch.bfloat16 else "fp32")
            g = got.detach().cpu()
            assert g.shape == ref.shape and g.dtype == ref.dtype, (name, g.shape, ref.shape, g.dtype, ref.dtype)
            if not torch.equal(g, ref):
                bad = (g.float() != ref.float()) | torch.isnan(g.float())
                idx = torch.nonzero(bad)
                raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r; max |diff| %g; per dim ranges %s" % (
                    name, int(bad.sum()), bad.numel(), idx[0].tolist(), float(g[tuple(idx[0])]), float(ref[tuple(idx[0])]),
                    float((g.float() - ref.float()).abs().max()), [(int(idx[:, d].min()), int(idx[:, d].max())) for d in range(idx.shape[1])]))
        assert torch.equal(got, again), "%s: the second call differs" % name
    for key in ran:
        EXACT_KERNELS.setdefault(key, set()).add(row["id"])


@pytest.mark.parametrize("row", GAUSS, ids=[r["id"] for r in GAUSS])
def test_gauss(row, monkeypatch):
    first, second, ran, prec = run_row(row, monkeypatch, gaussian=True)
    if not row["call"].startswith("torgb"):
        assert _expected(row) in ran, (row["kernel"], sorted(ran))
    worst, what, share = 0.0, "", 0.0
    for (name, got, want, A), (_, again, _, _) in zip(first, second):
        assert torch.equal(got, again), "%s: the second call differs" % name
        if name == "mask":
            assert torch.equal(got.cpu(), D.pack_mask(first[0][1].float().cpu())), "mask is not the sign of the stored output"
            continue
        g = got.detach().double().cpu()
        assert torch.isfinite(g).all(), name
        r = 1.0 if got.dtype == torch.bfloat16 else 0.0
        bound = r * 2.0 ** -8 * want.abs() + TOL32 * A
        err = (g - want).abs()  # (where the bound is zero — the zero fourth to-RGB channel — the result must be exact)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
        i = int(ratio.argmax())
        if float(ratio.view(-1)[i]) >= worst:
            worst, what = float(ratio.view(-1)[i]), name
            share = float((TOL32 * A).view(-1)[i] / bound.view(-1)[i]) if float(bound.view(-1)[i]) > 0 else 0.0
    _LINES.append("gauss %-52s %8.4f  %-8s fp32 term %.3f of the bound there" % (row["id"], worst, what, share))
    print("gauss %s: worst error / bound %.4f (%s)" % (row["id"], worst, what))
    assert worst <= 1.0, "%s: error / bound = %.4g" % (what, worst)
