"""The float64 definitions of tests/_param_defs.py (Adam and the operand copies, the style coefficients, the initial block),
the inputs, chain counts and limits that tests/test_param_kernels_gpu.py holds the kernels to, and an fp32 model of each
kernel's pass structure.  Runs without a GPU.

1. Each definition against an independent float64 computation (about 1e-12): torch.optim.Adam on float64 tensors over three
   steps from a non-zero step count; autograd of the ATen composition of the style coefficients; autograd of
   F.conv_transpose2d on the layer mean; the space-to-depth weight through F.conv2d; the copy layouts index by index.
2. The fp32 models (same summation order, fma where the kernel has fmaf, the explicitly rounded operations of adam_update)
   lie inside the GAUSS limits and match the EXACT class on the very inputs the GPU test uses.
3. Mutations of the models land OUTSIDE the limits on those inputs: the bounds bite.
4. The preconditions of the EXACT class are asserted from abs_terms (every sum, in units of its granule, below 2^24).

The chain counts N (fp32 roundings on the longest path of a term, counted without contraction) are derived in the docstring
of tests/test_param_kernels_gpu.py; nothing here is tuned against a kernel."""
import collections
import math

import pytest
import torch
import torch.nn.functional as F

import _param_defs as P
from test_linattn_defs_cpu import DT, EW, PRECS, U, equal_exact, gen, limit, worst  # noqa: F401

F32, F64 = torch.float32, torch.float64
ULP_RSQRT = 4  # rsqrtf: 2 ulp (OpenCL full profile), an ulp being at most 2^-23 of the value: 4 in units of 2^-24
N_M, N_V, N_P = 3, 4, 13


def t32(x):
    return torch.tensor(x, dtype=F32)


def fma(a, b, c):
    """fmaf on fp32 tensors: the double product of two floats is exact; one rounding of the sum to double, one to float."""
    return (a.double() * b.double() + c.double()).float()


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ================================================================ Adam and the copies =========================================
Tensor = collections.namedtuple("Tensor", "shape group copies")  # copies: (kind, scale) in registration order
C2 = 1 / 2 ** 0.5
ADAM_TENSORS = {
    # flat tensors: 4608 elements per block, float4 for a whole block of an aligned tensor, scalar otherwise
    "flat4608": Tensor((4608,), 0, ()),                 # exactly one whole block
    "flat9221": Tensor((9221,), 1, ()),                 # two whole blocks and a tail of 5
    "flat1": Tensor((1,), 0, ()),
    "linear": Tensor((17, 33), 1, ()),                  # a matrix without copies is flat
    # slab weights [N][C][T]: 8 x 64 x T per block
    "w16x64x9": Tensor((16, 64, 3, 3), 0, (("pack", None), ("pack_b", C2), ("s2d", None), ("s2d", C2))),  # float4 rows; even_c, full_n
    "w16x130x9": Tensor((16, 130, 3, 3), 1, (("pack", None), ("wsq", None), ("s2d", None))),   # C T % 4 != 0; ragged slab of 2
    "w12x33x9": Tensor((12, 33, 3, 3), 0, (("pack", None), ("wsq", None), ("s2d", None))),     # N % 8 != 0, odd C: !even_c, !full_n
    "w8x75x9": Tensor((8, 75, 3, 3), 1, (("pack", None), ("s2d", None))),                       # ragged odd slab: !even_c, full_n
    "w4x6x9": Tensor((4, 6, 3, 3), 0, (("pack", None), ("s2d", C2))),                           # N < 8: even_c, !full_n
    "w5x7x4": Tensor((5, 7, 2, 2), 1, (("pack", None), ("wsq", None))),                         # T = 4, float4 rows of 28, N < 8
    "w24x40x1": Tensor((24, 40, 1, 1), 0, (("pack", None), ("bf16mat", None), ("bf16mat", C2))),  # T = 1
    "initw18x24": Tensor((18, 24, 4, 4), 1, (("initw", None),)),                                # [18][384]: 6 slabs, rows 8 + 8 + 2
    "initw3x512": Tensor((3, 512, 4, 4), 0, (("initw", None),)),                                # [3][8192]: 128 slabs per row group
    "five": Tensor((8, 64, 3, 3), 1, (("pack", None), ("pack_b", C2), ("s2d", None), ("s2d", C2), ("wsq", None))),  # one copy too many
}
ADAM_GROUPS = [dict(lr=2e-4, betas=(0.5, 0.9), eps=1e-8), dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6)]
ADAM_CALLS = [(2, 1.0), (3, 0.5), (10001, 0.25)]  # (step count after the increment, factor on each group's lr)


def decades(g, shape):
    """randn times 10^u, u uniform in [-4, 4]: eight decades in one tensor."""
    return torch.randn(shape, generator=g) * 10.0 ** (torch.rand(shape, generator=g) * 8 - 4)


def adam_inputs(name, call):
    """(p, g, m, v) fp32.  Planted: element 0 g = 0; 1 m = v = 0; 2 v = 0 with m != 0; 3 v = 0, g = 0, m != 0 (the update is
    step_size * b1 * m / eps).  The one-element tensor takes plant 1, 0, 3 in the three calls."""
    shape = ADAM_TENSORS[name].shape
    g = gen("adam", name, call)
    p, gr, m = decades(g, shape), decades(g, shape), decades(g, shape)
    v = decades(g, shape) ** 2
    n = p.numel()
    for i in ([0, 1, 2, 3] if n >= 4 else [(1, 0, 3)[call]]):
        j = min(i, n - 1)
        if i in (0, 3):
            gr.view(-1)[j] = 0
        if i == 1:
            m.view(-1)[j] = 0
        if i in (1, 2, 3):
            v.view(-1)[j] = 0
    return p, gr, m, v


def adam_hyper(name, call):
    grp = ADAM_GROUPS[ADAM_TENSORS[name].group]
    step, f = ADAM_CALLS[call]
    return dict(step=step, lr=grp["lr"] * f, b1=grp["betas"][0], b2=grp["betas"][1], eps=grp["eps"])


def adam_ratios(want, p, m, v):
    """error / limit of the three results of one step against P.adam(...)"""
    out = {}
    for name, got, w, n in (("p", p, want.p, N_P), ("exp_avg", m, want.m, N_M), ("exp_avg_sq", v, want.v, N_V)):
        assert got.dtype == F32
        out[name] = worst(got.cpu(), w.value, limit(w, n, "fp32"))
    return out


def model_adam(p, g, m, v, step, lr, b1, b2, eps, mut=None):
    """adam_update of csrc/adam_pack.hip, operation by operation."""
    if mut == "swap_betas":
        b1, b2 = b2, b1
    ss, bc2 = t32(lr / (1 - b1 ** step)), t32(1.0 if mut == "no_bc2" else math.sqrt(1 - b2 ** step))
    B1, B2, E, one = t32(b1), t32(b2), t32(eps), t32(1.0)
    m1 = fma(B1, m, (one - B1) * g)
    v1 = fma(B2, v, ((one - B2) * g) * g)
    denom = torch.sqrt(v1 + E) / bc2 if mut == "eps_in_sqrt" else torch.sqrt(v1) / bc2 + E
    return p - (ss * m1) / denom, m1, v1


def copy_definitions(kind, w32, scale):
    """(a, b) of one registered copy, from the fp32 parameter: what the cache entry's value must hold."""
    if kind == "pack":
        return P.pack_fwd(w32, scale), P.pack_bwd(w32, scale)
    if kind == "pack_b":
        return None, P.pack_bwd(w32, scale)
    if kind == "s2d":
        return P.s2d_pack_fwd(w32, scale), P.s2d_pack_bwd(w32, scale)
    if kind in ("bf16mat", "initw"):
        return P.matrix(w32, scale), None
    raise KeyError(kind)


def wsq_n(taps):
    return taps + 1  # the square, then `taps` additions


def model_wsq(w, fused, mut=None):
    """The tap sum of squares: fmaf chain (wsq_kernel) or product and addition (the Adam launch's refresh)."""
    o, c = w.shape[:2]
    wt = w.reshape(o, c, -1)
    acc = torch.zeros(o, c)
    for k in range(wt.shape[2] - (1 if mut == "drop_tap" else 0)):
        acc = fma(wt[:, :, k], wt[:, :, k], acc) if fused else acc + wt[:, :, k] * wt[:, :, k]
    return acc


def model_pack_fwd(w32, scale, mut=None):
    n, c = w32.shape[:2]
    s = w32 if scale is None else w32 * t32(scale)
    s = s.reshape(n, c, -1)
    return (s if mut == "swap_tc" else s.permute(0, 2, 1)).contiguous().bfloat16().reshape(n, -1, c)


def test_adam_definition_is_torch_adam_in_float64():
    for grp in ADAM_GROUPS:
        g = gen("adam64", grp["lr"])
        p = torch.nn.Parameter(torch.randn(300, generator=g, dtype=F64))
        opt = torch.optim.Adam([p], lr=grp["lr"], betas=grp["betas"], eps=grp["eps"])
        m, v = torch.randn(300, generator=g, dtype=F64), torch.rand(300, generator=g, dtype=F64)
        opt.state[p] = {"step": torch.tensor(5.0), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        mine = (p.detach().clone(), m, v)
        for k in range(3):
            grad = torch.randn(300, generator=g, dtype=F64) * 10.0 ** k
            p.grad = grad.clone()
            opt.step()
            r = P.adam(mine[0], grad, mine[1], mine[2], 6 + k, grp["lr"], *grp["betas"], grp["eps"])
            mine = (r.p.value, r.m.value, r.v.value)
            st = opt.state[p]
            assert float(st["step"]) == 6 + k
            assert rel(mine[0], p.detach()) < 1e-12 and rel(mine[1], st["exp_avg"]) < 1e-12 and rel(mine[2], st["exp_avg_sq"]) < 1e-12


def test_space_to_depth_weight_is_the_stride_two_convolution():
    g = gen("s2d")
    x, w = torch.randn(2, 5, 8, 6, generator=g, dtype=F64), torch.randn(7, 5, 3, 3, generator=g, dtype=F64)
    want = F.conv2d(x, w, stride=2, padding=1)
    got = F.conv2d(P.space_to_depth(x), P.s2d_weight(w), padding=1)
    assert got.shape == want.shape and rel(got, want) < 1e-12
    assert int((P.s2d_weight(torch.ones(1, 1, 3, 3)) != 0).sum()) == 9  # every tap placed once, 27 zeros


def test_copy_layouts_index_by_index():
    w = torch.randn(3, 5, 2, 2, generator=gen("layout"))
    f, b, mt = P.pack_fwd(w, C2), P.pack_bwd(w, C2), P.matrix(w)
    for n in range(3):
        for c in range(5):
            for t in range(4):
                e = (t32(C2) * w[n, c, t // 2, t % 2]).bfloat16()
                assert f[n, t, c] == e and b[c, t, n] == e and mt[n, c * 4 + t] == w[n, c, t // 2, t % 2].bfloat16()
    assert tuple(f.shape) == (3, 4, 5) and tuple(b.shape) == (5, 4, 3) and tuple(mt.shape) == (3, 20)
    w9 = torch.randn(3, 5, 3, 3, generator=gen("layout9"))
    assert tuple(P.s2d_pack_fwd(w9).shape) == (3, 9, 20) and tuple(P.s2d_pack_bwd(w9).shape) == (20, 9, 3)
    assert torch.equal(model_pack_fwd(w, C2), f)
    assert not torch.equal(model_pack_fwd(w, C2, mut="swap_tc"), f), "mutation: T and C exchanged"
    assert rel(P.wsq(w).value, w.double().pow(2).sum(dim=(2, 3))) < 1e-15


@pytest.mark.parametrize("call", range(len(ADAM_CALLS)))
@pytest.mark.parametrize("name", list(ADAM_TENSORS))
def test_adam_model_is_inside_the_limits(name, call):
    inp, hy = adam_inputs(name, call), adam_hyper(name, call)
    p1, m1, v1 = model_adam(*inp, **hy)
    res = adam_ratios(P.adam(*inp, **hy), p1, m1, v1)
    assert all(r <= 1 for r in res.values()), res
    for kind, _ in ADAM_TENSORS[name].copies:
        if kind == "wsq":
            q = P.wsq(p1)
            for fused in (False, True):
                assert worst(model_wsq(p1, fused), q.value, limit(q, wsq_n(p1[0, 0].numel()), "fp32")) <= 1


def test_adam_inputs_hold_the_planted_elements_and_eight_decades():
    p, g, m, v = adam_inputs("flat9221", 0)
    assert g[0] == 0 and m[1] == 0 and v[1] == 0 and v[2] == 0 and m[2] != 0 and v[3] == 0 and g[3] == 0 and m[3] != 0
    assert float(g.abs().max() / g[g != 0].abs().min()) > 1e8
    hy = adam_hyper("flat9221", 0)
    want = P.adam(p, g, m, v, **hy).p.value
    assert abs(float(want[3] - (p[3].double() - hy["lr"] / (1 - hy["b1"] ** 2) * hy["b1"] * m[3].double() / hy["eps"]))) <= 1e-9 * abs(float(want[3]))


@pytest.mark.parametrize("mut,broken", [("eps_in_sqrt", ("p",)), ("no_bc2", ("p",)), ("swap_betas", ("p", "exp_avg", "exp_avg_sq"))])
def test_adam_mutations_break_the_comparison(mut, broken):
    inp, hy = adam_inputs("flat9221", 0), adam_hyper("flat9221", 0)
    res = adam_ratios(P.adam(*inp, **hy), *model_adam(*inp, mut=mut, **hy))
    assert all(res[k] > 1 for k in broken), (mut, res)


def test_wsq_mutation_breaks_the_comparison():
    w = adam_inputs("w16x130x9", 0)[0]
    q = P.wsq(w)
    lim = limit(q, wsq_n(9), "fp32")
    assert worst(model_wsq(w, True), q.value, lim) <= 1 and worst(model_wsq(w, True, mut="drop_tap"), q.value, lim) > 1


# ================================================================ style coefficients ==========================================
STYLE_SHAPES = [(1, 1, 1, 1), (3, 3, 5, 9), (2, 15, 3, 9), (5, 24, 40, 9), (7, 130, 77, 1), (3, 65, 17, 9), (2, 512, 512, 9)]  # (B, C, O, K)
STYLE_EPS = (1e-8, 1e-3)
StyleIn = collections.namedtuple("StyleIn", "style w gd gs1 d")


def style_counts(B, C, O, K):
    """wsq: the square and K additions.  acc (the argument of rsqrt): style + 1, s * s, the product with wsq, ceil(C / 16)
    additions in the lane, 4 shuffle additions, + eps (whose conversion to float is shorter than this path).  gstyle: the three
    products of dq, the product with wsq, ceil(O / 4) additions, two of the LDS tree, the product with 2 s1, + gs1.
    gw: dq (3), s * s, their product, B additions, the product with 2 w."""
    return dict(wsq=wsq_n(K), acc=3 + -(-C // 16) + 4 + 1, gs=3 + 1 + -(-O // 4) + 2 + 1 + 1, gw=3 + 1 + 1 + B + 1)


def style_inputs(shape, cls, eps):
    B, C, O, K = shape
    k = int(round(K ** 0.5))
    g = gen("style", shape, cls, eps)
    if cls == "exact":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        return StyleIn(ri(-3, 1, B, C) / 2, ri(-4, 4, O, C, k, k), ri(-4, 4, B, O), ri(-4, 4, B, C), 2.0 ** ri(-1, 0, B, O))
    style = 0.5 * torch.randn(B, C, generator=g)
    style[:, 0] = -1 + 1e-3 * torch.randn(B, generator=g)  # s1 near 0: this channel's share of d vanishes
    return StyleIn(style, torch.randn(O, C, k, k, generator=g), torch.randn(B, O, generator=g), torch.randn(B, C, generator=g), None)


def d_limit(want, n_acc):
    return EW["fp32"] * want.value + U * (ULP_RSQRT * want.abs_terms + n_acc * want.arg_terms)


def below_2_24(s, granule, what):
    assert float(s.abs_terms.max()) * granule < 2 ** 24, "%s: a sum of the exact class reaches 2^24 granules" % what


def style_ratios(shape, cls, eps, wsq_fn, fwd_fn, bwd_fn):
    """name -> error / limit (GAUSS) or True / False (EXACT: equality with float32(definition)).  wsq_fn(w), fwd_fn(style,
    wsq, eps) -> (s1, d), bwd_fn(gd, d, s1, wsq, w, gs1 or None) -> (gstyle, gw): the kernels, or their model.  The forward
    gets float32(definition of wsq); the backward the definition's d and s1 rounded to fp32 (EXACT: the handed-in powers of
    two), and the reference is taken from those."""
    inp, cnt, out = style_inputs(shape, cls, eps), style_counts(*shape), {}
    q, s1w = P.wsq(inp.w), P.s1_of(inp.style)
    wsq32 = q.value.float()
    dw = P.demod(inp.style, wsq32, eps)
    got_q = wsq_fn(inp.w)
    s1, d = fwd_fn(inp.style, wsq32, eps)
    assert got_q.dtype == s1.dtype == d.dtype == F32
    out["d"] = worst(d.cpu(), dw.value, d_limit(dw, cnt["acc"]))
    if cls == "exact":
        below_2_24(q, 1, "wsq")
        out["wsq"], out["s1"] = equal_exact(got_q.cpu(), q.value, "fp32"), equal_exact(s1.cpu(), s1w.value, "fp32")
        d32 = inp.d
    else:
        out["wsq"] = worst(got_q.cpu(), q.value, limit(q, cnt["wsq"], "fp32"))
        out["s1"] = worst(s1.cpu(), s1w.value, EW["fp32"] * s1w.value.abs())  # one addition
        d32 = dw.value.float()
    s32 = s1w.value.float()
    for tag, gs1 in (("", inp.gs1), (" (no gs1)", None)):
        want = P.modcoeff_bwd(inp.gd, d32, s32, wsq32, inp.w, gs1)
        gs, gw = bwd_fn(inp.gd, d32, s32, wsq32, inp.w, gs1)
        assert gs.dtype == gw.dtype == F32 and gw.shape == inp.w.shape
        if cls == "exact":
            below_2_24(want.gstyle, 32, "gstyle")  # dq in 1 / 16, 2 s1 in 1
            below_2_24(want.gw, 64, "gw")          # dq s1^2 in 1 / 64
            out["gstyle" + tag], out["gw" + tag] = equal_exact(gs.cpu(), want.gstyle.value, "fp32"), equal_exact(gw.cpu(), want.gw.value, "fp32")
        else:
            out["gstyle" + tag] = worst(gs.cpu(), want.gstyle.value, limit(want.gstyle, cnt["gs"], "fp32"))
            out["gw" + tag] = worst(gw.cpu(), want.gw.value, limit(want.gw, cnt["gw"], "fp32"))
    return out


def _xor_tree(v, width):
    """v += shfl_xor(v, o) for o = width / 2 .. 1 over the last dimension: every lane ends with the sum."""
    idx = torch.arange(width)
    o = width // 2
    while o:
        v = v + v[..., idx ^ o]
        o //= 2
    return v


def _pad(t, dim, mult):
    n = -t.shape[dim] % mult
    return t if n == 0 else torch.cat([t, torch.zeros(t.shape[:dim] + (n,) + t.shape[dim + 1:], dtype=t.dtype)], dim=dim)


def _dq32(gd, d, mut=None):
    dq = t32(-0.5) * gd * d * d
    return dq if mut == "d2" else dq * d


def model_style(mut=None):
    def wsq_fn(w):
        return model_wsq(w, True, mut)

    def fwd_fn(style, wsq32, eps):
        s = style if mut == "no_plus1" else style + t32(1.0)
        ss = _pad(s * s, 1, 16).reshape(s.shape[0], -1, 16)      # [B, j, lane]: channel 16 j + lane
        wq = _pad(wsq32, 1, 16).reshape(wsq32.shape[0], -1, 16)  # (a zero-padded term leaves the accumulator as it is)
        acc = torch.zeros(s.shape[0], wsq32.shape[0], 16)
        for j in range(ss.shape[1]):
            acc = fma(ss[:, None, j, :], wq[None, :, j, :], acc)
        a = _xor_tree(acc, 16)[..., 0] + t32(eps)
        return s, (1 / a.double().sqrt()).float()

    def bwd_fn(gd, d, s1, wsq32, w, gs1):
        B, C = s1.shape
        O = d.shape[1]
        dq = _dq32(gd, d, mut)
        dqp, wqp = _pad(dq, 1, 4).reshape(B, -1, 4), _pad(wsq32, 0, 4).reshape(-1, 4, C)
        part = torch.zeros(B, 4, C)
        for j in range(dqp.shape[1]):
            part = fma(dqp[:, j, :, None], wqp[None, j], part)
        t = (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])
        two = t32(1.0 if mut == "no2" else 2.0)
        gs = (torch.zeros(B, C) if gs1 is None else gs1) + two * s1 * t
        acc = torch.zeros(O, C)
        for b in range(B):
            acc = fma(dq[b, :, None], (s1[b] * s1[b])[None, :], acc)
        gw = t32(2.0) * w * acc.view(O, C, *([1] * (w.dim() - 2)))
        return gs, gw

    return wsq_fn, fwd_fn, bwd_fn


def test_style_definitions_are_autograd_of_the_composition():
    B, C, O, k = 3, 7, 5, 3
    g = gen("style64")
    style, w = torch.randn(B, C, generator=g, dtype=F64).requires_grad_(), torch.randn(O, C, k, k, generator=g, dtype=F64).requires_grad_()
    r1, r2 = torch.randn(B, C, generator=g, dtype=F64), torch.randn(B, O, generator=g, dtype=F64)
    s1 = style + 1
    d = torch.rsqrt((s1 * s1) @ w.pow(2).sum(dim=(2, 3)).t() + 1e-3)
    gs_d, gw_d = torch.autograd.grad((d * r2).sum(), [style, w], retain_graph=True)
    q = P.wsq(w.detach())
    assert rel(q.value, w.detach().pow(2).sum(dim=(2, 3))) < 1e-15
    assert rel(P.s1_of(style.detach()).value, s1.detach()) == 0 and rel(P.demod(style.detach(), q.value, 1e-3).value, d.detach()) < 1e-12
    both = P.modcoeff_bwd(r2, d.detach(), s1.detach(), q.value, w.detach(), r1)
    only = P.modcoeff_bwd(r2, d.detach(), s1.detach(), q.value, w.detach(), None)
    assert rel(both.gstyle.value, gs_d + r1) < 1e-12 and rel(only.gstyle.value, gs_d) < 1e-12
    assert rel(both.gw.value, gw_d) < 1e-12 and torch.equal(both.gw.value, only.gw.value)


@pytest.mark.parametrize("eps", STYLE_EPS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("shape", STYLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_style_model_is_inside_the_limits(shape, cls, eps):
    res = style_ratios(shape, cls, eps, *model_style())
    assert all(v is True or (v is not False and v <= 1) for v in res.values()), res
    if cls == "gauss":
        assert float(P.s1_of(style_inputs(shape, cls, eps).style).value[:, 0].abs().max()) < 0.01, "the planted column"


@pytest.mark.parametrize("mut,broken", [("drop_tap", ("wsq",)), ("d2", ("gstyle", "gw")), ("no_plus1", ("s1", "d")), ("no2", ("gstyle",))])
def test_style_mutations_break_the_comparison(mut, broken):
    res = style_ratios((5, 24, 40, 9), "gauss", 1e-8, *model_style(mut))
    assert all(res[k] > 1 for k in broken), (mut, res)
    res = style_ratios((5, 24, 40, 9), "exact", 1e-8, *model_style(mut))
    assert all((res[k] is False) if isinstance(res[k], bool) else res[k] > 1 for k in broken), (mut, res)


# ================================================================ initial block ===============================================
IB_SHAPES = [(1, 1, 1, 1), (3, 7, 18, 24), (3, 2, 514, 80), (65, 4, 33, 16), (130, 2, 18, 40), (2, 64, 20, 64), (2, 3, 1024, 16),
             (9, 7, 514, 512)]  # (B, L, D, C)
IB_OUTSIDE = [(2, 65, 18, 16), (2, 7, 1025, 16), (2, 7, 18, 513)]


def ib_counts(B, L, D, C):
    """x: the L additions and the division of the mean, the product, D additions.  dstyles: the product, 16 ceil(C / 64)
    additions in the lane, six shuffle additions, 1.f / L and the product with it.  dW: the mean, the product, B additions."""
    return dict(x=(L + 1) + 1 + D, ds=1 + 16 * -(-C // 64) + 6 + 2, dw=(L + 1) + 1 + B)


def ib_inputs(case, cls, prec):
    """(styles [B, L, D], W [D, C, 4, 4], gx [B, C, 4, 4]) fp32; in bf16 W and gx hold bf16 values (rounded first)."""
    B, L, D, C = case
    g = gen("ib", case, cls)
    if cls == "exact":
        ri = lambda *s: torch.randint(-4, 5, s, generator=g).float()
        return ri(B, 1, D).expand(B, L, D).contiguous(), ri(D, C, 4, 4), ri(B, C, 4, 4)
    styles, w, gx = torch.randn(B, L, D, generator=g), torch.randn(D, C, 4, 4, generator=g) / D ** 0.5, torch.randn(B, C, 4, 4, generator=g)
    return (styles, w.to(DT[prec]).float(), gx.to(DT[prec]).float())


def ib_ratios(case, cls, prec, fwd, dgrad, wgrad):
    """fwd(styles, w) -> x, dgrad(gx, w, L) -> dstyles, wgrad(styles, gx) -> dW: the kernels in precision `prec`, or their
    model.  x has the activation dtype, the gradients are fp32."""
    B, L, D, C = case
    styles, w, gx = ib_inputs(case, cls, prec)
    cnt, out = ib_counts(*case), {}
    xw, dsw, dww = P.initial_block(styles, w), P.initial_block_dstyles(gx, w, L), P.initial_block_dw(styles, gx)
    x, ds, dwg = fwd(styles, w), dgrad(gx, w, L), wgrad(styles, gx)
    assert x.dtype == DT[prec] and ds.dtype == dwg.dtype == F32
    assert tuple(x.shape) == (B, C, 4, 4) and tuple(ds.shape) == (B, L, D) and tuple(dwg.shape) == (D, C, 4, 4)
    ds = ds.cpu()
    out["dstyles rows"] = all(torch.equal(ds[:, 0], ds[:, l]) for l in range(L))
    if cls == "exact":
        for s, what in ((xw, "x"), (dsw, "dstyles"), (dww, "dW")):
            assert float(s.abs_terms.max()) * (L if what == "dstyles" else 1) < 2 ** 24, what
        out["x"], out["dW"] = equal_exact(x.cpu(), xw.value, prec), equal_exact(dwg.cpu(), dww.value, "fp32")
        if L & (L - 1) == 0:
            out["dstyles"] = equal_exact(ds, dsw.value, "fp32")
        else:  # s * (1.f / L): the rounding of the reciprocal and of the product
            out["dstyles"] = worst(ds, dsw.value, 2 * U * (1 + U) * dsw.value.abs())
    else:
        out["x"] = worst(x.cpu(), xw.value, limit(xw, cnt["x"], prec))
        out["dstyles"] = worst(ds, dsw.value, limit(dsw, cnt["ds"], "fp32"))
        out["dW"] = worst(dwg.cpu(), dww.value, limit(dww, cnt["dw"], "fp32"))
    return out


def _avg32(styles):
    a = torch.zeros(styles.shape[0], styles.shape[2])
    for l in range(styles.shape[1]):
        a = a + styles[:, l]
    return a / t32(float(styles.shape[1]))


def model_ib(prec, mut=None):
    def fwd(styles, w):
        avg, wm = _avg32(styles), w.reshape(w.shape[0], -1)
        acc = torch.zeros(styles.shape[0], wm.shape[1])
        for d in range(wm.shape[0]):
            acc = fma(avg[:, d, None], wm[None, d], acc)
        x = acc.view(styles.shape[0], -1, 16).clone()
        if mut == "swap_pixel":
            x[:, 0, [4, 5]] = x[:, 0, [5, 4]]
        return x.view(styles.shape[0], -1, 4, 4).to(DT[prec])

    def dgrad(gx, w, L):
        B, D = gx.shape[0], w.shape[0]
        g, wm = _pad(gx.reshape(B, -1, 16), 1, 64), _pad(w.reshape(D, -1, 16), 1, 64)  # [., c, p]
        acc = torch.zeros(B, D, 64)
        for c0 in range(0, g.shape[1], 64):
            for p in range(16):
                acc = fma(g[:, None, c0:c0 + 64, p], wm[None, :, c0:c0 + 64, p], acc)
        s = _xor_tree(acc, 64)[..., 0]
        if mut != "no_1_over_L":
            s = s * (t32(1.0) / t32(float(L)))
        return s[:, None, :].expand(B, L, D).contiguous()

    def wgrad(styles, gx):
        avg, g = _avg32(styles), gx.reshape(gx.shape[0], -1)
        acc = torch.zeros(avg.shape[1], g.shape[1])
        for b in range(gx.shape[0] - (1 if mut == "drop_sample" else 0)):
            acc = fma(avg[b, :, None], g[None, b], acc)
        return acc.view(avg.shape[1], *gx.shape[1:])

    return fwd, dgrad, wgrad


def test_initial_block_definitions_are_autograd_of_conv_transpose():
    B, L, D, C = 3, 5, 6, 7
    g = gen("ib64")
    styles, w = torch.randn(B, L, D, generator=g, dtype=F64).requires_grad_(), torch.randn(D, C, 4, 4, generator=g, dtype=F64).requires_grad_()
    gx = torch.randn(B, C, 4, 4, generator=g, dtype=F64)
    x = F.conv_transpose2d(styles.mean(dim=1)[:, :, None, None], w)
    gs, gw = torch.autograd.grad((x * gx).sum(), [styles, w])
    assert rel(P.initial_block(styles.detach(), w.detach()).value, x.detach()) < 1e-12
    assert rel(P.initial_block_dstyles(gx, w.detach(), L).value, gs) < 1e-12
    assert rel(P.initial_block_dw(styles.detach(), gx).value, gw) < 1e-12


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("cls", ("exact", "gauss"))
@pytest.mark.parametrize("case", IB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_initial_block_model_is_inside_the_limits(case, cls, prec):
    res = ib_ratios(case, cls, prec, *model_ib(prec))
    assert all(v is True or (v is not False and v <= 1) for v in res.values()), res


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mut,case,broken", [("no_1_over_L", (3, 7, 18, 24), "dstyles"), ("drop_sample", (65, 4, 33, 16), "dW"),
                                             ("swap_pixel", (3, 7, 18, 24), "x")])
def test_initial_block_mutations_break_the_comparison(mut, case, broken, prec):
    for cls in ("gauss", "exact"):
        r = ib_ratios(case, cls, prec, *model_ib(prec, mut))[broken]
        assert (r is False) if isinstance(r, bool) else r > 1, (mut, cls, r)
