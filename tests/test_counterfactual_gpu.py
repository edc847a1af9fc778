"""-m gpu: the counterfactual experiment on the MI355X — the edit kernel (csrc/style_edit.hip) bit for bit against
the fp32 definition of tests/_counterfactual_defs.py, the batched engine in fp32 mode against the naive batch-1 loop and
change_images at the bound test_attfind_batched_engine_on_hip_vs_reference_notebook_golden uses for batched against batch-1
on these kernels (2e-4 of the tensor's maximum), prefix sharing exactly, the sweep's FID values against FIDEvaluator fed by
hand, and the command line end to end."""
import csv
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attfind  # noqa: E402
import hip_backend as hb  # noqa: E402
import networks  # noqa: E402
import ops  # noqa: E402
import test_counterfactual_cpu as tc  # noqa: E402
from _counterfactual_defs import edit_levels, naive_images, segment_major  # noqa: E402
from conftest import load_golden  # noqa: E402
from test_attfind_cpu import build  # noqa: E402

DEV = "cuda:0"
TOL = 2e-4
MARGIN = 1024  # floats of NaN on either side of the kernel's output


@pytest.fixture(autouse=True)
def hip_impl():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    prev = ops.use_impl(ops.HipOps)
    ops.set_precision("fp32")
    hb.load_library()  # fails loudly if the extension is missing
    yield
    ops.set_precision("fp32")
    ops.use_impl(prev)


def close(got, want, tol=TOL):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(1e-3, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print("max |err| %.3e of max |want| %.3e" % (err, scale))
    assert err <= tol * scale, (err, scale)


# ---- the kernel ---------------------------------------------------------------------------------------------------------


def _generator_table(image_size=64, capacity=16, fmap_max=512):
    f = networks.generator_filters(image_size, capacity, fmap_max)
    seg = [0]
    for cin, cout in zip(f, f[1:]):
        seg += [seg[-1] + cin, seg[-1] + cin + cout]
    return seg


SEG_TABLES = {"two": [0, 2, 5], "three": [0, 1, 3, 67], "generator64": _generator_table()}


def _edit_list(seg, k):
    """k (direction, coordinate) pairs over the columns where an indexing mistake would show — 0, S - 1, the last column of
    every segment and the first of the next — with entry 1 the first coordinate again in the OPPOSITE direction and entry 3
    the third coordinate again in the SAME direction."""
    s = seg[-1]
    pool = [0, s - 1]
    for b in seg[1:-1]:
        pool += [b - 1, b]
    pool = list(dict.fromkeys(pool))
    edits = [(j % 2 if j % 3 else 1 - j % 2, pool[j % len(pool)]) for j in range(k)]
    if k >= 2:
        edits[1] = (1 - edits[0][0], edits[0][1])
    if k >= 4:
        edits[3] = edits[2]
    return edits


def _launch(coords, smin, smax, edits, base, levels, seg, shift):
    """The kernel's L * N * S floats (from inside a NaN-filled buffer whose margins are checked) as a numpy array."""
    n, s = coords.shape
    total = len(levels) * n * s
    buf = torch.full((total + 2 * MARGIN,), float("nan"), device=DEV)
    segs = hb.style_edit_levels(coords, smin, smax, [c for _, c in edits], [d for d, _ in edits], base, levels, seg, shift,
                                out=buf[MARGIN:MARGIN + total])
    assert [tuple(t.shape) for t in segs] == [(len(levels), n, b - a) for a, b in zip(seg, seg[1:])]
    assert segs[0].data_ptr() == buf.data_ptr() + 4 * MARGIN
    host = buf.cpu().numpy()
    assert np.isnan(host[:MARGIN]).all() and np.isnan(host[MARGIN + total:]).all(), "the kernel wrote outside its output"
    return host[MARGIN:MARGIN + total]


@pytest.mark.parametrize("table", sorted(SEG_TABLES))
@pytest.mark.parametrize("n", [1, 3, 65])
def test_style_edit_kernel_equals_the_fp32_definition_bit_for_bit(n, table):
    seg = SEG_TABLES[table]
    s = seg[-1]
    rng = np.random.RandomState(1000 * n + s)
    coords = rng.randn(n, s).astype(np.float32)
    smin, smax = rng.randn(s).astype(np.float32), rng.randn(s).astype(np.float32)  # Gaussian operands: no order assumed
    d_coords, d_smin, d_smax = (torch.from_numpy(a).to(DEV) for a in (coords, smin, smax))
    bases = {"zeros": np.zeros(n, dtype=np.int32), "ones": np.ones(n, dtype=np.int32),
             "mixed": (rng.rand(n) < 0.5).astype(np.int32)}
    checked = 0
    for k in (1, 2, 11, hb.style_edit_max_k()):
        edits = _edit_list(seg, k)
        for levels in (list(range(k + 1)), [min(3, k), 1, min(3, k)]):
            # every shift with every base-class pattern at K = 11; one pattern per shift at the other lengths
            pairs = [(sh, nm) for sh in (0.5, 1.0, 2.0) for nm in bases] if k == 11 else list(zip((0.5, 1.0, 2.0), bases))
            for shift, name in pairs:
                base = bases[name]
                want = segment_major(edit_levels(coords, smin, smax, edits, base, levels, shift), seg)
                got = _launch(d_coords, d_smin, d_smax, edits, torch.from_numpy(base).to(DEV), levels, seg, shift)
                same = got.view(np.int32) == want.view(np.int32)
                assert same.all(), (k, levels[:4], shift, name, int((~same).sum()), np.flatnonzero(~same)[:8])
                checked += 1
    assert checked == 36
    # the edits are not no-ops on these operands, and a second launch on another stream gives the same bits
    k = 11
    edits, levels, base = _edit_list(seg, k), list(range(k + 1)), torch.from_numpy(bases["mixed"]).to(DEV)
    first = _launch(d_coords, d_smin, d_smax, edits, base, levels, seg, 0.5)
    plain = segment_major(np.broadcast_to(coords, (k + 1,) + coords.shape).copy(), seg)
    assert (first != plain).any()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = _launch(d_coords, d_smin, d_smax, edits, base, levels, seg, 0.5)
    torch.cuda.current_stream().wait_stream(side)
    assert np.array_equal(first.view(np.int32), second.view(np.int32))


def test_style_edit_argument_validation_returns_before_a_launch():
    tc.test_style_edit_entry_point_rejects_bad_arguments_before_the_device()
    lib = hb.load_library()
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = hb._ptr
    before = t.clone()
    args = [p(t), p(t), p(t), p(i), p(i), p(i), p(i), p(i), p(t)]
    assert lib.stylex_style_edit_levels(*args, 2, 5, hb.style_edit_max_k() + 1, 1, 2, 1.0, hb._stream()) == -1
    assert lib.stylex_style_edit_levels(*args, 0, 5, 1, 1, 2, 1.0, hb._stream()) == -1
    args[8] = None
    assert lib.stylex_style_edit_levels(*args, 2, 5, 1, 1, 2, 1.0, hb._stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(t, before)
    tc.test_style_edit_wrapper_checks_what_the_device_cannot_report()


# ---- the engine ---------------------------------------------------------------------------------------------------------


def _model():
    g = load_golden("attfind_16")
    m, clf, _, noise = build(g, device=DEV)
    clf.b2 = clf.b2.clone()
    return g, m.to(DEV), clf, noise


def _base_coords(G, latents, noise):
    with torch.no_grad():
        w = torch.as_tensor(latents, device=DEV)
        return G(attfind.styles_def_to_tensor([(w, G.num_layers)]), noise.expand(len(w), -1, -1, -1), get_style_coords=True)[1]


@pytest.mark.parametrize("shift", [1.0, 0.5])
def test_engine_on_hip_vs_the_naive_loop_and_prefix_sharing(shift):
    """share_prefix=True against False is expected to be torch.equal: the blocks that run get the same style bits (the
    kernel's output rows), the same to-RGB style (the fused affine GEMM's third column block, as in the base pass) and the
    same launches on the same shapes."""
    g, m, clf, noise = _model()
    latents, smin, smax = g["out/latents"], g["out/minima"][0], g["out/maxima"][0]
    base_class = tc._split_classes(m.G, clf, latents, noise)
    assert sorted(set(base_class.tolist())) == [0, 1]
    levels = [0, 1, 2, 3, 4, 5, 3]
    styles = edit_levels(_base_coords(m.G, latents, noise).cpu().numpy(), smin, smax, tc.EDITS, base_class.cpu().numpy(), levels,
                         shift)
    runs = {}
    for share in (True, False):
        out = list(attfind.counterfactual_images(m.G, clf, latents, tc.EDITS, smin, smax, noise, levels, shift_size=shift,
                                                 image_batch=2, share_prefix=share))
        assert [k for k, _, _ in out] == levels * 2 and [img.shape[0] for _, img, _ in out] == [2] * 7 + [1] * 7
        runs[share] = out
    for i in range(3):
        want = naive_images(m.G, latents, noise, styles[:, i], i)
        first = 0 if i < 2 else 7
        for row in range(len(levels)):
            _, img, logits = runs[True][first + row]
            close(img[i % 2:i % 2 + 1], want[row:row + 1])
            close(logits[i % 2:i % 2 + 1], clf.classify_images(want[row:row + 1]))
    assert float((runs[True][5][1] - runs[True][0][1]).abs().max()) > 1e-3
    for (k, a, la), (_, b, lb) in zip(runs[True], runs[False]):
        assert torch.equal(a, b) and torch.equal(la, lb), (k, float((a - b).abs().max()))


def test_single_edit_on_hip_vs_change_images():
    g, m, clf, noise = _model()
    latents, smin, smax = g["out/latents"], g["out/minima"][0], g["out/maxima"][0]
    base_class = tc._split_classes(m.G, clf, latents, noise)
    for direction, sindex in ((0, 5), (1, 63), (0, 64), (1, 135)):
        got = [img for k, img, _ in attfind.counterfactual_images(m.G, clf, latents, [(direction, sindex)], smin, smax, noise,
                                                                  [1], image_batch=3)]
        for c in (0, 1):  # base class 0 swaps the direction
            rows = [i for i in range(3) if int(base_class[i]) == c]
            eff = direction if c == 1 else 1 - direction
            _, changed, _, _ = attfind.change_images(m.G, clf, latents[rows], sindex, eff, smin[sindex], smax[sindex], 1.0, noise)
            close(got[0][rows], changed)


# ---- the sweep's FID ----------------------------------------------------------------------------------------------------


class SmallFeatures(torch.nn.Module):
    """A stand-in for the Inception network: [B, 3, 32, 32] -> [B, 16, 4, 4]."""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(5)
        self.w = torch.nn.Parameter(torch.randn(16, 3, 8, 8, generator=gen) * 0.2, requires_grad=False)

    def forward(self, x):
        return torch.nn.functional.conv2d(x, self.w, stride=8).contiguous()


def test_sweep_fid_equals_the_evaluator_fed_by_hand():
    import fid

    g, m, clf, noise = _model()
    latents, smin, smax = g["out/latents"], g["out/minima"][0], g["out/maxima"][0]
    base_class = tc._split_classes(m.G, clf, latents, noise)
    tc._put_an_image_on_the_boundary(m.G, clf, latents, smin, smax, noise, base_class, 2.0)
    records = dict(latents=latents, minima=smin, maxima=smax, noise=g["out/noise"], original_images=g["out/original_images"])
    net = SmallFeatures().to(DEV)
    out = attfind.counterfactual_sweep(m, clf, records, tc.EDITS, num_attributes=4, shift_size=2.0, image_batch=2,
                                       fid=fid.FIDEvaluator(net, input_size=32))
    assert out["k"] == [1, 2, 3, 4] and len(out["fid"]) == 5 and np.array_equal(out["base_class"], base_class.cpu().numpy())
    originals = torch.from_numpy(g["out/original_images"]).to(DEV)
    hand = {k: fid.FIDEvaluator(net, input_size=32) for k in range(5)}
    flips = [0] * 4
    for ev in hand.values():
        for lo in (0, 2):
            ev.add_real(originals[lo:lo + 2])
    for k, img, logits in attfind.counterfactual_images(m.G, clf, latents, tc.EDITS[:4], smin, smax, noise, [0, 1, 2, 3, 4],
                                                        shift_size=2.0, image_batch=2):
        hand[k].add_fake(img)
        if k:
            rows = base_class[:2] if img.shape[0] == 2 else base_class[2:]
            flips[k - 1] += int((logits.argmax(dim=-1) != rows).sum())
    assert out["flips"] == flips and flips[0] == 1, (out["flips"], flips)
    for k in range(5):
        want = hand[k].value()
        print("k = %d: fid %.12g by hand %.12g" % (k, out["fid"][k], want))
        assert abs(out["fid"][k] - want) <= 1e-12 * abs(want), (k, out["fid"][k], want)
    assert len({round(v, 9) for v in out["fid"]}) > 1  # the levels are different image sets


# ---- the command line ---------------------------------------------------------------------------------------------------


def test_attfind_cli_counterfactual_end_to_end(tmp_path, monkeypatch):
    """16 px, 6 images, --counterfactual_fid 2 --fid_weights random:0, in this process.  The stand-in classifier's bias is
    set so that the six generated images fall into both classes (8.8: on the host double their logit differences are
    0.46, -1.3, -0.5, 1.5, 2.0, 3.3 with it) — the ranking needs both."""
    import attfind_cli

    argv, folder = tc.cli_case(tmp_path, monkeypatch, 6, bias_shift=8.8)
    attfind_cli.main(argv + ["--counterfactual_fid", "2", "--fid_weights", "random:0"])
    rows = list(csv.reader(open(folder / "counterfactual_fid.csv")))
    assert rows[0] == ["", "Original-Generated", "Original-Attribute 1", "Original-Attributes 1-2"]
    assert len(rows) == 2 and rows[1][0] == "0" and len(rows[1]) == 4
    values = [float(v) for v in rows[1][1:]]
    assert all(np.isfinite(v) and v >= 0 and "%.2f" % v == t for v, t in zip(values, rows[1][1:]))
    info = json.load(open(folder / "counterfactual.json"))
    rec = attfind.load_records(str(folder))
    assert sorted(set(info["base_class"])) == [0, 1]
    assert info["base_class"] == np.argmax(rec["base_prob"], axis=1).tolist()
    ranked = attfind.rank_class_directions(attfind.filter_unstable_images(np.array(rec["style_change"], copy=True)),
                                           rec["base_prob"])
    assert info["ranked"] == [[d, s] for d, s in ranked] and info["k"] == [1, 2]
    # the flip counts, recomputed on the loaded model's generator with the same classifier
    model = attfind_cli.load_model(dict(attfind_cli.DEFAULTS, name="cf", models_dir=str(tmp_path / "models"),
                                        results_dir=str(tmp_path / "res"), load_from=0, image_size=16, network_capacity=2,
                                        fmap_max=16, classifier_path=None), 0)
    flips = [0, 0]
    base = torch.tensor(info["base_class"], device=DEV)
    for k, _, logits in attfind.counterfactual_images(model.StylEx.G, model.classifier, rec["latents"], ranked[:2], rec["minima"],
                                                      rec["maxima"], rec["noise"], [1, 2], image_batch=32):
        flips[k - 1] += int((logits.argmax(dim=-1) != base).sum())
    assert info["flips"] == flips and info["flip_rate"] == [f / 6 for f in flips]
