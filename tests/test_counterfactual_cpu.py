"""The counterfactual experiment of the reference's stylex/FID_TensorFlow.ipynb without a GPU: the attribute
ranking against tests/golden/counterfactual_rank.npz (cells 9, 12 and 13 of that notebook executed as they are,
tools/make_golden_counterfactual.py), the edit rule's definition against itself, the batched engine on the CPU test double
against change_images and the naive loop, the sweep's counts, the table writer and the command line's new flags."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import attfind
import hip_backend
import ops
from _counterfactual_defs import edit_levels, naive_images, segment_major
from cpu_ops import CpuOracleOps
from test_attfind_cpu import GOLD, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_GOLD = os.path.join(ROOT, "tests", "golden", "counterfactual_rank.npz")
TOL = 2e-5  # the bound of test_batched_engine_vs_reference_notebook_golden, relative to the tensor's maximum


@pytest.fixture()
def cpu_double():
    prev = ops.use_impl(CpuOracleOps)
    yield
    ops.use_impl(prev)


def close(got, want, tol=TOL):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(1e-3, float(np.abs(want).max()))
    assert float(np.abs(got - want).max()) <= tol * scale, (float(np.abs(got - want).max()), scale)


# ---- ranking ------------------------------------------------------------------------------------------------------------


def test_rank_class_directions_equals_the_notebook_cells():
    g = np.load(RANK_GOLD)
    got = attfind.rank_class_directions(g["style_change_effect"], g["base_probs"], num_indices=int(g["num_indices"]),
                                        effect_threshold=float(g["effect_threshold"]))
    assert got == [tuple(int(v) for v in row) for row in g["ranked"]]
    assert all(type(d) is int and type(s) is int for d, s in got)
    coords = [s for _, s in got]
    assert len(got) > int(g["num_indices"]) and len(set(coords)) < len(coords)  # longer than num_indices, one duplicate
    # the defaults are cell 13's constants
    assert got == attfind.rank_class_directions(g["style_change_effect"], g["base_probs"])


def test_rank_class_directions_rejects_what_the_notebook_cannot_run():
    g = np.load(RANK_GOLD)
    effect, probs = g["style_change_effect"], g["base_probs"]
    for c in (0, 1):
        one_class = np.zeros_like(probs)
        one_class[:, c] = 1.0
        with pytest.raises(ValueError):
            attfind.rank_class_directions(effect, one_class)
    with pytest.raises(ValueError):
        attfind.rank_class_directions(np.concatenate((effect, effect[..., :1]), axis=-1), probs)
    with pytest.raises(ValueError):
        attfind.rank_class_directions(effect[..., :1], probs)


# ---- the definition against itself --------------------------------------------------------------------------------------


def _operands(n=7, s=12, seed=0):
    rng = np.random.RandomState(seed)
    coords = rng.randn(n, s).astype(np.float32)
    smin = (coords.min(axis=0) - rng.rand(s)).astype(np.float32)
    smax = (coords.max(axis=0) + rng.rand(s)).astype(np.float32)
    return coords, smin, smax


def test_definition_one_edit_is_the_change_images_arithmetic():
    coords, smin, smax = _operands()
    for direction in (0, 1):
        for shift in (0.5, 1.0, 2.0):
            got = edit_levels(coords, smin, smax, [(direction, 4)], np.ones(7, dtype=np.int64), [1], shift)[0]
            s = torch.from_numpy(coords.copy())
            target = float(smin[4]) if direction == 0 else float(smax[4])
            delta = (target - s[:, 4]) * shift  # change_images: delta = (target - coords) * shift; s += delta
            s[:, 4] += delta
            assert got.dtype == np.float32 and np.array_equal(got, s.numpy())


def test_definition_is_sequential():
    coords, smin, smax = _operands()
    ones = np.ones(7, dtype=np.int64)
    pair = [(0, 3), (1, 3)]
    for dtype in (np.float32, np.float64):
        end = edit_levels(coords, smin, smax, pair, ones, [2], 1.0, dtype)[0]
        assert np.allclose(end[:, 3], smax[3], rtol=1e-6)  # shift 1, opposite directions: the second target
        half = edit_levels(coords, smin, smax, pair, ones, [2], 0.5, dtype)[0]
        c = coords[:, 3].astype(dtype)
        parallel = c + (smin[3] - c) * dtype(0.5) + (smax[3] - c) * dtype(0.5)  # both shifts from the unedited value
        assert np.abs(half[:, 3] - parallel).min() > 1e-3
        other = np.delete(np.arange(12), 3)
        assert np.array_equal(half[:, other], coords[:, other].astype(dtype))


def test_definition_base_class_zero_swaps_every_direction():
    coords, smin, smax = _operands()
    edits = [(0, 3), (1, 5), (1, 3), (0, 11)]
    swapped = [(1 - d, s) for d, s in edits]
    levels = [0, 1, 2, 3, 4]
    for dtype in (np.float32, np.float64):
        a = edit_levels(coords, smin, smax, edits, np.zeros(7, dtype=np.int64), levels, 0.5, dtype)
        b = edit_levels(coords, smin, smax, swapped, np.ones(7, dtype=np.int64), levels, 0.5, dtype)
        assert np.array_equal(a, b)
        assert np.array_equal(a[0], coords.astype(dtype))
    mixed = edit_levels(coords, smin, smax, edits, np.array([0, 1, 0, 1, 1, 0, 1]), levels, 0.5)
    ones = edit_levels(coords, smin, smax, edits, np.ones(7, dtype=np.int64), levels, 0.5)
    zeros = edit_levels(coords, smin, smax, edits, np.zeros(7, dtype=np.int64), levels, 0.5)
    assert np.array_equal(mixed[:, [1, 3, 4, 6]], ones[:, [1, 3, 4, 6]]) and np.array_equal(mixed[:, [0, 2, 5]], zeros[:, [0, 2, 5]])


def test_torch_composition_equals_the_definition_bit_for_bit(cpu_double):
    """The path the CPU double takes (attfind.edited_styles without a fused op) against the fp32 definition."""
    coords, smin, smax = _operands(n=5, s=12, seed=3)
    edits = [(0, 3), (1, 5), (1, 3), (0, 11), (0, 0)]
    base = np.array([0, 1, 1, 0, 1])
    seg = [0, 2, 5, 12]
    for shift in (0.5, 1.0, 2.0):
        levels = [3, 1, 3, 0, 5]
        segs = attfind.edited_styles(torch.from_numpy(coords), edits, torch.from_numpy(smin), torch.from_numpy(smax),
                                     torch.from_numpy(base).to(torch.int32), levels, seg, shift)
        want = edit_levels(coords, smin, smax, edits, base, levels, shift)
        got = np.concatenate([t.numpy().reshape(-1) for t in segs])
        assert np.array_equal(got, segment_major(want, seg))
        assert [tuple(t.shape) for t in segs] == [(5, 5, 2), (5, 5, 3), (5, 5, 7)] and all(t.is_contiguous() for t in segs)


# ---- the engine on the CPU double ---------------------------------------------------------------------------------------

EDITS = [(1, 130), (0, 64), (1, 63), (0, 130), (1, 5)]  # last block, a block's first / the previous block's last column, a duplicate, first block


def _model():
    g = np.load(GOLD)
    m, clf, _, noise = build(g)
    clf.b2 = clf.b2.clone()
    return g, m, clf, noise


def _split_classes(G, clf, latents, noise):
    """Moves the stand-in classifier's bias so that the base images fall into both classes."""
    with torch.no_grad():
        w = torch.as_tensor(latents, device=noise.device)
        img = G(attfind.styles_def_to_tensor([(w, G.num_layers)]), noise.expand(len(w), -1, -1, -1))
        logits = clf.classify_images(img)
    d = torch.sort(logits[:, 0] - logits[:, 1])[0]
    clf.b2[1] += (d[0] + d[1]) / 2
    return clf.classify_images(img).argmax(dim=-1)


def test_single_edit_equals_change_images(cpu_double):
    g, m, clf, noise = _model()
    latents, smin, smax = g["out/latents"], g["out/minima"][0], g["out/maxima"][0]
    base_class = _split_classes(m.G, clf, latents, noise)
    assert sorted(set(base_class.tolist())) == [0, 1]
    seg = attfind.style_segments(m.G)
    assert seg == [0, 32, 64, 96, 112, 128, 136]
    for direction, sindex in ((0, 5), (1, 63), (0, 64), (1, 135)):
        got = list(attfind.counterfactual_images(m.G, clf, latents, [(direction, sindex)], smin, smax, noise, [1, 0],
                                                 image_batch=2))
        assert [k for k, _, _ in got] == [1, 0, 1, 0]
        images = torch.cat([img for k, img, _ in got if k == 1])
        logits = torch.cat([lg for k, _, lg in got if k == 1])
        for i in range(len(latents)):
            # base class 0 swaps the direction (cell 20's flip)
            eff = direction if int(base_class[i]) == 1 else 1 - direction
            base, changed, _, _ = attfind.change_images(m.G, clf, latents[i:i + 1], sindex, eff, smin[sindex], smax[sindex], 1.0,
                                                        noise)
            close(images[i:i + 1], changed)
            close(logits[i:i + 1], clf.classify_images(changed), 1e-4)
            # the edited style value: change_images' own arithmetic on this image's coordinate, bit for bit
            with torch.no_grad():
                _, sc = m.G(attfind.styles_def_to_tensor([(torch.from_numpy(latents[i:i + 1]), m.G.num_layers)]), noise,
                            get_style_coords=True)
            s = sc[:, sindex].clone()
            s += ((float(smin[sindex]) if eff == 0 else float(smax[sindex])) - sc[:, sindex]) * 1.0
            segs = attfind.edited_styles(sc.contiguous(), [(direction, sindex)], torch.from_numpy(smin), torch.from_numpy(smax),
                                         base_class[i:i + 1].to(torch.int32), [1], seg, 1.0)
            edited = torch.cat([t[0] for t in segs], dim=1)
            assert torch.equal(edited[:, sindex], s)
            keep = [c for c in range(136) if c != sindex]
            assert torch.equal(edited[:, keep], sc[:, keep])


@pytest.mark.parametrize("shift", [1.0, 0.5])
def test_engine_equals_the_naive_loop_and_shares_prefixes_exactly(cpu_double, shift):
    g, m, clf, noise = _model()
    latents, smin, smax = g["out/latents"], g["out/minima"][0], g["out/maxima"][0]
    base_class = _split_classes(m.G, clf, latents, noise)
    levels = [0, 1, 2, 3, 4, 5, 3]
    with torch.no_grad():
        _, sc = m.G(attfind.styles_def_to_tensor([(torch.from_numpy(latents), m.G.num_layers)]), noise.expand(3, -1, -1, -1),
                    get_style_coords=True)
    styles = edit_levels(sc.numpy(), smin, smax, EDITS, base_class.numpy(), levels, shift)
    runs = {}
    for share in (True, False):
        out = list(attfind.counterfactual_images(m.G, clf, latents, EDITS, smin, smax, noise, levels, shift_size=shift,
                                                 image_batch=2, share_prefix=share))
        assert [k for k, _, _ in out] == levels * 2 and [img.shape[0] for _, img, _ in out] == [2] * 7 + [1] * 7
        runs[share] = out
    for (_, a, la), (_, b, lb) in zip(runs[True], runs[False]):
        assert torch.equal(a, b) and torch.equal(la, lb)
    for i in range(3):
        want = naive_images(m.G, latents, noise, styles[:, i], i)
        first = 0 if i < 2 else 7
        for row in range(len(levels)):
            _, img, logits = runs[True][first + row]
            close(img[i % 2:i % 2 + 1], want[row:row + 1])
            close(logits[i % 2:i % 2 + 1], clf.classify_images(want[row:row + 1]), 1e-4)
    # the edits move the image: the comparison above is not between copies of the base image
    assert float((runs[True][5][1] - runs[True][0][1]).abs().max()) > 1e-3


def _put_an_image_on_the_boundary(G, clf, latents, smin, smax, noise, base_class, shift):
    """Moves the classifier's bias once more, midway between the base value and the one-edit value of the image whose
    logit difference the first edit moves most — without changing any base class — so that the sweep has a flip to count."""
    diffs = {}
    for k, _, logits in attfind.counterfactual_images(G, clf, latents, EDITS, smin, smax, noise, [0, 1], shift_size=shift,
                                                      image_batch=len(latents)):
        diffs[k] = logits[:, 0] - logits[:, 1]
    i = int((diffs[1] - diffs[0]).abs().argmax())
    assert float((diffs[1][i] - diffs[0][i]).abs()) > 0.02, "the first edit moves no image's logits enough to place a boundary"
    clf.b2[1] += (diffs[0][i] + diffs[1][i]) / 2
    with torch.no_grad():
        w = torch.as_tensor(latents, device=noise.device)
        logits = clf.classify_images(G(attfind.styles_def_to_tensor([(w, G.num_layers)]), noise.expand(len(w), -1, -1, -1)))
    assert torch.equal(logits.argmax(dim=-1), base_class), "the boundary move changed a base class"


def test_sweep_counts_and_level_zero(cpu_double):
    g, m, clf, noise = _model()
    latents, smin, smax = g["out/latents"], g["out/minima"][0], g["out/maxima"][0]
    base_class = _split_classes(m.G, clf, latents, noise)
    _put_an_image_on_the_boundary(m.G, clf, latents, smin, smax, noise, base_class, 2.0)
    records = dict(latents=latents, minima=smin, maxima=smax, noise=g["out/noise"], original_images=g["out/original_images"])
    out = attfind.counterfactual_sweep(m, clf, records, EDITS, num_attributes=4, shift_size=2.0, image_batch=2)
    assert out["k"] == [1, 2, 3, 4] and "fid" not in out
    assert np.array_equal(out["base_class"], base_class.numpy()) and out["base_class"].dtype == np.int64
    flips = [0] * 4
    base_images = []
    for k, img, logits in attfind.counterfactual_images(m.G, clf, latents, EDITS[:4], smin, smax, noise, [0, 1, 2, 3, 4],
                                                        shift_size=2.0, image_batch=3):
        if k == 0:
            base_images.append(img)
            assert np.array_equal(logits.argmax(dim=-1).numpy(), base_class.numpy())
        else:
            flips[k - 1] += int((logits.argmax(dim=-1) != base_class).sum())
    assert out["flips"] == flips and out["flip_rate"] == [f / 3 for f in flips]
    assert flips[0] == 1 and sum(flips) < 12, flips  # the image put on the boundary flips with the first edit
    with torch.no_grad():
        want = m.G(attfind.styles_def_to_tensor([(torch.from_numpy(latents), m.G.num_layers)]), noise.expand(3, -1, -1, -1))
    assert torch.equal(torch.cat(base_images), want)  # level 0 is the base image
    # fewer edits than num_attributes: as many levels as there are edits
    assert attfind.counterfactual_sweep(m, clf, records, EDITS[:2], num_attributes=10)["k"] == [1, 2]
    with pytest.raises(ValueError):
        attfind.counterfactual_sweep(m, clf, records, [], num_attributes=3)


# ---- the table, the command line, the C entry point ---------------------------------------------------------------------


def test_write_fid_table_text(tmp_path):
    path = str(tmp_path / "t.csv")
    attfind.write_fid_table([12.3456], path)
    assert open(path).read() == ",Original-Generated\n0,12.35\n"
    attfind.write_fid_table([12.3456, 7.0], path)
    assert open(path).read() == ",Original-Generated,Original-Attribute 1\n0,12.35,7.00\n"
    attfind.write_fid_table([float(i) + 0.125 for i in range(11)], path)
    names = ["Original-Generated", "Original-Attribute 1"] + ["Original-Attributes 1-%d" % i for i in range(2, 11)]
    assert open(path).read() == "," + ",".join(names) + "\n0," + ",".join("%d.12" % i for i in range(11)) + "\n"


def cli_case(tmp_path, monkeypatch, n_images, bias_shift=0.0):
    """A saved 16 px checkpoint (built on the host), a folder of `n_images` PNGs and attfind_cli's argument list for them;
    attfind_cli.load_model is patched to hand the model the small stand-in classifier (the seeded ResNet-18 at 224 px is
    minutes of CPU time), its second bias lowered by `bias_shift`.  Returns (argv, output folder)."""
    import attfind_cli
    import stylex_train as st
    from PIL import Image
    from standins import TinyClassifier

    data = tmp_path / "imgs"
    data.mkdir()
    rng = np.random.RandomState(3)
    for i in range(n_images):
        Image.fromarray(rng.randint(0, 255, (20, 24, 3), dtype=np.uint8)).save(data / f"{i}.png")
    torch.manual_seed(17)
    prev = ops.use_impl(CpuOracleOps)
    try:
        tr = st.Trainer(name="cf", base_dir=str(tmp_path), classifier=TinyClassifier(seed=1), device=torch.device("cpu"),
                        tensorboard_dir=None, image_size=16, network_capacity=2, fmap_max=16)
        tr.init_StylEx()
        with torch.no_grad():
            for blk in tr.StylEx.G.blocks:
                for lin in (blk.to_noise1, blk.to_noise2):
                    lin.weight.normal_(0, 0.3)
        tr.save(0)
    finally:
        ops.use_impl(prev)
    load_model = attfind_cli.load_model

    def load_with_small_classifier(a, device_index):
        model = load_model(a, device_index)
        clf = TinyClassifier(seed=1, image_size=16)
        clf.b2 = clf.b2.clone()
        clf.b2[1] -= bias_shift
        model.classifier = clf.to(model.device)
        return model

    monkeypatch.setattr(attfind_cli, "load_model", load_with_small_classifier)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    argv = ["--name", "cf", "--models_dir", str(tmp_path / "models"), "--results_dir", str(tmp_path / "res"), "--data", str(data),
            "--load_from", "0", "--num_images", str(n_images), "--chunk", "64", "--num_indices", "2", "--max_images", "3",
            "--classifier_path", "None"]
    return argv, tmp_path / "res" / "cf" / "attfind"


def test_cli_flags_default_off_and_unknown_flags_still_rejected(cpu_double, tmp_path, monkeypatch):
    """--counterfactual_fid defaults to 0; with 0 the experiment's modules are not imported and neither file is written
    (the CLI on the CPU double, in this process); an unknown flag stops the CLI as before."""
    import attfind_cli

    assert attfind_cli.DEFAULTS["counterfactual_fid"] == 0 and attfind_cli.DEFAULTS["fid_weights"] is None
    assert attfind_cli.DEFAULTS["counterfactual_shift"] == 1.0
    with pytest.raises(SystemExit) as e:
        attfind_cli.main(["--counterfactual_fids", "2"])
    assert "unknown arguments: counterfactual_fids" in str(e.value)

    argv, folder = cli_case(tmp_path, monkeypatch, 3)
    called = []
    monkeypatch.setattr(attfind_cli, "counterfactual_experiment", lambda *a, **k: called.append(1))
    for name in ("fid", "fid_inception"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    attfind_cli.main(argv + ["--counterfactual_fid", "0"])
    assert (folder / "significant_styles.json").is_file()
    assert not (folder / "counterfactual_fid.csv").exists() and not (folder / "counterfactual.json").exists()
    assert not called and "fid" not in sys.modules and "fid_inception" not in sys.modules


def test_style_edit_entry_point_rejects_bad_arguments_before_the_device():
    """No GPU here: a call that got past validation would report a launch error, not -1."""
    lib = hip_backend.load_library()
    max_k = hip_backend.style_edit_max_k()
    assert max_k >= 11
    storage = ctypes.create_string_buffer(64)  # never read: every call below must stop at validation
    buf = ctypes.c_void_p(ctypes.addressof(storage))
    ptrs = [buf] * 9
    ok = [2, 5, 1, 1, 2]  # N, S, K, L, G
    for hole in range(9):
        args = list(ptrs)
        args[hole] = None
        assert lib.stylex_style_edit_levels(*args, *ok, 1.0, None) == -1, hole
    for at in range(5):
        for bad in (0, -1):
            sizes = list(ok)
            sizes[at] = bad
            assert lib.stylex_style_edit_levels(*ptrs, *sizes, 1.0, None) == -1, (at, bad)
    assert lib.stylex_style_edit_levels(*ptrs, 2, 5, max_k + 1, 1, 2, 1.0, None) == -1
    assert lib.stylex_style_edit_levels(*ptrs, 2, 5, 1, 1, 6, 1.0, None) == -1  # more segments than columns
    assert lib.stylex_style_edit_levels(*ptrs, 1 << 20, 5, 1, 1 << 12, 2, 1.0, None) == -1  # L * N past 2^31 - 1


def test_style_edit_wrapper_checks_what_the_device_cannot_report():
    coords, smin, smax = (torch.from_numpy(a) for a in _operands(n=2, s=5))
    base = torch.zeros(2, dtype=torch.int32)
    good = dict(sindex=[0, 4], direction=[0, 1], level_k=[0, 2], seg_start=[0, 2, 5])
    bad = [dict(sindex=[0, 5]), dict(sindex=[-1, 4]), dict(direction=[0, 2]), dict(direction=[0]), dict(level_k=[3]),
           dict(level_k=[-1]), dict(level_k=[]), dict(seg_start=[0, 5, 5]), dict(seg_start=[1, 5]), dict(seg_start=[0, 2, 4]),
           dict(seg_start=[0, 3, 2, 5]), dict(seg_start=[0]),
           dict(sindex=[0] * (hip_backend.style_edit_max_k() + 1), direction=[0] * (hip_backend.style_edit_max_k() + 1))]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(ValueError):
            hip_backend.style_edit_levels(coords, smin, smax, a["sindex"], a["direction"], base, a["level_k"], a["seg_start"], 1.0)
    with pytest.raises(hip_backend.StylexHipError):  # valid arguments, but host tensors: there is no CPU fallback
        hip_backend.style_edit_levels(coords, smin, smax, good["sindex"], good["direction"], base, good["level_k"],
                                      good["seg_start"], 1.0)
