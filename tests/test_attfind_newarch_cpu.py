"""AttFind on the conditional ("new") architecture, the threshold pass, the batched first pass, the record loader and
the command line — on the CPU test double, against tests/golden/attfind_newarch_16.npz (the reference notebook's
extraction cell executed with USE_OLD_ARCHITECTURE = False, tools/make_golden_attfind_newarch.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import attfind
import ops
import stylex_train as st
from cpu_ops import CpuOracleOps
from standins import TinyClassifier
from test_attfind_cpu import GOLD as GOLD_OLD
from test_attfind_cpu import build as build_old
from test_attfind_cpu import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "attfind_newarch_16.npz")
TOL = 2e-5  # what test_batched_engine_vs_reference_notebook_golden passes to check()


def build(g, conditional, device="cpu"):
    """test_attfind_cpu.build with the architecture flag: the seeded model of the fixture, its noise weights, the
    stand-in classifier, the images and the noise plane."""
    size, cap, fmax = (int(v) for v in g["config"])
    torch.manual_seed(int(g["seed"]))
    np.random.seed(int(g["seed"]))
    m = st.StylEx(size, network_capacity=cap, fmap_max=fmax, rank=0 if device != "cpu" else None, conditional=conditional)
    m.eval()
    flat, off = torch.from_numpy(g["noise_weights"]), 0
    for blk in m.G.blocks:
        for lin in (blk.to_noise1, blk.to_noise2):
            for t in (lin.weight, lin.bias):
                t.data = flat[off:off + t.numel()].view_as(t).clone().to(t.device)
                off += t.numel()
    clf = TinyClassifier(seed=99, image_size=size).to(device)
    images = [torch.from_numpy(g["images"][i:i + 1]).to(device) for i in range(g["images"].shape[0])]
    return m, clf, images, torch.from_numpy(g["input_noise"]).to(device)


def close(got, want, tol=TOL):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = max(1e-3, float(np.abs(want).max()))
    assert float(np.abs(got - want).max()) <= tol * scale, (float(np.abs(got - want).max()), scale)


@pytest.fixture()
def cpu_double():
    prev = ops.use_impl(CpuOracleOps)
    yield
    ops.use_impl(prev)


def test_conditional_extraction_vs_reference_notebook_golden(cpu_double, tmp_path):
    """w = cat(encoder, softmax(logits)), D(generated, probabilities=softmax(classify(generated))), base_prob the raw
    logits: all nine datasets of the notebook's USE_OLD_ARCHITECTURE = False branch, read from stylex.conditional; and
    the written records come back through load_records (cell 12)."""
    g = np.load(GOLD)
    m, clf, images, noise = build(g, True)
    assert m.conditional
    for chunk in (256, 10):
        out = attfind.attfind_extraction(m, clf, images, len(images), noise, shift_size=float(g["shift_size"]), chunk=chunk,
                                         results_folder=str(tmp_path))
        check(out, g, TOL)
    assert out["latents"].shape[1] == 514
    close(out["latents"][:, 512:].sum(dim=1), np.ones(3, dtype=np.float32))  # probabilities, not logits
    rec = attfind.load_records(str(tmp_path))
    for k in ("style_change", "latents", "base_prob", "style_coordinates", "original_images", "discriminator", "noise"):
        assert np.array_equal(rec[k], out[k].numpy()), k
    assert np.array_equal(rec["minima"], out["minima"].numpy()[0]) and np.array_equal(rec["maxima"], out["maxima"].numpy()[0])
    assert np.array_equal(rec["distances"], attfind.style_vector_distances(rec["style_coordinates"], rec["minima"], rec["maxima"]))
    rec2 = attfind.load_records(str(tmp_path), threshold_index=2)
    assert all(rec2[k].shape[0] == 2 for k in ("style_change", "latents", "base_prob", "style_coordinates",
                                               "original_images", "discriminator", "distances"))
    assert rec2["noise"].shape == rec["noise"].shape and np.array_equal(rec2["minima"], rec["minima"])


def test_conditional_flag_overrides_the_model_attribute(cpu_double):
    """conditional=None reads stylex.conditional; an explicit True on the same model is the same computation, an explicit
    False builds the latent from logits (the default architecture's branch) and so must differ."""
    g = np.load(GOLD)
    m, clf, images, noise = build(g, True)
    a = attfind.find_discriminator_threshold(m, clf, images, 3, noise)
    b = attfind.find_discriminator_threshold(m, clf, images, 3, noise, conditional=True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = attfind.attfind_extraction(m, clf, images[:1], 1, noise, conditional=False)
    assert not np.allclose(c["latents"][:, 512:].numpy(), g["out/latents"][:1, 512:], atol=1e-3)


def test_batched_first_pass_vs_golden(cpu_double):
    """first_pass_batch=2 over 3 images: one full and one ragged batch, against the FIXTURE (not the batch-1 run)."""
    g = np.load(GOLD)
    m, clf, images, noise = build(g, True)
    out = attfind.attfind_extraction(m, clf, images, len(images), noise, shift_size=float(g["shift_size"]), chunk=64,
                                     first_pass_batch=2)
    check(out, g, TOL)
    g_old = np.load(GOLD_OLD)
    m, clf, images, noise = build_old(g_old)
    for fpb in (2, 3, 8):
        out = attfind.attfind_extraction(m, clf, images, len(images), noise, shift_size=float(g_old["shift_size"]), chunk=64,
                                         first_pass_batch=fpb)
        check(out, g_old, TOL)


def test_default_path_unchanged(cpu_double):
    g = np.load(GOLD_OLD)
    m, clf, images, noise = build_old(g)
    a = attfind.attfind_extraction(m, clf, images, len(images), noise, shift_size=float(g["shift_size"]), chunk=64)
    b = attfind.attfind_extraction(m, clf, images, len(images), noise, shift_size=float(g["shift_size"]), chunk=64,
                                   first_pass_batch=1)
    assert set(a) == set(b) == set(attfind.DATASETS)
    for k in attfind.DATASETS:
        assert torch.equal(a[k], b[k]), k
    check(a, g, TOL)


@pytest.mark.parametrize("conditional", [True, False])
def test_threshold_pass_vs_reference_notebook_golden(cpu_double, tmp_path, conditional):
    g = np.load(GOLD)
    prefix = "thr/" if conditional else "thr_old/"
    m, clf, images, noise = build(g, conditional)
    for fpb in (1, 2):
        out = attfind.find_discriminator_threshold(m, clf, images, len(images), noise, first_pass_batch=fpb,
                                                   threshold_folder=str(tmp_path))
        assert set(out) == {"discriminator_outputs", "generated_images"}
        assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in out.values())
        for k in out:
            close(out[k], g[prefix + k])
    stored = attfind._read_datasets(str(tmp_path), "discriminator_threshold")
    assert set(stored) == set(out) and all(np.array_equal(stored[k], out[k].numpy()) for k in out)
    # the first num_images items only
    two = attfind.find_discriminator_threshold(m, clf, iter(images), 2, noise)
    close(two["discriminator_outputs"], g[prefix + "discriminator_outputs"][:2])
    assert two["generated_images"].shape == (2, 3, 16, 16)


@pytest.mark.parametrize("first_pass_batch", [1, 2])
def test_discriminator_filter_drops_the_images_below_the_threshold(cpu_double, first_pass_batch):
    """This repository's meaning of use_discriminator (the notebook's `skip` flag is inverted): an image whose
    discriminator output is below the threshold is absent, the others keep loader order and their golden rows."""
    g = np.load(GOLD)
    m, clf, images, noise = build(g, True)
    d = g["out/discriminator"].reshape(-1)
    order = np.sort(d)
    for lo, hi in zip(order[:-1], order[1:]):
        assert hi - lo > 100 * TOL * max(1.0, float(np.abs(d).max())), "the golden's discriminator outputs are too close to cut between"
        thr = float(lo + hi) / 2
        kept = np.nonzero(d >= thr)[0]
        assert 0 < len(kept) < len(d)
        out = attfind.attfind_extraction(m, clf, images, len(images), noise, shift_size=float(g["shift_size"]), chunk=64,
                                         discriminator_threshold=thr, use_discriminator=True, first_pass_batch=first_pass_batch)
        for k in ("latents", "base_prob", "style_coordinates", "original_images", "discriminator"):
            close(out[k], g["out/" + k][kept])
        close(out["minima"], g["out/style_coordinates"][kept].min(axis=0)[None])
        close(out["maxima"], g["out/style_coordinates"][kept].max(axis=0)[None])
        assert out["style_change"].shape == (len(kept),) + g["out/style_change"].shape[1:]
        # without use_discriminator the threshold is not applied
        full = attfind.attfind_extraction(m, clf, images, len(images), noise, shift_size=float(g["shift_size"]), chunk=64,
                                          discriminator_threshold=thr, first_pass_batch=first_pass_batch)
        check(full, g, TOL)
    with pytest.raises(ValueError):
        attfind.attfind_extraction(m, clf, images, len(images), noise, discriminator_threshold=float(order[-1]) + 1.0,
                                   use_discriminator=True, first_pass_batch=first_pass_batch)


def test_change_images_needs_no_architecture_branch(cpu_double):
    """Cells 17-21 work on the stored latents: on the golden's 514-wide conditional latents (probabilities inside)
    change_images reproduces G of those latents as the base image, and its changed image is the generator's output with
    the coordinate's style bias moved — whose get_style_coords reads the target at that coordinate."""
    g = np.load(GOLD)
    m, clf, _, noise = build(g, True)
    G = m.G
    w_all = torch.from_numpy(g["out/latents"])
    smin, smax = g["out/minima"][0], g["out/maxima"][0]
    with torch.no_grad():
        want_base, coords = G(attfind.styles_def_to_tensor([(w_all, G.num_layers)]), noise.expand(3, -1, -1, -1),
                              get_style_coords=True)
    close(coords, g["out/style_coordinates"])
    n_coords = int(g["n_coords"])
    for sindex, direction in ((0, 1), (n_coords // 2, 0), (n_coords - 1, 1)):
        base, changed, p0, p1 = attfind.change_images(G, clf, g["out/latents"], sindex, direction, smin[sindex], smax[sindex],
                                                      1.0, noise, class_index=1)
        close(base, want_base.numpy(), 1e-5)
        close(p0, torch.softmax(torch.from_numpy(g["out/base_prob"]), dim=1)[:, 1].numpy(), 1e-4)
        target = smin[sindex] if direction == 0 else smax[sindex]
        k, j = attfind._block_of(G, sindex)
        block = G.blocks[k]
        lin, j = (block.to_style1, j) if j < block.input_channels else (block.to_style2, j - block.input_channels)
        for i in range(3):
            delta = float(target - g["out/style_coordinates"][i, sindex])
            w_tensor = attfind.styles_def_to_tensor([(w_all[i:i + 1], G.num_layers)])
            with torch.no_grad():
                lin.bias[j] += delta
                want, moved = G(w_tensor, noise, get_style_coords=True)
                lin.bias[j] -= delta
            assert abs(float(moved[0, sindex]) - float(target)) <= 1e-5 * max(1.0, abs(float(target)))
            close(changed[i:i + 1], want.numpy(), 1e-5)
            # logits after a full shift = base logits + the sweep's entry for that image, coordinate and direction
            logits = clf.classify_images(changed[i:i + 1])[0].numpy()
            close(logits, g["out/base_prob"][i] + g["out/style_change"][i, direction, sindex], 1e-4)


# ---- command line ---------------------------------------------------------------------------------------------------

CLI_MODEL = dict(image_size=16, network_capacity=2, fmap_max=16)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _records(folder):
    return attfind._read_datasets(folder, "style_change_records")


@pytest.mark.timeout(900)
def test_attfind_cli_end_to_end_one_and_two_ranks(cpu_double, tmp_path):
    """python attfind_cli.py on a saved conditional checkpoint and a folder of three PNGs: records, significant_styles.json
    (= find_significant_styles on the records after split_by_class) and the strips; the threshold pass; then the same
    extraction under two gloo ranks (torch.distributed.run, and the --multi_gpus spawn), equal to the one-rank records."""
    from PIL import Image

    data = tmp_path / "imgs"
    data.mkdir()
    rng = np.random.RandomState(3)
    for i in range(3):
        Image.fromarray(rng.randint(0, 255, (20, 24, 3), dtype=np.uint8)).save(data / f"{i}.png")
    torch.manual_seed(17)
    tr = st.Trainer(name="cond", base_dir=str(tmp_path), classifier=TinyClassifier(seed=1), new_architecture=True,
                    device=torch.device("cpu"), tensorboard_dir=None, **CLI_MODEL)
    tr.init_StylEx()
    with torch.no_grad():
        for blk in tr.StylEx.G.blocks:
            for lin in (blk.to_noise1, blk.to_noise2):
                lin.weight.normal_(0, 0.3)
    tr.save(0)
    launcher = os.path.join(ROOT, "tests", "_attfind_cli_cpu_double.py")
    env = dict(os.environ, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)

    def flags(name):
        return ["--name", "cond", "--models_dir", str(tmp_path / "models"), "--results_dir", str(tmp_path / name),
                "--data", str(data), "--new_architecture", "--load_from", "0", "--num_images", "3", "--chunk", "64",
                "--num_indices", "3", "--max_image_effect", "0.2", "--split_by_class", "False", "--max_images", "3",
                "--classifier_path", "None"]

    def run(cmd, **kw):
        out = subprocess.run(cmd, env=dict(env, **kw), capture_output=True, text=True, timeout=800, cwd=str(tmp_path))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        return out

    run([sys.executable, launcher] + flags("r1") + ["--first_pass_batch", "2"])
    folder = str(tmp_path / "r1" / "cond" / "attfind")
    one = _records(folder)
    n_coords = sum(b.num_style_coords for b in tr.StylEx.G.blocks)
    assert one["style_change"].shape == (3, 2, n_coords, 2) and one["latents"].shape == (3, 514)
    assert np.abs(one["style_change"]).max() > 0
    np.testing.assert_allclose(one["latents"][:, 512:].sum(axis=1), 1.0, rtol=1e-5)  # the conditional branch ran
    sel = json.load(open(os.path.join(folder, "significant_styles.json")))
    rec = attfind.load_records(folder)
    split = attfind.split_by_class(rec["base_prob"], rec["style_change"], rec["latents"], rec["distances"], rec["style_coordinates"])
    for c in (0, 1):
        want = []
        if len(split[c]["index"]):
            want = attfind.find_significant_styles(split[c]["effect"], 3, c, max_image_effect=0.2)
        assert sel["class_%d" % c] == [[int(d), int(s)] for d, s in want], (c, sel)
    assert sel["class_0"] or sel["class_1"]
    pngs = sorted(f for f in os.listdir(folder) if f.endswith(".png"))
    assert pngs and pngs == sorted(sel["images"])
    strip = np.array(Image.open(os.path.join(folder, pngs[0])))
    assert strip.shape == (3 * 16, 2 * 16, 3) and strip.dtype == np.uint8

    out = run([sys.executable, launcher] + flags("thr") + ["--find_threshold"])
    assert "discriminator outputs of 3 images" in out.stdout
    thr = attfind._read_datasets(str(tmp_path / "thr" / "cond" / "attfind"), "discriminator_threshold")
    np.testing.assert_allclose(thr["discriminator_outputs"], one["discriminator"], rtol=1e-5, atol=1e-6)
    assert thr["generated_images"].shape == (3, 3, 16, 16)

    run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(_free_port()), launcher] + flags("r2") + ["--multi_gpus"])
    run([sys.executable, launcher] + flags("r2s") + ["--multi_gpus", "--num_gpus", "2"], MASTER_PORT=str(_free_port()))
    for name in ("r2", "r2s"):
        two = _records(str(tmp_path / name / "cond" / "attfind"))
        for k in attfind.DATASETS:  # the bound of test_sweep_sharded_over_two_ranks_gloo, relative to the dataset's max
            scale = max(1e-3, float(np.abs(one[k]).max()))
            assert two[k].shape == one[k].shape and float(np.abs(two[k] - one[k]).max()) <= TOL * scale, (name, k)
        assert json.load(open(str(tmp_path / name / "cond" / "attfind" / "significant_styles.json"))) == sel
