"""Exact device input pipeline on the GPU: the ragged-batch kernels of csrc/resample_u8.hip against input_pipeline's
definition in torch integer ops (itself held to PIL and to the reference Dataset's tensors by
tests/test_resample_exact_cpu.py) — torch.equal everywhere —, the four legs of tests/golden/dataset_items.npz on cuda:0,
the launch count per batch, the pinned staging ring under a Prefetcher that runs ahead, and a Trainer with
device_pipeline=True and dataset_aug_prob > 0."""
import random

import numpy as np
import pytest
import torch

import hip_backend as hb
import input_pipeline as ip
import stylex_train as st
from test_resample_exact_cpu import ALPHAS, LEGS, check_fixture_leg, random_image

pytestmark = [pytest.mark.gpu, pytest.mark.against_definition]

SIZES = [(20, 14), (70, 33), (33, 70), (64, 64), (257, 131), (400, 300), (32, 57), (37, 32)]  # (h, w)
CPU = torch.device("cpu")


def boxes_for(h, w, s):
    """Augmentation boxes (top, left, height, width) on the geometry after Resize(s): the four corners, the whole image,
    one pixel less than the whole image from either end, a box of exactly (s, s) (no second resize) and of (s - 1, s + 1)."""
    rw, rh = st.resize_geometry(w, h, s)
    ch, cw = max(rh * 3 // 4, 1), max(rw * 3 // 4, 1)
    out = [(0, 0, ch, cw), (0, rw - cw, ch, cw), (rh - ch, 0, ch, cw), (rh - ch, rw - cw, ch, cw), (0, 0, rh, rw),
           (0, 0, rh - 1, rw - 1), (1, 1, rh - 1, rw - 1), (rh - s, rw - s, s, s)]
    if rw > s:
        out.append((1, 0, s - 1, s + 1))
    return out


def ragged_batch(s, c, alpha, seed):
    """Every size, and one whose shorter side already is s, plain (centre crop) and with every box of boxes_for."""
    rng = np.random.RandomState(seed)
    items = []
    for h, w in SIZES + [(s, s + 5)]:
        img = torch.from_numpy(random_image(rng, h, w, c, alpha))
        items.append(img)
        items += [(img, b) for b in boxes_for(h, w, s)]
    return items


def input_launches():
    return {r["kernel"]: r["launches"] for r in hb.timing_kernels() if r["cls"] == "input"}


@pytest.mark.parametrize("s", [32, 16])
@pytest.mark.parametrize("c,alpha", [(3, "uniform")] + [(4, a) for a in ALPHAS])
def test_kernels_equal_the_definition_on_a_ragged_batch(s, c, alpha):
    items = ragged_batch(s, c, alpha, seed=100 * s + c)
    plan = ip.BatchPlan(items, s)
    assert all(len(lst) > 0 for lst in plan.lists), "the batch reaches all five launches"
    want = ip.DevicePreprocessor(s, CPU)(items)
    hb.timing_enable(1)
    got = ip.DevicePreprocessor(s, torch.device("cuda:0"))(items)
    torch.cuda.synchronize()
    launches = input_launches()
    assert launches == {"resample_rows_u8_kernel": 2, "resample_cols_u8_kernel": 2, "crop_lut_u8_kernel": 1}, launches
    assert got.shape == want.shape == (len(items), c, s, s) and got.dtype == torch.float32
    bad = [i for i in range(len(items)) if not torch.equal(got[i].cpu(), want[i])]
    assert not bad, ("items differing from the definition", bad)


@pytest.mark.parametrize("tag,kw", LEGS)
def test_device_preprocessor_equals_reference_dataset_gpu(tmp_path, tag, kw):
    check_fixture_leg(torch.device("cuda:0"), tmp_path, tag, kw)
    assert input_launches(), "the batch went through the kernels"


def test_launches_per_batch_do_not_grow_with_the_batch():
    rng = np.random.RandomState(9)
    pre = ip.DevicePreprocessor(32, torch.device("cuda:0"))

    def mix(n):  # pairs of: resized twice (four launches), already at the training size (one)
        items = []
        for _ in range(n // 2):
            items.append((torch.from_numpy(random_image(rng, 70, 33, 3)), (3, 1, 30, 29)))
            items.append(torch.from_numpy(random_image(rng, 32, 32, 3)))
        return items

    counts = []
    for n in (2, 8):
        items = mix(n)
        hb.timing_enable(1)
        got = pre(items)
        torch.cuda.synchronize()
        counts.append(sum(input_launches().values()))
        assert torch.equal(got.cpu(), ip.DevicePreprocessor(32, CPU)(items))
    assert counts[0] == counts[1] == 5 and counts[0] <= 6, counts


def test_staging_ring_under_a_prefetcher_that_runs_ahead():
    s, dev = 32, torch.device("cuda:0")
    rng = np.random.RandomState(21)
    batches = []
    for b in range(8):  # growing and shrinking batches: the ring's buffers are reallocated and reused
        sizes = [SIZES[(b + i) % len(SIZES)] for i in range(2 + (3 * b) % 5)]
        items = []
        for i, (h, w) in enumerate(sizes):
            img = torch.from_numpy(random_image(rng, h, w, 3))
            items.append((img, boxes_for(h, w, s)[(b + i) % 8]) if i % 2 else img)
        batches.append(items)
    want = [ip.DevicePreprocessor(s, CPU)(items) for items in batches]
    pre = ip.DevicePreprocessor(s, dev, ring_slots=3)
    got = list(ip.Prefetcher(iter(batches), pre, dev, depth=2))
    torch.cuda.synchronize()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g.cpu(), w), "batch %d" % i
    assert sum(buf is not None for buf in pre.ring.bufs) == 3


def make_mixed_folder(tmp_path):
    from PIL import Image

    rng = np.random.RandomState(3)
    d = tmp_path / "imgs"
    d.mkdir()
    for i, (h, w) in enumerate([(32, 32), (48, 40), (40, 64), (70, 33), (33, 70), (32, 57), (37, 32), (64, 64)]):
        Image.fromarray(random_image(rng, h, w, 3)).save(d / f"{i:02d}.png")
    return d


def test_trainer_with_device_pipeline_and_dataset_aug_prob(tmp_path):
    """Two identically seeded Trainers consume bit-identical batches (the loader's draws come from its private generators,
    not from the globals the training thread uses), and training on them gives finite losses."""
    import ops
    from lpips_standin import LPIPSStandIn
    from standins import TinyClassifier

    dev = torch.device("cuda:0")
    folder = make_mixed_folder(tmp_path)

    def build(name):
        torch.manual_seed(42)
        np.random.seed(42)
        random.seed(42)
        tr = st.Trainer(name=name, base_dir=str(tmp_path), image_size=32, network_capacity=4, fmap_max=64, batch_size=2,
                        gradient_accumulate_every=2, classifier=TinyClassifier(seed=99).to(dev),
                        lpips_fn=LPIPSStandIn(seed=4242).to(dev), classifier_name="resnet", evaluate_every=10 ** 9,
                        save_every=10 ** 9, device=dev, device_pipeline=True, dataset_aug_prob=0.5, num_workers=0)
        tr.set_data_src(str(folder))
        return tr

    try:
        firsts = []
        for name in ("a", "b"):
            tr = build(name)
            firsts.append([next(tr.loader).clone() for _ in range(4)])
            if name == "a":
                tr.loader.close()
        for x, y in zip(*firsts):
            assert x.is_cuda and x.shape == (2, 3, 32, 32) and torch.equal(x, y)
        assert tr.dataset.aug_prob == 0.5 and tr.dataset.torch_rng is not None
        tr.save = lambda *a, **k: None
        tr.evaluate = lambda *a, **k: None
        for _ in range(2):
            tr.train()
        assert np.isfinite([tr.d_loss, tr.g_loss, tr.total_rec_loss, tr.total_kl_loss]).all()
        tr.loader.close()
    finally:
        ops.set_precision("fp32")
