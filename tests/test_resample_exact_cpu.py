"""Exact device input pipeline, the part that needs no GPU: input_pipeline's integer restatement of PIL's 8-bit bilinear
resize against PIL itself, DevicePreprocessor on RawImageFolder items against the tensors the REFERENCE's Dataset returned
(tests/golden/dataset_items.npz) — torch.equal everywhere —, RNG ownership of RawImageFolder, host-side validation of the
resample entry points, and the register budget of csrc/resample_u8.hip."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import hip_backend
import input_pipeline as ip
import stylex_train as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ALPHAS = ("set", "uniform", "opaque")


def random_image(rng, h, w, c, alpha="uniform"):
    """uint8 [h, w, c] noise; the alpha plane of a 4-channel image from {0, 255, 7, 200}, uniform, or all 255."""
    a = rng.randint(0, 256, (h, w, c)).astype(np.uint8)
    if c == 4 and alpha == "set":
        a[..., 3] = rng.choice(np.array([0, 255, 7, 200], dtype=np.uint8), (h, w))
    elif c == 4 and alpha == "opaque":
        a[..., 3] = 255
    return a


def pil_resize(a, ow, oh):
    from PIL import Image

    return np.asarray(Image.fromarray(a).resize((ow, oh), Image.BILINEAR))


def test_composable_resize_equals_pil():
    rng = np.random.RandomState(11)
    cases = []
    for i in range(240):
        h, w = (int(v) for v in rng.randint(3, 91, 2))
        oh, ow = (int(v) for v in rng.randint(2, 71, 2))
        cases.append((h, w, oh, ow, 3 + i % 2, ALPHAS[(i // 2) % 3]))
    for c in (3, 4):
        cases += [(300, 400, 16, 16, c, "set"),  # ksize 39 / 51
                  (14, 20, 32, 45, c, "uniform"),  # up
                  (30, 40, 30, 17, c, "set"), (30, 40, 11, 40, c, "uniform"),  # one axis unchanged
                  (30, 40, 30, 40, c, "uniform")]  # nothing to do: a copy, no premultiplied round trip
    assert pil_bilinear_ksize(400, 16) == 51 and pil_bilinear_ksize(300, 16) == 39
    bad = []
    for h, w, oh, ow, c, alpha in cases:
        a = random_image(rng, h, w, c, alpha)
        got = ip.resize_u8(torch.from_numpy(a), ow, oh).numpy()
        if not np.array_equal(got, pil_resize(a, ow, oh)):
            bad.append((h, w, oh, ow, c, alpha))
    assert not bad, ("%d of %d resizes differ from PIL" % (len(bad), len(cases)), bad[:10])


def pil_bilinear_ksize(in_size, out_size):
    return ip.pil_bilinear_coeffs(in_size, out_size)[0]


def load_dataset_fixture(tmp_path):
    """tests/golden/dataset_items.npz -> (folder with the fixture's PNG files, fixture)."""
    from conftest import load_golden

    g = load_golden("dataset_items")
    d = tmp_path / "fixture_imgs"
    d.mkdir()
    for i in range(len(g["modes"])):
        (d / ("%02d.png" % i)).write_bytes(g["png_%02d" % i].tobytes())
    return d, g


LEGS = [("p0", dict(aug_prob=0.)), ("p1", dict(aug_prob=1.)), ("half", dict(aug_prob=0.5)), ("transparent", dict(transparent=True))]


def check_fixture_leg(device, tmp_path, tag, kw):
    """DevicePreprocessor on RawImageFolder items against the reference Dataset's own tensors, all 12, bit for bit; with
    aug_prob > 0 the global generators end where the reference's ended (same draws in the same order)."""
    folder, g = load_dataset_fixture(tmp_path)
    s = int(g["image_size"])
    raw = ip.RawImageFolder(str(folder), s, **kw)
    order = sorted(range(len(raw)), key=lambda k: raw.paths[k].name)
    seed = int(g["seed"])
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    items = [raw[k] for k in order]
    if kw.get("aug_prob"):
        assert random.random() == float(g["pyrandom_after_" + tag])
        assert torch.rand(()).item() == float(g["torchrand_after_" + tag])
        assert any(isinstance(it, tuple) for it in items)
    pre = ip.DevicePreprocessor(s, device)
    want = torch.from_numpy(g["items_" + tag])
    got = torch.stack([pre([it])[0].cpu() for it in items])
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = [i for i in range(len(order)) if not torch.equal(got[i], want[i])]
    assert not bad, ("items differing from the reference's", bad, [tuple(g["shapes"][i]) for i in bad])
    whole = pre(items).cpu()  # and as one ragged batch
    assert torch.equal(whole, want)


@pytest.mark.parametrize("tag,kw", LEGS)
def test_device_preprocessor_equals_reference_dataset_cpu(tmp_path, tag, kw):
    check_fixture_leg(torch.device("cpu"), tmp_path, tag, kw)


def test_private_generators_leave_the_globals_alone(tmp_path):
    folder, g = load_dataset_fixture(tmp_path)
    s = int(g["image_size"])

    def boxes(seed):
        ds = ip.RawImageFolder(str(folder), s, aug_prob=0.5, py_rng=random.Random(seed),
                               torch_rng=torch.Generator().manual_seed(seed))
        return [it[1] if isinstance(it, tuple) else None for it in (ds[k] for k in range(len(ds)))]

    torch.manual_seed(123)
    random.seed(123)
    np.random.seed(123)
    py_state, torch_state, np_state = random.getstate(), torch.get_rng_state(), np.random.get_state()
    a, b, c = boxes(77), boxes(77), boxes(78)
    assert a == b and a != c
    assert any(x is not None for x in a) and any(x is None for x in a)
    assert random.getstate() == py_state and torch.equal(torch.get_rng_state(), torch_state)
    assert all(np.array_equal(u, v) for u, v in zip(np_state, np.random.get_state()))
    # without a private pair the same class draws from the globals
    ds = ip.RawImageFolder(str(folder), s, aug_prob=1.0)
    ds[0]
    assert random.getstate() != py_state and not torch.equal(torch.get_rng_state(), torch_state)


def plan_for_validation():
    rng = np.random.RandomState(5)
    items = [torch.from_numpy(random_image(rng, 40, 64, 3)),  # resized, centre crop
             (torch.from_numpy(random_image(rng, 70, 33, 3)), (3, 1, 30, 29)),  # resized, box, second resize
             torch.from_numpy(random_image(rng, 37, 32, 3))]  # crop only
    plan = ip.BatchPlan(items, 32)
    assert [len(lst) for lst in plan.lists] == [2, 2, 1, 1, 1]
    return plan


def test_resample_entry_points_reject_bad_jobs_without_gpu():
    """STYLEX_EINVAL before the device is touched: null pointers, C outside {3, 4}, an empty window, a window outside the
    image.  Only invalid calls are made (a valid one would launch)."""
    lib = hip_backend.load_library()
    plan = plan_for_validation()
    J = ip.JOB_INTS
    fj = [int(v) for v in plan.first_job]
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its host-side check
    out_floats = plan.n * plan.c * 32 * 32

    def call(kind, table, src=fake, dst=fake, lut=fake, out=fake, tdev=fake, host=True):
        t = np.ascontiguousarray(table, dtype=np.int32)
        th = ctypes.c_void_p(t.ctypes.data) if host else None
        if kind == "rows":
            return lib.stylex_resample_rows_u8(th, tdev, t.size, fj[0], 2, src, plan.image_bytes, dst, plan.inter_px, None)
        if kind == "cols":
            return lib.stylex_resample_cols_u8(th, tdev, t.size, fj[1], 2, src, plan.inter_px * 4, dst, plan.stage1_px, lut, out,
                                               out_floats, None)
        return lib.stylex_crop_lut_u8(th, tdev, t.size, fj[4], 1, src, plan.image_bytes, lut, out, out_floats, None)

    def edited(job, field, value):
        t = plan.table.copy()
        t[job * J + field] = value
        return t

    first = {"rows": fj[0], "cols": fj[1], "crop": fj[4]}
    for kind in ("rows", "cols", "crop"):
        j = first[kind]
        assert call(kind, plan.table, host=False) == -1
        assert call(kind, plan.table, tdev=None) == -1
        assert call(kind, plan.table, src=None) == -1
        assert call(kind, edited(j, 4, 5)) == -1  # C = 5
        assert call(kind, edited(j, 4, 2)) == -1  # C = 2
        assert call(kind, edited(j, 7, plan.table[j * J + 6])) == -1  # o1 == o0: empty window
        assert call(kind, edited(j, 9, plan.table[j * J + 8])) == -1  # p1 == p0
        assert call(kind, edited(j, 9, 10 ** 6)) == -1  # window past the image
        assert call(kind, edited(j, 8, -1)) == -1
        assert call(kind, edited(j, 13, 2 ** 30)) == -1  # store outside the destination
        assert call(kind, edited(j, 0, 2 ** 30)) == -1  # image outside the source buffer
    assert call("rows", plan.table, dst=None) == -1
    assert call("cols", plan.table, dst=None, out=None) == -1
    assert call("cols", plan.table, lut=None) == -1
    assert call("crop", plan.table, out=None) == -1
    assert call("crop", edited(fj[4], 7, 38)) == -1  # rows [2, 38) of a 37-row image
    assert call("rows", edited(fj[0], 5, 40)) == -1  # taps shifted past the right edge
    assert call("cols", edited(fj[1], 5, -30)) == -1  # taps above the first row
    assert hip_backend.resample_supported(3, 1000, 3072, 100)
    assert not hip_backend.resample_supported(1, 1000, 1024, 100)
    assert not hip_backend.resample_supported(3, 2 ** 31, 3072, 100)


KERNELS = ["resample_rows_u8_kernel", "resample_cols_u8_kernel", "crop_lut_u8_kernel"]


@pytest.mark.skipif(not os.path.isfile(HIPCC), reason="needs hipcc")
def test_resample_kernels_use_no_scratch(tmp_path):
    """Same hipcc remarks and parsing as tests/test_attn_kernel_resources.py."""
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "resample_u8.hip"), "-o",
                          str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    seen = {}
    for blk in blocks:
        name = blk.split()[0]
        scratch = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk)
        spill = re.search(r"VGPRs Spill: (\d+)", blk)
        vgprs = re.search(r" VGPRs: (\d+)", blk)
        seen[name] = (int(scratch.group(1)) if scratch else None, int(spill.group(1)) if spill else None)
        print(name, "VGPRs", vgprs.group(1) if vgprs else "?", "scratch", seen[name][0])
    for k in KERNELS:
        hits = {n: v for n, v in seen.items() if k in n}
        assert hits, (k, sorted(seen))
        for n, (scratch, spill) in hits.items():
            assert scratch == 0 and spill == 0, (n, "scratch bytes/lane", scratch, "spilled VGPRs", spill)
