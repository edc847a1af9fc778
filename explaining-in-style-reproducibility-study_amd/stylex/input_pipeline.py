"""Device-side input pipeline for ``Trainer.set_data_src`` — opt-in with
``Trainer(device_pipeline=True)`` / ``STYLEX_DEVICE_PIPELINE=1``.

The reference's ``Dataset`` (stylex/stylex_train.py:520-556) decodes, resizes (shorter side -> image_size, PIL
bilinear), crops (centre, or a RandomResizedCrop box with probability aug_prob) and converts every image on the host,
inside DataLoader workers, and the training loop then uploads float32 batches (32 x 3 x 256 x 256 x 4 B = 25 MB per
micro-step) with a blocking ``.cuda()``.  Once the step is tens of milliseconds that is the first non-kernel
bottleneck.  Here:

* workers only DECODE (``RawImageFolder``: PIL -> uint8 HWC tensor, no resampling, 4x fewer bytes than float32) and,
  with aug_prob > 0, draw the item's crop box in the reference's order;
* a prefetch thread (``Prefetcher``) packs the decoded images of a batch into ONE pinned staging buffer (a small ring,
  guarded by events), uploads it with one copy on its own HIP stream and keeps ``depth`` preprocessed batches ready,
  so ``next(loader)`` in ``train()`` never waits for PCIe or the host;
* resize / crop / [0,1] scaling run on the GPU (``DevicePreprocessor``), in PIL's own byte arithmetic restated in
  integers (below): every tensor equals the reference Dataset's BIT FOR BIT — resampled or not, RGB or RGBA, centre
  crop or augmentation box (tests/test_resample_exact_cpu.py, tests/test_resample_exact_gpu.py).  The ragged batch
  runs through csrc/resample_u8.hip in a constant number of launches; CPU tensors, and anything
  ``hip_backend.resample_supported`` refuses, take the same arithmetic in torch integer ops.
  ``resample="float"`` (``STYLEX_RESAMPLE=float``) keeps the earlier ``F.interpolate`` path (<= 1.5/255 from the
  reference where an image is resampled) for A/B timing.

PIL's ``Image.resize(size, BILINEAR)`` on 8-bit images, the definition both paths implement:

* a horizontal pass, then a vertical pass, uint8 in and uint8 out each; a pass over an axis whose size does not change
  has the single coefficient 1 << 22 and is the identity;
* per axis in_size -> out_size, in float64: scale = in_size / out_size, fs = max(scale, 1), support = fs,
  ksize = 2 * ceil(support) + 1; for output index xx: center = (xx + 0.5) * scale,
  xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), in_size) - xmin,
  w[x] = tri((x + xmin - center + 0.5) * (1 / fs)) for x < xmax, each divided by their sum (added in index order),
  k[x] = int(0.5 + w[x] * (1 << 22));
* out = clip(((1 << 21) + sum_x in[xmin + x] * k[x]) >> 22, 0, 255) — an int32 sum;
* RGBA: colours are premultiplied before the two passes (t = c * a + 128; ((t >> 8) + t) >> 8) and divided out after
  them (c unchanged for a in {0, 255}, else min(255 * c // a, 255));
* a resize to the size the image already has is a copy (no premultiplied round trip).

The default (host) pipeline stays the parity path: step goldens never go through this file.
"""
import functools
import os
import queue
import threading
from pathlib import Path
from random import random as _global_random

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils import data

EXTS = ["jpg", "jpeg", "png"]
PRECISION_BITS = 22  # PIL: 32 - 8 - 2


class RawImageFolder(data.Dataset):
    """Decode only: returns the image as a uint8 [H, W, C] tensor (C = 3, or 4 with transparent=True).  With
    aug_prob > 0 every item draws one Python ``random()`` and, when selected, its RandomResizedCrop box on the geometry
    after Resize (the reference's order, stylex_train.Dataset) and is returned as ``(image, (top, left, height,
    width))``.  The draws come from the GLOBAL generators inside a DataLoader worker (the loader reseeds them per
    worker); in-process from the private pair (`py_rng`: random.Random, `torch_rng`: torch.Generator) when given."""

    def __init__(self, folder, image_size, transparent=False, aug_prob=0., py_rng=None, torch_rng=None):
        super().__init__()
        self.folder, self.image_size, self.transparent, self.aug_prob = folder, image_size, transparent, aug_prob
        self.py_rng, self.torch_rng = py_rng, torch_rng
        self.paths = [p for ext in EXTS for p in Path(f"{folder}").glob(f"**/*.{ext}")]
        assert len(self.paths) > 0, f"No images were found in {folder} for training"

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, index):
        from PIL import Image

        img = Image.open(self.paths[index]).convert("RGBA" if self.transparent else "RGB")
        arr = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())
        if not self.aug_prob:
            return arr
        from stylex_train import random_resized_crop_box, resize_geometry

        in_worker = data.get_worker_info() is not None
        py_rng = None if in_worker else self.py_rng
        torch_rng = None if in_worker else self.torch_rng
        if not (py_rng.random() if py_rng is not None else _global_random()) < self.aug_prob:
            return arr
        w, h = resize_geometry(img.size[0], img.size[1], self.image_size)
        return arr, random_resized_crop_box(w, h, generator=torch_rng)


def collate_raw(items):
    return list(items)  # images of a batch may differ in size until the device has resized them


def target_geometry(h, w, s):
    """(resized_h, resized_w, top, left) of Resize(s) + CenterCrop(s) — the arithmetic of stylex_train.Dataset
    (= torchvision 0.11.1 on PIL images: shorter side -> s, longer side int(s * long / short) TRUNCATED, an image whose
    shorter side already is s untouched; crop offsets int(round((side - s) / 2.0)), round-half-to-even)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == s:
        rw, rh = w, h
    else:
        new_long = int(s * long / short)
        rw, rh = (s, new_long) if w <= h else (new_long, s)
    return rh, rw, int(round((rh - s) / 2.0)), int(round((rw - s) / 2.0))


# ---- PIL's bilinear coefficients ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=256)
def pil_bilinear_coeffs(in_size, out_size):
    """(ksize, bounds int32 [out_size, 2] = (xmin, count), coefficients int32 [out_size, ksize]) of one axis, float64 on
    the host in PIL's operation order (module docstring).  Read-only arrays, cached per (in_size, out_size)."""
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(np.ceil(support)) + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    t = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    w = np.where((t < 1.0) & (x < xmax[:, None]), 1.0 - t, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]  # sequential, in index order (np.sum adds pairwise)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    k.setflags(write=False)
    return ksize, bounds, k


# ---- the definition in torch integer ops (CPU tensors, and whatever the kernels refuse) --------------------------------

def _resample_axis(img, axis, out_size):
    """One PIL pass over `axis` (0: vertical, 1: horizontal) of a uint8 [H, W, C] tensor."""
    in_size = img.shape[axis]
    ksize, bounds, k = pil_bilinear_coeffs(in_size, out_size)
    dev = img.device
    idx = torch.from_numpy(bounds[:, 0].astype(np.int64))[:, None] + torch.arange(ksize)[None, :]
    idx = idx.clamp_(max=in_size - 1).to(dev)  # taps past the count carry coefficient 0
    kk = torch.from_numpy(k.copy()).to(dev)
    if axis == 1:
        taps = img[:, idx, :].to(torch.int32)  # [H, out, ksize, C]
        acc = (taps * kk[None, :, :, None]).sum(dim=2, dtype=torch.int32)
    else:
        taps = img[idx, :, :].to(torch.int32)  # [out, ksize, W, C]
        acc = (taps * kk[:, :, None, None]).sum(dim=1, dtype=torch.int32)
    return ((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS).clamp_(0, 255).to(torch.uint8)


def premultiply_u8(img):
    """RGBA -> premultiplied (PIL rgbA2rgba, MULDIV255), alpha unchanged."""
    a = img[..., 3:4].to(torch.int32)
    t = img[..., :3].to(torch.int32) * a + 128
    return torch.cat([(((t >> 8) + t) >> 8).to(torch.uint8), img[..., 3:4]], dim=-1)


def unpremultiply_u8(img):
    """premultiplied -> RGBA (PIL rgba2rgbA): colours untouched at alpha 0 and 255, else min(255 * c // a, 255)."""
    a = img[..., 3:4].to(torch.int32)
    c = img[..., :3].to(torch.int32)
    q = torch.div(255 * c, a.clamp(min=1), rounding_mode="floor").clamp_(max=255)
    c = torch.where((a == 0) | (a == 255), c, q)
    return torch.cat([c.to(torch.uint8), img[..., 3:4]], dim=-1)


def resize_u8(img, ow, oh):
    """``Image.resize((ow, oh), BILINEAR)`` of a uint8 [H, W, C] tensor (C = 4: RGBA), bit for bit."""
    h, w, c = img.shape
    if (w, h) == (ow, oh):
        return img
    if c == 4:
        img = premultiply_u8(img)
    if ow != w:
        img = _resample_axis(img, 1, ow)
    if oh != h:
        img = _resample_axis(img, 0, oh)
    return unpremultiply_u8(img) if c == 4 else img


def split_item(item):
    """A batch item is a uint8 [H, W, C] tensor, or (tensor, (top, left, height, width)) with its augmentation box."""
    if isinstance(item, (tuple, list)):
        img, box = item
        return img, (None if box is None else tuple(int(v) for v in box))
    return item, None


def preprocess_item_u8(img, box, s):
    """uint8 [H, W, C] -> uint8 [s, s, C]: the transform chain of stylex_train.Dataset up to ToTensor."""
    from stylex_train import center_crop_offsets, resize_geometry

    h, w = img.shape[0], img.shape[1]
    rw, rh = resize_geometry(w, h, s)
    img = resize_u8(img, rw, rh)
    if box is not None:
        top, left, ch, cw = box
        return resize_u8(img[top:top + ch, left:left + cw], s, s)
    left, top = center_crop_offsets(rw, rh, s)
    return img[top:top + s, left:left + s]


# ---- ragged batch for csrc/resample_u8.hip -----------------------------------------------------------------------------

JOB_INTS = 20  # int32 fields of one job, mirrored by RsJob in csrc/resample_u8.hip
FLAG_PREMUL, FLAG_UNPREMUL, FLAG_LUT = 1, 2, 4
_ALIGN = 16


def _job(src_off, src_h, src_w, src_bpp, c, in0, o0, o1, p0, p1, bounds_off, coef_off, ksize, dst_off, dst_stride,
         dst_plane, flags):
    return [src_off, src_h, src_w, src_bpp, c, in0, o0, o1, p0, p1, bounds_off, coef_off, ksize, dst_off, dst_stride,
            dst_plane, flags, 0, 0, 0]


class BatchPlan:
    """Host side of one ragged batch: where each image sits in the staging buffer, the job lists of the (at most five)
    launches and the coefficient tables, laid out as ONE int32 table behind the images."""

    def __init__(self, items, s):
        from stylex_train import center_crop_offsets, resize_geometry

        self.s, self.n = s, len(items)
        self.images = []
        self.c = None
        tables, table_at, n_table = [], {}, 0
        off = 0
        # job lists: rows/cols of the first launch pair (source: staging buffer), rows/cols of the second pair (source: the
        # stage-1 images of augmented items that were resized first), plain crops
        rows1, cols1, rows2, cols2, crops = [], [], [], [], []
        inter1 = inter2 = stage1 = 0  # pixels of the 4-byte intermediates

        def table(in_size, out_size):
            nonlocal n_table
            key = (in_size, out_size)
            if key not in table_at:
                ksize, bounds, k = pil_bilinear_coeffs(in_size, out_size)
                table_at[key] = (n_table, n_table + bounds.size, ksize, bounds)
                tables.append(bounds.reshape(-1))
                tables.append(k.reshape(-1))
                n_table += bounds.size + k.size
            return table_at[key]

        def resize_jobs(rows, cols, inter, src_off, sh, sw, bpp, c, x0, y0, iw, ih, ow, oh, wx, wy, ww, wh, dst, flags):
            """Jobs of resizing the (x0, y0, iw, ih) box of a source image to (ow, oh), computing the output window
            (wx, wy, ww, wh) only; dst = (offset, stride, plane) in destination elements, source offsets in bytes.
            Returns the intermediate's new fill (pixels)."""
            hb_, hc_, hk, _ = table(iw, ow)
            vb_, vc_, vk, vbounds = table(ih, oh)
            r0 = int(vbounds[wy, 0])
            r1 = int(vbounds[wy + wh - 1, 0] + vbounds[wy + wh - 1, 1])
            pre = FLAG_PREMUL if c == 4 else 0
            post = FLAG_UNPREMUL if c == 4 else 0
            rows.append(_job(src_off, sh, sw, bpp, c, x0, wx, wx + ww, y0 + r0, y0 + r1, hb_, hc_, hk, inter, ww, 0, pre))
            cols.append(_job(inter * 4, r1 - r0, ww, 4, c, -r0, wy, wy + wh, 0, ww, vb_, vc_, vk, dst[0], dst[1], dst[2],
                             flags | post))
            return inter + (r1 - r0) * ww

        for i, item in enumerate(items):
            img, box = split_item(item)
            assert img.dtype == torch.uint8 and img.dim() == 3, "items are uint8 [H, W, C] tensors"
            h, w, c = (int(v) for v in img.shape)
            assert self.c in (None, c), "images of one batch share their channel count"
            self.c = c
            self.images.append((img, off))
            final = (i * c * s * s, s, s * s)
            rw, rh = resize_geometry(w, h, s)
            first = (rw, rh) != (w, h)
            if box is None:
                left, top = center_crop_offsets(rw, rh, s)
                if first:
                    inter1 = resize_jobs(rows1, cols1, inter1, off, h, w, c, c, 0, 0, w, h, rw, rh, left, top, s, s, final,
                                         FLAG_LUT)
                else:
                    crops.append(_job(off, h, w, c, c, 0, top, top + s, left, left + s, 0, 0, 0, *final, FLAG_LUT))
            else:
                top, left, ch, cw = box
                assert 0 <= top and 0 <= left and 0 < ch and 0 < cw and top + ch <= rh and left + cw <= rw, (box, rw, rh)
                second = (cw, ch) != (s, s)
                if first and second:
                    inter1 = resize_jobs(rows1, cols1, inter1, off, h, w, c, c, 0, 0, w, h, rw, rh, left, top, cw, ch,
                                         (stage1, cw, 0), 0)
                    inter2 = resize_jobs(rows2, cols2, inter2, stage1 * 4, ch, cw, 4, c, 0, 0, cw, ch, s, s, 0, 0, s, s, final,
                                         FLAG_LUT)
                    stage1 += ch * cw
                elif first:
                    inter1 = resize_jobs(rows1, cols1, inter1, off, h, w, c, c, 0, 0, w, h, rw, rh, left, top, s, s, final,
                                         FLAG_LUT)
                elif second:
                    inter1 = resize_jobs(rows1, cols1, inter1, off, h, w, c, c, left, top, cw, ch, s, s, 0, 0, s, s, final,
                                         FLAG_LUT)
                else:
                    crops.append(_job(off, h, w, c, c, 0, top, top + s, left, left + s, 0, 0, 0, *final, FLAG_LUT))
            off += (h * w * c + _ALIGN - 1) // _ALIGN * _ALIGN
        self.image_bytes = off
        self.lists = [rows1, cols1, rows2, cols2, crops]
        jobs = [j for lst in self.lists for j in lst]
        self.first_job = np.cumsum([0] + [len(lst) for lst in self.lists])
        base = len(jobs) * JOB_INTS  # the coefficient tables follow the jobs: shift their offsets
        jt = np.asarray(jobs, dtype=np.int64).reshape(-1, JOB_INTS)
        has_table = jt[:, 12] > 0
        jt[has_table, 10] += base
        jt[has_table, 11] += base
        assert jt.max(initial=0) < 2 ** 31 and jt.min(initial=0) > -2 ** 31
        self.table = np.concatenate([jt.astype(np.int32).reshape(-1)] + tables) if len(tables) else \
            jt.astype(np.int32).reshape(-1)
        self.inter_px, self.stage1_px = max(inter1, inter2), stage1
        self.total_bytes = self.image_bytes + self.table.size * 4

    def pack(self, buf):
        """Copy the images and the table into the uint8 host buffer `buf` (>= total_bytes)."""
        for img, off in self.images:
            n = img.numel()
            buf[off:off + n].copy_(img.reshape(-1))
        tb = torch.from_numpy(self.table).view(torch.uint8)
        buf[self.image_bytes:self.total_bytes].copy_(tb)


class StagingRing:
    """`slots` pinned host buffers, grown to the high-water mark, used round robin.  An event recorded after a slot's
    upload is waited for before the slot is rewritten: the prefetch thread runs ahead of the device."""

    def __init__(self, slots, pinned):
        self.pinned = pinned
        self.bufs = [None] * slots
        self.events = [None] * slots
        self.i = 0

    def acquire(self, nbytes):
        i = self.i
        self.i = (i + 1) % len(self.bufs)
        if self.events[i] is not None:
            self.events[i].synchronize()
            self.events[i] = None
        if self.bufs[i] is None or self.bufs[i].numel() < nbytes:
            self.bufs[i] = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=self.pinned)
        return i, self.bufs[i]

    def uploaded(self, i):
        ev = torch.cuda.Event()
        ev.record()
        self.events[i] = ev


class DevicePreprocessor:
    """Batch items (uint8 HWC host images, each optionally with its augmentation box) -> float [B, C, S, S] in [0, 1]
    on `device`.  resample="exact" (default): the reference Dataset's tensors bit for bit, through the HIP kernels on a
    GPU and through the same integer arithmetic in torch elsewhere; resample="float": F.interpolate (A/B timing)."""

    def __init__(self, image_size, device, resample=None, ring_slots=4):
        self.s, self.device = image_size, device
        self.resample = resample or os.environ.get("STYLEX_RESAMPLE", "exact")
        assert self.resample in ("exact", "float"), self.resample
        # value/255 for the 256 byte values, computed on the HOST in fp32 exactly as the host pipeline does: a device
        # division by a scalar is a multiplication by the rounded reciprocal (1 ulp off for some values)
        self.lut = (torch.arange(256, dtype=torch.float32) / 255.0).to(device)
        self.ring = StagingRing(ring_slots, pinned=device.type == "cuda")

    def __call__(self, items):
        if self.resample == "float":
            return self._float(items)
        if self.device.type == "cuda":
            import hip_backend

            plan = BatchPlan(items, self.s)
            if hip_backend.resample_supported(plan.c, plan.total_bytes, plan.n * plan.c * self.s * self.s,
                                              max(plan.inter_px, plan.stage1_px)):
                return self._kernels(plan)
        return self._composable(items)

    def upload(self, plan):
        """Pack the batch into the next pinned ring buffer and upload it with one copy: (host buffer, device copy)."""
        slot, host = self.ring.acquire(plan.total_bytes)
        plan.pack(host)
        dev = host[:plan.total_bytes].to(self.device, non_blocking=True)
        self.ring.uploaded(slot)
        return host, dev

    def _kernels(self, plan):
        import hip_backend

        host, dev = self.upload(plan)
        return hip_backend.resample_batch(plan, host, dev, self.lut)

    def _composable(self, items):
        out = []
        for item in items:
            img, box = split_item(item)
            x = preprocess_item_u8(img.to(self.device), box, self.s)
            out.append(self.lut[x.long()].permute(2, 0, 1))
        return torch.stack(out).contiguous()

    def upload_float(self, items):
        """resample="float", first half: one pinned copy and one upload per image."""
        cuda = self.device.type == "cuda"
        staged = []
        for item in items:
            im, box = split_item(item)
            assert box is None, 'resample="float" has no augmentation stage'
            if cuda:
                im = im.pin_memory()
            staged.append(im.to(self.device, non_blocking=True))
        return staged

    def float_on_device(self, staged):
        s, out = self.s, []
        for im in staged:
            h, w = im.shape[0], im.shape[1]
            rh, rw, top, left = target_geometry(h, w, s)
            if (rh, rw) == (h, w):  # no resampling: table lookup, bit-identical to the host path
                x = self.lut[im[top:top + s, left:left + s].long()].permute(2, 0, 1).unsqueeze(0)
            else:
                x = F.interpolate(im.permute(2, 0, 1).unsqueeze(0).float(), size=(rh, rw), mode="bilinear",
                                  align_corners=False, antialias=True)
                x = x[:, :, top:top + s, left:left + s] / 255.0
            out.append(x)
        return torch.cat(out, dim=0).contiguous()

    def _float(self, items):
        return self.float_on_device(self.upload_float(items))


class Prefetcher:
    """Iterator over preprocessed device batches, produced `depth` ahead by a background thread on its own HIP stream.
    `source` is any iterator of host batches (lists of uint8 images, or ready tensors), `prepare` turns one into a
    device tensor.  next() hands the batch to the caller's current stream (event wait + record_stream)."""

    def __init__(self, source, prepare, device, depth=3):
        self.source, self.prepare, self.device = source, prepare, device
        self.q = queue.Queue(maxsize=depth)
        self.stream = torch.cuda.Stream(device=device) if device.type == "cuda" else None
        self._stop = False
        self.thread = threading.Thread(target=self._run, daemon=True, name="stylex-prefetch")
        self.thread.start()

    def _run(self):
        try:
            if self.stream is not None:
                torch.cuda.set_device(self.device)
            for host in self.source:
                if self._stop:
                    return
                if self.stream is not None:
                    with torch.cuda.stream(self.stream):
                        batch = self.prepare(host)
                        ev = torch.cuda.Event()
                        ev.record(self.stream)
                else:
                    batch, ev = self.prepare(host), None
                self.q.put((batch, ev))
            self.q.put((None, None))
        except BaseException as e:  # noqa: BLE001 — surfaced on the consumer side
            self.q.put((e, None))

    def __iter__(self):
        return self

    def __next__(self):
        batch, ev = self.q.get()
        if batch is None:
            raise StopIteration
        if isinstance(batch, BaseException):
            raise batch
        if ev is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            batch.record_stream(cur)
        return batch

    def close(self):
        self._stop = True
        try:
            while True:
                self.q.get_nowait()
        except queue.Empty:
            pass


def cycle(iterable):
    while True:
        for i in iterable:
            yield i


def make_device_loader(folder, image_size, batch_size, device, num_workers=0, transparent=False, sampler=None,
                       shuffle=True, depth=3, generator=None):
    """DataLoader over decoded images -> Prefetcher of preprocessed device batches; returns (iterator, dataset).
    `folder` may be an already built RawImageFolder (the Trainer sizes its DistributedSampler from it first).
    `generator`: the torch.Generator the loader draws its shuffles and worker seeds from — the loader is iterated on
    the prefetch thread, where draws from the global generator would race with the caller's."""
    ds = folder if isinstance(folder, RawImageFolder) else RawImageFolder(folder, image_size, transparent=transparent)
    loader = data.DataLoader(ds, num_workers=num_workers, batch_size=batch_size, sampler=sampler,
                             shuffle=shuffle and sampler is None, drop_last=True, collate_fn=collate_raw,
                             generator=generator)
    pre = DevicePreprocessor(image_size, device, ring_slots=depth + 1)
    return Prefetcher(cycle(loader), pre, device, depth=depth), ds
