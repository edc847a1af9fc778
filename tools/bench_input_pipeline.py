"""A/B of the device input pipeline's two resampling paths (stylex/input_pipeline.py): resample="exact" (PIL's byte
arithmetic in csrc/resample_u8.hip, one staging upload and at most five launches per batch) against resample="float"
(F.interpolate per image).  Per shape, B = 32, in ONE process after warm-up, alternating exact / float / float / exact:

* device time of the preprocessing alone, hipEvents around it with the batch already uploaded;
* host clock around pre(batch) (packing / pinning, upload, launches) ending in a device synchronise;
* launches of the library per batch, from the timing hook (the float path launches torch kernels only).

    python tools/bench_input_pipeline.py [--out profiles/input_pipeline_resample_ab.txt] [--rounds 20]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd")
for p in (ROOT, PKG, os.path.join(PKG, "stylex")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hip_backend as hb  # noqa: E402
import input_pipeline as ip  # noqa: E402

SHAPES = [(218, 178, 128, "CelebA 218x178 -> 128"), (1024, 1024, 256, "FFHQ 1024x1024 -> 256"),
          (256, 256, 256, "256x256 -> 256 (pass-through)")]


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def bench_shape(h, w, s, batch, rounds, dev):
    rng = np.random.RandomState(1)
    items = [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)) for _ in range(batch)]
    pre = {"exact": ip.DevicePreprocessor(s, dev, resample="exact"), "float": ip.DevicePreprocessor(s, dev, resample="float")}
    plan = ip.BatchPlan(items, s)
    assert hb.resample_supported(plan.c, plan.total_bytes, plan.n * plan.c * s * s, max(plan.inter_px, plan.stage1_px))
    host, dev_buf = pre["exact"].upload(plan)
    staged = pre["float"].upload_float(items)
    torch.cuda.synchronize()
    on_device = {"exact": lambda: hb.resample_batch(plan, host, dev_buf, pre["exact"].lut),
                 "float": lambda: pre["float"].float_on_device(staged)}
    whole = {k: (lambda k=k: pre[k](items)) for k in pre}
    diff = float((on_device["exact"]() - on_device["float"]()).abs().max()) * 255
    for _ in range(3):  # warm-up: code objects, allocator, pinned ring
        for k in pre:
            on_device[k]()
            whole[k]()
    torch.cuda.synchronize()
    hb.timing_enable(1)
    whole["exact"]()
    torch.cuda.synchronize()
    launches = {r["kernel"]: r["launches"] for r in hb.timing_kernels() if r["cls"] == "input"}
    hb.timing_enable(0)
    order = ("exact", "float", "float", "exact")
    dms = {(k, slot): [] for slot, k in enumerate(order)}
    hms = {(k, slot): [] for slot, k in enumerate(order)}
    for _ in range(rounds):
        for slot, k in enumerate(order):
            dms[(k, slot)].append(device_ms(on_device[k]))
        for slot, k in enumerate(order):
            hms[(k, slot)].append(host_ms(whole[k]))
    out = {"launches": launches, "max_abs_diff_in_bytes": diff}
    for name, table in (("device_ms", dms), ("host_ms", hms)):
        for k in ("exact", "float"):
            meds = [statistics.median(v) for (kk, _), v in table.items() if kk == k]
            out[name + "_" + k] = statistics.median([x for (kk, _), v in table.items() if kk == k for x in v])
            out[name + "_" + k + "_slots"] = meds
            out[name + "_" + k + "_spread"] = max(meds) - min(meds)  # same path, two slots of the A/B/B/A pattern
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_pipeline_resample_ab.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    hb.load_library()
    lines = ["# tools/bench_input_pipeline.py: resample=exact (csrc/resample_u8.hip) vs resample=float (F.interpolate), B = %d, RGB,"
             % a.batch,
             "# %d rounds of exact / float / float / exact after warm-up, %s; medians in ms; spread = difference of the medians"
             % (a.rounds, torch.cuda.get_device_name(0)),
             "# of the two slots of the SAME path.  device = hipEvents around the preprocessing with the batch already uploaded;",
             "# host = wall clock around pre(batch) (pack / pin, upload, launches) ending in a device synchronise."]
    for h, w, s, label in SHAPES:
        r = bench_shape(h, w, s, a.batch, a.rounds, dev)
        lines.append("")
        lines.append("%s" % label)
        lines.append("  library launches per batch (exact): %d  %s" % (sum(r["launches"].values()), r["launches"]))
        lines.append("  max |exact - float| = %.3f / 255" % r["max_abs_diff_in_bytes"])
        for name in ("device_ms", "host_ms"):
            for k in ("exact", "float"):
                lines.append("  %-9s %-5s median %8.3f   slots %s   spread %.3f" % (
                    name, k, r[name + "_" + k], " ".join("%8.3f" % v for v in r[name + "_" + k + "_slots"]),
                    r[name + "_" + k + "_spread"]))
            lines.append("  %-9s exact - float = %+.3f ms (float's own spread %.3f)" % (
                name, r[name + "_exact"] - r[name + "_float"], r[name + "_float_spread"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
