"""Writes tests/golden/jpeg_roundtrip.npz: a handful of 8-bit RGB images and what Pillow (libjpeg-turbo) decodes from the
JPEG it writes of them — the recorded side of tests/test_jpeg_defs_cpu.py, which holds the numpy definition of the device
round trip (tests/_jpeg_defs.py) to these bytes wherever Pillow is absent or linked against another libjpeg.

    python tools/make_golden_jpeg.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _jpeg_defs as jd  # noqa: E402

# (height, width, content kind, quality)
CASES = [(8, 8, "noise", 75), (16, 16, "saturated", 75), (24, 40, "smooth", 75), (19, 21, "noise", 75), (33, 17, "smooth", 75),
         (18, 22, "saturated", 75), (20, 18, "noise", 75), (40, 56, "noise", 10), (40, 56, "noise", 50), (40, 56, "noise", 100),
         (40, 56, "saturated", 100)]


def main():
    import PIL
    from PIL import features

    assert features.check_feature("libjpeg_turbo"), "the fixture records libjpeg-turbo's output"
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_turbo_version": np.array(str(features.version("libjpeg_turbo"))),
           "cases": np.array(CASES, dtype=str)}
    for i, (h, w, kind, q) in enumerate(CASES):
        im = jd.content(kind, h, w, seed=1000 + i)
        out["in_%d" % i], out["out_%d" % i] = im, jd.pillow_roundtrip(im, q)
    path = os.path.join(ROOT, "tests", "golden", "jpeg_roundtrip.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes), Pillow %s, libjpeg-turbo %s" % (path, os.path.getsize(path), PIL.__version__, out["libjpeg_turbo_version"]))


if __name__ == "__main__":
    main()
