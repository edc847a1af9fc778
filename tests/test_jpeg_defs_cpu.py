"""The numpy definition of the device JPEG round trip (tests/_jpeg_defs.py; kernels: csrc/jpeg_rt.hip) against
Pillow itself where it is linked with libjpeg-turbo, and always against Pillow's recorded output
(tests/golden/jpeg_roundtrip.npz, tools/make_golden_jpeg.py); 32-bit arithmetic is enough; the three C entry points reject
bad arguments before they touch a device."""
import ctypes

import numpy as np
import pytest

import _jpeg_defs as jd
import hip_backend
from conftest import load_golden

SIZES = [(8, 8), (16, 16), (24, 40), (19, 21), (33, 17), (18, 22), (20, 18), (100, 60), (128, 128)]


def _needs_turbo():
    features = pytest.importorskip("PIL.features")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow is not linked with libjpeg-turbo: the recorded fixture is the yardstick here")


@pytest.mark.parametrize("kind", jd.KINDS)
@pytest.mark.parametrize("h,w", SIZES)
def test_definition_equals_pillow_at_quality_75(h, w, kind):
    _needs_turbo()
    im = jd.content(kind, h, w, seed=h * 131 + w)
    assert np.array_equal(jd.roundtrip_image(im, 75), jd.pillow_roundtrip(im, 75))


@pytest.mark.parametrize("quality", [10, 50, 90, 95, 100])
def test_definition_equals_pillow_at_other_qualities(quality):
    _needs_turbo()
    im = jd.content("noise", 40, 56, seed=quality)
    assert np.array_equal(jd.roundtrip_image(im, quality), jd.pillow_roundtrip(im, quality))


def test_definition_equals_the_recorded_pillow_output():
    z = load_golden("jpeg_roundtrip")
    cases = z["cases"]
    assert len(cases) >= 6 and str(z["pillow_version"])
    for i, (h, w, kind, q) in enumerate(cases):
        im, want = z["in_%d" % i], z["out_%d" % i]
        assert im.shape == (int(h), int(w), 3) and im.dtype == np.uint8
        assert np.array_equal(jd.roundtrip_image(im, int(q)), want), (h, w, kind, q, str(z["pillow_version"]))


def test_int32_and_int64_evaluations_agree():
    """libjpeg-turbo's SIMD paths work in 32-bit lanes, the kernels in 32-bit registers: nothing may need more, least of all
    saturated inputs at quality 100 (the largest coefficients, divisors of 8)."""
    for kind, q, (h, w) in [("saturated", 100, (40, 56)), ("saturated", 75, (19, 21)), ("noise", 100, (33, 17)),
                            ("noise", 1, (24, 40)), ("smooth", 95, (18, 22))]:
        im = jd.content(kind, h, w, seed=q + h)
        assert np.array_equal(jd.roundtrip_image(im, q, np.int32), jd.roundtrip_image(im, q, np.int64)), (kind, q)
    extreme = np.zeros((16, 16, 3), dtype=np.uint8)
    extreme[::2, 1::2] = 255  # a checkerboard of black and white: the largest high-frequency coefficients
    extreme[1::2, ::2] = 255
    assert np.array_equal(jd.roundtrip_image(extreme, 100, np.int32), jd.roundtrip_image(extreme, 100, np.int64))


def test_round_trip_changes_most_bytes_of_noise():
    """A kernel that copies its input cannot pass a comparison with the definition."""
    im = jd.content("noise", 64, 64, seed=5)
    assert float((jd.roundtrip_image(im, 75) != im).mean()) > 0.9


def test_batch_form_and_the_byte_of_a_float_image():
    x = np.random.RandomState(3).rand(2, 3, 19, 21).astype(np.float32) * 1.2 - 0.1
    q = jd.to_byte(x)
    assert q.dtype == np.uint8 and q.min() == 0 and q.max() == 255
    out = jd.roundtrip_batch(q, 75)
    assert out.shape == q.shape and np.array_equal(out[1].transpose(1, 2, 0), jd.roundtrip_image(q[1].transpose(1, 2, 0), 75))


def test_reciprocal_of_the_kernel_is_exact():
    """The kernel divides by d = 8 q with m = floor(2^27 / d) + 1: (n m) >> 27 == n // d for every numerator the quantiser
    forms (|c| + d / 2 < 2^16) and every divisor of a baseline table."""
    n = np.arange(1 << 16, dtype=np.uint64)
    for q in range(1, 256):
        d = np.uint64(8 * q)
        m = np.uint64((1 << 27) // (8 * q) + 1)
        assert np.array_equal((n * m) >> np.uint64(27), n // d), q


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = hip_backend.load_library()
    EINVAL = -1
    buf = (ctypes.c_double * 4096)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731
    ws_bytes = lib.stylex_jpeg_roundtrip_workspace_bytes
    assert ws_bytes(2, 19, 21) == 2 * 32 * 32 * 3 // 2 and ws_bytes(1, 256, 256) == 256 * 256 * 3 // 2
    assert ws_bytes(0, 16, 16) == -1 and ws_bytes(1, 7, 16) == -1 and ws_bytes(1, 16, 7) == -1
    sh, st, need = i64(2, 16, 16), i64(768, 256, 16, 1), ws_bytes(2, 16, 16)
    rt = lib.stylex_jpeg_roundtrip
    assert rt(None, p, sh, st, 0, 75, p, need, None) == EINVAL
    assert rt(p, None, sh, st, 0, 75, p, need, None) == EINVAL
    assert rt(p, p, None, st, 0, 75, p, need, None) == EINVAL
    assert rt(p, p, sh, None, 0, 75, p, need, None) == EINVAL
    assert rt(p, p, sh, st, 0, 75, None, need, None) == EINVAL
    assert rt(p, p, sh, st, 0, 0, p, need, None) == EINVAL            # quality outside 1..100
    assert rt(p, p, sh, st, 0, 101, p, need, None) == EINVAL
    assert rt(p, p, i64(2, 7, 16), st, 0, 75, p, need, None) == EINVAL  # planes below 8 samples
    assert rt(p, p, i64(2, 16, 4), st, 0, 75, p, need, None) == EINVAL
    assert rt(p, p, i64(0, 16, 16), st, 0, 75, p, need, None) == EINVAL
    assert rt(p, p, sh, st, 0, 75, p, need - 1, None) == EINVAL        # workspace too small
    assert rt(p, p, sh, st, 0, 75, ctypes.c_void_p(base + 4), need, None) == EINVAL  # ... or misaligned
    assert rt(p, p, sh, i64(768, 256, -16, 1), 0, 75, p, need, None) == EINVAL
    assert rt(p, p, sh, i64(1 << 31, 256, 16, 1), 1, 75, p, need, None) == EINVAL     # input offsets past 2^31
    prep = lib.stylex_fid_prep_u8
    sh5 = i64(2, 16, 16, 299, 299)
    assert prep(None, p, sh5, None) == EINVAL
    assert prep(p, None, sh5, None) == EINVAL
    assert prep(p, p, None, None) == EINVAL
    assert prep(p, p, i64(2, 0, 16, 299, 299), None) == EINVAL
    assert prep(p, p, i64(1 << 20, 8, 8, 299, 299), None) == EINVAL  # output past 2^31 elements
