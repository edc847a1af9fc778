"""The numpy definition of the device JPEG round trip (csrc/jpeg_rt.hip): what libjpeg-turbo decodes from the
baseline JPEG it wrote of an 8-bit RGB image at quality q — 4:2:0, standard tables, the slow integer DCT (JDCT_ISLOW), fancy
upsampling — i.e. Pillow's ``save(format="JPEG", quality=q)`` -> ``open`` -> ``convert("RGB")``, without the (lossless)
entropy coder.  All arithmetic is integer; ``>>`` is the arithmetic shift; every function takes the integer type to
evaluate in (int64 by default, int32 to show that 32 bits are enough)."""
import numpy as np

# Annex K of the JPEG standard, natural (row-major) order
LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32).reshape(8, 8)

F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def fix(v):
    return int(v * 65536 + 0.5)


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def to_byte(x):
    """save_image's byte of a float image in [0, 1]: floor(clamp(x * 255 + 0.5, 0, 255)), two fp32 roundings."""
    x = np.asarray(x, dtype=np.float32)
    t = (x * np.float32(255)).astype(np.float32) + np.float32(0.5)
    return np.floor(np.clip(t, np.float32(0), np.float32(255))).astype(np.uint8)


def quant_tables(quality):
    """(luma, chroma) divisors [8, 8] of jpeg_set_quality(quality, force_baseline)."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA, CHROMA))


def _fdct_1d(d, first, dt):
    """jfdctint's butterfly along the last axis of d [..., 8]."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    out[2] = descale(z1 + t13 * F_0_765, n)
    out[6] = descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961, -z4 * F_0_390
    z3, z4 = z3 + z5, z4 + z5
    out[7], out[5] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n)
    out[3], out[1] = descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1).astype(dt)


def _idct_1d(c, n, dt):
    """jidctint's butterfly along the last axis of c [..., 8], results descaled by n bits."""
    c = [c[..., k] for k in range(8)]
    z2, z3 = c[2], c[6]
    z1 = (z2 + z3) * F_0_541
    t2, t3 = z1 - z3 * F_1_847, z1 + z2 * F_0_765
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961, -z4 * F_0_390
    z3, z4 = z3 + z5, z4 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([descale(o, n) for o in out], axis=-1).astype(dt)


def _codec_plane(p, q, dt):
    """A sample plane [h, w] (h, w multiples of 8) through forward DCT, quantisation by q [8, 8], dequantisation and
    the inverse DCT: the decoded plane, values in [0, 255]."""
    h, w = p.shape
    b = (p.astype(dt) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)  # [by, bx, row, col]
    b = _fdct_1d(b, True, dt)                                                    # rows
    b = _fdct_1d(b.transpose(0, 1, 3, 2), False, dt).transpose(0, 1, 3, 2)        # columns
    assert int(np.abs(b).max()) < 1 << 15
    q = q.astype(dt)
    d = 8 * q
    b = np.sign(b) * ((np.abs(b) + (d >> 1)) // d) * q
    b = _idct_1d(b.transpose(0, 1, 3, 2), 11, dt).transpose(0, 1, 3, 2)           # columns
    b = _idct_1d(b, 18, dt)                                                      # rows
    return np.clip(b + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def _pad_edge(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def roundtrip_image(rgb, quality=75, dt=np.int64):
    """rgb uint8 [H, W, 3] -> the decoded uint8 [H, W, 3]."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    assert H >= 8 and W >= 8, "planes below 8 samples take other upsampling paths in libjpeg"
    r, g, b = (rgb[..., k].astype(dt) for k in range(3))
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16
    Hm, Wm = -(-H // 16) * 16, -(-W // 16) * 16
    ch, cw = -(-H // 2), -(-W // 2)
    y = _pad_edge(y, Hm, Wm)
    planes = [y]
    bias = np.tile(np.array([1, 2], dtype=dt), Wm // 4)
    for c in (cb, cr):
        c = _pad_edge(c, 2 * ch, Wm)  # columns to the MCU width, rows to an even height only
        c = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        planes.append(_pad_edge(c, Hm // 2, Wm // 2))  # then the last DOWNSAMPLED row to the MCU height
    ql, qc = quant_tables(quality)
    y, cb, cr = (_codec_plane(p, q, dt) for p, q in zip(planes, (ql, qc, qc)))
    up = []
    for c in (cb, cr):
        c = c[:ch, :cw]
        above, below = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
        v = np.empty((2 * ch, cw), dtype=dt)
        v[0::2], v[1::2] = 3 * c + above, 3 * c + below
        left, right = np.concatenate([v[:, :1], v[:, :-1]], 1), np.concatenate([v[:, 1:], v[:, -1:]], 1)
        o = np.empty((2 * ch, 2 * cw), dtype=dt)
        o[:, 0::2], o[:, 1::2] = (3 * v + left + 8) >> 4, (3 * v + right + 7) >> 4
        up.append(o[:H, :W] - 128)
    y, (cb, cr) = y[:H, :W], up
    out = np.stack([y + ((fix(1.402) * cr + 32768) >> 16),
                    y + ((-fix(.34414) * cb + 32768 - fix(.71414) * cr) >> 16),
                    y + ((fix(1.772) * cb + 32768) >> 16)], axis=-1)
    assert out.dtype == dt
    return np.clip(out, 0, 255).astype(np.uint8)


def roundtrip_batch(x_u8, quality=75, dt=np.int64):
    """uint8 [B, 3, H, W] -> uint8 [B, 3, H, W]."""
    x_u8 = np.asarray(x_u8)
    return np.stack([roundtrip_image(im.transpose(1, 2, 0), quality, dt).transpose(2, 0, 1) for im in x_u8])


def pillow_roundtrip(rgb, quality=75):
    """The same through Pillow's encoder and decoder (in memory)."""
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, format="JPEG", quality=quality)
    buf.seek(0)
    return np.array(Image.open(buf).convert("RGB"))


def content(kind, h, w, seed):
    """The three kinds of test images, uint8 [h, w, 3]."""
    rng = np.random.RandomState(seed)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([128 + 100 * np.sin(xx / 7.0 + yy / 11.0), 128 + 90 * np.cos(xx / 5.0), 2.0 * xx + 1.5 * yy], -1)
        return np.clip(base + rng.randint(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
    assert kind == "saturated"
    return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


KINDS = ("noise", "smooth", "saturated")
