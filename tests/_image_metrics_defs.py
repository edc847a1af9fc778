"""Float64 definitions of the image-pair statistics (csrc/image_metrics.hip, hip_backend.image_pair_stats), written from
the formulas and independent of the kernel's pass structure; an fp32 model OF that pass structure, whose error against the
definition sets the SSIM limit of tests/test_image_metrics_gpu.py; and the input cases both test files share.

Definition (Wang et al. 2004, as the common packages compute it): per channel, an 11 x 11 Gaussian window (sigma 1.5,
normalised to sum 1) at the (H - 10) x (W - 10) valid positions; mu = E[.], population (co)variances E[..] - mu mu;
SSIM = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_x^2 + s_y^2 + C2)), C1 = 0.01^2, C2 = 0.03^2 (data
range 1); the mean over positions and channels.  Values: the byte an image file would hold, floor(clamp(v * 255 + 0.5, 0,
255)) with v * 255 + 0.5 evaluated exactly and rounded once to fp32 (include/stylex_hip.h: the byte of stylex_fid_prep), over
255; or clamp(v, 0, 1)."""
import functools

import numpy as np
import torch

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
FAMILIES = ("noise", "ramp", "outside")


def gaussian(size=WIN, sigma=SIGMA, normalise=True):
    d = np.arange(size, dtype=np.float64) - size // 2
    g = np.exp(-d * d / (2.0 * sigma * sigma))
    return g / g.sum() if normalise else g


# ---- value rules ------------------------------------------------------------------------------------------------------------

def _f32(t, channels):
    """The first `channels` planes of a torch tensor (fp32 or bf16, any strides) as a dense fp32 array: both exact."""
    return np.ascontiguousarray(t.detach().cpu()[:, :channels].float().numpy())


def byte_rule(v32):
    """fp32 array -> the bytes of the image file, as fp64."""
    t = (v32.astype(np.float64) * 255.0 + 0.5).astype(np.float32)  # 24 + 8 bits: the product is exact in fp64
    return np.floor(np.clip(t, np.float32(0.0), np.float32(255.0))).astype(np.float64)


def clamp_rule(v32):
    return np.clip(v32, np.float32(0.0), np.float32(1.0)).astype(np.float64)


# ---- SSIM in fp64 -----------------------------------------------------------------------------------------------------------

def ssim_map_direct(x, y):
    """x, y fp64 [..., H, W] -> SSIM at the valid positions [..., H - 10, W - 10], one non-separable 2-D window sum."""
    g = gaussian()
    w2 = np.outer(g, g)
    win = lambda a: np.einsum("...ij,ij->...", np.lib.stride_tricks.sliding_window_view(a, (WIN, WIN), axis=(-2, -1)), w2)  # noqa: E731
    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def ssim_map_separable(x, y):
    """The same with the window applied along W, then along H."""
    g = gaussian()

    def win(a):
        h = np.einsum("...k,k->...", np.lib.stride_tricks.sliding_window_view(a, WIN, axis=-1), g)
        return np.einsum("...k,k->...", np.lib.stride_tricks.sliding_window_view(h, WIN, axis=-2), g)

    mx, my = win(x), win(y)
    sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))


def pair_stats(x, y, channels=3, quantise=True):
    """The definition of hip_backend.image_pair_stats on two torch tensors: a dict of fp64 [B] arrays — sum_abs and sum_sq
    (of byte differences with `quantise`), mae, mse, psnr (data range 1; inf at mse 0) and ssim."""
    a, b = _f32(x, channels), _f32(y, channels)
    if quantise:
        da, db = byte_rule(a), byte_rule(b)
        va, vb, scale = da / 255.0, db / 255.0, 255.0
    else:
        da, db = clamp_rule(a), clamp_rule(b)
        va, vb, scale = da, db, 1.0
    d = da - db
    n = float(d[0].size)
    sum_abs, sum_sq = np.abs(d).sum((1, 2, 3)), (d * d).sum((1, 2, 3))
    mse = sum_sq / (scale * scale * n)
    with np.errstate(divide="ignore"):
        psnr = np.where(mse > 0, 10.0 * np.log10(1.0 / np.where(mse > 0, mse, 1.0)), np.inf)
    return dict(sum_abs=sum_abs, sum_sq=sum_sq, mae=sum_abs / (scale * n), mse=mse, psnr=psnr,
                ssim=ssim_map_direct(va, vb).mean((1, 2, 3)))


# ---- the fp32 model of the kernel's passes -----------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in fp64, the sum is rounded to fp64 and then to fp32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def ssim_model_fp32(x, y, channels=3, quantise=True, tile=16, mutation=None):
    """Per-image SSIM as the kernel computes it: values staged as fp32 under the value rule; a horizontal pass of x, y, x^2,
    y^2, xy (one fmaf per tap, squares and the product rounded on their own), the vertical pass of the five rows, the
    quotient in fp32 — then fp64: the sum over positions and channels and the division by their number.
    `mutation`: one wrong reading of the definition, for the tests that show the limit tells them apart —
    'same_padding', 'unnormalised', 'sigma_1', 'sample_covariance', 'c2_0.03', 'drop_last_channel', 'short_halo' (the tile's
    halo lacks its last column: the last tap of the positions in a tile's last column reads zero)."""
    a, b = _f32(x, channels), _f32(y, channels)
    if quantise:
        va = (byte_rule(a).astype(np.float32) / np.float32(255.0)).astype(np.float32)
        vb = (byte_rule(b).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    else:
        va, vb = clamp_rule(a).astype(np.float32), clamp_rule(b).astype(np.float32)
    if mutation == "drop_last_channel" and channels > 1:
        va, vb = va[:, :-1], vb[:, :-1]
    if mutation == "same_padding":
        pad = [(0, 0), (0, 0), (WIN // 2, WIN // 2), (WIN // 2, WIN // 2)]
        va, vb = np.pad(va, pad), np.pad(vb, pad)
    g = gaussian(sigma=1.0 if mutation == "sigma_1" else SIGMA, normalise=mutation != "unnormalised").astype(np.float32)
    c1 = np.float32(0.01) * np.float32(0.01)
    c2 = np.float32(0.03) if mutation == "c2_0.03" else np.float32(0.03) * np.float32(0.03)
    H, W = va.shape[-2:]
    Ho, Wo = H - WIN + 1, W - WIN + 1
    zero = np.zeros(va.shape[:-1] + (Wo,), np.float32)
    h = [zero, zero, zero, zero, zero]
    last_col = (np.arange(Wo) % tile) == tile - 1
    for k in range(WIN):
        p, q = va[..., k:k + Wo], vb[..., k:k + Wo]
        if mutation == "short_halo" and k == WIN - 1:
            p, q = np.where(last_col, np.float32(0), p), np.where(last_col, np.float32(0), q)
        h = [_fma32(g[k], p, h[0]), _fma32(g[k], q, h[1]), _fma32(g[k], p * p, h[2]), _fma32(g[k], q * q, h[3]),
             _fma32(g[k], p * q, h[4])]
    zero = np.zeros(va.shape[:-2] + (Ho, Wo), np.float32)
    v = [zero, zero, zero, zero, zero]
    for k in range(WIN):
        v = [_fma32(g[k], h[i][..., k:k + Ho, :], v[i]) for i in range(5)]
    mx, my, exx, eyy, exy = v
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sxx, syy, sxy = exx - mxx, eyy - myy, exy - mxy
    if mutation == "sample_covariance":
        n = np.float32(WIN * WIN)
        sxx, syy, sxy = sxx * (n / (n - 1)), syy * (n / (n - 1)), sxy * (n / (n - 1))
    a1, a2 = _fma32(np.float32(2), mxy, c1), _fma32(np.float32(2), sxy, c2)
    b1, b2 = (mxx + myy) + c1, (sxx + syy) + c2
    quot = (a1 * a2) / (b1 * b2)
    assert quot.dtype == np.float32
    return quot.astype(np.float64).mean((1, 2, 3))


MUTATIONS = ("same_padding", "unnormalised", "sigma_1", "sample_covariance", "c2_0.03", "drop_last_channel", "short_halo")


# ---- the inputs of the per-element tests ------------------------------------------------------------------------------------

def family_pair(family, shape, seed):
    """(x, y) fp32 CPU tensors of `shape` = (B, C, H, W): an image and a disturbed copy of it."""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    if family == "noise":  # Gaussian noise around 0.5
        x = 0.5 + 0.2 * torch.randn(shape, generator=g)
        y = x + 0.05 * torch.randn(shape, generator=g)
    elif family == "ramp":  # a smooth ramp with small noise: flat regions, where E[x^2] - mu^2 cancels worst
        ramp = torch.linspace(0.1, 0.9, W).view(1, 1, 1, W) * torch.linspace(0.5, 1.0, H).view(1, 1, H, 1)
        x = ramp + 0.002 * torch.randn(shape, generator=g)
        y = ramp + 0.002 * torch.randn(shape, generator=g)
    elif family == "outside":  # values outside [0, 1]: the clamp
        x = torch.rand(shape, generator=g) * 1.6 - 0.3
        y = x + 0.1 * torch.randn(shape, generator=g)
    else:
        raise ValueError(family)
    return x.contiguous(), y.contiguous()


def shapes(tile):
    """(B, planes, H, W, channels) of the per-element cases: a single window, one more column, one tile row exactly, a tile
    boundary crossed by one in each direction with unequal sides, three tile rows of one column, 64 px; B 1 and 5; 1, 3
    and 4 channels and a 4-plane input of which 3 are read."""
    T = tile
    return [(1, 3, 11, 11, 3), (1, 1, 11, 12, 1), (5, 3, 11, T + 10, 3), (1, 4, T + 9, T + 11, 4), (5, 4, 2 * T + 11, 11, 3),
            (1, 3, 64, 64, 3)]


OPERANDS = ("f32_f32", "f32_bf16cl", "sliced")


def make_operands(kind, x, y):
    """The operand forms of the GPU test, made on the CPU so that the definition sees the very values the kernel reads:
    dense fp32 pair; fp32 with a bf16 channels-last second operand; both as sliced views (non-zero storage offset,
    non-unit batch stride) of larger tensors."""
    if kind == "f32_f32":
        return x, y
    if kind == "f32_bf16cl":
        return x, y.bfloat16().contiguous(memory_format=torch.channels_last)
    if kind == "sliced":
        def view(t):
            big = torch.full((2 * t.shape[0] + 1, t.shape[1] + 1) + tuple(t.shape[2:]), 7.0)
            v = big[1::2, 1:]
            v.copy_(t)
            return v

        return view(x), view(y)
    raise ValueError(kind)


def cases(tile):
    """Every per-element case: (family, operand kind, quantise, channels, x, y), x and y CPU tensors as the kernel gets them."""
    out = []
    for fi, family in enumerate(FAMILIES):
        for si, (B, planes, H, W, channels) in enumerate(shapes(tile)):
            kind = OPERANDS[(fi + si) % len(OPERANDS)] if (H, W) != (64, 64) else None
            for k in (OPERANDS if kind is None else (kind,)):
                x, y = family_pair(family, (B, planes, H, W), 100 * fi + si)
                xo, yo = make_operands(k, x, y)
                for quantise in (True, False):
                    out.append((family, k, quantise, channels, xo, yo))
    return out


@functools.lru_cache(maxsize=None)
def model_errors(tile):
    """family -> the worst per-image |SSIM of the fp32 model - SSIM of the fp64 definition| over that family's cases."""
    worst = {f: 0.0 for f in FAMILIES}
    for family, _, quantise, channels, x, y in cases(tile):
        want = pair_stats(x, y, channels, quantise)["ssim"]
        got = ssim_model_fp32(x, y, channels, quantise, tile)
        worst[family] = max(worst[family], float(np.abs(got - want).max()))
    return worst


def ssim_limit(tile):
    """The SSIM limit of the GPU test: 4 x the worst measured error of the fp32 model against the definition over all the
    families (the factor covers another summation order inside a tile).  Measured against the definition, never against
    the kernel."""
    return 4.0 * max(model_errors(tile).values())


SUM_REL_BOUND = 2.0 ** -22  # quantise = 0: |d| one fp32 rounding, d^2 three (d, then d * d: (1 + e)^2 (1 + e')), fp64 sums
