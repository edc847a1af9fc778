"""Definitions the counterfactual tests hold the product to (tests/test_counterfactual_cpu.py, _gpu.py), written from the
rule itself, not from the product's code:

* ``edit_levels``: the edited style vectors, a sequential loop over the edit list per level in float64 or float32 numpy
  (every fp32 operation rounded on its own: numpy scalars / arrays of one dtype do not fuse);
* ``segment_major``: the kernel's output layout, element by element from its formula;
* ``naive_images``: the notebook's structure — batch 1, every generator block run, one image per level — fed with the
  definition's styles.
"""
import numpy as np
import torch


def edit_levels(coords, smin, smax, edits, base_class, levels, shift, dtype=np.float32):
    """[L, N, S]: level l = the first levels[l] (direction, coordinate) pairs applied IN LIST ORDER to every image:
    v[c] = v[c] + (target - v[c]) * shift, target = smin[c] when (direction == 0) != (base_class == 0), else smax[c]."""
    coords, smin, smax = (np.asarray(a).astype(dtype) for a in (coords, smin, smax))
    base_class = np.asarray(base_class)
    sh = dtype(shift)
    out = np.empty((len(levels),) + coords.shape, dtype=dtype)
    for row, k in enumerate(levels):
        v = coords.copy()
        for d, c in edits[:k]:
            towards_min = (d == 0) != (base_class == 0)
            target = np.where(towards_min, smin[c], smax[c]).astype(dtype)
            diff = (target - v[:, c]).astype(dtype)
            prod = (diff * sh).astype(dtype)
            v[:, c] = (v[:, c] + prod).astype(dtype)
        out[row] = v
    return out


def segment_major(levels_nls, seg_start):
    """The flat L * N * S buffer: column c of segment g at L * N * seg_start[g] + (l * N + n) * w_g + (c - seg_start[g])."""
    nl, n, s = levels_nls.shape
    assert seg_start[0] == 0 and seg_start[-1] == s
    flat = np.full(nl * n * s, np.nan, dtype=levels_nls.dtype)
    l, i = np.arange(nl)[:, None, None], np.arange(n)[None, :, None]
    for a, b in zip(seg_start, seg_start[1:]):
        c = np.arange(a, b)[None, None, :]
        flat[nl * n * a + (l * n + i) * (b - a) + (c - a)] = levels_nls[:, :, a:b]
    assert not np.isnan(flat).any()  # the formula reaches every element
    return flat


@torch.no_grad()
def naive_images(G, latents, noise, styles_ls, image_index):
    """The images of ONE latent for every level: batch 1, every block run, the block's (style1, style2) cut from
    styles_ls [L, S] (the definition's edited vector of that image)."""
    import attfind

    dev = next(G.parameters()).device
    w = torch.as_tensor(np.asarray(latents[image_index:image_index + 1]), dtype=torch.float32, device=dev)
    noise = torch.as_tensor(noise).to(dev)
    out = []
    for styles in styles_ls:
        styles = torch.as_tensor(styles, dtype=torch.float32, device=dev)[None]
        x = G.initial_conv(G.first_activation(attfind.styles_def_to_tensor([(w, G.num_layers)])))
        rgb, at = None, 0
        for li, block in enumerate(G.blocks):
            s1 = styles[:, at:at + block.input_channels]
            s2 = styles[:, at + block.input_channels:at + block.num_style_coords]
            at += block.num_style_coords
            if G.attns[li] is not None:
                x = G.attns[li](x)
            x, _ = block.forward_main(x, w, noise, styles=(s1.contiguous(), s2.contiguous()))
            rgb = block.to_rgb(x, rgb, w)
        out.append(rgb.float())
    return torch.cat(out)
