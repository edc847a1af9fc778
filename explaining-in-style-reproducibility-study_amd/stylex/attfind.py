"""Batched AttFind StyleSpace sweep — drop-in for the extraction cell of the reference's
``stylex/run_attfind_combined.ipynb`` (cell 5, :246-417), producing the same datasets (``style_change, latents,
base_prob, minima, maxima, style_coordinates, original_images, noise, discriminator``), for BOTH architectures the
notebook switches between with ``USE_OLD_ARCHITECTURE``:

* default: ``w = cat(encoder, logits)``, ``D(generated)``;
* conditional (``StylEx(conditional=True)``, the notebook's ``faces_new``): ``w = cat(encoder, softmax(logits))`` and
  ``D(generated, probabilities=softmax(classify(generated)))``; ``base_prob`` stays the raw logits.

``attfind_extraction`` / ``find_discriminator_threshold`` read the architecture from ``stylex.conditional``; everything
after the first pass (the sweep, ``change_images``, the ``visualize_*`` functions) works on the stored latents and has
no branch, like the notebook's cells 17-21.  ``load_records`` is cell 12's loader, ``attfind_cli.py`` the command line.

The notebook perturbs ONE style coordinate at a time by mutating ``to_style{1,2}.bias`` in place and re-running
the whole generator at batch 1: 2 x N_coords generator + classifier evaluations per image (2 x 2464 at 64 px).
Here the same arithmetic is restructured for the GPU:

* a perturbation is a per-sample additive offset on the block's style vector (``GeneratorBlock.forward_main(...,
  styles=)``) — no parameter is mutated, so perturbations of different coordinates batch together;
* a coordinate of block k only changes blocks k..L-1: the feature map and RGB entering block k are computed once
  per image and shared by all perturbations of that block (prefix caching);
* ``chunk`` perturbations (both directions of chunk/2 coordinates) run as one generator-suffix + classifier pass;
* under ``torch.distributed`` the sweep shards over images: every rank runs the cheap first pass on
  all images (1 evaluation each, so minima / maxima need no collective), sweeps images ``rank::world`` and one
  ``all_reduce(SUM)`` over the effect tensor (zero for foreign images) assembles the result on every rank;
* ``first_pass_batch`` > 1 runs that first pass (encoder, classifier, generator, discriminator, classifier of the
  generated image) on several loader items at once; 1, the default, is the notebook's batch-1 loop launch for launch.
"""
import os

import numpy as np
import torch
import torch.distributed as dist

import ops

DATASETS = ("style_change", "latents", "base_prob", "minima", "maxima", "style_coordinates", "original_images",
            "noise", "discriminator")


def styles_def_to_tensor(styles_def):
    return torch.cat([t[:, None, :].expand(-1, n, -1) for t, n in styles_def], dim=1)


def _prefix_states(G, w_tensor, noise):
    """Feature map / RGB entering every block for one image (batch 1), plus the unperturbed block styles."""
    # no_const: the first activation comes from the image's own w; a perturbed style BIAS does not enter it, so the
    # prefix states stay valid for every perturbation
    x = G.initial_conv(G.first_activation(w_tensor))
    rgb, states = None, []
    for li, block in enumerate(G.blocks):
        istyle = w_tensor[:, li]
        s1, s2 = block.to_style1(istyle), block.to_style2(istyle)
        if G.attns[li] is not None:  # attn_layers: the attention block sits on the block's input
            x = G.attns[li](x)
        states.append((x, rgb, s1, s2))
        x, _ = block.forward_main(x, istyle, noise, styles=(s1, s2))
        rgb = block.to_rgb(x, rgb, istyle)
    return states


def _suffix(G, k, x, rgb, w_tensor, noise, styles_k):
    """Blocks k..L-1 for a batch of perturbations of block k (styles_k = per-sample (style1, style2))."""
    p = styles_k[0].shape[0]
    w = w_tensor.expand(p, -1, -1)
    nz = noise.expand(p, -1, -1, -1)
    x = x.expand(p, -1, -1, -1)
    rgb = None if rgb is None else rgb.expand(p, -1, -1, -1)
    for li in range(k, len(G.blocks)):
        block = G.blocks[li]
        if li > k and G.attns[li] is not None:  # block k's own attention is already in its prefix state
            x = G.attns[li](x)
        x, _ = block.forward_main(x, w[:, li], nz, styles=styles_k if li == k else None)
        rgb = block.to_rgb(x, rgb, w[:, li])
    return rgb.float()


def _loader_groups(images, size):
    """Lists of up to size() loader items ([1,3,S,S] each), in loader order; size() is asked before every group."""
    it = iter(images)
    while True:
        group = []
        for _ in range(size()):
            item = next(it, None)
            if item is None:
                break
            group.append(item)
        if not group:
            return
        yield group


def _first_pass(stylex, classifier, group, noise, conditional):
    """Cell 5's per-image first pass for a list of [1,3,S,S] items run as ONE batch: (batch, w, generated image, style
    coordinates, discriminator output [b], logits of the generated image or None).  The conditional discriminator needs
    the generated image's probabilities, so there the logits are always computed; the default architecture leaves them
    to the caller (only kept images need them)."""
    G = stylex.G
    dev = noise.device
    batch = group[0].to(dev) if len(group) == 1 else torch.cat([t.to(dev) for t in group])
    b = batch.shape[0]
    enc = stylex.encoder(batch).reshape(b, -1)
    logits = classifier.classify_images(batch)
    w = torch.cat((enc, torch.softmax(logits, dim=1) if conditional else logits), dim=1)
    generated, sc = G(styles_def_to_tensor([(w, G.num_layers)]), noise.expand(b, -1, -1, -1), get_style_coords=True)
    gen_logits = None
    if conditional:
        gen_logits = classifier.classify_images(generated)
        d_out = stylex.D(generated, probabilities=torch.softmax(gen_logits, dim=1))
    else:
        d_out = stylex.D(generated)
    return batch, w, generated, sc, d_out.reshape(b), gen_logits


def _conditional(stylex, conditional):
    return bool(getattr(stylex, "conditional", False)) if conditional is None else bool(conditional)


@torch.no_grad()
def attfind_extraction(stylex, classifier, images, num_images, noise, shift_size=1.0, discriminator_threshold=None,
                       use_discriminator=False, chunk=256, results_folder=None, conditional=None, first_pass_batch=1):
    """images: iterable of [1,3,S,S] batches (the notebook's batch-size-1 loader).  Returns a dict of CPU tensors
    with the notebook's dataset names; with `results_folder` also writes style_change_records.{hdf5|npz}.
    `conditional`: None reads ``stylex.conditional``.  `use_discriminator` drops an image whose discriminator output is
    below `discriminator_threshold` (the notebook's own ``skip`` flag is inverted; not copied).  `first_pass_batch`
    loader items go through the first pass together; images are kept, and counted towards `num_images`, in loader order."""
    G = stylex.G
    dev = next(G.parameters()).device
    noise = noise.to(dev)
    conditional = _conditional(stylex, conditional)
    filtering = use_discriminator and discriminator_threshold is not None
    n_coords = sum(b.num_style_coords for b in G.blocks)
    latents, base_logits, coords, disc, originals = [], [], [], [], []
    # never more items in a group than images still wanted: a group cannot keep past num_images
    for group in _loader_groups(images, lambda: min(first_pass_batch, num_images - len(latents))):
        batch, w, generated, sc, d_out, gen_logits = _first_pass(stylex, classifier, group, noise, conditional)
        keep = list(range(batch.shape[0]))
        if filtering:
            keep = [j for j, d in enumerate(d_out.tolist()) if not d < discriminator_threshold]
        if keep and gen_logits is None:
            gen_logits = classifier.classify_images(generated)
        for j in keep:
            originals.append(batch[j])
            latents.append(w[j])
            coords.append(sc[j])
            disc.append(d_out[j:j + 1])
            base_logits.append(gen_logits[j])
    if not latents:
        raise ValueError("No images pass the threshold check")
    n = len(latents)
    coords = torch.stack(coords)
    minima, maxima = coords.min(dim=0)[0], coords.max(dim=0)[0]
    effects = torch.zeros(n, 2, n_coords, 2, device=dev)
    half = max(1, chunk // 2)
    sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if sharded else (0, 1)
    for i in range(rank, n, world):
        w_tensor = styles_def_to_tensor([(latents[i].unsqueeze(0), G.num_layers)])
        states = _prefix_states(G, w_tensor, noise)
        base = 0
        for k, block in enumerate(G.blocks):
            x_k, rgb_k, s1, s2 = states[k]
            c1 = block.input_channels
            for lo in range(0, block.num_style_coords, half):
                idx = torch.arange(lo, min(lo + half, block.num_style_coords), device=dev)
                sidx = base + idx
                cur = coords[i, sidx]
                # rows: [down for every coordinate of the chunk, then up]
                delta = torch.cat(((minima[sidx] - cur) * shift_size, (maxima[sidx] - cur) * shift_size))
                cols = torch.cat((idx, idx))
                rows = torch.arange(cols.numel(), device=dev)
                st1 = s1.expand(cols.numel(), -1).clone()
                st2 = s2.expand(cols.numel(), -1).clone()
                in1 = cols < c1
                st1[rows[in1], cols[in1]] += delta[in1]
                st2[rows[~in1], cols[~in1] - c1] += delta[~in1]
                logits = classifier.classify_images(_suffix(G, k, x_k, rgb_k, w_tensor, noise, (st1, st2)))
                diff = logits - base_logits[i][None]
                m = idx.numel()
                effects[i, 0, sidx] = diff[:m]
                effects[i, 1, sidx] = diff[m:]
            base += block.num_style_coords
    if sharded:
        dist.all_reduce(effects, op=dist.ReduceOp.SUM)
    out = {"style_change": effects, "latents": torch.stack(latents), "base_prob": torch.stack(base_logits),
           "minima": minima[None], "maxima": maxima[None], "style_coordinates": coords,
           "original_images": torch.stack(originals), "noise": noise, "discriminator": torch.stack(disc)}
    out = {k: v.detach().float().cpu() for k, v in out.items()}
    if results_folder is not None and rank == 0:
        write_records(out, results_folder)
    return out


def _write_datasets(datasets, folder, stem):
    """<stem>.hdf5 with one float dataset per entry; <stem>.npz when h5py is not installed."""
    try:
        import h5py
    except ImportError:
        np.savez(os.path.join(folder, stem + ".npz"), **{k: v.numpy() for k, v in datasets.items()})
        return
    with h5py.File(os.path.join(folder, stem + ".hdf5"), "w") as f:
        for k, v in datasets.items():
            f.create_dataset(k, data=v.numpy(), dtype="f")


def _read_datasets(folder, stem):
    path = os.path.join(folder, stem + ".hdf5")
    if os.path.isfile(path):
        import h5py

        with h5py.File(path, "r") as f:
            return {k: np.array(f[k]) for k in f.keys()}
    with np.load(os.path.join(folder, stem + ".npz")) as f:
        return {k: f[k] for k in f.files}


def write_records(out, results_folder):
    """style_change_records.hdf5 with the notebook's dataset names (:392-416); .npz when h5py is not installed."""
    _write_datasets({k: out[k] for k in DATASETS}, results_folder, "style_change_records")


def load_records(results_folder, threshold_index=None):
    """Cell 12: the arrays of style_change_records.{hdf5|npz} under their dataset names — the per-image ones truncated
    to the first `threshold_index` rows (``load_hdf5_results``), `noise` as stored, `minima` / `maxima` squeezed — plus
    `distances`, the [images, coords, 2] distances of every style coordinate to its minimum / maximum."""
    f = _read_datasets(results_folder, "style_change_records")
    out = {k: f[k][0:threshold_index] for k in ("style_change", "latents", "base_prob", "style_coordinates",
                                                "original_images", "discriminator")}
    out["noise"] = f["noise"]
    out["minima"], out["maxima"] = np.squeeze(f["minima"]), np.squeeze(f["maxima"])
    out["distances"] = style_vector_distances(out["style_coordinates"], out["minima"], out["maxima"])
    return out


THRESHOLD_DATASETS = ("discriminator_outputs", "generated_images")


@torch.no_grad()
def find_discriminator_threshold(stylex, classifier, images, num_images, noise, conditional=None, threshold_folder=None,
                                 first_pass_batch=1):
    """Cell 5's ``find_discriminator_threshold``: the discriminator output [n, 1] and the generated image [n, 3, S, S]
    of the first `num_images` loader items (CPU float tensors), from which a caller picks `discriminator_threshold`.
    With `threshold_folder` also writes discriminator_threshold.{hdf5|npz} under those two dataset names."""
    dev = next(stylex.G.parameters()).device
    noise = noise.to(dev)
    conditional = _conditional(stylex, conditional)
    disc, generated_images = [], []
    found = 0
    for group in _loader_groups(images, lambda: min(first_pass_batch, num_images - found)):
        _, _, generated, _, d_out, _ = _first_pass(stylex, classifier, group, noise, conditional)
        disc.append(d_out[:, None])
        generated_images.append(generated)
        found += d_out.shape[0]
    if not disc:
        raise ValueError("The loader holds no images")
    out = {"discriminator_outputs": torch.cat(disc), "generated_images": torch.cat(generated_images)}
    out = {k: v.detach().float().cpu() for k, v in out.items()}
    if threshold_folder is not None:
        _write_datasets(out, threshold_folder, "discriminator_threshold")
    return out


def find_significant_styles(style_change_effect, num_indices, class_index, max_image_effect=0.2, sindex_offset=0):
    """Greedy selection of the style coordinates that most raise `class_index` (notebook cell 15): repeatedly take the
    coordinate/direction with the largest mean positive effect over the images not yet explained (accumulated effect
    < max_image_effect).  style_change_effect: [images, 2 directions, coords, classes].  Returns
    [(direction, coordinate + sindex_offset)].  (The notebook's generator / classifier / latent arguments are unused.)"""
    effect = np.array(style_change_effect, copy=True)
    n_img, _, n_coords, _ = effect.shape
    direction = np.maximum(0, effect[:, :, :, class_index].reshape((n_img, -1)))
    images_effect = np.zeros(n_img)
    chosen = []
    while len(chosen) < num_indices:
        nxt = int(np.argmax(np.mean(direction[images_effect < max_image_effect], axis=0)))
        chosen.append(nxt)
        images_effect += direction[:, nxt]
        direction[:, nxt] = 0
    return [(x // n_coords, (x % n_coords) + sindex_offset) for x in chosen]


# ---- post-processing and visualisation cells of the notebook (cells 11, 12, 14, 17-21) ------------------------------


def filter_unstable_images(style_change_effect, effect_threshold=0.3, num_indices_threshold=150):
    """Cell 11: zero the effects of images on which more than `num_indices_threshold` coordinates move the classifier by
    more than `effect_threshold` (in place, like the notebook)."""
    unstable = np.sum(np.abs(style_change_effect) > effect_threshold, axis=(1, 2, 3)) > num_indices_threshold
    style_change_effect[unstable] = 0
    return style_change_effect


def style_vector_distances(all_style_vectors, style_min, style_max):
    """Cell 12 (tail): [images, coords, 2] = distance of every style coordinate to the minimum / to the maximum."""
    d = np.zeros((all_style_vectors.shape[0], all_style_vectors.shape[1], 2))
    d[:, :, 0] = all_style_vectors - style_min[None]
    d[:, :, 1] = style_max[None] - all_style_vectors
    return d


def split_by_class(base_probs, style_change_effect, W_values, all_style_vectors_distances, all_style_vectors):
    """Cell 14: the sweep's arrays split by the class the classifier assigns to the generated image."""
    labels = np.argmax(base_probs, axis=1)
    out = {}
    for c in range(2):
        idx = np.nonzero(labels == c)[0]
        out[c] = dict(effect=style_change_effect[idx].astype(np.float64), w=W_values[idx].astype(np.float64),
                      dist=all_style_vectors_distances[idx], style_vectors=all_style_vectors[idx], index=idx)
    return out


def _block_of(G, sindex):
    base = 0
    for k, block in enumerate(G.blocks):
        if sindex < base + block.num_style_coords:
            return k, sindex - base
        base += block.num_style_coords
    raise IndexError(sindex)


@torch.no_grad()
def change_images(G, classifier, dlatents, sindex, style_direction_index, s_style_min, s_style_max, shift_size, noise,
                  class_index=0):
    """Cells 17 + 19 for a BATCH of latents: the generated image of every latent, the image with style coordinate
    `sindex` moved towards its minimum (direction 0) or maximum (1) by `shift_size` times the distance, and the
    classifier's probability of `class_index` for both.  The notebook mutates ``to_style{1,2}.bias`` and runs the
    generator twice per image; here the shift is a per-sample offset on the block's style vector and all latents run
    as one pass.  Returns (base [n,3,S,S], changed [n,3,S,S], base_prob [n], change_prob [n])."""
    dev = next(G.parameters()).device
    w = torch.as_tensor(np.asarray(dlatents), dtype=torch.float32, device=dev)
    n = w.shape[0]
    noise = torch.as_tensor(noise).to(dev).expand(n, -1, -1, -1)
    k, widx = _block_of(G, int(sindex))
    base_img, coords = G(styles_def_to_tensor([(w, G.num_layers)]), noise, get_style_coords=True)
    target = float(s_style_min) if style_direction_index == 0 else float(s_style_max)
    delta = (target - coords[:, int(sindex)]) * shift_size
    x = G.initial_conv(G.first_activation(styles_def_to_tensor([(w, G.num_layers)])))
    rgb = None
    for li, block in enumerate(G.blocks):
        styles = None
        if li == k:
            s1, s2 = block.to_style1(w), block.to_style2(w)
            if widx < block.input_channels:
                s1 = s1.clone()
                s1[:, widx] += delta
            else:
                s2 = s2.clone()
                s2[:, widx - block.input_channels] += delta
            styles = (s1, s2)
        if G.attns[li] is not None:
            x = G.attns[li](x)
        x, _ = block.forward_main(x, w, noise, styles=styles)
        rgb = block.to_rgb(x, rgb, w)
    changed = rgb.float()
    base_img = base_img.float()
    p0 = torch.softmax(classifier.classify_images(base_img), dim=1)[:, class_index]
    p1 = torch.softmax(classifier.classify_images(changed), dim=1)[:, class_index]
    return base_img, changed, p0.cpu().numpy(), p1.cpu().numpy()


def pair_image(base, changed):
    """Cells 18 + 19: [S, 2S, 3] uint8, generated image left, changed image right (``draw_on_image``: clip to [0, 1],
    times 255, truncated to bytes; the probability text the notebook once drew is commented out there)."""
    def u8(img):
        return (np.clip(np.transpose(img.detach().cpu().numpy(), (1, 2, 0)), 0, 1) * 255).astype(np.uint8)
    return np.concatenate((u8(base), u8(changed)), axis=1)


def visualize_style(G, classifier, all_dlatents, style_change_effect, style_min, style_max, sindex, style_direction_index,
                    max_images, shift_size, noise, class_index=0, effect_threshold=0.3, seed=None,
                    allow_both_directions_change=False):
    """Cell 20: images on which moving coordinate `sindex` in direction `style_direction_index` changed the
    classifier's `class_index` output by more than `effect_threshold` in the sweep, shuffled (numpy global generator,
    seeded like the notebook), up to 10 x `max_images` candidates re-generated, those whose probability moves by at
    least `effect_threshold` kept, the first `max_images` stacked vertically; an empty array if fewer than three."""
    eff = style_change_effect[:, style_direction_index, sindex, class_index]
    idx = (np.abs(eff) > effect_threshold).nonzero()[0] if allow_both_directions_change else (eff > effect_threshold).nonzero()[0]
    if idx.size == 0:
        return np.array([])
    if seed is not None:
        np.random.seed(seed)
    np.random.shuffle(idx)
    idx = idx[:min(max_images * 10, len(idx))]
    base, changed, p0, p1 = change_images(G, classifier, np.asarray(all_dlatents)[idx], sindex, style_direction_index,
                                          style_min[sindex], style_max[sindex], shift_size, noise, class_index)
    rows = [pair_image(base[i], changed[i]) for i in range(len(idx)) if not np.abs(p1[i] - p0[i]) < effect_threshold]
    rows = rows[:max_images]
    return np.concatenate(rows, axis=0) if len(rows) >= 3 else np.array([])


def visualize_style_by_distance_in_s(G, classifier, all_dlatents, all_style_vectors_distances, style_min, style_max, sindex,
                                     style_sign_index, max_images, shift_size, noise, class_index=0):
    """Cell 21: the images whose coordinate `sindex` is farthest from the end it is moved to (largest distance first),
    base | changed pairs of the first `max_images`; an empty array if fewer than three."""
    idx = np.argsort(all_style_vectors_distances[:, sindex, style_sign_index])[::-1]
    if idx.size == 0:
        return np.array([])
    idx = idx[:min(max_images * 10, len(idx))]
    base, changed, _, _ = change_images(G, classifier, np.asarray(all_dlatents)[idx], sindex, style_sign_index,
                                        style_min[sindex], style_max[sindex], shift_size, noise, class_index)
    rows = [pair_image(base[i], changed[i]) for i in range(len(idx))]
    return np.concatenate(rows[:max_images], axis=0) if len(rows) >= 3 else np.array([])


# ---- the counterfactual experiment (stylex/FID_TensorFlow.ipynb cells 9, 12, 13, 20, 24, 25) --------------------


def rank_class_directions(style_change_effect, base_probs, num_indices=10, effect_threshold=0.2):
    """Cell 13 of FID_TensorFlow.ipynb on an (already filtered) effect tensor [images, 2, coords, 2]: per class c the greedy
    selection over the images of the OTHER class (``max_image_effect = 5 * effect_threshold``), the two selections joined
    into one list of (direction, coordinate) "for moving class 1 to class 0" — class 1's entries with the direction
    swapped, minus the coordinates class 0 selected, then class 0's — and sorted by descending
    ``mean(effect[:, d, s, 0]) + mean(effect[:, 1 - d, s, 1])`` over all images.  The list can be longer than `num_indices`
    and can hold a coordinate once per direction; the counterfactual sweep takes its first k entries."""
    effect = np.asarray(style_change_effect)
    if effect.ndim != 4 or effect.shape[-1] != 2 or effect.shape[1] != 2:
        raise ValueError("rank_class_directions needs a binary effect tensor [images, 2, coords, 2], got %s" % (effect.shape,))
    labels = np.argmax(np.asarray(base_probs), axis=1)
    members = {c: np.nonzero(labels == c)[0] for c in (0, 1)}
    for c in (0, 1):
        if members[c].size == 0:
            raise ValueError("rank_class_directions: no image of class %d" % c)
    sel = {c: find_significant_styles(effect[members[1 - c]].astype(np.float64), num_indices, c,
                                      max_image_effect=5 * effect_threshold) for c in (0, 1)}
    taken = {s for _, s in sel[0]}
    joined = [(1 - d, s) for d, s in sel[1] if s not in taken] + sel[0]
    scores = [np.mean(effect[:, d, s, 0]) + np.mean(effect[:, 1 - d, s, 1]) for d, s in joined]
    return [(int(joined[i][0]), int(joined[i][1])) for i in np.argsort(scores)[::-1]]


def style_segments(G):
    """[0, c1_0, c1_0 + f_0, ...]: where the blocks' style1 / style2 vectors start inside the style-coordinate vector."""
    seg = [0]
    for block in G.blocks:
        seg += [seg[-1] + block.input_channels, seg[-1] + block.num_style_coords]
    return seg


def edited_styles(coords, edits, style_min, style_max, base_class, levels, seg_start, shift_size=1.0):
    """Cell 20's edits for an image batch and every level at once: level k applies the first k (direction, coordinate)
    pairs IN LIST ORDER, each ``s += (target - s) * shift_size`` on the value the earlier ones left (the notebook recomputes
    the style vector after every bias mutation), target = the coordinate's minimum for direction 0 and maximum for 1, swapped
    for an image of base class 0 (its ``flip``).  coords [n, S] fp32, base_class [n] int32; returns one dense
    [levels, n, width] tensor per segment of `seg_start`.  One launch where the op surface has ``style_edit_levels``
    (csrc/style_edit.hip); else — the CPU test double — the fp32 torch composition below, which is also the definition
    the kernel is held to bit for bit."""
    fused = getattr(ops.impl(), "style_edit_levels", None)
    if fused is not None:
        return fused(coords, style_min, style_max, [s for _, s in edits], [d for d, _ in edits], base_class, levels,
                     seg_start, shift_size)
    return edited_styles_composition(coords, edits, style_min, style_max, base_class, levels, seg_start, shift_size)


def edited_styles_composition(coords, edits, style_min, style_max, base_class, levels, seg_start, shift_size=1.0):
    """edited_styles as indexed fp32 torch updates, change_images' arithmetic per edit: K indexed updates per level and
    one slice copy per segment."""
    out = []
    for k in levels:
        s = coords.clone()
        for d, c in edits[:k]:
            towards_min = (base_class == 0) != (d == 0)
            target = torch.where(towards_min, style_min[c], style_max[c])
            delta = (target - s[:, c]) * shift_size
            s[:, c] += delta
        out.append(s)
    out = torch.stack(out)
    return [out[:, :, a:b].contiguous() for a, b in zip(seg_start, seg_start[1:])]


def _rgb_style(block, istyle):
    """The to-RGB style as the generator's own forward gets it: the third column block of the fused affine GEMM where that
    runs (None: RGBBlock computes it itself) — so a block re-run with `styles=` overrides has the bits of the base pass."""
    fused = ops.style_affines(istyle, block.to_style1, block.to_style2, block.to_rgb.to_style)
    return None if fused is None else fused[2]


def _run_blocks(G, first, x, rgb, w_tensor, noise, styles_of):
    """Blocks first..L-1 as Generator.forward runs them (w_tensor [n, L, D]), every block on the overriding styles
    styles_of(li)."""
    per_layer = w_tensor.unbind(1)
    for li in range(first, len(G.blocks)):
        block, w = G.blocks[li], per_layer[li]
        if li > first and G.attns[li] is not None:  # block `first`'s own attention is already in its input
            x = G.attns[li](x)
        x, _ = block.forward_main(x, w, noise, styles=styles_of(li))
        rgb = block.to_rgb(x, rgb, w, style=_rgb_style(block, w), padded=True)
    if rgb.shape[1] == 4 and G.blocks[0].to_rgb.conv.filters == 3:
        rgb = rgb[:, :3]
    return rgb.float()


@torch.no_grad()
def counterfactual_images(G, classifier, dlatents, edits, style_min, style_max, noise, levels, shift_size=1.0,
                          image_batch=32, share_prefix=True):
    """Cell 20 (``create_counterfactual_dataset``) batched: yields (level_k, images [n, 3, S, S] fp32, logits [n, C]) per
    image batch and level — the image of every latent with the first level_k `edits` ((direction, coordinate) pairs, the
    list of rank_class_directions) applied together, and the classifier's logits on it.  Per image batch one base pass
    (``G(w, noise, get_style_coords=True)`` and the classifier: base_class = argmax, the notebook's
    ``get_classifier_results``), one call for the edited styles of all levels (edited_styles), then the levels in the order
    given.  Level k changes nothing before block m_k = the first block any of its k coordinates lives in: with
    `share_prefix` the feature map and RGB entering block m_k come from the base pass and only blocks m_k..L-1 run, on
    overriding styles; level 0 is the base image itself.  no_const and attn_layers: as in _prefix_states / _suffix (a style
    bias does not enter the first activation; a block's attention is part of its stored input).  share_prefix=False runs
    every block (the equality test, the timing record).  Memory is bounded by `image_batch`."""
    dev = next(G.parameters()).device

    def on_device(v):
        return torch.as_tensor(v if isinstance(v, torch.Tensor) else np.asarray(v), dtype=torch.float32, device=dev)

    w_all = on_device(dlatents)
    edits = [(int(d), int(s)) for d, s in edits]
    levels = [int(k) for k in levels]
    if any(not 0 <= k <= len(edits) for k in levels):
        raise ValueError("levels %s outside [0, %d]" % (levels, len(edits)))
    smin, smax = on_device(style_min).reshape(-1).contiguous(), on_device(style_max).reshape(-1).contiguous()
    noise = torch.as_tensor(noise).to(dev)
    seg = style_segments(G)
    first_block = [_block_of(G, s)[0] for _, s in edits]
    for lo in range(0, w_all.shape[0], image_batch):
        w = w_all[lo:lo + image_batch]
        n = w.shape[0]
        nz = noise.expand(n, -1, -1, -1)
        states = []
        w_tensor = styles_def_to_tensor([(w, G.num_layers)])
        base_img, coords = G(w_tensor, nz, get_style_coords=True, block_inputs=states)
        base_logits = classifier.classify_images(base_img)
        coords = coords.float().contiguous()
        if edits:
            base_class = base_logits.argmax(dim=-1).to(torch.int32)
            segs = edited_styles(coords, edits, smin, smax, base_class, levels, seg, shift_size)
        else:  # nothing to apply: every level is a copy
            segs = [coords[None, :, a:b].expand(len(levels), -1, -1).contiguous() for a, b in zip(seg, seg[1:])]
        for row, k in enumerate(levels):
            m = min(first_block[:k], default=len(G.blocks)) if share_prefix else 0
            if m == len(G.blocks):
                yield k, base_img, base_logits
                continue
            if share_prefix:
                x, rgb = states[m]
            else:
                x, rgb = G.initial_conv(G.first_activation(w_tensor)), None
                if G.attns[0] is not None:
                    x = G.attns[0](x)
            img = _run_blocks(G, m, x, rgb, w_tensor, nz, lambda li: (segs[2 * li][row], segs[2 * li + 1][row]))
            yield k, img, classifier.classify_images(img)


@torch.no_grad()
def counterfactual_sweep(stylex, classifier, records, edits, num_attributes=10, shift_size=1.0, fid=None, image_batch=32):
    """Cells 24 + 25's experiment (``fid_topk``) on AttFind records (``latents, minima, maxima, noise, original_images``):
    for k = 1..K (K = `num_attributes`, at most len(edits)) the counterfactual image of every latent with the first k
    `edits` applied, in one pass over the image batches (counterfactual_images, all levels per batch).  Returns
    ``k`` [1..K], ``flips`` [K] (images whose classifier argmax differs from their base class; counted on the device, read
    once at the end), ``flip_rate`` [K], ``base_class`` [N] and, with `fid` a fid.FIDEvaluator, ``fid`` [K + 1]:
    FID(original_images, generated) then FID(original_images, counterfactual_k), ``fid_topk``'s order — the real moments
    accumulated once, one FIDStats per level, every image through the lossless path (the notebook writes PNG files)."""
    G = stylex.G
    dev = next(G.parameters()).device
    edits = [(int(d), int(s)) for d, s in edits]
    top = min(int(num_attributes), len(edits))
    if top < 1:
        raise ValueError("counterfactual_sweep needs at least one edit and num_attributes >= 1")
    latents = np.asarray(records["latents"])
    n = latents.shape[0]
    flips = torch.zeros(top, dtype=torch.int64, device=dev)
    base_classes, stats = [], [None] * (top + 1)
    if fid is not None:
        from fid import FIDStats, frechet_distance

        originals = torch.as_tensor(np.asarray(records["original_images"]), dtype=torch.float32)
        fid.real = None
        for lo in range(0, n, image_batch):
            fid.add_real(originals[lo:lo + image_batch].to(dev))
    base = None
    for k, images, logits in counterfactual_images(G, classifier, latents, edits[:top], records["minima"], records["maxima"],
                                                   records["noise"], list(range(top + 1)), shift_size=shift_size,
                                                   image_batch=image_batch):
        if k == 0:
            base = logits.argmax(dim=-1)
            base_classes.append(base)
        else:
            flips[k - 1] += (logits.argmax(dim=-1) != base).sum()
        if fid is not None:
            fm = fid.features(images)
            if stats[k] is None:
                stats[k] = FIDStats(fm.shape[1], fm.device)
            stats[k].update(fm)
    counts = [int(v) for v in flips.tolist()]
    out = {"k": list(range(1, top + 1)), "flips": counts, "flip_rate": [c / n for c in counts],
           "base_class": torch.cat(base_classes).cpu().numpy().astype(np.int64)}
    if fid is not None:
        real = fid.real.mean_cov()
        out["fid"] = [frechet_distance(*real, *st.mean_cov()) for st in stats]
    return out


def write_fid_table(fids, path):
    """Cell 25 (``save_fids``) without pandas: the one-row table ``DataFrame.to_csv`` writes — an empty index header, the
    column names, then row 0 with every value formatted '.2f'."""
    names = ["Original-Generated", "Original-Attribute 1"] + ["Original-Attributes 1-%d" % i for i in range(2, len(fids))]
    with open(path, "w") as f:
        f.write("," + ",".join(names[:len(fids)]) + "\n")
        f.write("0," + ",".join(format(v, ".2f") for v in fids) + "\n")
