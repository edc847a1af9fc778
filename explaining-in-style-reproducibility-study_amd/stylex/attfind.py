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
