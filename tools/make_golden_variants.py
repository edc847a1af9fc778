"""TEST INFRASTRUCTURE — golden vectors of the training variants no_const, rel_disc_loss and top_k_training.  Runs only
where the reference source tree is present (STYLEX_REFERENCE): it imports the reference through oracle/ref_shim.py (the
sibling of tools/make_golden_attn.py: same shim, same seeds, same refusal rule) and writes data-only fixtures to
tests/golden/:

    steps_no_const.npz          3 Trainer.train() calls from step 0 with no_const=True
    steps_no_const_pl.npz       2 calls from step 5024, pl_mean 0.05 (call 0: gradient penalty AND path length) with no_const=True
    steps_rel_disc.npz          3 calls from step 0 with rel_disc_loss=True; also holds `dual_contrast_loss_error`, the text
                                of the exception the reference's own train() raises with dual_contrast_loss=True
    steps_top_k.npz             3 calls from step 1000 with top_k_training=True, gamma 0.5, frac 0.5 (k = 2 of 4)
    steps_newarch_variants.npz  3 calls from step 0 of the second architecture (stylex_train_new.py), all three on.  There
                                k == batch_size on every call: with k < batch_size stylex_train_new.py:1472 keeps the
                                (values, indices) tuple of topk and its own train() raises; that text is stored as
                                `top_k_error` (captured from step 1000, gamma 0.5)
    init_no_const.npz           seeded-init state dict of StylEx(no_const=True): keys, shapes, statistics

Every step fixture is run twice, with 1 and with 8 CPU threads; the per-call spread between the two runs,
max |a - b| / (1 + |b|) over the six scalars, is stored, and a fixture whose spread exceeds 1e-4 — a tenth of the 1e-3
the tests assert — is not written.

    python tools/make_golden_variants.py [--only no_const,no_const_pl,rel_disc,top_k,newarch,init]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_attn import SPREAD_LIMIT, _param_stats, ref_shim, save, seed_all, stats  # noqa: E402

TOP_K = dict(top_k_training=True, generator_top_k_gamma=0.5, generator_top_k_frac=0.5)
INIT_SEED = 311


def _trainer(mod, threads, variant, **over):
    size, cap, fmax, bs, gae = 32, 4, 64, 4, 2
    torch.set_num_threads(threads)
    cls = ref_shim.TinyClassifier(seed=99)
    gd = torch.Generator().manual_seed(7)
    batches = [torch.rand(bs, 3, size, size, generator=gd) for _ in range(8)]
    seed_all(42)
    kw = dict(image_size=size, network_capacity=cap, fmap_max=fmax, batch_size=bs, gradient_accumulate_every=gae,
              alternating_training=True, lr=2e-4, ttur_mult=1.5, rec_scaling=1, kl_scaling=1, aug_prob=0.)
    kw.update(variant)
    kw.update(over)
    tr = ref_shim.make_reference_trainer(mod, tempfile.mkdtemp(), cls, batches, **kw)
    return tr, (size, cap, fmax, bs, gae)


def _run_steps(mod, n, start, pl0, threads, variant):
    tr, cfg = _trainer(mod, threads, variant)
    tr.init_StylEx()
    tr.steps = start
    tr.pl_mean = pl0
    rows = []
    for i in range(n):
        tr.train()
        rows.append([tr.d_loss, tr.g_loss, tr.total_rec_loss, tr.total_kl_loss,
                     tr.last_gp_loss if tr.last_gp_loss is not None else np.nan,
                     tr.pl_mean if tr.pl_mean is not None else np.nan])
        print("threads=%d call %d" % (threads, i), rows[-1])
    names, pst = _param_stats(tr.StylEx)
    return np.array(rows, dtype=np.float64), names, pst, cfg


def gen_steps(mod, name, n, start, pl0, variant, new_architecture=False, **extra):
    a, names, pst, (size, cap, fmax, bs, gae) = _run_steps(mod, n, start, pl0, 1, variant)
    b = _run_steps(mod, n, start, pl0, 8, variant)[0]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    spread = np.nanmax(np.abs(a - b) / (1 + np.abs(b)), axis=1)
    print(name, "1-thread vs 8-thread spread per call:", spread)
    if not (spread <= SPREAD_LIMIT).all():
        raise SystemExit("%s: the reference's own 1- vs 8-thread spread %s exceeds %g: fixture NOT written"
                         % (name, spread, SPREAD_LIMIT))
    save(name, config=np.array([size, cap, fmax, bs, gae, 1, n, start]), pl_mean0=np.nan if pl0 is None else pl0,
         data_seed=7, seed=42, cls_seed=99, lpips_seed=4242, scalars=a, scalars_8_threads=b, thread_spread=spread,
         param_names=names, param_stats=pst, aug_prob=0., variant=json.dumps(variant, sort_keys=True),
         new_architecture=int(new_architecture), **extra)


def reference_error(mod, variant, start=0):
    """What the reference's own first train() call raises with `variant`: 'ExceptionType: message'."""
    tr, _ = _trainer(mod, 1, variant)
    tr.init_StylEx()
    tr.steps = start
    try:
        tr.train()
    except Exception as e:  # noqa: BLE001  (the point is to record whatever it raises)
        text = "%s: %s" % (type(e).__name__, e)
        print(variant, "->", text)
        return text
    raise SystemExit("%r ran in the reference: the rejection in the Trainer has lost its reason" % (variant,))


def gen_init(mod):
    size, cap, fmax = 32, 4, 64
    torch.manual_seed(INIT_SEED)
    m = mod.StylEx(image_size=size, network_capacity=cap, fmap_max=fmax, no_const=True)
    sd = m.state_dict()
    save("init_no_const", seed=INIT_SEED, config=np.array([size, cap, fmax]), keys=np.array(list(sd.keys())),
         shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]), stats=np.stack([stats(v) for v in sd.values()]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="no_const,no_const_pl,rel_disc,top_k,newarch,init")
    only = ap.parse_args().only.split(",")
    st = ref_shim.import_reference()
    if "init" in only:
        gen_init(st)
    if "no_const" in only:
        gen_steps(st, "steps_no_const", 3, 0, None, {"no_const": True})
    if "no_const_pl" in only:
        gen_steps(st, "steps_no_const_pl", 2, 5024, 0.05, {"no_const": True})
    if "rel_disc" in only:
        gen_steps(st, "steps_rel_disc", 3, 0, None, {"rel_disc_loss": True},
                  dual_contrast_loss_error=np.array(reference_error(st, {"dual_contrast_loss": True})))
    if "top_k" in only:
        gen_steps(st, "steps_top_k", 3, 1000, None, dict(TOP_K))
    if "newarch" in only:
        stn = ref_shim.import_reference_new()
        gen_steps(stn, "steps_newarch_variants", 3, 0, None, dict(top_k_training=True, no_const=True, rel_disc_loss=True),
                  new_architecture=True, top_k_error=np.array(reference_error(stn, dict(TOP_K), start=1000)))


if __name__ == "__main__":
    main()
