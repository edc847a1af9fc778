"""SHA-256 of what Trainer.train() publishes and leaves behind, for comparing two trees bit for bit on ONE machine: per
case the per-step scalar rows (d, g, rec, kl, gp, pl_mean) and every parameter after the golden's step count.  The
Trainers are built from the configs and seeds stored in the step goldens (their values are not read).  One process per
tree; MIOpen's algorithm choice is pinned and a throw-away Trainer runs first, both as in tools/determinism_check.py.
CPU: every config with draw-ahead 0, 1 and 2 on the oracle's CPU ops.  GPU: every config in fp32, bf16 and fp32 with
device_rng, and the graph path (warm-up, capture and replay of both step shapes) on the gae2_alt config.

    python tools/step_bits.py [--tree ROOT_OF_ANOTHER_CHECKOUT] [--device cpu|cuda:0]"""
import argparse
import hashlib
import json
import os
import random
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--device", default="cpu")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.tree)
PKG = os.path.join(ROOT, "explaining-in-style-reproducibility-study_amd")
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), PKG, os.path.join(PKG, "stylex")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ops  # noqa: E402
import stylex_train as st  # noqa: E402
from lpips_standin import LPIPSStandIn  # noqa: E402
from standins import TinyClassifier  # noqa: E402

GOLDENS = ["gae1_alt", "gae2_alt", "gae2_noalt", "gae2_pl", "gae2_aug", "newarch", "newarch_variants", "no_const",
           "no_const_pl", "rel_disc", "top_k", "attn", "attn_pl"]
DEV = torch.device(ARGS.device)


def sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:32]


def make_trainer(tag, tmp, **kw):
    """The Trainer of tests/golden/steps_<tag>.npz, as the step-parity tests build it."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "steps_%s.npz" % tag))
    size, cap, fmax, bs, gae, alt, n, start = (int(v) for v in g["config"])
    if "variant" in g.files:
        kw = dict(json.loads(str(g["variant"])), new_architecture=bool(int(g["new_architecture"])), **kw)
    if tag == "newarch":
        kw["new_architecture"] = True
    if "attn_layers" in g.files:
        kw["attn_layers"] = [int(v) for v in g["attn_layers"]]
    cls, lp = TinyClassifier(seed=int(g["cls_seed"])).to(DEV), LPIPSStandIn(seed=int(g["lpips_seed"])).to(DEV)
    gd = torch.Generator().manual_seed(int(g["data_seed"]))
    batches = [torch.rand(bs, 3, size, size, generator=gd) for _ in range(8)]
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(int(g["seed"]))
    tr = st.Trainer(name="t", base_dir=tmp, image_size=size, network_capacity=cap, fmap_max=fmax, batch_size=bs,
                    gradient_accumulate_every=gae, alternating_training=bool(alt),
                    lr=float(g["lr"]) if "lr" in g.files else 2e-4, ttur_mult=1.5, rec_scaling=1, kl_scaling=1,
                    classifier=cls, lpips_fn=lp, classifier_name="resnet", evaluate_every=10 ** 9, save_every=10 ** 9,
                    device=DEV, aug_prob=float(g["aug_prob"]) if "aug_prob" in g.files else 0., **kw)
    tr.loader = st.cycle(batches)
    tr.dataset = list(range(1000))
    tr.save = lambda *a, **k: None
    tr.evaluate = lambda *a, **k: None
    tr.init_StylEx()
    tr.steps = start
    pl0 = float(g["pl_mean0"]) if "pl_mean0" in g.files else float("nan")
    tr.pl_mean = None if np.isnan(pl0) else pl0
    return tr, n


def case(label, tag, tmp, calls=None, draw_ahead=None, **kw):
    tr, n = make_trainer(tag, tmp, **kw)
    if draw_ahead is not None:
        tr._draw_mode = draw_ahead
    rows = []
    for _ in range(calls or n):
        tr.train()
        rows.append([np.nan if v is None else v for v in (tr.d_loss, tr.g_loss, tr.total_rec_loss, tr.total_kl_loss,
                                                          tr.last_gp_loss, tr.pl_mean)])
    tr._drain_draw_ahead()
    if kw.get("graphs"):
        assert sorted(tr._graph_cache) == [False, True], "both step shapes captured"
    params = [p.detach().cpu().numpy() for p in tr.StylEx.parameters()]
    print("%-34s scalars %s  params %s" % (label, sha([np.array(rows, dtype=np.float64)]), sha(params)), flush=True)
    if DEV.type == "cuda":
        del tr
        torch.cuda.empty_cache()


def main():
    tmp = tempfile.mkdtemp(prefix="step_bits_")
    torch.backends.cudnn.deterministic = True
    if DEV.type == "cpu":
        from cpu_ops import CpuOracleOps

        ops.use_impl(CpuOracleOps)
        for tag in GOLDENS:
            for ahead in (0, 1, 2):
                case("cpu %s draw_ahead=%d" % (tag, ahead), tag, tmp, draw_ahead=ahead)
        return
    import hip_backend as hb

    hb.load_library()
    tr, _ = make_trainer("gae2_alt", tmp)  # the first Trainer of a process orders its double backward differently
    tr.train()
    torch.cuda.synchronize()
    del tr
    for tag in GOLDENS:
        for prec in ("fp32", "bf16"):
            ops.set_precision(prec)
            case("gpu %s %s" % (tag, prec), tag, tmp)
        ops.set_precision("fp32")
        case("gpu %s fp32 device_rng" % tag, tag, tmp, device_rng=True)
    # the set-up of tests/test_hip_parity.py::test_graph_replay_matches_eager: call 1 is eager, 2-3 warm both step
    # shapes up on the static buffers, 4-5 capture (and replay) them, 6-8 replay
    case("gpu gae2_alt fp32 graphs", "gae2_alt", tmp, calls=8, graphs=True, graph_warmup=1, gp_every=2)


if __name__ == "__main__":
    main()
