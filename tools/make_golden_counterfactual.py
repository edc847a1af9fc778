"""TEST INFRASTRUCTURE — golden vector of the counterfactual experiment's attribute ranking.  Runs only where the reference
source tree is present (STYLEX_REFERENCE).  Cells 9 (the split by class), 12 (``find_significant_styles``) and 13 (the
per-class selection, the join and the score ordering) of the reference's ``stylex/FID_TensorFlow.ipynb`` are executed AS
IS — their source is read from the notebook at run time, nothing of it is written anywhere — on a synthetic effect tensor.
The cells are numpy only; their ``tf.keras.models.Model`` annotations get a stand-in namespace.
tests/golden/counterfactual_rank.npz holds arrays only:

    style_change_effect [N, 2, S, 2], base_probs [N, 2]   the inputs
    num_indices, effect_threshold                          cell 13's constants, read back from its namespace
    ranked [M, 2]                                          cell 13's s_indices_and_signs: (direction, coordinate) rows
    class_counts [2]                                       images per class

    python tools/make_golden_counterfactual.py
"""
import json
import os
import sys
import types
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import ref_shim  # noqa: E402

NOTEBOOK = os.path.join(ref_shim.REF_STYLEX, "FID_TensorFlow.ipynb")
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden", "counterfactual_rank.npz")
N, S, SEED = 40, 24, 0


def inputs():
    rng = np.random.default_rng(SEED)
    effect = 0.03 * rng.standard_normal((N, 2, S, 2))
    effect[..., 1] = -effect[..., 0]  # a binary classifier's logits move against each other
    return effect, rng.standard_normal((N, 2))


def main():
    cells = json.load(open(NOTEBOOK))["cells"]
    src = {i: "".join(cells[i]["source"]) for i in (9, 12, 13)}
    assert "style_effect_classes[img_ind]" in src[9] and "def find_significant_styles(" in src[12]
    assert "all_sindex_joined_class_0" in src[13]
    effect, base_probs = inputs()
    labels = np.argmax(base_probs, axis=1)
    counts = np.bincount(labels, minlength=2)
    assert counts.min() > 0, "the notebook's selection needs images of both classes"
    # the three-line stand-in for the cells' tf.keras.models.Model annotations
    tf = types.SimpleNamespace(keras=types.SimpleNamespace(models=types.SimpleNamespace(Model=object)))
    ns = dict(np=np, tf=tf, Optional=Optional, base_probs=base_probs, label_size=2, style_change_effect=effect,
              W_values=np.zeros((N, 1)), all_style_vectors_distances=np.zeros((N, S, 2)), all_style_vectors=np.zeros((N, S)),
              generator=None, classifier=None, style_min=np.zeros(S), style_max=np.zeros(S))
    for i in (9, 12, 13):
        exec(compile(src[i], "FID_TensorFlow.ipynb cell %d" % i, "exec"), ns)
    num_indices, thr = int(ns["num_indices"]), float(ns["effect_threshold"])
    # the greedy loop takes a mean over the images still below max_image_effect: well defined only while one is left
    for c in (0, 1):
        eff = effect[labels == 1 - c]
        direction = np.maximum(0, eff[:, :, :, c].reshape((eff.shape[0], -1)))
        acc = np.zeros(eff.shape[0])
        for d, s in ns["s_indices_and_signs_dict"][c]:
            assert (acc < 5 * thr).any(), "no image left below max_image_effect: the notebook's mean is over nothing"
            acc += direction[:, d * S + s]
    ranked = np.array(ns["s_indices_and_signs"], dtype=np.int64)
    coords = ranked[:, 1].tolist()
    assert len(set(coords)) < len(coords), "the fixture should hold a coordinate in both directions (the duplicate case)"
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez(OUT, style_change_effect=effect, base_probs=base_probs, num_indices=np.int64(num_indices),
             effect_threshold=np.float64(thr), ranked=ranked, class_counts=counts.astype(np.int64))
    print("classes", counts.tolist(), "ranked", ranked.tolist())


if __name__ == "__main__":
    main()
