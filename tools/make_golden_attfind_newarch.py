"""TEST INFRASTRUCTURE — golden vectors of AttFind on the conditional ("new") architecture and of the threshold pass.
Runs only where the reference source tree is present (STYLEX_REFERENCE).  The extraction cell of the reference's
``stylex/run_attfind_combined.ipynb`` (cell 5) is executed AS IS — oracle/make_golden_attfind.py reads its source from
the notebook at run time, nothing of it is written anywhere — bound to the reference's ``stylex_train_new`` module with
``USE_OLD_ARCHITECTURE = False``, on the configuration of attfind_16.npz (16 px, capacity 4, fmap_max 64, 3 images,
shift 1.0, the same non-zero noise weights, TinyClassifier(seed=99)).  tests/golden/attfind_newarch_16.npz holds arrays only:

    out/<9 datasets>   the cell's ``attfind_extraction`` on the conditional StylEx
    thr/<2 datasets>   the cell's ``find_discriminator_threshold`` on the same model
    thr_old/<2>        the cell's ``find_discriminator_threshold`` on the default architecture (``USE_OLD_ARCHITECTURE =
                       True``, the reference's ``stylex_train`` StylEx of attfind_16.npz: same seed, same inputs)
    config, seed, shift_size, n_coords, images, input_noise, noise_weights   the inputs

    python tools/make_golden_attfind_newarch.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import make_golden_attfind as mga  # noqa: E402
from make_golden_attfind import ref_shim, save, seed_all  # noqa: E402

SIZE, CAP, FMAX, SEED, N_IMG, SHIFT = 16, 4, 64, 5, 3, 1.0


def setup(mod):
    """Model, classifier, images and noise plane drawn exactly as oracle/make_golden_attfind.py:main draws them."""
    seed_all(SEED)
    model = mod.StylEx(image_size=SIZE, network_capacity=CAP, fmap_max=FMAX)
    model.eval()
    g = torch.Generator().manual_seed(SEED + 1)
    for blk in model.G.blocks:
        for lin in (blk.to_noise1, blk.to_noise2):
            lin.weight.data = torch.randn(lin.weight.shape, generator=g) * 0.3
            lin.bias.data = torch.randn(lin.bias.shape, generator=g) * 0.1
    clf = ref_shim.TinyClassifier(seed=99, image_size=SIZE)
    images = [torch.rand(1, 3, SIZE, SIZE, generator=g) for _ in range(N_IMG)]
    noise = torch.rand(1, SIZE, SIZE, 1, generator=g)
    return model, clf, images, noise


def capture(fn, **kw):
    mga._FakeFile.captured = {}
    with torch.no_grad():
        fn(**kw)
    return dict(mga._FakeFile.captured)


def threshold_pass(ns, model, clf, images, noise):
    ns["noise"] = noise  # the cell's find_discriminator_threshold reads the notebook's global
    return capture(ns["find_discriminator_threshold"], stylex=model, classifier=clf, dataloader=iter(list(images)),
                   num_images=N_IMG, threshold_folder="/tmp", dataset_name=None, image_size=SIZE, batch_size=1, cuda_rank=0)


def main():
    st = ref_shim.import_reference()
    stn = ref_shim.import_reference_new()

    ns = mga.load_extraction_cell(stn)
    ns["USE_OLD_ARCHITECTURE"] = False
    model, clf, images, noise = setup(stn)
    assert model.D.fc.out_features == 2, "not the conditional discriminator"
    n_coords = sum(b.num_style_coords for b in model.G.blocks)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    # before the sweep: it adds and subtracts every shift on the to_style biases, which restores them only to rounding
    thr = threshold_pass(ns, model, clf, images, noise)
    out = capture(ns["attfind_extraction"], dataloader=list(images), num_images=N_IMG, results_folder="/tmp", stylex=model,
                  classifier=clf, dataset_name=None, noise=noise, num_style_coords=n_coords, shift_size=SHIFT,
                  discriminator_threshold=-0.5, image_size=SIZE, batch_size=1, cuda_rank=0, use_discriminator=False)
    for k, v in model.state_dict().items():  # the sweep mutates to_style biases in place and restores them
        assert torch.allclose(v, state[k], atol=1e-6), k
    # the two passes share their first pass
    assert np.array_equal(thr["discriminator_outputs"], out["discriminator"])
    noise_weights = torch.cat([torch.cat([b.to_noise1.weight.reshape(-1), b.to_noise1.bias, b.to_noise2.weight.reshape(-1),
                                          b.to_noise2.bias]) for b in model.G.blocks])

    ns_old = mga.load_extraction_cell(st)
    model_old, clf_old, images_old, noise_old = setup(st)
    assert all(torch.equal(a, b) for a, b in zip(images, images_old)) and torch.equal(noise, noise_old)
    thr_old = threshold_pass(ns_old, model_old, clf_old, images_old, noise_old)

    fixture = {"out/" + k: v for k, v in out.items()}
    fixture.update({"thr/" + k: v for k, v in thr.items()})
    fixture.update({"thr_old/" + k: v for k, v in thr_old.items()})
    save("attfind_newarch_16", config=np.array([SIZE, CAP, FMAX]), seed=SEED, shift_size=SHIFT, n_coords=n_coords,
         images=torch.cat(images), input_noise=noise, noise_weights=noise_weights, **fixture)
    print({k: v.shape for k, v in fixture.items()})


if __name__ == "__main__":
    main()
