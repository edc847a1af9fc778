"""stylex/train_classifier.py and stylex/bn_train.py without a GPU: the command line against the reference script's, the data
layer, the split, the freeze rule, checkpointing, and the composable path of the fused module — on the CPU it must be bit for
bit the plain tv_models loop.  Argument validation of the new C entry points (no device is touched)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import bn_train
import hip_backend
import train_classifier as tc
import tv_models

# stylex/train_mobilenet_classifier.py of the reference: flag -> default (store_true flags: False)
REFERENCE_FLAGS = {"freeze_all_layers": False, "amount_frozen_layers": 15, "dataset": "FFHQ-Aging", "labels": "gender", "lr": 0.01,
                   "batch_size": 200, "epochs": 50, "seed": 42, "checkpoint_name": "FFHQ-Gender.pth", "continue_training": False}


def make_folder(root, n=24, size=32, seed=3):
    """n tiny PNGs in two class folders whose class is visible (a bright or a dark disc)."""
    from PIL import Image

    rng = np.random.RandomState(seed)
    for i in range(n):
        cls = i % 2
        d = os.path.join(root, "bright" if cls else "dark")
        os.makedirs(d, exist_ok=True)
        img = rng.randint(0, 60, (size, size, 3)).astype(np.uint8) + (150 if cls else 0)
        Image.fromarray(img).save(os.path.join(d, "%03d.png" % i))
    return root


def test_flags_and_defaults_are_the_reference_scripts():
    args = tc.parse_args([])
    for flag, default in REFERENCE_FLAGS.items():
        assert getattr(args, flag) == default, flag
    assert (args.arch, args.pretrained, args.save_dir, args.image_size) == ("mobilenet_v2", None, "saved_models", 224)
    r = tc.parse_args(["--arch", "resnet18"])
    assert (r.lr, r.batch_size) == (1e-4, 128)
    r = tc.parse_args(["--arch", "resnet18", "--lr", "0.5", "--batch_size", "7", "--freeze_all_layers", "--continue_training"])
    assert (r.lr, r.batch_size, r.freeze_all_layers, r.continue_training) == (0.5, 7, True, True)


@pytest.mark.parametrize("n", [24, 101])
def test_split_lengths_and_membership(n):
    ds = torch.utils.data.TensorDataset(torch.arange(n))
    train, valid, test = tc.split_dataset(ds)
    a, b = int(n * 0.15), int(n * 0.15)
    assert (len(train), len(valid), len(test)) == (n - a - b, a, b) and len(train) >= int(n * 0.7)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(42)).tolist()
    assert list(train.indices) == perm[:len(train)] and list(valid.indices) == perm[len(train):len(train) + a]
    assert list(test.indices) == perm[len(train) + a:]


def test_freeze_rule():
    m = tc.build_model("mobilenet_v2", "random:1")
    frozen = {id(p) for layer in range(15) for p in m.features[layer].parameters()}
    assert all(p.requires_grad == (id(p) not in frozen) for p in m.parameters()) and frozen
    assert m.classifier[1].out_features == 2 and m.classifier[1].weight.requires_grad
    m = tc.build_model("mobilenet_v2", "random:1", freeze_all_layers=True)
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["classifier.1.weight", "classifier.1.bias"]
    r = tc.build_model("resnet18", "random:1")
    assert all(p.requires_grad for p in r.parameters()) and r.fc.out_features == 2
    again = tc.build_model("mobilenet_v2", "random:1")
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), tc.build_model("mobilenet_v2", "random:1").state_dict().values()))


def test_pretrained_file(tmp_path):
    with pytest.raises(FileNotFoundError, match="no_such_weights.pth"):
        tc.build_model("resnet18", str(tmp_path / "no_such_weights.pth"))
    src = tv_models.ResNet18()
    torch.save(src.state_dict(), tmp_path / "r18.pth")
    m = tc.build_model("resnet18", str(tmp_path / "r18.pth"))
    assert torch.equal(m.conv1.weight, src.conv1.weight) and m.fc.out_features == 2  # the head is replaced after loading


def test_labelling_by_sub_folders_and_by_csv(tmp_path):
    from PIL import Image

    root = make_folder(str(tmp_path / "folders"), n=6)
    ds = tc.LabelledImages(root, image_size=16)
    assert ds.classes == ["bright", "dark"] and [t for _, t in ds.samples] == [0, 0, 0, 1, 1, 1]
    x, t = ds[0]
    assert x.dtype == torch.float32 and x.shape[0] == 3 and min(x.shape[1:]) == 16 and t == 0
    flat = tmp_path / "flat"
    flat.mkdir()
    for i in (10, 2, 7):
        Image.fromarray(np.full((8, 8, 3), i, np.uint8)).save(flat / ("%05d.png" % i))
    with open(tmp_path / "by_number.csv", "w") as f:
        f.write("image_number,gender,age_group\n7,female,30-39\n10,male,0-2\n2,female,20-29\n")
    ds = tc.LabelledImages(str(flat), str(tmp_path / "by_number.csv"), "gender")
    assert [(os.path.basename(p), t) for p, t in ds.samples] == [("00002.png", 1), ("00007.png", 1), ("00010.png", 0)]
    ds = tc.LabelledImages(str(flat), str(tmp_path / "by_number.csv"), "age_group")
    assert ds.classes == ["0-2", "20-29", "30-39"] and [t for _, t in ds.samples] == [1, 2, 0]
    with open(tmp_path / "by_row.csv", "w") as f:
        f.write("gender\nmale\nfemale\nmale\n")
    ds = tc.LabelledImages(str(flat), str(tmp_path / "by_row.csv"), "gender")
    assert [t for _, t in ds.samples] == [0, 1, 0]  # rows against the SORTED file list
    # the transform: PIL bilinear resize of the smaller edge, / 255, ImageNet normalisation
    img = Image.fromarray(np.random.RandomState(0).randint(0, 255, (20, 30, 3)).astype(np.uint8))
    img.save(flat / "99999.png")
    ds = tc.LabelledImages(str(tmp_path / "folders"), image_size=10)
    ds.samples = [(str(flat / "99999.png"), 0)]
    want = torch.from_numpy(np.array(img.resize((15, 10), Image.BILINEAR))).permute(2, 0, 1).float() / 255
    want = (want - torch.tensor(tc._MEAN).view(3, 1, 1)) / torch.tensor(tc._STD).view(3, 1, 1)
    assert torch.equal(ds[0][0], want)


def test_best_validation_checkpoint_and_reload(tmp_path, monkeypatch):
    """Saved when the validation accuracy strictly improves (epochs 0 and 1 of 0.6, 0.9, 0.9, 0.7); the best is reloaded."""
    torch.manual_seed(0)
    model = nn.Sequential(nn.Flatten(), nn.Linear(12, 2))
    data = torch.utils.data.TensorDataset(torch.randn(8, 3, 2, 2), torch.randint(0, 2, (8,)))
    script = iter([0.5, 0.6, 0.5, 0.9, 0.5, 0.9, 0.5, 0.7])
    monkeypatch.setattr(tc, "evaluate_model", lambda *a: next(script))
    saved = []
    real_save = torch.save
    monkeypatch.setattr(torch, "save", lambda sd, path: (saved.append({k: v.clone() for k, v in sd.items()}), real_save(sd, path)))
    path = str(tmp_path / "ck" / "best.pth")
    losses = tc.train_model(model, 0.05, 4, 4, path, torch.device("cpu"), data, data, net=model)
    assert len(losses) == 8 and len(saved) == 2
    assert all(torch.equal(model.state_dict()[k], saved[1][k]) for k in saved[1])
    assert not torch.equal(saved[0]["1.weight"], saved[1]["1.weight"])


def test_continue_training(tmp_path, monkeypatch):
    root = make_folder(str(tmp_path / "d"), n=8, size=16)
    monkeypatch.chdir(tmp_path)
    calls = []
    monkeypatch.setattr(tc, "train_model", lambda model, **kw: calls.append(kw["checkpoint_path"]))
    monkeypatch.setattr(tc, "test_model", lambda *a, **kw: {"accuracy": 0.5})
    argv = ["--data", root, "--pretrained", "random:1", "--image_size", "16", "--num_workers", "0", "--checkpoint_name", "c.pth"]
    os.makedirs("saved_models")
    torch.save(tc.build_model("mobilenet_v2", "random:2").state_dict(), os.path.join("saved_models", "c.pth"))
    tc.main(tc.parse_args(argv))
    assert calls == []  # the checkpoint exists: loaded, tested, not trained
    tc.main(tc.parse_args(argv + ["--continue_training"]))
    assert calls == [os.path.join("saved_models", "c.pth")]
    assert json.load(open(os.path.join("classifier_results", "c.json"))) == {"accuracy": 0.5}
    os.remove(os.path.join("saved_models", "c.pth"))
    tc.main(tc.parse_args(argv))
    assert len(calls) == 2  # no checkpoint: trained


def plain_loop(model, lr, batch_size, epochs, train_dataset, dev):
    """The reference's loop on the plain tv_models module."""
    loader = tc._loader(train_dataset, batch_size, 0, dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    losses = []
    model.train()
    for _ in range(epochs):
        for images, targets in loader:
            loss = nn.CrossEntropyLoss()(model(images), targets)
            losses.append(loss.item())
            opt.zero_grad()
            loss.backward()
            opt.step()
    return losses


@pytest.mark.parametrize("arch", ["mobilenet_v2", "resnet18"])
def test_composable_path_is_the_plain_loop_bit_for_bit(arch, tmp_path):
    root = make_folder(str(tmp_path / "d"), n=24, size=32)
    train, valid, _ = tc.split_dataset(tc.LabelledImages(root, image_size=32))
    dev = torch.device("cpu")
    a, b = tc.build_model(arch, "random:5"), tc.build_model(arch, "random:5")
    fused = tc.training_module(a, dev)
    assert list(fused.state_dict().keys()) == list(b.state_dict().keys()) == list(a.state_dict().keys())
    assert all(p is q for p, q in zip(fused.parameters(), a.parameters()))
    assert sum(isinstance(m, bn_train.BatchNormAct) for m in fused.modules()) == (52 if arch == "mobilenet_v2" else 20)
    torch.manual_seed(11)
    got = tc.train_model(a, 1e-3, 8, 2, str(tmp_path / "a.pth"), dev, train, valid, net=fused)
    torch.manual_seed(11)  # Dropout draws from torch's global stream
    want = plain_loop(b, 1e-3, 8, 2, train, dev)
    assert len(got) == 6
    # train_model evaluates between the epochs (no RNG use, eval mode): the first epoch is comparable outright, the
    # second as well because evaluation changes no state
    assert got == want, (got, want)
    # and in eval mode the fused module is the plain one
    x = torch.randn(2, 3, 32, 32)
    a.load_state_dict(b.state_dict())
    assert torch.equal(fused.eval()(x), b.eval()(x))


def test_batchnormact_eval_is_batchnorm2d_and_state_is_the_parents():
    torch.manual_seed(1)
    ref, m = nn.BatchNorm2d(5), bn_train.BatchNormAct(5, act="relu")
    assert list(m.state_dict().keys()) == list(ref.state_dict().keys())
    ref.running_mean.normal_(), ref.running_var.uniform_(0.5, 2), ref.weight.data.normal_(), ref.bias.data.normal_()
    m.load_state_dict(ref.state_dict(), strict=True)
    x, r = torch.randn(3, 5, 4, 4), torch.randn(3, 5, 4, 4)
    assert torch.equal(m.eval()(x), F.relu(ref.eval()(x)))
    assert torch.equal(m(x, r), F.relu(ref(x) + r))
    m.train(), ref.train()
    m.act = "relu6"
    assert torch.equal(m(x), F.relu6(ref(x))) and int(m.num_batches_tracked) == 1 == int(ref.num_batches_tracked)
    assert torch.equal(m.running_var, ref.running_var)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m(torch.zeros(1, 5, 1, 1))
    assert bn_train.NEED_MORE_VALUES.startswith("Expected more than 1 value per channel when training")


def test_new_entry_points_reject_bad_arguments_without_a_device():
    lib = hip_backend.load_library()
    EINVAL, p, d = -1, ctypes.c_void_p(4096), 1e-5  # p: a non-null, 16-byte aligned address that is never dereferenced
    assert lib.stylex_bn_train_workspace_bytes(0, 4, 4) == -1 and lib.stylex_bn_train_workspace_bytes(2, 4, 49) == 2 * 4 * 8
    assert lib.stylex_bn_train_workspace_bytes(8, 4, 12544) == 2 * 4 * 13 * 8
    assert lib.stylex_softmax_ce_workspace_bytes(4, 1025) == -1 and lib.stylex_softmax_ce_workspace_bytes(4, 1024) == 32
    ws = 1 << 20
    stats = lambda *a: lib.stylex_bn_stats_nchw(*a)  # noqa: E731
    assert stats(None, p, p, None, None, 0.1, 2, 4, 4, p, ws, None) == EINVAL
    assert stats(p, None, p, None, None, 0.1, 2, 4, 4, p, ws, None) == EINVAL
    assert stats(p, p, p, None, None, 0.1, 2, 4, 4, None, ws, None) == EINVAL
    assert stats(p, p, p, p, None, 0.1, 2, 4, 4, p, ws, None) == EINVAL  # one running buffer without the other
    assert stats(p, p, p, None, None, 0.1, 1, 4, 1, p, ws, None) == EINVAL  # n < 2
    assert stats(p, p, p, None, None, 0.1, 2, 4, 4, p, 8, None) == -2  # STYLEX_EWORKSPACE
    fwd = lambda *a: lib.stylex_bn_act_nchw_fwd(*a)  # noqa: E731
    assert fwd(None, p, p, p, p, None, p, d, 2, 4, 4, 0, None) == EINVAL
    assert fwd(p, p, p, p, p, None, None, d, 2, 4, 4, 0, None) == EINVAL
    assert fwd(p, p, p, p, p, None, p, d, 2, 4, 4, 3, None) == EINVAL  # an unknown act
    assert fwd(p, p, p, p, p, None, p, d, 2, 4, 4, -1, None) == EINVAL
    assert fwd(p, p, p, p, p, None, p, d, 2, 0, 4, 1, None) == EINVAL
    red = lambda *a: lib.stylex_bn_act_nchw_bwd_reduce(*a)  # noqa: E731
    assert red(None, p, p, p, p, p, p, d, 2, 4, 4, 1, p, ws, None) == EINVAL
    assert red(p, None, p, p, p, p, p, d, 2, 4, 4, 1, p, ws, None) == EINVAL  # a gate without y
    assert red(p, p, p, p, p, p, p, d, 2, 4, 4, 7, p, ws, None) == EINVAL
    assert red(p, p, p, p, p, p, p, d, 1, 4, 1, 1, p, ws, None) == EINVAL
    assert red(p, p, p, p, p, p, p, d, 2, 4, 4, 1, None, ws, None) == EINVAL
    app = lambda *a: lib.stylex_bn_act_nchw_bwd_apply(*a)  # noqa: E731
    assert app(None, p, p, p, p, p, p, p, p, p, d, 2, 4, 4, 1, None) == EINVAL
    assert app(p, p, p, p, p, p, p, p, None, None, d, 2, 4, 4, 1, None) == EINVAL  # neither output
    assert app(p, p, None, p, p, p, p, p, p, None, d, 2, 4, 4, 1, None) == EINVAL  # gx without x
    assert app(p, p, p, p, p, p, p, p, p, p, d, 2, 4, 4, 5, None) == EINVAL
    assert app(p, p, p, p, p, p, p, p, p, p, d, 1, 4, 1, 1, None) == EINVAL
    assert lib.stylex_softmax_ce_fwd(None, p, p, p, 4, 10, p, ws, None) == EINVAL
    assert lib.stylex_softmax_ce_fwd(p, p, p, p, 4, 1025, p, ws, None) == EINVAL  # K > 1024
    assert lib.stylex_softmax_ce_fwd(p, p, p, p, 0, 10, p, ws, None) == EINVAL
    assert lib.stylex_softmax_ce_fwd(p, p, p, p, 4, 10, p, 8, None) == -2
    assert lib.stylex_softmax_ce_bwd(p, p, None, p, 4, 10, None) == EINVAL
    assert lib.stylex_softmax_ce_bwd(p, p, p, p, 4, 1025, None) == EINVAL


def test_selection_tests_say_no_on_the_cpu():
    m = bn_train.BatchNormAct(3).train()
    assert not m.fused(torch.zeros(2, 3, 4, 4)) and not bn_train.softmax_ce_fused(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
    loss, n_ok = bn_train.softmax_cross_entropy(torch.tensor([[1.0, 2.0], [3.0, 0.0]]), torch.tensor([1, 1]))
    assert int(n_ok) == 1 and torch.equal(loss, F.cross_entropy(torch.tensor([[1.0, 2.0], [3.0, 0.0]]), torch.tensor([1, 1])))
