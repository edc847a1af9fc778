"""The training variants no_const, rel_disc_loss and top_k_training on the CPU test double: step fixtures captured from
the reference (tools/make_golden_variants.py) in both architectures, the no_const module (state dict, seeded init,
checkpoints), AttFind with no_const, the top-k schedule, the options that stay rejected, the drop-in CLI and two ranks
over gloo.  Without the feature every test here stops at an assert in Generator.__init__ / Trainer.__init__."""
import functools
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attfind
import cli
import networks
import ops
import stylex_train as st
import stylex_train_new as stn
from cpu_ops import CpuOracleOps
from conftest import load_golden
from test_host_logic_cpu import assert_param_stats, make_trainer, run_steps
from test_oracle_vs_golden import assert_same_stats, stats

ALL_ON = dict(no_const=True, rel_disc_loss=True, top_k_training=True, generator_top_k_gamma=0.5, generator_top_k_frac=0.5)
STEP_FIXTURES = ["steps_no_const", "steps_no_const_pl", "steps_rel_disc", "steps_top_k", "steps_newarch_variants"]


@pytest.fixture(autouse=True)
def cpu_double():
    prev = ops.use_impl(CpuOracleOps)
    yield
    ops.use_impl(prev)


def variant_trainer(g, tmp_path, device=None):
    """The Trainer of a steps_* fixture of tools/make_golden_variants.py: its options and its architecture."""
    kw = json.loads(str(g["variant"]))
    cls = stn.Trainer if int(g["new_architecture"]) else st.Trainer
    return make_trainer(g, tmp_path, device=device, trainer_cls=functools.partial(cls, **kw))


def check_steps(name, tmp_path, device=None):
    g = load_golden(name)
    assert (g["thread_spread"] <= 1e-4).all()  # the reference against itself, a tenth of the bound below
    tr, n = variant_trainer(g, tmp_path, device)
    rows = run_steps(tr, n)
    gold = g["scalars"]
    print(name, "rows", rows, "gold", gold, sep="\n")
    np.testing.assert_allclose(rows[0], gold[0], rtol=5e-5, atol=5e-6, equal_nan=True)
    np.testing.assert_allclose(rows, gold, rtol=1e-3, atol=1e-3, equal_nan=True)
    assert_param_stats(tr, g)
    return tr


@pytest.mark.parametrize("name", STEP_FIXTURES)
def test_trainer_step_parity_with_variants_cpu(name, tmp_path):
    tr = check_steps(name, tmp_path)
    assert tr.new_architecture == (name == "steps_newarch_variants")


def test_top_k_fixture_selects_fewer_than_the_batch(tmp_path):
    """steps_top_k starts where k = 2 of 4 (the fixture would pass with the option ignored if k were the batch)."""
    g = load_golden("steps_top_k")
    tr, _ = variant_trainer(g, tmp_path)
    assert tr.top_k_training and tr._generator_top_k() == 2 and tr.batch_size == 4
    g = load_golden("steps_newarch_variants")
    tr, _ = variant_trainer(g, tmp_path)
    assert tr.top_k_training and tr.rel_disc_loss and tr.no_const and tr._generator_top_k() is None


# ---- no_const: the module ----------------------------------------------------------------------------------------------

def no_const_model(g):
    s, cap, fmax = (int(v) for v in g["config"])
    torch.manual_seed(int(g["seed"]))
    return st.StylEx(s, network_capacity=cap, fmap_max=fmax, no_const=True)


def test_no_const_state_dict_keys_and_seeded_init():
    g = load_golden("init_no_const")
    m = no_const_model(g)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert "G.to_initial_block.weight" in sd and "GE.to_initial_block.weight" in sd
    assert not [k for k in sd if k.endswith("initial_block")] and not hasattr(m.G, "initial_block")
    assert isinstance(m.G.to_initial_block, torch.nn.ConvTranspose2d) and m.G.to_initial_block.bias is None
    for i, (k, v) in enumerate(sd.items()):
        assert ",".join(map(str, v.shape)) == str(g["shapes"][i]), k
        assert_same_stats(g["stats"][i], stats(v), k)
    # the default generator is untouched
    torch.manual_seed(0)
    plain = st.StylEx(16, network_capacity=2, fmap_max=16)
    assert "G.initial_block" in plain.state_dict() and not hasattr(plain.G, "to_initial_block")


def test_reference_layout_state_dict_loads_strictly():
    """A state dict in the reference's layout: its keys and shapes as recorded from the reference itself."""
    g = load_golden("init_no_const")
    m = no_const_model(g)
    gen = torch.Generator().manual_seed(3)
    sd = {str(k): torch.randn([int(v) for v in str(s).split(",")] if str(s) else [], generator=gen)
          for k, s in zip(g["keys"], g["shapes"])}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.G.to_initial_block.weight, sd["G.to_initial_block.weight"])
    assert tuple(m.G.to_initial_block.weight.shape) == (514, m.G.initial_conv.weight.shape[1], 4, 4)


def test_first_activation_is_the_reference_formula():
    torch.manual_seed(2)
    G = networks.Generator(16, 514, network_capacity=2, no_const=True, fmap_max=16)
    styles = torch.randn(3, G.num_layers, 514)
    want = G.to_initial_block(styles.mean(dim=1)[:, :, None, None])
    assert torch.equal(G.first_activation(styles), want)
    # x[b, c, i, j] = sum_d mean_l(styles[b, l, d]) * W[d, c, i, j]
    ein = torch.einsum("bd,dcij->bcij", styles.double().mean(dim=1), G.to_initial_block.weight.double())
    assert (want.double() - ein).abs().max().item() < 1e-5


def test_checkpoint_round_trip_with_no_const(tmp_path):
    g = load_golden("steps_no_const")
    tr, _ = variant_trainer(g, tmp_path)
    del tr.save  # make_trainer stubs it out
    tr.train()
    tr.save(0)
    want = {k: v.clone() for k, v in tr.StylEx.state_dict().items()}
    assert json.loads(tr.config_path.read_text())["no_const"] is True
    tr2 = st.Trainer(name="t", base_dir=str(tmp_path), image_size=8, classifier=tr.classifier, lpips_fn=tr.lpips_fn,
                     classifier_name="resnet")  # the configuration comes from the saved config file
    assert not tr2.no_const
    tr2.load(0)
    assert tr2.no_const and tr2.image_size == 32
    got = tr2.StylEx.state_dict()
    assert list(got) == list(want) and "G.to_initial_block.weight" in got
    for k in want:
        assert torch.equal(got[k].cpu(), want[k].cpu()), k


def test_ema_and_averaging_reset_with_no_const():
    torch.manual_seed(4)
    m = st.StylEx(16, network_capacity=2, fmap_max=16, no_const=True)
    with torch.no_grad():
        m.G.to_initial_block.weight.add_(1.0)
    before = m.GE.to_initial_block.weight.clone()
    m.EMA()
    want = before * m.ema_beta + (1 - m.ema_beta) * m.G.to_initial_block.weight
    assert torch.allclose(m.GE.to_initial_block.weight, want)
    m.reset_parameter_averaging()
    assert torch.equal(m.GE.to_initial_block.weight, m.G.to_initial_block.weight)


# ---- AttFind -------------------------------------------------------------------------------------------------------------

def test_attfind_with_no_const_equals_unbatched_generator_forwards():
    """16 px model with no_const: every coordinate's perturbed image from the batched prefix / suffix walk equals a plain
    G(...) forward with the block's style bias moved (what the reference notebook does); the first activation depends on
    w, not on the bias, so the cached prefix serves every perturbation."""
    torch.manual_seed(5)
    m = st.StylEx(16, network_capacity=4, fmap_max=32, no_const=True)
    G = m.G
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in G.parameters():  # leave the zero-initialised noise maps non-trivial
            if p.abs().sum() == 0:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
        w = torch.randn(1, 514, generator=gen)
        noise = torch.rand(1, 16, 16, 1, generator=gen)
        w_tensor = attfind.styles_def_to_tensor([(w, G.num_layers)])
        states = attfind._prefix_states(G, w_tensor, noise)
        for k, block in enumerate(G.blocks):
            x_k, rgb_k, s1, s2 = states[k]
            for coord in range(block.num_style_coords):
                first = coord < block.input_channels
                j = coord if first else coord - block.input_channels
                d1, d2 = torch.zeros_like(s1), torch.zeros_like(s2)
                (d1 if first else d2)[0, j] = 0.7
                got = attfind._suffix(G, k, x_k, rgb_k, w_tensor, noise, (s1 + d1, s2 + d2))
                lin = block.to_style1 if first else block.to_style2
                lin.bias[j] += 0.7
                want = G(w_tensor, noise)
                lin.bias[j] -= 0.7
                assert (got - want).abs().max().item() <= 1e-5, (k, coord)


def test_change_images_runs_with_no_const():
    from standins import TinyClassifier

    torch.manual_seed(7)
    m = st.StylEx(16, network_capacity=4, fmap_max=32, no_const=True)
    gen = torch.Generator().manual_seed(8)
    w = torch.randn(3, 514, generator=gen)
    noise = torch.rand(1, 16, 16, 1, generator=gen)
    base, changed, p0, p1 = attfind.change_images(m.G, TinyClassifier(seed=1), w.numpy(), 5, 1, -1.0, 1.0, 1.0, noise)
    assert base.shape == changed.shape == (3, 3, 16, 16) and p0.shape == p1.shape == (3,)
    with torch.no_grad():
        want = m.G(attfind.styles_def_to_tensor([(w, m.G.num_layers)]), noise.expand(3, -1, -1, -1))
    assert (base - want).abs().max().item() <= 1e-5
    assert (changed - base).abs().max().item() > 0


# ---- the losses ------------------------------------------------------------------------------------------------------------

def test_composable_losses_are_the_reference_expressions():
    gen = torch.Generator().manual_seed(9)
    real, fake = torch.randn(6, generator=gen), torch.randn(6, generator=gen)
    want = (F.relu(1 + (real - fake.mean())) + F.relu(1 - (fake - real.mean()))).mean()
    assert torch.equal(st.hinge_loss(real, fake, True), want)
    assert torch.equal(st.hinge_loss(real, fake), (F.relu(1 + real) + F.relu(1 - fake)).mean())
    assert torch.equal(st.gen_hinge_loss(fake, None, 2), fake.topk(k=2, largest=False)[0].mean())
    assert torch.equal(st.gen_hinge_loss(fake, None, 6), fake.mean()) and torch.equal(st.gen_hinge_loss(fake, None), fake.mean())


def reference_k(steps, batch_size, gae, n_data, gamma, frac):
    """reference stylex_train.py:1402-1404"""
    epochs = (steps * batch_size * gae) / n_data
    k_frac = max(gamma ** epochs, frac)
    return math.ceil(batch_size * k_frac)


def test_top_k_schedule_is_the_reference_expression(tmp_path):
    from lpips_standin import LPIPSStandIn
    from standins import TinyClassifier

    cls, lp = TinyClassifier(seed=1), LPIPSStandIn(seed=2)
    seen_full = seen_less = seen_exact = 0
    for batch, gae, n_data, gamma, frac in [(4, 2, 1000, 0.5, 0.5), (8, 1, 64, 0.99, 0.5), (5, 3, 300, 0.9, 0.2),
                                            (16, 1, 16, 0.5, 0.25), (3, 2, 10, 0.7, 0.34)]:
        tr = st.Trainer(name="k", base_dir=str(tmp_path), image_size=16, network_capacity=2, fmap_max=16, batch_size=batch,
                        gradient_accumulate_every=gae, classifier=cls, lpips_fn=lp, device=torch.device("cpu"),
                        top_k_training=True, generator_top_k_gamma=gamma, generator_top_k_frac=frac)
        tr.dataset = list(range(n_data))
        for steps in (0, 1, 2, 3, 7, 16, 50, 125, 1000, 20000):
            tr.steps = steps
            want = reference_k(steps, batch, gae, n_data, gamma, frac)
            got = tr._generator_top_k()
            assert got == (None if want == batch else want), (batch, gae, n_data, gamma, frac, steps, got, want)
            seen_full += want == batch
            seen_less += want < batch
            # the ceil lands on an integer: batch * k_frac is one already
            k_frac = max(gamma ** ((steps * batch * gae) / n_data), frac)
            seen_exact += float(batch * k_frac).is_integer() and want < batch
    assert seen_full >= 5 and seen_less >= 20 and seen_exact >= 5, (seen_full, seen_less, seen_exact)
    off = st.Trainer(name="k", base_dir=str(tmp_path), image_size=16, network_capacity=2, fmap_max=16, classifier=cls,
                     lpips_fn=lp, device=torch.device("cpu"))
    assert off._generator_top_k() is None and not off.rel_disc_loss and not off.top_k_training


# ---- what stays rejected ---------------------------------------------------------------------------------------------------

def test_rejected_options_name_their_reasons(tmp_path):
    from lpips_standin import LPIPSStandIn
    from standins import TinyClassifier

    kw = dict(name="r", base_dir=str(tmp_path), image_size=16, network_capacity=2, fmap_max=16, batch_size=2,
              classifier=TinyClassifier(seed=99), lpips_fn=LPIPSStandIn(seed=4242), device=torch.device("cpu"))
    recorded = str(load_golden("steps_rel_disc")["dual_contrast_loss_error"])
    assert recorded == "ValueError: too many values to unpack (expected 2)"
    with pytest.raises(RuntimeError) as e:
        st.Trainer(dual_contrast_loss=True, **kw)
    assert recorded in str(e.value) and "stylex_train.py:1398" in str(e.value)
    with pytest.raises(AssertionError, match="vector_quantize_pytorch"):
        st.Trainer(fq_layers=[1], **kw)
    with pytest.raises(AssertionError, match="contrastive_learner"):
        st.Trainer(cl_reg=True, **kw)
    with pytest.raises(AssertionError, match="apex"):
        st.Trainer(fp16=True, **kw)
    # the second architecture: top-k with k < batch has no reference behaviour either
    recorded = str(load_golden("steps_newarch_variants")["top_k_error"])
    tr = stn.Trainer(top_k_training=True, generator_top_k_gamma=0.5, **kw)
    tr.dataset = list(range(10))
    tr.steps = 0
    assert tr._generator_top_k() is None
    tr.steps = 100
    with pytest.raises(RuntimeError) as e:
        tr._generator_top_k()
    assert recorded in str(e.value) and "stylex_train_new.py:1472" in str(e.value)


# ---- the drop-in CLI ---------------------------------------------------------------------------------------------------------

def test_train_from_folder_with_the_three_flags_cpu(tmp_path):
    from PIL import Image

    data = tmp_path / "imgs"
    data.mkdir()
    rng = np.random.RandomState(0)
    for i in range(6):
        Image.fromarray(rng.randint(0, 255, (40, 48, 3), dtype=np.uint8)).save(data / f"{i}.png")
    cli.train_from_folder(str(data), str(tmp_path / "results"), str(tmp_path / "models"), "v", True, image_size=32,
                          network_capacity=4, fmap_max=64, batch_size=2, gradient_accumulate_every=2, num_train_steps=2,
                          num_workers=0, save_every=1, evaluate_every=1, tensorboard_dir=None, classifier_path=None,
                          no_const=True, rel_disc_loss=True, top_k_training=True, generator_top_k_gamma=0.01)
    assert (tmp_path / "models" / "v" / "model_1.pt").exists()
    cfg = json.loads((tmp_path / "models" / "v" / ".config.json").read_text())
    assert cfg["no_const"] is True
    ck = torch.load(tmp_path / "models" / "v" / "model_1.pt")
    assert "G.to_initial_block.weight" in ck["StylEx"] and "G.initial_block" not in ck["StylEx"]
    assert all(torch.isfinite(v).all() for v in ck["StylEx"].values() if torch.is_floating_point(v))


# ---- two ranks over gloo -----------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_worker(rank, world, port, tmp, q):
    import random
    import sys

    import torch.distributed as dist

    err = open(os.path.join(tmp, "rank%d.stderr" % rank), "w")  # a full pipe must not be able to block a rank
    os.dup2(err.fileno(), 2)
    sys.stderr = err
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lpips_standin import LPIPSStandIn
        from standins import TinyClassifier

        ops.use_impl(CpuOracleOps)
        size, bs = 32, 4  # global batch 4 -> 2 per rank
        gd = torch.Generator().manual_seed(7 + rank)
        batches = [torch.rand(bs // world, 3, size, size, generator=gd) for _ in range(8)]
        torch.manual_seed(1000 + rank)
        tr = st.Trainer(name="r%d" % rank, base_dir=tmp, image_size=size, network_capacity=4, fmap_max=64, batch_size=bs,
                        gradient_accumulate_every=2, lr=2e-4, ttur_mult=1.5, rec_scaling=1, kl_scaling=1,
                        classifier=TinyClassifier(seed=99), lpips_fn=LPIPSStandIn(seed=4242), classifier_name="resnet",
                        evaluate_every=10 ** 9, save_every=10 ** 9, is_ddp=True, rank=rank, world_size=world,
                        device=torch.device("cpu"), **ALL_ON)
        tr.loader = st.cycle(batches)
        tr.dataset = list(range(1000))
        tr.save = lambda *a, **k: None
        tr.evaluate = lambda *a, **k: None
        tr.init_StylEx()
        tr.steps = 1003  # neither a penalty nor an averaging-reset call; k = 1 of the 2 samples of a rank
        k = tr._generator_top_k()
        trained = lambda: [p for n, p in tr.StylEx.named_parameters() if not n.startswith(("GE.", "SE."))]  # noqa: E731
        w0 = torch.cat([p.detach().reshape(-1) for p in trained()])
        random.seed(5 + rank)
        np.random.seed(5 + rank)
        torch.manual_seed(5 + rank)
        for _ in range(2):
            tr.train()
        w1 = torch.cat([p.detach().reshape(-1) for p in trained()])
        gathered = [torch.zeros_like(w1) for _ in range(world)]
        dist.all_gather(gathered, w1)
        first = dict(tr.StylEx.named_parameters())["G.to_initial_block.weight"]
        q.put((rank, k, all(torch.equal(gathered[0], t) for t in gathered), float((w1 - w0).abs().max()),
               tr.d_loss, tr.g_loss, first.grad is not None and float(first.grad.abs().max()) > 0))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_gloo_with_the_three_options(tmp_path):
    import torch.multiprocessing as mp

    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=500) for _ in range(world)]
    except Exception:
        for r in range(world):
            print(open(os.path.join(str(tmp_path), "rank%d.stderr" % r)).read()[-4000:])
        raise
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, k, same, moved, d_loss, g_loss, first_grad in res:
        assert k == 1, k
        assert same, "replicas diverged after two all-reduced steps with the three options on"
        assert moved > 0 and first_grad
        assert np.isfinite(d_loss) and np.isfinite(g_loss)
