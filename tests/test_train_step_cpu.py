"""The host logic of Trainer.train() that decides what the GPU runs, on the CPU test double: the static (graph) form of
a micro-step against the drawn form, the ONE phase sequence (Trainer._run_step) under its four users, and the
alternating schedule's draw state.  The expected call lists and kinds below were read off the Trainer as it was before
the sequence was shared (three written-out copies: train(), the warm-up branch and the capture closures)."""
import numpy as np
import pytest
import torch

import ops
import stylex_train as st
from cpu_ops import CpuOracleOps
from conftest import load_golden
from test_host_logic_cpu import make_trainer


@pytest.fixture(autouse=True)
def cpu_double():
    prev = ops.use_impl(CpuOracleOps)
    yield
    ops.use_impl(prev)


@pytest.fixture
def trainer(tmp_path):
    tr, _ = make_trainer(load_golden("steps_gae2_alt"), tmp_path, device=torch.device("cpu"))
    assert tr.StylEx.G.num_layers <= 4  # the 16 / 32 px model
    return tr


# ---- 1. static binding equals the drawn form ---------------------------------------------------------------------------


def draw_noise_micro(tr, tt, monkeypatch):
    """A noise micro-step as _draw_d draws it: noise_list (tt None) or mixed_list with its split forced to `tt`."""
    G = tr.StylEx.G
    if tt is None:
        latents = st.noise_list(tr._rank_batch, G.num_layers, tr._z_dim, device=tr.device)
    else:
        with monkeypatch.context() as mp:
            mp.setattr(torch, "rand", lambda *a, **k: torch.tensor((tt + 0.5) / G.num_layers))
            latents = st.mixed_list(tr._rank_batch, G.num_layers, tr._z_dim, device=tr.device)
        assert [n for _, n in latents] == [tt, G.num_layers - tt]
    return st._Micro("noise", st.image_noise(tr._rank_batch, G.image_size, device=tr.device), latents=latents)


def check_binding(tr, e):
    bound = tr._bind_micro("d", 0, e)
    assert bound.kind == "noise_static" and bound.cond is None and bound.batch is None
    with torch.no_grad():
        want = st.styles_def_to_tensor(st.latent_to_w(tr.StylEx.S, e.latents))
        got = tr._styles_of(bound)
    assert got.shape == want.shape and torch.equal(got, want)
    assert torch.equal(bound.inoise, e.inoise) and bound.inoise is not e.inoise
    return bound


@pytest.mark.parametrize("first", ["single", 0, 1, "last"])
@pytest.mark.parametrize("second", ["single", 0, 1, "last"])
def test_static_binding_equals_the_drawn_form(trainer, first, second, monkeypatch):
    """Bind a draw into the static buffers and evaluate the styles; then a second, different draw into the SAME buffers
    (what a replay relies on) — a single-latent draw after a mixed one included: nothing of the earlier z2 / tt stays."""
    tr = trainer
    split = {"single": None, "last": tr.StylEx.G.num_layers - 1}
    a = check_binding(tr, draw_noise_micro(tr, split.get(first, first), monkeypatch))
    b = check_binding(tr, draw_noise_micro(tr, split.get(second, second), monkeypatch))
    assert all(x is y for x, y in zip(a.latents, b.latents)) and a.inoise is b.inoise


def test_bound_encoder_micro_step_encodes_its_conditioning_buffer(trainer):
    tr = trainer
    d = tr._draw_d([0, 1], st._DrawState(), True)
    assert [e.kind for e in d.micro] == ["noise", "enc"] and d.micro[1].batch is d.micro[1].cond
    bound = tr._bind_micro("d", 1, d.micro[1])
    assert bound.kind == "enc" and bound.batch is bound.cond and bound.batch is not d.micro[1].batch
    assert torch.equal(bound.batch, d.micro[1].batch) and torch.equal(bound.inoise, d.micro[1].inoise)


# ---- 2. the users run one sequence -------------------------------------------------------------------------------------

EAGER = ["d_phase", "d_sync", "resolve", "opt_D", "g_phase", "g_sync", "opt_G", "loss_stack"]
WARMUP = ["resolve", "d_phase", "d_sync", "opt_D", "g_phase", "g_sync", "opt_G", "bump", "loss_stack"]
# the three capture closures: seg_d = [accumulators,] d_phase, pack_all | seg_g = opt_D, g_phase, pack_all | seg_tail = opt_G,
# loss_stack; _bump_packs() before each and after the last
CAPTURE = ["resolve", "bump", "d_phase", "d_pack", "bump", "opt_D", "g_phase", "g_pack", "bump", "opt_G", "loss_stack", "bump"]
# the replay loop: graph 0, the previous step's scalars (if a copy is pending), all-reduce D, graph 1, all-reduce G, graph 2
REPLAY = ["resolve", "d_sync", "g_sync", "bump"]
REPLAY_TRACE = ["graph0", "resolve", "d_sync", "graph1", "g_sync", "graph2", "bump"]


def without_sync(calls):
    return [c for c in calls if c not in ("d_sync", "g_sync", "d_pack", "g_pack")]


class FakeSync:
    def __init__(self, which, rec):
        self.all_reduce = lambda: rec(which + "_sync")
        self.pack_all = lambda: rec(which + "_pack")


def recording_trainer(tr, ddp):
    """Phase, sync, optimiser-step, resolve, bump and loss-stack methods replaced by recorders.  `calls` holds their
    names; `trace` additionally holds the markers of the fake segment runners."""
    calls, trace = [], []

    def rec(name, result=None):
        calls.append(name)
        trace.append(name)
        return result

    tr.is_ddp = ddp
    tr._d_sync, tr._g_sync = FakeSync("d", rec), FakeSync("g", rec)
    tr._d_phase = lambda *a, **k: rec("d_phase")
    tr._g_phase = lambda *a, **k: rec("g_phase")
    tr._opt_step = lambda opt: rec("opt_D" if opt is tr.StylEx.D_opt else "opt_G")
    tr._resolve_losses = lambda *a, **k: rec("resolve", setattr(tr, "_pending", None))
    tr._bump_packs = lambda: rec("bump")
    tr._loss_stack = lambda acc: rec("loss_stack", torch.zeros(5))
    tr._new_acc = lambda: {}
    return calls, trace


class FakeGraph:
    """Stands in for torch.cuda.graph: records the segment's body once, when it is captured, and nothing at a replay."""

    def __init__(self, i, trace):
        self.replay = lambda: trace.append("graph%d" % i)


def fake_capture(graphs, trace):
    def run(i, seg):
        graphs.append(FakeGraph(i, trace))
        return seg()
    return run


@pytest.mark.parametrize("ddp", [True, False])
def test_the_users_of_the_step_driver_run_one_sequence(trainer, ddp):
    tr = trainer
    calls, trace = recording_trainer(tr, ddp)
    only = (lambda c: c) if ddp else without_sync
    step = ([[0, 1]], None, None, True, False, 2, True)

    out = tr._run_step("eager", *step, acc={}, st=st._DrawState())
    assert calls == only(EAGER) and out.shape == (5,)

    del calls[:]
    out = tr._run_step("warmup", *step)
    assert calls == only(WARMUP) and out.shape == (5,) and tr._graph_warm == {True}

    del calls[:]
    graphs = []
    out = tr._run_step("capture", *step, run=fake_capture(graphs, trace))
    assert calls == only(CAPTURE) and out.shape == (5,) and len(graphs) == 3

    def replay(i, seg):
        graphs[i].replay()

    del calls[:]
    tr._pending = None  # the capture call itself: its scalars were resolved before the capture
    assert tr._run_step("replay", *step, run=replay) is None
    assert calls == only(REPLAY[1:])
    del calls[:], trace[:]
    tr._pending = object()  # every later call
    tr._run_step("replay", *step, run=replay)
    assert calls == only(REPLAY) and trace == only(REPLAY_TRACE)


@pytest.mark.parametrize("ddp", [True, False])
def test_train_and_the_graph_path_go_through_the_driver(trainer, ddp):
    """The same lists through the production callers: train() (eager) and _train_graphed() — first call of a step shape
    warms up, the second captures and replays, the third replays — with a fake in place of the capturing runner."""
    tr = trainer
    calls, trace = recording_trainer(tr, ddp)
    only = (lambda c: c) if ddp else without_sync
    tr._capture_into = lambda graphs, apply_gp: fake_capture(graphs, trace)
    tr.steps = 1  # a call at step 0 ends with a checkpoint, which resolves once more
    tr.train()
    assert calls == only(EAGER)
    expected = [WARMUP, CAPTURE + REPLAY[1:], REPLAY]
    for want in expected:
        del calls[:]
        out = tr._train_graphed([0, 1], st._DrawState(), False, 2)
        assert calls == only(want) and out.shape == (5,)
        tr._pending = object()
    assert sorted(tr._graph_cache) == [False] and len(tr._graph_cache[False][0]) == 3


def test_the_phase_sequence_is_written_once():
    import inspect

    src = inspect.getsource(st)
    assert src.count("_opt_step(m.D_opt)") == 1 and src.count("_opt_step(m.G_opt)") == 1
    assert 'getattr(self, "_' not in inspect.getsource(st.Trainer)


# ---- 3. the draw state -------------------------------------------------------------------------------------------------

KINDS = {"gae1_alt": [["noise"]] * 3, "gae2_alt": [["noise", "enc"]] * 3}  # D phase and G phase alike, every call


@pytest.mark.parametrize("draw_ahead", [0, 1, 2])
@pytest.mark.parametrize("tag", ["gae1_alt", "gae2_alt"])
def test_alternating_schedule_is_the_same_with_and_without_draw_ahead(tag, draw_ahead, tmp_path):
    tr, _ = make_trainer(load_golden("steps_" + tag), tmp_path, device=torch.device("cpu"))
    assert tr.alternating_training
    tr._draw_mode = draw_ahead
    d_kinds, g_kinds = [], []
    draw_d, draw_g = tr._draw_d, tr._draw_g

    def rec_d(*a):
        out = draw_d(*a)
        d_kinds.append([e.kind for e in out.micro])
        return out

    def rec_g(*a):
        out = draw_g(*a)
        g_kinds.append([e.kind for e in out.micro])
        return out

    tr._draw_d, tr._draw_g = rec_d, rec_g
    for _ in range(3):
        tr.train()
    tr._drain_draw_ahead()
    assert (tr._draw_worker is not None) == (draw_ahead > 0)
    # draw-ahead 2 has prefetched the fourth call's discriminator-phase draw by now (not after the first call: step 0 ends
    # with evaluate / save draws)
    assert len(d_kinds) == (4 if draw_ahead == 2 else 3) and len(g_kinds) == 3
    assert d_kinds[:3] == KINDS[tag] and g_kinds == KINDS[tag]
    assert np.isfinite([tr.d_loss, tr.g_loss]).all()
