"""The operand cache's validity policy (stylex/operand_cache.py) on CPU tensors: no event, no stream, no kernel library.
Build functions are counted closures; the GPU side of the same rules (stream ordering, prepack, the fused Adam refresh)
is in test_hip_parity.py."""
import os
import subprocess
import sys

import pytest
import torch

import hip_backend as hb
import operand_cache as oc


@pytest.fixture(autouse=True)
def empty_caches():
    hb.pack_cache_clear()
    yield
    hb.pack_cache_clear()


def param(*shape):
    return torch.nn.Parameter(torch.randn(*shape))


class Doubler:
    """build(): (2 * owner, ...) of the owners' CURRENT values, counting its calls."""

    def __init__(self, *owners):
        self.owners, self.calls = owners, 0

    def __call__(self):
        self.calls += 1
        return tuple(2 * o.detach() for o in self.owners)


def test_unchanged_parameter_builds_once_and_serves_the_same_tensor():
    w = param(4, 3, 3, 3)
    build = Doubler(w)
    first = oc.packs.get((w,), "pack", build, precision=hb.BF16)
    again = oc.packs.get((w,), "pack", build, precision=hb.BF16)
    assert build.calls == 1 and all(a is b for a, b in zip(first, again))
    oc.packs.get((w,), "pack", build, precision=hb.BF16_ACT)  # another variant: its own entry
    assert build.calls == 2 and len(oc.packs) == 2


def test_version_bump_and_stamp_rebuild_in_place():
    w = param(4, 3, 3, 3)
    build = Doubler(w)
    oc.packs.get((w,), "wsq", build)
    n = len(oc.packs)
    with torch.no_grad():
        w.mul_(-0.5)
    (got,) = oc.packs.get((w,), "wsq", build)
    assert build.calls == 2 and torch.equal(got, 2 * w.detach()) and len(oc.packs) == n, "replaced, not accumulated"
    version = w._version
    oc.mark_updated([w])
    oc.packs.get((w,), "wsq", build)
    assert w._version == version and build.calls == 3 and len(oc.packs) == n
    assert hb.mark_updated is oc.mark_updated and hb._gen is oc.stamp


def test_data_swap_rebuilds_pack_vector_and_second_owner():
    """`p.data = other`: same object, same `_version`, new address — every kind must miss."""
    w, b, b2 = param(4, 3, 3, 3), param(4), param(4)
    build = Doubler(w)
    oc.packs.get((w,), "pack", build, precision=hb.BF16)
    calls = [0]

    def twice(t):
        calls[0] += 1
        return 2 * t

    hb.cached_vector("x2", twice, b)
    assert hb.cached_vector("x2", twice, b) is hb.cached_vector("x2", twice, b) and calls[0] == 1
    pair = Doubler(b, b2)
    oc.vectors.get((b, b2), "vec", pair, tag="pair")
    stamps = [oc.stamp(t) for t in (w, b, b2)]
    w.data = w.data.clone() + 1
    b.data = b.data.clone() + 1
    (got,) = oc.packs.get((w,), "pack", build, precision=hb.BF16)
    assert build.calls == 2 and torch.equal(got, 2 * w.detach())
    assert torch.equal(hb.cached_vector("x2", twice, b), 2 * b.detach()) and calls[0] == 2
    oc.vectors.get((b, b2), "vec", pair, tag="pair")
    assert pair.calls == 2
    b2.data = b2.data.clone() + 1  # only the SECOND owner
    got = oc.vectors.get((b, b2), "vec", pair, tag="pair")
    assert pair.calls == 3 and torch.equal(got[1], 2 * b2.detach())
    assert stamps == [oc.stamp(t) for t in (w, b, b2)], "the swaps advanced no stamp: the address alone caught them"


def test_equal_valued_parameter_never_hits():
    w = param(4, 3, 3, 3)
    twin = torch.nn.Parameter(w.detach().clone())
    bw, bt = Doubler(w), Doubler(twin)
    oc.packs.get((w,), "s2d", bw)
    oc.packs.get((twin,), "s2d", bt)
    assert (bw.calls, bt.calls) == (1, 1)
    plain = w.detach().clone()  # not a Parameter: built every time, never kept
    bp = Doubler(plain)
    n = len(oc.packs)
    oc.packs.get((plain,), "s2d", bp), oc.packs.get((plain,), "s2d", bp)
    assert bp.calls == 2 and len(oc.packs) == n


@pytest.mark.parametrize("which", [0, 1])
def test_two_owner_entry_misses_when_either_owner_is_stamped(which):
    w, b = param(4, 3), param(4)
    build = Doubler(w, b)
    oc.packs.get((w, b), "eql", build, lr_mul=0.1)
    oc.packs.get((w, b), "eql", build, lr_mul=0.1)
    assert build.calls == 1
    oc.mark_updated([(w, b)[which]])
    oc.packs.get((w, b), "eql", build, lr_mul=0.1)
    assert build.calls == 2 and len(oc.packs) == 1


def test_capacity_overflow_clears_and_clear_empties_both():
    cache = oc.Cache(3, switched=True, store_capturing=True)
    ws = [param(2, 2) for _ in range(4)]
    builds = [Doubler(w) for w in ws]
    for w, build in zip(ws[:3], builds):
        cache.get((w,), "bf16mat", build)
    assert len(cache) == 3
    cache.get((ws[3],), "bf16mat", builds[3])  # at capacity: cleared wholesale, then stored
    assert len(cache) == 1
    cache.get((ws[0],), "bf16mat", builds[0])
    assert builds[0].calls == 2 and len(cache) == 2
    w, b = param(4, 3, 3, 3), param(4)
    oc.packs.get((w,), "pack", Doubler(w), precision=hb.F32)
    hb.cached_vector("x2", lambda t: 2 * t, b)
    assert len(oc.packs) == 1 and len(oc.vectors) == 1
    hb.pack_cache_clear()
    assert len(oc.packs) == 0 and len(oc.vectors) == 0


def test_cache_check_raises_on_an_unstamped_change(monkeypatch):
    monkeypatch.setattr(oc, "CHECK", True)
    w = param(4, 3, 3, 3)
    build = Doubler(w)
    oc.packs.get((w,), "pack", build, precision=hb.BF16)
    oc.packs.get((w,), "pack", build, precision=hb.BF16)
    w.data.mul_(3.0)  # a raw-kernel style update: same address, no version bump, no stamp
    with pytest.raises(RuntimeError, match="stale operand"):
        oc.packs.get((w,), "pack", build, precision=hb.BF16)


def test_pack_cache_switch_applies_to_packs_only(monkeypatch):
    monkeypatch.setattr(oc, "ON", False)
    w, b = param(4, 3, 3, 3), param(4)
    build, vec = Doubler(w), Doubler(b)
    oc.packs.get((w,), "wsq", build), oc.packs.get((w,), "wsq", build)
    oc.vectors.get((b,), "vec", vec, tag="t"), oc.vectors.get((b,), "vec", vec, tag="t")
    assert build.calls == 2 and vec.calls == 1


def test_adam_copies_selection_and_slot_order():
    """hip_backend._adam_copies_of: which kinds the fused Adam step refreshes, in descriptor slot order — sorted by
    (str(tag), scale, kind code), tag = the precision of a plain pack, else the kind."""
    w = param(4, 3, 3, 3)
    c = 0.5 ** 0.5
    bf = lambda: (torch.zeros(108, dtype=torch.bfloat16), torch.zeros(108, dtype=torch.bfloat16))  # noqa: E731
    put = oc.packs.put
    put((w,), "pack", bf(), precision=hb.BF16)
    put((w,), "pack", bf(), precision=hb.BF16_ACT)
    put((w,), "pack", (torch.zeros(108), torch.zeros(108)), precision=hb.F32)
    put((w,), "pack", (None, bf()[1]), precision=hb.BF16_ACT, scale=c)
    put((w,), "s2d", bf())
    put((w,), "bf16mat", bf()[:1])
    put((w,), "wsq", (torch.zeros(4, 3),))
    put((w,), "padc", (torch.zeros(4, 8, 3, 3),), extra=5)
    put((w,), "fwd_as_dgrad", bf()[:1], precision=hb.BF16_ACT)
    put((w,), "pack", bf(), precision=hb.BF16_ACT, derived=True, extra=5)
    put((w,), "eql", (torch.zeros(4, 3, 3, 3), None), lr_mul=0.1)
    assert len(oc.packs.entries_of(w)) == 11
    got = [(code, scale) for _, code, scale, _, _ in hb._adam_copies_of(w)]
    assert got == [(0, 1.0), (0, c), (0, 1.0), (0, 1.0), (1, 1.0), (2, 1.0)]
    kinds = [(e.kind, e.precision) for e, *_ in hb._adam_copies_of(w)]
    assert kinds == [("pack", hb.BF16), ("pack", hb.BF16_ACT), ("pack", hb.BF16_ACT), ("bf16mat", None), ("s2d", None), ("wsq", None)]
    w.data = w.data.clone()
    assert hb._adam_copies_of(w) == [], "copies of the old storage are not the kernel's to rewrite"


def test_importing_the_cache_loads_no_ctypes():
    """In a fresh interpreter.  torch imports ctypes for its own loader, so the check is what `import operand_cache` ADDS
    to an interpreter that has torch: neither ctypes (were torch to stop) nor hip_backend with its ctypes signature table."""
    src = os.path.dirname(os.path.abspath(oc.__file__))
    code = ("import sys, torch; sys.path.insert(0, %r); had = set(sys.modules); import operand_cache; "
            "new = set(sys.modules) - had; sys.exit(int('ctypes' in new or 'hip_backend' in sys.modules))" % src)
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
