"""Cache of parameter-derived operand copies: packed conv weights, GEMM matrices, tap sums of squares, scaled linear
parameters, bias vectors, the bf16 copy of the no_const transposed-conv weight (`initw`).  The one place that knows what an entry holds and when it may be served (torch only: CPU ranks
import it for `mark_updated` without loading the kernel library).

An entry is served only while every owner is the same live object, at the same address (`p.data = other` and
`module.to(...)` keep the object and its version), with the same modification stamp it was built from."""
import os
import weakref

import torch

ON = os.environ.get("STYLEX_PACK_CACHE", "1") != "0"  # probe switch: 0 = repack on every use
# STYLEX_CACHE_CHECK=1 (debug; costs a host sync per lookup): every entry remembers a checksum of the parameters it was
# built from, and a hit whose parameters no longer have that checksum raises — the failure mode of round 3's
# stale-operand bug (an update path that bumps neither Parameter._version nor the `mark_updated` stamp).
CHECK = os.environ.get("STYLEX_CACHE_CHECK", "0") == "1"
KINDS = ("pack", "s2d", "bf16mat", "wsq", "padc", "fwd_as_dgrad", "eql", "vec", "initw")


def stream_id():
    """Raw handle of the current stream (hip_backend installs its cheaper reader of the same handle)."""
    return int(torch.cuda.current_stream().cuda_stream)


def stamp(t):
    """Modification stamp of a parameter: torch's version counter AND our own generation counter.  The fused Adam
    (torch._fused_adam_, the speed mode's optimiser) updates parameters WITHOUT bumping `_version` (measured: 0 -> 0
    across a step, foreach / plain Adam 0 -> 1), so the Trainer stamps every parameter it steps (`mark_updated`)."""
    return None if t is None else (t._version, getattr(t, "_stylex_gen", 0))


def mark_updated(params):
    """Call after an optimiser step that may not bump Parameter._version: invalidates the cached operand copies."""
    for p in params:
        p._stylex_gen = getattr(p, "_stylex_gen", 0) + 1


def _checksum(owners):
    return tuple((float(w.sum()), float(w.abs().sum())) for w in (o.detach().double() for o in owners))


def _key(owners, kind, precision=None, scale=None, derived=False, extra=None, lr_mul=None, tag=None):
    return (tuple(map(id, owners)), kind, precision, scale, derived, extra, lr_mul, tag)


class Entry:
    """One cached value.  `derived`: built from a tensor computed from the owner (its padded copy), `extra`: the zero
    input channels that copy appends, `tag`: which vector of the owners a `vec` entry holds."""
    __slots__ = ("owners", "ptrs", "stamps", "value", "event", "stream_id", "checksum", "kind", "recipe",
                 "precision", "scale", "derived", "extra", "lr_mul", "tag")

    def __init__(self, owners, key, value, recipe):
        _, self.kind, self.precision, self.scale, self.derived, self.extra, self.lr_mul, self.tag = key  # see _key
        assert self.kind in KINDS, self.kind
        self.owners = tuple(weakref.ref(o) for o in owners)
        self.ptrs = tuple(o.data_ptr() for o in owners)
        self.value, self.recipe = value, recipe


class Cache:
    """One entry per (owners, kind, variant), replaced rather than accumulated; cleared wholesale at `capacity`."""

    def __init__(self, capacity, switched, store_capturing):
        self.capacity, self.switched, self.store_capturing = capacity, switched, store_capturing
        self._entries = {}
        self._of = {}      # id(owner) -> keys of its entries
        self.recipes = {}  # key -> (owner weakrefs, function that builds the entry again): what `prepack` replays

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()
        self._of.clear()

    def lookup(self, owners, kind, **variant):
        """The valid entry, ordered before the current stream's next kernel, or None."""
        e = self._entries.get(_key(owners, kind, **variant)) if ON or not self.switched else None
        if e is None:
            return None
        for ref, ptr, st, o in zip(e.owners, e.ptrs, e.stamps, owners):
            if ref() is not o or o.data_ptr() != ptr or stamp(o) != st:  # (a live object's address cannot be recycled)
                return None
        if CHECK and e.checksum is not None:  # debug: a hit whose source changed without a stamp is a stale operand
            now = _checksum(owners)
            if now != e.checksum:
                raise RuntimeError("stale operand %r served: the parameter changed (checksum %r -> %r) without "
                                   "Parameter._version / mark_updated() advancing" % (e.kind, e.checksum, now))
        # Values may have been produced on another HIP stream (the Trainer forks independent branches over side streams,
        # `prepack` runs on its own): make the consumer stream wait for the producing kernel and keep the block alive for
        # it.  Raw handles first: building a Stream object costs more than the whole lookup.
        if e.event is not None and e.stream_id != stream_id():
            cur = torch.cuda.current_stream()
            cur.wait_event(e.event)
            for t in e.value:
                if t is not None:
                    t.record_stream(cur)
        return e

    def put(self, owners, kind, value, recipe=None, **variant):
        cuda = any(t is not None and t.is_cuda for t in value)  # CPU values: no event, no stream
        if cuda and not self.store_capturing and torch.cuda.is_current_stream_capturing():
            return None
        if len(self._entries) >= self.capacity:
            self.clear()
        key = _key(owners, kind, **variant)
        e = self._entries[key] = Entry(owners, key, value, recipe)
        event = torch.cuda.Event() if cuda else None
        if cuda:
            event.record()
        self.revalidate(e, event, stream_id() if cuda else None)
        for o in owners:
            self._of.setdefault(id(o), set()).add(key)
        if recipe is not None:
            if len(self.recipes) >= 4 * self.capacity:
                self.recipes.clear()
            self.recipes[key] = (e.owners, recipe)
        return e

    def get(self, owners, kind, build, cacheable=True, usable=None, recipe=None, **variant):
        """Lookup, else build and put.  `build()` returns the value tuple; `usable(entry)`: a valid entry may still lack
        what the caller needs (one of the two layouts of a pack).  Only values of Parameters are kept."""
        owners = tuple(o for o in owners if o is not None)
        if not (cacheable and all(isinstance(o, torch.nn.Parameter) for o in owners)):
            return build()
        e = self.lookup(owners, kind, **variant)
        if e is not None and (usable is None or usable(e)):
            return e.value
        value = build()
        self.put(owners, kind, value, recipe, **variant)
        return value

    def entries_of(self, p):
        """Entries of owner `p` at its current address, valid or stale (the fused Adam step rewrites them in place)."""
        found = (self._entries.get(k) for k in self._of.get(id(p), ()))
        return [e for e in found if e is not None and any(r() is p and ptr == p.data_ptr() for r, ptr in zip(e.owners, e.ptrs))]

    def revalidate(self, entry, event, sid):
        """`entry.value` holds what its owners hold now, once `event` (recorded on stream `sid`) has passed: a new entry,
        or one whose value the fused Adam step rewrote in place."""
        owners = tuple(r() for r in entry.owners)
        entry.event, entry.stream_id = event, sid
        entry.stamps = tuple(stamp(o) for o in owners)
        entry.checksum = _checksum(owners) if CHECK else None

    def replay(self, params):
        """[(live owners, recipe)] of every entry whose first owner is one of `params`; forgets entries of dead owners."""
        ids, todo = {id(p) for p in params}, []
        for key, (refs, fn) in list(self.recipes.items()):
            owners = tuple(r() for r in refs)
            if any(o is None for o in owners):
                del self.recipes[key]
                self._entries.pop(key, None)
            elif id(owners[0]) in ids:
                todo.append((owners, fn))
        return todo


packs = Cache(512, switched=True, store_capturing=True)
vectors = Cache(4096, switched=False, store_capturing=False)
