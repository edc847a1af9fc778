"""Data-parallel plumbing: one process per GPU, ``torch.distributed`` (backend "nccl" = RCCL
over xGMI on ROCm; "gloo" in the CPU tests).

The reference's multi-GPU path is vestigial (DDP wrappers around S/G/D only, the encoder is never
wrapped — stylex/stylex_train.py:1188-1193, README.md:81).  Here gradient exchange is explicit
(class GradSync): the gradients of a phase live in persistent flat fp32 buckets (every .grad is a
view after the bucket's pack) that are all-reduced in place, averaged by the collective itself
(ReduceOp.AVG on RCCL).  DEFAULT since round 5 (the design SURVEY §8(e) specifies): 32 MB buckets
launched from autograd hooks INSIDE the last backward of the phase, strictly in index order on
every rank — the path the gloo tests (2 and 4 ranks), the 1-rank RCCL identity test and the
2-rank gloo run of bench.py exercise, so that what ships is what is tested the day a multi-GPU box
appears.  ``STYLEX_DDP_OVERLAP=0`` / ``GradSync(overlap=False)``: 128 MB buckets issued AFTER the
backward.  Non-final micro-steps never communicate (== ``no_sync``, :274-285).
"""
import os

import torch
import torch.distributed as dist


def is_dist():
    """True inside an initialised process group (a 1-rank group still runs the collectives: used to smoke-test
    the RCCL path on a single-GPU box)."""
    return dist.is_available() and dist.is_initialized()


def broadcast_parameters(module, src=0):
    """Make every rank start from rank-``src`` weights and buffers."""
    if not is_dist():
        return
    import operand_cache

    with torch.no_grad():
        ts = list(module.parameters()) + list(module.buffers())
        for t in ts:
            dist.broadcast(t.detach(), src=src)  # detach() shares the version counter (t.data has its own)
    # the broadcast writes through a detached alias: stamp the parameters so that no cached operand pack made from the
    # pre-broadcast weights can be served (operand_cache.stamp)
    operand_cache.mark_updated(ts)


def _backend_averages():
    """ReduceOp.AVG exists on RCCL only; over gloo (the CPU tests, and the two-ranks-on-one-GPU test that runs the HIP
    kernels under a real two-rank exchange) the buckets are summed and divided by the world size afterwards."""
    return dist.get_backend() == "nccl"


class GradSync:
    """Bucketed gradient all-reduce on persistent flat buffers, overlapped with the backward pass.

    Parameters are grouped into persistent flat fp32 buckets in reverse order (~ the order their gradients become
    ready).  A bucket's gradients are moved into it by ONE multi-tensor copy right before its collective, and from
    then on every ``p.grad`` IS a view into the bucket: the collective runs on the bucket directly, nothing is
    scattered back, the optimiser reads the reduced values in place, and the buffers are the same on every step
    (also under HIP-graph replay).  `arm()` before the last
    backward of a phase turns on per-parameter post-accumulate hooks: when every gradient of the next bucket IN INDEX
    ORDER is ready its all-reduce is launched from inside the backward, so the xGMI transfer runs under the rest of
    the backward (a 2-GPU all-reduce of the 400 MB of a step is ~7 ms on one xGMI link).  Buckets are launched
    strictly in index order on every rank — the collective sequence never depends on which gradient happened to
    arrive first.  `all_reduce()` after the backward launches what is left and waits.  Without `arm()` everything is
    launched by `all_reduce()` (same result).  Non-final micro-steps never communicate (== ``no_sync``,
    reference stylex_train.py:274-285)."""

    def __init__(self, params, bucket_bytes=None, overlap=None):
        # Default (round 5): the in-backward launch — 32 MB buckets from autograd hooks.  Rounds 3-4 kept it opt-in for
        # want of a >= 2-GPU RCCL run; no such box exists in this environment, and a default nobody tests is worse than a
        # default the gloo tests, the 1-rank RCCL identity test and bench.py's 2-rank gloo run all go through.
        # STYLEX_DDP_OVERLAP=0: few large (128 MB) collectives issued after the backward.
        import os

        self.overlap = (os.environ.get("STYLEX_DDP_OVERLAP", "1") == "1") if overlap is None else bool(overlap)
        if bucket_bytes is None:
            bucket_bytes = (32 if self.overlap else 128) * 1024 * 1024
        seen, self.params = set(), []
        for p in params:
            if id(p) not in seen and p.requires_grad:
                seen.add(id(p))
                self.params.append(p)
        self.buckets, cur, cur_bytes = [], [], 0
        for p in reversed(self.params):  # reverse order ~ the order gradients become ready
            cur.append(p)
            cur_bytes += p.numel() * 4
            if cur_bytes >= bucket_bytes:
                self.buckets.append(cur)
                cur, cur_bytes = [], 0
        if cur:
            self.buckets.append(cur)
        self._bucket_of = {id(p): bi for bi, bucket in enumerate(self.buckets) for p in bucket}
        self.flats, self._views = [], {}
        for bucket in self.buckets:
            # every view starts on a 16-byte boundary: the fused Adam + pack kernel reads gradients with float4 loads
            # (csrc/adam_pack.hip), and a view behind an odd-sized bias would otherwise be 4-byte aligned only
            flat = torch.zeros(sum((p.numel() + 3) & ~3 for p in bucket), dtype=torch.float32, device=bucket[0].device)
            off = 0
            for p in bucket:
                self._views[id(p)] = flat[off:off + p.numel()].view_as(p)
                off += (p.numel() + 3) & ~3
            self.flats.append(flat)
        self._armed = False
        # First-use self-check of the in-backward launch path (round 6, ADVICE): no >= 2-GPU RCCL run of it exists, so the
        # first `checks` overlapped all_reduce() calls verify what MUST hold afterwards on any correct run — every rank
        # holds the SAME averaged buckets — with two tiny collectives (MAX and MIN of a per-bucket checksum vector).  A
        # mismatch (a bucket reduced before its gradients were complete on some rank, buckets launched in different orders)
        # falls back to the post-backward path with a warning instead of training on corrupt gradients.
        self._selfcheck_left = int(os.environ.get("STYLEX_DDP_SELFCHECK", "2")) if self.overlap else 0
        self._reset()
        with torch.no_grad():
            for p in self.params:  # adopt gradients that already exist, then bind every .grad to its view
                v = self._views[id(p)]
                if p.grad is not None:
                    v.copy_(p.grad)
                p.grad = v
        for p in self.params:
            p.register_post_accumulate_grad_hook(self._on_grad)

    def _reset(self):
        self._nograd = []
        self._ready = [0] * len(self.buckets)
        self._streams = [set() for _ in self.buckets]  # HIP streams that produced gradients of the bucket
        self._next = 0
        self._works = []

    @torch.no_grad()
    def zero_grad(self):
        """Replaces optimizer.zero_grad(): every .grad is dropped, so that autograd hands each parameter its freshly
        computed gradient by reference (no add launch per parameter, no 400 MB fill per step).  The gradients are moved
        into the persistent flat bucket — ONE multi-tensor copy per bucket — right before the bucket's collective
        (`_launch`), after which .grad IS the bucket view the optimiser reads.  Measured on the 1-rank RCCL path:
        accumulating in place into pre-bound views cost ~450 tiny add launches per step (664 vs 720 images/s)."""
        for p in self.params:
            p.grad = None

    def no_sync(self):
        from contextlib import nullcontext

        return nullcontext()  # collectives only ever start after arm() / all_reduce()

    def arm(self):
        """Call right before the last backward of the phase (earlier micro-step backwards only accumulate)."""
        if is_dist() and self.overlap:
            self._reset()
            self._armed = True

    def _on_grad(self, p):
        if not self._armed:
            return
        bi = self._bucket_of[id(p)]
        if p.grad is not None and p.grad.is_cuda:
            # gradients of one bucket may be produced on different HIP streams: remember WHICH (a hash insert), and make
            # the launching stream wait for the others once, when the bucket is complete (`_launch`).  Rounds 3-5 recorded
            # one event per parameter gradient here (~230 event objects + records per step: 3 % of a 1-rank step)
            self._streams[bi].add(torch.cuda.current_stream())
        self._ready[bi] += 1
        while self._next < len(self.buckets) and self._ready[self._next] == len(self.buckets[self._next]):
            self._launch(self._next)

    @torch.no_grad()
    def pack_all(self):
        """Move every gradient into its bucket and bind .grad to the views, without communicating.  Used at the end of
        a CAPTURED phase: the copies become part of the HIP graph (a replay recomputes the gradients into the
        capture-time tensors and these copies refill the buckets), the collectives are issued eagerly afterwards.
        A parameter WITHOUT a gradient in the captured phase keeps ``.grad = None`` (its bucket slice is zeroed inside
        the graph for the collective), so the optimiser step captured next skips it exactly as the eager path and a
        single GPU do — binding the zeroed view would make the captured Adam advance its step count and decay its
        moments on every replay."""
        captured = bool(self.flats) and self.flats[0].is_cuda and torch.cuda.is_current_stream_capturing()
        for bi in range(len(self.buckets)):
            self._pack(bi, bind_nograd=not captured)

    @torch.no_grad()
    def _launch(self, bi):
        assert bi == self._next
        if self._streams[bi]:
            cur = torch.cuda.current_stream()
            import ops  # in-launch accumulation of twice-used blocks: streams that added into a gradient behind the engine's back

            for st in ops._GACC_STREAMS:
                if st != cur:
                    cur.wait_stream(st)
            for st in self._streams[bi]:
                if st != cur:
                    cur.wait_stream(st)  # one event per (bucket, foreign producing stream), recorded now: everything that
                    #                      stream has enqueued so far, the bucket's gradients included
        self._pack(bi)
        flat = self.flats[bi]
        avg = _backend_averages()  # RCCL averages inside the collective; gloo has no AVG (sum, then divide in all_reduce())
        self._works.append(dist.all_reduce(flat, op=dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM, async_op=True))
        self._next += 1

    @torch.no_grad()
    def _pack(self, bi, bind_nograd=True):
        dst, src = [], []
        for p in self.buckets[bi]:
            v = self._views[id(p)]
            if p.grad is None:  # no gradient this phase: contributes zeros to the collective ...
                v.zero_()
                if not bind_nograd:
                    continue
                self._nograd.append(p)  # ... and goes back to None afterwards (all_reduce), as on one GPU
            elif p.grad is not v:
                dst.append(v)
                src.append(p.grad)
            p.grad = v
        if dst:
            torch._foreach_copy_(dst, src)  # one multi-tensor launch moves the bucket's gradients into the flat buffer

    @torch.no_grad()
    def all_reduce(self):
        if not is_dist():
            return
        armed_run = self._armed
        if not self._armed:
            self._reset()
        self._armed = False
        world = dist.get_world_size()
        while self._next < len(self.buckets):
            self._launch(self._next)
        avg = _backend_averages()
        for flat, work in zip(self.flats, self._works):
            work.wait()
            if not avg:
                flat.div_(world)
        if self._selfcheck_left > 0 and self.overlap and world > 1 and armed_run:
            self._selfcheck_left -= 1
            self._selfcheck()
        # A parameter without a gradient in this phase has none on ANY rank (every rank runs the same schedule: same
        # phase, same micro-steps, same alternating / encoder switches), so its reduced "gradient" is exactly zero.
        # Leave .grad = None as the single-GPU path and the reference's DDP do — Adam then skips the parameter instead
        # of advancing its step count and decaying its moments with a zero gradient.
        for p in self._nograd:
            p.grad = None
        self._reset()


def _gradsync_selfcheck(self):
    """Every rank must hold identical buckets after the averaging collectives: compare a checksum per bucket across
    the ranks (MAX == MIN).  One host sync, on the first overlapped steps only."""
    import warnings

    sums = torch.stack([f.double().sum() + f.double().abs().sum() * 1e-3 for f in self.flats])
    hi, lo = sums.clone(), sums.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    scale = hi.abs().clamp_min(1e-30)
    bad = ((hi - lo).abs() / scale > 1e-6) | ~torch.isfinite(hi - lo)
    if bool(bad.any()):
        self.overlap = False
        warnings.warn("GradSync: the ranks disagree on %d of %d averaged gradient buckets after the in-backward launch path; "
                      "falling back to the post-backward all-reduce (STYLEX_DDP_OVERLAP=0)" % (int(bad.sum()), len(self.flats)))
    return not bool(bad.any())


GradSync._selfcheck = _gradsync_selfcheck


def all_reduce_max_(t):
    """In-place MAX over the ranks, no host synchronisation (the NaN flag of a step rides this)."""
    if is_dist():
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t


def all_reduce_scalar_flag(flag, device):
    """OR of a boolean across ranks (used so that every rank agrees on a NaN restart)."""
    if not is_dist():
        return flag
    t = torch.tensor([1.0 if flag else 0.0], device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return bool(t.item() > 0)
