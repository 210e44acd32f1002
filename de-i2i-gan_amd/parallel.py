"""Data-parallel minibatch sharding: one process per GPU, gradient all-reduce over RCCL/xGMI overlapped with backward.

The reference is single-device; this is the build's addition (section 8e).  Design for the
MI355X node (8 GPUs, point-to-point xGMI, no switch):

* Each rank runs the full D step and G step on its shard of the batch; the only exchange is SUM all-reduce of the
  gradients that step produced.  The 1/world averaging is folded into the fused Adam kernel's ``grad_scale`` -- no
  extra pass over the gradients.
* Overlap: a ``post_accumulate_grad`` hook fires as soon as autograd has finished a parameter's gradient.  Large
  gradients (>= ``direct_bytes``) are all-reduced in place immediately, small ones are coalesced into flat buckets of
  ``bucket_bytes``.  Collectives are issued on a dedicated side stream that waits on an event recorded on the compute
  stream, so RCCL traffic runs under the remaining backward kernels.  Backward reaches the discriminator's 134 MB
  ``enc_blk.5`` weight gradient first, so the biggest message has the whole rest of backward to hide behind.
* Every rank sees the same autograd graph, so hooks fire in the same order on every rank and the collective
  sequence matches without negotiation.  Parameters that get no gradient in a step (the never-executed
  ``norm_s`` / ``conv_s``; all of D during the G step) simply never enter a collective.
* BatchNorm statistics stay local (per-shard), like torch DDP without SyncBN; ``broadcast_buffers`` copies rank 0's
  running stats to every rank (torch DDP ``broadcast_buffers`` semantics) -- parity definition in SURVEY.md 8e.
* ``sync_bn=True`` (DefectGanTrainer / MAETrainer, opt-in): synchronised BatchNorm.  Every training-mode BatchNorm of the generator
  takes its statistics, and its backward its two reductions, over the GLOBAL batch: N ranks, each on its rows, then compute what ONE
  process computes on the whole batch (the reference's own single-process run; tests/test_ddp_sync_bn_gpu.py holds two ranks to its
  goldens) instead of the gradient-accumulation semantics above.  Mechanism (``ops.bn_sync``): each layer's finalize runs as stage 1 (this
  rank's records -> one fp64 message for all groups of the layer: 2C + 1 doubles per group forward, 2C backward), a SUM all-reduce of
  that message in the compute stream's order, stage 2 (finalize / apply from the summed message).  The messages travel on a process
  group of their own (``dist.new_group``) so that the latency-bound messages of backward need not queue behind the gradient buckets on
  the gradients' communicator -- the reason for the second group, not a measured result.  dweight / dbias of the layer stay LOCAL: the
  gradient exchange sums parameter gradients over ranks afterwards, the global sums would be counted ``world`` times.  Every rank
  computes the same running statistics from the same summed message, so ``broadcast_buffers`` does nothing.  The MAE stage draws its
  patch mask for the global batch on every rank (same RNG consumption; rank 0's CPU RNG state is broadcast at attach) and keeps its
  rows.  Every rank must hold the same number of rows.  The equality covers the SPADE generator with the default options,
  ``use_spectral`` and ``cycle_gan``; ``add_noise``, ``diff_aug`` and the SEAN blocks' host-drawn embeddings are per-rank random numbers: they run with
  ``sync_bn`` but equal no single-process run (``opt.embed_rng = "device"`` with one ``embed_seed`` draws the global batch's embeddings,
  each rank its rows: ops.embed_draw's ``row0``).  Counted apart from the gradients: ``stats["sync_bn_collectives"]`` / ``["sync_bn_bytes"]``.
  Off (the default): nothing changes -- same kernels, same launches, same bits.  Eval-mode BatchNorm never exchanges.
* ``attach_ddp`` broadcasts rank 0's parameters and buffers (spectral-norm u / v included) once, one flat message per
  network, like torch DDP does at construction: replicas start identical whatever each rank's seed or checkpoint was.
* ``measure=True`` brackets every collective with events on the side stream and marks the end of backward on the compute
  stream; ``overlap_report()`` then says how much of the exchange ran under backward kernels (bench.py prints it).
* ``comm_dtype="bf16"``: the messages travel as bf16 (half the bytes on the per-link-bound xGMI rings: D's step is 180 MB in fp32,
  134 MB of it one tensor): each gradient is rounded to bf16 on the side stream, summed by RCCL in bf16, and widened back into
  the fp32 gradient the optimizer reads; the 1/world stays in Adam.  One rounding of every addend and of every partial sum
  (2^-9 relative each): tests/test_ddp_gloo.py bounds the error against the fp32 exchange.  Default fp32 (bit-exact sums).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import time

import torch
import torch.distributed as dist


class GradReducer:
    def __init__(self, process_group=None, bucket_bytes: int = 16 << 20, direct_bytes: int = 4 << 20, overlap: bool = True,
                 force_collectives: bool = False, measure: bool = False, comm_dtype: str = "fp32", sync_bn: bool = False,
                 stats_group=None):
        if not dist.is_initialized():
            raise RuntimeError("GradReducer needs an initialised torch.distributed process group")
        self.pg = process_group
        self.world, self.rank = dist.get_world_size(process_group), dist.get_rank(process_group)
        self.sync_bn = bool(sync_bn)
        self.stats_pg = stats_group if stats_group is not None else process_group      # BatchNorm statistics messages (attach_ddp: own group)
        self.bucket_bytes, self.direct_bytes, self.overlap = bucket_bytes, direct_bytes, overlap
        self.active = self.world > 1 or force_collectives      # force: run the collective path on a 1-rank group (tests)
        self._attached = set()
        self._side: Dict[torch.device, torch.cuda.Stream] = {}
        self._bucket: List[torch.Tensor] = []
        self._bucket_nbytes = 0
        self._inflight = []          # (work, flat, [grads]) to finish in reduce()
        self.stats = {"collectives": 0, "bytes": 0, "sync_bn_collectives": 0, "sync_bn_bytes": 0}
        self.measure = measure
        if comm_dtype not in ("fp32", "bf16"):
            raise ValueError(f"comm_dtype [{comm_dtype}] is not supported (fp32 | bf16)")
        self.comm_dtype = torch.bfloat16 if comm_dtype == "bf16" else torch.float32
        self._spans = []             # measure: (start event, end event) of every collective, on the side stream
        self._bwd_done = []          # measure: compute-stream event at the entry of reduce() = backward's last kernel
        self._span_marks = []        # index into _spans at each reduce() call

    # ---- wiring ------------------------------------------------------------------------------------------
    def attach(self, net: torch.nn.Module) -> None:
        """Register the gradient-ready hooks (once per network)."""
        if id(net) in self._attached:
            return
        self._attached.add(id(net))
        if not self.overlap:
            return
        for p in net.parameters():
            p.register_post_accumulate_grad_hook(self._on_grad_ready)

    def _comm_stream(self, device):
        if device.type != "cuda":
            return None
        s = self._side.get(device)
        if s is None:
            s = torch.cuda.Stream(device=device)
            self._side[device] = s
        return s

    # ---- hook path (during backward) ---------------------------------------------------------------------
    def _on_grad_ready(self, p: torch.Tensor) -> None:
        g = p.grad
        if g is None or not self.active:
            return
        nbytes = g.numel() * g.element_size()
        if nbytes >= self.direct_bytes:
            self._launch([g], flat=None)
        else:
            self._bucket.append(g)
            self._bucket_nbytes += nbytes
            if self._bucket_nbytes >= self.bucket_bytes:
                self._flush_bucket()

    def _flush_bucket(self) -> None:
        if self._bucket:
            grads, self._bucket, self._bucket_nbytes = self._bucket, [], 0
            self._launch(grads, flat=True)

    def _launch(self, grads: List[torch.Tensor], flat) -> None:
        t_host = time.perf_counter()
        try:
            self._launch_inner(grads, flat)
        finally:
            self.stats["launch_host_ms"] = self.stats.get("launch_host_ms", 0.0) + 1e3 * (time.perf_counter() - t_host)

    def _launch_inner(self, grads: List[torch.Tensor], flat) -> None:
        dev = grads[0].device
        side = self._comm_stream(dev)
        if side is not None:
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(dev))      # the gradient's producer kernels
            side.wait_event(ready)
            from . import ops
            wg = ops.wgrad_stream(dev)                        # ... and the weight gradients computed on ops' side stream
            if wg is not None:
                side.wait_stream(wg)
            ctx = torch.cuda.stream(side)
        else:
            ctx = _NullCtx()
        with ctx:
            if self.measure and side is not None:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record(side)
            narrow = self.comm_dtype != grads[0].dtype
            if flat:
                buf = torch.cat([g.reshape(-1) for g in grads])
                for g in grads:
                    if side is not None:
                        g.record_stream(side)
                if narrow:
                    buf = buf.to(self.comm_dtype)
            else:
                buf = grads[0]
                if side is not None:
                    buf.record_stream(side)
                if narrow:
                    buf, flat = buf.reshape(-1).to(self.comm_dtype), True       # (copied back into the fp32 gradient in reduce())
            work = dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.pg, async_op=True)
            if self.measure and side is not None:
                work.wait()                       # stream-ordered on the side stream (no host block for NCCL work)
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record(side)
                self._spans.append((e0, e1))
        self.stats["collectives"] += 1
        self.stats["bytes"] += buf.numel() * buf.element_size()
        self._inflight.append((work, buf if flat else None, grads))

    # ---- after backward ----------------------------------------------------------------------------------
    def reduce(self, *nets: torch.nn.Module) -> None:
        """Finish the step's gradient exchange for the networks one backward pass produced gradients for: after this returns
        (stream-ordered), every ``p.grad`` holds the SUM over ranks.  Use ``FusedAdam.grad_scale = 1/world`` (set by ``attach_ddp``)
        for the average."""
        if not self.active:
            return
        t_host = time.perf_counter()
        if self.measure and torch.cuda.is_available():
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(torch.cuda.current_stream())
            self._bwd_done.append(ev)
        for net in nets:
            if id(net) not in self._attached or not self.overlap:
                for p in net.parameters():                  # no-overlap path: same bucketing, issued now
                    if p.grad is not None:
                        self._on_grad_ready(p)
        self._flush_bucket()
        for work, flat, grads in self._inflight:
            dev = grads[0].device
            side = self._comm_stream(dev)
            ctx = torch.cuda.stream(side) if side is not None else _NullCtx()
            with ctx:
                work.wait()
                if flat is not None:                    # bucket (or narrowed message) -> the fp32 gradients, ONE multi-tensor launch
                    views, off = [], 0
                    for g in grads:
                        n = g.numel()
                        views.append(flat[off:off + n].view_as(g))
                        off += n
                    torch._foreach_copy_(grads, views)
        for dev, side in self._side.items():
            torch.cuda.current_stream(dev).wait_stream(side)    # optimizer kernels run after the reduced grads land
        self._inflight = []
        self.stats["reduce_host_ms"] = self.stats.get("reduce_host_ms", 0.0) + 1e3 * (time.perf_counter() - t_host)
        if self.measure:
            self._span_marks.append(len(self._spans))

    def overlap_report(self):
        """(measure=True; call after a device synchronise)  Per optimizer step: time the collectives occupied the side
        stream, and the part of it that ran AFTER backward's last kernel (exposed: the optimizer waits for it)."""
        if not self._bwd_done:
            return None
        comm = exposed = 0.0
        lo = 0
        for ev, hi in zip(self._bwd_done, self._span_marks):
            for e0, e1 in self._spans[lo:hi]:
                comm += e0.elapsed_time(e1)
            if hi > lo:
                exposed += max(0.0, ev.elapsed_time(self._spans[hi - 1][1]))
            lo = hi
        n = len(self._bwd_done)
        self._spans, self._bwd_done, self._span_marks = [], [], []
        return {"backward_passes": n, "comm_ms_per_pass": comm / n, "exposed_ms_per_pass": exposed / n,
                "overlap_frac": (1.0 - exposed / comm) if comm > 0 else None}

    def broadcast_parameters(self, net: torch.nn.Module, src: int = 0) -> None:
        """Rank ``src``'s parameters and buffers to every rank, one flat message per dtype (torch DDP does this when it
        wraps a module).  Parameters are written through ``.data`` and stamped so that packed weight copies refresh.  Like every
        other collective of the reducer it runs on a one-rank group too when ``force_collectives`` asks for it (tests)."""
        if not self.active:
            return
        with torch.no_grad():
            tensors = [p.data for p in net.parameters()] + [b for b in net.buffers()]
            for dt in sorted({t.dtype for t in tensors}, key=str):
                group = [t for t in tensors if t.dtype == dt]
                flat = torch.cat([t.reshape(-1) for t in group])
                dist.broadcast(flat, src=src, group=self.pg)
                off = 0
                for t in group:
                    n = t.numel()
                    t.copy_(flat[off:off + n].view_as(t))
                    off += n
            from . import ops
            ops.mark_written(*net.parameters(), *net.buffers())

    def sync_bn_exchange(self, msg: torch.Tensor) -> None:
        """SUM ``msg`` (one BatchNorm layer's fp64 statistics message, ops.bn_sync) over the ranks in place, ordered on the current
        stream like any kernel: RCCL joins the current stream on both sides, gloo returns when the sum is there."""
        if not self.active:
            return
        dist.all_reduce(msg, op=dist.ReduceOp.SUM, group=self.stats_pg)
        self.stats["sync_bn_collectives"] += 1
        self.stats["sync_bn_bytes"] += msg.numel() * msg.element_size()

    def ada_exchange(self, pair: torch.Tensor, rows: int) -> int:
        """SUM ``pair`` (ops.AdaState's measured int64 (sum of signs, logit count): 16 bytes) over the ranks in place, between the
        controller's two launches and in the current stream's order; -> the number of real images over all ranks (every rank holds
        ``rows``).  Integers: N ranks on their rows then hold the accumulators and the p of one process on the whole batch."""
        if not self.active:
            return rows
        dist.all_reduce(pair, op=dist.ReduceOp.SUM, group=self.pg)
        self.stats["ada_collectives"] = self.stats.get("ada_collectives", 0) + 1
        return rows * self.world

    def bn_scope(self):
        """The scope a trainer runs its model calls in: ``ops.bn_sync`` of this reducer with ``sync_bn`` on an active group, else nothing."""
        if self.sync_bn and self.active:
            from . import ops
            return ops.bn_sync(self)
        return _NullCtx()

    def broadcast_buffers(self, net: torch.nn.Module, src: int = 0) -> None:
        bufs = [b for b in net.buffers() if b.is_floating_point()]
        if not self.active or not bufs or self.sync_bn:       # (sync_bn: every rank computed them from the same summed statistics)
            return
        flat = torch.cat([b.reshape(-1) for b in bufs])
        dist.broadcast(flat, src=src, group=self.pg)
        views, off = [], 0
        for b in bufs:
            n = b.numel()
            views.append(flat[off:off + n].view_as(b))
            off += n
        with torch.no_grad():
            torch._foreach_copy_(bufs, views)              # one multi-tensor launch (18 buffers in the generator)


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _broadcast_rng_state(process_group, device) -> None:
    """rank 0's global CPU RNG state on every rank"""
    state = torch.get_rng_state()
    if dist.get_backend(process_group) == "nccl":          # RCCL moves device tensors only
        state = state.to(device)
    dist.broadcast(state, src=0, group=process_group)
    torch.set_rng_state(state.cpu())


def attach_ddp(trainer, process_group=None, sync_bn: bool = False, **kw) -> GradReducer:
    """Make a DefectGanTrainer, an MAETrainer or a stargan ``Solver`` data-parallel: gradients are summed across ranks after each
    backward and averaged inside the fused Adam kernel.  The two trainers: generator BatchNorm statistics stay per rank and the
    buffers follow rank 0 -- or, with ``sync_bn=True``, are taken over the global batch, which makes N ranks on their rows equal ONE
    process on the whole batch (module docstring: mechanism, and which options the equality covers -- ``add_noise``, ``diff_aug`` and
    SEAN's host-drawn embeddings are per-rank random numbers and equal no single-process run).  Solver: see ``_attach_solver`` (it has no batch statistics:
    ``sync_bn`` is a ValueError)."""
    from .stargan import Solver
    if isinstance(trainer, Solver):
        if sync_bn:
            raise ValueError("attach_ddp(solver, sync_bn=True): the stargan-v2 networks have no batch statistics to synchronise")
        return _attach_solver(trainer, process_group, **kw)
    if sync_bn:        # the statistics messages on a communicator of their own (every rank of the group calls attach_ddp: collective)
        ranks = dist.get_process_group_ranks(process_group) if process_group is not None else None
        kw["stats_group"] = dist.new_group(ranks=ranks)
    red = GradReducer(process_group, sync_bn=sync_bn, **kw)
    release = getattr(trainer, "release_graphs", None)          # (graph_step: the captured step has no collectives)
    if release is not None:
        release()
    for name, net in trainer.model.networks.items():
        red.attach(net)
        red.broadcast_parameters(net)
        trainer.optimizers[name].grad_scale = 1.0 / red.world
    mask_token = getattr(trainer.model, "mask_token", None)         # MAE stage: trained by the generator's optimizer
    if isinstance(mask_token, torch.nn.Module):
        red.attach(mask_token)
        red.broadcast_parameters(mask_token)
    if sync_bn and red.world > 1:                                   # the MAE stage's mask draws: the same global draw on every rank
        _broadcast_rng_state(process_group, torch.device(trainer.opt.device))
    if getattr(trainer.model, "diffaug_p", None) is not None:       # opt.diff_aug_p / opt.ada_target: the global batch's gates on every
        trainer.model.ada_ranks = red                               # rank (one diff_aug_seed), the measured pair summed over the ranks
    if getattr(trainer.model, "embed_bank", None) is not None:      # opt.embed_rng = "device": SEAN's embeddings drawn for the global
        trainer.model.embed_ranks = red                             # batch's rows (one embed_seed on every rank)
    trainer.reducer = red
    return red


def _attach_solver(solver, process_group=None, **kw) -> GradReducer:
    """stargan-v2: the reducer on the four trained networks; rank 0's parameters of ``nets`` and ``nets_ema`` and rank 0's global CPU
    RNG state (DiffAugment's draws, and whatever the caller draws from it next) on every rank; 1/world in the four Adams.  Attach
    before the first iteration (the Adam moments are not exchanged).  ``Solver.train_iteration`` then reduces exactly the gradients each
    ``step()`` consumes, the discarded ones (D during the G updates, S during the reference-guided one) are not computed."""
    red = GradReducer(process_group, **kw)
    for name, net in vars(solver.nets).items():
        red.attach(net)
        red.broadcast_parameters(net)
        getattr(solver.optims, name).grad_scale = 1.0 / red.world
    for net in vars(solver.nets_ema).values():
        red.broadcast_parameters(net)
    if red.world > 1:
        _broadcast_rng_state(process_group, solver.device)
    solver.reducer = red
    return red
