"""Fused multi-tensor Adam on the HIP kernel (csrc/adam.hip): one launch per optimizer step.

A ``torch.optim.Optimizer`` subclass, so ``lr_scheduler``s, ``param_groups`` / ``add_param_group`` and
``torch.amp.GradScaler`` keep working the way the reference's trainers use them (trainers/base_trainer.py:68-126,
mae_trainer.py:28,139-158).  Semantics = torch.optim.Adam (no amsgrad), or torch.optim.AdamW with ``weight_decay > 0``
(decoupled: p *= 1 - lr*wd before the update): parameters whose ``grad`` is None are skipped and get no state.
``ema_lerp_`` is stargan-v2's parameter EMA on the same pointer table (csrc/adam.hip); ``EmaGroup`` is the defectGAN / MAE
trainers' (``opt.ema_beta``): the same launch per G update, buffers included, and a device-read form for captured graphs.

``FusedAdam.step`` is one path, eager or under graph capture (``torch.cuda.is_current_stream_capturing()``): it gathers the launch
groups, takes each group's device pointer table from the cache (capturing: from a slot ``graph_reserve`` made) and hands it to
``_launch``, which picks the entry point.  Captured launches are the ``_dev`` kernels: they read (lr, 1 - b1^t, sqrt(1 - b2^t),
1 - lr*wd) from a device table of the next ``HYPER_ROWS`` steps (``adam_hyper_rows``, the same host arithmetic as the eager
launch), indexed by a device counter that a one-thread kernel advances after each update, so a replayed step sees its own step's
values without a host wait.  ``graph_take_plan`` hands the recorded launches (``_CapturedLaunch``; ``EmaGroup`` keeps the same
records through the same ``_GraphCapture``) to the owner of the graph, which calls ``graph_prepare`` before and ``graph_finish``
after every replay: the host work the graph cannot do (uploading the pointer tables once, rewriting the rows when the lr changed
or they run out, ``state["step"]`` and the ``_dei2i_epoch`` stamps).

``max_grad_norm`` (``torch.nn.utils.clip_grad_norm_`` over every parameter of the optimizer, L2): the step first sums g^2 over
each launch group's pointer table (``dei2i_grad_sumsq``, fixed-order partials, no atomics), one more launch turns the partials into
``grad_scale * min(1, max_grad_norm / (norm + 1e-6))`` in device memory, and the Adam launches read their gradient scale from
there (the ``_clip`` entry points): no host wait, no gradient written, the same launches eagerly and in a captured graph."""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from . import ops


def _dev_ptr(tensor, offset=0):
    return ctypes.c_void_p(tensor.data_ptr() + offset)


class _PointerTable:
    """The pointer table of one multi-tensor launch of csrc/adam.hip on the host: one row ``(p, g, aux0, aux1, numel)`` (a
    ``dei2i_adam_rec``) per entry ``(p, g, aux0, aux1)`` of fp32 tensors, ``aux`` tensors or None.  ``p`` must be contiguous; a
    ``g`` that is not is copied, and the copy lives as long as this object: keep it until the launch is queued."""

    def __init__(self, who, entries):
        self.rows, self.hold, self.max_n = [], [], 0
        self.device = entries[0][0].device
        for p, g, aux0, aux1 in entries:
            ops._require_gpu(p, who)
            if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous():
                raise TypeError(f"{who} expects contiguous fp32 tensors to update, from fp32 gradients or sources")
            g = g if g.is_contiguous() else g.contiguous()
            self.hold.append(g)
            self.rows.append((p.data_ptr(), g.data_ptr(), 0 if aux0 is None else aux0.data_ptr(),
                              0 if aux1 is None else aux1.data_ptr(), p.numel()))
            self.max_n = max(self.max_n, p.numel())

    def upload(self, into=None):
        """-> the rows on the device, through pinned memory and stream-ordered: in the first rows of ``into``, or a new tensor"""
        host = torch.empty((len(self.rows), L.ADAM_REC_WORDS), dtype=torch.int64, pin_memory=True)
        host.copy_(torch.tensor(self.rows, dtype=torch.int64))
        if into is None:
            return host.to(self.device, non_blocking=True)
        into[:len(self.rows)].copy_(host, non_blocking=True)
        return into

    def cached(self, cache):
        """-> the rows on the device, uploaded only when a pointer moved since the launch that left them in ``cache`` (in steady
        state the caching allocator hands every gradient the address it had the step before)"""
        key = (self.device, len(self.rows), self.rows[0][0])
        hit = cache.get(key)
        if hit is None or hit[0] != self.rows:
            hit = cache[key] = (self.rows, self.upload())
        return hit[1]

    def args(self, table_dev):
        """the (table_dev, count, max_n) every entry point of csrc/adam.hip begins with"""
        return _dev_ptr(table_dev), len(self.rows), self.max_n


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers' ``step`` methods share: the closure and the cache of uploaded pointer tables."""

    @staticmethod
    def _closure_loss(closure):
        if closure is None:
            return None
        with torch.enable_grad():
            return closure()

    def _tables(self):
        return self.__dict__.setdefault("_table_cache", {})


class _CapturedLaunch:
    """One multi-tensor launch recorded into a graph.  ``table``: its pointer table on the host (holding the graph's own gradients
    or sources, at fixed addresses from replay to replay), which ``upload`` copies into the reserved ``table_dev`` once, after the
    capture and before the first replay.  ``rows``: the device rows (a ``_RowTable``) the launch reads at a device index, or None.
    ``info``, FusedAdam's: ``group`` (index), ``params``, ``wd`` (decoupled), ``frozen``: the (max_grad_norm or None, grad_scale)
    recorded as launch arguments, ``clip``: the clipping buffers the graph reads and writes by address, kept alive with it."""

    def __init__(self, table, table_dev, rows=None, **info):
        self.table, self.table_dev, self.rows, self.uploaded = table, table_dev, rows, False
        self.__dict__.update(info)

    def upload(self):
        if not self.uploaded:
            self.table.upload(into=self.table_dev)      # (a reserved slot: rows for the whole group)
            self.uploaded = True


class _GraphCapture:
    """The bookkeeping of the capture protocol, for FusedAdam and EmaGroup.  ``graph_reserve`` leaves ``{key: [slots]}``: device
    buffers made before the capture (one allocated inside it comes from the graph's pool, whose blocks earlier nodes of the same
    replay may use as scratch -- they would overwrite what ``graph_prepare`` uploaded).  The recording takes them one by one and
    notes each launch; ``graph_take_plan`` hands the notes to the owner of the graph."""

    def _take_reserved(self, key, error):
        slots = self.__dict__.get("_graph_reserve", {}).get(key)
        if not slots:
            raise RuntimeError(error)
        return slots.pop(0)

    def _recorded(self, launch):
        self.__dict__.setdefault("_graph_plan", []).append(launch)

    def graph_take_plan(self):
        """-> the launches recorded since the last call (the graph just captured owns them); unused reserved tables are dropped"""
        self.__dict__.pop("_graph_reserve", None)
        return self.__dict__.pop("_graph_plan", [])


class FusedAdam(_FusedOptimizer, _GraphCapture):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, weight_decay=0.0, decoupled=True,
                 max_grad_norm=None):
        """``decoupled=False``: torch.optim.Adam's weight decay (L2: the gradient becomes g + wd * p before the moments -- what
        stargan-v2's optimizers use, core/solver.py:52-56) instead of AdamW's.  ``max_grad_norm`` (None or 0: off; a plain attribute,
        read at every step): the gradients ``g * grad_scale`` of all the optimizer's parameters are clipped to this joint L2 norm
        inside the update; ``grad_norm`` is their norm before clipping, on the device."""
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = float(grad_scale)
        self.decoupled = bool(decoupled)
        self.max_grad_norm = max_grad_norm
        self._clip_norm()

    def _clip_norm(self):
        """-> ``max_grad_norm`` as a float > 0, or None: no clipping"""
        c = self.max_grad_norm
        if c is None or c == 0:
            return None
        if not float(c) > 0.0:
            raise ValueError(f"|max_grad_norm {c}| is invalid (> 0; None or 0 turns clipping off)")
        return float(c)

    @property
    def grad_norm(self):
        """One-element device view: the L2 norm of ``g * grad_scale`` over every parameter the last clipped step updated, before
        clipping (None until such a step has run).  Reading it does not wait for the device."""
        out = self.__dict__.get("_clip_out")
        return None if out is None else out[:1]

    def _launch_groups(self, reach):
        """One launch per param group and step count: yields (group index, group, t, the group's parameters with a gradient that
        reach step ``t = reach(p, state)`` now, weight decay, whether it is the coupled kind)."""
        for gi, group in enumerate(self.param_groups):
            by_step = {}
            for p in group["params"]:
                if p.grad is not None:
                    by_step.setdefault(reach(p, self.state[p]), []).append(p)
            wd = float(group.get("weight_decay", 0.0))
            for t, plist in by_step.items():
                yield gi, group, t, plist, wd, wd > 0.0 and not self.decoupled

    def _table(self, plist):
        return _PointerTable("FusedAdam", [(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in plist])

    @staticmethod
    def _reach(p, st):
        if len(st) == 0:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        st["step"] += 1
        return st["step"]

    @staticmethod
    def _reach_captured(p, st):            # (host state is left to graph_finish: the capture runs nothing)
        if len(st) == 0:                   # zeros_like inside the capture would reset the moments on every replay
            raise RuntimeError("FusedAdam: a parameter received its first gradient while a graph was being captured "
                               "(capture after the set of parameters with a gradient has settled: raise graph_warmup)")
        return st["step"] + 1

    @torch.no_grad()
    def step(self, closure=None):
        """One pointer table per launch group serves the norm (``max_grad_norm``) and the update, so a gradient that had to be copied
        is copied once.  Eager, it comes from the cache.  Recorded into a graph, it is a slot ``graph_reserve`` made, which
        ``graph_prepare`` fills after the capture: the gradients it points to are the graph's own, at fixed addresses."""
        loss = self._closure_loss(closure)
        capturing = torch.cuda.is_current_stream_capturing()
        max_norm = self._clip_norm()
        launches = []
        for gi, group, t, plist, wd, coupled in self._launch_groups(self._reach_captured if capturing else self._reach):
            table = self._table(plist)
            if capturing:
                table_dev, hyper = self._take_reserved(gi, "FusedAdam: no table reserved for this group (call graph_reserve() "
                                                           "before the capture)")
                hyper.t0, hyper.t, hyper.key = t, t, None
            else:
                table_dev, hyper = table.cached(self._tables()), None
            launches.append((gi, group, t, plist, wd, coupled, table, table_dev, hyper))
        scale = None
        if launches and max_norm is not None:      # (buffers reserved before a capture, like the tables: never allocated inside it)
            scale = self._clip_scale(ops._lib_for(launches[0][3][0]), [(table, table_dev) for *_, table, table_dev, _ in launches],
                                     max_norm, reserve=not capturing)
        for launch in launches:
            self._launch(scale, max_norm, *launch)
        return loss

    def _launch(self, scale, max_norm, gi, group, t, plist, wd, coupled, table, table_dev, hyper):
        """One group's update.  ``hyper`` None: the step's values go by value; else (under capture) the kernel reads them from
        ``hyper``'s rows, one more launch advances their index, and the launch is noted for ``graph_prepare``, which checks the
        arguments frozen into the graph.  ``scale``: where ``_clip_scale`` left the gradient scale, or None: ``grad_scale``.
        Coupled L2 decay (g*grad_scale + wd*p) happens inside the kernel: p.grad is left as the caller's."""
        lib, dev = ops._lib_for(plist[0]), hyper is not None
        b1, b2 = group["betas"]
        if scale is not None:
            step, rest = lib.dei2i_adam_step_clip_dev if dev else lib.dei2i_adam_step_clip, (scale, int(coupled), wd)
        elif coupled:
            step, rest = lib.dei2i_adam_step_l2_dev if dev else lib.dei2i_adam_step_l2, (self.grad_scale, wd)
        else:
            step, rest = (lib.dei2i_adam_step_dev, (self.grad_scale,)) if dev else (lib.dei2i_adam_step, (self.grad_scale, wd))
        values = ((_dev_ptr(hyper.table), _dev_ptr(hyper.index), hyper.rows, b1, b2, group["eps"]) if dev else
                  (float(group["lr"]), b1, b2, group["eps"], 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)))
        L.check(step(*table.args(table_dev), *values, *rest, ops._stream()),
                "adam_step" + ("_clip" if scale is not None else "") + ("_dev" if dev else ""))
        if dev:
            L.check(lib.dei2i_index_advance(_dev_ptr(hyper.index), ops._stream()), "index_advance")
            self._recorded(_CapturedLaunch(table, table_dev, hyper, group=gi, params=plist, wd=0.0 if coupled else wd,
                                           frozen=(max_norm, self.grad_scale),
                                           clip=self.__dict__.get("_clip_bufs") if scale is not None else None))
        ops.mark_written(*plist)           # (under capture too: later passes of the capture must repack)

    # ---- global-norm clipping -----------------------------------------------------------------------------------------
    def _clip_buffers(self, reserve):
        """-> (partials, out): room for the partial sums of any split of the parameters into launch groups (a group's grid is no
        wider than its longest parameter's, its rows no more than its parameters), and (norm, scale).  Both persist; ``reserve``
        False (inside a capture, whose pool must not hold them): raise instead of allocating."""
        key = tuple(len(group["params"]) for group in self.param_groups)
        bufs = self.__dict__.get("_clip_bufs")
        if bufs is None or bufs[0] != key:
            if not reserve:
                raise RuntimeError("FusedAdam: no clipping buffers reserved (call graph_reserve() before the capture)")
            lib = L.load()
            groups = [group["params"] for group in self.param_groups if group["params"]]
            need = sum(lib.dei2i_grad_sumsq_blocks(max(p.numel() for p in params)) * len(params) for params in groups)
            device = groups[0][0].device
            if self.__dict__.get("_clip_out") is None or self._clip_out.device != device:
                self._clip_out = torch.zeros(2, dtype=torch.float32, device=device)
            bufs = self._clip_bufs = (key, torch.empty(max(need, 1), dtype=torch.float32, device=device), self._clip_out)
        return bufs[1], bufs[2]

    def _clip_scale(self, lib, tables, max_norm, reserve):
        """One dei2i_grad_sumsq per (host table, device table), their partials appended, and one dei2i_grad_clip_finalize over all of
        them: -> the device address of ``grad_scale * min(1, max_norm / (norm + 1e-6))``, which the ``_clip`` updates read"""
        partial, out = self._clip_buffers(reserve)
        used = 0
        for table, table_dev in tables:
            if table.device != partial.device:
                raise ValueError("FusedAdam: max_grad_norm needs every parameter of the optimizer on one device")
            cells = lib.dei2i_grad_sumsq_blocks(table.max_n) * len(table.rows)
            if used + cells > partial.numel():
                raise RuntimeError("FusedAdam: the clipping buffers are too small for this step's launch groups")
            L.check(lib.dei2i_grad_sumsq(*table.args(table_dev), _dev_ptr(partial, 4 * used), ops._stream()), "grad_sumsq")
            used += cells
        L.check(lib.dei2i_grad_clip_finalize(_dev_ptr(partial), used, self.grad_scale, max_norm, _dev_ptr(out), ops._stream()),
                "grad_clip_finalize")
        return _dev_ptr(out, 4)

    # ---- graph capture ------------------------------------------------------------------------------------------------
    def graph_reserve(self):
        """Before a capture: device tables for every launch group the captured step can make (one per distinct step count
        among the parameters, plus one), and with ``max_grad_norm`` the clipping buffers, outside the graph's memory pool."""
        if self._clip_norm() is not None and any(group["params"] for group in self.param_groups):
            self._clip_buffers(reserve=True)
        reserve = {}
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            steps = {self.state[p]["step"] for p in params if self.state.get(p)}
            reserve[gi] = [(torch.empty((len(params), L.ADAM_REC_WORDS), dtype=torch.int64, device=params[0].device),
                            _HyperTable(params[0].device, 0)) for _ in range(len(steps) + 1)]
        self._graph_reserve = reserve

    def graph_prepare(self, plan):
        """Before a replay of a graph holding ``plan``: the rows of every group cover this step with the current lr
        (a stream-ordered upload only when they do not)."""
        for g in plan:
            if g.frozen != (self._clip_norm(), self.grad_scale):
                raise RuntimeError(f"FusedAdam: (max_grad_norm, grad_scale) = {(self._clip_norm(), self.grad_scale)} now, but the graph "
                                   f"was captured with {g.frozen}, which are arguments frozen into it (call the trainer's "
                                   "release_graphs(), or capture again)")
            g.upload()
            group = self.param_groups[g.group]
            b1, b2 = group["betas"]
            # (the step from the state, not the mirror: an eager call between two replays has advanced it)
            g.rows.ensure(self.state[g.params[0]]["step"] + 1, float(group["lr"]), b1, b2, g.wd)

    def graph_finish(self, plan):
        """After a replay: the host state the eager step would have left (``p.grad`` is the trainer's)."""
        for g in plan:
            g.rows.advance()
            for p in g.params:
                self.state[p]["step"] += 1
            ops.mark_written(*g.params)


HYPER_ROWS = 4096


def adam_hyper_rows(lr, b1, b2, decoupled_decay, t0, count):
    """(count, 4) float32 rows (lr, 1 - b1^t, sqrt(1 - b2^t), 1 - lr*decoupled_decay) for t = t0 .. t0 + count - 1: the floats
    the eager ``FusedAdam._launch`` hands the kernel (python doubles rounded to float, the last one float arithmetic)."""
    out = np.empty((count, 4), dtype=np.float32)
    lr32 = np.float32(lr)
    out[:, 0] = lr32
    out[:, 3] = np.float32(1.0) - lr32 * np.float32(decoupled_decay)
    for i in range(count):
        t = t0 + i
        out[i, 1] = 1.0 - b1 ** t
        out[i, 2] = math.sqrt(1.0 - b2 ** t)
    return out


class _RowTable:
    """``rows`` rows of ``width`` floats + the int32 row index the ``_dev`` kernels read, in one device buffer (one upload).
    ``t0``: the step of row 0; ``t``: the step the next replay runs (host mirror of t0 + index); ``key``: what the rows were
    computed from.  A subclass's ``_rows(t, key)`` gives the (rows, width) float32 rows from step ``t`` on.  ``STRIDE``: the
    distance between the steps of two rows, 1 or (an index into the key) ``key[STRIDE]``."""
    WIDTH = 1
    STRIDE = None

    def _stride(self, key):
        return 1 if self.STRIDE is None else key[self.STRIDE]

    def __init__(self, device, t, rows):
        self.rows = rows
        self.buf = torch.empty(rows * self.WIDTH + 1, dtype=torch.float32, device=device)      # (written by the first refresh)
        self.table = self.buf[:rows * self.WIDTH]
        self.index = self.buf[rows * self.WIDTH:].view(torch.int32)
        self.t0, self.t = t, t
        self.key = None            # no rows yet: the first ensure() uploads
        self._host = None

    def refresh(self, t, *key):
        """Rows from step ``t`` on and index 0, one stream-ordered upload on the current stream (outside any capture)."""
        cells = self.rows * self.WIDTH
        host = torch.empty(cells + 1, dtype=torch.float32, pin_memory=True)
        host[:cells].copy_(torch.from_numpy(np.ascontiguousarray(self._rows(t, key), dtype=np.float32).reshape(-1)))
        host[cells:].view(torch.int32).fill_(0)
        self.buf.copy_(host, non_blocking=True)
        self._host = host          # (the caching host allocator keeps the block until the copy has run; this is belt and braces)
        self.t0 = self.t = t
        self.key = key

    def ensure(self, t, *key):
        """The device index is at step ``t``'s row, computed from ``key`` (else: rewrite from ``t`` on)."""
        if self.key != key or t != self.t or (t - self.t0) // self._stride(key) >= self.rows - 1:
            self.refresh(t, *key)

    def advance(self):
        self.t += self._stride(self.key)


class _HyperTable(_RowTable):
    """Device rows of ``adam_hyper_rows``; the key is (lr, b1, b2, decoupled decay)."""
    WIDTH = 4

    def __init__(self, device, t, rows=HYPER_ROWS):
        super().__init__(device, t, rows)

    def _rows(self, t, key):
        lr, b1, b2, wd = key
        return adam_hyper_rows(lr, b1, b2, wd, t, self.rows)


def ema_lerp_(ema_params, params, weight):
    """``e.copy_(torch.lerp(p, e, weight))`` for every pair, in place, one launch (stargan-v2 moving_average, core/solver.py:549-551).
    Every updated tensor is stamped (``ops.mark_written``): the packed-weight caches of the EMA network are keyed on it."""
    ema_params, params = list(ema_params), list(params)
    if len(ema_params) != len(params):
        raise ValueError("ema_lerp_: parameter lists differ in length")
    if not params:
        return
    for e, p in zip(ema_params, params):
        if e.shape != p.shape or not p.is_contiguous():
            raise TypeError("ema_lerp_ expects pairs of contiguous fp32 tensors of one shape")
        if e.device != p.device:
            raise ValueError("ema_lerp_: the EMA copy and the parameter are on different devices")
    table = _PointerTable("ema_lerp_", [(e, p, None, None) for e, p in zip(ema_params, params)])
    lib = ops._lib_for(ema_params[0])
    L.check(lib.dei2i_ema_lerp(*table.args(table.cached(_ema_tables)), float(weight), ops._stream()), "ema_lerp")
    ops.mark_written(*ema_params)


_ema_tables = {}

EMA_ROWS = 4096


def ema_options(opt):
    """-> (ema_beta, ema_start_iter, ema_inference) of an option object, absent options at their defaults (0.0: no EMA, 0, True)"""
    beta = float(getattr(opt, "ema_beta", 0.0) or 0.0)
    if not 0.0 <= beta < 1.0:
        raise ValueError(f"|ema_beta {beta}| is invalid (0 <= ema_beta < 1; 0 turns the EMA off)")
    return beta, int(getattr(opt, "ema_start_iter", 0) or 0), bool(getattr(opt, "ema_inference", True))


def clip_options(opt):
    """-> ``opt.max_grad_norm`` as a float > 0, or None (absent, None or 0: no clipping).  Only the Adam family clips."""
    c = getattr(opt, "max_grad_norm", None)
    if c is None or c == 0:
        return None
    if not float(c) > 0.0:
        raise ValueError(f"|max_grad_norm {c}| is invalid (> 0; None or 0 turns clipping off)")
    if getattr(opt, "optimizer", None) in ("sgd", "rmsprop"):
        raise NotImplementedError(f"max_grad_norm with optimizer={opt.optimizer!r} (only FusedAdam clips by global norm)")
    return float(c)


def validation_options(opt, metric_names=()):
    """-> {"val_freq": epochs between two validation passes of ``train()`` (absent, None or 0: 0 = never), "val_max_batches" (None:
    the whole loader), "val_seed" (default 0: the seed of validation's own draws), "save_best": the metric of ``metric_names`` whose
    best value keeps a "best" checkpoint, or None}.  ``metric_names``: what the asking trainer's ``validate()`` returns."""
    freq = getattr(opt, "val_freq", None)
    freq = 0 if freq is None else freq
    if isinstance(freq, bool) or int(freq) != freq or freq < 0:
        raise ValueError(f"|val_freq {freq}| is invalid (a whole number of epochs >= 0; None or 0 turns validation off)")
    batches = getattr(opt, "val_max_batches", None)
    if batches is not None and (isinstance(batches, bool) or int(batches) != batches or batches <= 0):
        raise ValueError(f"|val_max_batches {batches}| is invalid (a whole number of batches > 0; None: the whole loader)")
    seed = getattr(opt, "val_seed", None)
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 2 ** 63:
        raise ValueError(f"|val_seed {seed}| is invalid (a whole number in [0, 2^63))")
    best = getattr(opt, "save_best", None) or None
    if best is not None and best not in metric_names:
        raise ValueError(f"|save_best {best}| is invalid (the metrics of this stage: {' | '.join(metric_names)})")
    return {"val_freq": int(freq), "val_max_batches": None if batches is None else int(batches), "val_seed": int(seed),
            "save_best": best}


LOWER_IS_BETTER = ("l1",)          # (every other validation metric: higher is better)


def ada_options(opt, diffaug_stage=True):
    """-> None (``opt.diff_aug_p`` absent or None and ``opt.ada_target`` absent, None or 0: DiffAugment as it was), or the dict
    {"p": the initial (or, without a target, the fixed) probability, "target": r_t's target or None (no controller), "interval"
    (D updates per adjustment, default 4), "kimg" (thousands of real images for p to cross 0..1, default 500), "p_max" (default 1)}.
    ``diffaug_stage``: whether the asking trainer's stage applies DiffAugment at all (the MAE stage does not)."""
    p, target = getattr(opt, "diff_aug_p", None), getattr(opt, "ada_target", None)
    target = None if target is None or target == 0 else target
    if p is None and target is None:
        return None
    on = "diff_aug_p" if p is not None else "ada_target"
    if not diffaug_stage:
        raise ValueError(f"|{on}| gates DiffAugment, which the MAE stage does not apply (the defectGAN stage only)")
    if p is not None and not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"|diff_aug_p {p}| is invalid (0 <= diff_aug_p <= 1; None turns the gate off)")
    if target is not None and not 0.0 < float(target) < 1.0:
        raise ValueError(f"|ada_target {target}| is invalid (0 < ada_target < 1; None or 0 turns the controller off)")
    if not getattr(opt, "diff_aug", ""):
        raise ValueError(f"|{on}| needs a non-empty diff_aug (the policies it gates)")
    if getattr(opt, "diff_aug_rng", None) != "device":
        raise ValueError(f"|{on}| needs diff_aug_rng='device' (the gates are drawn on the GPU, next to the parameters)")
    interval, kimg, p_max = getattr(opt, "ada_interval", None), getattr(opt, "ada_kimg", None), getattr(opt, "ada_p_max", None)
    interval, kimg, p_max = 4 if interval is None else interval, 500.0 if kimg is None else kimg, 1.0 if p_max is None else p_max
    if target is not None:
        if int(interval) != interval or interval <= 0:
            raise ValueError(f"|ada_interval {interval}| is invalid (a whole number of D updates > 0)")
        if not float(kimg) > 0.0:
            raise ValueError(f"|ada_kimg {kimg}| is invalid (> 0)")
        if not 0.0 <= float(p_max) <= 1.0:
            raise ValueError(f"|ada_p_max {p_max}| is invalid (0 <= ada_p_max <= 1)")
    return {"p": 0.0 if p is None else float(p), "target": None if target is None else float(target), "interval": int(interval),
            "kimg": float(kimg), "p_max": float(p_max)}


def ema_weight(iters, start_iter, beta):
    """The lerp weight of the G update that ends with ``trainer.iters == iters``: 0 (the copy follows the live weights) up to
    ``start_iter``, ``beta`` after it."""
    return 0.0 if iters <= start_iter else beta


def ema_weight_rows(iters, num_critics, start_iter, beta, count):
    """(count,) float32: row j is ``ema_weight`` of the j-th G update after iteration ``iters`` (G updates end at the multiples of
    ``num_critics``), the float the eager launch hands the kernel."""
    ends = (iters // num_critics + 1 + np.arange(count, dtype=np.int64)) * num_critics
    return np.where(ends <= start_iter, np.float32(0.0), np.float32(beta)).astype(np.float32)


class _WeightRows(_RowTable):
    """Device rows of ``ema_weight_rows``: a "step" is the iteration a G update ends at; the key is (num_critics, start_iter, beta),
    whose first entry is also the distance between two steps."""
    STRIDE = 0

    def __init__(self, device, rows=EMA_ROWS):
        super().__init__(device, 0, rows)

    def _rows(self, t, key):
        num_critics, start_iter, beta = key
        return ema_weight_rows(t - num_critics, num_critics, start_iter, beta, self.rows)


class EmaGroup(_GraphCapture):
    """The EMA copies of a set of trained tensors and the buffers that go with them, updated once per G update by the defectGAN and
    MAE trainers.  ``lerp``: pairs (e, p) of fp32 tensors, ``e = lerp(p, e, weight)`` in one launch of csrc/adam.hip's EMA kernel;
    ``copy``: pairs (e, b) of buffers, ``e = b``: the contiguous fp32 ones in one more launch of that kernel with weight 0, which is
    an exact copy, the others (``num_batches_tracked``) through ``copy_``.

    Eager, ``update(weight)`` passes the weight by value.  Under graph capture it records the ``_dev`` kernel, which reads its
    weight from device rows (``ema_weight_rows``) at a device index that one ``dei2i_index_advance`` moves after the launch, so that
    a replay uses its own update's weight: the switch from copying to averaging (``ema_start_iter``) happens between two replays of
    one graph.  The owner of the graph calls ``graph_reserve`` before the capture (tables outside the graph's memory pool, like
    ``FusedAdam.graph_reserve``), ``graph_take_plan`` after it, and ``graph_prepare`` / ``graph_finish`` around every replay."""

    def __init__(self, lerp, copy=()):
        self.lerp = [(e, p) for e, p in lerp]
        fused = [e.dtype == torch.float32 and b.dtype == torch.float32 and e.is_contiguous() and b.is_contiguous() for e, b in copy]
        self.copy = [pair for pair, f in zip(copy, fused) if f]
        self.plain = [pair for pair, f in zip(copy, fused) if not f]
        for e, p in self.lerp + self.copy + self.plain:
            if e.shape != p.shape or e.device != p.device or e.dtype != p.dtype:
                raise ValueError("EmaGroup: a copy differs from its source in shape, dtype or device")
        if not self.lerp:
            raise ValueError("EmaGroup: nothing to average")
        self.device = self.lerp[0][0].device

    def _launches(self):
        """(pairs, whether their weight is the update's: else 0) of the kernel launches of one update"""
        return [(pairs, lerps) for pairs, lerps in ((self.lerp, True), (self.copy, False)) if pairs]

    @torch.no_grad()
    def update(self, weight):
        """One update with ``weight`` (``ema_weight``).  While a graph is being captured the launches are recorded in their device-read
        form and ``weight`` is not used: every replay reads its own from the rows ``graph_prepare`` keeps."""
        if torch.cuda.is_current_stream_capturing():
            self._update_captured()
            return
        for pairs, lerps in self._launches():
            ema_lerp_([e for e, _ in pairs], [p for _, p in pairs], weight if lerps else 0.0)
        for e, b in self.plain:
            e.copy_(b)

    # ---- graph capture ------------------------------------------------------------------------------------------------
    def graph_reserve(self):
        """Before a capture: a device pointer table per launch and the weight rows, outside the graph's memory pool."""
        tables = [torch.empty((len(pairs), L.ADAM_REC_WORDS), dtype=torch.int64, device=self.device) for pairs, _ in self._launches()]
        self._graph_reserve = {"table": tables, "weights": [_WeightRows(self.device)]}

    def _update_captured(self):
        error = "EmaGroup: no table reserved (call graph_reserve() before the capture; one update per capture)"
        lib = ops._lib_for(self.lerp[0][0])
        for pairs, lerps in self._launches():
            table, table_dev = _PointerTable("EmaGroup", [(e, p, None, None) for e, p in pairs]), self._take_reserved("table", error)
            weights = self._take_reserved("weights", error) if lerps else None
            if lerps:
                L.check(lib.dei2i_ema_lerp_dev(*table.args(table_dev), _dev_ptr(weights.table), _dev_ptr(weights.index), weights.rows,
                                               ops._stream()), "ema_lerp_dev")
                L.check(lib.dei2i_index_advance(_dev_ptr(weights.index), ops._stream()), "index_advance")
            else:
                L.check(lib.dei2i_ema_lerp(*table.args(table_dev), 0.0, ops._stream()), "ema_lerp")
            self._recorded(_CapturedLaunch(table, table_dev, weights))
        for e, b in self.plain:
            e.copy_(b)

    def graph_take_plan(self):
        """-> the update recorded since the last call (None: none); an unused reservation is dropped"""
        return super().graph_take_plan() or None

    def graph_prepare(self, plan, iters, num_critics, start_iter, beta):
        """Before a replay, after ``iters`` iterations, of a graph holding ``plan``: the pointer tables are on the device (uploaded
        once) and the device index is at the row of the G update this replay makes, the one that ends iteration ``iters + 1``."""
        for launch in plan:
            launch.upload()
            if launch.rows is not None:
                launch.rows.ensure(iters + 1, int(num_critics), int(start_iter), float(beta))

    def graph_finish(self, plan):
        """After a replay: the host mirror of the index, and the stamps the eager update would have moved."""
        for launch in plan:
            if launch.rows is not None:
                launch.rows.advance()
        ops.mark_written(*[e for e, _ in self.lerp + self.copy])


class _FusedPlain(_FusedOptimizer):
    """torch.optim.SGD / torch.optim.RMSprop as trainers/base_trainer.py:71-74 constructs them (``optim_cls(params, lr=...)``: no
    momentum, no weight decay; RMSprop alpha 0.99, eps 1e-8, not centered) on csrc/adam.hip's second kernel: one launch per step,
    parameters whose ``grad`` is None skipped (no state), ``grad_scale`` like FusedAdam (the data-parallel 1/world)."""
    KIND = None

    def __init__(self, params, lr, grad_scale=1.0, **defaults):
        if lr < 0.0:
            raise ValueError("invalid learning rate")
        super().__init__(params, dict(lr=lr, **defaults))
        self.grad_scale = float(grad_scale)

    @torch.no_grad()
    def step(self, closure=None):
        loss = self._closure_loss(closure)
        for group in self.param_groups:
            plist = [p for p in group["params"] if p.grad is not None]
            if not plist:
                continue
            lib = ops._lib_for(plist[0])
            table = _PointerTable(type(self).__name__, [(p, p.grad, self._square_avg(p), None) for p in plist])
            table_dev = table.cached(self._tables())
            L.check(lib.dei2i_sgd_rmsprop_step(*table.args(table_dev), self.KIND, float(group["lr"]), float(group.get("alpha", 0.0)),
                                               float(group.get("eps", 0.0)), self.grad_scale, ops._stream()), "sgd_rmsprop_step")
            ops.mark_written(*plist)
        return loss

    def _square_avg(self, p):
        """RMSprop's state of ``p``, made on its first step and counted (None for SGD, which has none)"""
        if self.KIND != 1:
            return None
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            st["square_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        st["step"] += 1
        return st["square_avg"]


class FusedSGD(_FusedPlain):
    KIND = 0

    def __init__(self, params, lr, grad_scale=1.0):
        super().__init__(params, lr, grad_scale)


class FusedRMSprop(_FusedPlain):
    KIND = 1

    def __init__(self, params, lr, alpha=0.99, eps=1e-8, grad_scale=1.0):
        super().__init__(params, lr, grad_scale, alpha=alpha, eps=eps)
