"""``opt.graph_step``: the D step, and the D step + G step, of the defectGAN stage and of the MAE pre-training stage replayed from
captured HIP graphs.

The eager step enqueues ~750 kernels through ~2 000 autograd-Function applies; the host, not the GPU, bounds it.  In graph mode
the trainer's ``step`` runs eagerly for ``opt.graph_warmup`` calls (on the stream the capture will use, so every workspace
exists before the capture), then captures the graph the iteration needs -- D only, or D + G (``num_critics > 1`` replays both)
-- and from then on copies the inputs into static device buffers, replays, and does the host bookkeeping the replay cannot:
``iters``, each optimizer's ``state["step"]`` and the rows of its device hyper-parameter table (optim.FusedAdam), the
``_dei2i_epoch`` stamps (eager code repacks afterwards), ``p.grad`` and one queued device copy of the step's losses.  With
``opt.ema_beta`` the G step ends with the EMA update (optim.EmaGroup), captured in its device-read form: its tables are reserved,
prepared and finished next to the optimizers', and go with the graphs.

A call whose inputs differ in shape, dtype or device from the captured ones runs eagerly on the current stream and keeps the
graphs.  ``release_graphs()`` drops them; a checkpoint load, a change of ``opt.compute_dtype`` and ``attach_ddp`` do so too.
What the capture cannot honour raises ``NotImplementedError`` (``unsupported``).

``opt.diff_aug`` is captured when its parameters are drawn on the device (``opt.diff_aug_rng = "device"``: ops.DiffAugRng, whose
call counter lives in device memory and advances inside the draw launch, so every replay draws what the eager call would have
drawn); with host draws, which a capture would freeze into every replay, it is refused.  The MAE stage's patch masks follow the
same rule (``opt.mask_rng = "device"``: ops.mask_draw / ops.mask_fill; host-drawn masks are refused), and so does its
``opt.grad_scaler``, whose overflow check reads the device once per update.  The SEAN generator is captured with device-drawn
style embeddings (``opt.embed_rng = "device"``: ops.embed_draw on the model's ``EmbedBank``, which the model owns and which
outlives the graphs); with host draws, with ``use_running_stats`` (per-sample host reads) and with ``style_distill`` (a backward
inside the forward) it is refused.  Its four generator passes run one after another: the capture stays one chain."""
import contextlib

import torch

from .. import ops
from ..optim import FusedAdam

_streams = {}


def capture_stream(device):
    """The one stream every graph-mode trainer of a device warms up and captures on (ops.capture_stream)."""
    dev = torch.device(device)
    st = _streams.get(dev)
    if st is None:
        st = _streams[dev] = torch.cuda.Stream(device=dev)
    ops.capture_stream = st
    return st


def unsupported(trainer):
    """-> the first option the captured step cannot honour (None: all supported)"""
    opt = trainer.opt
    if getattr(trainer, "draws_masks", False) and getattr(trainer.model, "mask_rng", None) is None:
        return ("MAETrainer with host-drawn masks (its masks are made on the host and uploaded per update; build the trainer with "
                "mask_rng='device' to draw them on the GPU)")
    scaler = getattr(trainer, "scaler", None)
    if scaler is not None and scaler.is_enabled():
        return "grad_scaler=True (its overflow check is a host sync per update)"
    if getattr(opt, "diff_aug", "") and getattr(trainer.model, "diffaug_rng", None) is None:
        return ("diff_aug with host draws (its parameters are drawn from the CPU RNG and uploaded per call; build the trainer with "
                "diff_aug_rng='device' to draw them on the GPU)")
    if opt.style_norm_block_type == "sean":
        if getattr(opt, "use_running_stats", False):
            return ("style_norm_block_type='sean' with use_running_stats=True (its tracked codes are read per sample with .item() "
                    "into Python lists)")
        if getattr(opt, "style_distill", False):
            return "style_norm_block_type='sean' with style_distill=True (its backward runs inside the SEAN layers' forward)"
        if getattr(trainer.model, "embed_bank", None) is None:
            return ("style_norm_block_type='sean' (it draws style embeddings with the host's random.choices; build the trainer with "
                    "embed_rng='device' to draw them on the GPU)")
    elif opt.style_norm_block_type != "spade":
        return f"style_norm_block_type={opt.style_norm_block_type!r} (only the SPADE and SEAN generators are captured)"
    if getattr(trainer, "reducer", None) is not None:
        return "an attached GradReducer (collectives inside a capture)"
    if not all(type(o) is FusedAdam for o in trainer.optimizers.values()):
        return f"optimizer={opt.optimizer!r} (only the Adam family reads its hyper-parameters from device memory)"
    if ops.wants_fp8(getattr(opt, "compute_dtype", "bf16")):
        return "compute_dtype='fp8' (not captured)"
    if torch.device(opt.device).type != "cuda":
        return "a CPU device"
    return None


class _Captured:
    """One graph and what its replays need on the host."""

    def __init__(self, graph, with_g, plans, grads, keys, losses, keep, ema=None):
        self.graph, self.with_g, self.plans, self.grads, self.keys, self.losses, self.keep, self.ema = \
            graph, with_g, plans, grads, keys, losses, keep, ema


class GraphStep:
    def __init__(self, trainer):
        self.tr = trainer
        self.calls = 0                   # graph-mode calls since the last release (the first graph_warmup of them are eager)
        self.graphs = {}                 # with_g -> _Captured
        self.sig = None                  # (shape, dtype, device) of the step's inputs the graphs were captured for
        self.static = None               # their device buffers
        self.stamp = None                # (model load serial, compute_dtype) at capture

    # ---- lifetime ------------------------------------------------------------------------------------------------------
    def release(self):
        if self.graphs:
            torch.cuda.synchronize()     # (no replay still running when the graphs and their pools go)
        self.graphs, self.sig, self.static, self.stamp = {}, None, None, None
        self.calls = 0

    def _stamp(self):
        return (getattr(self.tr.model, "load_serial", 0), getattr(self.tr.opt, "compute_dtype", "bf16"))

    # ---- the step ------------------------------------------------------------------------------------------------------
    def step(self, *inputs):
        """``inputs``: the trainer's own ``step`` arguments (three tensors for the defectGAN stage, two for the MAE stage)"""
        tr = self.tr
        why = unsupported(tr)
        if why is not None:
            raise NotImplementedError(f"graph_step does not support {why}")
        if self.stamp is not None and self.stamp != self._stamp():
            self.release()
        sig = tuple((tuple(t.shape), t.dtype, t.device) for t in inputs)
        if self.calls < int(getattr(tr.opt, "graph_warmup", 3)):
            self.calls += 1
            with self._on_capture_stream():
                tr._eager_step(*inputs)
            return
        if self.sig is not None and sig != self.sig:
            tr._eager_step(*inputs)      # (the last, smaller batch of an epoch): the graphs stay
            return
        if self.static is None:
            dev = torch.device(tr.opt.device)
            self.static = tuple(torch.empty(t.shape, dtype=t.dtype, device=dev) for t in inputs)
            self.sig = sig
        for dst, src in zip(self.static, inputs):
            dst.copy_(src, non_blocking=True)
        with_g = (tr.iters + 1) % tr.opt.num_critics == 0
        cap = self.graphs.get(with_g)
        if cap is None:
            cap = self.graphs[with_g] = self._capture(with_g)
            self.stamp = self._stamp()
        with self._on_capture_stream():      # the table uploads and the replay, on one stream
            for name, plan in cap.plans.items():
                tr.optimizers[name].graph_prepare(plan)
            if cap.ema is not None:
                tr.model.ema_graph_prepare(cap.ema, tr.iters)
            cap.graph.replay()
        tr.iters += 1
        for name, plan in cap.plans.items():
            tr.optimizers[name].graph_finish(plan)
        if cap.ema is not None:
            tr.model.ema_group.graph_finish(cap.ema)
        for p, g in cap.grads:
            p.grad = g
        if tr.defer_loss_sync:
            tr._pending.append((cap.keys, cap.losses.clone()))
        else:
            for (kind, name), v in zip(cap.keys, cap.losses.tolist()):      # the one read of the step
                tr.losses[kind][name].append(v)

    @contextlib.contextmanager
    def _on_capture_stream(self):
        """Work inside goes on the capture stream, after the caller's stream (the inputs) and before its later work."""
        st = capture_stream(self.tr.opt.device)
        cur = torch.cuda.current_stream(st.device)
        st.wait_stream(cur)
        with torch.cuda.stream(st):
            yield
        cur.wait_stream(st)

    def _trained_modules(self):
        """the networks, and the MAE stage's mask token (a module of the model that is no network: the G optimizer trains it)"""
        model = self.tr.model
        token = getattr(model, "mask_token", None)
        return list(model.networks.values()) + ([token] if isinstance(token, torch.nn.Module) else [])

    def _capture(self, with_g):
        """Record one D (+ G) step on the static inputs.  Every decision the host takes while recording is frozen into the graph,
        so the recording must take the decisions every replay needs: every packed weight copy is rebuilt (all stamps moved),
        the SPADE label-set memo is dropped.  Nothing runs: the caller replays the graph for this iteration."""
        tr = self.tr
        st = capture_stream(tr.opt.device)
        for o in tr.optimizers.values():
            o.graph_take_plan()
            o.graph_reserve()
        ema = getattr(tr.model, "ema_group", None) if with_g else None      # (opt.ema_beta: the G update ends with the EMA's)
        if ema is not None:
            ema.graph_take_plan()
            ema.graph_reserve()
        for net in self._trained_modules():
            ops.mark_written(*net.parameters())
        if hasattr(tr.model, "_label_sets"):
            tr.model._label_sets = None
        keep = list(ops._workspaces.values())        # the graph writes them by address: they must outlive it
        torch.cuda.synchronize()
        ops.capture_serial += 1
        graph = torch.cuda.CUDAGraph(keep_graph=True)      # (the captured graph stays alive next to its executable form)
        tr._graph_records = []
        try:
            with torch.cuda.graph(graph, stream=st):
                tr._train_discriminator_once(*self.static)
                if with_g:
                    tr._train_generator_once(*self.static)
                keys = [k for ks, _ in tr._graph_records for k in ks]
                losses = torch.cat([s for _, s in tr._graph_records])
        finally:
            tr._graph_records = None
        graph.instantiate()
        keep += [w for w in ops._workspaces.values() if all(w is not k for k in keep)]
        plans = {name: o.graph_take_plan() for name, o in tr.optimizers.items()}
        plans = {name: plan for name, plan in plans.items() if plan}
        grads = [(p, p.grad) for net in self._trained_modules() for p in net.parameters()]
        return _Captured(graph, with_g, plans, grads, keys, losses, keep, ema.graph_take_plan() if ema is not None else None)
