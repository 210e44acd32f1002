"""Autograd bindings of the HIP kernels (libdei2i_hip.so).  One ``torch.autograd.Function`` per fused op.

Internal activations are NHWC tensors of the compute dtype (bf16, or f32 in parity mode) whose last dimension is the
channel count padded to a 16-byte vector.  NCHW fp32 appears only at the module boundary (inputs, outputs,
parameters, gradients, state_dict), as in the reference.  Every op requires a GPU tensor; there is no fallback.

Random numbers: ``NoiseInjection`` draws with torch's device RNG; ``diff_augment`` draws its per-sample parameters from the global
CPU RNG and uploads them (the reference's draws), or, given a ``DiffAugRng``, on the device from a counter-based generator whose
call count lives in device memory -- the form a captured graph can replay.  The MAE stage's patch masks have the same two sources
(utils/masks.py on the host; ``mask_draw`` with a ``DeviceRng`` of its own), and so have SEAN's style embeddings (python's
``random.choices`` in the model; ``embed_draw`` on an ``EmbedBank``).
"""
from __future__ import annotations

import ctypes
import weakref
from ctypes import byref, c_int, c_void_p
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from . import _lib as L

ACT = {"none": L.ACT_NONE, None: L.ACT_NONE, "relu": L.ACT_RELU, "leaky_relu": L.ACT_LRELU}
# the ReLU family as a negative-side slope (what the per-image affine, the operand-path and the SPADE backward kernels take)
ACT_SLOPE = {L.ACT_NONE: 1.0, L.ACT_RELU: 0.0, L.ACT_LRELU: 0.2}
_SLOPE_ACT = {slope: act for act, slope in ACT_SLOPE.items()}


@dataclass(frozen=True)
class Precision:
    name: str
    code: int
    dtype: torch.dtype
    vec: int

    def pad(self, c: int) -> int:
        return (c + self.vec - 1) // self.vec * self.vec


BF16 = Precision("bf16", L.BF16, torch.bfloat16, 8)
F32 = Precision("f32", L.F32, torch.float32, 4)


# ---- fp8 forward mode (BASELINE.json configs[4]) ----------------------------------------------------------------
# compute_dtype "fp8": tensors, backward and every other kernel are those of the bf16 mode; inside an fp8_forward(True)
# scope the FORWARD GEMM of the stride-1 3x3 convolutions the fp8 kernel takes runs on e4m3 operands (activations
# quantised with the fixed scale FP8_ACT_SCALE -- they follow a normalisation layer, |x| = O(1) -- weights with
# 448 / amax|w| computed on the device).  Layers the fp8 kernel does not take run in bf16 as usual (that is the bf16
# product path, not a fallback of a failed fp8 call: eligibility is asked first).
FP8_ACT_SCALE = 16.0
_fp8_forward = False


class _GlobalScope:
    """``with`` scope of a module-level switch: sets the module global named ``var`` to ``self.value`` for the block and puts the
    previous value back on exit.  The switches stay plain module attributes (tests and the benchmark read them)."""
    var = None

    def __enter__(self):
        g = globals()
        self.prev, g[self.var] = g[self.var], self.value
        return self

    def __exit__(self, *exc):
        globals()[self.var] = self.prev
        return False


class fp8_forward(_GlobalScope):
    var = "_fp8_forward"

    def __init__(self, on: bool):
        self.value = bool(on)


# fused conv + norm + act (halo-resident kernels).  Run-time switches for same-box A/B timing and for the parity tests of
# fused against unfused:
#   fuse_norm : statistics of a conv's / affine kernel's output from its own epilogue (no separate moments pass)  -- ON
#   fuse_pro  : BatchNorm / SPADE apply on the CONSUMER conv's operand path (the normalised tensor is never written) -- OFF:
#               measured at 256x256 batch 16 (profiles/r02_b_*): the in-LDS transform costs +33 us on a 99 us conv and
#               +34 us on a 91 us wgrad (it is repeated per output-channel tile and again in the wgrad, in kernels whose
#               VALU slots compete with the MFMA issue) against ~39 us of statistics + modulate kernels saved: +1.4 ms/step.
#   fuse_ring : SPADE -> nearest x2 upsample -> conv keeps the normalised tensor at the SOURCE resolution (+ the logical
#               image's 2-pixel frame in a compact ring tensor): the 4x larger upsampled tensor is never written or read -- ON
#   fuse_bwd  : the backward REDUCTIONS of a SPADE / BatchNorm layer (sum dxhat, sum dxhat*xhat, ... per channel) from the epilogue
#               of the input-gradient launch of the conv behind it, while the dz tile is on chip -- the streaming pass that read
#               dz and x again (spade_bwd_partial / bn_bwd_partial) is not launched -- ON
fuse_norm = True
fuse_pro = False
fuse_ring = True
fuse_bwd = True

# The side channel from an autograd Function to its output tensor (a Function cannot set attributes on what it returns: autograd
# wraps it): the forward leaves attribute -> value here, the public wrapper clears the record before .apply and moves whatever
# is present onto the output afterwards.  _dei2i_fp8: the e4m3 copy a normalisation kernel wrote beside its output;
# _dei2i_stats: (partial records, records per image) of a producer (see _stats_of); _dei2i_bwd_hint: see _NormBwdHint.
# _dei2i_stats and _dei2i_fp8 DESCRIBE the tensor's values, so they are bound to its autograd version counter at hand-over
# (_dei2i_at_version): after an in-place write (y.mul_(2), y.add_(res)) the consumer ignores them and measures the tensor itself (_handed).
_handover = {}


def _attach(out):
    if _handover:
        for name, value in _handover.items():
            setattr(out, name, value)
        out._dei2i_at_version = out._version
        _handover.clear()
    return out


def _handed(t, name):
    """The value a producer left on ``t`` under ``name``, or None: nothing left, or ``t`` was written in place since (reading
    ``_version`` is host-only, ~0.1 us)."""
    value = getattr(t, name, None)
    if value is not None and getattr(t, "_dei2i_at_version", None) != t._version:
        return None
    return value


def _fp8_copy_wanted(prec, c: int) -> bool:
    return _fp8_forward and prec is BF16 and c % 128 == 0


def wants_fp8(name) -> bool:
    return name in ("fp8", "fp8_e4m3", "e4m3")


def get_precision(name) -> Precision:
    if isinstance(name, Precision):
        return name
    if name in (None, "bf16", "bfloat16") or wants_fp8(name):
        return BF16
    if name in ("f32", "fp32", "float32"):
        return F32
    raise ValueError(f"compute dtype [{name}] is not supported (bf16 | f32)")


def precision_of(t: torch.Tensor) -> Precision:
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported activation dtype {t.dtype}")


def _require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"de-i2i-gan_amd.{what}: tensor is on {t.device}; the HIP kernels need a GPU tensor "
                           "(there is no CPU fallback)")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else c_void_p(t.data_ptr())


def _f32c(t: torch.Tensor, strict: str = None) -> torch.Tensor:
    """``t`` as a kernel reads an fp32 operand through its raw pointer: ``t`` itself when it is fp32 and contiguous, else a converted
    copy -- or, with ``strict`` (the op's name), a TypeError: the ops that write derived weights do not convert."""
    if t.dtype == torch.float32 and t.is_contiguous():
        return t
    if strict is not None:
        raise TypeError(f"{strict} expects a contiguous fp32 weight")
    return t.float().contiguous()


# The current stream's handle straight from the C layer: ``torch.cuda.current_stream()`` builds a Stream object per call (~8 us of host
# time, several hundred calls per step -- the short steps (MAE stage, recipe options) are host-bound).
_raw_stream_of = torch._C._cuda_getCurrentRawStream
_current_device = torch._C._cuda_getDevice


def _stream_id(device=None) -> int:
    """hipStream_t (as an int) of the current stream of ``device`` (None / index-less: the current device)"""
    idx = getattr(device, "index", device)
    return _raw_stream_of(_current_device() if idx is None else idx)


def _stream():
    return c_void_p(_raw_stream_of(_current_device()))


_initialised = set()


def _lib_for(t: torch.Tensor):
    lib = L.load()
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    if dev not in _initialised:
        L.check(lib.dei2i_init(dev), "init")
        _initialised.add(dev)
    return lib


_workspaces = {}


def _workspace(device, nbytes: int, slot: str = "splitk") -> torch.Tensor:
    """Scratch of one kernel launch (split-K slabs, the padded dgrad frame, ...), reused launch after launch ON ONE STREAM: every
    stream that runs ops has its own set (two chains of a forked pass -- ``forked_chains`` -- must not share slabs)."""
    key = (torch.device(device), slot)
    sid = _stream_id(torch.device(device))
    if sid != _default_stream_id(key[0]):
        key = key + (sid,)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(max(nbytes // 4 + 1, 1 << 20), dtype=torch.float32, device=device)
        _workspaces[key] = ws
    return ws


_default_stream_ids = {}


def _default_stream_id(device):
    sid = _default_stream_ids.get(device)
    if sid is None:
        sid = _default_stream_ids[device] = torch.cuda.default_stream(device).cuda_stream
    return sid


# ---- in-place accumulation of parameter gradients within one backward pass --------------------------------------
# The G step applies every generator layer four times (defectgan_model.py:185-190), so autograd would receive four
# gradients per parameter and sum them with one add kernel each (171 launches per step).  Instead the first backward
# node of a parameter in a pass returns a fresh gradient tensor and remembers it under the pass's graph-task id; the
# later nodes of the same pass add into that memory inside their own kernels (wgrad reduce, BatchNorm finalize) and
# return None -- autograd treats an undefined gradient as "no contribution" and still runs the parameter's
# AccumulateGrad (and its post-accumulate hooks: the data-parallel reducer) once, after its last node.
# Only a WEAK reference is kept: the tensor lives exactly as long as autograd's input buffer holds it, so
# AccumulateGrad can still steal it (no copy), and a later node that finds the reference dead -- the engine dropped
# the gradient (torch.autograd.grad(inputs=[activation]): the accumulator is not executed) or replaced it by an
# out-of-place sum with another op's contribution -- simply returns a fresh tensor of its own, which is always correct.
# Non-leaf weights (concatenated gamma|beta) are not tracked.
_grad_slots = {}


def _grad_target(param, shape, device, stream=None):
    """-> (tensor to return to autograd or None, its address, accumulate flag); ``stream``: the stream the caller's kernels run on
    when that is not the current one (the weight-gradient side stream)"""
    tid = torch._C._current_graph_task_id()
    key = param.data_ptr() if (param.is_leaf and tid >= 0) else None
    # (in-place accumulation is a read-modify-write ordered by ONE stream: a node that runs on another stream -- the two chains of
    #  a forked pass -- returns its own tensor and autograd sums them, with its own stream synchronisation)
    sid = 0
    if key is not None and torch.device(device).type == "cuda":
        sid = stream.cuda_stream if stream is not None else _stream_id(torch.device(device))
    if key is not None:
        slot = _grad_slots.get(key)
        if slot is not None and slot[0] == tid and slot[2] == tuple(shape) and slot[3] == sid:
            first = slot[1]()
            if first is not None:                       # still the tensor in autograd's input buffer
                return None, first.data_ptr(), 1
    t = torch.empty(shape, dtype=torch.float32, device=device)
    if key is not None:
        _grad_slots[key] = (tid, weakref.ref(t), tuple(shape), sid)
    return t, t.data_ptr(), 0


def _wants_grad(ctx, idx: int) -> bool:
    """needs_input_grad[idx], and the engine will actually consume that gradient in this pass (False for a parameter
    under torch.autograd.grad(inputs=[something else]): its wgrad would be computed and dropped)."""
    if not ctx.needs_input_grad[idx]:
        return False
    node = ctx.next_functions[idx][0]
    if node is None:
        return True
    try:
        return bool(torch._C._will_engine_execute_node(node))
    except RuntimeError:
        # torch refuses the query for a LEAF that torch.autograd.grad(inputs=[that leaf]) captures -- its gradient is wanted
        return True


# ---- spectral normalisation of a conv weight (csrc/spectral.hip) --------------------------------------------------
class _SpectralWeight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight_orig, u, v, iterate: bool):
        _require_gpu(weight_orig, "spectral_weight")
        w = _f32c(weight_orig.detach(), strict="spectral_weight")
        cout, k = w.shape[0], w[0].numel()
        lib = _lib_for(w)
        dev = w.device
        scratch = torch.empty(lib.dei2i_spectral_scratch_floats(cout, k), dtype=torch.float32, device=dev)
        u_used = torch.empty(cout, dtype=torch.float32, device=dev)
        v_used = torch.empty(k, dtype=torch.float32, device=dev)
        scal = torch.empty(4, dtype=torch.float32, device=dev)
        w_eff = torch.empty_like(w)
        L.check(lib.dei2i_spectral_fwd(cout, k, _p(w), _p(u), _p(v), 1 if iterate else 0, _p(scratch), _p(u_used), _p(v_used),
                                       _p(scal), _p(w_eff), _stream()), "spectral_fwd")
        if iterate:                      # the buffers were updated in place through raw pointers: bump their cache stamps
            mark_written(u, v)
        ctx.save_for_backward(w_eff, u_used, v_used, scal)
        ctx.param = weight_orig
        return w_eff

    @staticmethod
    def backward(ctx, g):
        w_eff, u_used, v_used, scal = ctx.saved_tensors
        g = g.contiguous()
        cout, k = w_eff.shape[0], w_eff[0].numel()
        lib = _lib_for(w_eff)
        scratch = torch.empty(1024, dtype=torch.float32, device=g.device)
        # the same parameter's later forwards of this backward pass add into the first one's tensor (see _grad_target)
        dw, dw_ptr, accumulate = _grad_target(ctx.param, w_eff.shape, g.device)
        L.check(lib.dei2i_spectral_bwd(cout, k, _p(g), _p(w_eff), _p(u_used), _p(v_used), _p(scal), _p(scratch), c_void_p(dw_ptr),
                                       accumulate, _stream()), "spectral_bwd")
        return dw, None, None, None


def spectral_weight(weight_orig, u, v, iterate: bool):
    """weight_orig / sigma(weight_orig, u, v) with torch.nn.utils.spectral_norm's semantics; ``iterate`` runs one power
    iteration on the (u, v) buffers in place first (training mode)."""
    return _SpectralWeight.apply(weight_orig, u, v, bool(iterate))


# ---- eval-mode BatchNorm folded into the conv in front of it ------------------------------------------------------
# The generator passes of the D step (defectgan_model.py:251-262) and inference run BatchNorm on its RUNNING statistics: a fixed
# per-channel affine.  Folded into the conv's weights (and a bias), BN + LeakyReLU happen in the conv's own epilogue and the
# BatchNorm-apply pass over the conv's output -- a read and a write of the largest tensors of the pass -- is not run.
fold_eval_bn = True


def fold_bn_weight(weight, bn_weight, bn_bias, running_mean, running_var, eps: float):
    """-> (w_eff = a[co] * weight[co], b_eff = bn_bias - running_mean * a) with a = bn_weight * rsqrt(running_var + eps); no
    autograd (eval / no-grad passes only).  ``w_eff`` is marked as derived per call: its packed copy travels with the call."""
    _require_gpu(weight, "fold_bn_weight")
    w = _f32c(weight.detach(), strict="fold_bn_weight")
    cout, k = w.shape[0], w[0].numel()
    w_eff, b_eff = torch.empty_like(w), torch.empty(cout, dtype=torch.float32, device=w.device)
    L.check(_lib_for(w).dei2i_fold_bn_weight(cout, k, _p(w), _p(bn_weight.detach()), _p(bn_bias.detach()), _p(running_mean), _p(running_var),
                                             float(eps), _p(w_eff), _p(b_eff), _stream()), "fold_bn_weight")
    w_eff._dei2i_per_call = True
    return w_eff, b_eff


# ---- NoiseInjection's draw (architecture.py:385-389): N(0,1) on the activations' device; tests install a provider ----
noise_source = None


def draw_noise(shape, device):
    if noise_source is not None:
        return noise_source(tuple(shape))
    return torch.randn(shape, device=device)


class _NoiseInject(torch.autograd.Function):
    """x + weight * noise on an NHWC activation (one noise value per pixel, one scalar weight): one HIP launch forward;
    backward hands dy through and reduces dweight = sum(noise * rowsum(dy)) through ordered block partials."""

    @staticmethod
    def forward(ctx, x, weight, noise):
        _require_gpu(x, "noise_inject")
        prec = precision_of(x)
        x = x.contiguous()
        rows, c = x.numel() // x.shape[-1], x.shape[-1]
        noise = noise.detach().to(device=x.device, dtype=torch.float32).contiguous()
        if noise.numel() != rows:
            raise ValueError(f"noise_inject: {noise.numel()} noise values for {rows} pixels")
        w = weight.detach().reshape(1)
        out = torch.empty_like(x)
        lib = _lib_for(x)
        L.check(lib.dei2i_noise_fwd(prec.code, rows, c, _p(x), _p(noise), _p(w), _p(out), _stream()), "noise_fwd")
        ctx.prec, ctx.wshape, ctx.param = prec, weight.shape, weight
        ctx.save_for_backward(noise)
        return out

    @staticmethod
    def backward(ctx, dy):
        (noise,) = ctx.saved_tensors
        dw = None
        if _wants_grad(ctx, 1):
            dy = dy.contiguous()
            rows, c = noise.numel(), dy.shape[-1]
            part = torch.empty(1024, dtype=torch.float32, device=dy.device)
            dw, dw_ptr, accumulate = _grad_target(ctx.param, ctx.wshape, dy.device)
            L.check(_lib_for(dy).dei2i_noise_bwd(ctx.prec.code, rows, c, _p(dy), _p(noise), _p(part), c_void_p(dw_ptr), accumulate,
                                                 _stream()), "noise_bwd")
        return (dy if ctx.needs_input_grad[0] else None), dw, None


def noise_inject(x, weight, noise):
    """NoiseInjection on an NHWC activation: ``noise`` holds one value per pixel ((N,1,H,W) as the reference draws it)."""
    return _NoiseInject.apply(x, weight, noise)


_const_vecs = {}


def _const_vec(device, n: int, value: float) -> torch.Tensor:
    key = (device, n, value)
    v = _const_vecs.get(key)
    if v is None:
        v = torch.full((n,), value, dtype=torch.float32, device=device)
        _const_vecs[key] = v
    return v


# --------------------------------------------------------------------------------------------------------------
# convolution
# --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConvGeom:
    """nn.Conv2d geometry of one reference conv (architecture.py:51-56,95-100,228-233; normalization.py:17-22)."""
    cin: int
    cout: int
    k: int
    stride: int = 1
    pad: int = 0
    reflect: bool = False
    up: bool = False      # nearest x2 upsample fused in front of the conv (architecture.py:203)


_descs = {}


def _desc(prec: Precision, g: ConvGeom, n: int, h: int, w: int, cins: int, couts: int) -> L.ConvDesc:
    """The conv descriptor of (geometry, shape): made once (a ctypes structure costs ~3 us to build, a step asks ~500 times; the
    library only reads it)."""
    key = (prec.code, g, n, h, w, cins, couts)
    d = _descs.get(key)
    if d is None:
        if len(_descs) > 4096:
            _descs.clear()
        d = _descs[key] = L.ConvDesc(prec.code, n, h, w, g.cin, g.cout, cins, couts, g.k, g.k, g.stride, g.pad,
                                     L.PAD_REFLECT if g.reflect else L.PAD_ZERO, 1 if g.up else 0)
    return d


def mark_written(*tensors) -> None:
    """A kernel wrote these tensors through raw pointers, which moves no autograd version counter: packed copies made of them
    are stale.  The one writer of the ``_dei2i_epoch`` stamp; ``PackedWeights._stamp`` is its one reader."""
    for t in tensors:
        t._dei2i_epoch = getattr(t, "_dei2i_epoch", 0) + 1


class PackedWeights:
    """Kernel-layout copies of one conv weight: forward [Cout][k*k][CinS] and dgrad (per stride-parity class
    [Cin][taps][CoutS]).  Re-packed lazily when any source parameter changed (autograd version counter, or the
    ``_dei2i_epoch`` stamp the fused Adam sets because it updates parameters through raw pointers)."""

    def __init__(self):
        self._key = None
        self.fwd = None
        self.dgrad = None
        self.fp8 = None            # (packed e4m3 forward weights, dequant scalar) of the fp8 forward mode
        self._packed_on = None     # (stream id, event) of the last pack launch: another stream waits for it before reading

    def __deepcopy__(self, memo):
        return PackedWeights()     # (a copied module -- the models' EMA networks -- packs its own weights)

    def _mark_packed(self):
        # (the event object is made once per cache: constructing one per pack launch -- every conv weight after every optimizer step --
        #  was ~20 us of host time each; re-recording moves it to the newest pack launch, which is the one a reader has to wait for)
        ev = self._packed_on[1] if self._packed_on is not None else torch.cuda.Event()
        ev.record()
        self._packed_on = (_stream_id(), ev, capture_serial)

    def _await_pack(self):
        if self._packed_on is not None and self._packed_on[0] != _stream_id():
            # a capture may only wait on events recorded inside it; a pack launched before the capture began is complete by
            # then (graph_capture synchronises the device first)
            if self._packed_on[2] != capture_serial and torch.cuda.is_current_stream_capturing():
                return
            torch.cuda.current_stream().wait_event(self._packed_on[1])

    @staticmethod
    def _stamp(t: torch.Tensor):
        return (t.data_ptr(), t._version, getattr(t, "_dei2i_epoch", 0))      # (the epoch: written by mark_written alone)

    def get(self, weight: torch.Tensor, sources, prec: Precision, geom: ConvGeom, cins: int, couts: int, need_dgrad: bool,
            need_fwd: bool = True, per_call: bool = False):
        # per_call: the weight is DERIVED from the sources anew on every forward and differs between calls whose sources
        # carry the same stamps by the time backward runs (spectral norm: u, v are iterated in place by later forwards)
        # -- its own address identifies the call, and the sources' stamps (moved by those later forwards) must not
        key = ((), prec.code, cins, couts, self._stamp(weight)) if per_call else \
            (tuple(self._stamp(s) for s in sources), prec.code, cins, couts, None)
        if key == self._key and (self.fwd is not None or not need_fwd) and (self.dgrad is not None or not need_dgrad):
            self._await_pack()        # the hit: nothing to build (this is the call of every conv of every pass)
            return self.fwd, self.dgrad
        lib = _lib_for(weight)
        if key != self._key:
            self._key, self.fwd, self.dgrad, self.fp8 = key, None, None, None
        d = _desc(prec, geom, 1, max(geom.k, 4), max(geom.k, 4), cins, couts)
        w = _f32c(weight.detach())
        self._await_pack()            # (copies packed by a launch on ANOTHER stream: the two chains of a forked pass share weights)

        def alloc(layout):
            t = torch.empty(getattr(lib, f"dei2i_packed_{layout}_elems")(byref(d)), dtype=prec.dtype, device=weight.device)
            setattr(self, layout, t)
            return t
        missing = [layout for layout, need in (("fwd", need_fwd), ("dgrad", need_dgrad)) if need and getattr(self, layout) is None]
        if len(missing) == 2:                                                         # the training path: one launch
            L.check(lib.dei2i_pack_weight_both(byref(d), _p(w), _p(alloc("fwd")), _p(alloc("dgrad")), _stream()), "pack_weight_both")
        else:
            for layout in missing:
                L.check(getattr(lib, "dei2i_pack_weight_" + layout)(byref(d), _p(w), _p(alloc(layout)), _stream()), "pack_weight_" + layout)
        if missing:
            self._mark_packed()
        return self.fwd, self.dgrad

    def get_fp8(self, weight: torch.Tensor, sources, prec: Precision, geom: ConvGeom, cins: int, couts: int):
        """e4m3 forward weights (per-tensor scale 448 / amax|w|, computed on the device) and the dequant scalar
        1 / (activation scale * weight scale); cached with the same stamps as the bf16 copies."""
        key = (tuple(self._stamp(s) for s in sources), prec.code, cins, couts, None)
        if key != self._key:
            self._key, self.fwd, self.dgrad, self.fp8 = key, None, None, None
        if self.fp8 is None:
            lib = _lib_for(weight)
            d = _desc(prec, geom, 1, 8, 32, cins, couts)
            w = _f32c(weight.detach())
            amax = torch.linalg.vector_norm(w, ord=float("inf")).reshape(1)
            wq = torch.empty(geom.cout * geom.k * geom.k * cins, dtype=torch.uint8, device=weight.device)
            dequant = torch.empty(1, dtype=torch.float32, device=weight.device)
            L.check(lib.dei2i_pack_weight_fwd_fp8(byref(d), _p(w), _p(amax), FP8_ACT_SCALE, _p(wq), _p(dequant), _stream()),
                    "pack_weight_fwd_fp8")
            self.fp8 = (wq, dequant)
        return self.fp8


def _stats_of(t, n, hw, c):
    """The statistics records a producer kernel left for tensor ``t`` ((N, chunks, 2, C) fp32, chunks), or None."""
    st = _handed(t, "_dei2i_stats")
    if st is None:
        return None
    partial, chunks = st
    if partial.shape != (n, chunks, 2, c) or partial.device != t.device:
        return None
    return partial, chunks


def _leave_stats(n, chunks, c, device):
    """-> fresh (N, chunks, 2, C) fp32 records for the kernel about to write a tensor AND its per-channel moments, left for the norm
    layer that reads that tensor next (the public wrapper moves them onto the output: _attach; _stats_of reads them)."""
    partial = torch.empty((n, chunks, 2, c), dtype=torch.float32, device=device)
    _handover["_dei2i_stats"] = (partial, chunks)
    return partial


def _moment_records(lib, prec, x, n, hw, c):
    """-> ((N, chunks, 2, C) fp32 moment records of the NHWC tensor ``x`` with hw pixels per image, chunks): the records its
    producer left (conv epilogue / affine kernel, see _stats_of) when ``fuse_norm`` is on and they fit, else one statistics pass."""
    have = _stats_of(x, n, hw, c) if fuse_norm else None
    if have is not None:
        return have
    chunks = lib.dei2i_moments_chunks(hw)
    partial = torch.empty((n, chunks, 2, c), dtype=torch.float32, device=x.device)
    L.check(lib.dei2i_moments_partial(prec.code, n, hw, c, _p(x), _p(partial), _stream()), "moments_partial")
    return partial, chunks


def _in_stats(lib, prec, x, n, hw, c, eps):
    """-> (mean, rstd), (N, C) fp32: the InstanceNorm statistics of ``x``"""
    mean = torch.empty((n, c), dtype=torch.float32, device=x.device)
    rstd = torch.empty((n, c), dtype=torch.float32, device=x.device)
    partial, chunks = _moment_records(lib, prec, x, n, hw, c)
    L.check(lib.dei2i_in_finalize(n, hw, c, chunks, _p(partial), eps, _p(mean), _p(rstd), _stream()), "in_finalize")
    return mean, rstd


def _affine_act(lib, prec, x, a, b, res, act, groups=1, stats=None, xq=None, xq_scale=1.0, what="affine_act"):
    """-> act(a[g, c] * x + b[g, c] (+ res)) in one launch over the contiguous (..., C) tensor ``x``: ``groups`` equal row groups with
    coefficient rows a, b (groups, C) fp32.  ``stats``: the (N, chunks, 2, C) records the launch fills with the output's per-image
    moments (x is NHWC then; see _leave_stats), or ``xq``: uint8 storage for an e4m3 copy of the output times ``xq_scale`` (fp8_forward)."""
    c = x.shape[-1]
    if not isinstance(a, torch.Tensor):               # two python numbers: the same coefficients for every channel
        a, b = _const_vec(x.device, c, a), _const_vec(x.device, c, b)
    out = torch.empty_like(x)
    if stats is not None:
        n = x.shape[0]
        L.check(lib.dei2i_affine_act_stats_fwd(prec.code, groups, n, x.numel() // (n * c), c, _p(x), _p(a), _p(b), _p(res), act, _p(out),
                                               _p(stats), _stream()), what)
    else:
        L.check(lib.dei2i_affine_act_fwd(prec.code, groups, x.numel() // (groups * c), c, _p(x), _p(a), _p(b), _p(res), act, _p(out),
                                         _p(xq), xq_scale, _stream()), what)
    return out


def _img_affine_act(lib, prec, x, a, b, slope):
    """-> act(a[n, c] * x + b[n, c]) in one pass over the NHWC tensor ``x``; a, b (N, C) fp32; slope: see ACT_SLOPE"""
    n, h, w, c = x.shape
    cv = c // prec.vec
    if 256 % cv == 0 or cv % 256 == 0:                # (the per-image kernel keeps one channel vector per thread)
        out = torch.empty_like(x)
        L.check(lib.dei2i_affine_act_img_fwd(prec.code, n, h * w, c, _p(x), _p(a), _p(b), slope, _p(out), _stream()), "affine_act_img")
        return out
    return _affine_act(lib, prec, x, a, b, None, _SLOPE_ACT[slope], groups=n)     # odd channel counts: the per-channel kernel, one group per image


class _NormBwdHint:
    """What the input-gradient launch of a conv needs to take the backward reductions of the norm layer in FRONT of the conv in
    its epilogue (csrc/conv_halo16.hip EPIN; include/dei2i_hip.h: dei2i_epi_norm), and where it leaves them: the norm's forward
    makes one, hangs it on its output tensor (``_dei2i_bwd_hint``) and keeps it; the conv that reads that tensor picks it up;
    in backward the conv's dgrad fills ``partial`` and the norm's backward -- handed that very dz tensor -- skips its own
    streaming pass.  kind 1: SPADE class mode + ReLU (x, gb, mean, rstd, up); kind 2: BatchNorm + act (x = y, a, b, mean, rstd)."""
    __slots__ = ("kind", "x", "gb", "mean", "rstd", "a", "b", "act", "up", "group_images", "partial", "chunks", "dz", "dz_version")

    def __init__(self, kind, x, mean, rstd, gb=None, a=None, b=None, act=0, up=False, group_images=0):
        self.kind, self.x, self.mean, self.rstd, self.gb, self.a, self.b, self.act, self.up = kind, x, mean, rstd, gb, a, b, act, up
        self.group_images = group_images                  # kind 2: a / b / mean / rstd are (groups, C) -- images per group, 0: (C,)
        self.partial = self.chunks = self.dz = self.dz_version = None

    def give(self, partial, chunks, dz):
        # the dz tensor itself is held until the norm's backward has looked at it: while this reference exists autograd's input
        # buffer cannot add a second consumer's gradient INTO dz (it accumulates in place only into a buffer nobody else holds),
        # so "same storage, same version" below means "exactly what the dgrad kernel reduced"
        self.partial, self.chunks, self.dz, self.dz_version = partial, chunks, dz, dz._version

    def drop(self):
        self.partial = self.chunks = self.dz = self.dz_version = None

    def take(self, dz):
        """-> (partial, records per image) when ``dz`` is the tensor the conv's dgrad wrote them for, else None (another
        consumer's gradient was added to it, or the dgrad took a kernel without that epilogue)."""
        partial, chunks, mine, version = self.partial, self.chunks, self.dz, self.dz_version
        self.drop()
        if (partial is None or not dz.is_contiguous() or dz.data_ptr() != mine.data_ptr() or dz.shape != mine.shape
                or dz._version != version):
            return None
        bwd_fused_counts["taken"] += 1
        return partial, chunks


bwd_fused_counts = {"epilogue": 0, "taken": 0}   # dgrad launches that took the reductions / norm backwards that used them (tests)


def _sources(sources, weight):
    """The parameters a conv's ``weight`` is made of (their stamps key its packed copies): the weight itself unless the caller says"""
    return tuple(sources) if sources is not None else (weight,)


def _packing(weight, cache, sources, input_grad=False):
    """-> (cache, per_call, need_dgrad) of a conv forward.  per_call: a weight derived anew for THIS call (spectral norm in training
    mode, an eval-folded BatchNorm) -- its packed copies travel with the call (a fresh cache, kept on ctx), not with the module,
    whose single slot the next call would overwrite before this call's backward asks for the dgrad layout.  need_dgrad: trainable
    sources (a backward pass of this optimizer step will want that layout, also when THIS call is the D step's no-grad generator
    pass) or ``input_grad`` (a frozen weight behind an input that needs a gradient: D inside the G step) -> both in one pack launch."""
    per_call = bool(getattr(weight, "_dei2i_per_call", False))
    if per_call:
        cache = PackedWeights()
    return cache, per_call, input_grad or any(s_.requires_grad for s_ in sources)


def _conv_out(lib, d, n, couts, prec, device):
    """-> the uninitialised (N, Ho, Wo, CoutS) output of the conv ``d``"""
    ho, wo = c_int(), c_int()
    lib.dei2i_conv2d_out_shape(byref(d), byref(ho), byref(wo))
    return torch.empty((n, ho.value, wo.value, couts), dtype=prec.dtype, device=device)


def _bn_pro(a, b, act):
    """-> (ProDesc, the tensors it points into): BatchNorm apply + activation on a conv's operand path (see _BnActConv)"""
    return L.ProDesc(a.data_ptr(), b.data_ptr(), 0, ACT_SLOPE[act], None), (a, b)


def _spade_pro(coefs, ring, c, ring_mode=False):
    """-> (ProDesc, the tensors it points into) of _SpadeConv: the interior coefficients A | B = coefs[2] | coefs[3] and the frame's
    ring tensor; ``ring_mode``: the conv's input is normalised already, only the ring is read"""
    if ring_mode:
        return L.ProDesc(None, None, 0, 0.0, ring.data_ptr()), (ring,)
    return L.ProDesc(coefs[2].data_ptr(), coefs[3].data_ptr(), c, 0.0, ring.data_ptr()), (coefs, ring)


def _skip_forward(op, x, gb, skip, up):
    """-> (x, gb) contiguous.  ``skip``: the op also hands x through as a second output (the res block's identity branch: its gradient
    is then added inside the backward-apply kernel, not by a separate autograd add launch) -- x must be the tensor the kernels read"""
    xc = x.contiguous()
    if skip and (up or xc is not x):
        raise ValueError(f"{op}(skip=True) wants a contiguous activation and no upsample")
    return xc, gb.contiguous()


def _skip_backward(op, dskip, x):
    """-> the identity branch's gradient as the backward-apply kernel adds it to dx (None: that branch was not used)"""
    if dskip is not None:
        dskip = dskip.contiguous()
        if dskip.dtype != x.dtype or dskip.shape != x.shape:
            raise RuntimeError(f"{op}: identity-branch gradient does not match the activation")
    return dskip


def _attach_skip(result, skip):
    """_attach for an op called with ``skip``: its Function returned (out, x) then, and the handover belongs on out"""
    return (_attach(result[0]), result[1]) if skip else _attach(result)


def _conv_dgrad(lib, prec, geom, x_shape, couts, g, weight, cache, sources, per_call, dtype, device, hint=None):
    """Gradient w.r.t. the conv's physical input (N, H, W, CinS) from g = dL/dy (activation already folded in).  ``hint``: the
    norm layer that produced the input (_NormBwdHint) -- its backward reductions are taken in this launch when the kernel can."""
    n, h, w, cins = x_shape
    d = _desc(prec, geom, n, h, w, cins, couts)
    _, wd = cache.get(weight, sources, prec, geom, cins, couts, need_dgrad=True, need_fwd=False, per_call=per_call)
    if hint is not None:
        hint.drop()
        up = 1 if hint.up else 0
        if (fuse_bwd and prec is BF16 and tuple(hint.x.shape) == (n, h >> up, w >> up, cins) and hint.x.is_contiguous()
                and lib.dei2i_conv2d_dgrad_norm_supported(byref(d))):
            chunks = lib.dei2i_conv2d_dgrad_norm_chunks(byref(d))
            partial = torch.empty((n, chunks, 4 if hint.kind == 1 else 2, cins), dtype=torch.float32, device=device)
            dx = torch.empty(x_shape, dtype=dtype, device=device)
            en = L.EpiNormDesc(hint.kind, up, hint.act, hint.group_images, hint.x.data_ptr(), hint.mean.data_ptr(), hint.rstd.data_ptr(),
                               hint.gb.data_ptr() if hint.gb is not None else None,
                               hint.a.data_ptr() if hint.a is not None else None,
                               hint.b.data_ptr() if hint.b is not None else None, partial.data_ptr())
            L.check(lib.dei2i_conv2d_dgrad_input_norm(byref(d), _p(g), _p(wd), _p(dx), byref(en), _stream()), "conv2d_dgrad_input_norm")
            hint.give(partial, chunks, dx)
            bwd_fused_counts["epilogue"] += 1
            return dx
    ws = _workspace(device, lib.dei2i_conv2d_workspace_bytes(byref(d)))
    dx = torch.empty(x_shape, dtype=dtype, device=device)
    ext = None
    if (geom.reflect and geom.pad > 0) or geom.up:           # the dgrad frame differs from the input: scratch
        oh, ow = c_int(), c_int()
        lib.dei2i_conv2d_dgrad_shape(byref(d), byref(oh), byref(ow))
        ext = _workspace(device, n * oh.value * ow.value * cins * dx.element_size(), slot="dgrad_frame")
    L.check(lib.dei2i_conv2d_dgrad_input(byref(d), _p(g), _p(wd), _p(ext), _p(dx), _p(ws), ws.numel() * 4, _stream()),
            "conv2d_dgrad_input")
    return dx


def _wgrad_scratch(lib, d, device, slot="wgrad"):
    packed = lib.dei2i_wgrad_slab_elems(byref(d))
    # partial slabs: up to 64, or as many as fit 96 MB (a (co, ci, 9-tap) register block per CU is 256 x 295 KB)
    return _workspace(device, max(packed * 4, min(max(packed * 4 * 64, 96 << 20), 512 << 20)), slot=slot)


# ---- weight gradients on a side stream ---------------------------------------------------------------------------
# Nothing inside a backward pass reads the gradient of a LEAF weight: it goes into the tensor autograd's AccumulateGrad will
# hand to ``param.grad`` (see _grad_target), and the optimizer reads it after the pass.  So those wgrad launches (and their slab
# reduces) need not sit between the dgrad of their layer and the normalisation backward of the previous one on the one
# stream: they run on a second stream, behind an event on the main stream (their operands), with their own split-K scratch;
# the main stream waits for the side stream once, in a callback the engine runs at the end of the pass -- before anyone can
# look at ``param.grad``.  One-workgroup-per-CU MFMA kernels (the wgrads) then overlap the HBM-bound normalisation /
# activation backward kernels and the tails / prologues of the dgrads instead of queueing behind them.  Gradients of
# non-leaf weights (spectral norm's effective weight, concatenated heads / gamma|beta weights) ARE read inside the pass by
# the next autograd node and stay on the main stream.  The data-parallel reducer makes its all-reduce stream wait for the
# side stream as well (parallel.GradReducer._launch).
# The side stream reads its operands -- above all the incoming gradient g -- after the node has returned, and autograd may write
# into g IN PLACE on the main stream meanwhile: ``ops.add``'s backward hands the same g to the residual branch's conv and to the
# shortcut, and behind an identity shortcut g lands in the block input's InputBuffer, which adds the other branch's gradient into it
# (``g.add_(dx)``) when it holds the only reference.  So every side-stream launch keeps its operands referenced until an event
# behind it on the side stream has completed (or the pass's join): with a second reference autograd adds out of place (same bits).
wgrad_side_stream = True
_wgrad_streams = {}
_wgrad_join_pending = {}         # device -> graph-task id of the pass whose end-of-pass join is queued
_wgrad_pins = {}                 # device -> [(event on the side stream, operands the side stream reads)], oldest first


def wgrad_stream(device):
    """The side stream the leaf-weight gradients of the current / last backward pass were computed on (None: none yet)."""
    return _wgrad_streams.get(torch.device(device))


def _wgrad_join(device, tid):
    def join():
        if _wgrad_join_pending.get(device) == tid:
            del _wgrad_join_pending[device]
        side = _wgrad_streams[device]
        _wgrad_pins.pop(device, None)          # every stream that goes on waits for the side stream below
        if capture_stream is not None and _capturing(side):
            # inside a graph capture only streams of the capture may wait (a wait on the default stream -- not captured -- would
            # invalidate it): the current stream, the capture's own stream and the chain streams the pass forked into it
            for st in (torch.cuda.current_stream(device), capture_stream) + tuple(_chain_streams.get(torch.device(device), ())):
                if _capturing(st):
                    st.wait_stream(side)
            return
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.default_stream(device).wait_stream(side)
        for st in _chain_streams.get(torch.device(device), ()):       # (whichever stream the caller goes on with)
            st.wait_stream(side)
        if capture_stream is not None:                                 # (graph mode's eager warm-up steps run on that stream)
            capture_stream.wait_stream(side)
    return join


# ---- graph capture (trainers' graph_step) ----------------------------------------------------------------------------------
capture_stream = None            # the stream graph_step captures (and warms up) on; None: graph mode is not in use
capture_serial = 0               # +1 per capture: events recorded before the current capture are not waited on inside it


def _capturing(stream) -> bool:
    with torch.cuda.stream(stream):
        return torch.cuda.is_current_stream_capturing()


def _conv_wgrad(lib, prec, geom, x, g, weight, pro=None, keep=()):
    """OIHW fp32 weight gradient (in-place accumulated across the nodes of one pass: _grad_target); ``pro``: the conv's
    input was normalised on the operand path, x is the un-normalised tensor; ``keep``: the tensors ``pro`` points into."""
    n, h, w, cins = x.shape
    d = _desc(prec, geom, n, h, w, cins, g.shape[-1])
    dev = x.device
    side = None
    tid = torch._C._current_graph_task_id()
    # only when AccumulateGrad will STEAL the tensor (param.grad undefined): with a defined .grad it launches `grad += dw` on the
    # main stream in the middle of the pass, before the end-of-pass join -- those gradients stay on the main stream
    if wgrad_side_stream and weight.is_leaf and tid >= 0 and weight.grad is None:
        side = _wgrad_streams.get(dev)
        if side is None:
            side = _wgrad_streams[dev] = torch.cuda.Stream(device=dev)
    if side is not None:
        # the side stream's split-K scratch is allocated (and re-grown) ON the side stream: the caching allocator then hands a
        # dropped buffer's block only to later side-stream allocations, which run behind the kernels that still use it
        with torch.cuda.stream(side):
            scratch = _wgrad_scratch(lib, d, dev, "wgrad_side")
        if capture_stream is not None and torch.cuda.is_current_stream_capturing():
            # graph capture (trainers/graph_step.py): the launch stays on the capturing stream, so the graph is one chain of nodes,
            # with the side stream's scratch -- the split-K count follows the scratch's size, and this one gives the eager bits
            side = None
    else:
        scratch = _wgrad_scratch(lib, d, dev, "wgrad")
    # (all leaf-weight gradients of a pass run on the ONE side stream, whichever stream their node belongs to: they accumulate in place
    #  across the chains of a forked pass too -- and no autograd add ever reads them before the end-of-pass join)
    dw, dw_ptr, accumulate = _grad_target(weight, weight.shape, dev, stream=side)

    def launch():
        if pro is None:
            L.check(lib.dei2i_conv2d_wgrad_oihw(byref(d), _p(x), _p(g), _p(scratch), scratch.numel(), c_void_p(dw_ptr), accumulate,
                                                _stream()), "conv2d_wgrad")
        else:
            L.check(lib.dei2i_conv2d_wgrad_oihw_pro(byref(d), _p(x), _p(g), _p(scratch), scratch.numel(), c_void_p(dw_ptr), accumulate,
                                                    byref(pro), _stream()), "conv2d_wgrad_pro")
    if side is None:
        launch()
        return dw
    side.wait_stream(torch.cuda.current_stream(dev))          # x, g (and an earlier node's contribution to dw) are ready
    with torch.cuda.stream(side):
        launch()
    for t in (x, g, dw) + tuple(keep):                        # the allocator must not hand their memory out before the side stream is done
        if t is not None:
            t.record_stream(side)
    pins = _wgrad_pins.setdefault(dev, [])
    while pins and pins[0][0].query():                        # (one stream: events complete in order)
        pins.pop(0)
    done = torch.cuda.Event()
    done.record(side)
    pins.append((done, (x, g) + tuple(keep)))                 # no in-place write into them until the side stream has read them
    if _wgrad_join_pending.get(dev) != tid:                   # (a pass that raised never ran its callback: its id is stale)
        _wgrad_join_pending[dev] = tid
        torch.autograd.Variable._execution_engine.queue_callback(_wgrad_join(dev, tid))
    return dw


# ---- double backward (stargan-v2's R1 penalty, core/solver.py:573-583) ---------------------------------------------
# r1_reg differentiates d sum(D(x)) / dx with create_graph=True and back-propagates 0.5 * |that|^2 into D's parameters: the
# BACKWARD pass of D's input gradient is itself differentiated.  While such a graph is being recorded (grad mode on inside a
# backward: create_graph=True) the ops below compute their input gradients with autograd Functions of their own
# -- each a linear map whose transpose is again one of the kernels: the conv's input gradient (transpose: the forward conv;
# with respect to the weight: the wgrad kernel on (incoming, dy)), the activation mask, the average pool, the layout changes.
# Parameter gradients of that first-order pass are not needed (r1_reg asks for the input gradient only) and stay on the plain path.
def _second_order(g) -> bool:
    # grad mode is ON inside a backward pass exactly when it runs with create_graph=True; the incoming gradient itself need not
    # require grad (the seed of d sum(D(x)) is a constant) -- the result still depends on the weights
    return torch.is_grad_enabled() and g is not None


class _ActBwd(torch.autograd.Function):
    """g = dy * act'(z) with the mask taken from the activation's OUTPUT z (ReLU family): linear in dy, mask constant"""

    @staticmethod
    def forward(ctx, dy, z, act: int):
        dy = dy.contiguous()
        g = torch.empty_like(dy)
        L.check(_lib_for(dy).dei2i_act_bwd(precision_of(dy).code, dy.numel(), _p(dy), _p(z), act, _p(g), _stream()), "act_bwd")
        ctx.act = act
        ctx.save_for_backward(z)
        return g

    @staticmethod
    def backward(ctx, gg):
        (z,) = ctx.saved_tensors
        return _ActBwd.apply(gg.contiguous(), z, ctx.act), None, None


class _ConvDgradFn(torch.autograd.Function):
    """dx = W^T (*) g: the conv's input gradient as a function of (g, W).  Its own gradients: with respect to g the FORWARD conv of
    the incoming gradient, with respect to W the weight-gradient kernel on (x := incoming, dy := g).  Plain geometry only (zero
    padding, no fused upsample): what the discriminators differentiated twice use."""

    @staticmethod
    def forward(ctx, g, weight, cache, sources, geom: ConvGeom, x_shape, prec):
        lib = _lib_for(g)
        g = g.contiguous()
        ctx.geom, ctx.cache, ctx.sources, ctx.prec = geom, cache, sources, prec
        ctx.save_for_backward(g, weight)
        return _conv_dgrad(lib, prec, geom, tuple(x_shape), g.shape[-1], g, weight, cache, sources, False, g.dtype, g.device)

    @staticmethod
    def backward(ctx, gdx):
        g, weight = ctx.saved_tensors
        gdx = gdx.contiguous()
        dg = dw = None
        if ctx.needs_input_grad[0]:
            dg = _Conv2d.apply(gdx, weight.detach(), None, ctx.cache, ctx.sources, ctx.geom, L.ACT_NONE, False)
        if _wants_grad(ctx, 1):
            dw = _conv_wgrad(_lib_for(g), ctx.prec, ctx.geom, gdx, g, weight)
        return dg, dw, None, None, None, None, None


class _Conv2d(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, cache: PackedWeights, sources, geom: ConvGeom, act: int, want_stats: bool = False):
        _require_gpu(x, "conv2d")
        prec = precision_of(x)
        # the norm layer that wrote x left what this conv's dgrad needs to take its backward reductions (see _NormBwdHint)
        ctx.hint = getattr(x, "_dei2i_bwd_hint", None) if (x.is_contiguous() and not geom.up) else None
        x = x.contiguous()
        n, h, w, cins = x.shape
        couts = prec.pad(geom.cout)
        lib = _lib_for(x)
        d = _desc(prec, geom, n, h, w, cins, couts)
        cache, per_call, want_dgrad = _packing(weight, cache, sources, bool(ctx.needs_input_grad[0]))
        use_fp8 = bool(_fp8_forward and prec is BF16 and not per_call and lib.dei2i_conv2d_fp8_supported(byref(d)))
        wf = None if use_fp8 else cache.get(weight, sources, prec, geom, cins, couts, need_dgrad=want_dgrad, per_call=per_call)[0]
        y = _conv_out(lib, d, n, couts, prec, x.device)
        b32 = None if bias is None else _f32c(bias.detach())
        # the epilogue of the halo-resident kernel can leave the per-channel statistics of y for the norm that follows
        stats_fused = bool(want_stats and fuse_norm and not use_fp8 and prec is BF16 and lib.dei2i_conv2d_fused_supported(byref(d), 0))
        if use_fp8:
            wq, dequant = cache.get_fp8(weight, sources, prec, geom, cins, couts)
            xq = _handed(x, "_dei2i_fp8")            # written by the producing normalisation kernel in the same pass
            if xq is not None and xq.numel() == x.numel():
                del x._dei2i_fp8                     # one consumer: release the copy after this launch
            else:
                xq = _workspace(x.device, x.numel(), slot="fp8_act")
                L.check(lib.dei2i_quantize_fp8(x.numel(), _p(x), FP8_ACT_SCALE, _p(xq), _stream()), "quantize_fp8")
            L.check(lib.dei2i_conv2d_fwd_fp8(byref(d), _p(xq), _p(wq), _p(b32), _p(dequant), act, _p(y), _stream()),
                    "conv2d_fwd_fp8")
        elif stats_fused:
            partial = _leave_stats(n, lib.dei2i_conv2d_stats_chunks(byref(d)), couts, x.device)
            L.check(lib.dei2i_conv2d_fwd_fused(byref(d), _p(x), _p(wf), _p(b32), act, _p(y), None, _p(partial), _stream()),
                    "conv2d_fwd_fused")
        else:
            ws = _workspace(x.device, lib.dei2i_conv2d_workspace_bytes(byref(d)))
            L.check(lib.dei2i_conv2d_fwd(byref(d), _p(x), _p(wf), _p(b32), act, _p(y), _p(ws), ws.numel() * 4, _stream()),
                    "conv2d_fwd")
        ctx.geom, ctx.act, ctx.cache, ctx.sources, ctx.prec, ctx.per_call = geom, act, cache, sources, prec, per_call
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, y if act != L.ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        geom, prec, act = ctx.geom, ctx.prec, ctx.act
        lib = _lib_for(x)
        dy = dy.contiguous()
        couts = dy.shape[-1]
        st = _stream()
        if _second_order(dy):                                # the input gradient as a differentiable function of dy (see _ConvDgradFn)
            if (geom.reflect and geom.pad > 0) or geom.up or ctx.per_call:
                raise NotImplementedError("double backward through a reflect-padded / upsample-fused / per-call-weight conv is not built")
            g2 = _ActBwd.apply(dy, y, act) if act != L.ACT_NONE else dy
            dx2 = _ConvDgradFn.apply(g2, weight, ctx.cache, ctx.sources, geom, tuple(x.shape), prec) if ctx.needs_input_grad[0] else None
            dw2 = _conv_wgrad(lib, prec, geom, x, g2.detach(), weight) if _wants_grad(ctx, 1) else None
            db2 = None
            if ctx.has_bias and _wants_grad(ctx, 2):
                db2 = g2.detach().float().sum(dim=(0, 1, 2))[:geom.cout]
            return dx2, dw2, db2, None, None, None, None, None
        if act != L.ACT_NONE:
            g = torch.empty_like(dy)
            L.check(lib.dei2i_act_bwd(prec.code, dy.numel(), _p(dy), _p(y), act, _p(g), st), "act_bwd")
        else:
            g = dy
        dx = dw = db = None
        if _wants_grad(ctx, 1):                              # (first: on its side stream it then runs beside the dgrad)
            dw = _conv_wgrad(lib, prec, geom, x, g, weight)
        if _wants_grad(ctx, 0):
            dx = _conv_dgrad(lib, prec, geom, tuple(x.shape), couts, g, weight, ctx.cache, ctx.sources, ctx.per_call, x.dtype, x.device,
                             hint=ctx.hint)
        if ctx.has_bias and _wants_grad(ctx, 2):
            dbf = torch.empty(couts, dtype=torch.float32, device=x.device)
            rows = g.numel() // couts
            part = torch.empty(lib.dei2i_colsum_blocks(rows) * couts, dtype=torch.float32, device=x.device)
            L.check(lib.dei2i_colsum(prec.code, rows, couts, _p(g), _p(part), _p(dbf), st), "colsum")
            db = dbf if couts == geom.cout else dbf[:geom.cout].clone()
        return dx, dw, db, None, None, None, None, None


def conv2d(x, weight, bias, cache: PackedWeights, geom: ConvGeom, act="none", sources=None, stats=False):
    """y = act(conv(x) + bias) on an NHWC activation; ``weight`` is the reference's OIHW fp32 parameter.  ``stats``: a
    BatchNorm / InstanceNorm follows -- leave the statistics records of y with it when the kernel can (see _stats_of)."""
    _handover.clear()
    return _attach(_Conv2d.apply(x, weight, bias, cache, _sources(sources, weight), geom, ACT[act], bool(stats)))


# --------------------------------------------------------------------------------------------------------------
# layout at the module boundary
# --------------------------------------------------------------------------------------------------------------
# The two conversions are each other's transpose: a Function's forward and its partner's first-order backward are the same launch
# (the two plain functions); while a double-backward graph is recorded (_second_order) the backward is the partner Function itself.
def _nchw_to_nhwc(x, prec: Precision, cs: int, size=None):
    """NCHW -> (N, h, w, cs) NHWC of ``prec`` (channels zero-padded to cs); ``size``: nearest resize to (h, w) on the way"""
    x = _f32c(x)
    n, c, hs, ws = x.shape
    h, w = (hs, ws) if size is None else size
    out = torch.empty((n, h, w, cs), dtype=prec.dtype, device=x.device)
    L.check(_lib_for(x).dei2i_nchw_to_nhwc_resize(prec.code, n, c, hs, ws, h, w, cs, _p(x), _p(out), _stream()), "nchw_to_nhwc")
    return out


def _nhwc_to_nchw(x, prec: Precision, c: int):
    """NHWC of ``prec`` -> (N, c, H, W) fp32: the first c channels"""
    x = x.contiguous()
    n, h, w, cs = x.shape
    out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    L.check(_lib_for(x).dei2i_nhwc_to_nchw(prec.code, n, c, h, w, cs, _p(x), _p(out), _stream()), "nhwc_to_nchw")
    return out


class _ToNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, prec: Precision, size):
        _require_gpu(x, "to_nhwc")
        out = _nchw_to_nhwc(x, prec, prec.pad(x.shape[1]), size)
        ctx.c, ctx.prec, ctx.resized = x.shape[1], prec, tuple(out.shape[1:3]) != tuple(x.shape[2:])
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.resized:
            raise RuntimeError("to_nhwc with nearest resize is only differentiable w.r.t. nothing (label maps)")
        if _second_order(g):                              # R1-style penalties differentiate this backward: the conversion is linear
            return _ToNCHW.apply(g, ctx.c), None, None
        return _nhwc_to_nchw(g, ctx.prec, ctx.c), None, None


class _ToNCHW(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c: int):
        _require_gpu(x, "to_nchw")
        ctx.prec, ctx.cs = precision_of(x), x.shape[-1]
        return _nhwc_to_nchw(x, ctx.prec, c)

    @staticmethod
    def backward(ctx, g):
        if _second_order(g):
            return _ToNHWC.apply(g, ctx.prec, None), None
        return _nchw_to_nhwc(g, ctx.prec, ctx.cs), None


def to_nhwc(x_nchw, prec: Precision, size=None):
    """NCHW fp32 -> NHWC compute dtype (channels zero-padded); ``size`` fuses F.interpolate(mode='nearest')."""
    return _ToNHWC.apply(x_nchw, prec, size)


def to_nchw(x_nhwc, c: int):
    return _ToNCHW.apply(x_nhwc, c)


# --------------------------------------------------------------------------------------------------------------
# BatchNorm2d (+ LeakyReLU) (+ residual)
# --------------------------------------------------------------------------------------------------------------
forked_chains = True             # the G loss's two independent chains of generator passes on two streams (models/defectgan_model.py)
_chain_streams = {}


def chain_streams(device):
    """The two streams the chains of a forked pass run on (created once per device)."""
    dev = torch.device(device)
    st = _chain_streams.get(dev)
    if st is None:
        st = _chain_streams[dev] = (torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev))
    return st


# ---- passes of the same network that share nothing but the parameters, as ONE batch -----------------------------------------
# The G loss's chain heads (bg -> fake_defects, df -> fake_normals) and its chain tails (-> recover_normals, -> recover_defects)
# are pairs of independent passes of the same generator (defectgan_model.py:185-190).  Everything in the generator acts per
# sample except training-mode BatchNorm, whose statistics are per PASS: with ``bn_batch_groups(g)`` a training-mode BatchNorm
# takes its statistics (and its backward reductions) over each of g equal groups of the batch separately, so that one pass over
# the concatenated batch is the same function as the g passes -- with half the launches, half the per-launch tails and
# weight-gradient reductions, and every conv at twice the tile count.  The running statistics are updated per group through
# ``bn_running_deferred`` (pass_index = one index per group), which replays them in the reference's pass order.
label_path_batched = True        # SPADE's gamma | beta table convs of all modules in one launch per direction (csrc/label_path.hip)
paired_passes = True             # the G loss's four generator passes as two passes over 2 x batch (models/defectgan_model.py)
bn_groups = 1


class bn_batch_groups(_GlobalScope):
    var = "bn_groups"

    def __init__(self, groups: int):
        self.value = int(groups)


# ---- two independent chains of generator passes on two streams ---------------------------------------------------
# The G loss runs the generator four times (defectgan_model.py:185-190): fake_defects -> recover_normals and fake_normals ->
# recover_defects are two chains that share nothing but the parameters.  On two streams the kernels of one chain fill the other
# chain's kernel tails and launch boundaries (a dependent kernel boundary is ~1.7 us and the step has ~1 350 of them) and its
# HBM-bound passes run beside the other's MFMA-bound ones.  What has to stay ordered is BatchNorm's running-statistics update
# (running = (1 - m) * running + m * batch, four times, in the reference's pass order): inside a ``bn_running_deferred`` scope a
# training-mode BatchNorm leaves m * batch of its pass in a buffer of its own, and ``apply()`` replays the updates in the order
# the passes were NUMBERED, on the joining stream.
class bn_running_deferred:
    current = None

    _arenas = {}                     # device -> flat fp32 zeros the passes' buffers are carved from (zeroed again by apply(): one fill per step)

    def __init__(self):
        self.updates = []            # (pass index, running_mean, running_var, num_batches_tracked, m * batch mean, m * batch var, momentum)
        self.pass_index = 0
        self._used = {}

    def __enter__(self):
        self.prev, bn_running_deferred.current = bn_running_deferred.current, self
        return self

    def __exit__(self, *exc):
        bn_running_deferred.current = self.prev
        return False

    def take_groups(self, running_mean, running_var, num_batches_tracked, momentum, groups):
        """Zeroed buffers for this pass's m * batch statistics, one pair per group, evenly spaced in ONE block -- (groups, 2, n): group
        g's mean at row (g, 0), its variance at (g, 1) -- so that one finalize launch serves all groups (dei2i_bn_finalize_train:
        stride 2 n)."""
        dev, n = running_mean.device, running_mean.numel()
        arena, off = bn_running_deferred._arenas.get(dev), self._used.get(dev, 0)
        if arena is None or off + 2 * n * groups > arena.numel() or running_mean.dtype != torch.float32:
            block = torch.zeros(groups * 2 * n, dtype=torch.float32, device=dev)
            self._want = getattr(self, "_want", 0) + 2 * n * groups
        else:
            block = arena[off:off + 2 * n * groups]
            self._used[dev] = off + 2 * n * groups
        block = block.view(groups, 2, n)
        for g in range(groups):
            index = self.pass_index[g] if isinstance(self.pass_index, (tuple, list)) else self.pass_index
            self.updates.append((index, running_mean, running_var, num_batches_tracked, block[g, 0], block[g, 1], momentum))
        return block

    def apply(self):
        """running <- (1 - m) * running + (m * batch) for every recorded update, passes in index order (on the current stream,
        which must already wait for the streams the passes ran on)"""
        for k in sorted({u[0] for u in self.updates}):
            ups = [u for u in self.updates if u[0] == k]
            for m in sorted({u[6] for u in ups}):
                sel = [u for u in ups if u[6] == m]
                run = [u[1] for u in sel] + [u[2] for u in sel]
                torch._foreach_mul_(run, 1.0 - m)
                torch._foreach_add_(run, [u[4] for u in sel] + [u[5] for u in sel])
            counters = [u[3] for u in ups if u[3] is not None]
            if counters:
                torch._foreach_add_(counters, 1)
        devs = {u[1].device for u in self.updates}
        self.updates = []
        for dev in devs:                         # the arena is all zeros again for the next scope; grown to what this one asked for
            need = self._used.get(dev, 0) + getattr(self, "_want", 0)
            arena = bn_running_deferred._arenas.get(dev)
            if arena is None or arena.numel() < need:
                bn_running_deferred._arenas[dev] = torch.zeros(max(need, 1 << 12), dtype=torch.float32, device=dev)
            elif self._used.get(dev, 0):
                arena[:self._used[dev]].zero_()
        self._used, self._want = {}, 0


# ---- a batch sharded over processes: training-mode BatchNorm over the GLOBAL batch (synchronised BatchNorm) --------------------
# Inside ``bn_sync(exchange)`` every training-mode BatchNorm finalizes in three stages instead of one launch, forward and backward
# (csrc/reduce.hip: dei2i_bn_sync_*): this process's records -> one small fp64 message for all groups of the layer; ``exchange(msg)``
# sums the message over the ranks in place, stream-ordered on the current stream (an all-reduce: ``parallel.GradReducer`` with
# ``sync_bn``; any callable on the tensor serves); finalize / apply from the summed message.  The scope is read when the layer's FORWARD
# runs and kept with it, so its backward exchanges whether or not the scope is still open.  ``rank`` / ``world`` tell the callers that
# draw per-sample random numbers on the host (the MAE stage's patch masks) which rows of the global batch are theirs; every rank holds the same number of rows (backward's 1 / global pixels is world x local).
class bn_sync:
    current = None

    def __init__(self, exchange, rank: int = 0, world: int = 1):
        self.exchange = getattr(exchange, "sync_bn_exchange", exchange)
        self.rank, self.world = int(getattr(exchange, "rank", rank)), int(getattr(exchange, "world", world))

    def __enter__(self):
        self.prev, bn_sync.current = bn_sync.current, self
        return self

    def __exit__(self, *exc):
        bn_sync.current = self.prev
        return False


def _bn_coefs(lib, y, prec, weight, bias, running_mean, running_var, training, momentum, eps, num_batches_tracked, groups=1, sync=None):
    """BatchNorm2d statistics + affine coefficients of an NHWC tensor: a[c] = weight * rstd, b[c] = bias - mean * a (batch
    statistics in training mode, running statistics otherwise; running buffers and the counter are updated in place).
    a, b, mean, rstd of shape (groups, C): training-mode statistics per group of the batch (see bn_batch_groups).
    The statistics come from the records its producer left (conv epilogue / affine_act_stats) when there are any.
    ``sync``: the bn_sync scope of a training-mode layer -- the statistics are those of the batch summed over the ranks."""
    n, h, w, c = y.shape
    dev, st = y.device, _stream()
    w32, b32 = _f32c(weight.detach()), _f32c(bias.detach())
    nf = w32.numel()
    if n % groups or nf > c or running_mean.numel() != nf or running_var.numel() != nf:
        raise ValueError(f"batchnorm_act: {groups} groups over a batch of {n} / {nf} features for a {c}-channel activation")
    deferred = bn_running_deferred.current if training else None
    if groups > 1 and (deferred is None or not isinstance(deferred.pass_index, (tuple, list)) or len(deferred.pass_index) != groups):
        raise RuntimeError("batchnorm_act: grouped batch statistics want a bn_running_deferred scope with one pass index per group")
    # the channel stride is padded to a 16-byte vector (c > num_features: widths that are no multiple of 8 / 4): the kernels index
    # every per-channel vector up to c, so hand them padded copies -- weight = bias = 0 makes the padded channels' a = b = 0 (their
    # activations stay zero) -- and copy the live running statistics back
    if nf < c:
        w32, b32 = (torch.cat([v, v.new_zeros(c - nf)]) for v in (w32, b32))
    a, b = (torch.empty((groups, c), dtype=torch.float32, device=dev) for _ in range(2))
    if not training:
        rm, rv = running_mean, running_var
        if nf < c:
            rm, rv = torch.cat([rm.detach(), rm.new_zeros(c - nf)]), torch.cat([rv.detach(), rv.new_ones(c - nf)])
        L.check(lib.dei2i_bn_finalize_eval(c, _p(w32), _p(b32), _p(rm), _p(rv), eps, _p(a), _p(b), st), "bn_finalize_eval")
        return a, b, rm.detach().clone().view(1, c), torch.rsqrt(rv.detach() + eps).view(1, c), nf
    mean, rstd = (torch.empty((groups, c), dtype=torch.float32, device=dev) for _ in range(2))
    partial, chunks = _moment_records(lib, prec, y, n, h * w, c)
    if deferred is not None:                     # this pass's m * batch statistics go to buffers of their own (see bn_running_deferred)
        block = deferred.take_groups(running_mean, running_var, num_batches_tracked, float(momentum), groups)       # (groups, 2, nf)
        rm, rv, num_batches_tracked = block[:, 0], block[:, 1], None
    else:                                        # (groups == 1) the module's own buffers and counter
        rm, rv = running_mean.view(1, nf), running_var.view(1, nf)
    live = rm, rv
    if nf < c:                                   # c-sized rows for the kernel; the live [:nf] is copied back below
        pad = torch.zeros((groups, 2, c), dtype=torch.float32, device=dev)
        if deferred is None:                     # (the deferred buffers are zeros already)
            pad[0, 0, :nf], pad[0, 1, :nf] = running_mean, running_var
        rm, rv = pad[:, 0], pad[:, 1]
    if sync is not None:
        msg = torch.empty((groups, 2 * c + 1), dtype=torch.float64, device=dev)      # sum x | sum x^2 | count, every group in one message
        L.check(lib.dei2i_bn_sync_fwd_sums(groups, n // groups, h * w, c, chunks, _p(partial), _p(msg), st), "bn_sync_fwd_sums")
        sync.exchange(msg)
        L.check(lib.dei2i_bn_sync_fwd_finalize(groups, c, _p(msg), _p(w32), _p(b32), _p(rm), _p(rv), rm.stride(0), momentum, eps,
                                               _p(mean), _p(rstd), _p(a), _p(b), _p(num_batches_tracked), _stream()), "bn_sync_fwd_finalize")
    else:
        L.check(lib.dei2i_bn_finalize_train(groups, n // groups, h * w, c, chunks, _p(partial), _p(w32), _p(b32), _p(rm), _p(rv), rm.stride(0),
                                            momentum, eps, _p(mean), _p(rstd), _p(a), _p(b), _p(num_batches_tracked), st), "bn_finalize_train")
    if nf < c:
        live[0].copy_(rm[:, :nf])
        live[1].copy_(rv[:, :nf])
    return a, b, mean, rstd, nf


def _bn_backward(lib, prec, dout, y, a, b, mean, rstd, act, training, weight, bias, nf, hint=None, sync=None):
    """-> (dy, dweight, dbias) of z = act(a*y + b) given dL/dz (csrc/reduce.hip: bn_bwd_partial / bn_bwd_apply).  ``hint``: the
    dgrad of the conv behind the layer may have left the reduction records already (_NormBwdHint).  a, b, mean, rstd of shape
    (groups, C): statistics per group of the batch (bn_batch_groups) -- the reductions and the apply run per group, the
    parameter gradients are summed over the groups.  ``sync``: the bn_sync scope the forward ran in -- dy takes the reductions of the
    batch summed over the ranks; dweight / dbias stay this process's share (the gradient exchange totals parameter gradients)."""
    st = _stream()
    have = hint.take(dout) if hint is not None else None
    dout = dout.contiguous()
    n, h, w, c = y.shape
    groups = a.shape[0]
    pixels = n // groups * h * w
    if have is not None:
        partial, chunks = have[0], n // groups * have[1]     # (n, records per image, 2, c): a group's records are contiguous
    else:
        chunks = lib.dei2i_bn_bwd_chunks(pixels)
        partial = torch.empty((groups * chunks, 2, c), dtype=torch.float32, device=y.device)
        L.check(lib.dei2i_bn_bwd_partial(prec.code, groups, pixels, c, _p(dout), _p(y), _p(a), _p(b), _p(mean), _p(rstd), act,
                                         _p(partial), st), "bn_bwd_partial")
    if nf < c:                    # padded channel stride: c-sized scratch vectors, sliced to num_features below
        wb = torch.empty((2, c), dtype=torch.float32, device=y.device)
        dw_ptr, db_ptr, accumulate = wb[0].data_ptr(), wb[1].data_ptr(), 0
    else:
        # the parameters' gradient is written, or added to when an earlier use of them in this pass holds the tensor already
        dweight, dw_ptr, accumulate = _grad_target(weight, (c,), y.device)
        dbias, db_ptr, acc_b = _grad_target(bias, (c,), y.device)
        if accumulate != acc_b:
            # one of the pair lost its first gradient tensor (see _grad_target): give both a fresh tensor
            dweight = torch.empty((c,), dtype=torch.float32, device=y.device)
            dbias = torch.empty((c,), dtype=torch.float32, device=y.device)
            dw_ptr, db_ptr, accumulate = dweight.data_ptr(), dbias.data_ptr(), 0
    dy = torch.empty_like(y)
    gsum = torch.empty((groups, 2, c), dtype=torch.float32, device=y.device)      # each group's own sums, read by its share of the apply
    if sync is not None and training:
        msg = torch.empty((groups, 2, c), dtype=torch.float64, device=y.device)        # sum g*xhat | sum g, every group in one message
        L.check(lib.dei2i_bn_sync_bwd_sums(groups, c, _p(partial), chunks, _p(msg), c_void_p(dw_ptr), c_void_p(db_ptr), accumulate, st),
                "bn_sync_bwd_sums")
        sync.exchange(msg)
        # (every rank holds the same number of rows: the global group is world x this process's pixels)
        L.check(lib.dei2i_bn_sync_bwd_apply(prec.code, groups, pixels, pixels * sync.world, c, _p(dout), _p(y), _p(a), _p(b), _p(mean),
                                            _p(rstd), act, _p(msg), _p(gsum), _p(dy), _stream()), "bn_sync_bwd_apply")
    else:
        L.check(lib.dei2i_bn_bwd_apply(prec.code, groups, pixels, c, _p(dout), _p(y), _p(a), _p(b), _p(mean), _p(rstd), act, 1 if training else 0,
                                       _p(partial), chunks, _p(gsum), c_void_p(dw_ptr), c_void_p(db_ptr), accumulate, _p(dy), st), "bn_bwd_apply")
    if nf < c:
        dweight, dbias = wb[0, :nf].clone(), wb[1, :nf].clone()
    return dy, dweight, dbias


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, weight, bias, res, running_mean, running_var, training: bool, momentum: float, eps: float, act: int,
                num_batches_tracked=None, want_stats: bool = False):
        _require_gpu(y, "batchnorm_act")
        prec = precision_of(y)
        y = y.contiguous()
        n, h, w, c = y.shape
        lib = _lib_for(y)
        dev = y.device
        groups = bn_groups if training else 1
        ctx.sync = bn_sync.current if training else None
        a, b, mean, rstd, nf = _bn_coefs(lib, y, prec, weight, bias, running_mean, running_var, training, momentum, eps,
                                         num_batches_tracked, groups, sync=ctx.sync)
        if res is not None:
            res = res.contiguous()
        xq = torch.empty(y.numel(), dtype=torch.uint8, device=dev) if _fp8_copy_wanted(prec, c) else None
        # the statistics records of the output in the same pass (an InstanceNorm / BatchNorm reads this tensor next)
        partial = _leave_stats(n, lib.dei2i_moments_chunks(h * w), c, dev) if (want_stats and fuse_norm and xq is None) else None
        # every group in one launch (grid.y = group; coefficient rows (groups, c))
        out = _affine_act(lib, prec, y, a, b, res, act, groups, stats=partial, xq=xq, xq_scale=FP8_ACT_SCALE)
        if xq is not None:
            _handover["_dei2i_fp8"] = xq
        ctx.prec, ctx.act, ctx.training, ctx.has_res = prec, act, training, res is not None
        ctx.params, ctx.nf = (weight, bias), nf
        ctx.save_for_backward(y, a, b, mean, rstd)
        ctx.hint = None
        if fuse_bwd and prec is BF16 and ctx.needs_input_grad[0]:
            ctx.hint = _NormBwdHint(2, y, mean, rstd, a=a, b=b, act=act, group_images=n // groups if groups > 1 else 0)
            _handover["_dei2i_bwd_hint"] = ctx.hint
        return out

    @staticmethod
    def backward(ctx, dout):
        y, a, b, mean, rstd = ctx.saved_tensors
        weight, bias = ctx.params
        dy, dweight, dbias = _bn_backward(_lib_for(y), ctx.prec, dout, y, a, b, mean, rstd, ctx.act, ctx.training, weight, bias, ctx.nf,
                                          hint=ctx.hint, sync=ctx.sync)
        return dy, dweight, dbias, (dout if ctx.has_res else None), None, None, None, None, None, None, None, None


def batchnorm_act(y, weight, bias, running_mean, running_var, training, act="none", res=None, momentum=0.1, eps=1e-5,
                  num_batches_tracked=None, stats=False):
    """num_batches_tracked: the module's int64 counter, incremented inside the statistics kernel in training mode.
    ``stats``: a norm layer reads the output next -- leave its statistics records with it (see _stats_of)."""
    _handover.clear()
    return _attach(_BatchNormAct.apply(y, weight, bias, res, running_mean, running_var, bool(training), float(momentum), float(eps),
                                       ACT[act], num_batches_tracked, bool(stats)))


class _BnActConv(torch.autograd.Function):
    """conv(act(BatchNorm(y1))) with the BatchNorm apply + activation on the conv's operand path (architecture.py:116-118
    followed by the next block's conv, e.g. the two halves of a ResBlock, architecture.py:139-156): the normalised tensor is
    never written -- forward, and the weight gradient in backward, re-normalise y1's halo tiles in LDS (ConvPro, csrc/geom.h)."""

    @staticmethod
    def forward(ctx, y1, bn_w, bn_b, weight, running_mean, running_var, training, momentum, eps, act, num_batches_tracked,
                cache: PackedWeights, sources, geom: ConvGeom, want_stats):
        prec = precision_of(y1)
        y1 = y1.contiguous()
        n, h, w, c = y1.shape
        lib = _lib_for(y1)
        ctx.sync = bn_sync.current if training else None
        a, b, mean, rstd, nf = _bn_coefs(lib, y1, prec, bn_w, bn_b, running_mean, running_var, training, momentum, eps,
                                         num_batches_tracked, sync=ctx.sync)
        couts = prec.pad(geom.cout)
        d = _desc(prec, geom, n, h, w, c, couts)
        cache, per_call, need_dgrad = _packing(weight, cache, sources)
        wf = cache.get(weight, sources, prec, geom, c, couts, need_dgrad=need_dgrad, per_call=per_call)[0]
        y = _conv_out(lib, d, n, couts, prec, y1.device)
        pro, _ = _bn_pro(a, b, act)
        partial = _leave_stats(n, lib.dei2i_conv2d_stats_chunks(byref(d)), couts, y1.device) if want_stats else None
        L.check(lib.dei2i_conv2d_fwd_fused(byref(d), _p(y1), _p(wf), None, L.ACT_NONE, _p(y), byref(pro), _p(partial), _stream()),
                "conv2d_fwd_fused(bn)")
        ctx.prec, ctx.act, ctx.training, ctx.nf, ctx.geom = prec, act, training, nf, geom
        ctx.cache, ctx.sources, ctx.params, ctx.per_call = cache, sources, (bn_w, bn_b), per_call
        ctx.save_for_backward(y1, a, b, mean, rstd, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        y1, a, b, mean, rstd, weight = ctx.saved_tensors
        prec, geom = ctx.prec, ctx.geom
        lib = _lib_for(y1)
        dy = dy.contiguous()
        dw = None
        if _wants_grad(ctx, 3):
            pro, keep = _bn_pro(a, b, ctx.act)
            dw = _conv_wgrad(lib, prec, geom, y1, dy, weight, pro, keep=keep)
        dy1 = dbw = dbb = None
        if _wants_grad(ctx, 0) or _wants_grad(ctx, 1) or _wants_grad(ctx, 2):
            hint = _NormBwdHint(2, y1, mean, rstd, a=a, b=b, act=ctx.act)
            dh = _conv_dgrad(lib, prec, geom, tuple(y1.shape), dy.shape[-1], dy, weight, ctx.cache, ctx.sources, ctx.per_call, y1.dtype,
                             y1.device, hint=hint)
            bn_w, bn_b = ctx.params
            dy1, dbw, dbb = _bn_backward(lib, prec, dh, y1, a, b, mean, rstd, ctx.act, ctx.training, bn_w, bn_b, ctx.nf, hint=hint,
                                         sync=ctx.sync)
        return (dy1, dbw, dbb, dw) + (None,) * 11


def bn_act_conv_supported(y1, bn_weight, weight, geom: ConvGeom, need_grad: bool) -> bool:
    """Can conv(act(BatchNorm(y1))) run with the norm on the conv's operand path?  (bf16, halo-resident forward kernel takes
    the shape, and -- when gradients are needed -- so does the halo-resident wgrad kernel; plain weights only)"""
    if not (fuse_norm and fuse_pro and y1.is_cuda and y1.dtype == torch.bfloat16 and not _fp8_forward) or bn_groups > 1:
        return False
    if getattr(weight, "_dei2i_per_call", False) or bn_weight.numel() != y1.shape[-1]:
        return False
    lib = _lib_for(y1)
    n, h, w, c = y1.shape
    d = _desc(BF16, geom, n, h, w, c, BF16.pad(geom.cout))
    if not lib.dei2i_conv2d_fused_supported(byref(d), 1):
        return False
    return bool(lib.dei2i_conv2d_wgrad_pro_supported(byref(d))) if need_grad else True


def bn_act_conv(y1, bn_weight, bn_bias, running_mean, running_var, training, act, weight, cache, geom, momentum=0.1, eps=1e-5,
                num_batches_tracked=None, sources=None, stats=False):
    """conv(act(BatchNorm2d(y1))), the norm + activation fused into the conv (ask bn_act_conv_supported first)."""
    _handover.clear()
    return _attach(_BnActConv.apply(y1, bn_weight, bn_bias, weight, running_mean, running_var, bool(training), float(momentum),
                                    float(eps), ACT[act], num_batches_tracked, cache, _sources(sources, weight), geom, bool(stats)))


def add(x, res, stats=False):
    """x + res on NHWC activations (NormResBlock identity branch, architecture.py:350).  ``stats``: a norm layer reads the
    sum next -- leave its statistics records with it."""
    c = x.shape[-1]
    _handover.clear()
    return _attach(_AffineAdd.apply(x, res, _const_vec(x.device, c, 1.0), _const_vec(x.device, c, 0.0), bool(stats)))


class _AffineAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, ones, zeros, want_stats=False):
        _require_gpu(x, "add")
        prec = precision_of(x)
        x, res = x.contiguous(), res.contiguous()
        lib = _lib_for(x)
        partial = None
        if want_stats and fuse_norm and x.dim() == 4:
            partial = _leave_stats(x.shape[0], lib.dei2i_moments_chunks(x.shape[1] * x.shape[2]), x.shape[-1], x.device)
        return _affine_act(lib, prec, x, ones, zeros, res, L.ACT_NONE, stats=partial, what="add")

    @staticmethod
    def backward(ctx, g):
        return g, g, None, None, None


# --------------------------------------------------------------------------------------------------------------
# SPADE (InstanceNorm * (1+gamma) + beta) + ReLU, optional fused nearest x2 upsample of x
# --------------------------------------------------------------------------------------------------------------
def _spade_backward(lib, prec, dout, dskip, x, gb, mean, rstd, up, gb_mode, out_shape, hint=None, slope=0.0, want_dgb=True):
    """-> (dx, dgb) of z = act(IN(x)*(1+gamma)+beta) given dL/dz at the (upsampled) output resolution -- the one backward of SPADE
    + ReLU (``slope`` 0), InstanceNorm + act and AdaIN / affine InstanceNorm + act (class mode on an all-zero / a replicated
    table; slope 0.2 LeakyReLU, 1 none).  dskip (optional) is added to dx inside the apply kernel (the res block's identity
    branch).  ``want_dgb`` False (class mode): no table gradient, dgb is None.  ``hint`` (SPADE only): the dgrad of the conv
    behind the layer may have left the reduction records already (_NormBwdHint); the 24 border classes of the table's gradient
    are then all that is left of the first pass."""
    st = _stream()
    dev = x.device
    have = hint.take(dout) if (hint is not None and gb_mode == 1) else None
    dout = dout.contiguous()
    n, h, w, c = out_shape
    dgb = torch.empty_like(gb) if want_dgb else None   # dense (N,H,W,2C), or the (N,5,5,2C) class table -- both written in full
    if have is not None:
        partial, chunks = have
        L.check(lib.dei2i_spade_bwd_border(prec.code, n, h, w, c, 1 if up else 0, _p(dout), _p(x), _p(mean), _p(rstd), _p(gb), slope,
                                           _p(dgb), st), "spade_bwd_border")
    else:
        chunks = lib.dei2i_moments_chunks(h * w)
        partial = torch.empty((n, chunks, 4, c), dtype=torch.float32, device=dev)
        L.check(lib.dei2i_spade_bwd_partial(prec.code, n, h, w, c, 1 if up else 0, _p(dout), _p(x), _p(mean), _p(rstd),
                                            _p(gb), gb_mode, slope, _p(dgb), _p(partial), st), "spade_bwd_partial")
    coef = torch.empty((n, 2, c), dtype=torch.float32, device=dev)
    dx = torch.empty_like(x)
    L.check(lib.dei2i_spade_bwd_apply(prec.code, n, h, w, c, 1 if up else 0, _p(dout), _p(x), _p(mean), _p(rstd), _p(gb), gb_mode, slope,
                                      _p(partial), chunks, _p(dgb) if gb_mode == 1 else None, _p(coef), _p(dskip), _p(dx), st),
            "spade_bwd_apply")
    return dx, dgb


class _SpadeRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gb, up: bool, gb_mode: int, eps: float, skip: bool = False):
        _require_gpu(x, "spade_relu")
        prec = precision_of(x)
        x, gb = _skip_forward("spade_relu", x, gb, skip, up)
        n, hs, ws, c = x.shape
        h, w = (hs * 2, ws * 2) if up else (hs, ws)
        lib = _lib_for(x)
        st = _stream()
        dev = x.device
        # statistics of the upsampled tensor == statistics of the source tensor (every pixel replicated 4x)
        mean, rstd = _in_stats(lib, prec, x, n, hs * ws, c, eps)
        out = torch.empty((n, h, w, c), dtype=prec.dtype, device=dev)
        xq = torch.empty(out.numel(), dtype=torch.uint8, device=dev) if _fp8_copy_wanted(prec, c) else None
        L.check(lib.dei2i_spade_act_fwd(prec.code, n, h, w, c, 1 if up else 0, _p(x), _p(mean), _p(rstd), _p(gb), gb_mode,
                                        _p(out), _p(xq), FP8_ACT_SCALE, st), "spade_act_fwd")
        if xq is not None:
            _handover["_dei2i_fp8"] = xq
        ctx.prec, ctx.up, ctx.gb_mode = prec, up, gb_mode
        ctx.out_shape = (n, h, w, c)
        ctx.save_for_backward(x, gb, mean, rstd)        # backward recomputes the ReLU mask; the output is not kept
        ctx.hint = None
        if fuse_bwd and gb_mode == 1 and prec is BF16 and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            ctx.hint = _NormBwdHint(1, x, mean, rstd, gb=gb, up=up)
            _handover["_dei2i_bwd_hint"] = ctx.hint
        return (out, x) if skip else out

    @staticmethod
    def backward(ctx, dout, dskip=None):
        x, gb, mean, rstd = ctx.saved_tensors
        if dout is None:                                 # only the identity branch was used
            return (dskip,) + (None,) * 5
        dx, dgb = _spade_backward(_lib_for(x), ctx.prec, dout, _skip_backward("spade_relu", dskip, x), x, gb, mean, rstd, ctx.up,
                                  ctx.gb_mode, ctx.out_shape, hint=ctx.hint)
        return dx, dgb, None, None, None, None


def spade_relu(x, gb, up: bool, gb_mode: int, eps: float = 1e-5, skip: bool = False):
    """relu(IN(x) * (1 + gamma) + beta); with ``skip`` -> (that, x): x handed through for the res block's identity add."""
    _handover.clear()
    return _attach_skip(_SpadeRelu.apply(x, gb, bool(up), int(gb_mode), float(eps), bool(skip)), skip)


class _SpadeConv(torch.autograd.Function):
    """conv(relu(SPADE(up(x)))) -- architecture.py:241-245 (NormConvBlock) and :343-350 (NormResBlock) with
    normalization.py:24-37 -- for the constant-label-map case (class table, gb_mode 1), the InstanceNorm apply + modulate +
    ReLU (+ nearest x2 upsample) on the conv's operand path: one small preparation kernel (statistics finalize, interior
    coefficients, the 2-pixel frame's values) and the conv; the normalised tensor is never written.  Backward: the input
    gradient of the conv at the logical resolution, the weight gradient with the same operand-path transform, then the
    SPADE backward kernels of the unfused op."""

    @staticmethod
    def forward(ctx, x, gb, weight, up, eps, skip, cache: PackedWeights, sources, geom: ConvGeom, want_stats, ring_mode=False):
        # ring_mode (up only): instead of normalising on the conv's operand path, write z at the SOURCE resolution with the
        # interior-class coefficients (one elementwise pass over the small tensor) and let the conv read it through its fused
        # upsample, the logical frame's pixels from the ring tensor -- see fuse_ring
        prec = precision_of(x)
        x, gb = _skip_forward("spade_conv", x, gb, skip, up)
        n, hs, ws, c = x.shape
        h, w = (hs * 2, ws * 2) if up else (hs, ws)
        lib = _lib_for(x)
        st = _stream()
        dev = x.device
        partial, chunks = _moment_records(lib, prec, x, n, hs * ws, c)
        coefs = torch.empty((4, n, c), dtype=torch.float32, device=dev)          # mean | rstd | A | B
        ring = torch.empty((n, lib.dei2i_ring_pixels(h, w), c), dtype=prec.dtype, device=dev)
        L.check(lib.dei2i_spade_prep(prec.code, n, hs, ws, c, 1 if up else 0, _p(x), _p(partial), chunks, eps, _p(gb),
                                     _p(coefs[0]), _p(coefs[1]), _p(coefs[2]), _p(coefs[3]), _p(ring), st), "spade_prep")
        couts = prec.pad(geom.cout)
        d = _desc(prec, geom, n, hs, ws, c, couts)
        cache, per_call, need_dgrad = _packing(weight, cache, sources)
        wf = cache.get(weight, sources, prec, geom, c, couts, need_dgrad=need_dgrad, per_call=per_call)[0]
        y = torch.empty((n, h, w, couts), dtype=prec.dtype, device=dev)
        out_partial = _leave_stats(n, lib.dei2i_conv2d_stats_chunks(byref(d)), couts, dev) if want_stats else None
        z_src = None
        if ring_mode:
            z_src = torch.empty_like(x)
            L.check(lib.dei2i_affine_act_img_fwd(prec.code, n, hs * ws, c, _p(x), _p(coefs[2]), _p(coefs[3]), 0.0, _p(z_src), st),
                    "affine_act_img")
            L.check(lib.dei2i_conv2d_fwd_ring(byref(d), _p(z_src), _p(ring), _p(wf), None, L.ACT_NONE, _p(y), _p(out_partial), st),
                    "conv2d_fwd_ring")
        else:
            pro, _ = _spade_pro(coefs, ring, c)
            L.check(lib.dei2i_conv2d_fwd_fused(byref(d), _p(x), _p(wf), None, L.ACT_NONE, _p(y), byref(pro), _p(out_partial), st),
                    "conv2d_fwd_fused(spade)")
        ctx.prec, ctx.up, ctx.geom, ctx.cache, ctx.sources, ctx.ring_mode, ctx.per_call = prec, up, geom, cache, sources, ring_mode, per_call
        ctx.out_shape = (n, h, w, c)
        ctx.save_for_backward(x, gb, coefs, ring, weight, z_src)
        return (y, x) if skip else y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, gb, coefs, ring, weight, z_src = ctx.saved_tensors
        prec, geom, up = ctx.prec, ctx.geom, ctx.up
        if dy is None:                                   # only the identity branch was used
            return (dskip,) + (None,) * 10
        lib = _lib_for(x)
        dy = dy.contiguous()
        n, h, w, c = ctx.out_shape
        dskip = _skip_backward("spade_conv", dskip, x)
        dw = None
        if _wants_grad(ctx, 2):
            # (ring mode: the conv's input was z_src (+ ring) -- no transform in the wgrad)
            pro, keep = _spade_pro(coefs, ring, c, ctx.ring_mode)
            dw = _conv_wgrad(lib, prec, geom, z_src if ctx.ring_mode else x, dy, weight, pro, keep=keep)
        dx = dgb = None
        if _wants_grad(ctx, 0) or _wants_grad(ctx, 1):
            # dL/dz at the LOGICAL (upsampled) resolution: the conv seen as a plain conv on z (the SPADE backward sums the
            # 2x2 cells itself, and needs the per-logical-pixel mask and class)
            g_log = ConvGeom(geom.cin, geom.cout, geom.k, geom.stride, geom.pad, geom.reflect, False)
            hint = _NormBwdHint(1, x, coefs[0], coefs[1], gb=gb, up=up)
            dz = _conv_dgrad(lib, prec, g_log, (n, h, w, c), dy.shape[-1], dy, weight, ctx.cache, ctx.sources, ctx.per_call, x.dtype,
                             x.device, hint=hint)
            dx, dgb = _spade_backward(lib, prec, dz, dskip, x, gb, coefs[0], coefs[1], up, 1, ctx.out_shape, hint=hint)
        elif dskip is not None:
            dx = dskip
        return (dx, dgb, dw) + (None,) * 8


def spade_conv_supported(x, weight, geom: ConvGeom, need_grad: bool):
    """How can conv(relu(SPADE(up(x)))) run fused?  -> "pro" (the norm on the conv's operand path: fuse_pro), "ring" (upsampling
    blocks: z at the source resolution + the frame's ring tensor: fuse_ring) or None.  ``geom`` carries the upsample flag."""
    if not (fuse_norm and x.is_cuda and x.dtype == torch.bfloat16 and not _fp8_forward):
        return None
    lib = _lib_for(x)
    n, hs, ws, c = x.shape
    d = _desc(BF16, geom, n, hs, ws, c, BF16.pad(geom.cout))
    wg_ok = (not need_grad) or bool(lib.dei2i_conv2d_wgrad_pro_supported(byref(d)))
    if fuse_pro and wg_ok and lib.dei2i_conv2d_fused_supported(byref(d), 1):
        return "pro"
    if fuse_ring and geom.up and wg_ok and lib.dei2i_conv2d_ring_supported(byref(d)):
        return "ring"
    return None


def spade_conv(x, gb, weight, cache, geom: ConvGeom, eps: float = 1e-5, skip: bool = False, sources=None, stats=False, mode="pro"):
    """conv(relu(IN(up(x)) * (1 + gamma) + beta)) with the class table ``gb`` (N,5,5,2C); ``geom.up`` = nearest x2 upsample in
    front of the norm.  With ``skip`` -> (y, x).  ``mode``: what spade_conv_supported answered."""
    _handover.clear()
    return _attach_skip(_SpadeConv.apply(x, gb, weight, bool(geom.up), float(eps), bool(skip), cache, _sources(sources, weight), geom,
                                         bool(stats), mode == "ring"), skip)


# --------------------------------------------------------------------------------------------------------------
# InstanceNorm2d(affine=False) + activation, AvgPool2d(2, 2): the blocks of the conv StyleExtractor (extractor.py:50-80)
# --------------------------------------------------------------------------------------------------------------
_zero_tables = {}


def _zero_table(device, dtype, n, c):
    key = (torch.device(device), dtype, n, c)
    t = _zero_tables.get(key)
    if t is None:
        if len(_zero_tables) > 16:
            _zero_tables.clear()
        t = _zero_tables[key] = torch.zeros((n, 5, 5, 2 * c), dtype=dtype, device=device)
    return t


class _InstanceNormAct(torch.autograd.Function):
    """z = act(InstanceNorm2d(x)), affine=False, eps 1e-5 (architecture.py:79-118 with norm_layer=nn.InstanceNorm2d): per-(n, c)
    statistics (the producer's records when it left any), then one affine + activation pass with per-image coefficients
    A = rstd, B = -mean * rstd.  ``slope``: 0.2 LeakyReLU, 0 ReLU, 1 none.  Backward: the SPADE backward (_spade_backward) in class
    mode on an all-zero table, no table gradient; ``res`` (optional) is added to the output and its gradient passed through."""

    @staticmethod
    def forward(ctx, x, slope: float, res, eps: float):
        _require_gpu(x, "instance_norm_act")
        prec = precision_of(x)
        x = x.contiguous()
        n, h, w, c = x.shape
        lib = _lib_for(x)
        mean, rstd = _in_stats(lib, prec, x, n, h * w, c, eps)
        out = _img_affine_act(lib, prec, x, rstd, -mean * rstd, slope)
        if res is not None:
            out = out + res
        ctx.prec, ctx.slope, ctx.has_res = prec, slope, res is not None
        ctx.save_for_backward(x, mean, rstd)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, mean, rstd = ctx.saved_tensors
        n, c = x.shape[0], x.shape[3]
        dx, _ = _spade_backward(_lib_for(x), ctx.prec, dout, None, x, _zero_table(x.device, x.dtype, n, c), mean, rstd, False, 1,
                                tuple(x.shape), slope=ctx.slope, want_dgb=False)
        return dx, None, (dout if ctx.has_res else None), None


def instance_norm_act(x, act="none", res=None, eps=1e-5):
    """act(InstanceNorm2d(x)) (+ res) on an NHWC activation with H, W >= 4; act: "none" | "relu" | "leaky_relu" """
    return _InstanceNormAct.apply(x, ACT_SLOPE[ACT[act or "none"]], res, float(eps))


# ---- SPADE's label path, second stage, batched over the modules of a generator (csrc/label_path.hip) ---------------------------
def label_gamma_beta_supported(actv, hidden: int, convs) -> bool:
    """Can ``label_gamma_beta`` take these modules?  (bf16, <= 16 modules, hidden a multiple of 32 up to 128, every norm_nc a multiple
    of 16, plain convs with a bias)"""
    if not (actv.is_cuda and actv.dtype == torch.bfloat16 and actv.dim() == 4 and tuple(actv.shape[1:3]) == (5, 5)):
        return False
    if not (1 <= len(convs) <= 16 and hidden % 32 == 0 and 32 <= hidden <= 128 and actv.shape[-1] == hidden * len(convs)):
        return False
    for g, b in convs:
        if g.bias is None or b.bias is None or g.weight.shape != b.weight.shape or tuple(g.weight.shape[1:]) != (hidden, 3, 3):
            return False
        if g.weight.shape[0] % 16 != 0 or g.weight.dtype != torch.float32 or getattr(g.weight, "_dei2i_per_call", False):
            return False
    return True


class _LabelGammaBeta(torch.autograd.Function):
    """(gamma | beta tables of every module) = conv3x3(actv slice; mlp_gamma | mlp_beta) + bias, all modules in one launch per direction
    (normalization.py:20-22,33-35 on the 5 x 5 class image).  actv: (N, 5, 5, modules * hidden), module i reads channels
    [i * hidden, (i + 1) * hidden).  params: (gamma.weight, gamma.bias, beta.weight, beta.bias) per module."""

    @staticmethod
    def forward(ctx, actv, hidden, cache, *params):
        _require_gpu(actv, "label_gamma_beta")
        actv = actv.contiguous()
        n_img, _, _, ctot = actv.shape
        nmod = len(params) // 4
        lib, st, dev = _lib_for(actv), _stream(), actv.device
        stamps = tuple(PackedWeights._stamp(params[4 * i + k]) for i in range(nmod) for k in (0, 2))
        if cache.get("stamps") != stamps:               # filters moved (an optimizer step): both bf16 layouts of every module, one launch
            cache["packed"] = [(torch.empty(lib.dei2i_label_gb_packed_elems(params[4 * i].shape[0], hidden), dtype=torch.bfloat16, device=dev),
                                torch.empty(lib.dei2i_label_gb_packed_elems(params[4 * i].shape[0], hidden), dtype=torch.bfloat16, device=dev))
                               for i in range(nmod)]
            cache["stamps"] = None
        packed = cache["packed"]
        mods = (L.LabelMod * nmod)()
        outs = []
        for i in range(nmod):
            gw, gbias, bw, bbias = (t.detach() for t in params[4 * i:4 * i + 4])
            c = gw.shape[0]
            gb = torch.empty((n_img, 5, 5, 2 * c), dtype=torch.bfloat16, device=dev)
            outs.append(gb)
            mods[i] = L.LabelMod(gw.data_ptr(), bw.data_ptr(), gbias.data_ptr(), bbias.data_ptr(), packed[i][0].data_ptr(),
                                 packed[i][1].data_ptr(), gb.data_ptr(), None, None, None, None, c, i * hidden, 1, 0)
        if cache["stamps"] is None:
            L.check(lib.dei2i_label_gb_pack(mods, nmod, hidden, st), "label_gb_pack")
            cache["stamps"] = stamps
        L.check(lib.dei2i_label_gb_fwd(mods, nmod, hidden, ctot, n_img, _p(actv), st), "label_gb_fwd")
        ctx.hidden, ctx.packed, ctx.nmod = hidden, packed, nmod
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(actv, *params)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dgbs):
        actv, *params = ctx.saved_tensors
        hidden, nmod = ctx.hidden, ctx.nmod
        n_img, _, _, ctot = actv.shape
        lib, st, dev = _lib_for(actv), _stream(), actv.device
        mods = (L.LabelMod * nmod)()
        grads, keep = [], []
        for i in range(nmod):
            c = params[4 * i].shape[0]
            g = dgbs[i]
            if g is not None:
                g = g.contiguous()
                if g.dtype != torch.bfloat16 or tuple(g.shape) != (n_img, 5, 5, 2 * c):
                    raise RuntimeError("label_gamma_beta: the table gradient does not match the table")
                keep.append(g)
            dgw, dbw = torch.empty_like(params[4 * i]), torch.empty_like(params[4 * i + 2])
            dgbias, dbbias = torch.empty_like(params[4 * i + 1]), torch.empty_like(params[4 * i + 3])
            grads += [dgw, dgbias, dbw, dbbias]
            mods[i] = L.LabelMod(None, None, None, None, ctx.packed[i][0].data_ptr(), ctx.packed[i][1].data_ptr(),
                                 g.data_ptr() if g is not None else None, dgw.data_ptr(), dbw.data_ptr(), dgbias.data_ptr(), dbbias.data_ptr(),
                                 c, i * hidden, 1 if g is not None else 0, 0)
        dactv = None
        if ctx.needs_input_grad[0]:
            dactv = torch.empty_like(actv)
            L.check(lib.dei2i_label_gb_dgrad(mods, nmod, hidden, ctot, n_img, _p(dactv), st), "label_gb_dgrad")
        L.check(lib.dei2i_label_gb_wgrad(mods, nmod, hidden, ctot, n_img, _p(actv), st), "label_gb_wgrad")
        # (a module whose table got no gradient -- it did not run in this loss graph -- hands None to its filters, like the unfused graph)
        return (dactv, None, None) + tuple(gr if (ctx.needs_input_grad[3 + k] and dgbs[k // 4] is not None) else None
                                           for k, gr in enumerate(grads))


def label_gamma_beta(actv, hidden: int, convs, cache: dict):
    """-> [(N, 5, 5, 2 * norm_nc) gamma | beta table per module]; ``convs``: (mlp_gamma, mlp_beta) conv modules per SPADE module, in the
    order of their channel slices in ``actv``; ``cache``: a dict the caller keeps (the packed filters live there between steps)."""
    params = []
    for g, b in convs:
        params += [g.weight, g.bias, b.weight, b.bias]
    return list(_LabelGammaBeta.apply(actv, int(hidden), cache, *params))


class _SplitRows(torch.autograd.Function):
    """x -> consecutive row blocks of x (views, sizes given): what ``x[a:b]`` per block does, with ONE launch in backward (the
    concatenation of the blocks' gradients) instead of a zero fill + a copy per block and an add per extra block."""

    @staticmethod
    def forward(ctx, x, *sizes):
        ctx.set_materialize_grads(False)
        ctx.sizes, ctx.meta = sizes, (x.shape, x.dtype, x.device)
        outs, off = [], 0
        for n in sizes:
            outs.append(x.narrow(0, off, n))
            off += n
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        shape, dtype, device = ctx.meta
        if all(g is None for g in grads):
            return (None,) + (None,) * len(ctx.sizes)
        parts = [g if g is not None else torch.zeros((n,) + tuple(shape[1:]), dtype=dtype, device=device)
                 for g, n in zip(grads, ctx.sizes)]
        return (torch.cat(parts, 0),) + (None,) * len(ctx.sizes)


def split_rows(x, sizes):
    """The consecutive row blocks of ``x`` (dim 0) as views; see _SplitRows."""
    if sum(sizes) != x.shape[0]:
        raise ValueError(f"split_rows: blocks {list(sizes)} do not cover {x.shape[0]} rows")
    if not x.requires_grad or not torch.is_grad_enabled():
        return tuple(x.split(list(sizes), 0))
    return _SplitRows.apply(x, *[int(n) for n in sizes])


class _Scale(torch.autograd.Function):
    """x * s on an NHWC activation (stargan-v2's "/ sqrt(2)" after every residual add, core/model.py:67,121)"""

    @staticmethod
    def forward(ctx, x, s: float):
        _require_gpu(x, "scale")
        ctx.s = s
        return _affine_act(_lib_for(x), precision_of(x), x.contiguous(), float(s), 0.0, None, L.ACT_NONE, what="scale")

    @staticmethod
    def backward(ctx, g):
        return _Scale.apply(g, ctx.s), None


def scale(x, s: float):
    return _Scale.apply(x, float(s))


class _Act(torch.autograd.Function):
    """a stand-alone activation of the ReLU family on an NHWC activation (stargan-v2 applies LeakyReLU(0.2) to a tensor whose
    un-activated value also feeds the block's shortcut, core/model.py:52-63)"""

    @staticmethod
    def forward(ctx, x, act: int):
        _require_gpu(x, "act")
        out = _affine_act(_lib_for(x), precision_of(x), x.contiguous(), 1.0, 0.0, None, act, what="act")
        ctx.act = act
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        return _ActBwd.apply(g.contiguous(), out, ctx.act), None


def leaky_relu(x):
    return _Act.apply(x, L.ACT_LRELU)


class _InAffineAct(torch.autograd.Function):
    """z = act(InstanceNorm2d(x) * (1 + gamma) + beta), gamma / beta (N, C) fp32 -- stargan-v2's AdaIN (core/model.py:69-80) and its
    InstanceNorm2d(affine=True) (gamma = weight - 1, beta = bias for every image) with the LeakyReLU(0.2) that follows both at every
    call site (model.py:53-61,104-112,333-334).  Forward: statistics -> per-image coefficients A = rstd (1 + gamma), B = beta - mean A
    -> one affine + activation pass.  Backward: the SPADE backward (_spade_backward) in class mode on the replicated table with the
    activation's slope; the table's 25 classes are summed back to (N, C).  gamma / beta are rounded to the compute dtype first, so
    that forward and backward see the same values."""

    @staticmethod
    def forward(ctx, x, gamma, beta, slope: float, eps: float):
        _require_gpu(x, "in_affine_act")
        prec = precision_of(x)
        x = x.contiguous()
        n, h, w, c = x.shape
        lib = _lib_for(x)
        dev = x.device
        cl = gamma.shape[1]
        gb = torch.zeros((n, 2 * c), dtype=prec.dtype, device=dev)
        gb[:, :cl] = gamma.detach().to(prec.dtype)
        gb[:, c:c + cl] = beta.detach().to(prec.dtype)
        mean, rstd = _in_stats(lib, prec, x, n, h * w, c, eps)
        a = rstd * (1.0 + gb[:, :c].float())
        b = gb[:, c:].float() - mean * a
        out = _img_affine_act(lib, prec, x, a, b, slope)
        ctx.prec, ctx.slope, ctx.cl = prec, slope, cl
        ctx.save_for_backward(x, mean, rstd, gb)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, mean, rstd, gb = ctx.saved_tensors
        n, h, w, c = x.shape
        if h < 4 or w < 4:
            raise NotImplementedError("in_affine_act backward needs H, W >= 4 (class-mode SPADE kernels)")
        table = gb.view(n, 1, 1, 2 * c).expand(n, 5, 5, 2 * c).contiguous()
        dx, dtable = _spade_backward(_lib_for(x), ctx.prec, dout, None, x, table, mean, rstd, False, 1, tuple(x.shape), slope=ctx.slope)
        dgb = dtable.float().sum(dim=(1, 2))              # (N, 2C): the 25 classes hold the same (gamma | beta)
        return dx, dgb[:, :ctx.cl], dgb[:, c:c + ctx.cl], None, None


def in_affine_act(x, gamma, beta, act="leaky_relu", eps=1e-5):
    """act(InstanceNorm2d(x) * (1 + gamma) + beta) on an NHWC activation; gamma / beta: (N, C) fp32 (autograd flows into them)"""
    return _InAffineAct.apply(x, gamma, beta, ACT_SLOPE[ACT[act or "none"]], float(eps))


class _AvgPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, "avgpool2")
        x = x.contiguous()
        n, h, w, c = x.shape
        out = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
        L.check(_lib_for(x).dei2i_avgpool2_fwd(precision_of(x).code, n, h, w, c, _p(x), _p(out), _stream()), "avgpool2_fwd")
        ctx.shape = (n, h, w, c)
        return out

    @staticmethod
    def backward(ctx, dout):
        if _second_order(dout):
            return _AvgPool2Bwd.apply(dout, ctx.shape)
        return _avgpool2_bwd(dout, ctx.shape)


def _avgpool2_bwd(dout, shape):
    """-> the (N, H, W, C) = ``shape`` input gradient of the average pool: each value of ``dout`` / 4 to its 2x2 cell"""
    n, h, w, c = shape
    dout = dout.contiguous()
    dx = torch.empty(shape, dtype=dout.dtype, device=dout.device)
    L.check(_lib_for(dout).dei2i_avgpool2_bwd(precision_of(dout).code, n, h, w, c, _p(dout), _p(dx), _stream()), "avgpool2_bwd")
    return dx


class _AvgPool2Bwd(torch.autograd.Function):
    """the average pool's input gradient as a function of the output gradient (_avgpool2_bwd); transpose: the pool"""

    @staticmethod
    def forward(ctx, dout, shape):
        return _avgpool2_bwd(dout, shape)

    @staticmethod
    def backward(ctx, gdx):
        return _AvgPool2.apply(gdx), None


def avgpool2(x):
    """nn.AvgPool2d(2, 2) on an NHWC activation (H, W even)"""
    return _AvgPool2.apply(x)


def upsample2(x):
    """nearest x2 upsample of an NHWC activation that no conv absorbs (stargan-v2's AdainResBlk shortcut when the channel count does not
    change, core/model.py:101-105): the average pool's adjoint spreads a value / 4 over its 2x2 cell, so this is 4 x that kernel"""
    n, h, w, c = x.shape
    return scale(_AvgPool2Bwd.apply(x, (n, 2 * h, 2 * w, c)), 4.0)


# --------------------------------------------------------------------------------------------------------------
# DiffAugment (utils/diffaug.py) as fused HIP kernels (csrc/diffaug.hip): one affine operator per sample and canonical-order policy
# run; its input gradient is the adjoint, whose own gradient is the forward's linear part -- differentiable to any order (the R1
# penalty of stargan-v2 differentiates D(DiffAugment(x)) with respect to x with create_graph=True).  No image is saved: the
# per-sample parameter table and the run's flags are all either direction needs.
# --------------------------------------------------------------------------------------------------------------
def _diffaug_run(x, tab, run, mode: int):
    color, ch, cw = run
    x = x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    lib = _lib_for(x)
    partial = torch.empty(lib.dei2i_diffaug_partial_floats(n), dtype=torch.float32, device=x.device) if color else None
    L.check(lib.dei2i_diffaug(mode, n, c, h, w, ch, cw, int(color), _p(x), _p(tab), _p(partial), _p(out), _stream()), "diffaug")
    return out


class _DiffAug(torch.autograd.Function):
    """mode 0: y = Cut Trans (L x + beta); mode 1: its linear part (beta = 0)"""

    @staticmethod
    def forward(ctx, x, tab, run, mode, host):
        ctx.tab, ctx.run, ctx.host = tab, run, host       # (host: the pinned source of tab's upload, alive while the graph is)
        return _diffaug_run(x, tab, run, mode)

    @staticmethod
    def backward(ctx, g):
        return _DiffAugAdjoint.apply(g, ctx.tab, ctx.run), None, None, None, None


class _DiffAugAdjoint(torch.autograd.Function):
    """the input gradient L Trans^T Cut g; linear in g, its transpose is the forward's linear part"""

    @staticmethod
    def forward(ctx, g, tab, run):
        ctx.tab, ctx.run = tab, run
        return _diffaug_run(g, tab, run, 2)

    @staticmethod
    def backward(ctx, gg):
        return _DiffAug.apply(gg, ctx.tab, ctx.run, 1, None), None, None


# The blit runs (flip -> rot90, csrc/blit.hip): a permutation of the pixels per sample, whose input gradient is the inverse
# permutation of the output gradient and whose own gradient is the forward again -- exact to any order.  Nothing is saved but the codes.
def _blit_run(x, codes, inverse: int):
    x = x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    L.check(_lib_for(x).dei2i_blit(n, c, h, w, _p(codes), inverse, _p(x), _p(out), _stream()), "blit")
    return out


class _Blit(torch.autograd.Function):
    """y = B x, B the sample's dihedral element"""

    @staticmethod
    def forward(ctx, x, codes, host):
        ctx.codes, ctx.host = codes, host                  # (host: the pinned source of the codes' upload, alive while the graph is)
        return _blit_run(x, codes, 0)

    @staticmethod
    def backward(ctx, g):
        return _BlitInverse.apply(g, ctx.codes), None, None


class _BlitInverse(torch.autograd.Function):
    """B^T g = B^-1 g; its transpose is the forward"""

    @staticmethod
    def forward(ctx, g, codes):
        ctx.codes = codes
        return _blit_run(g, codes, 1)

    @staticmethod
    def backward(ctx, gg):
        return _Blit.apply(gg, ctx.codes, None), None


# The warp runs (scale -> rotate -> aniso, csrc/warp.hip): one bilinear resampling per sample, a linear map whose input gradient is
# its transpose applied to the output gradient -- a gather with the forward's own weights, no atomics -- and whose own gradient is the
# forward again: differentiable to any order and bit-reproducible.  Nothing is saved but the record table.
def _warp_run(x, tab, adjoint: int):
    x = x.contiguous()
    if x.dtype != torch.float32:
        x = x.float()
    n, c, h, w = x.shape
    out = torch.empty_like(x)
    L.check(_lib_for(x).dei2i_warp(n, c, h, w, _p(tab), adjoint, _p(x), _p(out), _stream()), "warp")
    return out


class _Warp(torch.autograd.Function):
    """y = W x, W the sample's bilinear resampling matrix"""

    @staticmethod
    def forward(ctx, x, tab, host):
        ctx.tab, ctx.host = tab, host                      # (host: the pinned source of the table's upload, alive while the graph is)
        return _warp_run(x, tab, 0)

    @staticmethod
    def backward(ctx, g):
        return _WarpAdjoint.apply(g, ctx.tab), None, None


class _WarpAdjoint(torch.autograd.Function):
    """W^T g; its transpose is the forward"""

    @staticmethod
    def forward(ctx, g, tab):
        ctx.tab = tab
        return _warp_run(g, tab, 1)

    @staticmethod
    def backward(ctx, gg):
        return _Warp.apply(gg, ctx.tab, None), None


# Data-parallel stargan-v2 (stargan.Solver under parallel.attach_ddp): each rank holds rows [rank * n, (rank + 1) * n) of the global
# batch, and the reference augments the whole global batch with one draw per function.  Inside ``diffaug_sharded(rank, world)`` the
# draws are those of the global batch (utils.diffaug.draw_params(shard=...)) and only the rank's rows are uploaded and applied.
diffaug_shard = None


class diffaug_sharded(_GlobalScope):
    var = "diffaug_shard"

    def __init__(self, rank: int, world: int):
        self.value = (int(rank), int(world))


# Device-drawn parameters.  The host path above draws from the global CPU RNG and uploads per call, which a captured step would
# freeze into every replay.  ``DiffAugRng`` is a counter-based generator instead (Philox4x32-10, csrc/diffaug.hip
# dei2i_diffaug_draw): the seed travels in the kernel arguments, the call count is one word of device memory that every draw launch
# advances itself, and a record is a pure function of (seed, call, run, global row) -- an eager call and a replay of its capture
# draw the same table, every replay a new one, and a rank's rows are the slice of the global batch's table without any broadcast.
class DeviceRng:
    """The seed and the device call counter of ``diff_augment(..., rng=...)`` and of ``mask_draw`` (one instance each: a draw launch
    of either advances its own counter).  The counter is allocated here, outside any capture, and must outlive every graph that
    recorded a draw on it.  ``state()`` / ``set_state()`` synchronise: not for use inside a step."""

    def __init__(self, seed: int, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceRng draws on the GPU; device {self.device} is not one (there is no CPU fallback)")
        self.seed = int(seed) & (2 ** 64 - 1)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)      # (the bits of one unsigned 64-bit word)
        self.device = self.counter.device                    # (with its index)

    def state(self):
        """-> (seed, number of draw launches so far)"""
        return self.seed, int(self.counter.item()) & (2 ** 64 - 1)

    def set_state(self, state):
        seed, calls = state
        calls = int(calls) & (2 ** 64 - 1)
        self.seed = int(seed) & (2 ** 64 - 1)
        torch.cuda.synchronize(self.device)                  # (draws queued on any stream read the old count)
        self.counter.fill_(calls - 2 ** 64 if calls >= 2 ** 63 else calls)
        torch.cuda.synchronize(self.device)


DiffAugRng = DeviceRng          # (the name it was introduced under)


def _gate_word(p, device, what):
    """``p`` of the gated draw: a one-element fp32 tensor on ``device`` (the launch reads it there)"""
    if not isinstance(p, torch.Tensor) or p.numel() != 1 or p.dtype != torch.float32 or p.device != device or not p.is_contiguous():
        raise ValueError(f"{what}: p is a one-element fp32 tensor on {device} (the draw launch reads it from device memory)")
    return p


def _run_kind(names):
    """utils.diffaug.BLIT / WARP for a run of those kinds, None for a color / translation / cutout run"""
    from .utils.diffaug import BLIT, WARP, is_blit_run, is_warp_run
    return BLIT if is_blit_run(names) else WARP if is_warp_run(names) else None


def diffaug_draw(rng: DiffAugRng, policy, n, h, w, row0=0, p=None):
    """One dei2i_diffaug_draw launch on the current stream: -> (tab, runs), ``tab`` a device int32 (len(runs), n, 8) table of struct
    dei2i_diffaug_rec for global rows [row0, row0 + n), ``runs`` the (has_color, cut_h, cut_w) list of utils.diffaug.draw_params.
    Nothing is read from the host RNG and nothing is uploaded.  ``p`` (a one-element fp32 device tensor in [0, 1]): the gated
    draw dei2i_diffaug_draw_p instead -- each policy applies to a row with probability ``p``, read on the device by the launch.
    A policy with blit runs (flip -> rot90): ``runs`` holds ``utils.diffaug.BLIT`` at their places and ``tab`` the records of the
    other runs in order (``None``, and no launch, when there is none); ``blit_draw`` draws the codes, after this call.  Warp runs
    (scale -> rotate -> aniso) alike: ``utils.diffaug.WARP`` at their places, their records drawn by ``warp_draw``, after both."""
    from .utils.diffaug import REC_FIELDS, check_policy, policy_runs
    check_policy(policy, h, w)
    whole = policy_runs(policy)
    if not 0 < len(whole) <= L.DIFFAUG_MAX_RUNS:
        raise ValueError(f"diff_augment with a device RNG takes 1..{L.DIFFAUG_MAX_RUNS} canonical-order runs; {policy!r} has {len(whole)}")
    names = [run for run in whole if _run_kind(run) is None]
    bit = {"color": L.DIFFAUG_COLOR, "translation": L.DIFFAUG_TRANSLATION, "cutout": L.DIFFAUG_CUTOUT}
    flags, runs = 0, []
    for r, run in enumerate(names):
        flags |= sum(bit[name] for name in run) << (3 * r)
        cut = "cutout" in run
        runs.append(("color" in run, int(h * 0.5 + 0.5) if cut else 0, int(w * 0.5 + 0.5) if cut else 0))
    affine = iter(runs)
    runs = [_run_kind(run) or next(affine) for run in whole]
    if not names:
        return None, runs
    tab = torch.empty((len(names), n, REC_FIELDS), dtype=torch.int32, device=rng.device)
    lib = _lib_for(tab)
    if p is None:
        L.check(lib.dei2i_diffaug_draw(rng.seed, _p(rng.counter), len(names), flags, n, int(row0), h, w, _p(tab), _stream()), "diffaug_draw")
    else:
        L.check(lib.dei2i_diffaug_draw_p(rng.seed, _p(rng.counter), len(names), flags, n, int(row0), h, w,
                                         _p(_gate_word(p, rng.device, "diffaug_draw")), _p(tab), _stream()), "diffaug_draw_p")
    return tab, runs


def blit_draw(rng: DiffAugRng, policy, n, row0=0, p=None):
    """One dei2i_blit_draw launch on the current stream: -> a device int32 (blit runs, n) table, row b the codes f | k << 1 of the
    b-th blit run of ``policy`` for global rows [row0, row0 + n) (the counter-word layout: include/dei2i_hip.h -- the run word is the
    run's index in the whole list).  ``p``: the gated draw dei2i_blit_draw_p.  A policy without a blit run raises ValueError."""
    from .utils.diffaug import is_blit_run, policy_runs
    whole = policy_runs(policy)
    if not 0 < len(whole) <= L.DIFFAUG_MAX_RUNS:
        raise ValueError(f"diff_augment with a device RNG takes 1..{L.DIFFAUG_MAX_RUNS} canonical-order runs; {policy!r} has {len(whole)}")
    bit = {"flip": L.BLIT_FLIP, "rot90": L.BLIT_ROT90}
    flags = count = 0
    for r, run in enumerate(whole):
        if is_blit_run(run):
            flags |= sum(bit[name] for name in run) << (2 * r)
            count += 1
    if not count:
        raise ValueError(f"blit_draw: {policy!r} holds no flip or rot90")
    codes = torch.empty((count, n), dtype=torch.int32, device=rng.device)
    lib = _lib_for(codes)
    if p is None:
        L.check(lib.dei2i_blit_draw(rng.seed, _p(rng.counter), len(whole), flags, n, int(row0), _p(codes), _stream()), "blit_draw")
    else:
        L.check(lib.dei2i_blit_draw_p(rng.seed, _p(rng.counter), len(whole), flags, n, int(row0),
                                      _p(_gate_word(p, rng.device, "blit_draw")), _p(codes), _stream()), "blit_draw_p")
    return codes


def warp_draw(rng: DiffAugRng, policy, n, row0=0, p=None):
    """One dei2i_warp_draw launch on the current stream: -> a device int32 (warp runs, n, 8) table, row b the records (the 8-word rows
    of dei2i_warp, the floats stored bitwise) of the b-th warp run of ``policy`` for global rows [row0, row0 + n) (the counter-word
    layout: include/dei2i_hip.h -- the run word is the run's index in the whole list).  ``p``: the gated draw dei2i_warp_draw_p.
    A policy without a warp run raises ValueError."""
    from .utils.diffaug import REC_FIELDS, is_warp_run, policy_runs
    whole = policy_runs(policy)
    if not 0 < len(whole) <= L.DIFFAUG_MAX_RUNS:
        raise ValueError(f"diff_augment with a device RNG takes 1..{L.DIFFAUG_MAX_RUNS} canonical-order runs; {policy!r} has {len(whole)}")
    bit = {"scale": L.WARP_SCALE, "rotate": L.WARP_ROTATE, "aniso": L.WARP_ANISO}
    flags = count = 0
    for r, run in enumerate(whole):
        if is_warp_run(run):
            flags |= sum(bit[name] for name in run) << (3 * r)
            count += 1
    if not count:
        raise ValueError(f"warp_draw: {policy!r} holds no scale, rotate or aniso")
    tab = torch.empty((count, n, REC_FIELDS), dtype=torch.int32, device=rng.device)
    lib = _lib_for(tab)
    if p is None:
        L.check(lib.dei2i_warp_draw(rng.seed, _p(rng.counter), len(whole), flags, n, int(row0), _p(tab), _stream()), "warp_draw")
    else:
        L.check(lib.dei2i_warp_draw_p(rng.seed, _p(rng.counter), len(whole), flags, n, int(row0),
                                      _p(_gate_word(p, rng.device, "warp_draw")), _p(tab), _stream()), "warp_draw_p")
    return tab


class AdaState:
    """The device words of adaptive discriminator augmentation (csrc/ada.hip): ``p`` and ``rt`` (one-element fp32 views of one
    buffer: the probability the gated draw reads, the last computed r_t = E[sign(D(real))]), the measured ``pair`` (int64: sum of
    signs, logit count) and the accumulators ``acc`` (int64: sum_sign, n_logits, rows, calls).  All allocated here, outside any
    capture; they must outlive every graph that recorded a launch on them.  ``measure`` then ``apply`` once per D update, on one
    stream; between the two a data-parallel run SUMs ``pair`` over its ranks.  ``state()`` / ``set_state()`` synchronise: not for use
    inside a step."""

    def __init__(self, device, p=0.0, target=0.6, interval=4, kimg=500.0, p_max=1.0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"AdaState runs on the GPU; device {self.device} is not one (there is no CPU fallback)")
        self.target, self.interval, self.p_max = float(target), int(interval), float(p_max)
        self.inv_images = ctypes.c_float(1.0 / (float(kimg) * 1000.0)).value     # (once, as fp32: the kernel argument)
        self.p_rt = torch.tensor([float(p), 0.0], dtype=torch.float32, device=self.device)
        self.p, self.rt = self.p_rt[0:1], self.p_rt[1:2]
        self.pair = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.acc = torch.zeros(4, dtype=torch.int64, device=self.device)
        self.device = self.p_rt.device                       # (with its index)

    def measure(self, *logits):
        """``pair`` = (sum of sign, count) over every logit of the tensors: one launch per stretch of memory (tensors that are
        consecutive slices of one buffer, such as the splits of a batched discriminator pass, are one stretch)"""
        spans = []
        for t in logits:
            t = t.detach()
            if t.device != self.device:
                raise ValueError(f"AdaState.measure: the state lives on {self.device}, the logits on {t.device}")
            t = (t if t.dtype == torch.float32 else t.float()).contiguous()
            if t.numel() == 0:
                continue
            if spans and spans[-1][0].data_ptr() + 4 * spans[-1][1] == t.data_ptr() \
                    and spans[-1][0].untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
                spans[-1][1] += t.numel()
            else:
                spans.append([t, t.numel()])
        if not spans:
            raise ValueError("AdaState.measure needs at least one logit")
        lib = _lib_for(self.pair)
        for i, (t, count) in enumerate(spans):
            L.check(lib.dei2i_ada_measure(_p(t), count, _p(self.pair), int(i > 0), _stream()), "ada_measure")

    def apply(self, rows):
        """Add ``pair`` and ``rows`` (the real images the discriminator saw, over all ranks) to the accumulators; every ``interval``
        calls move ``p`` by rows / (kimg * 1000) towards the target and start over"""
        lib = _lib_for(self.pair)
        L.check(lib.dei2i_ada_apply(_p(self.pair), int(rows), _p(self.p_rt), _p(self.acc), self.interval, self.target, self.inv_images,
                                    self.p_max, _stream()), "ada_apply")

    def state(self):
        """-> {"p", "rt" (floats), "sum_sign", "n_logits", "rows", "calls" (ints)}"""
        p, rt = self.p_rt.tolist()
        return dict(zip(("sum_sign", "n_logits", "rows", "calls"), self.acc.tolist()), p=p, rt=rt)

    def set_state(self, state):
        torch.cuda.synchronize(self.device)                  # (launches queued on any stream read the old words)
        self.p_rt.copy_(torch.tensor([state["p"], state["rt"]], dtype=torch.float32))
        self.acc.copy_(torch.tensor([int(state[k]) for k in ("sum_sign", "n_logits", "rows", "calls")], dtype=torch.int64))
        torch.cuda.synchronize(self.device)


# ---- state digest (csrc/adam.hip: state_digest_kernel) -----------------------------------------------------------------------
DIGEST_ROWS_PER_LAUNCH = 4096


def state_digest(tensors, rows_per_launch=None):
    """-> a one-element int64 device tensor: the bits of the 64-bit digest of a list of device tensors,
    ``sum_k sum_i splitmix64(splitmix64((k << 32) | i) + w[k][i])`` mod 2^64 over the 32-bit words ``w[k][i]`` of tensor k's memory
    (include/dei2i_hip.h).  It depends on every bit, on a word's place in its tensor and on a tensor's place in the list.  One
    multi-tensor launch and a one-workgroup sum per ``rows_per_launch`` tensors (default ``DIGEST_ROWS_PER_LAUNCH``), queued on the
    current stream: nothing waits for the device.  Tensors that are not contiguous are copied; one that is not on the GPU, whose
    byte size is no multiple of 4 or that holds more than 2^32 words raises."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("state_digest needs at least one tensor")
    per = DIGEST_ROWS_PER_LAUNCH if rows_per_launch is None else int(rows_per_launch)
    if not 0 < per <= L.DIGEST_MAX_ROWS:
        raise ValueError(f"state_digest: |rows_per_launch {rows_per_launch}| is invalid (1..{L.DIGEST_MAX_ROWS})")
    rows, hold = [], []
    device = tensors[0].device
    for k, t in enumerate(tensors):
        _require_gpu(t, "state_digest")
        if t.device != device:
            raise ValueError(f"state_digest: tensor {k} is on {t.device}, tensor 0 on {device}")
        nbytes = t.numel() * t.element_size()
        if nbytes % 4:
            raise ValueError(f"state_digest: tensor {k} ({tuple(t.shape)}, {t.dtype}) holds {nbytes} bytes, not a whole number of "
                             "32-bit words")
        if nbytes // 4 > 2 ** 32:
            raise ValueError(f"state_digest: tensor {k} holds more than 2^32 words")
        t = t.detach()
        t = t if t.is_contiguous() else t.contiguous()
        if nbytes and t.data_ptr() % 4:
            raise ValueError(f"state_digest: tensor {k} does not start at a 4-byte boundary")
        hold.append(t)                                       # (a copy lives until its launch is queued)
        rows.append((t.data_ptr() if nbytes else 0, 0, 0, 0, nbytes // 4))
    lib = _lib_for(tensors[0])
    host = torch.empty((len(rows), L.ADAM_REC_WORDS), dtype=torch.int64, pin_memory=True)
    host.copy_(torch.tensor(rows, dtype=torch.int64))
    table = host.to(device, non_blocking=True)
    out = torch.empty(1, dtype=torch.int64, device=device)
    for row0 in range(0, len(rows), per):
        count = min(per, len(rows) - row0)
        max_n = max(1, max(r[4] for r in rows[row0:row0 + count]))
        partial = torch.empty(lib.dei2i_state_digest_blocks(max_n) * count, dtype=torch.int64, device=device)
        L.check(lib.dei2i_state_digest(c_void_p(table[row0].data_ptr()), count, max_n, row0, _p(partial), int(row0 > 0),
                                       _p(out), _stream()), "state_digest")
    return out


def diff_augment(x, policy="", rng=None, p=None):
    """DiffAugment(x, policy) of utils/diffaug.py on an NCHW fp32 GPU image batch, one or two launches per canonical-order policy
    run (one per blit run: flip -> rot90, csrc/blit.hip; one per warp run: scale -> rotate -> aniso, csrc/warp.hip).
    ``policy == ""`` returns ``x`` itself.  ``rng=None``: the same draws from
    the global CPU RNG as utils/diffaug.py, one upload of the parameter table per call.  ``rng`` a ``DiffAugRng``: the table is drawn
    on the device by one more launch (``diffaug_draw``), the codes of the blit runs by one more (``blit_draw``, after it) and the
    matrices of the warp runs by one more (``warp_draw``, last) -- the
    CPU RNG is not touched, nothing is uploaded, and the call can be captured into a graph.
    Inside ``diffaug_sharded`` ``x`` is one rank's rows of the global batch (above).  ``p`` (needs ``rng``): a one-element fp32 device
    tensor, the probability with which each policy applies to a row (``diffaug_draw``); the apply launches are the same.
    An unknown policy name raises KeyError and rot90 on a non-square batch ValueError, before anything is drawn."""
    if p is not None and rng is None:
        raise ValueError("diff_augment: p gates the device-drawn table; it needs rng (a DiffAugRng)")
    if not policy:
        return x
    _require_gpu(x, "diff_augment")
    if x.dim() != 4 or x.dtype != torch.float32:
        raise TypeError("diff_augment expects an NCHW fp32 image batch")
    from .utils.diffaug import BLIT, WARP, check_policy, draw_params
    n, _, h, w = x.shape
    check_policy(policy, h, w)
    if rng is not None:
        if rng.device != x.device:
            raise ValueError(f"diff_augment: the DiffAugRng lives on {rng.device}, the images on {x.device}")
        row0 = diffaug_shard[0] * n if diffaug_shard is not None else 0
        tab, runs = diffaug_draw(rng, policy, n, h, w, row0=row0, p=p)
        codes = blit_draw(rng, policy, n, row0=row0, p=p) if BLIT in runs else None
        mats = warp_draw(rng, policy, n, row0=row0, p=p) if WARP in runs else None
        host = None
    else:
        rec, runs = draw_params(policy, n, h, w, shard=diffaug_shard)
        blits = [r for r, run in enumerate(runs) if run == BLIT]
        warps = [r for r, run in enumerate(runs) if run == WARP]
        if blits or warps:               # (the affine runs' records, the warp runs' records, then one code word per sample: one upload)
            import numpy as np
            others = [r for r in range(len(runs)) if r not in blits and r not in warps]
            rec = np.concatenate([rec[others].reshape(-1), rec[warps].reshape(-1), rec[blits, :, 0].reshape(-1)])
        host = torch.empty(rec.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(torch.from_numpy(rec))
        tab = host.to(x.device, non_blocking=True)
        if blits or warps:
            a, b = len(others) * n * 8, (len(others) + len(warps)) * n * 8
            tab, mats, codes = tab[:a].view(len(others), n, 8), tab[a:b].view(len(warps), n, 8), tab[b:].view(len(blits), n)
    affine = blit = warp = 0
    for run in runs:
        if run == BLIT:
            x = _Blit.apply(x, codes[blit], host)
            blit += 1
        elif run == WARP:
            x = _Warp.apply(x, mats[warp], host)
            warp += 1
        else:
            x = _DiffAug.apply(x, tab[affine], run, 0, host)
            affine += 1
    return x


# --------------------------------------------------------------------------------------------------------------
# Device-drawn shifted patch masks of the MAE stage and the mask-token fill (csrc/mask.hip).  utils/masks.py draws the row shift,
# the column shift and the per-patch keep bits from the CPU RNG and uploads them; ``mask_draw`` draws them on the device from a
# ``DeviceRng`` instead (the counter-word layout: include/dei2i_hip.h) and ``mask_fill`` expands and applies them in one launch that
# reads the shifts from device memory -- both can be captured into a graph, and every replay masks other patches.
# --------------------------------------------------------------------------------------------------------------
def mask_draw(rng: DeviceRng, n, h, w, patch, mask_ratio, row0=0):
    """One dei2i_mask_draw launch on the current stream: -> (shift, keep), ``shift`` a device int32 (2,) tensor (row shift, column
    shift, each in [0, patch)), ``keep`` a device uint8 (n, 1, h/patch + 1, w/patch + 1) tensor (1 = patch kept, with probability
    1 - mask_ratio) for global rows [row0, row0 + n).  Nothing is read from the host RNG and nothing is uploaded."""
    n, h, w, patch = int(n), int(h), int(w), int(patch)
    if patch <= 0 or h % patch or w % patch:
        raise ValueError(f"mask_draw: {h}x{w} is not a whole number of {patch}x{patch} patches")
    gh, gw = h // patch + 1, w // patch + 1
    shift = torch.empty(2, dtype=torch.int32, device=rng.device)
    keep = torch.empty((n, 1, gh, gw), dtype=torch.uint8, device=rng.device)
    lib = _lib_for(keep)
    L.check(lib.dei2i_mask_draw(rng.seed, _p(rng.counter), n, int(row0), gh, gw, patch, 1.0 - float(mask_ratio), _p(shift), _p(keep),
                                _stream()), "mask_draw")
    return shift, keep


def _mask_geometry(imgs, keep, shift, patch, what):
    if not imgs.is_cuda:
        raise ValueError(f"{what}: the images are on {imgs.device}; the HIP kernels need a GPU tensor (there is no CPU fallback)")
    if imgs.dim() != 4 or imgs.dtype != torch.float32:
        raise TypeError(f"{what} expects an NCHW fp32 image batch")
    n, _, h, w = imgs.shape
    patch = int(patch)
    if patch <= 0 or h % patch or w % patch:
        raise ValueError(f"{what}: {h}x{w} is not a whole number of {patch}x{patch} patches")
    if keep.device != imgs.device or shift.device != imgs.device:
        raise ValueError(f"{what}: keep is on {keep.device}, shift on {shift.device}, the images on {imgs.device}")
    if keep.dtype != torch.uint8 or tuple(keep.shape) != (n, 1, h // patch + 1, w // patch + 1):
        raise ValueError(f"{what}: keep must be uint8 {(n, 1, h // patch + 1, w // patch + 1)}, not {keep.dtype} {tuple(keep.shape)}")
    if shift.dtype != torch.int32 or tuple(shift.shape) != (2,):
        raise ValueError(f"{what}: shift must be int32 (2,), not {shift.dtype} {tuple(shift.shape)}")
    return patch


class _MaskFill(torch.autograd.Function):
    @staticmethod
    def forward(ctx, imgs, token, keep, shift, patch):
        imgs, keep, shift = imgs.contiguous(), keep.contiguous(), shift.contiguous()
        n, c, h, w = imgs.shape
        filled = torch.empty_like(imgs)
        mask = torch.empty((n, 1, h, w), dtype=torch.float32, device=imgs.device)
        strides = None
        if token is not None:
            view = token.detach().expand(n, c, h, w)       # (stride 0 on every broadcast dim)
            strides = (ctypes.c_int64 * 4)(*view.stride())
        lib = _lib_for(imgs)
        L.check(lib.dei2i_mask_fill(n, c, h, w, patch, _p(shift), _p(keep), _p(imgs), _p(token), strides, _p(filled), _p(mask),
                                    _stream()), "mask_fill")
        ctx.keep, ctx.shift, ctx.patch = keep, shift, patch
        ctx.token_shape = None if token is None else tuple(token.shape)
        ctx.save_for_backward(mask)
        ctx.mark_non_differentiable(mask)
        return filled, mask

    @staticmethod
    def backward(ctx, g, _g_mask):
        g_imgs = g_token = None
        if ctx.needs_input_grad[0]:            # (the images are data: nothing on the hot path asks)
            g_imgs = g * ctx.saved_tensors[0]
        if ctx.token_shape is not None and ctx.needs_input_grad[1]:
            g = g.contiguous()
            n, c, h, w = g.shape
            full = torch.empty((1, c, h, w), dtype=torch.float32, device=g.device)
            lib = _lib_for(g)
            L.check(lib.dei2i_mask_fill_bwd(n, c, h, w, ctx.patch, _p(ctx.shift), _p(ctx.keep), _p(g), _p(full), _stream()),
                    "mask_fill_bwd")
            shape = (1,) * (4 - len(ctx.token_shape)) + ctx.token_shape
            dims = [d for d in range(1, 4) if shape[d] == 1 and full.shape[d] != 1]
            g_token = (torch.sum(full, dim=dims, keepdim=True) if dims else full).reshape(ctx.token_shape)
        return g_imgs, g_token, None, None, None


def mask_fill(imgs, keep, shift, patch, token=None):
    """``MaskToken`` on a device-side patch mask in one launch: -> (filled, mask), ``mask`` the (N,1,H,W) fp32 pixel mask
    ``utils.masks.expand_shifted_mask(keep, shift[0], shift[1], patch, H, W)`` and ``filled = imgs`` where it is 1, ``token`` (a
    tensor that broadcasts to one image (1,C,H,W); None: zero) where it is 0.  ``keep`` (N,1,H/patch+1,W/patch+1) uint8 and ``shift``
    (2,) int32 are plain device tensors (``mask_draw`` makes them; the shifts are read on the device).  Differentiable in ``token``
    (deterministic: the batch is summed in ascending order) and, with a torch op, in ``imgs``."""
    patch = _mask_geometry(imgs, keep, shift, patch, "mask_fill")
    if token is not None:
        if token.device != imgs.device or token.dtype != torch.float32:
            raise ValueError(f"mask_fill: the token is {token.dtype} on {token.device}, the images fp32 on {imgs.device}")
        if token.dim() > 4 or (token.dim() == 4 and token.shape[0] != 1):
            raise ValueError(f"mask_fill: a token of shape {tuple(token.shape)} does not broadcast to one image")
        torch.broadcast_shapes(tuple(token.shape), (1,) + tuple(imgs.shape[1:]))       # (raises when it does not)
    return _MaskFill.apply(imgs, token, keep, shift, patch)


# --------------------------------------------------------------------------------------------------------------
# Device-drawn style embeddings of the SEAN generator (csrc/embed.hip).  The reference draws them per sample with python's
# ``random.choices`` from the list stored for the sample's label tuple, which reads every label row on the host.  ``EmbedBank`` packs
# the lists into one device tensor once; ``embed_draw`` draws the rows' indices on the device from the bank's own ``DeviceRng`` (the
# counter-word layout: include/dei2i_hip.h) and gathers them -- two launches that can be captured into a graph, and every replay
# draws other embeddings.
# --------------------------------------------------------------------------------------------------------------
EMBED_MAX_LABEL_NC = L.EMBED_MAX_LABEL_NC


def embed_pack(embeddings, label_nc, embed_nc):
    """The host half of ``EmbedBank``: ``{label tuple: [tensor (embed_nc,), ...]}`` -> (bank, table) on the CPU.  ``bank``: fp32
    (total, embed_nc), the lists in ascending combination index (``sum_i label[i] << (label_nc - 1 - i)``: the first label is the
    slowest digit, torch.cartesian_prod order), each in its own order; ``table``: int32 (1 << label_nc, 2) of (offset, count), a
    combination the file does not hold counting as an empty list.  ValueError naming the key: a key that is no tuple of ``label_nc``
    zeros and ones, an embedding that is not an fp32 (embed_nc,) tensor."""
    label_nc, embed_nc = int(label_nc), int(embed_nc)
    if not 1 <= label_nc <= EMBED_MAX_LABEL_NC:
        raise ValueError(f"EmbedBank: |label_nc {label_nc}| is invalid (1..{EMBED_MAX_LABEL_NC}: the table has 2^label_nc rows)")
    if embed_nc <= 0:
        raise ValueError(f"EmbedBank: |embed_nc {embed_nc}| is invalid")
    lists = {}
    for key, embeds in embeddings.items():
        bits = tuple(key) if isinstance(key, (tuple, list)) else None
        if bits is None or len(bits) != label_nc or any(b not in (0, 1) for b in bits):
            raise ValueError(f"EmbedBank: key {key!r} is not a tuple of {label_nc} labels, each 0 or 1")
        for j, e in enumerate(embeds):
            if not isinstance(e, torch.Tensor) or tuple(e.shape) != (embed_nc,) or e.dtype != torch.float32:
                what = f"{tuple(e.shape)} {e.dtype}" if isinstance(e, torch.Tensor) else type(e).__name__
                raise ValueError(f"EmbedBank: embedding {j} of key {key!r} is {what}, not an fp32 ({embed_nc},) tensor")
        combo = 0
        for b in bits:
            combo = (combo << 1) | int(b)
        lists[combo] = list(embeds)
    table = torch.zeros((1 << label_nc, 2), dtype=torch.int32)
    rows = []
    for combo in sorted(c for c in lists if lists[c]):       # (an empty list stays (0, 0), like a missing key)
        table[combo, 0], table[combo, 1] = len(rows), len(lists[combo])
        rows.extend(e.detach().cpu() for e in lists[combo])
    if len(rows) >= 2 ** 31:
        raise ValueError(f"EmbedBank: {len(rows)} embeddings; the index is 32 bits wide")
    bank = torch.stack(rows) if rows else torch.zeros((0, embed_nc), dtype=torch.float32)
    return bank, table


class EmbedBank:
    """The embeddings of ``opt.embed_path`` packed for ``embed_draw`` (``embed_pack``): ``bank`` fp32 (max(total, 1), embed_nc) and
    ``table`` int32 (1 << label_nc, 2) on the device, the generator ``rng`` (a ``DeviceRng``: seed and call counter) and the
    ``invalid`` word, the count of label rows with an entry that is neither 0 nor 1 (their embeddings are zeros).  All allocated
    here, outside any capture; they must outlive every graph that recorded a draw on them.  ``invalid()`` synchronises: not for use
    inside a step."""

    def __init__(self, embeddings, label_nc, embed_nc, seed, device):
        self.rng = DeviceRng(seed, device)                   # (refuses a CPU device)
        self.device = self.rng.device
        self.label_nc, self.embed_nc = int(label_nc), int(embed_nc)
        bank, table = embed_pack(embeddings, label_nc, embed_nc)
        self.total = bank.shape[0]
        if self.total == 0:                                  # (every list empty: one row that no index ever names)
            bank = torch.zeros((1, self.embed_nc), dtype=torch.float32)
        self.bank = bank.to(self.device)
        self.table = table.to(self.device)
        self.invalid_word = torch.zeros(1, dtype=torch.int64, device=self.device)

    def invalid(self):
        """-> the number of invalid label rows drawn for so far"""
        return int(self.invalid_word.item()) & (2 ** 64 - 1)

    def digest(self):
        """``state_digest`` over the bank and the table: a one-element int64 device tensor"""
        return state_digest([self.bank, self.table])


def embed_draw(bank: EmbedBank, labels, num_embeds, row0=0):
    """SEAN's style embeddings for a batch of label rows: -> (feat, index), ``feat`` fp32 (N, num_embeds, embed_nc), ``index`` int32
    (N, num_embeds) the bank rows they are (-1: zeros -- the row's combination has no embeddings, or the row is invalid), for global
    rows [row0, row0 + N).  ``labels``: (N, label_nc) or (N, label_nc, 1, 1) on the bank's device, any float or integer dtype.  One
    dei2i_embed_draw and one dei2i_embed_gather launch on the current stream: nothing is read on the host and nothing is uploaded."""
    _require_gpu(labels, "embed_draw")
    if labels.device != bank.device:
        raise ValueError(f"embed_draw: the bank lives on {bank.device}, the labels on {labels.device}")
    if labels.dim() == 4 and tuple(labels.shape[2:]) == (1, 1):
        labels = labels.reshape(labels.shape[0], labels.shape[1])
    if labels.dim() != 2 or labels.shape[1] != bank.label_nc or labels.shape[0] == 0:
        raise ValueError(f"embed_draw: labels of shape {tuple(labels.shape)}; expected (N, {bank.label_nc}) or (N, {bank.label_nc}, 1, 1)")
    if labels.dtype == torch.bool or labels.is_complex():
        raise TypeError(f"embed_draw: labels of dtype {labels.dtype}; expected a float or integer dtype")
    num_embeds = int(num_embeds)
    if num_embeds <= 0:
        raise ValueError(f"embed_draw: |num_embeds {num_embeds}| is invalid")
    n = labels.shape[0]
    labels = _f32c(labels.detach())
    index = torch.empty((n, num_embeds), dtype=torch.int32, device=bank.device)
    feat = torch.empty((n, num_embeds, bank.embed_nc), dtype=torch.float32, device=bank.device)
    lib = _lib_for(feat)
    L.check(lib.dei2i_embed_draw(bank.rng.seed, _p(bank.rng.counter), n, int(row0), bank.label_nc, num_embeds, _p(labels), _p(bank.table),
                                 bank.total, _p(index), _p(bank.invalid_word), _stream()), "embed_draw")
    L.check(lib.dei2i_embed_gather(n * num_embeds, bank.embed_nc, _p(index), _p(bank.bank), bank.bank.shape[0], _p(feat), _stream()),
            "embed_gather")
    return feat, index


# --------------------------------------------------------------------------------------------------------------
# generator heads: tanh / sigmoid / compose  (generator.py:268-270), NaN guard (generator.py:266-267)
# --------------------------------------------------------------------------------------------------------------
class _Compose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, raw, x_in):
        _require_gpu(raw, "compose")
        prec = precision_of(raw)
        raw = raw.contiguous()
        x32 = _f32c(x_in.detach())
        n, h, w, cs = raw.shape
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=raw.device)
        prob = torch.empty((n, 1, h, w), dtype=torch.float32, device=raw.device)
        lib = _lib_for(raw)
        L.check(lib.dei2i_compose_fwd(prec.code, n, h, w, cs, _p(raw), _p(x32), _p(out), _p(prob), _stream()), "compose_fwd")
        ctx.prec = prec
        ctx.save_for_backward(raw, x32)
        return out, prob

    @staticmethod
    def backward(ctx, d_out, d_prob):
        raw, x32 = ctx.saved_tensors
        n, h, w, cs = raw.shape
        lib = _lib_for(raw)
        d_out = d_out.contiguous().float() if d_out is not None else None
        d_prob = d_prob.contiguous().float() if d_prob is not None else None
        d_raw = torch.empty_like(raw)
        d_x = torch.empty_like(x32) if ctx.needs_input_grad[1] else None
        if d_out is None and d_x is not None:
            d_x.zero_()
        L.check(lib.dei2i_compose_bwd(ctx.prec.code, n, h, w, cs, _p(raw), _p(x32), _p(d_out), _p(d_prob), _p(d_raw), _p(d_x),
                                      _stream()), "compose_bwd")
        return d_raw, d_x


def compose(raw, x_in):
    """(out, prob) = (x*(1-p) + tanh(raw[..., :3])*p, p = sigmoid(raw[..., 3])) as NCHW fp32."""
    return _Compose.apply(raw, x_in)


_nan_flags = {}


def nan_guard_(x):
    """In-place nan_to_num applied only if any NaN is present (reference semantics) -- no device->host sync."""
    _require_gpu(x, "nan_guard")
    prec = precision_of(x)
    flag = _nan_flags.get(x.device)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=x.device)
        _nan_flags[x.device] = flag
    lib = _lib_for(x)
    L.check(lib.dei2i_nan_guard(prec.code, x.numel(), _p(x), _p(flag), _stream()), "nan_guard")
    return x


# --------------------------------------------------------------------------------------------------------------
# losses (models/base_model.py:68-80)
# --------------------------------------------------------------------------------------------------------------
class _LossKind(NamedTuple):
    """One element-wise scalar loss (csrc/reduce.hip): the mean over i of term(a[i], b[i])."""
    name: str
    fwd: str             # entry points: fwd(n, a, b, [const,] out, stream), bwd(n, a, b, [const,] gout, da, [db,] stream)
    bwd: str
    takes_const: bool    # where there is no tensor ``b``, a python constant stands for it (else zeros)
    grad_b: bool         # ``b`` gets a gradient when it requires one (else it is detached)


class _ScalarLoss(torch.autograd.Function):
    """The one Function of the element-wise kinds.  A kind is a subclass that binds its record: ``_L1.apply(a, b)`` is this
    forward with ``_L1.kind`` (a class per kind, so that a kind's ``apply`` can be wrapped on its own: the tests' kink tape
    records the l1 sites that way)."""
    kind: _LossKind = None

    @classmethod
    def apply(cls, a, b, const: float = 0.0):
        return super().apply(cls.kind, a, b, const)

    @staticmethod
    def forward(ctx, kind: _LossKind, a, b, const: float):
        _require_gpu(a, kind.name)
        a = a.contiguous().float()
        bb = None if b is None else (b if kind.grad_b else b.detach()).contiguous().float()
        if bb is not None and bb.numel() != a.numel():
            raise ValueError(f"{kind.name}: target size mismatch")
        out = torch.empty((), dtype=torch.float32, device=a.device)      # written (not accumulated) by the finalize kernel
        ctx.kind, ctx.const = kind, (const,) if kind.takes_const else ()
        L.check(getattr(_lib_for(a), kind.fwd)(a.numel(), _p(a), _p(bb), *ctx.const, _p(out), _stream()), kind.fwd)
        ctx.save_for_backward(a, bb)
        return out

    @staticmethod
    def backward(ctx, g):
        a, bb = ctx.saved_tensors
        kind = ctx.kind
        g = g.contiguous().float()
        da = torch.empty_like(a) if ctx.needs_input_grad[1] else None
        db = torch.empty_like(bb) if (kind.grad_b and bb is not None and ctx.needs_input_grad[2]) else None
        if da is None and db is None:
            return None, None, None, None
        grads = (_p(da), _p(db)) if kind.grad_b else (_p(da),)
        L.check(getattr(_lib_for(a), kind.bwd)(a.numel(), _p(a), _p(bb), *ctx.const, _p(g), *grads, _stream()), kind.bwd)
        return None, da, db, None


class _BceLogits(_ScalarLoss):
    kind = _LossKind("bce_logits", "dei2i_bce_logits_fwd", "dei2i_bce_logits_bwd", takes_const=True, grad_b=False)


class _L1(_ScalarLoss):
    kind = _LossKind("l1", "dei2i_l1_fwd", "dei2i_l1_bwd", takes_const=False, grad_b=True)


class _Mse(_ScalarLoss):
    kind = _LossKind("mse", "dei2i_mse_fwd", "dei2i_mse_bwd", takes_const=True, grad_b=True)


def bce_logits(x, target):
    """binary_cross_entropy_with_logits(x, target), mean.  ``target`` is a tensor or a python float constant."""
    if isinstance(target, (int, float)):
        return _BceLogits.apply(x, None, float(target))
    return _BceLogits.apply(x, target)


def l1(a, b=None):
    """l1_loss(a, b), mean; ``b=None`` means zeros (sd_con, defectgan_model.py:231-236)."""
    return _L1.apply(a, b)


def mse(a, b=0.0):
    """mse_loss(a, b), mean.  ``b`` is a tensor (it gets its gradient when it requires one) or a python number."""
    if b is None or isinstance(b, (int, float)):
        return _Mse.apply(a, None, float(b or 0.0))
    return _Mse.apply(a, b)


class _CceLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target):
        _require_gpu(x, "cce_logits")
        if x.dim() < 2 or any(d != 1 for d in x.shape[2:]) or x.numel() == 0:
            raise ValueError(f"cce_logits: logits of shape {tuple(x.shape)}; expected (N, C) or (N, C, 1, ..., 1)")
        rows, classes = x.shape[0], x.shape[1]
        if target.numel() != x.numel():
            raise ValueError("cce_logits: target size mismatch")
        x = x.contiguous().float()
        t = target.detach().contiguous().float()
        out = torch.empty((), dtype=torch.float32, device=x.device)      # written (not accumulated) by the finalize kernel
        lib = _lib_for(x)
        L.check(lib.dei2i_cce_logits_fwd(rows, classes, _p(x), _p(t), _p(out), _stream()), "cce_fwd")
        ctx.save_for_backward(x, t)
        return out

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        g = g.contiguous().float()
        dx = torch.empty_like(x)
        lib = _lib_for(x)
        L.check(lib.dei2i_cce_logits_bwd(x.shape[0], x.shape[1], _p(x), _p(t), _p(g), _p(dx), _stream()), "cce_bwd")
        return dx, None


def cce_logits(x, target):
    """cross_entropy(x, target), mean over the rows: ``x`` is (N, C) or (N, C, 1, ..., 1), ``target`` a tensor of as many elements
    holding class weights (one-hot rows: the class-index form; multi-hot and all-zero rows are legal).  No gradient goes to the target."""
    if not isinstance(target, torch.Tensor):
        raise ValueError("cce_logits: the target is a tensor of class weights, one row per sample")
    return _CceLogits.apply(x, target)


# --------------------------------------------------------------------------------------------------------------
# Validation metrics (csrc/metrics.hip; trainer.validate()): per image the sums PSNR, L1 and SSIM are made of in ONE pass over the
# two image batches, and the classifier's confusion counts -- float64 / int64 device tensors that add up over a loader, read by
# the host once (``metrics_summary`` / ``clf_scores``).  No autograd.
# --------------------------------------------------------------------------------------------------------------
SSIM_WINDOW = 11
IMAGE_SUMS = ("sse", "sae", "sse_masked", "sae_masked", "count_masked", "ssim_sum")
CLF_KINDS = {"bce": L.CLF_MULTI, "mse": L.CLF_MULTI, "cce": L.CLF_ARGMAX}


def image_metrics(x, y, mask=None, data_range=2.0):
    """-> float64 (N, 6) device tensor, per image (``IMAGE_SUMS``): the sums of (x-y)^2 and |x-y| over its C*H*W elements; the same
    two over the elements of the pixels where ``mask`` (N,1,H,W) is not 0, and their count (zeros without a mask); the sum of SSIM
    (Wang et al. 2004: 11 x 11 Gaussian window, sigma 1.5, no padding, C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = ``data_range``) over the
    C*(H-10)*(W-10) window positions.  ``x``, ``y``: NCHW image batches of one shape; other dtypes or layouts than contiguous fp32
    are converted.  Two launches on the current stream, no atomics, nothing read on the host: bit-reproducible, capturable."""
    if x.dim() != 4 or tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"image_metrics: x of shape {tuple(x.shape)}, y of shape {tuple(y.shape)}; expected two NCHW batches of one shape")
    n, c, h, w = x.shape
    if n == 0 or c == 0 or h < SSIM_WINDOW or w < SSIM_WINDOW:
        raise ValueError(f"image_metrics: {n} x {c} x {h} x {w} images; the {SSIM_WINDOW} x {SSIM_WINDOW} SSIM window needs H, W >= "
                         f"{SSIM_WINDOW} (and N, C > 0)")
    if mask is not None and tuple(mask.shape) != (n, 1, h, w):
        raise ValueError(f"image_metrics: mask of shape {tuple(mask.shape)}; expected {(n, 1, h, w)}")
    if not float(data_range) > 0.0:
        raise ValueError(f"image_metrics: |data_range {data_range}| is invalid (> 0)")
    _require_gpu(x, "image_metrics")
    if y.device != x.device or (mask is not None and mask.device != x.device):
        raise ValueError(f"image_metrics: x is on {x.device}, y on {y.device}" + (f", the mask on {mask.device}" if mask is not None else ""))
    x, y = _f32c(x.detach()), _f32c(y.detach())
    mask = None if mask is None else _f32c(mask.detach())
    lib = _lib_for(x)
    words = lib.dei2i_image_metrics_ws_doubles(n, c, h, w)
    if words <= 0:
        raise ValueError(f"image_metrics: a batch of shape {(n, c, h, w)} is too large (N*C*H*W < 2^40, C*H*W < 2^31)")
    ws = torch.empty(words, dtype=torch.float64, device=x.device)
    out = torch.empty((n, len(IMAGE_SUMS)), dtype=torch.float64, device=x.device)
    L.check(lib.dei2i_image_metrics(n, c, h, w, _p(x), _p(y), _p(mask), float(data_range), _p(ws), _p(out), _stream()), "image_metrics")
    return out


def clf_counts(logits, targets, kind, out=None):
    """Confusion counts of a classifier head: ``logits`` (N, K) or (N, K, 1, ..., 1) against ``targets`` of as many elements.
    ``kind`` "bce" / "mse" (multi-label): class k of a row is predicted when its logit is > 0 (a logit of 0 is a negative), wanted
    when its target is > 0.5; "cce": the row's argmax against the targets' argmax.  -> int64 (4K + 1,) device tensor TP[K] | FP[K] |
    FN[K] | TN[K] | rows right in every class: ``out`` (the caller's, ADDED to: a loader sums without a host read) or a fresh one."""
    if kind not in CLF_KINDS:
        raise ValueError(f"clf_counts: |kind {kind}| is invalid ({' | '.join(CLF_KINDS)})")
    if logits.dim() < 2 or any(d != 1 for d in logits.shape[2:]) or logits.numel() == 0:
        raise ValueError(f"clf_counts: logits of shape {tuple(logits.shape)}; expected (N, K) or (N, K, 1, ..., 1)")
    if targets.numel() != logits.numel():
        raise ValueError("clf_counts: target size mismatch")
    n, k = logits.shape[0], logits.shape[1]
    _require_gpu(logits, "clf_counts")
    if targets.device != logits.device:
        raise ValueError(f"clf_counts: the logits are on {logits.device}, the targets on {targets.device}")
    if out is None:
        out = torch.zeros(4 * k + 1, dtype=torch.int64, device=logits.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (4 * k + 1,) or out.device != logits.device or not out.is_contiguous():
        raise ValueError(f"clf_counts: out must be a contiguous int64 ({4 * k + 1},) tensor on {logits.device}")
    logits, targets = _f32c(logits.detach().reshape(n, k)), _f32c(targets.detach().reshape(n, k))
    L.check(_lib_for(logits).dei2i_clf_counts(n, k, _p(logits), _p(targets), CLF_KINDS[kind], _p(out), _stream()), "clf_counts")
    return out


IMAGE_SCORES = ("psnr", "ssim", "l1", "psnr_masked")
CLF_SCORES = ("acc", "f1")


def image_scores(sums, chw, data_range=2.0):
    """``image_metrics`` rows (M, 6) of images of shape ``chw`` = (C, H, W) -> float64 (4,) device tensor (``IMAGE_SCORES``), torch ops
    on M numbers: the mean over the images of 10 log10(L^2 / max(mse, 1e-10 L^2)) (an exact reconstruction scores 100 dB), of the mean
    SSIM and of the mean |x-y|, and the PSNR over the masked elements, averaged over the images that have any (NaN when none has)."""
    c, h, w = (int(v) for v in chw)
    sums = sums.reshape(-1, len(IMAGE_SUMS)).double()
    peak = float(data_range) ** 2

    def psnr(mse):
        return 10.0 * torch.log10(peak / mse.clamp_min(1e-10 * peak))

    count = sums[:, 4]
    masked = torch.where(count > 0, psnr(sums[:, 2] / count.clamp_min(1.0)), torch.full_like(count, float("nan")))
    return torch.stack([psnr(sums[:, 0] / (c * h * w)).mean(),
                        (sums[:, 5] / (c * (h - SSIM_WINDOW + 1) * (w - SSIM_WINDOW + 1))).mean(),
                        (sums[:, 1] / (c * h * w)).mean(), torch.nanmean(masked)])


def clf_scores_dev(counts):
    """``clf_counts`` words -> float64 (2,) device tensor (``CLF_SCORES``): the share of rows right in every class, and the macro F1
    = mean of 2 TP / (2 TP + FP + FN) over the classes with any positive target (NaN when there is none)"""
    k = (counts.numel() - 1) // 4
    tp, fp, fn, tn = counts[:4 * k].double().reshape(4, k)
    rows = tp[0] + fp[0] + fn[0] + tn[0]
    f1 = torch.where(tp + fn > 0, 2 * tp / (2 * tp + fp + fn).clamp_min(1.0), torch.full_like(tp, float("nan")))
    return torch.stack([counts[4 * k].double() / rows, torch.nanmean(f1)])


def metrics_summary(sums, chw, data_range=2.0):
    """Accumulated ``image_metrics`` rows (the batches' outputs concatenated) of images of shape ``chw`` = (C, H, W) -> {"psnr",
    "ssim", "l1", "psnr_masked"} as Python floats (``image_scores``), with ONE device read."""
    return dict(zip(IMAGE_SCORES, image_scores(sums, chw, data_range).tolist()))


def clf_scores(counts):
    """Accumulated ``clf_counts`` words -> {"acc", "f1"} as Python floats (``clf_scores_dev``), with one device read"""
    return dict(zip(CLF_SCORES, clf_scores_dev(counts).tolist()))
