"""No host-side cache of the hot path serves stale data: every cache of DESIGN.md section 4's table, populated, then its data
changed by every writer that may change it, then read again through the HIP kernels.

The kernels themselves are pinned elsewhere (test_conv_exact_gpu.py and its siblings); what stands between them and a correct step is
Python that memoises on tensor identity, ``Tensor._version`` and the ``_dei2i_epoch`` stamp.  A missed invalidation does not crash, it
hands a correct kernel the operand of an earlier call, so "stale" must be unambiguous:

* integer writers (the new weights W1 are integers): test_conv_exact_gpu.py's recipe.  x, dy, W0 and W1 come from {-1, 0, 1}, every
  sum is an exact integer (|y|, |dx| <= 256, |dw| < 2^24), the result must ``torch.equal`` the float64 reference on W1, and the
  references on W0 and on W1 differ in at least half of their elements (asserted where the case is built,
  test_host_caches_cpu.integer_case);
* writers that leave non-integer weights (Adam, RMSprop, init_weights, spectral norm, the BatchNorm fold): bit-equality with the same
  call on a fresh ``ops.PackedWeights()`` AND float64 on the rounded new weights at test_ops_gpu.py's bounds (2e-4 / 1.5e-2 of the
  tensor's maximum), where the old-weight and new-weight references are asserted to lie at least 10 bounds apart (printed).

Shapes are the smallest that reach the code: N = 2, 16 -> 16, 3x3 at 8x8 for the packed layouts; the smallest batch the halo gates
admit (from the gates' expressions and the CU count, like test_conv_fused_exact_gpu.py) for the epilogue statistics, the operand-path
entry points and the fp8 copy.  Wall time of the file on an MI355X with 16 CPU threads: 6.8 s for its 61 tests (the slowest, the
one-rank gloo group of the broadcast case, 1.0 s; the captured step 0.5 s)."""
import copy
import os
import socket
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

from oracle import defectgan_oracle as O
from test_conv_exact_gpu import _counts, n_halo8, n_halo16
from test_host_caches_cpu import differ, integer_case, ints
from test_optim_edges_gpu import K_ROUND, adam_mv, adam_p, f32, worst

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"f32": 2e-4, "bf16": 1.5e-2}                 # test_ops_gpu.py / test_reduce_edges_gpu.py: of the tensor's maximum
PNAMES = ["bf16", "f32"]


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


def note(*a):
    print("[host-caches]", *a, flush=True)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dtype_of(pname):
    return torch.bfloat16 if pname == "bf16" else torch.float32


def rounded(t, pname):
    return t.to(torch.bfloat16).float() if pname == "bf16" else t


def nhwc(t, pname):
    """NCHW fp32 cpu -> NHWC compute-dtype GPU tensor (channel counts here are multiples of the vector: no padding)"""
    assert t.shape[1] % 8 == 0
    return t.permute(0, 2, 3, 1).contiguous().to(DEV, dtype_of(pname))


def nchw(t):
    """NHWC GPU tensor -> NCHW float64 cpu"""
    return t.detach().double().cpu().permute(0, 3, 1, 2).contiguous()


def differ_live(a, b):
    """``differ`` over the elements that are non-zero in either tensor (outputs behind a ReLU are zero in half of theirs)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    live = (a != 0) | (b != 0)
    return (a != b)[live].double().mean().item()


def relmax(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def conv_ref(x, w, gy, pad=1):
    """float64 F.conv2d and its gradients -> (y, dx, dw)"""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv2d(xr, wr, padding=pad)
    dx, dw = torch.autograd.grad(y, [xr, wr], gy.double())
    return y.detach(), dx, dw


def conv_pass(call, weight, x, gy, pname):
    """one forward and backward of ``call`` (activation -> activation) -> (y, dx, dw) on the CPU in float64"""
    xg = nhwc(x, pname).requires_grad_(True)
    y = call(xg)
    grads = torch.autograd.grad(y, [xg, weight] if weight.requires_grad else [xg], nhwc(gy, pname))
    torch.cuda.synchronize()
    return nchw(y), nchw(grads[0]), (grads[1].detach().double().cpu() if weight.requires_grad else None)


def assert_exact(got, c, which, tag):
    y, dx, dw = got
    for name, g, r in (("y", y, c[f"y{which}"]), ("dx", dx, c[f"dx{which}"]), ("dw", dw, c["dw"])):
        if g is not None:
            assert torch.equal(g, r), f"{tag}: {name} differs from the float64 reference on W{which} in {differ(g, r):.3f} of its elements" + \
                (f"; from the one on W{1 - which} in {differ(g, c[f'{name}{1 - which}']):.3f}" if name != "dw" else "")


def assert_close_and_powerful(got, fresh, ref_new, ref_old, pname, tag):
    """the checks of a writer that leaves non-integer weights (module docstring)"""
    tol = TOL[pname]
    for name, g, f, rn, ro in zip(("y", "dx", "dw"), got, fresh, ref_new, ref_old):
        assert torch.equal(g, f), f"{tag}: {name} is not what a fresh PackedWeights gives ({differ(g, f):.3f} of the elements)"
        if name != "dw":              # (dw does not depend on the weight)
            apart = relmax(ro, rn)
            note(f"{tag}: {name} old-weight and new-weight references {apart:.3g} apart = {apart / tol:.0f} bounds")
            assert apart >= 10 * tol, f"{tag}: a broken case -- the references on the old and the new weights are {apart:.3g} apart"
        e = relmax(g, rn)
        assert e < tol, f"{tag}: {name} {e:.3g} from float64 on the new weights (bound {tol})"


def make_net(ops):
    from de_i2i_gan_amd.networks.architecture import Conv2d
    from de_i2i_gan_amd.networks.base_network import BaseNetwork

    class Net(BaseNetwork):
        def __init__(self):
            super().__init__()
            self.conv = Conv2d(16, 16, 3, padding=1, bias=False)
    return Net().to(DEV)


# =====================================================================================================================================
# A. packed weights against every writer
# =====================================================================================================================================
def _rand_grad(w, seed):
    w.grad = torch.randn(w.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _w_copy(net, c, ops):
    with torch.no_grad():
        net.conv.weight.copy_(c["W1"].to(DEV))
    return True


def _w_load_state_dict(net, c, ops):
    net.load_state_dict({"conv.weight": c["W1"]})
    return True


def _w_torch_sgd(net, c, ops):
    net.conv.weight.grad = (c["W0"] - c["W1"]).to(DEV)          # lr = 1: W0 - (W0 - W1), exact
    torch.optim.SGD([net.conv.weight], lr=1.0).step()
    return True


def _w_fused_sgd(net, c, ops):
    from de_i2i_gan_amd import optim
    net.conv.weight.grad = (c["W0"] - c["W1"]).to(DEV)
    optim.FusedSGD([net.conv.weight], lr=1.0).step()
    return True


def _w_fused_adam(net, c, ops):
    from de_i2i_gan_amd import optim
    _rand_grad(net.conv.weight, 21)
    optim.FusedAdam([net.conv.weight], lr=0.5).step()
    return False


def _w_fused_rmsprop(net, c, ops):
    from de_i2i_gan_amd import optim
    _rand_grad(net.conv.weight, 22)
    optim.FusedRMSprop([net.conv.weight], lr=0.5).step()
    return False


def _w_ema_lerp(net, c, ops):
    from de_i2i_gan_amd import optim
    optim.ema_lerp_([net.conv.weight], [c["W1"].to(DEV)], 0.0)       # weight 0: an exact copy of the source
    return True


def _w_ema_group(net, c, ops):
    from de_i2i_gan_amd import optim
    optim.EmaGroup([(net.conv.weight, c["W1"].to(DEV))]).update(0.0)
    return True


def _w_to_device(net, c, ops):
    net.to("cpu")
    with torch.no_grad():
        net.conv.weight.copy_(c["W1"])
    net.to(torch.device(DEV))                                           # new storage
    return True


def _w_data_assign(net, c, ops):
    net.conv.weight.data = c["W1"].to(DEV).clone()
    return True


def _w_init_normal(net, c, ops):
    torch.manual_seed(11)
    net.init_weights("normal", 0.5)
    return False


def _w_init_none(net, c, ops):
    torch.manual_seed(12)
    net.init_weights("none")                                            # through reset_parameters
    return False


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _w_broadcast(net, c, ops):
    """parallel.GradReducer.broadcast_parameters on a one-rank gloo group with forced collectives: rank 0's values are this process's
    own, written through ``.data`` just before (no stamp moves) -- the broadcast copies them through ``.data`` as well and stamps."""
    import torch.distributed as dist
    from de_i2i_gan_amd.parallel import GradReducer
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(_free_port())
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        stamp = ops.PackedWeights._stamp(net.conv.weight)
        net.conv.weight.data.copy_(c["W1"].to(DEV))
        assert ops.PackedWeights._stamp(net.conv.weight) == stamp
        GradReducer(force_collectives=True).broadcast_parameters(net)
        assert ops.PackedWeights._stamp(net.conv.weight) != stamp
    finally:
        dist.destroy_process_group()
    return True


WRITERS = {"copy_": _w_copy, "load_state_dict": _w_load_state_dict, "torch_sgd": _w_torch_sgd, "fused_sgd": _w_fused_sgd,
           "fused_adam": _w_fused_adam, "fused_rmsprop": _w_fused_rmsprop, "ema_lerp": _w_ema_lerp, "ema_group": _w_ema_group,
           "to_device": _w_to_device, "data_assign": _w_data_assign, "init_normal": _w_init_normal, "init_none": _w_init_none,
           "broadcast": _w_broadcast}


@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_packed_weights_follow_every_writer(ops, writer, pname):
    """forward + backward with W0 (populates the forward and the dgrad layout of the module's one cache), the writer, forward +
    backward again: the second pass is the float64 reference on the NEW weights"""
    c = integer_case("plain")
    net = make_net(ops)
    with torch.no_grad():
        net.conv.weight.copy_(c["W0"].to(DEV))
    geom, cache = net.conv.geom(False), net.conv._packed
    tag = f"{writer} {pname}"
    assert_exact(conv_pass(net.conv, net.conv.weight, c["x"], c["gy"], pname), c, 0, tag + " before")
    assert cache.fwd is not None and cache.dgrad is not None
    exact = WRITERS[writer](net, c, ops)
    w = net.conv.weight
    assert net.conv._packed is cache and w.is_cuda
    got = conv_pass(net.conv, w, c["x"], c["gy"], pname)
    if exact:
        assert torch.equal(w.detach().cpu(), c["W1"]), "the writer did not leave W1"
        assert_exact(got, c, 1, tag)
        return
    w_new = w.detach().cpu()
    assert differ(w_new, c["W0"]) >= 0.5
    fresh = conv_pass(lambda xg: ops.conv2d(xg, w, None, ops.PackedWeights(), geom), w, c["x"], c["gy"], pname)
    ref_new = conv_ref(c["x"], rounded(w_new, pname), c["gy"])
    assert_close_and_powerful(got, fresh, ref_new, (c["y0"], c["dx0"], c["dw"]), pname, tag)


def test_packed_weights_after_a_replayed_graph_step():
    """A captured defectGAN step writes every parameter from inside the graph; graph_step stamps them after the replay.  The eager eval
    forward that follows must equal the same forward on a deep copy of the generator, whose caches are empty
    (PackedWeights.__deepcopy__).  No float64 reference here: the step's kernels are pinned by test_graph_step_gpu.py."""
    from test_graph_step_gpu import SMALL, batch, build
    c = SMALL
    tr = build(c, "bf16", graph_step=True, graph_warmup=1)
    try:
        netG = tr.model.netG
        bg, lab, df = (t.to(DEV) for t in batch(c, 0))
        probe = lambda net: [t.detach().clone() for t in _eval_forward(net, bg, lab)]     # noqa: E731
        before = probe(netG)                                           # populates every cache of the eval path
        for i in range(3):                                             # one eager warm-up step, the capture + replay, one more replay
            tr.step(*(t.to(DEV) for t in batch(c, i)))
        assert tr._graphs is not None and len(tr._graphs.graphs) == 1
        torch.cuda.synchronize()
        after = probe(netG)
        netG.clear_spade_cache()            # (the G step's tables carry autograd history, which deepcopy refuses)
        twin = copy.deepcopy(netG)
        want = probe(twin)
        for a, b_, w_ in zip(after, before, want):
            assert differ(a.cpu(), b_.cpu()) >= 0.5, "a broken case: three steps left the generator's output where it was"
            assert torch.equal(a, w_), f"the eval forward after the replay differs from a fresh copy's in {differ(a.cpu(), w_.cpu()):.3f}"
    finally:
        tr.release_graphs()


def _eval_forward(net, bg, lab):
    was = net.training
    net.eval()
    try:
        with torch.no_grad():
            return net(bg, lab)
    finally:
        net.train(was)


@pytest.mark.parametrize("pname", PNAMES)
def test_a_forward_only_pack_is_completed_not_repeated(ops, pname):
    """a no-grad forward packs the forward layout alone; the call that then needs the dgrad layout packs only that one and the forward
    copy keeps its storage and its bits"""
    c = integer_case("plain")
    prec = ops.get_precision(pname)
    w = c["W1"].to(DEV)                                                 # (no gradient: nothing asks for the dgrad layout)
    geom, cache = ops.ConvGeom(16, 16, 3, 1, 1, False, False), ops.PackedWeights()
    xg = nhwc(c["x"], pname)
    y = ops.conv2d(xg, w, None, cache, geom)
    assert cache.fwd is not None and cache.dgrad is None and torch.equal(nchw(y), c["y1"])
    fwd, ptr, bits = cache.fwd, cache.fwd.data_ptr(), cache.fwd.clone()
    y, dx, _ = conv_pass(lambda t: ops.conv2d(t, w, None, cache, geom), w, c["x"], c["gy"], pname)
    assert cache.dgrad is not None and cache.fwd is fwd and cache.fwd.data_ptr() == ptr and torch.equal(cache.fwd, bits)
    assert torch.equal(y, c["y1"]) and torch.equal(dx, c["dx1"])
    wf, wd = cache.get(w, (w,), prec, geom, 16, 16, need_dgrad=True)
    assert wf is fwd and wd is cache.dgrad                              # a hit


def test_one_cache_serves_both_precisions_in_turn(ops):
    """the key holds prec.code: bf16, then f32, then bf16 again through ONE cache, with a weight write in between"""
    c = integer_case("plain")
    w = torch.nn.Parameter(c["W0"].to(DEV))
    geom, cache = ops.ConvGeom(16, 16, 3, 1, 1, False, False), ops.PackedWeights()
    call = lambda t: ops.conv2d(t, w, None, cache, geom)               # noqa: E731
    for pname in ("bf16", "f32", "bf16"):
        assert_exact(conv_pass(call, w, c["x"], c["gy"], pname), c, 0, f"W0 {pname}")
        assert cache.fwd.dtype == dtype_of(pname) and cache.dgrad.dtype == dtype_of(pname)
    with torch.no_grad():
        w.copy_(c["W1"].to(DEV))
    for pname in ("f32", "bf16", "f32"):
        assert_exact(conv_pass(call, w, c["x"], c["gy"], pname), c, 1, f"W1 {pname}")


@pytest.mark.parametrize("writer", ["copy_", "ema_lerp", "fused_adam"])
def test_fp8_weight_copy_after_a_weight_write(ops, writer):
    """PackedWeights.get_fp8 under ops.fp8_forward: after a write the e4m3 bytes and the dequant scalar are those of a fresh pack (and not
    the old ones).  CinS % 128 == 0 at the 8 x 32 descriptor get_fp8 packs with."""
    gen = torch.Generator().manual_seed(31)
    w0, w1 = (torch.randn(128, 128, 3, 3, generator=gen) * s for s in (0.05, 0.11))
    net = SimpleNet(torch.nn.Parameter(w0.to(DEV)))
    w = net.conv.weight
    geom, cache = ops.ConvGeom(128, 128, 3, 1, 1, True, False), ops.PackedWeights()
    with ops.fp8_forward(True):
        q0, d0 = (t.clone() for t in cache.get_fp8(w, (w,), ops.BF16, geom, 128, 128))
        assert cache.get_fp8(w, (w,), ops.BF16, geom, 128, 128)[0] is cache.fp8[0]                 # a hit
        WRITERS[writer](net, {"W1": w1}, ops)
        q1, d1 = cache.get_fp8(w, (w,), ops.BF16, geom, 128, 128)
        qf, df = ops.PackedWeights().get_fp8(w, (w,), ops.BF16, geom, 128, 128)
    torch.cuda.synchronize()
    assert differ(q0.cpu(), qf.cpu()) >= 0.5 and d0.item() != df.item(), "a broken case: the write left the e4m3 copy where it was"
    assert torch.equal(q1, qf) and torch.equal(d1, df)


class SimpleNet:
    """what the writers of section A address: ``net.conv.weight``"""

    def __init__(self, weight):
        self.conv = type("Holder", (), {})()
        self.conv.weight = weight


def spectral_inputs():
    """(weight_orig, u, v): one dominant singular pair and a start vector almost orthogonal to it, so that the first and the second
    power iteration give weights that differ by more than their own magnitude (1.24 of max |w_eff| in float64)"""
    g = torch.Generator().manual_seed(7)
    a, b = F.normalize(torch.randn(16, generator=g), dim=0), F.normalize(torch.randn(144, generator=g), dim=0)
    w = (1.5 * torch.outer(a, b) + 0.05 * torch.randn(16, 144, generator=g)).view(16, 16, 3, 3)
    u = torch.randn(16, generator=g)
    u = F.normalize(u - (u @ a) * a + 0.05 * a, dim=0)
    v = F.normalize(torch.randn(144, generator=g), dim=0)
    return w, u, v


@pytest.mark.parametrize("pname", PNAMES)
def test_spectral_conv_applied_twice_before_one_backward(ops, pname):
    """The per-call path: a training-mode SpectralConv2d derives its weight anew in every forward (u, v iterate in place), so the
    packed copies travel with the call.  Two forwards, then one backward: each input gradient is that of its OWN forward's weight
    (oracle.weight_of in float64, as test_spectral_edges_gpu.py uses it) -- not of the other call's."""
    from de_i2i_gan_amd.networks.architecture import SpectralConv2d
    w, u, v = spectral_inputs()
    conv = SpectralConv2d(16, 16, 3, padding=1, bias=False).to(DEV).train()
    conv.load_state_dict({"weight_orig": w, "weight_u": u, "weight_v": v})
    c = integer_case("plain")
    x1, x2, gy1, gy2 = c["x"], ints(c["x"].shape, 41), c["gy"], ints(c["gy"].shape, 42)
    S = {"c.weight_orig": w.double(), "c.weight_u": u.double().clone(), "c.weight_v": v.double().clone()}
    r1 = O.weight_of(S, "c.weight", True)
    r2 = O.weight_of(S, "c.weight", True)
    own = conv_ref(x1, r1, gy1), conv_ref(x2, r2, gy2)
    crossed = conv_ref(x1, r2, gy1), conv_ref(x2, r1, gy2)
    xg1, xg2 = (nhwc(t, pname).requires_grad_(True) for t in (x1, x2))
    y1, y2 = conv(xg1), conv(xg2)
    dx1, dx2, dw = torch.autograd.grad([y1, y2], [xg1, xg2, conv.weight_orig], [nhwc(gy1, pname), nhwc(gy2, pname)])
    torch.cuda.synchronize()
    tol = TOL[pname]
    for i, (y, dx) in enumerate(((y1, dx1), (y2, dx2))):
        for name, g, mine, other in (("y", y, own[i][0], crossed[i][0]), ("dx", dx, own[i][1], crossed[i][1])):
            apart = relmax(other, mine)
            note(f"spectral twice {pname}: {name}{i + 1} own-weight and other-call references {apart:.3g} apart = {apart / tol:.0f} bounds")
            assert apart >= 10 * tol, "a broken case"
            e = relmax(nchw(g), mine)
            assert e < tol, f"{name}{i + 1}: {e:.3g} from the float64 reference on its own forward's weight (bound {tol})"
    assert dw.shape == w.shape and torch.isfinite(dw).all()


@pytest.mark.parametrize("pname", PNAMES)
def test_eval_folded_batchnorm_after_running_var_changed(ops, pname):
    """ConvBlock in eval mode under no_grad folds BatchNorm's running statistics into the conv weight per call (ops.fold_bn_weight): a
    change of running_var between two calls -- in place, and through a raw-pointer style write that moves no version -- must show"""
    from de_i2i_gan_amd.networks.architecture import BatchNorm2d, ConvBlock
    c = integer_case("plain")
    block = ConvBlock(16, 16, (3, 3), padding=1, norm_layer=BatchNorm2d, act_layer="leaky_relu").to(DEV).eval()
    conv, bn = block.conv_block[0], block.conv_block[1]
    gen = torch.Generator().manual_seed(51)
    with torch.no_grad():
        conv.weight.copy_(c["W0"].to(DEV))
        bn.weight.copy_((1 + 0.2 * torch.randn(16, generator=gen)).to(DEV))
        bn.bias.copy_((0.3 * torch.randn(16, generator=gen)).to(DEV))
        bn.running_mean.copy_((0.5 * torch.randn(16, generator=gen)).to(DEV))
        bn.running_var.copy_((0.5 + torch.rand(16, generator=gen)).to(DEV))
    assert block.folds_eval_bn() is False                               # grad mode: not folded

    def reference():
        a = bn.weight.detach().double().cpu() / (bn.running_var.double().cpu() + bn.eps).sqrt()
        w_eff = rounded((c["W0"].double() * a.view(-1, 1, 1, 1)).float(), pname).double()
        b_eff = bn.bias.detach().double().cpu() - bn.running_mean.double().cpu() * a
        return F.leaky_relu(F.conv2d(c["x"].double(), w_eff, b_eff, padding=1), 0.2)

    tol, refs, outs = TOL[pname], [], []
    writes = [lambda: None, lambda: bn.running_var.mul_(16.0), lambda: bn.running_var.data.copy_(bn.running_var.data / 64.0)]
    for write in writes:
        write()
        with torch.no_grad():
            assert block.folds_eval_bn()
            outs.append(nchw(block(nhwc(c["x"], pname))))
        refs.append(reference())
    for i, (got, ref) in enumerate(zip(outs, refs)):
        if i:
            apart = relmax(refs[i - 1], ref)
            note(f"bn fold {pname} write {i}: references before and after {apart:.3g} apart = {apart / tol:.0f} bounds")
            assert apart >= 10 * tol, "a broken case"
        e = relmax(got, ref)
        assert e < tol, f"call {i}: {e:.3g} from float64 on the current running_var (bound {tol})"


def _halo_case(ops, cin, cout, h, w_, n, seed, up=False):
    """integer operands of a 3x3 reflect conv at a halo-kernel shape: x (density 1/2), W0, W1"""
    return ints((n, cin, h, w_), seed, 0.5), ints((cout, cin, 3, 3), seed + 1), ints((cout, cin, 3, 3), seed + 2)


def test_bn_act_conv_reads_the_written_weight(ops, monkeypatch):
    """ops.bn_act_conv (BatchNorm + LeakyReLU on the conv's operand path; ``fuse_pro`` switched on for the test) packs through the
    same cache: after a raw-pointer write of the weight it equals the call on a fresh cache, bit for bit, and differs from its first
    result in at least half of the elements.  64 -> 128 at 8 x 32, the smallest batch halo_conv_shape_ok admits."""
    from de_i2i_gan_amd import optim
    monkeypatch.setattr(ops, "fuse_pro", True)
    n = n_halo8(1, 128)(cu_count())
    x, w0, w1 = _halo_case(ops, 64, 128, 8, 32, n, 61)
    y1 = nhwc(x, "bf16")
    w = torch.nn.Parameter(w0.to(DEV))
    gen = torch.Generator().manual_seed(62)
    bw, bb = (torch.nn.Parameter(t.to(DEV)) for t in (1 + 0.2 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen)))
    geom, cache = ops.ConvGeom(64, 128, 3, 1, 1, True, False), ops.PackedWeights()
    gy = nhwc(ints((n, 128, 8, 32), 63, 0.25), "bf16")
    assert ops.bn_act_conv_supported(y1, bw, w, geom, True), "the gate refuses 64 -> 128 at 8 x 32: name another shape"

    def run(cache):
        rm, rv = torch.zeros(64, device=DEV), torch.ones(64, device=DEV)
        yg = y1.clone().requires_grad_(True)
        _counts()
        out = ops.bn_act_conv(yg, bw, bb, rm, rv, True, "leaky_relu", w, cache, geom)
        fams = _counts()
        dy1, dw = torch.autograd.grad(out, [yg, w], gy)
        torch.cuda.synchronize()
        assert fams.get("halo_conv", 0) + fams.get("halo16_conv", 0) == 1 and "gather_v1" not in fams, fams
        return out.detach(), dy1, dw

    first = run(cache)
    optim.ema_lerp_([w], [w1.to(DEV)], 0.0)
    second, fresh = run(cache), run(ops.PackedWeights())
    assert torch.equal(w.detach().cpu(), w1)
    for name, a, b_, f in zip(("y", "dy1"), first, second, fresh):
        assert differ(a.float().cpu(), f.float().cpu()) >= 0.5, f"a broken case: {name} does not depend on the weight"
        assert torch.equal(b_, f), f"{name} after the write differs from a fresh cache's in {differ(b_.float().cpu(), f.float().cpu()):.3f}"


def test_spade_conv_reads_the_written_weight(ops):
    """ops.spade_conv on an up-sampling block (the ring form, the product's default): the same sequence.  64 -> 128 from 8 x 16 to 16 x 32,
    the smallest batch halo16_shape_ok admits."""
    from de_i2i_gan_amd import optim
    n = n_halo16(1, 128)(cu_count())
    x, w0, w1 = _halo_case(ops, 64, 128, 8, 16, n, 71)
    xs = nhwc(x, "bf16")
    w = torch.nn.Parameter(w0.to(DEV))
    geom, cache = ops.ConvGeom(64, 128, 3, 1, 1, True, True), ops.PackedWeights()
    gb = (0.25 * torch.randn(n, 5, 5, 128, generator=torch.Generator().manual_seed(72))).to(DEV, torch.bfloat16)
    gy = nhwc(ints((n, 128, 16, 32), 73, 0.25), "bf16")
    mode = ops.spade_conv_supported(xs, None, geom, True)
    assert mode is not None, "the gate refuses 64 -> 128 from 8 x 16: name another shape"

    def run(cache):
        xg = xs.clone().requires_grad_(True)
        _counts()
        out = ops.spade_conv(xg, gb, w, cache, geom, mode=mode)
        fams = _counts()
        dx, dw = torch.autograd.grad(out, [xg, w], gy)
        torch.cuda.synchronize()
        assert fams.get("halo_conv", 0) + fams.get("halo16_conv", 0) == 1 and "gather_v1" not in fams, fams
        return out.detach(), dx, dw

    first = run(cache)
    optim.ema_lerp_([w], [w1.to(DEV)], 0.0)
    second, fresh = run(cache), run(ops.PackedWeights())
    assert torch.equal(w.detach().cpu(), w1)
    for name, a, b_, f in zip(("y", "dx"), first, second, fresh):
        assert differ(a.float().cpu(), f.float().cpu()) >= 0.5, f"a broken case: {name} does not depend on the weight"
        assert torch.equal(b_, f), f"{name} after the write differs from a fresh cache's in {differ(b_.float().cpu(), f.float().cpu()):.3f}"


def test_label_path_filters_follow_a_raw_pointer_write(ops):
    """ops.label_gamma_beta keeps the bf16 layouts of every SPADE module's gamma / beta filters in a dict the generator holds
    (``_packed_label_path``), keyed on the filters' stamps.  Two modules, hidden 32, norm_nc 16, integer data: tables and the input
    gradient (the second layout) equal float64 on the filters as they are after ``ema_lerp_`` rewrote them through raw pointers."""
    from de_i2i_gan_amd import optim
    from de_i2i_gan_amd.networks.architecture import Conv2d
    hidden, C, nm, N = 32, 16, 2, 2
    actv = ints((N, nm * hidden, 5, 5), 111, 0.5).abs()
    gys = [ints((N, 2 * C, 5, 5), 112 + i, 0.5) for i in range(nm)]
    W = [[ints((C, hidden, 3, 3), 120 + 10 * v + k) for k in range(2 * nm)] for v in (0, 1)]       # [version][gamma0, beta0, gamma1, beta1]
    B = [ints((C,), 140 + k) for k in range(2 * nm)]
    convs = [(Conv2d(hidden, C, 3, padding="same").to(DEV), Conv2d(hidden, C, 3, padding="same").to(DEV)) for _ in range(nm)]
    flat = [m for pair in convs for m in pair]
    with torch.no_grad():
        for m, w, b in zip(flat, W[0], B):
            m.weight.copy_(w.to(DEV))
            m.bias.copy_(b.to(DEV))

    def reference(ws):
        a = actv.double().requires_grad_(True)
        tabs = [torch.cat([F.conv2d(a[:, i * hidden:(i + 1) * hidden], ws[2 * i + k].double(), B[2 * i + k].double(), padding=1)
                           for k in range(2)], 1) for i in range(nm)]
        (da,) = torch.autograd.grad(tabs, [a], [g.double() for g in gys])
        assert max(t.abs().max() for t in tabs) <= 256 and da.abs().max() <= 256
        return [t.detach() for t in tabs], da

    def run(cache):
        a = nhwc(actv, "bf16").requires_grad_(True)
        assert ops.label_gamma_beta_supported(a, hidden, convs)
        tabs = ops.label_gamma_beta(a, hidden, convs, cache)
        (da,) = torch.autograd.grad(tabs, [a], [nhwc(g, "bf16") for g in gys])
        torch.cuda.synchronize()
        return [nchw(t) for t in tabs], nchw(da)

    ref0, ref1 = reference(W[0]), reference(W[1])
    assert all(differ(x, y) >= 0.5 for x, y in zip(ref0[0], ref1[0])) and differ(ref0[1], ref1[1]) >= 0.5
    cache = {}
    tabs, da = run(cache)
    assert all(torch.equal(t, r) for t, r in zip(tabs, ref0[0])) and torch.equal(da, ref0[1])
    optim.ema_lerp_([m.weight for m in flat], [w.to(DEV) for w in W[1]], 0.0)
    tabs, da = run(cache)
    for i, (t, r) in enumerate(zip(tabs, ref1[0])):
        assert torch.equal(t, r), f"table {i} differs from float64 on the new filters in {differ(t, r):.3f} of its elements"
    assert torch.equal(da, ref1[1]), f"the input gradient differs from float64 on the new filters in {differ(da, ref1[1]):.3f}"


# =====================================================================================================================================
# B. the other caches
# =====================================================================================================================================
def _spectral_eval(conv, xg):
    conv.eval()
    with torch.no_grad():
        return conv(xg).clone()


@pytest.mark.parametrize("iterate_by", ["training_forward", "op"])
def test_frozen_spectral_weight_follows_u_and_v(ops, iterate_by):
    """SpectralConv2d._frozen_weight: an eval no-grad forward, a power iteration of (u, v) -- a training forward, or the op itself on the
    module's buffers, which only the ``mark_written`` stamp reports --, an eval no-grad forward: the last one uses the new (u, v),
    bit-equal to a module built fresh from the same state_dict"""
    from de_i2i_gan_amd.networks.architecture import SpectralConv2d
    w, u, v = spectral_inputs()
    conv = SpectralConv2d(16, 16, 3, padding=1, bias=False).to(DEV)
    conv.load_state_dict({"weight_orig": w, "weight_u": u, "weight_v": v})
    xg = nhwc(integer_case("plain")["x"], "f32")
    first = _spectral_eval(conv, xg)
    assert "_frozen_weight" in conv.__dict__ and torch.equal(_spectral_eval(conv, xg), first)
    if iterate_by == "training_forward":
        conv.train()
        conv(xg)
    else:
        ops.spectral_weight(conv.weight_orig, conv.weight_u, conv.weight_v, True)
        assert "_frozen_weight" in conv.__dict__
    last = _spectral_eval(conv, xg)
    fresh = SpectralConv2d(16, 16, 3, padding=1, bias=False).to(DEV)
    fresh.load_state_dict(conv.state_dict())
    want = _spectral_eval(fresh, xg)
    torch.cuda.synchronize()
    assert differ(first.cpu(), want.cpu()) >= 0.5, "a broken case: the iteration left the weight where it was"
    assert torch.equal(last, want), f"the frozen weight is stale: {differ(last.cpu(), want.cpu()):.3f} of the output differs"


def _labels(seed, n=2):
    lab = torch.zeros(n, 6, 1, 1)
    for j in range(n):
        lab[j, (seed + j) % 6] = 1
    return lab.to(DEV)


@pytest.fixture
def spade(ops, monkeypatch):
    from de_i2i_gan_amd.networks.architecture import SPADE
    torch.manual_seed(81)
    m = SPADE(label_nc=6, norm_nc=16, hidden_nc=8).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(4.0)                   # (the default initialisation gives tables within a bf16 rounding of each other)
    real, calls = m._gamma_beta, []
    monkeypatch.setattr(m, "_gamma_beta", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    m.calls = calls
    return m


def _fresh_spade(spade_mod):
    from de_i2i_gan_amd.networks.architecture import SPADE
    twin = SPADE(label_nc=6, norm_nc=16, hidden_nc=8).to(DEV)
    twin.load_state_dict(spade_mod.state_dict())
    return twin


def _spade_x():
    return nhwc(torch.randn(2, 16, 8, 8, generator=torch.Generator().manual_seed(82)), "bf16")


def test_spade_table_cache_hits_and_misses(ops, spade):
    """SPADE._gb_cache in class mode at 8 x 8: what is served from the memo equals, bit for bit, what a module built fresh from the same
    state_dict computes -- after every event of DESIGN.md's row for this cache"""
    from de_i2i_gan_amd import optim
    x, lab, other = _spade_x(), _labels(0), _labels(3)
    out1 = spade(x, lab)
    assert torch.equal(spade(x, lab), out1) and len(spade.calls) == 1                      # the same label tensor twice: a hit
    with torch.no_grad():
        assert torch.equal(spade(x, lab), out1) and len(spade.calls) == 1                  # no-grad after grad: served by the grad table
    lab.copy_(other)                                                                       # an in-place label change: a miss
    out2 = spade(x, lab)
    want2 = _fresh_spade(spade)(x, other)
    assert len(spade.calls) == 2 and differ_live(out1, want2) >= 0.5
    assert torch.equal(out2, want2)
    for p in spade.parameters():                                                           # a parameter written by FusedAdam: a miss
        p.grad = torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).to(DEV)
    optim.FusedAdam(list(spade.parameters()), lr=0.5).step()
    out3 = spade(x, lab)
    want3 = _fresh_spade(spade)(x, lab)
    torch.cuda.synchronize()
    assert len(spade.calls) == 3 and differ_live(out2, want3) >= 0.5
    assert torch.equal(out3, want3)


def test_spade_grad_call_is_not_served_by_a_no_grad_table(ops, spade):
    x, lab = _spade_x(), _labels(1)
    with torch.no_grad():
        quiet = spade(x, lab)
    assert len(spade.calls) == 1 and not quiet.requires_grad
    out = spade(x, lab)
    assert len(spade.calls) == 2 and out.requires_grad and torch.equal(out, quiet)
    grads = torch.autograd.grad(out.float().sum(), list(spade.parameters()))              # the table carries history
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)


def test_spade_prime_equals_unprimed_calls(ops, spade):
    x, a, b = _spade_x(), _labels(0), _labels(2)
    spade.prime((a, b), ops.BF16)
    assert len(spade.calls) == 1
    got = spade(x, a), spade(x, b)
    assert len(spade.calls) == 1                                                           # both single calls served by the one pass
    twin = _fresh_spade(spade)
    want = twin(x, a), twin(x, b)
    torch.cuda.synchronize()
    assert differ_live(want[0], want[1]) >= 0.5
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_spade_cache_holds_the_dropped_label_tensor(ops, spade):
    x, lab = _spade_x(), _labels(0)
    spade(x, lab)
    old_id = id(lab)
    del lab
    assert [id(seg) for seg, _ in spade._gb_cache.values()] == [old_id]
    later = [_labels(4) for _ in range(32)]
    assert all(id(t) != old_id for t in later)
    out = spade(x, later[0])
    assert len(spade.calls) == 2 and torch.equal(out, _fresh_spade(spade)(x, later[0]))


def _stats_setup(ops):
    """y = conv(x, stats=True) on integer data at the smallest shape whose epilogue leaves statistics records (64 -> 128 at 8 x 32,
    halo_conv_shape_ok's smallest batch) -> (x, w, cache, geom, n)"""
    n = n_halo8(1, 128)(cu_count())
    x, w0, _ = _halo_case(ops, 64, 128, 8, 32, n, 91)
    return nhwc(x, "bf16"), w0.to(DEV), ops.ConvGeom(64, 128, 3, 1, 1, True, False), n


def _count_moments(ops, monkeypatch, t):
    lib, calls = ops._lib_for(t), []
    real = lib.dei2i_moments_partial
    monkeypatch.setattr(lib, "dei2i_moments_partial", lambda *a: (calls.append(1), real(*a))[1])
    return calls


@pytest.mark.parametrize("consumer", ["batchnorm", "instance_norm"])
@pytest.mark.parametrize("touch", ["untouched", "contiguous", "mul_", "add_", "view"])
def test_statistics_records_against_an_in_place_write(ops, monkeypatch, consumer, touch):
    """``_dei2i_stats``: the conv epilogue's moment records ride on y.  Untouched (and through a no-op ``.contiguous()``) the norm that
    follows USES them -- no dei2i_moments_partial launch: the fix must not switch the fusion off --; after ``y.mul_(2)`` / ``y.add_(y)``
    it must measure the tensor itself, and a full view ``y[:]`` does not inherit them.  Either way the result is the float64
    normalisation of the tensor as it is in memory, at test_reduce_edges_gpu.py's bound."""
    xg, w, geom, n = _stats_setup(ops)
    y = ops.conv2d(xg, w, None, ops.PackedWeights(), geom, stats=True)
    assert hasattr(y, "_dei2i_stats"), "the conv left no records: name another shape"
    calls = _count_moments(ops, monkeypatch, y)
    y0 = nchw(y)
    assert y0.abs().max() <= 256 and torch.equal(y0, y0.round())
    if touch == "mul_":
        y.mul_(2)
    elif touch == "add_":
        y.add_(y)
    given = {"contiguous": y.contiguous(), "view": y[:]}.get(touch, y)
    stored = nchw(given)
    assert torch.equal(stored, y0 * (2 if touch in ("mul_", "add_") else 1))
    gen = torch.Generator().manual_seed(92)
    wt, bs = 1 + 0.2 * torch.randn(128, generator=gen), 0.1 * torch.randn(128, generator=gen)
    if consumer == "batchnorm":
        rm, rv = torch.zeros(128, device=DEV), torch.ones(128, device=DEV)
        out = ops.batchnorm_act(given, wt.to(DEV), bs.to(DEV), rm, rv, True, "none")
        ref = F.batch_norm(stored, None, None, wt.double(), bs.double(), True, 0.1, 1e-5)
        stale = F.batch_norm(y0, None, None, wt.double(), bs.double(), True, 0.1, 1e-5) + (stored - y0) * \
            (wt.double() / (y0.var(dim=(0, 2, 3), unbiased=False) + 1e-5).sqrt()).view(1, -1, 1, 1)
    else:
        out = ops.instance_norm_act(given, "none")
        ref = F.instance_norm(stored, eps=1e-5)
        stale = (stored - y0.mean(dim=(2, 3), keepdim=True)) / (y0.var(dim=(2, 3), unbiased=False, keepdim=True) + 1e-5).sqrt()
    torch.cuda.synchronize()
    tol = TOL["bf16"]
    if touch in ("mul_", "add_"):
        apart = relmax(stale, ref)           # what the records of the tensor BEFORE the write would give
        note(f"stats {consumer} {touch}: stale-record and correct references {apart:.3g} apart = {apart / tol:.0f} bounds")
        assert apart >= 10 * tol, "a broken case"
    e = relmax(nchw(out), ref)
    assert e < tol, f"{consumer} after {touch}: {e:.3g} from the float64 normalisation of the stored tensor (bound {tol})"
    assert calls == ([] if touch in ("untouched", "contiguous") else [1]), (touch, "moments passes launched:", len(calls))


@pytest.mark.parametrize("touch", ["untouched", "mul_"])
def test_fp8_activation_copy_against_an_in_place_write(ops, monkeypatch, touch):
    """``_dei2i_fp8``: under ops.fp8_forward a BatchNorm leaves an e4m3 copy of its output for the fp8 conv that reads it.  Untouched the
    conv uses it (no dei2i_quantize_fp8 launch); after ``z.mul_(2)`` it must quantise the tensor itself: bit-equal to the conv of a
    plain tensor of the same values, and far from the conv of the unscaled one."""
    n = n_halo8(1, 128)(cu_count())
    gen = torch.Generator().manual_seed(95)
    yg = nhwc(torch.randn(n, 128, 8, 32, generator=gen), "bf16")
    w = (torch.randn(128, 128, 3, 3, generator=gen) * 0.05).to(DEV)
    geom, cache = ops.ConvGeom(128, 128, 3, 1, 1, True, False), ops.PackedWeights()
    ones, zeros = torch.ones(128, device=DEV), torch.zeros(128, device=DEV)
    lib, calls = ops._lib_for(yg), []
    real = lib.dei2i_quantize_fp8
    monkeypatch.setattr(lib, "dei2i_quantize_fp8", lambda *a: (calls.append(1), real(*a))[1])
    with ops.fp8_forward(True):
        d = ops._desc(ops.BF16, geom, n, 8, 32, 128, 128)
        assert lib.dei2i_conv2d_fp8_supported(byref(d)) == 1, "the gate refuses 128 -> 128 at 8 x 32: name another shape"
        z = ops.batchnorm_act(yg, ones, zeros, zeros.clone(), ones.clone(), True, "none")
        assert hasattr(z, "_dei2i_fp8")
        unscaled = ops.conv2d(z.clone(), w, None, cache, geom)
        assert calls == [1]                                            # (a clone carries no copy)
        if touch == "mul_":
            z.mul_(2)
        _counts()
        out = ops.conv2d(z, w, None, cache, geom)
        fams = _counts()
        want = ops.conv2d(z.clone(), w, None, cache, geom)
    torch.cuda.synchronize()
    assert fams == {"halo_conv_fp8": 1}, fams
    assert len(calls) == (2 if touch == "untouched" else 3), (touch, "quantise launches:", len(calls))
    assert torch.equal(out, want), f"{differ(out.float().cpu(), want.float().cpu()):.3f} of the output differs from the conv of the stored tensor"
    if touch == "mul_":
        assert differ(out.float().cpu(), unscaled.float().cpu()) >= 0.5, "a broken case"


# ---- _PointerTable.cached through FusedAdam ------------------------------------------------------------------------------------
ADAM = dict(lr=0.125, b1=0.5, b2=0.999, eps=1e-8)


def _adam_h(t):
    return dict(lr=f32(ADAM["lr"]), b1=f32(ADAM["b1"]), b2=f32(ADAM["b2"]), eps=f32(ADAM["eps"]), c1=f32(1.0 - ADAM["b1"] ** t),
                c2=f32((1.0 - ADAM["b2"] ** t) ** 0.5), gs=1.0, wd=0.0, alpha=0.0, coupled=False)


def _adam_state(opt, p):
    st = opt.state.get(p)
    if not st:
        return torch.zeros(p.shape), torch.zeros(p.shape)
    return st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone()


def _checked_step(opt, params, t, tag):
    """one FusedAdam.step, every parameter against the float64 formula on the state before the step, at the counted bounds of
    test_optim_edges_gpu.py (k roundings of 2^-24 of the combined magnitudes, every element)"""
    before = [(p.detach().cpu().clone(), p.grad.detach().cpu().clone().contiguous()) + _adam_state(opt, p) for p in params]
    opt.step()
    torch.cuda.synchronize()
    h, k = _adam_h(t), K_ROUND["adam"]
    for p, (p0, g0, m0, v0) in zip(params, before):
        m1, v1 = (opt.state[p][n].cpu() for n in ("exp_avg", "exp_avg_sq"))
        m_ref, v_ref, S_m, S_v = adam_mv(p0, g0, m0, v0, h, torch.float64)
        p_ref, S_p = adam_p(p0, m1, v1, h, torch.float64)
        for name, got, ref, S in (("m", m1, m_ref, S_m), ("v", v1, v_ref, S_v), ("p", p.detach().cpu(), p_ref, S_p)):
            e = worst(got, ref, S)
            assert e <= k[name], (tag, f"step {t}", name, p.numel(), e, k[name])
        assert not torch.equal(p.detach().cpu(), p0), (tag, "a broken case: the step moved nothing")


def _adam_params():
    gen = torch.Generator().manual_seed(101)
    return [torch.nn.Parameter((torch.randn(n, generator=gen) * 0.5).to(DEV)) for n in (1027, 5)]


def _grads(params, seed):
    gen = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen).to(DEV)


def test_adam_pointer_table_follows_moved_gradients(ops):
    """``_PointerTable.cached``: three steps; ``zero_grad(set_to_none=True)`` and fresh gradient tensors between steps 1 and 2, a gradient
    installed from a non-contiguous view (the table holds a contiguous copy's address) between steps 2 and 3"""
    from de_i2i_gan_amd import optim
    params = _adam_params()
    opt = optim.FusedAdam(params, lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"])
    _grads(params, 102)
    _checked_step(opt, params, 1, "first")
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in params)
    keep = [torch.empty(4096, device=DEV) for _ in range(4)]             # (so that the allocator hands the gradients other addresses)
    _grads(params, 103)
    _checked_step(opt, params, 2, "after set_to_none")
    gen = torch.Generator().manual_seed(104)
    wide = [torch.randn(p.numel(), 2, generator=gen).to(DEV) for p in params]
    for p, wd_ in zip(params, wide):
        p.grad = wd_[:, 0]
        assert not p.grad.is_contiguous()
    _checked_step(opt, params, 3, "strided gradient")
    del keep


def test_adam_pointer_table_follows_a_moved_parameter(ops):
    """two steps with ``p.data = p.data.clone()`` in between: the second step updates the NEW storage (float64 Adam at the counted
    bounds) and leaves the old one, which the test holds, bit-unchanged -- a stale table would update memory nobody reads"""
    from de_i2i_gan_amd import optim
    params = _adam_params()
    opt = optim.FusedAdam(params, lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]), eps=ADAM["eps"])
    _grads(params, 105)
    _checked_step(opt, params, 1, "first")
    old = [p.data for p in params]
    snapshot = [t.clone() for t in old]
    for p in params:
        p.data = p.data.clone()
    assert all(p.data_ptr() != o.data_ptr() for p, o in zip(params, old))
    _checked_step(opt, params, 2, "after the move")
    assert all(torch.equal(o, s) for o, s in zip(old, snapshot)), "the step wrote the storage the parameter had left"


# ---- _workspace ------------------------------------------------------------------------------------------------------------------
def _ws_run(ops, name, caches, pname="bf16"):
    c = integer_case(name)
    n, cin, cout = c["x"].shape[0], c["x"].shape[1], c["W1"].shape[0]
    w = c["W1"].to(DEV)
    geom = ops.ConvGeom(cin, cout, 3, 1, 1, False, False)
    _counts()
    y = ops.conv2d(nhwc(c["x"], pname), w, None, caches.setdefault(name, ops.PackedWeights()), geom)
    return y, _counts()


def test_split_k_workspace_grows_and_is_kept_per_stream(ops):
    """``ops._workspace``: a conv that takes gather_v1 with split-K (test_conv_exact_gpu.py's a-nk4-co72), a larger one whose 16 slabs
    do not fit the slot (it grows: a new buffer), the first again; then the same on a non-default stream, which gets a slot of its own"""
    key = (torch.device(DEV), "splitk")
    ops._workspaces.pop(key, None)                                     # (an earlier test of the process may have grown it already)
    caches = {}
    y, fams = _ws_run(ops, "splitk", caches)
    assert fams == {"gather_v1": 1, "splitk_finalize": 1}, fams
    small = ops._workspaces[key]
    assert torch.equal(nchw(y), integer_case("splitk")["y1"])
    y, fams = _ws_run(ops, "grow", caches)
    assert fams.get("splitk_finalize") == 1 and set(fams) <= {"gather_v1", "splitk_finalize"}, fams
    grown = ops._workspaces[key]
    assert grown is not small and grown.numel() > small.numel(), "the larger conv fits the slot: name a larger one"
    assert torch.equal(nchw(y), integer_case("grow")["y1"])
    y, _ = _ws_run(ops, "splitk", caches)
    assert ops._workspaces[key] is grown and torch.equal(nchw(y), integer_case("splitk")["y1"])

    before = set(ops._workspaces)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = [_ws_run(ops, name, caches)[0] for name in ("splitk", "grow", "splitk")]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    added = set(ops._workspaces) - before
    assert added == {key + (side.cuda_stream,)}, added
    assert ops._workspaces[key] is grown
    for name, y in zip(("splitk", "grow", "splitk"), outs):
        assert torch.equal(nchw(y), integer_case(name)["y1"]), name
