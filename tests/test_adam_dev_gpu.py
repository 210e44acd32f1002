"""dei2i_adam_step_dev / dei2i_adam_step_l2_dev (csrc/adam.hip): the hyper-parameters from a device table indexed by a device
counter, bitwise equal to the argument forms over 20 steps with a changing lr, a table refresh in between (8-row tables),
grad_scale != 1 and weight decay; and torch.optim.Adam within FusedAdam's tolerance.  FusedAdam.step() captured and replayed
equals eager steps bit for bit, also when one param group splits into two launch groups (with and without max_grad_norm)."""
import ctypes

import pytest
import torch

from de_i2i_gan_amd import _lib as L
from de_i2i_gan_amd import ops
from de_i2i_gan_amd.optim import _HyperTable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(7,), (3, 5, 2, 2), (129,), (64, 3, 4, 4), (1,), (1000,)]


def maxrel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


def table(ps, gs, ms, vs):
    rows = [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, g, m, v in zip(ps, gs, ms, vs)]
    return torch.tensor(rows, dtype=torch.int64).to(DEV), max(r[4] for r in rows)


def lr_at(step):
    return 2e-4 if step < 10 else 5e-5 * (1 + step % 3)


@pytest.mark.parametrize("coupled", [False, True])
def test_dev_forms_equal_argument_forms(coupled):
    torch.manual_seed(3)
    lib = L.load()
    ops._lib_for(torch.empty(1, device=DEV))
    b1, b2, eps, gscale, wd = 0.5, 0.999, 1e-8, 0.5, 1e-2
    p0 = [torch.randn(s, device=DEV) for s in SHAPES]
    A = [[t.clone() for t in p0], [torch.zeros_like(t) for t in p0], [torch.zeros_like(t) for t in p0]]
    B = [[t.clone() for t in p0], [torch.zeros_like(t) for t in p0], [torch.zeros_like(t) for t in p0]]
    grads = [torch.empty_like(t) for t in p0]
    ta, n = table(A[0], grads, A[1], A[2])
    tb, _ = table(B[0], grads, B[1], B[2])
    hyper = _HyperTable(torch.device(DEV), 1, rows=8)
    ref = [t.clone().requires_grad_(True) for t in p0]
    topt = torch.optim.Adam(ref, lr=lr_at(1), betas=(b1, b2), eps=eps, weight_decay=wd if coupled else 0.0)
    refreshes = 0
    for t in range(1, 21):
        for g in grads:
            g.normal_()
        lr = lr_at(t)
        # argument form, exactly FusedAdam._launch's arguments
        fn = lib.dei2i_adam_step_l2 if coupled else lib.dei2i_adam_step
        L.check(fn(ctypes.c_void_p(ta.data_ptr()), len(SHAPES), n, lr, b1, b2, eps, 1.0 - b1 ** t, (1.0 - b2 ** t) ** 0.5, gscale,
                   wd, ops._stream()), "adam_step")
        # device-table form
        host = hyper._host
        hyper.ensure(t, lr, b1, b2, 0.0 if coupled else wd)
        refreshes += hyper._host is not host
        if coupled:
            rc = lib.dei2i_adam_step_l2_dev(ctypes.c_void_p(tb.data_ptr()), len(SHAPES), n, ctypes.c_void_p(hyper.table.data_ptr()),
                                            ctypes.c_void_p(hyper.index.data_ptr()), hyper.rows, b1, b2, eps, gscale, wd, ops._stream())
        else:
            rc = lib.dei2i_adam_step_dev(ctypes.c_void_p(tb.data_ptr()), len(SHAPES), n, ctypes.c_void_p(hyper.table.data_ptr()),
                                         ctypes.c_void_p(hyper.index.data_ptr()), hyper.rows, b1, b2, eps, gscale, ops._stream())
        L.check(rc, "adam_step_dev")
        L.check(lib.dei2i_index_advance(ctypes.c_void_p(hyper.index.data_ptr()), ops._stream()), "index_advance")
        hyper.advance()
        for x, y in zip(A, B):
            for a, b in zip(x, y):
                assert torch.equal(a, b), t
        # torch.optim.Adam: AdamW-style decay by hand for the decoupled form
        for group in topt.param_groups:
            group["lr"] = lr
        with torch.no_grad():
            for r, g in zip(ref, grads):
                r.grad = g * gscale
                if not coupled:
                    r.mul_(1.0 - lr * wd)
        topt.step()
    assert refreshes >= 3                         # the first upload, the lr changes and the end of the 8 rows
    assert int(hyper.index.item()) == hyper.t - hyper.t0
    for a, r in zip(A[0], ref):
        assert maxrel(a, r.detach()) < 2e-6


def test_index_outside_rows_leaves_tensors():
    lib = L.load()
    p = torch.randn(300, device=DEV)
    g, m, v = torch.randn_like(p), torch.zeros_like(p), torch.zeros_like(p)
    tab, n = table([p], [g], [m], [v])
    hyper = _HyperTable(torch.device(DEV), 1, rows=2)
    hyper.ensure(1, 1e-3, 0.9, 0.999, 0.0)
    hyper.index.fill_(2)
    before = p.clone()
    L.check(lib.dei2i_adam_step_dev(ctypes.c_void_p(tab.data_ptr()), 1, n, ctypes.c_void_p(hyper.table.data_ptr()),
                                    ctypes.c_void_p(hyper.index.data_ptr()), hyper.rows, 0.9, 0.999, 1e-8, 1.0, ops._stream()), "dev")
    assert torch.equal(p, before) and not m.any()


@pytest.mark.parametrize("wd,decoupled", [(0.0, True), (1e-2, True), (1e-2, False)])
def test_captured_fused_adam_step_equals_eager(wd, decoupled):
    """FusedAdam.step() recorded into a graph and replayed (graph_prepare / replay / graph_finish) against eager steps of a twin
    optimizer: bitwise equal parameters, moments and state["step"] over 20 steps with an lr change and one eager step of the
    captured optimizer in between (the replays after it pick up its step count)."""
    from de_i2i_gan_amd.optim import FusedAdam
    torch.manual_seed(5)
    p0 = [torch.randn(s, device=DEV) for s in SHAPES]
    pe = [torch.nn.Parameter(t.clone()) for t in p0]
    pg = [torch.nn.Parameter(t.clone()) for t in p0]
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=wd, decoupled=decoupled, grad_scale=0.5)
    oe, og = FusedAdam(pe, **kw), FusedAdam(pg, **kw)
    grads = [torch.empty_like(t) for t in p0]

    def new_grads(t):
        gen = torch.Generator(device=DEV).manual_seed(100 + t)
        for g in grads:
            g.copy_(torch.randn(g.shape, device=DEV, generator=gen))
        for a, b, g in zip(pe, pg, grads):
            a.grad = g.clone()
            b.grad = g                     # (the captured table points at these buffers)

    def check(t):
        torch.cuda.synchronize()
        for a, b in zip(pe, pg):
            assert torch.equal(a, b), t
            sa, sb = oe.state[a], og.state[b]
            assert sa["step"] == sb["step"], t
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), t

    for t in range(1, 3):                  # eager warm-up: the state exists before the capture
        new_grads(t)
        oe.step()
        og.step()
    check(2)
    graph = torch.cuda.CUDAGraph()
    og.graph_reserve()
    with torch.cuda.graph(graph):
        og.step()
    plan = og.graph_take_plan()
    assert plan and all(s["step"] == 2 for s in og.state.values())      # the capture ran nothing
    for t in range(3, 23):
        if t == 9:
            for o in (oe, og):
                o.param_groups[0]["lr"] = 5e-5
        new_grads(t)
        oe.step()
        if t == 14:
            og.step()                      # an eager step between replays
        else:
            og.graph_prepare(plan)
            graph.replay()
            og.graph_finish(plan)
        check(t)


SPLIT_NUMELS = [3, 8, 13, 2053]            # the scalar loop only, the float4 loop only, both, and three workgroups in x
LAGGING = 2                                # the 13-element parameter: no gradient on the first step


@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
@pytest.mark.parametrize("decoupled", [True, False])
def test_captured_step_of_a_split_param_group_equals_eager(decoupled, max_grad_norm):
    """One param group whose parameters stand at two step counts (one of them got its first gradient a step late) makes two
    launch groups, each with its own reserved pointer table and hyper-parameter rows, and with ``max_grad_norm`` one norm over
    both.  Captured and replayed 5 times with an lr change, against eager steps of a twin: bitwise equal parameters, moments,
    ``state["step"]`` and ``grad_norm``.  (|0.5 g| is about 23 x the step's amplitude: on both sides of 0.5.)"""
    from de_i2i_gan_amd.optim import FusedAdam
    torch.manual_seed(7)
    p0 = [torch.randn(n, device=DEV) for n in SPLIT_NUMELS]
    pe = [torch.nn.Parameter(t.clone()) for t in p0]
    pg = [torch.nn.Parameter(t.clone()) for t in p0]
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=1e-2, decoupled=decoupled, grad_scale=0.5, max_grad_norm=max_grad_norm)
    oe, og = FusedAdam(pe, **kw), FusedAdam(pg, **kw)
    grads = [torch.empty_like(t) for t in p0]

    def new_grads(t, skip=()):
        gen = torch.Generator(device=DEV).manual_seed(200 + t)
        for i, (a, b, g) in enumerate(zip(pe, pg, grads)):
            g.copy_(torch.randn(g.shape, device=DEV, generator=gen) * (1.0 if t % 2 else 0.01))
            a.grad = None if i in skip else g.clone()
            b.grad = None if i in skip else g       # (the captured tables point at these buffers)

    def check(t):
        torch.cuda.synchronize()
        if max_grad_norm is None:
            assert oe.grad_norm is None and og.grad_norm is None
        else:
            assert torch.equal(oe.grad_norm, og.grad_norm), t
        for a, b in zip(pe, pg):
            assert torch.equal(a, b), t
            sa, sb = oe.state[a], og.state[b]
            assert sa["step"] == sb["step"], t
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), t

    for t in range(1, 3):                  # eager warm-up: every parameter has its state before the capture
        new_grads(t, skip=(LAGGING,) if t == 1 else ())
        oe.step()
        og.step()
    check(2)
    assert [og.state[p]["step"] for p in pg] == [2, 2, 1, 2]
    graph = torch.cuda.CUDAGraph()
    og.graph_reserve()
    with torch.cuda.graph(graph):
        og.step()
    plan = og.graph_take_plan()
    assert len(plan) == 2                                                # two launch groups of one param group
    assert [og.state[p]["step"] for p in pg] == [2, 2, 1, 2]             # the capture ran nothing
    seen = []
    for t in range(3, 8):
        if t == 5:
            for o in (oe, og):
                o.param_groups[0]["lr"] = 5e-5
        new_grads(t)
        oe.step()
        og.graph_prepare(plan)
        graph.replay()
        og.graph_finish(plan)
        check(t)
        if max_grad_norm is not None:
            seen.append(float(og.grad_norm))
    assert [og.state[p]["step"] for p in pg] == [7, 7, 6, 7]
    if max_grad_norm is not None:
        assert any(n > max_grad_norm for n in seen) and any(n < max_grad_norm for n in seen)
