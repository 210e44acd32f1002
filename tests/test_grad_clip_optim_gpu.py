"""``FusedAdam(max_grad_norm=c)``: global-norm clipping inside the fused update (optim.py, csrc/adam.hip) against
``torch.nn.utils.clip_grad_norm_`` followed by torch.optim.Adam / AdamW-by-hand on ``grad_scale * g``, eager and captured.

Tolerances.  Parameters: the ``maxrel < 2e-6`` of test_adam_dev_gpu.py without clipping -- the clip scale perturbs g by a few 2^-24
relative, which moves p by lr times that.  ``optimizer.grad_norm``: the bound of test_grad_clip_kernel_gpu.py, k * 2^-24 relative with
k = (chain + 9) / 2 + 1; at SHAPES the longest tensor (3072 elements) sizes a grid of 3 workgroups a row, every row fits one float4
trip and a tail element, chain = 5, k = 8."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(7,), (3, 5, 2, 2), (129,), (64, 3, 4, 4), (1,), (1000,)]        # test_adam_dev_gpu.py's
U = 2.0 ** -24
K_NORM = (5 + 9) / 2 + 1
AMPS = [0.2, 3.0, 0.3, 2.0, 0.1, 4.0]          # per-step gradient scale: |0.5 g| is about 33 x these, on both sides of C
C = 30.0


def maxrel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-12)).item()


def note(*a):
    print("[grad-clip-optim]", *a, flush=True)


def fresh(seed=3):
    torch.manual_seed(seed)
    return [torch.randn(s, device=DEV) for s in SHAPES]


def grads_at(t, shapes=SHAPES):
    gen = torch.Generator(device=DEV).manual_seed(100 + t)
    return [torch.randn(s, device=DEV, generator=gen) * AMPS[t % len(AMPS)] for s in shapes]


def reference_step(ref, topt, grads, gscale, c, lr, wd, coupled):
    """clip_grad_norm_ on gscale * g, then torch.optim.Adam (its own weight decay when coupled, AdamW's by hand otherwise)"""
    with torch.no_grad():
        for r, g in zip(ref, grads):
            r.grad = None if g is None else g * gscale
    norm = torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], c)
    with torch.no_grad():
        if not coupled:
            for r in ref:
                if r.grad is not None:
                    r.mul_(1.0 - lr * wd)
    topt.step()
    return norm


@pytest.mark.parametrize("coupled", [False, True])
def test_clipped_steps_match_torch(coupled):
    from de_i2i_gan_amd.optim import FusedAdam
    lr, wd, gscale = 2e-4, 1e-2, 0.5
    p0 = fresh()
    mine = [torch.nn.Parameter(t.clone()) for t in p0]
    ref = [t.clone().requires_grad_(True) for t in p0]
    opt = FusedAdam(mine, lr=lr, betas=(0.5, 0.999), weight_decay=wd, decoupled=not coupled, grad_scale=gscale, max_grad_norm=C)
    topt = torch.optim.Adam(ref, lr=lr, betas=(0.5, 0.999), eps=1e-8, weight_decay=wd if coupled else 0.0)
    assert opt.grad_norm is None
    norms, worst = [], 0.0
    for t in range(6):
        grads = grads_at(t)
        keep = [g.clone() for g in grads]
        for p, g in zip(mine, grads):
            p.grad = g
        opt.step()
        for p, g, k in zip(mine, grads, keep):
            assert p.grad is g and torch.equal(g, k)                 # gradients are never written
        want = reference_step(ref, topt, grads, gscale, C, lr, wd, coupled)
        got = opt.grad_norm
        assert got.shape == (1,) and got.device.type == "cuda"
        err = abs(float(got) - float(want)) / float(want)
        worst = max(worst, err / U)
        assert err <= K_NORM * U, (t, float(got), float(want))
        norms.append(float(want))
    note(f"coupled={coupled}: norms {[round(n, 2) for n in norms]}, grad_norm vs clip_grad_norm_: worst {worst:.3f} u (bound {K_NORM} u)")
    assert any(n > C for n in norms) and any(n < C for n in norms)   # some steps clip, some do not
    for a, r in zip(mine, ref):
        assert maxrel(a.detach(), r.detach()) < 2e-6


@pytest.mark.parametrize("wd,decoupled", [(0.0, True), (1e-2, True), (1e-2, False)])
def test_a_huge_max_grad_norm_is_bitwise_no_clipping(wd, decoupled):
    from de_i2i_gan_amd.optim import FusedAdam
    p0 = fresh()
    a = [torch.nn.Parameter(t.clone()) for t in p0]
    b = [torch.nn.Parameter(t.clone()) for t in p0]
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=wd, decoupled=decoupled, grad_scale=0.5)
    oa, ob = FusedAdam(a, **kw), FusedAdam(b, max_grad_norm=1e30, **kw)
    for t in range(3):
        for x, y, g in zip(a, b, grads_at(t)):
            x.grad, y.grad = g, g.clone()
        oa.step()
        ob.step()
        for x, y in zip(a, b):
            assert torch.equal(x, y), t
            assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]), t
            assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"]), t
            assert oa.state[x]["step"] == ob.state[y]["step"] == t + 1
    assert oa.grad_norm is None and float(ob.grad_norm) > 0


def test_two_param_groups_share_one_norm_and_a_missing_gradient_is_skipped():
    """The norm is over every parameter of the optimizer with a gradient, across param groups (two launches, one scale); a parameter
    whose grad is None is left out of the norm and gets no state."""
    from de_i2i_gan_amd.optim import FusedAdam
    lr, gscale, skip = 2e-4, 0.5, 2
    p0 = fresh()
    mine = [torch.nn.Parameter(t.clone()) for t in p0]
    ref = [t.clone().requires_grad_(True) for t in p0]
    opt = FusedAdam([{"params": mine[:3]}, {"params": mine[3:], "lr": 5e-5}], lr=lr, betas=(0.5, 0.999), grad_scale=gscale, max_grad_norm=C)
    topt = torch.optim.Adam([{"params": ref[:3]}, {"params": ref[3:], "lr": 5e-5}], lr=lr, betas=(0.5, 0.999), eps=1e-8)
    clipped = 0
    for t in range(1, 4):
        grads = grads_at(t)
        grads[skip] = None
        for p, g in zip(mine, grads):
            p.grad = g
        opt.step()
        want = reference_step(ref, topt, grads, gscale, C, lr, 0.0, True)
        exact = torch.cat([g.double().flatten() for g in grads if g is not None]).norm().item() * gscale
        assert abs(float(opt.grad_norm) - exact) <= K_NORM * U * exact
        assert abs(float(opt.grad_norm) - float(want)) <= K_NORM * U * float(want)
        alone = torch.cat([g.double().flatten() for g in grads[:3] if g is not None]).norm().item() * gscale
        assert alone < 0.5 * exact                                   # (a per-group norm would be far off)
        clipped += float(want) > C
    assert clipped >= 1
    assert len(opt.state[mine[skip]]) == 0 and torch.equal(mine[skip], p0[skip])
    for i, (a, r) in enumerate(zip(mine, ref)):
        assert maxrel(a.detach(), r.detach()) < 2e-6, i


def test_a_non_contiguous_gradient_is_copied_once_for_norm_and_update():
    from de_i2i_gan_amd.optim import FusedAdam
    p0 = fresh()
    a = [torch.nn.Parameter(t.clone()) for t in p0]
    b = [torch.nn.Parameter(t.clone()) for t in p0]
    kw = dict(lr=2e-4, betas=(0.5, 0.999), grad_scale=0.5, max_grad_norm=C)
    oa, ob = FusedAdam(a, **kw), FusedAdam(b, **kw)
    for t in (1, 3):                                                 # (AMPS: both clip)
        grads = grads_at(t)
        strided = torch.randn(4, 4, 3, 64, device=DEV).mul_(AMPS[t]).permute(3, 2, 1, 0)      # SHAPES[3], not contiguous
        assert strided.shape == SHAPES[3] and not strided.is_contiguous()
        before = strided.clone()
        for i, (x, y, g) in enumerate(zip(a, b, grads)):
            x.grad = strided if i == 3 else g
            y.grad = strided.contiguous() if i == 3 else g.clone()
        oa.step()
        ob.step()
        assert a[3].grad is strided and torch.equal(strided, before) and not strided.is_contiguous()
        assert torch.equal(oa.grad_norm, ob.grad_norm) and float(oa.grad_norm) > C
        for x, y in zip(a, b):
            assert torch.equal(x, y)
            assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"])
            assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])


@pytest.mark.parametrize("wd,decoupled", [(0.0, True), (1e-2, True), (1e-2, False)])
def test_captured_clipped_step_equals_eager(wd, decoupled):
    """test_adam_dev_gpu.py's test_captured_fused_adam_step_equals_eager with clipping on: bitwise equal parameters, moments, steps and
    grad_norm over 12 steps with an lr change; changing max_grad_norm after the capture is refused by graph_prepare."""
    from de_i2i_gan_amd.optim import FusedAdam
    p0 = fresh(5)
    pe = [torch.nn.Parameter(t.clone()) for t in p0]
    pg = [torch.nn.Parameter(t.clone()) for t in p0]
    kw = dict(lr=2e-4, betas=(0.5, 0.999), weight_decay=wd, decoupled=decoupled, grad_scale=0.5, max_grad_norm=C)
    oe, og = FusedAdam(pe, **kw), FusedAdam(pg, **kw)
    grads = [torch.empty_like(t) for t in p0]

    def new_grads(t):
        for g, fresh_g in zip(grads, grads_at(t)):
            g.copy_(fresh_g)
        for a, b, g in zip(pe, pg, grads):
            a.grad = g.clone()
            b.grad = g                     # (the captured table points at these buffers)

    def check(t):
        torch.cuda.synchronize()
        assert torch.equal(oe.grad_norm, og.grad_norm), t
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
    norm_buffer = og.grad_norm.data_ptr()
    graph = torch.cuda.CUDAGraph()
    og.graph_reserve()
    with torch.cuda.graph(graph):
        og.step()
    plan = og.graph_take_plan()
    assert plan and all(s["step"] == 2 for s in og.state.values())      # the capture ran nothing
    assert og.grad_norm.data_ptr() == norm_buffer                        # the eager steps' buffers, not the graph pool's
    seen = []
    for t in range(3, 15):
        if t == 9:
            for o in (oe, og):
                o.param_groups[0]["lr"] = 5e-5
        new_grads(t)
        oe.step()
        if t == 11:
            og.step()                      # an eager step between replays
        else:
            og.graph_prepare(plan)
            graph.replay()
            og.graph_finish(plan)
        check(t)
        seen.append(float(og.grad_norm))
    assert any(n > C for n in seen) and any(n < C for n in seen)
    og.max_grad_norm = 2 * C
    with pytest.raises(RuntimeError, match="release_graphs"):
        og.graph_prepare(plan)
    og.max_grad_norm = None
    with pytest.raises(RuntimeError, match="release_graphs"):
        og.graph_prepare(plan)
    og.max_grad_norm = C
    og.grad_scale = 0.25
    with pytest.raises(RuntimeError, match="release_graphs"):
        og.graph_prepare(plan)

