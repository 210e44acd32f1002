"""``opt.max_grad_norm`` in the DefectGanTrainer / MAETrainer step at the smallest golden configurations (t0_img32_b2,
m0_img32_b2_position): against the same trainer without the option and ``torch.nn.utils.clip_grad_norm_`` applied by hand before
every ``optimizer.step``; the graph_step twin against the eager twin, bit for bit (the recorded norms included); the MAE stage under
``opt.grad_scaler``; the refusals.

Tolerances.  Post-Adam parameters in f32: test_model_gpu.py's -- norms of every tensor within 1e-3 (its ``maxrel``), every element
within 5 lr.  Adam is nearly invariant to the scale of its gradient, so the parameters alone would hardly tell a clipped run from an
unclipped one: the first moments, which carry the clip factor (0.0038 for G, 0.69 for D at the first update), are held to the same
1e-3 after the first step, as the relative L2 distance over all tensors of an optimizer (a bias in front of an InstanceNorm has a
gradient of pure rounding noise, which no two runs share; it does not weigh in that measure).  The recorded norm against the float64 norm
of the hand-clipped twin's gradients: at the very first D update both twins hold the same weights, so the bound is the kernel test's
k * 2^-24 with k = (chain + 9) / 2 + 1 = 8 (every tensor of these networks fits one float4 trip of its launch and a tail element:
chain = 5, asserted below); afterwards the twins' parameters agree to 1e-3 and so do the norms.  The MAE pair with and without the
GradScaler: test_mae_gpu.py's for that pair -- parameter norms within 1e-3, the mask token within two sign-like steps (4 lr + 1e-6).

MAX_NORM sits below the norms the first steps measure at these configurations (printed by the tests: DESIGN.md section 7); every
test asserts that the recorded norm exceeded it."""
import numpy as np
import pytest
import torch

import test_graph_mae_gpu as GM
import test_graph_step_gpu as GS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)        # t0_img32_b2 / m0_img32_b2_position (GM.MAE)
U = 2.0 ** -24
# measured over the first 9 steps without clipping, f32 and bf16 alike: defectGAN D 0.0058 .. 0.019, G 1.04 .. 1.48; MAE D 0.0106 .. 0.0145,
# G 0.53 .. 0.99 -- one option serves every optimizer of a trainer, so it sits below D's
MAX_NORM = {"gan": 0.004, "mae": 0.008}
MAE_OVER = dict(mask_rng="device", mask_seed=GM.SEED)


def note(*a):
    print("[grad-clip-trainer]", *a, flush=True)


def maxrel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def clip_by_hand(tr, max_norm):
    """What a user writes today: clip_grad_norm_ over the optimizer's parameters right before each optimizer.step().  -> {name: [the
    float64 norm of the gradients before clipping, per update]}"""
    log = {}
    for name, o in tr.optimizers.items():
        def step(*a, _o=o, _step=o.step, _log=log.setdefault(name, []), **k):
            params = [p for g in _o.param_groups for p in g["params"] if p.grad is not None]
            _log.append(torch.cat([p.grad.double().flatten() for p in params]).norm().item())
            torch.nn.utils.clip_grad_norm_(params, max_norm)
            return _step(*a, **k)
        o.step = step
    return log


def trained_tensors(tr):
    out = {}
    for name, o in tr.optimizers.items():
        for gi, group in enumerate(o.param_groups):
            for pi, p in enumerate(group["params"]):
                out[f"{name}.{gi}.{pi}"] = (p.detach(), o.state[p].get("exp_avg") if o.state.get(p) else None)
    return out


def assert_tracks(clipped, by_hand, lr):
    a, b = trained_tensors(clipped), trained_tensors(by_hand)
    assert a.keys() == b.keys() and len(a) > 10
    pn = np.array([[float(x[k][0].double().norm()) for k in a] for x in (a, b)])
    assert maxrel(pn[0], pn[1]) < 1e-3
    for k in a:
        assert (a[k][0] - b[k][0]).abs().max().item() <= 5 * lr, k


def assert_moments_track(clipped, by_hand):
    a, b = trained_tensors(clipped), trained_tensors(by_hand)
    for name in clipped.optimizers:
        keys = [k for k in a if k.startswith(name + ".") and a[k][1] is not None]
        assert len(keys) >= 5 and all(b[k][1] is not None for k in keys)
        x = torch.cat([a[k][1].double().flatten() for k in keys])
        y = torch.cat([b[k][1].double().flatten() for k in keys])
        dist = ((x - y).norm() / y.norm()).item()
        note(f"first moments of {name} after the first step, clipped vs by hand: relative L2 distance {dist:.2e}")
        assert dist < 1e-3, name


def check_chain(tr):
    """every launch of these networks runs one float4 trip and at most one tail element per thread: chain = 5, k = 8"""
    for o in tr.optimizers.values():
        for group in o.param_groups:
            longest = max(p.numel() for p in group["params"])
            assert longest <= 524288                                  # (one grid-stride trip)


def eager_pair(build, run, kind, steps=3, **over):
    c = MAX_NORM[kind]
    clipped = build(T0, "f32", max_grad_norm=c, **over)
    by_hand = build(T0, "f32", **over)
    assert "grad_norm" in clipped.loss_types and "grad_norm" not in by_hand.loss_types
    assert all(o.max_grad_norm == c for o in clipped.optimizers.values())
    assert all(o.max_grad_norm is None for o in by_hand.optimizers.values())
    check_chain(clipped)
    log = clip_by_hand(by_hand, c)
    # in turn, step by step: nothing in these configurations draws from an RNG the twins share (no noise, no DiffAugment; the MAE
    # masks come from each model's own seeded generator)
    for i, _ in zip(run(clipped, T0, steps), run(by_hand, T0, steps)):
        if i == 0:
            assert_moments_track(clipped, by_hand)
    clipped.flush_losses()
    by_hand.flush_losses()
    rec = clipped.losses["grad_norm"]
    assert sorted(rec) == ["D", "G"] and len(rec["D"]) == len(rec["G"]) == steps          # one entry per D and per G update
    assert "grad_norm" not in by_hand.losses and sorted(by_hand.losses) == sorted(by_hand.loss_types)
    note(f"{kind} f32 recorded norms D {rec['D']} G {rec['G']} (max_grad_norm {c}); by hand, float64: D {log['D']} G {log['G']}")
    first = abs(rec["D"][0] - log["D"][0]) / log["D"][0]
    note(f"{kind} first D update: recorded vs float64 {first / U:.3f} u (bound 8 u)")
    assert first <= 8 * U
    for name in ("D", "G"):
        assert len(log[name]) == steps
        assert maxrel(rec[name], log[name]) < 1e-3, name
        assert max(rec[name]) > c, name                               # the option did clip
    return clipped, by_hand


# ---- DefectGanTrainer -----------------------------------------------------------------------------------------------------
def test_defectgan_eager_matches_clip_grad_norm_by_hand():
    clipped, by_hand = eager_pair(GS.build, GS.run, "gan")
    assert_tracks(clipped, by_hand, lr=2e-4)
    assert sorted(by_hand.losses) == ["aux", "clf", "gan"]             # the option off: exactly the keys there were
    assert sorted(clipped.losses) == ["aux", "clf", "gan", "grad_norm"]


def test_defectgan_graph_twin_is_bitwise_the_eager_twin():
    """num_critics = 2: the D graph and the D + G graph are both replayed; the snapshots hold every parameter, buffer, moment, step
    count and loss list -- the recorded norms among them"""
    tr = GS.compare(T0, steps=9, num_critics=2, expect_graphs=2, max_grad_norm=MAX_NORM["gan"])
    rec = tr.losses["grad_norm"]
    assert len(rec["D"]) == 9 and len(rec["G"]) == 4
    assert max(rec["D"]) > MAX_NORM["gan"] and max(rec["G"]) > MAX_NORM["gan"]


def test_changing_the_option_after_the_capture_is_refused():
    tr = GS.build(T0, "bf16", graph_step=True, graph_warmup=2, max_grad_norm=MAX_NORM["gan"])
    for _ in GS.run(tr, T0, 4):
        pass
    tr.optimizers["D"].max_grad_norm = 2 * MAX_NORM["gan"]
    bg, lab, df = (t.to(DEV) for t in GS.batch(T0, 9))
    with pytest.raises(RuntimeError, match="release_graphs"):
        tr.step(bg, lab, df)
    tr.release_graphs()
    tr.step(bg, lab, df)                                               # (warms up and captures again)
    tr.release_graphs()


# ---- MAETrainer -----------------------------------------------------------------------------------------------------------
def test_mae_eager_matches_clip_grad_norm_by_hand():
    clipped, by_hand = eager_pair(GM.build, GM.run, "mae", **MAE_OVER)
    assert len(clipped.optimizers["G"].param_groups) == 2              # the mask token: one norm with the generator's
    assert_tracks(clipped, by_hand, lr=1.5e-4)
    assert sorted(by_hand.losses) == ["clf", "gan", "rec"]


def test_mae_graph_twin_is_bitwise_the_eager_twin():
    tr = GM.compare(T0, steps=9, num_critics=2, expect_graphs=2, draws_per_step=lambda steps: steps + steps // 2,
                    max_grad_norm=MAX_NORM["mae"])
    rec = tr.losses["grad_norm"]
    assert len(rec["D"]) == 9 and len(rec["G"]) == 4
    assert max(rec["D"]) > MAX_NORM["mae"] and max(rec["G"]) > MAX_NORM["mae"]


def test_mae_grad_scaler_clips_the_unscaled_gradients():
    """GradScaler.step has un-scaled the gradients before it calls FusedAdam.step: the clipped run through the scaler equals the
    clipped run without it, to test_mae_gpu.py's tolerance for that pair, and records the norm of the un-scaled gradients"""
    c = MAX_NORM["mae"]
    runs = {}
    for scaled in (False, True):
        tr = GM.build(T0, "f32", grad_scaler=scaled, max_grad_norm=c, **MAE_OVER)
        assert tr.scaler.is_enabled() == scaled
        for _ in GM.run(tr, T0, 2):
            pass
        tr.flush_losses()
        runs[scaled] = tr
    plain, scaled = runs[False], runs[True]
    assert scaled.scaler.get_scale() == 65536.0                        # no update was skipped
    a, b = trained_tensors(scaled), trained_tensors(plain)
    pn = np.array([[float(x[k][0].double().norm()) for k in a] for x in (a, b)])
    assert maxrel(pn[0], pn[1]) < 1e-3
    tok = (scaled.model.mask_token.mask_token - plain.model.mask_token.mask_token).abs().max().item()
    assert tok < 2 * 2 * 1.5e-4 + 1e-6
    for name in ("D", "G"):
        got, want = scaled.losses["grad_norm"][name], plain.losses["grad_norm"][name]
        assert len(got) == len(want) == 2 and max(want) > c
        assert maxrel(got, want) < 1e-3, (name, got, want)             # (not 65536 times it)


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["sgd", "rmsprop"])
def test_plain_optimizers_refuse_the_option(optimizer):
    with pytest.raises(NotImplementedError, match="max_grad_norm"):
        GS.build(T0, "f32", optimizer=optimizer, max_grad_norm=1.0)
    tr = GS.build(T0, "f32", optimizer=optimizer, max_grad_norm=0)     # 0: off, as before
    assert tr.max_grad_norm is None and "grad_norm" not in tr.loss_types
