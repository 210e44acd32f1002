"""opt.ema_beta: the EMA copies of what the G optimizer trains (model.ema: netG, AdaIN's netE, the MAE stage's mask token) in the
DefectGanTrainer / MAETrainer step, eager and replayed from captured graphs.

ema_beta = 0.9 throughout, so that one update moves a copy far above rounding.  The recurrence is checked against float64 with the
bound of tests/test_ema_kernel_gpu.py (four roundings of quantities of at most 2 max(|p|, |e|)): |e - (0.9 e_prev + 0.1 p)| <=
8 * 2^-24 * max(|p|, |e_prev|) per element; everything else is bit for bit."""
from pathlib import Path

import pytest
import torch

import test_graph_mae_gpu as GM
from test_graph_step_gpu import DEV, SMALL, assert_same, batch, build, run, snapshot

pytestmark = pytest.mark.gpu
BETA = 0.9
EMA = dict(ema_beta=BETA)


def live_of(tr, label):
    m = tr.model
    return {"G": m.netG, "E": getattr(m, "netE", None), "mask_token": getattr(m, "mask_token", None)}[label]


def ema_params(tr):
    return {label: {k: v.detach().clone() for k, v in twin.named_parameters()} for label, twin in tr.model.ema.items()}


def ema_state(tr):
    """every parameter and buffer of every copy"""
    return {f"{label}.{k}": v.detach().clone() for label, twin in tr.model.ema.items() for k, v in twin.state_dict().items()}


def check_update(tr, prev, start, labels=None):
    """after a step that made a G update: the recurrence of every EMA parameter (``prev``: ema_params before the step), and every
    buffer of the copies equal to the live one"""
    for label, twin in tr.model.ema.items():
        live = live_of(tr, label)
        named_e, named_p = dict(twin.named_parameters()), dict(live.named_parameters())
        assert named_e.keys() == named_p.keys() and len(named_e) > 0, label
        averaged = 0
        for k, e in named_e.items():
            p = named_p[k].detach()
            if tr.iters <= start:
                assert torch.equal(e, p), (tr.iters, label, k)
                continue
            was = prev[label][k]
            ref = 0.9 * was.double() + 0.1 * p.double()
            err = (e.double() - ref).abs()
            bound = 8 * 2.0 ** -24 * torch.maximum(p.abs(), was.abs()).double()
            assert bool((err <= bound).all()), (tr.iters, label, k, (err / bound.clamp_min(1e-300)).max().item())
            averaged += not torch.equal(e, p) and not torch.equal(e, was)
        assert tr.iters <= start or averaged > len(named_e) // 2, (tr.iters, label, averaged)      # (neither end of the lerp)
        named_e, named_b = dict(twin.named_buffers()), dict(live.named_buffers())
        assert named_e.keys() == named_b.keys(), label
        for k, e in named_e.items():
            assert torch.equal(e, named_b[k]), (tr.iters, label, k)
    for label in labels or ():
        assert label in tr.model.ema


def files(tr):
    return sorted(p.name for p in (Path(tr.opt.ckpt_dir) / tr.opt.name).iterdir())


# ---- 1. off by default --------------------------------------------------------------------------------------------------
def test_off_by_default():
    tr = build(SMALL, "bf16")
    assert tr.model.ema == {} and tr.model.ema_group is None
    for _ in run(tr, SMALL, 1):
        pass
    tr.save_latest(1)
    assert files(tr) == ["iter.txt", "latest_net_D.pth", "latest_net_G.pth"]


def test_beta_zero_is_off():
    assert build(SMALL, "bf16", ema_beta=0.0).model.ema == {}


# ---- 2. the eager recurrence, and the live training it leaves alone -------------------------------------------------------
@pytest.fixture(scope="module")
def eager_run():
    """5 eager steps with the EMA starting after iteration 2: the trainer, and its snapshot after every step"""
    tr = build(SMALL, "bf16", ema_start_iter=2, **EMA)
    assert sorted(tr.model.ema) == ["G"] and sorted(tr.model.networks) == ["D", "G"] and sorted(tr.optimizers) == ["D", "G"]
    twin = tr.model.ema["G"]
    assert not twin.training and all(not m.training for m in twin.modules())
    assert all(not p.requires_grad for p in twin.parameters())
    assert twin.prec is tr.model.netG.prec and twin.opt is tr.opt             # (compared by identity in the ops: shared, not copied)
    assert all(torch.equal(a, b) for a, b in zip(twin.state_dict().values(), tr.model.netG.state_dict().values()))
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(twin.state_dict().values(), tr.model.netG.state_dict().values()))
    snaps = []
    prev = ema_params(tr)
    for _ in run(tr, SMALL, 5):
        check_update(tr, prev, start=2)
        prev = ema_params(tr)
        snaps.append(snapshot(tr))
    tracked = [k for k in ema_state(tr) if k.endswith("num_batches_tracked")]
    assert tracked and all(int(ema_state(tr)[k]) > 0 for k in tracked)
    return tr, snaps


def test_recurrence_and_buffers(eager_run):
    tr, snaps = eager_run
    assert tr.iters == 5 and len(snaps) == 5


def test_live_training_is_untouched(eager_run):
    _, snaps = eager_run
    plain = build(SMALL, "bf16")
    for i in run(plain, SMALL, 5):
        assert_same(snaps[i], snapshot(plain), i)


def test_two_critics_update_on_g_iterations_only():
    tr = build(SMALL, "bf16", num_critics=2, **EMA)
    before, prev = ema_state(tr), ema_params(tr)
    for _ in run(tr, SMALL, 6):
        now = ema_state(tr)
        changed = [k for k in now if not torch.equal(now[k], before[k])]
        if tr.iters % 2:
            assert not changed, (tr.iters, changed[:4])
        else:
            assert changed, tr.iters
            check_update(tr, prev, start=0)
        before, prev = now, ema_params(tr)


# ---- 3. graph mode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_critics, steps, graphs", [(1, 8, 1), (2, 9, 2)])
def test_graph_mode_equals_eager(num_critics, steps, graphs):
    """the switch from copying to averaging (ema_start_iter = 5) falls among the replayed steps"""
    over = dict(ema_start_iter=5, num_critics=num_critics, **EMA)
    eager = build(SMALL, "bf16", **over)
    want = [(snapshot(eager), ema_state(eager)) for _ in run(eager, SMALL, steps)]
    assert not torch.equal(want[-1][1]["G.stem.conv_block.0.weight"], eager.model.netG.state_dict()["stem.conv_block.0.weight"])
    del eager
    torch.cuda.synchronize()
    tr = build(SMALL, "bf16", graph_step=True, graph_warmup=3, **over)
    for i in run(tr, SMALL, steps):
        assert_same(want[i][0], snapshot(tr), i)
        assert_same(want[i][1], ema_state(tr), f"{i} (EMA)")
    assert len(tr._graphs.graphs) == graphs
    tr.release_graphs()


def test_graph_mode_with_an_eager_call_between_replays():
    """iteration 6 gets a smaller batch and runs eagerly: the device index is then one G update behind the host, the rows are
    rewritten before the next replay, and the switch (ema_start_iter = 7) comes right after it"""
    over = dict(ema_start_iter=7, **EMA)
    hooks = {5: lambda tr: 1}
    eager = build(SMALL, "bf16", **over)
    want = [(snapshot(eager), ema_state(eager)) for _ in run(eager, SMALL, 9, hooks=hooks)]
    del eager
    torch.cuda.synchronize()
    tr = build(SMALL, "bf16", graph_step=True, graph_warmup=3, **over)
    for i in run(tr, SMALL, 9, hooks=hooks):
        assert_same(want[i][0], snapshot(tr), i)
        assert_same(want[i][1], ema_state(tr), f"{i} (EMA)")
    assert len(tr._graphs.graphs) == 1
    tr.release_graphs()


# ---- 4. inference and checkpoints -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    tr = build(SMALL, "bf16", **EMA)
    for _ in run(tr, SMALL, 3):
        pass
    return tr


def generate(tr, state=None):
    if state is not None:
        tr.model.netG.load_state_dict(state)
    bg, lab, _ = batch(SMALL, 50)
    return tr.model("inference", bg.to(DEV), lab.to(DEV))


def test_inference_runs_the_ema_copy(trained):
    other = build(SMALL, "bf16")
    with_ema = generate(trained)
    want = generate(other, trained.model.ema["G"].state_dict())
    assert all(torch.equal(a, b) for a, b in zip(with_ema, want))
    trained.opt.ema_inference = False
    try:
        live = generate(trained)
    finally:
        trained.opt.ema_inference = True
    want = generate(other, trained.model.netG.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(live, want))
    assert not torch.equal(live[0], with_ema[0])


def resume(tr, **over):
    return build(SMALL, "bf16", ckpt_dir=tr.opt.ckpt_dir, name=tr.opt.name, load_model_name=tr.opt.name, continue_training=True, **over)


def test_checkpoint_restores_the_ema(trained):
    trained.save_latest(1)
    assert files(trained) == ["iter.txt", "latest_net_D.pth", "latest_net_G.pth", "latest_net_G_ema.pth"]
    again = resume(trained, **EMA)
    assert again.iters == 3
    assert_same(ema_state(trained), ema_state(again), "resumed")
    assert not torch.equal(ema_state(again)["G.stem.conv_block.0.weight"], again.model.netG.state_dict()["stem.conv_block.0.weight"])
    # model.load on a live trainer restores them too
    for _ in run(again, SMALL, 1):
        pass
    again.model.load("latest")
    assert_same(ema_state(trained), ema_state(again), "reloaded")


def test_resuming_a_run_saved_without_ema_starts_from_the_live_weights():
    plain = build(SMALL, "bf16")
    for _ in run(plain, SMALL, 2):
        pass
    plain.save_latest(1)
    tr = resume(plain, **EMA)
    state, live = ema_state(tr), tr.model.netG.state_dict()
    assert len(state) == len(live) > 0
    for k, v in live.items():
        assert torch.equal(state["G." + k], v) and torch.equal(v, plain.model.netG.state_dict()[k]), k


# ---- 5. the MAE stage: the mask token is averaged too -----------------------------------------------------------------------
MAE_OVER = dict(mask_rng="device", mask_seed=GM.SEED, **EMA)


def test_mae_stage_eager():
    tr = GM.build(GM.SMALL, "bf16", ema_start_iter=1, **MAE_OVER)
    assert sorted(tr.model.ema) == ["G", "mask_token"] and sorted(tr.model.networks) == ["D", "G"]
    prev = ema_params(tr)
    for _ in GM.run(tr, GM.SMALL, 4):
        check_update(tr, prev, start=1, labels=["mask_token"])
        prev = ema_params(tr)
    # mae_inference repairs with the copies (the generator and the token); the same mask for both calls
    bg, lab = GM.batch(GM.SMALL, 50)
    rng = tr.model.mask_rng.state()
    with_ema = tr.model("mae_inference", bg.to(DEV), lab.to(DEV))
    tr.model.mask_rng.set_state(rng)
    again = tr.model("mae_inference", bg.to(DEV), lab.to(DEV))
    tr.opt.ema_inference = False
    tr.model.mask_rng.set_state(rng)
    live = tr.model("mae_inference", bg.to(DEV), lab.to(DEV))
    assert torch.equal(with_ema[0], again[0])
    assert not torch.equal(with_ema[0], live[0])
    tr.model.save("latest")
    assert files(tr) == ["latest_net_D.pth", "latest_net_G.pth", "latest_net_G_ema.pth", "latest_net_mask_token_ema.pth"]
    saved = ema_state(tr)
    for _ in GM.run(tr, GM.SMALL, 1):
        pass
    tr.opt.load_model_name = tr.opt.name
    tr.model.load("latest")
    GM.assert_same(saved, ema_state(tr), "reloaded")


def test_mae_stage_graph_mode_equals_eager():
    over = dict(ema_start_iter=4, **MAE_OVER)
    eager = GM.build(GM.SMALL, "bf16", **over)
    want = [(GM.snapshot(eager), ema_state(eager)) for _ in GM.run(eager, GM.SMALL, 6)]
    assert any(k.startswith("mask_token.") for k in want[0][1])
    del eager
    torch.cuda.synchronize()
    tr = GM.build(GM.SMALL, "bf16", graph_step=True, graph_warmup=3, **over)
    for i in GM.run(tr, GM.SMALL, 6):
        GM.assert_same(want[i][0], GM.snapshot(tr), i)
        GM.assert_same(want[i][1], ema_state(tr), f"{i} (EMA)")
    assert len(tr._graphs.graphs) == 1
    tr.release_graphs()


# ---- 6. AdaIN: the style extractor is averaged too ---------------------------------------------------------------------------
def test_adain_extractor():
    import test_adain_gpu as A
    _, _, c, _ = A.load()
    tr = build(c, "bf16", style_norm_block_type="adain", sean_alpha=c.get("sean_alpha", 0), latent_dim=c["latent_dim"],
               ema_start_iter=1, **EMA)
    assert sorted(tr.model.ema) == ["E", "G"] and sorted(tr.optimizers) == ["D", "E", "G"]
    prev = ema_params(tr)
    for _ in run(tr, c, 2):
        check_update(tr, prev, start=1, labels=["E"])
        prev = ema_params(tr)
