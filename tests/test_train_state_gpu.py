"""opt.train_state: a run that is stopped, saved and continued is the run that was never stopped, bit for bit.

Every case: run A takes 2K steps uninterrupted; run B takes K steps and saves (``save_latest``), then a NEW trainer built with
``continue_training`` -- after the process-wide RNGs have been set to something else -- takes the remaining K.  Compared with
``torch.equal`` / ``==``: every parameter and buffer of every network, the MAE stage's mask token, every optimizer moment and step
count, every EMA tensor, the ADA words, the device generators' counters, every learning rate and ``initial_lr``, the losses the
last K steps recorded, and ``state_digest()``.  Inputs come from the batch functions' own ``torch.Generator``.  Nothing needs a
tolerance.  K = 3 is odd, so with ``num_critics = 2`` the save falls between a D-only iteration and the next G update."""
import shutil
from pathlib import Path

import pytest
import torch

import test_graph_mae_gpu as GM
import test_graph_step_gpu as GS
from helpers import make_opt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)        # the 32 x 32, batch-2 golden configuration
K = 3

AUG = dict(diff_aug="color,translation,cutout", diff_aug_rng="device", diff_aug_seed=1234)
RECIPE = dict(AUG, use_spectral=True, add_noise=True, ada_target=0.6, diff_aug_p=0.5, ada_interval=2, ada_kimg=0.064, ema_beta=0.9,
              ema_start_iter=2, max_grad_norm=1.0, num_critics=2)
MAE = dict(GM.MAE, mask_rng="device", mask_seed=GM.SEED)


def trainer_class(mae):
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer
    return MAETrainer if mae else DefectGanTrainer


def build(mae=False, resume=None, **over):
    """a fresh trainer from one seed, or (``resume``: a trainer that has saved) one that continues its run"""
    over = {"train_state": True, **over}
    if resume is not None:
        torch.manual_seed(999)                              # (what the resumed run must NOT go on from)
        torch.cuda.manual_seed(555)
        return trainer_class(mae)(make_opt(C, DEV, "bf16", defer_loss_sync=True, ckpt_dir=resume.opt.ckpt_dir, name=resume.opt.name,
                                           load_model_name=resume.opt.name, continue_training=True, **over))
    torch.manual_seed(123)
    tr = trainer_class(mae)(make_opt(C, DEV, "bf16", defer_loss_sync=True, **over))
    torch.cuda.manual_seed(77)
    return tr


def steps(tr, start, stop, mae=False):
    for i in range(start, stop):
        inputs = GM.batch(C, i) if mae else GS.batch(C, i)
        tr.step(*[t.to(DEV) for t in inputs])


def loss_lists(tr):
    tr.flush_losses()
    return {(kind, k): list(v) for kind, d in tr.losses.items() for k, v in d.items()}


def full_state(tr):
    """everything a continued run has to agree on"""
    model, out = tr.model, {}
    modules = dict({f"net_{k}": v for k, v in model.networks.items()}, **{f"ema_{k}": v for k, v in model.ema.items()})
    token = getattr(model, "mask_token", None)
    if isinstance(token, torch.nn.Module):
        modules["mask_token"] = token
    for name, mod in modules.items():
        for k, v in mod.state_dict().items():
            out[f"{name}.{k}"] = v.detach().clone()
    for name, o in tr.optimizers.items():
        for gi, group in enumerate(o.param_groups):
            out[f"{name}.lr.{gi}"] = (group["lr"], group.get("initial_lr"))
            for pi, p in enumerate(group["params"]):
                for k, v in (o.state.get(p) or {}).items():
                    out[f"{name}.state.{gi}.{pi}.{k}"] = v.clone() if isinstance(v, torch.Tensor) else v
    if getattr(model, "ada", None) is not None:
        out["ada.p_rt"], out["ada.acc"] = model.ada.p_rt.clone(), model.ada.acc.clone()
    for key in ("diffaug_rng", "mask_rng"):
        if getattr(model, key, None) is not None:
            out[key] = getattr(model, key).state()
    scaler = getattr(tr, "scaler", None)
    if scaler is not None and scaler.is_enabled():
        out["grad_scaler"] = scaler.state_dict()
    out["digest"] = tr.state_digest()
    out["iters"] = int(tr.iters)
    return out


_runs = {}


def uninterrupted(mae=False, k=K, **over):
    """run A, once per option set: -> (its full state after 2k steps, the losses its last k steps recorded)"""
    key = repr((mae, k, sorted(over.items())))
    if key not in _runs:
        _runs[key] = _uninterrupted(mae, k, over)
    return _runs[key]


def _uninterrupted(mae, k, over):
    tr = build(mae, **over)
    steps(tr, 0, k, mae)
    before = loss_lists(tr)
    steps(tr, k, 2 * k, mae)
    last = {key: v[len(before.get(key, [])):] for key, v in loss_lists(tr).items()}
    state = full_state(tr)
    tr.release_graphs()
    return state, last


def check_resume(mae=False, k=K, **over):
    want, want_losses = uninterrupted(mae, k, **over)
    first = build(mae, **over)
    steps(first, 0, k, mae)
    first.save_latest(1)
    first.release_graphs()
    again = build(mae, resume=first, **over)
    assert again.train_state_restored is True and again.iters == k
    del first
    steps(again, k, 2 * k, mae)
    got, got_losses = full_state(again), loss_lists(again)
    again.graphs_captured = len(again._graphs.graphs) if again._graphs is not None else 0
    again.release_graphs()
    GS.assert_same(want, got, "resumed")
    assert got_losses == want_losses and any(len(v) > 0 for v in got_losses.values())
    moments = [k for k in got if k.endswith(".exp_avg_sq")]
    assert moments and all(bool(got[k].abs().sum() > 0) for k in moments[:4])
    return want, again


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def test_a_plain_adam_eager():
    """(before train-state files existed the resumed half restarted every Adam at step 0 with zero moments)"""
    want, tr = check_resume()
    assert sorted(want["digest"]) == ["net_D", "net_G", "optim_D", "optim_G"]
    assert want["D.state.0.0.step"] == 2 * K and want["G.state.0.0.step"] == 2 * K


def test_a_lr_after_an_epoch_boundary():
    """an 'exp' schedule stepped once before the save: the resumed trainer's schedulers are fast-forwarded at construction and no
    stored lr is decayed again"""
    over = dict(scheduler="exp", lr_decay=0.01)
    a = build(**over)
    steps(a, 0, 1)
    a._update_per_epoch(1)
    steps(a, 1, 2)
    b = build(**over)
    steps(b, 0, 1)
    b._update_per_epoch(1)
    b.save_latest(2)                                        # (iter.txt: the epoch to continue with)
    again = build(resume=b, **over)
    assert again.first_epoch == 2 and again.train_state_restored
    steps(again, 1, 2)
    want, got = full_state(a), full_state(again)
    assert want["G.lr.0"][0] < 2e-4 and want["G.lr.0"][1] == 2e-4
    GS.assert_same(want, got, "after an epoch boundary")


def test_b_recipe_options_two_critics():
    want, _ = check_resume(**RECIPE)
    assert sorted(want["digest"]) == ["ada", "net_D", "net_G", "net_G_ema", "optim_D", "optim_G"]
    assert want["diffaug_rng"][1] > 0 and want["D.state.0.0.step"] == 2 * K and want["G.state.0.0.step"] == K
    assert any(not torch.equal(v, want["net_G" + k[5:]]) for k, v in want.items() if k.startswith("ema_G.") and v.is_floating_point())


def test_c_recipe_options_under_graph_step():
    """Replayed from captured graphs.  Two warm-up calls (G's first update, at iteration 2, must be eager: its moments are made
    there) and k = 5, so that both halves of run B replay both graphs (iterations 3-5 and 8-10) and the save still falls on an
    odd iteration; A = B, and both = eager."""
    graph = dict(graph_step=True, graph_warmup=2)
    want, tr = check_resume(k=5, **graph, **RECIPE)
    assert tr.graphs_captured == 2                          # (the resumed half captured and replayed D and D + G)
    eager, eager_losses = uninterrupted(k=5, **RECIPE)
    GS.assert_same(eager, want, "graph_step against eager")
    assert uninterrupted(k=5, **graph, **RECIPE)[1] == eager_losses


def test_d_host_drawn_diffaugment():
    """the draws come from the CPU RNG, which the resumed process has re-seeded in between"""
    check_resume(diff_aug="color,translation,cutout")


@pytest.mark.parametrize("grad_scaler", [False, True])
def test_e_mae_stage(grad_scaler):
    want, _ = check_resume(mae=True, grad_scaler=grad_scaler, **MAE)
    assert want["mask_rng"] == (GM.SEED, 2 * 2 * K) and "mask_token" in want["digest"]
    assert ("grad_scaler" in want) == grad_scaler
    assert any(k.startswith("G.state.1.0.") for k in want)                       # (the mask token's own param group)


# ---- the files ------------------------------------------------------------------------------------------------------------------
def files(tr):
    return sorted(p.name for p in (Path(tr.opt.ckpt_dir) / tr.opt.name).iterdir())


@pytest.fixture(scope="module")
def saved():
    """a plain trainer after K steps and save_latest"""
    tr = build()
    steps(tr, 0, K)
    tr.save_latest(1)
    return tr


def copy_of(saved, tmp_path):
    """-> a trainer-like handle on a private copy of the checkpoint directory"""
    shutil.copytree(Path(saved.opt.ckpt_dir) / saved.opt.name, tmp_path / saved.opt.name)
    return type("Saved", (), {"opt": type("Opt", (), {"ckpt_dir": tmp_path, "name": saved.opt.name})})


def test_one_more_file_and_no_temporary(saved):
    assert files(saved) == ["iter.txt", "latest_net_D.pth", "latest_net_G.pth", "latest_train_state.pth"]
    off = build(train_state=False)
    steps(off, 0, 1)
    off.save_latest(1)
    assert files(off) == ["iter.txt", "latest_net_D.pth", "latest_net_G.pth"]
    assert off.train_state is False and off.train_state_restored is None
    saved.save_checkpoint(7, 7)                              # (the numbered save of train(): the same method)
    assert files(saved) == ["7_net_D.pth", "7_net_G.pth", "7_train_state.pth", "iter.txt", "latest_net_D.pth", "latest_net_G.pth",
                            "latest_train_state.pth"]


def test_file_loads_with_weights_only(saved):
    state = torch.load(Path(saved.opt.ckpt_dir) / saved.opt.name / "latest_train_state.pth", weights_only=True)
    assert state["format_version"] == 1 and state["iters"] == K and state["epoch"] == 1
    assert sorted(state["optimizers"]) == ["D", "G"] and sorted(state["digests"]) == ["net_D", "net_G"]
    assert sorted(state["rng"]) == ["cpu", "device"]
    assert state["optimizers"]["G"][0][0]["step"] == K and state["optimizers"]["G"][0][0]["exp_avg"].device.type == "cpu"
    assert state["digests"] == {k: v for k, v in saved.state_digest().items() if k.startswith("net_")}


def test_weights_of_another_iteration_are_refused(saved, tmp_path):
    from de_i2i_gan_amd.networks import save_network
    handle = copy_of(saved, tmp_path)
    other = build(resume=handle)
    steps(other, K, K + 1)
    save_network(other.model.netG, "G", "latest", other.opt)           # G of iteration K + 1 next to everything else of K
    with pytest.raises(RuntimeError, match="latest_net_G.pth"):
        build(resume=handle)


def test_without_the_file_the_resume_is_from_weights_only(saved, tmp_path, capsys):
    handle = copy_of(saved, tmp_path)
    (tmp_path / saved.opt.name / "latest_train_state.pth").unlink()
    capsys.readouterr()
    tr = build(resume=handle)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "train state" in ln]
    assert tr.train_state_restored is False and len(lines) == 1 and "weights only" in lines[0]
    assert tr.iters == K and not tr.optimizers["G"].state
    for k, v in saved.model.netG.state_dict().items():
        assert torch.equal(v, tr.model.netG.state_dict()[k]), k


def test_iter_txt_of_another_save_is_refused(saved, tmp_path):
    handle = copy_of(saved, tmp_path)
    (tmp_path / saved.opt.name / "iter.txt").write_text("1\n2\n")
    with pytest.raises(RuntimeError, match="iter.txt"):
        build(resume=handle)


def test_a_format_version_from_the_future_is_refused(saved, tmp_path):
    handle = copy_of(saved, tmp_path)
    path = tmp_path / saved.opt.name / "latest_train_state.pth"
    torch.save(dict(torch.load(path, weights_only=True), format_version=2), path)
    with pytest.raises(RuntimeError, match="format version 2"):
        build(resume=handle)


def test_sean_is_refused():
    with pytest.raises(NotImplementedError, match="sean"):
        build(style_norm_block_type="sean")
