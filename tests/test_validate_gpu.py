"""trainer.validate() on both stages, the validation hook of DefectGanTrainer.train() and the "best" checkpoint.

Values: the metrics validate() returns equal the float64 reference (tests/metrics_reference.py) on the tensors the same seeded
passes produce -- ``_repair_mask`` for the MAE stage, ``model("inference", ...)`` for the defectGAN stage -- within the kernel
test's bounds; the classifier scores are ratios of exact integers.  The invariant: ``step, step, validate, step`` leaves what
``step, step, step`` leaves, bit for bit, and validation itself moves no RNG state, counter, buffer, flag or digest."""
import itertools
import random

import numpy as np
import pytest
import torch

import metrics_reference as R
import test_graph_mae_gpu as GM
import test_graph_step_gpu as GS
from test_metrics_kernel_gpu import SSIM_TOL, SUM_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C32 = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)        # the 32 x 32, batch-2 golden configuration
C64 = GS.SMALL                                                                      # the 64 x 64 one
AUG = dict(diff_aug="color,translation,cutout", diff_aug_rng="device", diff_aug_seed=1234)
# The error sums here are not the kernel test's cases, so their bound is reasoned, not measured: a float64 sum of n terms of one
# sign is within n * 2^-53 relative of the exact one in any order, the kernel's and numpy's alike; n <= 3 * 64 * 64.
SUM_TOL = max(SUM_RTOL, 2 * 3 * 64 * 64 * 2.0 ** -53)
PSNR_TOL = SUM_TOL * 10 / np.log(10) + 1e-12               # d psnr = 10 / ln 10 * d mse / mse; log10 and the mean round too


def same_floats(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def close(got, want, names, where):
    for name in names:
        g, w = got[name], want[name]
        tol = SSIM_TOL if name.endswith("ssim") else PSNR_TOL if "psnr" in name else 2 * SUM_TOL * abs(w) if name == "l1" else 1e-12
        print(f"[validate] {where} {name}: {g!r} (reference {w!r})")
        assert (np.isnan(g) and np.isnan(w)) or abs(g - w) <= tol, (where, name, g, w)


def gan_loaders(c, first, count, device=None):
    """the ``defects`` / ``background`` pair on ``count`` fixed batches"""
    batches = [GS.batch(c, first + i) for i in range(count)]
    if device is not None:
        batches = [tuple(t.to(device) for t in b) for b in batches]
    return {"defects": [(df, lab, None) for _, lab, df in batches],
            "background": itertools.cycle([(bg, lab, None) for bg, lab, _ in batches])}


def mae_loader(c, first, count):
    return [GM.batch(c, first + i) + (None,) for i in range(count)]


def host_state(tr):
    """what validation must leave alone, next to ``state_digest()``"""
    model = tr.model
    out = {"cpu_rng": torch.get_rng_state(), "device_rng": torch.cuda.get_rng_state(DEV), "python_rng": random.getstate(),
           "iters": int(tr.iters)}
    for key in ("diffaug_rng", "mask_rng", "embed_rng"):
        rng = getattr(model, key, None)
        if rng is not None:
            out[key] = rng.state()
            out[key + ".id"] = id(rng)
    nets = dict(model.networks, **{f"ema_{k}": v for k, v in model.ema.items()})
    for name, net in nets.items():
        out[f"{name}.training"] = tuple(m.training for m in net.modules())
        for k, v in net.named_buffers():
            out[f"{name}.{k}"] = v.detach().clone()
    out["table_marks"] = model.netG.table_marks()
    return out


def check_invariant(mod, c, dtype, validate, steps=3, at=1, **over):
    """``mod``: GS (defectGAN) or GM (MAE) -- build / run / snapshot.  -> the validated trainer (its graphs still held)"""
    from de_i2i_gan_amd import ops
    tr = mod.build(c, dtype, **over)
    for i in mod.run(tr, c, steps):
        if i == at:
            before, digest, serial = host_state(tr), tr.state_digest(), ops.capture_serial
            graphs = None if tr._graphs is None else dict(tr._graphs.graphs)
            scores = validate(tr)
            assert set(scores) == set(tr.metric_names) and all(len(tr.metrics[k]) == 1 for k in scores)
            mod.assert_same(before, host_state(tr), "validate")
            assert tr.state_digest() == digest
    got = mod.snapshot(tr)
    if over.get("graph_step"):
        assert graphs and ops.capture_serial == serial                     # no capture after the validation ...
        assert tr._graphs.graphs.keys() == graphs.keys() and all(tr._graphs.graphs[k] is graphs[k] for k in graphs)      # ... same graphs
    plain = mod.build(c, dtype, **over)
    for _ in mod.run(plain, c, steps):
        pass
    mod.assert_same(mod.snapshot(plain), got, "after validate")
    assert tr.state_digest() == plain.state_digest()
    plain.release_graphs()
    return tr


# ---- 1. MAE stage: values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, masks", [("f32", "host"), ("bf16", "host"), ("bf16", "device")])
def test_mae_values_equal_the_reference(dtype, masks):
    over = dict(mask_rng="device", mask_seed=GM.SEED) if masks == "device" else {}
    tr = GM.build(C32, dtype, val_seed=11, **over)
    for _ in GM.run(tr, C32, 1):
        pass
    loader = mae_loader(C32, 60, 2)
    got = tr.validate(loader)
    assert list(got) == list(tr.metric_names) and all(isinstance(v, float) for v in got.values())
    model, sums, counts = tr.model, [], 0
    with tr._validation_scope():                              # the same seeded passes, tensors taken out
        model.netD.eval()
        model.netG.eval()
        with model._ema_scope():
            for imgs, labels, _ in loader:
                imgs, labels = imgs.to(DEV), labels.to(DEV)
                predicted, mask = model._repair_mask(imgs, labels)
                assert tuple(mask.shape) == (2, 1, 32, 32) and 0 < float(mask.mean()) < 1
                sums.append(R.image_sums(predicted.float().cpu().numpy(), imgs.cpu().numpy(), 1.0 - mask.float().cpu().numpy()))
                logits = model.netD(imgs)[1]
                counts = counts + R.clf_counts(logits.float().reshape(2, -1).cpu().numpy(), labels.cpu().numpy(), "bce")
    want = R.image_scores(np.concatenate(sums), (3, 32, 32))
    want.update({"clf_" + k: v for k, v in R.clf_scores(counts).items()})
    close(got, want, tr.metric_names, f"mae {dtype} {masks}")
    again = tr.validate(loader)                               # the same masks: identical floats
    assert same_floats(again, got)
    assert all(tr.metrics[k][0] == tr.metrics[k][1] or np.isnan(tr.metrics[k][0]) for k in got) and len(tr.metrics["psnr"]) == 2
    assert tr.validate(loader, max_batches=1)["psnr"] != got["psnr"]


# ---- 2. defectGAN stage: values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c, dtype", [(C32, "f32"), (C32, "bf16"), (C64, "bf16")])
def test_defectgan_values_equal_the_reference(c, dtype):
    tr = GS.build(c, dtype)
    for _ in GS.run(tr, c, 1):
        pass
    got = tr.validate(gan_loaders(c, 60, 2))
    assert list(got) == list(tr.metric_names)
    model, s = tr.model, c["image_size"]
    cyc, cyc_df, real, fake = [], [], 0, 0
    with tr._validation_scope():
        for bg, lab, df in (GS.batch(c, 60), GS.batch(c, 61)):
            bg, lab, df = bg.to(DEV), lab.to(DEV), df.to(DEV)
            normal = torch.zeros_like(lab)
            normal[:, 0] = 1                                 # class 0 one-hot: the normal label
            fake_df = model("inference", bg, lab)[0]
            restored = model("inference", fake_df, normal)[0]
            recovered = model("inference", model("inference", df, normal)[0], lab)[0]
            cyc.append(R.image_sums(restored.float().cpu().numpy(), bg.cpu().numpy()))
            cyc_df.append(R.image_sums(recovered.float().cpu().numpy(), df.cpu().numpy()))
            real = real + R.clf_counts(model.netD(df)[1].float().reshape(2, -1).cpu().numpy(), lab.cpu().numpy(), "bce")
            fake = fake + R.clf_counts(model.netD(fake_df)[1].float().reshape(2, -1).cpu().numpy(), lab.cpu().numpy(), "bce")
    want = {}
    for prefix, sums in (("cyc_", cyc), ("cyc_df_", cyc_df)):
        scores = R.image_scores(np.concatenate(sums), (3, s, s))
        want.update({prefix + k: scores[k] for k in ("psnr", "ssim")})
    for suffix, counts in (("_real", real), ("_fake", fake)):
        want.update({f"clf_{k}{suffix}": v for k, v in R.clf_scores(counts).items()})
    close(got, want, tr.metric_names, f"defectgan {dtype} {s}")
    assert same_floats(tr.validate(gan_loaders(c, 60, 2)), got)


# ---- 3. the invariant -----------------------------------------------------------------------------------------------------------
def gan_validate(c):
    return lambda tr: tr.validate(gan_loaders(c, 80, 2), max_batches=2)


def mae_validate(c):
    return lambda tr: tr.validate(mae_loader(c, 80, 2))


@pytest.mark.parametrize("dtype, over", [("f32", {}), ("bf16", dict(add_noise=True, use_spectral=True, diff_aug="color,translation,cutout")),
                                         ("bf16", dict(AUG, num_critics=2))])
def test_defectgan_eager_invariant(dtype, over):
    """host-drawn DiffAugment moves the CPU RNG, NoiseInjection the device RNG, device draws their counter: all where they were"""
    check_invariant(GS, C32, dtype, gan_validate(C32), **over)


def test_defectgan_graph_step_invariant():
    tr = check_invariant(GS, C64, "bf16", gan_validate(C64), steps=4, at=2, graph_step=True, graph_warmup=1, **AUG)
    assert tr.model.diffaug_rng.state()[1] > 0
    tr.release_graphs()


def test_defectgan_ema_invariant_and_which_weights_are_read():
    tr = check_invariant(GS, C32, "bf16", gan_validate(C32), ema_beta=0.9)
    with_ema = tr.validate(gan_loaders(C32, 80, 2))["cyc_psnr"]
    tr.opt.ema_inference = False
    try:
        live = tr.validate(gan_loaders(C32, 80, 2))["cyc_psnr"]
    finally:
        tr.opt.ema_inference = True
    assert live != with_ema
    plain = GS.build(C32, "bf16")                              # the live weights of the same run, no EMA anywhere
    for _ in GS.run(plain, C32, 3):
        pass
    assert plain.validate(gan_loaders(C32, 80, 2))["cyc_psnr"] == live


@pytest.mark.parametrize("dtype, over", [("f32", {}), ("bf16", dict(mask_rng="device", mask_seed=GM.SEED))])
def test_mae_eager_invariant(dtype, over):
    check_invariant(GM, C32, dtype, mae_validate(C32), **over)


def test_mae_graph_step_invariant():
    tr = check_invariant(GM, C64, "bf16", mae_validate(C64), steps=4, at=2, graph_step=True, graph_warmup=1, mask_rng="device",
                         mask_seed=GM.SEED)
    assert tr.model.mask_rng.state() == (GM.SEED, 8)          # two draws per step, none by the validation
    tr.release_graphs()


def test_mae_ema_invariant_and_which_weights_are_read():
    tr = check_invariant(GM, C32, "bf16", mae_validate(C32), ema_beta=0.9, mask_rng="device", mask_seed=GM.SEED)
    with_ema = tr.validate(mae_loader(C32, 80, 2))["psnr"]
    tr.opt.ema_inference = False
    try:
        live = tr.validate(mae_loader(C32, 80, 2))["psnr"]
    finally:
        tr.opt.ema_inference = True
    assert live != with_ema


# ---- 4. a validation pass, then a train pass on the same label tensor --------------------------------------------------------------
@pytest.mark.parametrize("steps_before", [0, 1])
def test_validate_then_step_on_the_same_label_tensor(steps_before):
    """the SPADE tables and the label-set memo of the validation pass are gone when the step primes (and before the first step the
    generator's table marks are those of an untouched tree): the step equals the one without the validation"""
    bg, lab, df = (t.to(DEV) for t in GS.batch(C32, 7))
    got = []
    for validate in (True, False):
        tr = GS.build(C32, "bf16")
        for _ in GS.run(tr, C32, steps_before):
            pass
        if validate:
            tr.validate({"defects": [(df, lab, None)], "background": iter([(bg, lab, None)])})
            assert all(not m._gb_cache for m in tr.model.netG._table_modules())
        tr.step(bg, lab, df)
        tr.step(bg, lab, df)
        got.append((GS.snapshot(tr), tr.state_digest()))
    GS.assert_same(got[1][0], got[0][0], "validate, then step")
    assert got[0][1] == got[1][1]


# ---- 5. the hook of train() and the "best" checkpoint ------------------------------------------------------------------------------
def best_files(tr):
    run = tr.opt.ckpt_dir / tr.opt.name
    return sorted(p.name for p in run.iterdir() if p.name.startswith("best")) if run.exists() else []


@pytest.mark.parametrize("name", ["cyc_psnr", "clf_f1_fake"])
def test_train_validates_and_keeps_the_best_checkpoint(name):
    over = dict(num_epochs=2, iters_per_epoch=2, scheduler="exp", val_freq=1, val_max_batches=1, save_best=name, train_state=True)
    tr = GS.build(C32, "bf16", **over)
    at_save = {}
    save = tr.save_checkpoint

    def spy(label, epoch, latest=False):
        save(label, epoch, latest)
        if label == "best":
            at_save["digest"], at_save["epoch"], at_save["iters"] = tr.state_digest(), epoch, tr.iters
    tr.save_checkpoint = spy
    tr.train(gan_loaders(C32, 0, 2, DEV), gan_loaders(C32, 90, 2, DEV))
    assert tr.iters == 4 and all(len(tr.metrics[k]) == 2 for k in tr.metric_names)
    assert best_files(tr) == ["best.txt", "best_net_D.pth", "best_net_G.pth", "best_train_state.pth"]
    epoch, iters, value = (tr.opt.ckpt_dir / tr.opt.name / "best.txt").read_text().strip().split(",")
    values = tr.metrics[name]
    assert not any(np.isnan(v) for v in values)
    assert int(epoch) == int(np.argmax(values)) + 1 == at_save["epoch"] and int(iters) == at_save["iters"] == 2 * int(epoch)
    assert float(value) == max(values) and tr.best == (int(epoch), int(iters), float(value))
    # the "best" label resumes like any other: the digests check, and the state is the one that was saved
    torch.manual_seed(999)
    again = GS.build(C32, "bf16", ckpt_dir=tr.opt.ckpt_dir, name="again", load_model_name=tr.opt.name, which_epoch="best",
                     **dict(over, num_epochs=4))
    assert again.train_state_restored is True and again.state_digest() == at_save["digest"]


def test_val_freq_skips_epochs_and_off_reads_no_loader():
    over = dict(num_epochs=2, iters_per_epoch=1, scheduler="exp")
    tr = GS.build(C32, "bf16", val_freq=2, **over)
    tr.train(gan_loaders(C32, 0, 1, DEV), gan_loaders(C32, 90, 1, DEV))
    assert [len(tr.metrics[k]) for k in tr.metric_names] == [1] * 8 and best_files(tr) == []
    off = GS.build(C32, "bf16", **over)
    off.train(gan_loaders(C32, 0, 1, DEV), val_loaders=None)
    assert dict(off.metrics) == {} and off.iters == 2


def test_mae_maybe_save_best_keeps_the_lower_l1():
    tr = GM.build(C32, "bf16", save_best="l1")
    assert tr.maybe_save_best(1) is False                     # nothing validated yet
    tr.validate(mae_loader(C32, 60, 1))
    assert tr.maybe_save_best(1) is True and "best_net_G.pth" in best_files(tr)
    tr.validate(mae_loader(C32, 60, 1))                       # the same score: not better
    assert tr.maybe_save_best(2) is False and tr.best[0] == 1
    tr.metrics["l1"].append(tr.best[2] / 2)                   # lower is better for l1
    assert tr.maybe_save_best(3) is True and tr.best[0] == 3
    tr.metrics["l1"].append(float("nan"))
    assert tr.maybe_save_best(4) is False
