"""opt.val_freq / val_max_batches / val_seed / save_best on the host: an invalid value, or a metric the stage does not have, is
refused when a trainer is constructed, before a model is built (optim.validation_options); ``train()`` with ``val_freq`` on and no
``val_loaders`` is refused at entry."""
from types import SimpleNamespace

import pytest

from helpers import make_opt

from de_i2i_gan_amd.optim import validation_options

C = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)
MAE = dict(loss_weight=[10, 3, 1], mask_token_type="position", mask_ratio=0.75, patch_size=8)


def construct(stage, **over):
    from de_i2i_gan_amd.trainers import base_trainer
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer

    def no_model(opt):
        raise AssertionError("a model was built before the options were checked")

    saved = base_trainer.create_model
    base_trainer.create_model = no_model
    try:
        if stage == "mae":
            return MAETrainer(make_opt(C, "cpu", **MAE, **over))
        return DefectGanTrainer(make_opt(C, "cpu", **over))
    finally:
        base_trainer.create_model = saved


@pytest.mark.parametrize("stage", ["defectgan", "mae"])
@pytest.mark.parametrize("freq", [-1, 1.5, -0.5])
def test_invalid_val_freq_is_refused_before_a_model_is_built(stage, freq):
    with pytest.raises(ValueError, match="val_freq"):
        construct(stage, val_freq=freq)


@pytest.mark.parametrize("stage, name", [("defectgan", "psnr"), ("defectgan", "fid"), ("mae", "cyc_psnr"), ("mae", "accuracy")])
def test_unknown_save_best_is_refused_and_lists_the_valid_names(stage, name):
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer
    names = (MAETrainer if stage == "mae" else DefectGanTrainer).metric_names
    with pytest.raises(ValueError, match="save_best") as err:
        construct(stage, save_best=name)
    assert all(n in str(err.value) for n in names)


def test_metric_names_of_the_stages():
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer
    assert set(MAETrainer.metric_names) == {"l1", "psnr", "ssim", "psnr_masked", "clf_acc", "clf_f1"}
    assert set(DefectGanTrainer.metric_names) == {"cyc_psnr", "cyc_ssim", "cyc_df_psnr", "cyc_df_ssim", "clf_acc_real", "clf_f1_real",
                                                  "clf_acc_fake", "clf_f1_fake"}


@pytest.mark.parametrize("batches", [0, -2, 2.5])
def test_invalid_val_max_batches(batches):
    with pytest.raises(ValueError, match="val_max_batches"):
        validation_options(SimpleNamespace(val_max_batches=batches))


@pytest.mark.parametrize("seed", [-1, 0.5, 2 ** 63])
def test_invalid_val_seed(seed):
    with pytest.raises(ValueError, match="val_seed"):
        validation_options(SimpleNamespace(val_seed=seed))


def test_absent_options_mean_off():
    off = {"val_freq": 0, "val_max_batches": None, "val_seed": 0, "save_best": None}
    assert validation_options(SimpleNamespace(), ("psnr",)) == off
    assert validation_options(SimpleNamespace(val_freq=None, val_max_batches=None, val_seed=None, save_best=None), ("psnr",)) == off
    assert validation_options(SimpleNamespace(val_freq=0, save_best=""), ("psnr",)) == off
    assert validation_options(SimpleNamespace(val_freq=2.0, val_max_batches=3, val_seed=7, save_best="l1"), ("psnr", "l1")) == \
        {"val_freq": 2, "val_max_batches": 3, "val_seed": 7, "save_best": "l1"}


def test_train_with_val_freq_needs_val_loaders():
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    tr = DefectGanTrainer.__new__(DefectGanTrainer)              # (train() checks at entry, before it touches anything else)
    tr.val_opts = validation_options(SimpleNamespace(val_freq=1), DefectGanTrainer.metric_names)
    with pytest.raises(ValueError, match="val_loaders"):
        tr.train({"defects": [], "background": iter(())}, None)
