"""opt.ema_beta on the host: the option's range is checked when a trainer is constructed, and the weight rows of the captured EMA
update (optim.ema_weight_rows: row j is the weight of the j-th coming G update) are the floats the eager update passes by value
(optim.ema_weight of the iteration that update ends)."""
import ctypes

import numpy as np
import pytest

from helpers import make_opt

from de_i2i_gan_amd.optim import ema_options, ema_weight, ema_weight_rows

C = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)
BETA = 0.999


@pytest.mark.parametrize("beta", [-0.1, 1.0])
@pytest.mark.parametrize("stage", ["defectgan", "mae"])
def test_invalid_beta_is_refused_at_trainer_construction(beta, stage):
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer
    with pytest.raises(ValueError, match="ema_beta"):
        if stage == "mae":
            MAETrainer(make_opt(C, "cpu", loss_weight=[10, 3, 1], mask_token_type="position", mask_ratio=0.75, patch_size=8, ema_beta=beta))
        else:
            DefectGanTrainer(make_opt(C, "cpu", ema_beta=beta))


def test_absent_options_mean_no_ema():
    assert ema_options(make_opt(C, "cpu")) == (0.0, 0, True)
    assert ema_options(make_opt(C, "cpu", ema_beta=0.5, ema_start_iter=7, ema_inference=False)) == (0.5, 7, False)


def rows(iters, num_critics, start, count=8):
    out = ema_weight_rows(iters, num_critics, start, BETA, count)
    assert out.dtype == np.float32 and out.shape == (count,)
    return out


def test_weight_rows_follow_the_g_updates():
    b = np.float32(BETA)
    assert rows(0, 1, 3).tolist() == [0, 0, 0, b, b, b, b, b]                  # G updates end iterations 1, 2, 3, 4, ...
    assert rows(0, 2, 3).tolist() == [0, b, b, b, b, b, b, b]                  # ... 2, 4, 6, ...
    assert rows(10, 1, 3).tolist() == [b] * 8
    assert rows(10, 2, 3).tolist() == [b] * 8
    assert rows(3, 2, 6).tolist() == [0, 0, b, b, b, b, b, b]                  # after iteration 3: 4, 6, 8, ...
    assert rows(0, 1, 0).tolist() == [b] * 8                                   # the default start: averaging from the first update


@pytest.mark.parametrize("num_critics", [1, 2, 3])
@pytest.mark.parametrize("start", [0, 5, 6])
def test_weight_rows_are_the_eager_arguments(num_critics, start):
    """bit for bit what ctypes' c_float makes of the python float the eager update passes, at every starting iteration"""
    for iters in range(0, 12):
        got = rows(iters, num_critics, start, 16)
        ends = [(iters // num_critics + 1 + j) * num_critics for j in range(16)]
        want = np.array([ctypes.c_float(ema_weight(e, start, BETA)).value for e in ends], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (iters, ends)
