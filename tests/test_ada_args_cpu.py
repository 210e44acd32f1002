"""optim.ada_options: what opt.diff_aug_p / opt.ada_target (gated DiffAugment and its controller) accept, what turns them off and
what they refuse -- a pure function of the option object, so no GPU is needed.  Also the CPU half of the kernel tests' setup: the
numpy reference of the gated table (tests/test_ada_kernels_gpu.py) has all-on, all-off and mixed rows at the seed those tests use."""
from types import SimpleNamespace

import numpy as np
import pytest

from de_i2i_gan_amd.optim import ada_options

ON = dict(diff_aug="color,translation,cutout", diff_aug_rng="device")


def _opt(**kw):
    return SimpleNamespace(**kw)


def test_absent_none_and_zero_are_off():
    assert ada_options(_opt()) is None
    assert ada_options(_opt(diff_aug_p=None, ada_target=None)) is None
    assert ada_options(_opt(ada_target=0)) is None and ada_options(_opt(ada_target=0.0, **ON)) is None
    assert ada_options(_opt(diff_aug="color", diff_aug_rng="host")) is None          # (neither option: nothing is asked of the others)
    assert ada_options(_opt(), diffaug_stage=False) is None                            # the MAE stage without the options
    assert ada_options(_opt(ada_interval=0, ada_kimg=-1, ada_p_max=7)) is None         # (the controller's options alone turn nothing on)


def test_documented_values_and_defaults():
    assert ada_options(_opt(diff_aug_p=0, **ON)) == {"p": 0.0, "target": None, "interval": 4, "kimg": 500.0, "p_max": 1.0}
    assert ada_options(_opt(diff_aug_p=1, **ON))["p"] == 1.0 and ada_options(_opt(diff_aug_p=0.25, **ON))["p"] == 0.25
    got = ada_options(_opt(ada_target=0.6, **ON))
    assert got == {"p": 0.0, "target": 0.6, "interval": 4, "kimg": 500.0, "p_max": 1.0}
    got = ada_options(_opt(ada_target=0.6, diff_aug_p=0.5, ada_interval=2, ada_kimg=0.064, ada_p_max=0.8, **ON))
    assert got == {"p": 0.5, "target": 0.6, "interval": 2, "kimg": 0.064, "p_max": 0.8}
    assert ada_options(_opt(ada_target=0.6, ada_interval=None, ada_kimg=None, ada_p_max=None, **ON))["interval"] == 4
    assert ada_options(_opt(diff_aug_p=0.5, ada_target=0, **ON))["target"] is None      # target 0: a fixed p


@pytest.mark.parametrize("over, name", [
    (dict(diff_aug_p=0.5, diff_aug_rng="device"), "diff_aug_p"),                       # no diff_aug
    (dict(diff_aug_p=0.5, diff_aug="", diff_aug_rng="device"), "diff_aug_p"),
    (dict(ada_target=0.6, diff_aug="", diff_aug_rng="device"), "ada_target"),
    (dict(diff_aug_p=0.5, diff_aug="color"), "diff_aug_p"),                            # no device RNG
    (dict(diff_aug_p=0.5, diff_aug="color", diff_aug_rng="host"), "diff_aug_p"),
    (dict(ada_target=0.6, diff_aug="color", diff_aug_rng="host"), "ada_target"),
    (dict(diff_aug_p=-0.01, **ON), "diff_aug_p"),
    (dict(diff_aug_p=1.01, **ON), "diff_aug_p"),
    (dict(diff_aug_p=float("nan"), **ON), "diff_aug_p"),
    (dict(ada_target=1.0, **ON), "ada_target"),
    (dict(ada_target=-0.2, **ON), "ada_target"),
    (dict(ada_target=float("nan"), **ON), "ada_target"),
    (dict(ada_target=0.6, ada_interval=0, **ON), "ada_interval"),
    (dict(ada_target=0.6, ada_interval=2.5, **ON), "ada_interval"),
    (dict(ada_target=0.6, ada_kimg=0, **ON), "ada_kimg"),
    (dict(ada_target=0.6, ada_kimg=-3, **ON), "ada_kimg"),
    (dict(ada_target=0.6, ada_p_max=1.5, **ON), "ada_p_max"),
    (dict(ada_target=0.6, ada_p_max=-0.1, **ON), "ada_p_max"),
])
def test_refusals_name_the_option(over, name):
    with pytest.raises(ValueError, match=name):
        ada_options(_opt(**over))


@pytest.mark.parametrize("over, name", [(dict(diff_aug_p=0.5, **ON), "diff_aug_p"), (dict(ada_target=0.6, **ON), "ada_target")])
def test_the_mae_stage_refuses_them(over, name):
    with pytest.raises(ValueError, match=name):
        ada_options(_opt(**over), diffaug_stage=False)


def test_the_gated_reference_has_all_on_all_off_and_mixed_rows_at_the_test_seed():
    from test_ada_kernels_gpu import N_HALF, SEED_HALF, gate_reference
    gates = gate_reference(SEED_HALF, 0, "color,translation,cutout", N_HALF, 0, np.float32(0.5))[0]
    on = gates.sum(axis=1)
    assert (on == 3).any() and (on == 0).any() and ((on > 0) & (on < 3)).any()
