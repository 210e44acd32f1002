"""Global-norm gradient clipping, the part that needs no GPU: the new entry points of csrc/adam.hip (dei2i_grad_sumsq,
dei2i_grad_clip_finalize, dei2i_adam_step_clip, dei2i_adam_step_clip_dev) refuse bad arguments with DEI2I_ERR_BAD_ARG before anything
is launched (the pattern of test_optim_spectral_args_cpu.py); dei2i_grad_sumsq_blocks is host arithmetic and is checked against the
grid rule of the Adam launch restated here; the trainers' opt.max_grad_norm is validated before anything is built; and with the
option absent FusedAdam's constructor is the one it was."""
import ctypes
import inspect
from types import SimpleNamespace

import pytest

from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
P = ctypes.c_void_p(64)            # any non-null address: the checks below fail before a pointer is used
NAN = float("nan")

TABLE_BAD = (dict(table=None), dict(count=0), dict(count=-1), dict(max_n=0), dict(max_n=-4))


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib
    return _lib.load()


def test_grad_sumsq_checks_its_arguments(lib):
    def call(table=P, count=1, max_n=8, partial=P):
        return lib.dei2i_grad_sumsq(table, count, max_n, partial, None)
    for kw in TABLE_BAD + (dict(partial=None),):
        assert call(**kw) == BAD_ARG, kw


def test_grad_clip_finalize_checks_its_arguments(lib):
    def call(partial=P, n_partials=4, grad_scale=1.0, max_norm=1.0, out=P):
        return lib.dei2i_grad_clip_finalize(partial, n_partials, grad_scale, max_norm, out, None)
    for kw in (dict(partial=None), dict(out=None), dict(n_partials=0), dict(n_partials=-1), dict(max_norm=0.0), dict(max_norm=-1.0),
               dict(max_norm=NAN)):
        assert call(**kw) == BAD_ARG, kw


@pytest.mark.parametrize("coupled", [0, 1])
def test_adam_step_clip_checks_its_arguments(lib, coupled):
    def call(table=P, count=1, max_n=8, scale=P):
        return lib.dei2i_adam_step_clip(table, count, max_n, 1e-3, 0.5, 0.999, 1e-8, 0.5, 0.5, scale, coupled, 1e-2, None)
    for kw in TABLE_BAD + (dict(scale=None),):
        assert call(**kw) == BAD_ARG, kw


@pytest.mark.parametrize("coupled", [0, 1])
def test_adam_step_clip_dev_checks_its_arguments(lib, coupled):
    def call(table=P, count=1, max_n=8, hyper=P, index=P, rows=4, scale=P):
        return lib.dei2i_adam_step_clip_dev(table, count, max_n, hyper, index, rows, 0.5, 0.999, 1e-8, scale, coupled, 1e-2, None)
    for kw in TABLE_BAD + (dict(hyper=None), dict(index=None), dict(rows=0), dict(rows=-1), dict(scale=None)):
        assert call(**kw) == BAD_ARG, kw


@pytest.mark.parametrize("n", [1, 4, 1027, 1028, 524288, 524289, 10 ** 9])
def test_grad_sumsq_blocks_is_the_adam_grid_rule(lib, n):
    """table_grid(max_n, 4, 512, count).x: 256-thread workgroups at four elements a thread for the longest tensor, between 1 and 512"""
    assert lib.dei2i_grad_sumsq_blocks(n) == min(512, max(1, (n // 4 + 255) // 256))


@pytest.mark.parametrize("bad", [-1.0, -1e-9, NAN])
def test_trainer_refuses_an_invalid_max_grad_norm(bad):
    from de_i2i_gan_amd.trainers.base_trainer import BaseTrainer
    with pytest.raises(ValueError, match="max_grad_norm"):       # (at the top of __init__: nothing else of the options is read)
        BaseTrainer(SimpleNamespace(max_grad_norm=bad, optimizer="adam"))


@pytest.mark.parametrize("optimizer", ["sgd", "rmsprop"])
def test_trainer_refuses_clipping_outside_the_adam_family(optimizer):
    from de_i2i_gan_amd.trainers.base_trainer import BaseTrainer
    with pytest.raises(NotImplementedError, match="max_grad_norm"):
        BaseTrainer(SimpleNamespace(max_grad_norm=1.0, optimizer=optimizer))


def test_clip_options_off_and_on():
    from de_i2i_gan_amd.optim import clip_options
    for opt in (SimpleNamespace(), SimpleNamespace(max_grad_norm=None), SimpleNamespace(max_grad_norm=0),
                SimpleNamespace(max_grad_norm=0.0, optimizer="sgd")):
        assert clip_options(opt) is None
    assert clip_options(SimpleNamespace(max_grad_norm=2, optimizer="adamw")) == 2.0


def test_fused_adam_constructor_defaults_are_unchanged():
    import torch
    from de_i2i_gan_amd.optim import FusedAdam
    sig = inspect.signature(FusedAdam.__init__)
    assert list(sig.parameters) == ["self", "params", "lr", "betas", "eps", "grad_scale", "weight_decay", "decoupled", "max_grad_norm"]
    assert {k: v.default for k, v in sig.parameters.items() if k not in ("self", "params")} == \
        dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, weight_decay=0.0, decoupled=True, max_grad_norm=None)
    o = FusedAdam([torch.nn.Parameter(torch.zeros(3))])
    assert o.max_grad_norm is None and o.grad_norm is None and o.grad_scale == 1.0 and o.decoupled
    assert o.defaults == dict(o.defaults, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0) and "max_grad_norm" not in o.defaults
    for bad in (-1.0, NAN):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdam([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=bad)
