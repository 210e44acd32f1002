"""The cce and mse loss entry points (include/dei2i_hip.h: dei2i_cce_logits_*, dei2i_mse_*) refuse bad arguments with
DEI2I_ERR_BAD_ARG before anything is launched -- the library's convention (test_bn_sync_args_cpu.py) -- so this runs without a GPU.
The cce kernels have no cap on `classes` (one wavefront per row, its lanes loop), so there is no above-the-cap case; a negative
count is refused like zero.  BaseModel._cal_loss names all four kinds when it refuses one."""
import ctypes
from types import SimpleNamespace

import pytest

from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
P = ctypes.c_void_p(64)            # any non-null address: the checks below fail before a pointer is used


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib
    return _lib.load()


def test_cce_fwd_checks_its_arguments(lib):
    def call(rows=4, classes=6, x=P, target=P, out=P):
        return lib.dei2i_cce_logits_fwd(rows, classes, x, target, out, None)
    for kw in (dict(rows=0), dict(classes=0), dict(classes=-1), dict(x=None), dict(target=None), dict(out=None)):
        assert call(**kw) == BAD_ARG, kw


def test_cce_bwd_checks_its_arguments(lib):
    def call(rows=4, classes=6, x=P, target=P, gout=P, dx=P):
        return lib.dei2i_cce_logits_bwd(rows, classes, x, target, gout, dx, None)
    for kw in (dict(rows=0), dict(classes=0), dict(classes=-1), dict(x=None), dict(target=None), dict(gout=None), dict(dx=None)):
        assert call(**kw) == BAD_ARG, kw


def test_mse_fwd_checks_its_arguments(lib):
    def call(n=16, a=P, b=P, out=P):
        return lib.dei2i_mse_fwd(n, a, b, 0.0, out, None)
    for kw in (dict(n=0), dict(a=None), dict(out=None), dict(n=0, b=None)):
        assert call(**kw) == BAD_ARG, kw


def test_mse_bwd_checks_its_arguments(lib):
    def call(n=16, a=P, b=P, gout=P, da=P, db=P):
        return lib.dei2i_mse_bwd(n, a, b, 0.0, gout, da, db, None)
    for kw in (dict(n=0), dict(a=None), dict(gout=None), dict(n=0, da=None, db=None)):
        assert call(**kw) == BAD_ARG, kw


def test_unknown_loss_kind_names_the_four_kinds():
    from de_i2i_gan_amd.models.base_model import BaseModel, _LOSSES
    assert {"bce", "cce", "l1", "mse"} <= set(_LOSSES)
    with pytest.raises(ValueError) as err:
        BaseModel(SimpleNamespace())._cal_loss(None, None, "nope")
    for kind in ("nope", "bce", "cce", "l1", "mse"):
        assert kind in str(err.value)
