"""The staged BatchNorm entry points (include/dei2i_hip.h: dei2i_bn_sync_*) refuse bad arguments with DEI2I_ERR_BAD_ARG before
anything is launched -- like their one-launch neighbours -- so this runs without a GPU."""
import ctypes

import pytest

from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG

P = ctypes.c_void_p(64)            # any non-null address: the checks below fail before a pointer is used


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib
    return _lib.load()


def test_fwd_sums_checks_its_arguments(lib):
    for groups, n, hw, c, chunks, partial, msg in [(0, 1, 4, 8, 1, P, P), (1, 0, 4, 8, 1, P, P), (1, 1, 0, 8, 1, P, P), (1, 1, 4, 0, 1, P, P),
                                                   (1, 1, 4, 8, 0, P, P), (1, 1, 4, 8, 1, None, P), (1, 1, 4, 8, 1, P, None)]:
        assert lib.dei2i_bn_sync_fwd_sums(groups, n, hw, c, chunks, partial, msg, None) == BAD_ARG


def test_fwd_finalize_checks_its_arguments(lib):
    def call(groups=1, c=8, msg=P, weight=P, bias=P, rm=P, rv=P, stride=8, mean=P, rstd=P, a=P, b=P):
        return lib.dei2i_bn_sync_fwd_finalize(groups, c, msg, weight, bias, rm, rv, stride, 0.1, 1e-5, mean, rstd, a, b, None, None)
    for kw in (dict(groups=0), dict(c=0), dict(msg=None), dict(weight=None), dict(bias=None), dict(mean=None), dict(rstd=None), dict(a=None),
               dict(b=None), dict(rv=None), dict(rm=None), dict(groups=2, stride=4)):       # one running buffer only; groups closer than C
        assert call(**kw) == BAD_ARG, kw


def test_bwd_sums_checks_its_arguments(lib):
    def call(groups=1, c=8, partial=P, chunks=1, sums=P, dw=P, db=P):
        return lib.dei2i_bn_sync_bwd_sums(groups, c, partial, chunks, sums, dw, db, 0, None)
    for kw in (dict(groups=0), dict(c=0), dict(partial=None), dict(chunks=0), dict(sums=None), dict(dw=None), dict(db=None)):
        assert call(**kw) == BAD_ARG, kw


@pytest.mark.parametrize("dtype", [0, 1])
def test_bwd_apply_checks_its_arguments(lib, dtype):
    def call(groups=1, pixels=16, count=32, c=8, dz=P, y=P, a=P, b=P, mean=P, rstd=P, sums=P, gsum=P, dy=P):
        return lib.dei2i_bn_sync_bwd_apply(dtype, groups, pixels, count, c, dz, y, a, b, mean, rstd, 2, sums, gsum, dy, None)
    for kw in (dict(groups=0), dict(pixels=0), dict(count=8), dict(c=6), dict(c=0), dict(dz=None), dict(y=None), dict(a=None), dict(b=None),
               dict(mean=None), dict(rstd=None), dict(sums=None), dict(gsum=None), dict(dy=None)):   # count: not below this process's pixels
        assert call(**kw) == BAD_ARG, kw
