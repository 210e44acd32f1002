"""The entry points of csrc/adam.hip and csrc/spectral.hip and the three layout conversions of csrc/elementwise.hip refuse bad
arguments with DEI2I_ERR_BAD_ARG before anything is launched (the pattern of test_bn_sync_args_cpu.py), so this runs without a GPU;
dei2i_spectral_scratch_floats is host arithmetic and is checked at the shapes of test_spectral_edges_gpu.py."""
import ctypes

import pytest

from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
P = ctypes.c_void_p(64)            # any non-null address: the checks below fail before a pointer is used

# (Cout, Cin, kh, kw) of test_spectral_edges_gpu.py
SPECTRAL_SHAPES = [(63, 7, 3, 3), (65, 16, 2, 2), (80, 65, 1, 1), (80, 3, 3, 3), (3, 257, 1, 1), (3, 513, 1, 1), (2, 1025, 1, 1),
                   (257, 8, 1, 1), (300, 4, 3, 3), (4, 1028, 4, 4), (257, 2049, 1, 1), (264, 500, 2, 2)]


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib
    return _lib.load()


TABLE_BAD = (dict(table=None), dict(count=0), dict(count=-1), dict(max_n=0), dict(max_n=-4))


@pytest.mark.parametrize("name", ["dei2i_adam_step", "dei2i_adam_step_l2"])
def test_adam_step_checks_its_arguments(lib, name):
    def call(table=P, count=1, max_n=8):
        return getattr(lib, name)(table, count, max_n, 1e-3, 0.5, 0.999, 1e-8, 0.5, 0.5, 1.0, 0.0, None)
    for kw in TABLE_BAD:
        assert call(**kw) == BAD_ARG, kw


@pytest.mark.parametrize("coupled", [False, True])
def test_adam_step_dev_checks_its_arguments(lib, coupled):
    def call(table=P, count=1, max_n=8, hyper=P, index=P, rows=4):
        if coupled:
            return lib.dei2i_adam_step_l2_dev(table, count, max_n, hyper, index, rows, 0.5, 0.999, 1e-8, 1.0, 1e-2, None)
        return lib.dei2i_adam_step_dev(table, count, max_n, hyper, index, rows, 0.5, 0.999, 1e-8, 1.0, None)
    for kw in TABLE_BAD + (dict(hyper=None), dict(index=None), dict(rows=0), dict(rows=-1)):
        assert call(**kw) == BAD_ARG, kw


def test_sgd_rmsprop_step_checks_its_arguments(lib):
    def call(table=P, count=1, max_n=8, kind=0):
        return lib.dei2i_sgd_rmsprop_step(table, count, max_n, kind, 1e-3, 0.99, 1e-8, 1.0, None)
    for kw in TABLE_BAD + (dict(kind=-1), dict(kind=2)):
        assert call(**kw) == BAD_ARG, kw


def test_ema_lerp_and_index_advance_check_their_arguments(lib):
    def call(table=P, count=1, max_n=8):
        return lib.dei2i_ema_lerp(table, count, max_n, 0.999, None)
    for kw in TABLE_BAD:
        assert call(**kw) == BAD_ARG, kw
    assert lib.dei2i_index_advance(None, None) == BAD_ARG


def test_spectral_fwd_checks_its_arguments(lib):
    def call(cout=8, k=16, w=P, u=P, v=P, scratch=P, u_used=P, v_used=P, scal=P, w_eff=P, iterate=1):
        return lib.dei2i_spectral_fwd(cout, k, w, u, v, iterate, scratch, u_used, v_used, scal, w_eff, None)
    for iterate in (0, 1):
        for kw in (dict(cout=0), dict(cout=-1), dict(k=0), dict(k=-1), dict(w=None), dict(u=None), dict(v=None), dict(scratch=None),
                   dict(u_used=None), dict(v_used=None), dict(scal=None), dict(w_eff=None)):
            assert call(iterate=iterate, **kw) == BAD_ARG, (iterate, kw)


def test_spectral_bwd_checks_its_arguments(lib):
    def call(cout=8, k=16, g=P, w_eff=P, u_used=P, v_used=P, scal=P, scratch=P, dw=P, accumulate=0):
        return lib.dei2i_spectral_bwd(cout, k, g, w_eff, u_used, v_used, scal, scratch, dw, accumulate, None)
    for accumulate in (0, 1):
        for kw in (dict(cout=0), dict(cout=-1), dict(k=0), dict(k=-1), dict(g=None), dict(w_eff=None), dict(u_used=None),
                   dict(v_used=None), dict(scal=None), dict(scratch=None), dict(dw=None)):
            assert call(accumulate=accumulate, **kw) == BAD_ARG, (accumulate, kw)


def test_fold_bn_weight_checks_its_arguments(lib):
    def call(cout=8, k=16, w=P, bn_w=P, bn_b=P, rm=P, rv=P, w_eff=P, b_eff=P):
        return lib.dei2i_fold_bn_weight(cout, k, w, bn_w, bn_b, rm, rv, 1e-5, w_eff, b_eff, None)
    for kw in (dict(cout=0), dict(cout=-1), dict(k=0), dict(k=-1), dict(w=None), dict(bn_w=None), dict(bn_b=None), dict(rm=None),
               dict(rv=None), dict(w_eff=None), dict(b_eff=None)):
        assert call(**kw) == BAD_ARG, kw


@pytest.mark.parametrize("shape", SPECTRAL_SHAPES)
def test_spectral_scratch_floats(lib, shape):
    cout, k = shape[0], shape[1] * shape[2] * shape[3]
    assert lib.dei2i_spectral_scratch_floats(cout, k) == k + 2 * cout + (k + 63) // 64 + 1024


@pytest.mark.parametrize("dtype,vec", [(0, 8), (1, 4)])
def test_layout_entry_points_check_their_arguments(lib, dtype, vec):
    def resize(n=1, c=3, hs=4, ws=5, h=8, w=3, cs=vec, src=P, dst=P):
        return lib.dei2i_nchw_to_nhwc_resize(dtype, n, c, hs, ws, h, w, cs, src, dst, None)

    def to_nhwc(n=1, c=3, h=4, w=5, cs=vec, src=P, dst=P):
        return lib.dei2i_nchw_to_nhwc(dtype, n, c, h, w, cs, src, dst, None)

    def to_nchw(n=1, c=3, h=4, w=5, cs=vec, src=P, dst=P):
        return lib.dei2i_nhwc_to_nchw(dtype, n, c, h, w, cs, src, dst, None)

    common = (dict(n=0), dict(n=-1), dict(c=0), dict(c=-1), dict(h=0), dict(h=-1), dict(w=0), dict(w=-1), dict(src=None), dict(dst=None),
              dict(c=vec + 1), dict(c=2 * vec, cs=vec),                        # Cs < C
              dict(cs=vec + 1), dict(cs=vec - 1), dict(c=1, cs=vec // 2))      # Cs % vec != 0 (the last two with Cs >= C)
    for kw in common + (dict(hs=0), dict(hs=-1), dict(ws=0), dict(ws=-1)):
        assert resize(**kw) == BAD_ARG, kw
    for kw in common:
        assert to_nhwc(**kw) == BAD_ARG, kw
        assert to_nchw(**kw) == BAD_ARG, kw
