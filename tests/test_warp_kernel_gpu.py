"""GPU: ``dei2i_warp`` (csrc/warp.hip) driven with hand-written record tables, forward and adjoint, against the numpy reference of
tests/warp_reference.py BIT FOR BIT, and against the kernels it must agree with where the maps coincide (dei2i_blit for the eight
dihedral matrices, the translation launch of dei2i_diffaug for integer shifts).  Both buffers of every launch lie between sentinel
guard bands that are compared afterwards: bounds are checked by value.  The workgroup tile is 32 x 8 pixels and the adjoint sums
four channels per pass, so the shapes straddle 8 rows, 32 columns and 4 channels."""
import ctypes

import numpy as np
import pytest
import torch

import blit_reference as B
import warp_reference as R
from test_warp_cpu import GARBAGE, _random_usable, _rotation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
GUARD = 256
SENTINEL = 0x7FC5A5A5          # a NaN pattern no kernel writes


class Guarded:
    """``numel`` fp32 words between two sentinel bands; ``off``: the interior starts ``off`` floats past a 16-byte boundary"""

    def __init__(self, numel, off=0, fill=None):
        self.lo, self.numel = GUARD + off, numel
        self.flat = torch.full((numel + 2 * GUARD + off,), SENTINEL, dtype=torch.int32, device=DEV)
        assert (self.flat.data_ptr() + 4 * self.lo) % 16 == 4 * off
        if fill is not None:
            self.flat[self.lo:self.lo + numel] = torch.from_numpy(np.ascontiguousarray(fill, dtype=F).reshape(-1)).view(torch.int32).to(DEV)
        self.ptr = ctypes.c_void_p(self.flat.data_ptr() + 4 * self.lo)

    def check(self):
        assert bool((self.flat[:self.lo] == SENTINEL).all()) and bool((self.flat[self.lo + self.numel:] == SENTINEL).all()), \
            "a write outside the buffer"

    def values(self, shape):
        return self.flat[self.lo:self.lo + self.numel].cpu().view(torch.float32).reshape(shape).numpy()


def _table(rec):
    rec = np.asarray(rec, dtype=F)
    tab = np.zeros((len(rec), 8), dtype=F)
    tab[:, :rec.shape[1]] = rec
    return torch.from_numpy(tab).to(DEV)


def launch(x, rec, adjoint, src_off=0, dst_off=0):
    """one dei2i_warp call on a numpy (N, C, H, W) batch -> numpy output; both buffers guarded, the source compared afterwards"""
    from de_i2i_gan_amd import ops
    x = np.ascontiguousarray(x, dtype=F)
    n, c, h, w = x.shape
    tab = _table(rec)
    src, dst = Guarded(x.size, src_off, fill=x), Guarded(x.size, dst_off)
    lib = ops._lib_for(tab)
    assert lib.dei2i_warp(n, c, h, w, ctypes.c_void_p(tab.data_ptr()), adjoint, src.ptr, dst.ptr, ops._stream()) == 0
    torch.cuda.synchronize()
    src.check(), dst.check()
    assert np.array_equal(src.values(x.shape).view(np.int32), x.view(np.int32)), "the launch wrote to its input"
    return dst.values(x.shape)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, dtype=F).view(np.int32), np.asarray(b, dtype=F).view(np.int32))


def _data(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


SHAPES = [(1, 1, 1, 1), (3, 3, 5, 7), (2, 1, 33, 65), (1, 3, 64, 64), (1, 2, 8, 32), (1, 1, 9, 33), (1, 1, 7, 31), (2, 4, 3, 3), (1, 5, 6, 5),
          (1, 9, 2, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_forward_and_adjoint_equal_the_reference_bit_for_bit(shape):
    x = _data(shape, 1)
    for seed in (0, 1):
        rec = _random_usable(shape[0], seed)                          # another matrix per sample
        rec[:, 4:6] = np.random.default_rng(seed).uniform(-1.5, 1.5, (shape[0], 2))
        assert same_bits(launch(x, rec, 0), R.forward(x, rec)), ("forward", seed)
        assert same_bits(launch(x, rec, 1), R.adjoint(x, rec)), ("adjoint", seed)


def test_input_and_output_one_float_off_16_byte_alignment():
    x = _data((2, 3, 9, 12), 2)
    rec = _random_usable(2, 5)
    for src_off, dst_off in ((1, 0), (0, 1), (1, 1), (3, 2)):
        assert same_bits(launch(x, rec, 0, src_off, dst_off), R.forward(x, rec))
        assert same_bits(launch(x, rec, 1, src_off, dst_off), R.adjoint(x, rec))


def test_the_identity_matrix_returns_the_input():
    for shape in ((2, 3, 33, 65), (1, 1, 1, 1), (1, 2, 8, 32)):
        x = torch.from_numpy(_data(shape, 3))
        ident = [R.IDENTITY] * shape[0]
        assert torch.equal(torch.from_numpy(launch(x.numpy(), ident, 0)), x)
        assert torch.equal(torch.from_numpy(launch(x.numpy(), ident, 1)), x)


def _dihedral(code, s):
    """the sampling matrix of blit code f | k << 1 on an s x s image, read off tests/blit_reference.py's index map"""
    i, j = s // 2, s // 2
    (a, b), (ai, bi), (aj, bj) = (B.source_index(code, i, j, s, s), B.source_index(code, i + 1, j, s, s), B.source_index(code, i, j + 1, s, s))
    return [bj - b, bi - b, aj - a, ai - a, 0, 0]


@pytest.mark.parametrize("s", [9, 32])
def test_the_quarter_turn_and_mirror_matrices_equal_the_blit_kernel(s):
    from de_i2i_gan_amd import ops
    x = _data((8, 2, s, s), 4)
    rec = np.array([_dihedral(code, s) for code in range(8)], dtype=F)
    assert sorted(map(tuple, rec[[0, 2, 4, 6], :4].tolist())) == sorted([(1, 0, 0, 1), (0, -1, 1, 0), (-1, 0, 0, -1), (0, 1, -1, 0)])
    xd = torch.from_numpy(x).to(DEV)
    codes = torch.arange(8, dtype=torch.int32, device=DEV)
    for inverse in (0, 1):
        want = torch.empty_like(xd)
        assert ops._lib_for(xd).dei2i_blit(8, 2, s, s, ops._p(codes), inverse, ops._p(xd), ops._p(want), ops._stream()) == 0
        assert torch.equal(torch.from_numpy(launch(x, rec, inverse)).to(DEV), want), inverse
    assert same_bits(launch(x, rec, 0), B.blit(x, np.arange(8)))


def test_integer_shifts_equal_the_translation_launch():
    from de_i2i_gan_amd import ops
    h, w = 6, 9
    shifts = [(0, 0), (1, 0), (0, -1), (-2, 3), (5, 8), (-5, -8), (6, 0), (0, 9), (-6, 2), (7, -12), (100, 100)]          # (tv, tu), some >= H or W
    n = len(shifts)
    x = _data((n, 3, h, w), 5)
    rec = np.array([[1, 0, 0, 1, tu, tv] for tv, tu in shifts], dtype=F)
    tab = np.zeros((n, 8), dtype=np.int32)
    tab.view(F)[:, 0] = 1
    tab[:, 4], tab[:, 5] = [s[0] for s in shifts], [s[1] for s in shifts]
    xd, td = torch.from_numpy(x).to(DEV), torch.from_numpy(tab).to(DEV)
    for mode, adjoint in ((0, 0), (2, 1)):
        want = torch.empty_like(xd)
        assert ops._lib_for(xd).dei2i_diffaug(mode, n, 3, h, w, 0, 0, 0, ops._p(xd), ops._p(td), None, ops._p(want), ops._stream()) == 0
        assert torch.equal(torch.from_numpy(launch(x, rec, adjoint)).to(DEV), want), mode
    assert not launch(x, rec, 0)[-1].any()


def test_magnification_and_minification_by_two_along_each_axis():
    x = _data((4, 2, 10, 13), 6)
    rec = np.array([[2, 0, 0, 1, 0, 0], [0.5, 0, 0, 1, 0, 0], [1, 0, 0, 2, 0, 0], [1, 0, 0, 0.5, 0, 0]], dtype=F)
    assert same_bits(launch(x, rec, 0), R.forward(x, rec)) and same_bits(launch(x, rec, 1), R.adjoint(x, rec))
    both = np.array([[2, 0, 0, 2, 0, 0], [0.5, 0, 0, 0.5, 0, 0], [2, 0, 0, 0.5, 0, 0], [0.5, 0, 0, 2, 0, 0]], dtype=F)
    assert same_bits(launch(x, both, 0), R.forward(x, both)) and same_bits(launch(x, both, 1), R.adjoint(x, both))


def test_rotation_by_45_degrees_with_taps_leaving_through_every_edge_and_corner():
    h, w = 9, 11
    rows, want = [], {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)} - {(0, 0)}          # (row side, column side) a tap pair leaves by
    seen = set()
    for tv in np.arange(-4, 4.5, 0.5):
        for tu in np.arange(-5, 5.5, 0.5):
            row = _rotation(45)[:4] + [tu, tv]
            valid, u0, v0, _ = R.taps(np.array(row, dtype=F), h, w)
            sides = {((-1 if v < 0 else 1 if v + 1 >= h else 0), (-1 if u < 0 else 1 if u + 1 >= w else 0)) for u, v in zip(u0[valid], v0[valid])}
            if sides - seen:
                rows.append(row)
                seen |= sides
    assert want <= seen and len(rows) >= 1                                # every edge and every corner, by the reference's own taps
    rows.append(_rotation(45, s=1.5))
    rec = np.array(rows, dtype=F)
    x = _data((len(rows), 2, h, w), 7)
    assert same_bits(launch(x, rec, 0), R.forward(x, rec)) and same_bits(launch(x, rec, 1), R.adjoint(x, rec))


def test_the_adjoint_launch_is_the_transpose_of_the_forward_launch():
    h, w = 5, 7
    basis = np.eye(h * w, dtype=F).reshape(h * w, 1, h, w)
    for row in (_random_usable(1, 9)[0], np.array(_rotation(45, s=0.75), dtype=F), np.array([0.5, 0, 0, 2, 0.5, -0.25], dtype=F)):
        rec = np.repeat(row[None], h * w, axis=0)
        fwd = launch(basis, rec, 0).reshape(h * w, h * w)                 # row k: the forward of basis image k
        adj = launch(basis, rec, 1).reshape(h * w, h * w)
        assert fwd.any() and same_bits(adj, np.ascontiguousarray(fwd.T))


def test_garbage_tables_are_the_identity_and_stay_inside_the_buffers():
    for shape in ((len(GARBAGE), 3, 5, 7), (len(GARBAGE), 1, 33, 65)):
        x = torch.from_numpy(_data(shape, 8))
        for adjoint in (0, 1):
            assert torch.equal(torch.from_numpy(launch(x.numpy(), GARBAGE, adjoint)), x)          # (launch compares all four guard bands)
    words = np.array([0x7FC00000, 0xFF800000, 0x7F800000, 0, 0x7149F2CA, 1, 0x80000001, 0xFFFFFFFF], dtype=np.uint32)
    tab = np.random.default_rng(0).choice(words, size=(64, 8)).view(F)          # NaN, +-inf, zeros, 1e30, denormals in every slot
    x = _data((64, 2, 6, 9), 9)
    for adjoint in (0, 1):
        got = launch(x, tab[:, :6], adjoint)
        assert same_bits(got, R.forward(x, tab[:, :6]) if not adjoint else R.adjoint(x, tab[:, :6]))
    huge = np.array([[1, 0, 0, 1, 3e38, 3e38], [4, 0, 0, 0.25, -3e38, 0], [0.25, 0, 0, 0.25, 1e9, -1e9]], dtype=F)      # usable, wholly outside
    x = _data((3, 2, 6, 9), 10)
    assert not launch(x, huge, 0).any() and not launch(x, huge, 1).any()


def test_bad_arguments_are_refused():
    from de_i2i_gan_amd import ops
    from de_i2i_gan_amd._lib import ERR_BAD_ARG
    x = torch.zeros(2 * 3 * 4 * 5 + 8, dtype=torch.float32, device=DEV)
    y = torch.full((2 * 3 * 4 * 5,), 7.0, dtype=torch.float32, device=DEV)
    tab = _table([R.IDENTITY] * 2)
    lib, st = ops._lib_for(x), ops._stream()
    px, py, pt = (ctypes.c_void_p(t.data_ptr()) for t in (x, y, tab))

    def call(n=2, c=3, h=4, w=5, t=pt, adjoint=0, src=px, dst=py):
        return lib.dei2i_warp(n, c, h, w, t, adjoint, src, dst, st)

    assert call() == 0
    y.fill_(7.0)
    for bad in (dict(t=None), dict(src=None), dict(dst=None), dict(n=0), dict(c=-1), dict(h=0), dict(w=0), dict(dst=px),
                dict(dst=ctypes.c_void_p(x.data_ptr() + 16)), dict(n=2 ** 20, c=2 ** 10, h=2 ** 5, w=2 ** 5), dict(c=2 ** 11, h=2 ** 10, w=2 ** 10),
                dict(n=1, c=1, h=1, w=2 ** 16 + 1), dict(n=1, c=1, h=2 ** 16 + 1, w=1)):
        for adjoint in (0, 1):
            assert call(adjoint=adjoint, **bad) == ERR_BAD_ARG, bad
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                     # the refused calls launched nothing


def test_two_launches_are_bit_identical():
    x = _data((3, 3, 33, 65), 11)
    rec = _random_usable(3, 12)
    for adjoint in (0, 1):
        assert same_bits(launch(x, rec, adjoint), launch(x, rec, adjoint))
