"""GPU: dei2i_blit (csrc/blit.hip) through the C entry point, against the numpy index maps of tests/blit_reference.py.

A permutation moves values and computes nothing, so every comparison is exact.  The images are ``arange`` (a misplaced pixel cannot
hide); a batch of 8 rows holds the 8 codes; the sizes straddle the 32 x 32 tile (31, 32, 33, 64, 65) and the float4 / scalar split
(W % 4, a pointer off the 16-byte grid); both sides of the output carry sentinels."""
import ctypes

import numpy as np
import pytest
import torch

import blit_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
GUARD = 64
SENTINEL = -12345.0
_P = ctypes.c_void_p


def _arange(n, c, h, w):
    return torch.arange(n * c * h * w, dtype=torch.float32).view(n, c, h, w)


def _blit(x, codes, inverse=0, offset=0):
    """the launch on a guarded output; ``offset`` floats shift both buffers off their allocation's alignment"""
    from de_i2i_gan_amd import ops
    n, c, h, w = x.shape
    src = torch.empty(offset + x.numel(), device=DEV)[offset:]
    src.copy_(x.reshape(-1))
    buf = torch.full((offset + GUARD + x.numel() + GUARD,), SENTINEL, device=DEV)
    dst = buf[offset + GUARD:offset + GUARD + x.numel()]
    codes = torch.as_tensor(np.asarray(codes, dtype=np.int64).astype(np.int32)).to(DEV)
    rc = ops._lib_for(src).dei2i_blit(n, c, h, w, _P(codes.data_ptr()), inverse, _P(src.data_ptr()), _P(dst.data_ptr()), ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((buf[:offset + GUARD] == SENTINEL).all()) and bool((buf[offset + GUARD + x.numel():] == SENTINEL).all())
    return dst.view(x.shape).cpu()


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("s", [1, 4, 31, 32, 33, 64, 65])
def test_all_eight_codes_on_square_images(s, c):
    x = _arange(8, c, s, s)
    codes = np.arange(8)
    want = R.blit(x.numpy(), codes)
    got = _blit(x, codes)
    assert np.array_equal(got.numpy(), want), [k for k in range(8) if not np.array_equal(got[k].numpy(), want[k])]
    back = _blit(got, codes, inverse=1)
    assert torch.equal(back, x)
    assert np.array_equal(_blit(x, codes, inverse=1).numpy(), R.blit(x.numpy(), [R.inverse_code(k) for k in codes]))


@pytest.mark.parametrize("h, w, offset", [(5, 12, 0), (7, 33, 0), (5, 12, 1), (33, 64, 3), (3, 6, 0)],
                         ids=["5x12", "7x33", "5x12-unaligned", "33x64-unaligned", "3x6"])
def test_flip_on_non_square_images_and_unaligned_pointers(h, w, offset):
    x = _arange(4, 3, h, w)
    codes = [0, 1, 1, 0]
    got = _blit(x, codes, offset=offset)
    assert np.array_equal(got.numpy(), R.blit(x.numpy(), codes))
    assert torch.equal(got[1], x[1].flip(2)) and torch.equal(got[0], x[0])
    assert torch.equal(_blit(got, codes, inverse=1, offset=offset), x)


def test_unaligned_square_images_take_the_scalar_path():
    x = _arange(8, 2, 36, 36)
    got = _blit(x, np.arange(8), offset=1)
    assert np.array_equal(got.numpy(), R.blit(x.numpy(), np.arange(8)))


def test_garbage_code_words_stay_in_bounds_and_lose_their_rot_bits_off_the_square():
    x = _arange(6, 3, 5, 12)
    words = [0xFFFFFFFF, 0x7FFFFFFE, 6, 7, -8, 0x12345679]          # & 7: 7, 6, 6, 7, 0, 1 -> f only: 1, 0, 0, 1, 0, 1
    for inverse in (0, 1):
        got = _blit(x, np.array(words, dtype=np.int64), inverse=inverse)
        assert np.array_equal(got.numpy(), R.blit(x.numpy(), [1, 0, 0, 1, 0, 1]))
    sq = _arange(3, 1, 33, 33)
    assert np.array_equal(_blit(sq, np.array([0xFFFFFFFF, 0xFFFFFFFA, 8 + 3], dtype=np.int64)).numpy(), R.blit(sq.numpy(), [7, 2, 3]))


@pytest.mark.parametrize("s", [6, 33])
def test_the_inverse_launch_is_the_adjoint_exactly(s):
    """<B x, g> == <x, B^T g> on small integers: every product and partial sum is an integer below 2^24"""
    gen = torch.Generator().manual_seed(s)
    x = torch.randint(-8, 9, (8, 3, s, s), generator=gen).float()
    g = torch.randint(-8, 9, (8, 3, s, s), generator=gen).float()
    codes = np.arange(8)
    bx, btg = _blit(x, codes), _blit(g, codes, inverse=1)
    lhs, rhs = (bx * g).sum(dim=(1, 2, 3)), (x * btg).sum(dim=(1, 2, 3))
    assert torch.equal(lhs, rhs) and bool((lhs != 0).any())


def test_bad_arguments_are_refused():
    from de_i2i_gan_amd import ops
    x = torch.zeros(2 * 3 * 8 * 8, device=DEV)
    y = torch.full((2 * 3 * 8 * 8,), SENTINEL, device=DEV)
    codes = torch.zeros(2, dtype=torch.int32, device=DEV)
    lib = ops._lib_for(x)

    def blit(n=2, c=3, h=8, w=8, table=codes.data_ptr(), src=x.data_ptr(), dst=y.data_ptr()):
        return lib.dei2i_blit(n, c, h, w, _P(table) if table else None, 0, _P(src) if src else None, _P(dst) if dst else None, ops._stream())

    for bad in (dict(n=0), dict(c=0), dict(h=0), dict(w=-1), dict(table=None), dict(src=None), dict(dst=None),
                dict(dst=x.data_ptr()), dict(dst=x.data_ptr() + 16), dict(n=2 ** 20, c=2 ** 10, h=2 ** 10, w=1),
                dict(n=1, c=2 ** 11, h=2 ** 10, w=2 ** 10)):
        assert blit(**bad) == BAD_ARG, bad
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())                               # the refused calls launched nothing
    assert blit() == 0
    torch.cuda.synchronize()
    assert bool((y == 0).all())
