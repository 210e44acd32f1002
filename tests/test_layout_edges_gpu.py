"""The layout conversions at the module boundary (nchw_to_nhwc_kernel / nhwc_to_nchw_kernel, csrc/elementwise.hip) through their
three C entry points, bit for bit in both compute dtypes.  The test owns every destination: it is carved out of a buffer with 64 spare
elements on each side, all pre-filled with a NaN sentinel, so a lane the kernel does not write (the zero-padded channels included)
and a write past either end both show.  Seams: the 16-byte channel vectors (8 bf16 / 4 fp32 lanes; C = 3, 20, 1 leave partly padded
vectors, C = 8 none), the fused nearest resize ``src = floor(dst * in / out)`` that every label map takes, the grid cap of 4096
workgroups x 256 threads and the grid-stride trip behind it, and the fp32 -> bf16 rounding at ties, the overflow edge, +-inf, NaN.

The resize reference is the integer rule of the kernel's comment; it is asserted equal to F.interpolate(mode="nearest") on the CPU
at every size pair used here.  The two are NOT equal everywhere: torch scales by an fp32 factor that rounds across an integer for a
few (in, out) pairs (DESIGN.md section 4 lists them); those pairs are the documented difference and are not tested."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
DTYPES = ["bf16", "f32"]
SENTINEL = {"bf16": 0x7FC1, "f32": 0x7FC0ABCD}                        # quiet NaNs with a payload
RESIZE_PAIRS = [((5, 7), (8, 3)), ((3, 4), (7, 9)), ((7, 5), (7, 5)), ((1, 1), (4, 6)), ((16, 16), (4, 4)), ((4, 4), (16, 16))]
CANARY_SHAPES = [(2, 3, 5, 7), (1, 20, 3, 5), (3, 8, 1, 1), (1, 1, 9, 1)]


def prec_of(pname):
    from de_i2i_gan_amd import ops
    return ops.BF16 if pname == "bf16" else ops.F32


def itype(dtype):
    return torch.int16 if dtype == torch.bfloat16 else torch.int32


def bits(t):
    return t.contiguous().view(itype(t.dtype))


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib as L
    from de_i2i_gan_amd import ops
    ops._lib_for(torch.empty(1, device=DEV))
    return L.load()


def stream():
    from de_i2i_gan_amd import ops
    return ops._stream()


class Guarded:
    """``numel`` elements of ``dtype`` between two guards of GUARD elements, everything pre-filled with the sentinel"""

    def __init__(self, numel, dtype):
        self.numel, self.dtype = numel, dtype
        self.sent = SENTINEL["bf16" if dtype == torch.bfloat16 else "f32"]
        self.flat = torch.full((numel + 2 * GUARD,), self.sent, dtype=itype(dtype), device=DEV)
        self.ptr = ctypes.c_void_p(self.flat.data_ptr() + GUARD * self.flat.element_size())
        assert self.ptr.value % 16 == 0

    def interior(self):
        return self.flat[GUARD:GUARD + self.numel]

    def check(self, ref):
        """every interior element equals ``ref`` (bit patterns), every spare element is still the sentinel"""
        assert (self.flat[:GUARD] == self.sent).all() and (self.flat[GUARD + self.numel:] == self.sent).all(), "a write outside the tensor"
        want = bits(ref).reshape(-1).to(DEV)
        assert want.numel() == self.numel
        assert torch.equal(self.interior(), want), "interior differs (an unwritten lane holds the sentinel)"


def nearest_index(n_out, n_in):
    return (torch.arange(n_out, dtype=torch.int64) * n_in) // n_out   # the kernel's rule: src = floor(dst * in / out)


def ref_nhwc(x, size, prec):
    """NCHW fp32 CPU -> (N, H, W, Cs) of the compute dtype: nearest resize by the integer rule, channels zero-padded"""
    n, c, hs, ws = x.shape
    h, w = size
    g = x[:, :, nearest_index(h, hs)][:, :, :, nearest_index(w, ws)]
    out = torch.zeros(n, h, w, prec.pad(c), dtype=torch.float32)
    out[..., :c] = g.permute(0, 2, 3, 1)
    return out.to(prec.dtype)


def to_nhwc_direct(lib, x, size, prec, resize_entry=True):
    n, c, hs, ws = x.shape
    h, w = size
    cs = prec.pad(c)
    dst = Guarded(n * h * w * cs, prec.dtype)
    xd = x.to(DEV)
    if resize_entry:
        rc = lib.dei2i_nchw_to_nhwc_resize(prec.code, n, c, hs, ws, h, w, cs, ctypes.c_void_p(xd.data_ptr()), dst.ptr, stream())
    else:
        assert (h, w) == (hs, ws)
        rc = lib.dei2i_nchw_to_nhwc(prec.code, n, c, h, w, cs, ctypes.c_void_p(xd.data_ptr()), dst.ptr, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return dst


def to_nchw_direct(lib, nhwc, c):
    """nhwc: CPU (N, H, W, Cs) tensor of the compute dtype -> Guarded fp32 NCHW destination"""
    n, h, w, cs = nhwc.shape
    prec = prec_of("bf16" if nhwc.dtype == torch.bfloat16 else "f32")
    dst = Guarded(n * c * h * w, torch.float32)
    src = nhwc.to(DEV)
    assert lib.dei2i_nhwc_to_nchw(prec.code, n, c, h, w, cs, ctypes.c_void_p(src.data_ptr()), dst.ptr, stream()) == 0
    torch.cuda.synchronize()
    return dst


# ---- a. canary ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", CANARY_SHAPES)
def test_canary_both_directions(lib, shape, pname):
    prec = prec_of(pname)
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(5 + c)
    x = torch.randn(shape, generator=gen)
    ref = ref_nhwc(x, (h, w), prec)
    assert not bits(ref)[..., c:].any()                                # the padded lanes of the reference are +0
    to_nhwc_direct(lib, x, (h, w), prec, resize_entry=False).check(ref)
    to_nhwc_direct(lib, x, (h, w), prec, resize_entry=True).check(ref)
    # back: the padded lanes of the source hold garbage that must not reach the output
    src = ref.clone()
    src[..., c:] = 7.0
    to_nchw_direct(lib, src, c).check(src[..., :c].permute(0, 3, 1, 2).float().contiguous())


# ---- b. the fused nearest resize --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RESIZE_PAIRS)
def test_integer_rule_equals_torch_nearest_at_the_tested_sizes(pair):
    (hs, ws), (h, w) = pair
    x = torch.arange(2 * 3 * hs * ws, dtype=torch.float32).reshape(2, 3, hs, ws)
    mine = x[:, :, nearest_index(h, hs)][:, :, :, nearest_index(w, ws)]
    assert torch.equal(mine, F.interpolate(x, size=(h, w), mode="nearest"))


@gpu
@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("pair", RESIZE_PAIRS)
def test_nearest_resize(lib, pair, pname):
    from de_i2i_gan_amd import ops
    prec = prec_of(pname)
    (hs, ws), (h, w) = pair
    gen = torch.Generator().manual_seed(hs * 100 + w)
    x = torch.randn(2, 3, hs, ws, generator=gen)
    ref = ref_nhwc(x, (h, w), prec)
    torch_ref = torch.zeros_like(ref)
    torch_ref[..., :3] = F.interpolate(x, size=(h, w), mode="nearest").permute(0, 2, 3, 1).to(prec.dtype)
    assert torch.equal(bits(ref), bits(torch_ref))
    dst = to_nhwc_direct(lib, x, (h, w), prec)
    dst.check(ref)
    xg = x.to(DEV).requires_grad_(True)
    out = ops.to_nhwc(xg, prec, size=(h, w))
    assert out.shape == ref.shape and out.dtype == prec.dtype
    assert torch.equal(bits(out.detach()).reshape(-1), dst.interior())
    if (h, w) != (hs, ws):
        with pytest.raises(RuntimeError, match="nearest resize"):
            out.float().sum().backward()


# ---- c. past the grid cap ---------------------------------------------------------------------------------------------------------
@gpu
def test_resize_past_the_grid_cap(lib):
    """(1, 3, 7, 5) -> 1025 x 1025 in bf16: 1 050 625 channel vectors, 2 049 more than 4096 x 256 threads"""
    prec = prec_of("bf16")
    x = torch.randn(1, 3, 7, 5, generator=torch.Generator().manual_seed(9))
    assert 1025 * 1025 > 4096 * 256
    to_nhwc_direct(lib, x, (1025, 1025), prec).check(ref_nhwc(x, (1025, 1025), prec))


@gpu
@pytest.mark.parametrize("pname", DTYPES)
def test_to_nchw_past_the_grid_cap(lib, pname):
    """(1, 3, 1025, 1025): 3 151 875 items, three trips of the 4096 x 256 grid and a partial fourth"""
    prec = prec_of(pname)
    gen = torch.Generator().manual_seed(10)
    src = torch.randn(1, 1025, 1025, prec.pad(3), generator=gen).to(prec.dtype)
    to_nchw_direct(lib, src, 3).check(src[..., :3].permute(0, 3, 1, 2).float().contiguous())


# ---- d. fp32 -> bf16 rounding -------------------------------------------------------------------------------------------------------
def f32_from_bits(*patterns):
    return torch.tensor(patterns, dtype=torch.int64).to(torch.int32).view(torch.float32)


@gpu
def test_bf16_rounding_edges(lib):
    prec = prec_of("bf16")
    special = torch.cat([
        torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 65504.0]),
        torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)]),   # ties: to the even 1.0, up to the even 1 + 2^-6, and negative
        f32_from_bits(0x7F7F7FFF, 0x7F7F8000),                               # just below the overflow tie -> bf16 max; the tie -> inf
    ])
    gen = torch.Generator().manual_seed(12)
    rnd = torch.randn(256 - special.numel(), generator=gen)
    rnd[::2] *= 2.0 ** 30
    rnd[1::2] *= 2.0 ** -30
    x = torch.cat([special, rnd]).reshape(1, 8, 4, 8)
    fin = x[torch.isfinite(x) & (x != 0)]
    assert (fin.abs() >= 2.0 ** -126).all()                            # no denormal inputs
    want = x.to(torch.bfloat16)
    # the reference rounds as the comments above say (65504 -> 65536 = 0x4780)
    wb = (bits(want).reshape(-1).to(torch.int32) & 0xFFFF).tolist()
    assert wb[:4] == [0x0000, 0x8000, 0x7F80, 0xFF80] and wb[5:11] == [0x4780, 0x3F80, 0x3F82, 0xBF80, 0x7F7F, 0x7F80]
    ref = want.permute(0, 2, 3, 1).contiguous()                        # (1, 4, 8, 8): C = Cs = 8
    dst = to_nhwc_direct(lib, x, (4, 8), prec)
    assert (dst.flat[:GUARD] == dst.sent).all() and (dst.flat[GUARD + dst.numel:] == dst.sent).all()
    got = dst.interior().cpu().view(torch.bfloat16).reshape(ref.shape)
    nan = ref.isnan()
    assert nan.sum() == 1 and torch.equal(got.isnan(), nan)            # NaN stays NaN (payload not compared)
    assert torch.equal(bits(got)[~nan], bits(ref)[~nan])
    # and back: bf16 -> fp32 is exact
    back = to_nchw_direct(lib, got, 8)
    out = back.interior().cpu().view(torch.float32).reshape(1, 8, 4, 8)
    wantf = got.permute(0, 3, 1, 2).float().contiguous()
    nanf = wantf.isnan()
    assert torch.equal(out.isnan(), nanf) and torch.equal(bits(out)[~nanf], bits(wantf)[~nanf])
