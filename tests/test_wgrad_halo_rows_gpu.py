"""The halo-resident wgrad kernel (csrc/wgrad_halo.hip) on the smallest shapes its halo-row loop can go wrong on.

The 9-taps-per-wave instances (<128,64,1,*>, <64,128,1,*>) walk a half-tile by HALO row: the fragment of halo row hy serves
tap row ty of tile row hy - ty.  A dropped, doubled or mis-paired (row, tap) product shows on one 4 x 32 half-tile already, so
the shapes here are tiny and the kernel is forced (option wgrad_halo = 2; such shapes normally stay on wgrad_v2 / v1).

Reference: oracle.defectgan_oracle.conv2d (+ upsample2x) in float64 on bf16-rounded operands; tolerance: test_ops_gpu.py's
bf16 bound (1.5e-2 of the tensor's max).  The exact cases use integer data (|x|, |dy| <= 3, at most 2 048 pixels: every
dw element is an integer below 2^24) and ask for equality.

The operand-path (PRO) instances are driven through the library's entry point dei2i_conv2d_wgrad_oihw_pro with hand-made
coefficients / ring tensors: the fused FORWARD kernels that ops.spade_conv / ops.bn_act_conv need refuse images this small
(dei2i_conv2d_fused_supported / _ring_supported want half a chip of tiles), the weight-gradient entry point does not.  The
reference for them is the unfused composition: z = act(A * x + B) rounded to bf16 (ring pixels taken from the ring tensor),
then the oracle's conv."""
import math
from ctypes import byref, c_void_p

import pytest
import torch

from oracle import defectgan_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1.5e-2             # test_ops_gpu.py TOL["bf16"]


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


@pytest.fixture()
def forced(ops, request):
    """force the halo wgrad kernel; count its launches"""
    from de_i2i_gan_amd import _lib
    lib = _lib.load()
    lib.dei2i_set_option(b"wgrad_halo", 2)
    request.addfinalizer(lambda: lib.dei2i_set_option(b"wgrad_halo", 1))
    _lib.launch_counts(reset=True)
    return lambda: _lib.launch_counts(reset=True).get("wgrad_halo", 0)


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def nhwc(t, cs=None):
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, cs or c, dtype=t.dtype)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


def bf16r(t):
    return t.bfloat16().float()


def int_pattern(n, c, h, w):
    """integers in [-3, 3] that depend on row, column, channel and image: no two taps see the same shifted image"""
    i, ch, y, x = torch.meshgrid(torch.arange(n), torch.arange(c), torch.arange(h), torch.arange(w), indexing="ij")
    return ((3 * y + x + 2 * ch + 5 * i) % 7 - 3).float()


def ref_grads(x, w, gy, reflect, up):
    """float64 (dx, dw) of the oracle's conv on operands that are already bf16-representable"""
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = O.conv2d(O.upsample2x(xr) if up else xr, wr, stride=1, pad=1, mode="reflect" if reflect else "zeros")
    return torch.autograd.grad(y, [xr, wr], gy.double())


def run_conv_backward(ops, x, w, gy, reflect, up):
    cout, cin = w.shape[:2]
    prec = ops.BF16
    xg = x.to(DEV).requires_grad_(True)
    wg = w.to(DEV).requires_grad_(True)
    geom = ops.ConvGeom(cin, cout, 3, 1, 1, reflect, up)
    y = ops.conv2d(ops.to_nhwc(xg, prec), wg, None, ops.PackedWeights(), geom, "none")
    y.backward(nhwc(gy, prec.pad(cout)).to(DEV).to(prec.dtype))
    torch.cuda.synchronize()
    return xg.grad, wg.grad


# (cin, cout, H, W (source), N, reflect, up)
CASES = [
    # <128,64>: one half-tile (halo rows 0 and 5 both reflections; every (hy, ty) pairing exactly once), two tile rows,
    # tile_next wrapping in x, y and image
    (64, 128, 4, 32, 1, True, False),
    (64, 128, 8, 32, 1, True, False),
    (64, 128, 8, 64, 2, True, False),
    # general DMA path: c0 + BCO > ldy (row guards in the write-back); zero padding (zero rows in the halo)
    (128, 96, 8, 32, 2, True, False),
    (64, 128, 8, 32, 2, False, False),
    # <64,128>
    (128, 48, 8, 32, 2, True, False),
    (128, 64, 8, 32, 2, True, False),
    # up-conv read (g.up = 1): source 8 x 16 -> 16 x 32
    (128, 64, 8, 16, 2, True, True),
    (256, 128, 8, 16, 2, True, True),
    # <64,64,2>: the taps-over-two-wave-groups heads variant (tile-row loop, unchanged)
    (64, 4, 16, 32, 4, True, False),
]


@pytest.mark.parametrize("case", CASES)
def test_wgrad_halo_small_shapes(ops, forced, case):
    cin, cout, H, W, N, reflect, up = case
    torch.manual_seed(11 + CASES.index(case))
    x = bf16r(torch.randn(N, cin, H, W))
    w = bf16r(torch.randn(cout, cin, 3, 3) * math.sqrt(2.0 / (cin * 9)))
    gy = bf16r(torch.randn(N, cout, H << up, W << up))
    dx_ref, dw_ref = ref_grads(x, w, gy, reflect, up)
    forced()
    dx, dw = run_conv_backward(ops, x, w, gy, reflect, up)
    assert forced() == 1, "the halo wgrad kernel did not take the shape"
    e_dw, e_dx = maxrel(dw, dw_ref), maxrel(dx, dx_ref)
    print(f"wgrad_halo {case}: dw {e_dw:.3e} dx {e_dx:.3e}")
    assert e_dw < TOL, "wgrad"
    assert e_dx < TOL, "dgrad"


@pytest.mark.parametrize("cin,cout,H,W,N", [(64, 128, 8, 64, 2), (128, 64, 8, 32, 2)])
def test_wgrad_halo_exact_on_integers(ops, forced, cin, cout, H, W, N):
    """<128,64,1,false> / <64,128,1,false>: every (pixel, tap) product once -- integer sums, equal to the reference"""
    assert N * H * W <= 2048
    torch.manual_seed(3)
    x = int_pattern(N, cin, H, W)
    gy = torch.randint(-3, 4, (N, cout, H, W)).float()
    w = bf16r(torch.randn(cout, cin, 3, 3) * 0.05)
    _, dw_ref = ref_grads(x, w, gy, True, False)
    forced()
    _, dw = run_conv_backward(ops, x, w, gy, True, False)
    assert forced() == 1
    assert dw_ref.abs().max().item() < 2 ** 24
    bad = (dw.double().cpu() != dw_ref).sum().item()
    print(f"exact <{cout},{cin}>: {bad} of {dw_ref.numel()} elements differ, max |dw| {dw_ref.abs().max().item():.0f}")
    assert bad == 0


# ---- operand-path (PRO) instances ----------------------------------------------------------------------------------------

def ring_pixels(H, W):
    return 4 * W + 4 * (H - 4)


def ring_coords(H, W):
    """(y, x) of ring pixel r of an H x W frame (csrc/geom.h: rows 0, 1 | rows H-2, H-1 | rows 2 .. H-3: columns 0, 1, W-2, W-1)"""
    out = [(y, x) for y in (0, 1) for x in range(W)] + [(y, x) for y in (H - 2, H - 1) for x in range(W)]
    out += [(y, x) for y in range(2, H - 2) for x in (0, 1, W - 2, W - 1)]
    assert len(out) == ring_pixels(H, W)
    return out


def wgrad_pro(ops, forced, x_nhwc, gy, cin, cout, up, A=None, B=None, n_stride=0, slope=1.0, ring=None):
    """dei2i_conv2d_wgrad_oihw_pro on device tensors -> dw (cout, cin, 3, 3) fp32"""
    from de_i2i_gan_amd import _lib as L
    prec = ops.BF16
    xd = x_nhwc.to(DEV).to(prec.dtype).contiguous()
    gd = nhwc(gy, prec.pad(cout)).to(DEV).to(prec.dtype).contiguous()
    lib = ops._lib_for(xd)
    n, h, w, c = xd.shape
    geom = ops.ConvGeom(cin, cout, 3, 1, 1, True, up)
    d = ops._desc(prec, geom, n, h, w, c, gd.shape[-1])
    assert lib.dei2i_conv2d_wgrad_pro_supported(byref(d))
    scratch = ops._wgrad_scratch(lib, d, xd.device)
    keep = [t.to(DEV).contiguous() if t is not None else None for t in (A, B)]
    rd = ring.to(DEV).to(prec.dtype).contiguous() if ring is not None else None
    pro = L.ProDesc(keep[0].data_ptr() if A is not None else None, keep[1].data_ptr() if B is not None else None, n_stride, slope,
                    rd.data_ptr() if rd is not None else None)
    dw = torch.zeros(cout, cin, 3, 3, dtype=torch.float32, device=DEV)
    forced()
    L.check(lib.dei2i_conv2d_wgrad_oihw_pro(byref(d), ops._p(xd), ops._p(gd), ops._p(scratch), scratch.numel(), c_void_p(dw.data_ptr()), 0,
                                            byref(pro), ops._stream()), "conv2d_wgrad_pro")
    torch.cuda.synchronize()
    assert forced() == 1
    return dw


def act_ref(x, A, B, slope):
    """z = act(A * x + B) per (image, channel) in fp32 like the kernel (one fma, then the leaky branch), rounded to bf16"""
    w = torch.addcmul(B[:, :, None, None], A[:, :, None, None], x)
    return bf16r(torch.where(w > 0, w, slope * w))


def ring_compose(z_src, ring, up):
    """the conv's logical input: nearest x2 of z_src with the two-pixel border ring taken from the ring tensor (N, ring_pix, C)"""
    z = O.upsample2x(z_src) if up else z_src.clone()
    H, W = z.shape[-2:]
    ys, xs = zip(*ring_coords(H, W))
    z[:, :, list(ys), list(xs)] = ring.permute(0, 2, 1)
    return z


def dw_reference(z, gy, cout):
    zr = z.double()
    wr = torch.zeros(cout, z.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(O.conv2d(zr, wr, stride=1, pad=1, mode="reflect"), [wr], gy.double())[0]


@pytest.mark.parametrize("cin,cout", [(128, 64), (256, 128)])
def test_wgrad_halo_pro_ring_redirect(ops, forced, cin, cout):
    """SPADE -> upsample -> conv, ring mode (A == nullptr): the source-resolution z plus the logical frame's ring tensor;
    source 8 x 16, N = 2.  <64,128,1,true> and <128,64,1,true>."""
    N, hs, ws = 2, 8, 16
    torch.manual_seed(21)
    z_src = bf16r(torch.relu(torch.randn(N, cin, hs, ws)))
    ring = bf16r(torch.relu(torch.randn(N, ring_pixels(2 * hs, 2 * ws), cin) + 0.5))
    gy = bf16r(torch.randn(N, cout, 2 * hs, 2 * ws))
    ref = dw_reference(ring_compose(z_src, ring, True), gy, cout)
    dw = wgrad_pro(ops, forced, nhwc(z_src), gy, cin, cout, True, ring=ring)
    e = maxrel(dw, ref)
    print(f"pro ring {cin}->{cout}: dw {e:.3e}")
    assert e < TOL


@pytest.mark.parametrize("kind,cin,cout", [("spade", 128, 64), ("spade", 256, 128), ("bn", 64, 128), ("bn", 128, 64)])
def test_wgrad_halo_pro_transform(ops, forced, kind, cin, cout):
    """the norm on the operand path (ops.fuse_pro): "spade" = per-image coefficients + ReLU behind an upsample, ring pixels from the
    ring tensor (source 8 x 16); "bn" = one coefficient set + LeakyReLU at 8 x 32.  N = 2: the coefficients reload per image."""
    N = 2
    up = kind == "spade"
    hs, ws = (8, 16) if up else (8, 32)
    torch.manual_seed(23)
    x = bf16r(torch.randn(N, cin, hs, ws) * 1.3 + 0.2)
    gy = bf16r(torch.randn(N, cout, hs << up, ws << up))
    if up:
        A, B, slope = 0.5 + torch.rand(N, cin), 0.3 * torch.randn(N, cin), 0.0
        ring = bf16r(torch.relu(torch.randn(N, ring_pixels(2 * hs, 2 * ws), cin) + 0.5))
        z = ring_compose(act_ref(x, A, B, slope), ring, True)
        dw = wgrad_pro(ops, forced, nhwc(x), gy, cin, cout, True, A=A, B=B, n_stride=cin, slope=slope, ring=ring)
    else:
        A, B, slope = 0.5 + torch.rand(1, cin), 0.3 * torch.randn(1, cin), 0.2
        z = act_ref(x, A.expand(N, cin), B.expand(N, cin), slope)
        dw = wgrad_pro(ops, forced, nhwc(x), gy, cin, cout, False, A=A, B=B, n_stride=0, slope=slope)
    e = maxrel(dw, dw_reference(z, gy, cout))
    print(f"pro {kind} {cin}->{cout}: dw {e:.3e}")
    assert e < TOL


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 64)])
def test_wgrad_halo_pro_exact_on_integers(ops, forced, cin, cout):
    """<128,64,1,true> / <64,128,1,true>: z = relu(A * x + B) with integer coefficients per image stays an integer <= 7"""
    N, H, W = 2, 8, 32
    torch.manual_seed(5)
    x = int_pattern(N, cin, H, W)
    gy = torch.randint(-3, 4, (N, cout, H, W)).float()
    A = torch.randint(1, 3, (N, cin)).float()
    B = torch.randint(-1, 2, (N, cin)).float()
    z = act_ref(x, A, B, 0.0)
    assert z.abs().max().item() <= 7
    ref = dw_reference(z, gy, cout)
    assert ref.abs().max().item() < 2 ** 24
    dw = wgrad_pro(ops, forced, nhwc(x), gy, cin, cout, False, A=A, B=B, n_stride=cin, slope=0.0)
    bad = (dw.double().cpu() != ref).sum().item()
    print(f"exact PRO <{cout},{cin}>: {bad} of {ref.numel()} elements differ")
    assert bad == 0
