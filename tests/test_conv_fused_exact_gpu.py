"""The six fused entry points of the halo conv kernels BIT-EXACTLY on small dyadic data, at the seams of their own code:
dei2i_conv2d_fwd_fused (statistics epilogue; operand-path normalisation PRO), dei2i_conv2d_fwd_ring, dei2i_conv2d_wgrad_oihw_pro,
dei2i_conv2d_dgrad_input_norm (FOLD + EPIN) and dei2i_conv2d_fwd_fp8 / dei2i_pack_weight_fwd_fp8 (csrc/conv_halo.hip, conv_halo16.hip,
wgrad_halo.hip, fp8.hip, conv_api.hip).  test_conv_exact_gpu.py pins the same kernels through the three plain entry points only; the
template instances and epilogues selected here are otherwise judged by the 1.5e-2 / 4e-3 .. 5e-2 / "rms error below 6 %" bounds of
test_fused_norm_gpu.py and test_fp8_gpu.py, which a few wrong pixels or channels out of 10^6 pass.

Why it is exact.  x, w, dy, the bias and the ring tensors are drawn from {-1, 0, 1} (test_conv_exact_gpu.ternary, its densities) and
the coefficients from sets that keep every intermediate on a dyadic grid:
  A in {1, 2, -1}, B in {+-0.5, +-1.5}: v = A x + B is a half-integer, never 0 (asserted), so the kink conventions of z > 0 and
      act_grad_from_out cannot matter; slope in {0, 0.25, 1}: z = max(v, 0) + slope min(v, 0) is a multiple of 1/8, |z| <= 3.5: a bf16 value;
  mean an integer, rstd in {0.5, 1, 2}, 1 + gamma in {1, 2, -1}, beta in {+-0.5, +-1.5}.  In the kind-1 (SPADE) cases x comes from
      {-2, 0, 2} and mean is even, so that xhat = (x - mean) rstd is an INTEGER and z = xhat (1 + gamma) + beta a half-integer: never 0
      (asserted) -- with ternary x and rstd = 0.5, xhat (1 + gamma) + beta would hit 0 and the kink would decide.
Every product is then exact and every fp32 partial sum is a multiple of the data's smallest step ("unit": 1, 1/2 or 1/8 per case)
whose magnitude stays below 2^24 units, hence exact in ANY order (MFMA order, the st8 / reduce_rows16 butterflies, slab sums).  The
conditions are asserted on the float64 REFERENCE of every case, nothing excluded:
  max |y| <= 256, max |dx| <= 256, fold magnitude <= 256, max |dw| < 2^24 units (the four bounds of test_conv_exact_gpu.py), the
      fp32 value of every output exact (K max|z| max|w| < 2^24 units);
  every per-image, per-channel sum of MAGNITUDES that enters a statistics or partial record < 2^24 units: sum |y|, sum y^2 (unit^2),
      sum |g|, sum |g xhat|, sum |dxhat|, sum |dxhat xhat| -- the per-image total of non-negative terms bounds every partial sum
      inside any tile, in any order.
An output that is a half- or eighth-integer above 128 / 32 is no bf16 value: the kernel's exact fp32 value is then rounded ONCE, and so
is the reference (float64 -> fp32 exactly -> bf16 to nearest even); the stored values stay multiples of the unit, so their sums stay
exact.  The project's real slope 0.2 is not exact: one LeakyReLU case checks y bit for bit against max(v, 0) + 0.2f min(v, 0) rounded
once and its statistics against the float64 sums of the stored values within n 2^-24 sum |term| (n = pixels per image: the worst
case of an fp32 sum of n terms in any order, one more rounding for a product that is not fused) -- derived, not tuned.

Harness: the C entry points on the caller's tensors; every output (y, dx, dw, the statistics / partial records, the slab scratch) is
NaN-filled before the call and carved from a larger allocation with sentinel guard rows (test_conv_exact_gpu.guarded), so a record or
pixel that is never written fails the comparison instead of showing the previous result the allocator hands back.  Comparison:
torch.equal on the whole tensor (padded channels exactly 0); statistics and partial records are summed over the chunks of each image
in float64 and compared with == against the reference's per-image sums -- the consumers (dei2i_bn_finalize_train, dei2i_in_finalize,
dei2i_bn_bwd_apply, dei2i_spade_bwd_apply) sum the chunks, so per-image totals are the contract, not the record order.  Each case
names the kernel family it is about and asserts it through dei2i_launch_counts; batch sizes come from the gates' own expressions
(n_halo16 / n_halo8) and the device's CU count, so each is the smallest batch its gate admits (112 .. 224 images of 8 x 32 or
16 x 32 pixels on 256 CUs).

Reference: float64 on the CPU.  z is built first (affine + activation, nearest upsample, then the 2-pixel frame replaced by ring
values drawn INDEPENDENTLY of x, laid out in the order geom.h documents: rows 0, 1 | rows H-2, H-1 | for rows 2 .. H-3 the columns
0, 1, W-2, W-1), then padded (F.pad reflect, or zeros: a zero-padded border stays 0, it is NOT act(B)), then F.conv2d; gradients from
F.conv_transpose2d / torch.autograd.grad.  The reflected halo of a ring pixel is therefore the ring's value too.

test_reference_conditions builds the reference of EVERY case for 256 CUs without a GPU and asserts the conditions above, so a seed or
density that breaks exactness fails before any GPU time is spent.  It is the only test of the file that is not marked ``gpu``; a
module-level ``pytestmark`` would mark it too and it would be skipped exactly where it is meant to run, so the marks are per test.
The maxima it prints (pytest -s), largest over the cases at 256 CUs: max |y| 165 (b-bn-zero; bound 256), max |dx| = fold magnitude
72 (the 32x64 and 48x96 dgrads), max |dw| 718 units with sum |dy z| 4 043 units (d-t2-coef; bound 2^24), sum |y| 40 819 units and
sum y^2 6 707 840 units^2 (b-stats-pro, unit 1/2; the integer cases stay below 29 064 / 638 820), kind-2 sum |g| 43 266 and
sum |g xhat| 173 960 units (e-k2-48x96), kind-1 sum |dxhat| 82 638, sum |dxhat xhat| 336 404, interior sum |g xhat| 152 920 and
sum |g| 37 934 (e-k1-48x96) -- all below 2^24 = 16 777 216.  a-leaky: its statistics sit at 0.006 of their bound.

Sensitivity (scratch builds, one line each, not committed): the PRO transform also run for htab[pix] == -1 -> b-bn-zero and
b-ring-zero fail; the inm2 factor of ep[2] dropped -> all five kind-1 cases (e-k1-*) fail; dq multiplied after the bias add -> all
four fp8 convolution cases (f-*) fail.  Four more of the same kind in conv_halo16.hip: the ring pixel of the neighbouring slot
(ring_index(y, x ^ 1)) -> the four c-ring-* cases; the statistics record of the second N tile not written -> a-co136 and
a-co72-two-phase; the interior mask one pixel column too wide -> the five e-k1-* cases; the coefficient row of the neighbouring
group -> e-k2-groups and e-k2-groups-relu.  Every other case passes under each.

Wall time of the file on an MI355X box with 16 CPU threads: 32 s for its 100 tests (56 on the GPU, 44 reference conditions), most
of it the float64 references on the CPU; no test takes more than 1.2 s."""
import zlib
from ctypes import byref, c_void_p

import pytest
import torch
import torch.nn.functional as F

from test_conv_exact_gpu import (BAD_ARG, DEV, _counts, act_ref, cdiv, guarded, guards_intact, n_halo16, n_halo8, nhwc, ops,  # noqa: F401
                                 ternary, where_report)

gpu = pytest.mark.gpu
from de_i2i_gan_amd._lib import ERR_WORKSPACE as WORKSPACE
LIMIT = float(2 ** 24)


def choice(gen, shape, values):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=gen)]


def seed_of(cid):
    return zlib.crc32(cid.encode())          # stable under added or reordered cases


# ---- building blocks of the references -------------------------------------------------------------------------------------------
def affine_act(x, A, B, slope):
    """z = max(v, 0) + slope min(v, 0), v = A x + B with A, B (rows, C), rows = 1 (one set for the batch) or N (one per image)"""
    v = A[:, :, None, None] * x + B[:, :, None, None]
    assert bool((v != 0).all()), "v = A x + B hits the kink"
    return v.clamp_min(0) + slope * v.clamp_max(0)


def frame_mask(hl, wl):
    iy = (torch.arange(hl) >= 2) & (torch.arange(hl) < hl - 2)
    ix = (torch.arange(wl) >= 2) & (torch.arange(wl) < wl - 2)
    return ~(iy[:, None] & ix[None, :])


def ring_layout(zl):
    """the ring tensor (N, ring_pixels, C) of the logical image zl (N, C, Hl, Wl) in the order of geom.h"""
    n, c, hl, wl = zl.shape
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(n, -1, c)      # noqa: E731
    side = zl[:, :, 2:hl - 2][:, :, :, [0, 1, wl - 2, wl - 1]]
    return torch.cat([rows(zl[:, :, 0:2]), rows(zl[:, :, hl - 2:hl]), rows(side)], dim=1)


def logical_z(gen, case, x, A, B):
    """(zl: the conv's logical input in float64, ring tensor or None) of a forward / wgrad case"""
    pro = case.get("pro")
    z = affine_act(x, A, B, pro["slope"]) if pro and pro.get("coef", True) else x
    zl = F.interpolate(z, scale_factor=2, mode="nearest") if case["up"] else z
    ring = None
    if case.get("ring"):
        r = ternary(gen, tuple(zl.shape), 0.5)                  # independent of x: NOT what the affine gives there
        zl = torch.where(frame_mask(*zl.shape[-2:]), r, zl)
        ring = ring_layout(zl)
        assert ring.shape[1] == 4 * zl.shape[-1] + 4 * (zl.shape[-2] - 4)
    return zl, ring


def conv_ref(zl, w, b, case):
    k, s, p = case.get("k", 3), case.get("s", 1), 1
    if case["reflect"]:
        return F.conv2d(F.pad(zl, (p, p, p, p), mode="reflect"), w, b, stride=s)
    return F.conv2d(zl, w, b, stride=s, padding=p)


def unit_of(case):
    pro = case.get("pro")
    if not pro or not pro.get("coef", True):
        return 1.0
    return 0.125 if pro["slope"] == 0.25 else 0.5


def draw_pro(gen, case, n, cin):
    pro = case.get("pro")
    if not pro or not pro.get("coef", True):
        return None, None
    rows = n if pro["form"] == "spade" else 1
    A = choice(gen, (rows, cin), [1.0, 2.0, -1.0])
    B = choice(gen, (rows, cin), [0.5, -0.5, 1.5, -1.5])
    if rows > 1:
        assert not torch.equal(A[0], A[1]) and not torch.equal(B[0], B[1])      # a wrong img * n_stride must show
    return A, B


# ---- A .. C, F: forward cases ----------------------------------------------------------------------------------------------------
# H, W: physical input (before the fused upsample).  pro: {form: "bn" (n_stride = 0) | "spade" (n_stride = CinS, per-image rows), slope}
# (dei2i_conv2d_fwd_fused / _fwd_ring ask the 8 x 32 kernel's gate first, 64-channel slices, before they try the 16 x 32 kernel: Cin % 64 == 0)
# ring: the 2-pixel frame of the logical image comes from a ring tensor.  entry: fused | ring | fp8.  dw: weight density (default 7/8).
H16, H16S2, H8, FP8 = "halo16_conv", "halo16_s2", "halo_conv", "halo_conv_fp8"


def fwd(cid, seam, cin, cout, H, W, N, must, reflect=True, up=False, bias=False, act="none", stats=True, entry="fused", **ex):
    return dict(id=cid, seam=seam, cin=cin, cout=cout, H=H, W=W, N=N, must=must, reflect=reflect, up=up, bias=bias, act=act, stats=stats,
                entry=entry, kind="fwd", **ex)


BN0, BN1, BNQ, SP = ({"form": "bn", "slope": 0.0}, {"form": "bn", "slope": 1.0}, {"form": "bn", "slope": 0.25}, {"form": "spade", "slope": 0.0})
FORWARD = [
    # ---- A. statistics epilogue (pro = NULL) ----
    fwd("a-one-tile", "16x32 kernel, one tile per image: two records per tile, one per 8-row half", 64, 128, 16, 32, n_halo16(1, 128), H16),
    fwd("a-co136", "16x32 kernel, CoutS = 136: ragged second N tile, the n0 + c < ldc guard of the records", 64, 136, 16, 32, n_halo16(1, 136), H16),
    fwd("a-co72-two-phase", "16x32 kernel, the 64-channel two-phase instance (CoutS = 72: two N tiles)", 64, 72, 16, 32, n_halo16(1, 72), H16),
    fwd("a-up", "16x32 kernel with the fused upsample, source 8x16", 64, 64, 8, 16, n_halo16(1, 64), H16, up=True),
    fwd("a-bias-relu", "16x32 kernel, bias + ReLU: statistics of the post-activation stored values, zero padding", 64, 128, 16, 32,
        n_halo16(1, 128), H16, reflect=False, bias=True, act="relu"),
    fwd("a-s2-reflect", "stride-2 4x4 form, reflect padding", 64, 128, 32, 64, n_halo16(1, 128), H16S2, k=4, s=2),
    fwd("a-s2-zero", "stride-2 4x4 form, zero padding + bias", 64, 128, 32, 64, n_halo16(1, 128), H16S2, k=4, s=2, reflect=False, bias=True),
    fwd("a-h8", "8x32 kernel where the 16-row one refuses: H = 8, one record per tile", 64, 128, 8, 32, n_halo8(1, 128), H8),
    fwd("a-h24-bn64", "8x32 kernel, H = 24 (three tile rows) on the BN = 64 instance, CoutS = 72: ragged second N tile", 128, 72, 24, 32,
        n_halo8(3, 72), H8),
    fwd("a-leaky", "LeakyReLU 0.2: y rounded once, statistics within the fp32 summation bound", 64, 128, 16, 32, n_halo16(1, 128), H16,
        act="leaky_relu"),
    # ---- B. operand-path normalisation (8x32 kernel, halo_conv_kernel<BN, false, PRO = true>) ----
    fwd("b-bn-reflect", "BatchNorm form (n_stride = 0), reflect padding, slope 0", 64, 128, 8, 32, n_halo8(1, 128), H8, stats=False, pro=BN0),
    fwd("b-bn-zero", "zero padding with B != 0 in every channel and slope 1: a border pixel that becomes act(B) = B instead of 0 fails",
        64, 128, 8, 32, n_halo8(1, 128), H8, stats=False, pro=BN1, reflect=False),
    fwd("b-bn-slope-quarter", "slope 0.25: the negative branch, z a multiple of 1/8; two tile rows", 64, 128, 16, 32, n_halo8(2, 128), H8,
        stats=False, pro=BNQ),
    fwd("b-spade-slices3", "SPADE form (per-image coefficients), three 64-channel slices: the halo double buffer ends on an odd slice",
        192, 64, 8, 32, n_halo8(1, 64), H8, stats=False, pro=SP, dw=0.5),
    fwd("b-spade-cins512", "CinS = 512: the gate's limit, eight slices", 512, 64, 8, 32, n_halo8(1, 64), H8, stats=False, pro=SP, dw=0.25),
    fwd("b-ring", "ring tensor, up = 0, two tile rows: rows 0, 1, H-2, H-1 and the side columns from ring_index", 64, 128, 16, 32,
        n_halo8(2, 128), H8, stats=False, pro=SP, ring=True),
    fwd("b-ring-up", "ring tensor with the fused upsample, source 4x16", 64, 128, 4, 16, n_halo8(1, 128), H8, stats=False, pro=SP, ring=True, up=True),
    fwd("b-ring-zero", "ring tensor with zero padding: padding stays 0, frame pixels stay as given", 64, 64, 8, 32, n_halo8(1, 64), H8,
        stats=False, pro=BN1, ring=True, reflect=False),
    fwd("b-stats-pro", "pro together with stats in one call", 64, 128, 8, 32, n_halo8(1, 128), H8, pro=BN0),
    # ---- C. fwd_ring (16x32 kernel with a ring tensor and the fused upsample; each also without statistics) ----
    fwd("c-ring-8x16", "z_src at source size 8x16: one tile per image", 64, 128, 8, 16, n_halo16(1, 128), H16, entry="ring", up=True, ring=True),
    fwd("c-ring-16x32", "z_src 16x32: two tile rows and columns, the 64-channel instance", 64, 64, 16, 32, n_halo16(4, 64), H16, entry="ring",
        up=True, ring=True),
    # ---- F. fp8 (halo_conv_kernel<BN, FP8 = true>): amax = 224, act_scale = 1 -> packed weights 2 w, dequant 0.5 ----
    fwd("f-one-slice", "one 128-channel slice, H = 8, bias: dequant must not touch the bias", 128, 128, 8, 32, n_halo8(1, 128), FP8,
        entry="fp8", stats=False, bias=True),
    fwd("f-up-cins256", "CinS = 256 with the fused upsample", 256, 128, 4, 16, n_halo8(1, 128), FP8, entry="fp8", stats=False, bias=True, up=True),
    fwd("f-bn64-leaky", "CoutS = 64 (the BN = 64 instance), bias + LeakyReLU rounded once", 128, 64, 8, 32, n_halo8(1, 64), FP8, entry="fp8",
        stats=False, bias=True, act="leaky_relu"),
    fwd("f-co192-zero", "Cout = 192: second N tile ragged, zero padding", 128, 192, 8, 32, n_halo8(1, 192), FP8, entry="fp8", stats=False,
        bias=True, reflect=False),
]


def forward_reference(case, cu):
    """float64 reference of a forward case: inputs, the stored bf16 output (NHWC) and the per-image sums of the stored values"""
    gen = torch.Generator().manual_seed(seed_of(case["id"]))
    cin, cout, H, W, k = case["cin"], case["cout"], case["H"], case["W"], case.get("k", 3)
    N = case["N"](cu)
    assert cin % 8 == 0
    unit = unit_of(case)
    x = ternary(gen, (N, cin, H, W), min(0.5, 576.0 / (cin * k * k)))
    A, B = draw_pro(gen, case, N, cin)
    zl, ring = logical_z(gen, case, x, A, B)
    w = ternary(gen, (cout, cin, k, k), case.get("dw", 7.0 / 8.0))
    b = ternary(gen, (cout,), 1.0) if case["bias"] else None
    pre = conv_ref(zl, w, b, case)
    couts = cdiv(cout, 8) * 8
    # the conditions for bit-exactness, on the reference, no element excluded
    m = {"max_y": pre.abs().max().item()}                                                # (in data units, not in `unit`)
    assert m["max_y"] <= 256, ("max |y|", m["max_y"])
    assert cin * k * k * zl.abs().max().item() / unit + 1 < LIMIT                         # every fp32 accumulator value is exact
    assert torch.equal(pre / unit, (pre / unit).round()) and torch.equal(pre.float().double(), pre)
    y_st = act_ref(pre, case["act"], torch.bfloat16)                                     # rounded once; NCHW
    ys = y_st.double()
    s0, s1 = ys.sum(dim=(2, 3)), (ys * ys).sum(dim=(2, 3))
    sum_abs, sum_sq = ys.abs().sum(dim=(2, 3)), s1
    if case["stats"] and case["act"] != "leaky_relu":
        assert torch.equal(ys / unit, (ys / unit).round())                               # stored values stay on the grid
        m["sum_abs_y"], m["sum_y2"] = sum_abs.max().item() / unit, sum_sq.max().item() / unit ** 2
        assert m["sum_abs_y"] < LIMIT and m["sum_y2"] < LIMIT, m
    stats_ref = torch.zeros(N, 2, couts, dtype=torch.float64)
    stats_ref[:, 0, :cout], stats_ref[:, 1, :cout] = s0, s1
    # a-leaky: |fp32 sum in any order - exact sum| <= (n - 1) u sum |term|; the squares one more rounding each when not fused
    npix = pre.shape[-2] * pre.shape[-1]
    stats_tol = torch.zeros_like(stats_ref)
    stats_tol[:, 0, :cout], stats_tol[:, 1, :cout] = npix * 2.0 ** -24 * sum_abs, npix * 2.0 ** -24 * sum_sq
    return dict(N=N, x=x, A=A, B=B, ring=ring, w=w, b=b, y=nhwc(y_st, couts, torch.bfloat16), stats=stats_ref, stats_tol=stats_tol,
                unit=unit, maxima=m, out_hw=tuple(pre.shape[-2:]))


def pro_desc(L, case, cins, A, B, ring):
    """(struct dei2i_pro, the device tensors it points to)"""
    pro = case.get("pro") or {}
    keep = [t.float().to(DEV) if t is not None else None for t in (A, B)]
    keep.append(ring.to(torch.bfloat16).to(DEV) if ring is not None else None)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    n_stride = cins if pro.get("form") == "spade" else 0
    return L.ProDesc(ptr(keep[0]), ptr(keep[1]), n_stride, float(pro.get("slope", 0.0)), ptr(keep[2])), keep


def run_forward(ops, case, with_stats):
    from de_i2i_gan_amd import _lib as L
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    r = forward_reference(case, cu)
    N, cin, cout, k = r["N"], case["cin"], case["cout"], case.get("k", 3)
    cins, couts = cin, cdiv(cout, 8) * 8
    geom = ops.ConvGeom(cin, cout, k, case.get("s", 1), 1, case["reflect"], case["up"])
    d = ops._desc(ops.BF16, geom, N, case["H"], case["W"], cins, couts)
    bd = r["b"].float().to(DEV) if r["b"] is not None else None
    wd = r["w"].float().to(DEV)
    lib = ops._lib_for(wd)
    st = ops._stream()
    ho, wo = r["out_hw"]
    ybuf, y, yg = guarded((N, ho, wo, couts), torch.bfloat16)
    chunks = lib.dei2i_conv2d_stats_chunks(byref(d))
    assert chunks == (ho // 8) * (wo // 32)
    sbuf, stats, sg = guarded((N, chunks, 2, couts), torch.float32)
    sp = ops._p(stats) if with_stats else None
    act = ops.ACT[case["act"]]
    if case["entry"] == "fp8":
        xd = nhwc(r["x"], cins, torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
        wq = torch.full((cout * 9 * cins,), 0x7F, dtype=torch.uint8, device=DEV)           # 0x7f: e4m3 NaN
        dq = torch.full((1,), float("nan"), device=DEV)
        amax = torch.full((1,), 224.0, device=DEV)
        L.check(lib.dei2i_pack_weight_fwd_fp8(byref(d), ops._p(wd), ops._p(amax), 1.0, ops._p(wq), ops._p(dq), st), "pack_weight_fwd_fp8")
        torch.cuda.synchronize()
        assert dq.item() == 0.5
        assert torch.equal(wq.view(torch.float8_e4m3fn).float().cpu().view(cout, 9, cins),
                           2 * r["w"].permute(0, 2, 3, 1).reshape(cout, 9, cin).float())
        assert lib.dei2i_conv2d_fp8_supported(byref(d)) == 1
        _counts()
        rc = lib.dei2i_conv2d_fwd_fp8(byref(d), ops._p(xd), ops._p(wq), ops._p(bd), ops._p(dq), act, ops._p(y), st)
    else:
        xd = nhwc(r["x"], cins, torch.bfloat16).to(DEV)
        wf, _ = ops.PackedWeights().get(wd, (wd,), ops.BF16, geom, cins, couts, need_dgrad=False)
        torch.cuda.synchronize()
        _counts()
        if case["entry"] == "ring":
            ringd = r["ring"].to(torch.bfloat16).to(DEV)
            assert lib.dei2i_conv2d_ring_supported(byref(d)) == 1
            rc = lib.dei2i_conv2d_fwd_ring(byref(d), ops._p(xd), ops._p(ringd), ops._p(wf), ops._p(bd), act, ops._p(y), sp, st)
        else:
            pd, keep = pro_desc(L, case, cins, r["A"], r["B"], r["ring"])
            has_pro = case.get("pro") is not None
            assert lib.dei2i_conv2d_fused_supported(byref(d), int(has_pro)) == 1
            rc = lib.dei2i_conv2d_fwd_fused(byref(d), ops._p(xd), ops._p(wf), ops._p(bd), act, ops._p(y), byref(pd) if has_pro else None, sp, st)
    torch.cuda.synchronize()
    fam = _counts()
    assert rc == 0, (case["id"], rc)
    fails = []
    got = y.cpu()
    if not torch.equal(got, r["y"]):
        fails.append("y: " + where_report(got, r["y"], band=2 if case.get("ring") else 1))
    sgot = stats.double().sum(dim=1).cpu()
    if not with_stats:
        if not bool(torch.isnan(stats).all().item()):
            fails.append("statistics were written without a stats pointer")
    elif case["act"] == "leaky_relu":
        err = (sgot - r["stats"]).abs()
        print(f"{case['id']}: statistics error / bound, max over records: {(err / r['stats_tol'].clamp_min(1e-300)).max().item():.3f}")
        if not bool((err <= r["stats_tol"]).all().item()):                 # (a NaN record fails: NaN <= tol is False)
            fails.append(f"statistics beyond the fp32 summation bound: {int((~(err <= r['stats_tol'])).sum())} sums")
    elif not torch.equal(sgot, r["stats"]):
        bad = ((sgot != r["stats"]) | torch.isnan(sgot)).nonzero()
        fails.append(f"statistics: {len(bad)} of {sgot.numel()} per-image sums differ ({int(torch.isnan(sgot).sum())} NaN); first (n, q, c): "
                     + "; ".join(f"{tuple(i)}: got {sgot[tuple(i)].item()} want {r['stats'][tuple(i)].item()}" for i in bad[:8].tolist()))
    for nm, (buf, g) in {"y": (ybuf, yg), "statistics": (sbuf, sg)}.items():
        if not guards_intact(buf, g):
            fails.append(f"the guard rows of {nm} were written")
    assert not fails, f"{case['id']} ({case['seam']}):\n" + "\n".join(fails)
    assert fam == {case["must"]: 1}, f"{case['id']}: the case is listed for {case['must']} but ran {fam}"


@gpu
@pytest.mark.parametrize("case", [c for c in FORWARD if c["id"][0] == "a"], ids=lambda c: c["id"])
def test_statistics_epilogue_exact(ops, case):
    """A. dei2i_conv2d_fwd_fused(..., stats): st8 / reduce_rows16 of conv_halo16.hip (3x3 and stride-2 forms) and the st8 block of conv_halo.hip"""
    run_forward(ops, case, True)


@gpu
@pytest.mark.parametrize("case", [c for c in FORWARD if c["id"][0] == "b"], ids=lambda c: c["id"])
def test_operand_path_normalisation_exact(ops, case):
    """B. dei2i_conv2d_fwd_fused(..., pro): the coefficient table, the in-place transform of the landed halo, htab's three kinds of pixel"""
    run_forward(ops, case, case["stats"])


@gpu
@pytest.mark.parametrize("with_stats", [True, False], ids=["stats", "no-stats"])
@pytest.mark.parametrize("case", [c for c in FORWARD if c["id"][0] == "c"], ids=lambda c: c["id"])
def test_fwd_ring_exact(ops, case, with_stats):
    """C. dei2i_conv2d_fwd_ring: halo16_conv with a ring tensor and the fused x2 upsample"""
    run_forward(ops, case, with_stats)


@gpu
@pytest.mark.parametrize("case", [c for c in FORWARD if c["id"][0] == "f"], ids=lambda c: c["id"])
def test_fp8_forward_exact(ops, case):
    """F. dei2i_conv2d_fwd_fp8: ternary e4m3 bytes, packed weights 2 w, dequant 0.5, ternary bias: y == conv + bias fails if the dequant
    factor is skipped or applied to the bias, or if the byte-pair k-permutation of the two operands disagrees"""
    run_forward(ops, case, False)


@gpu
def test_fp8_weight_pack_bytes_and_dequant(ops):
    """F. dei2i_pack_weight_fwd_fp8: bytes == (w s).clamp(+-448) -> float8_e4m3fn laid out [Cout][tap][CinS], padded input channels
    byte 0; 448 / amax = 128 is a power of two and one element of magnitude amax is planted, so the scale has no rounding of its own.
    Magnitudes span the normal and the subnormal range of e4m3 down to its smallest subnormal (none rounds to a signed zero)."""
    from de_i2i_gan_amd import _lib as L
    gen = torch.Generator().manual_seed(41)
    cin, cins, cout, amax, act_scale = 120, 128, 72, 3.5, 16.0
    s = 448.0 / amax
    mag = (torch.randn(cout, cin, 3, 3, generator=gen).abs() * 10.0 ** (-4 * torch.rand(cout, cin, 3, 3, generator=gen))).clamp(2.0 ** -9 / s, amax)
    w = mag * (torch.randint(0, 2, mag.shape, generator=gen) * 2 - 1)
    w[0, 0, 0, 0], w[1, 2, 1, 1], w[3, 5, 2, 0] = amax, -amax, 0.0
    d = ops._desc(ops.BF16, ops.ConvGeom(cin, cout, 3, 1, 1, True, False), 4, 8, 32, cins, cout)
    wd, am = w.to(DEV), torch.full((1,), amax, device=DEV)
    lib = ops._lib_for(wd)
    pad = 256                                                                   # guard bytes (guarded() is for float types)
    qbuf = torch.full((cout * 9 * cins + 2 * pad,), 0x7F, dtype=torch.uint8, device=DEV)      # 0x7f: e4m3 NaN
    wq = qbuf[pad:-pad].view(cout, 9, cins)
    dbuf, dq, dg = guarded((1,), torch.float32)
    L.check(lib.dei2i_pack_weight_fwd_fp8(byref(d), ops._p(wd), ops._p(am), act_scale, ops._p(wq), ops._p(dq), ops._stream()), "pack_weight_fwd_fp8")
    torch.cuda.synchronize()
    ref = torch.zeros(cout, 9, cins, dtype=torch.uint8)
    ref[:, :, :cin] = (w * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).permute(0, 2, 3, 1).reshape(cout, 9, cin)
    assert int((ref[:, :, :cin] & 0x7F == 0).sum()) == 1          # the planted zero only
    got = wq.cpu()
    assert torch.equal(got, ref), where_report(got, ref)
    assert dq.item() == 1.0 / (act_scale * s) == 2.0 ** -11
    assert bool((qbuf[:pad] == 0x7F).all().item()) and bool((qbuf[-pad:] == 0x7F).all().item()) and guards_intact(dbuf, dg)


# ---- D. wgrad_oihw_pro ------------------------------------------------------------------------------------------------------------
# one case per wgrad_halo tile of wgrad_halo_shape_ok x three forms.  12 x 32 images, N = 3: nine 4 x 32 half-tiles in two pixel
# splits of 5 and 4, so a split crosses an image boundary (the per-image coefficients are re-read) and two slabs are summed.
def wg(cid, seam, cin, cout, form, **ex):
    pro = {"coef": False} if form == "ring" else {**SP, "slope": ex.pop("slope", 0.0)}
    up = form == "ring"
    return dict(id=cid, seam=seam, cin=cin, cout=cout, H=6 if up else 12, W=16 if up else 32, N=lambda cu: 3, up=up, reflect=ex.pop("reflect", True),
                pro=pro, ring=form != "coef", kind="wgrad", **ex)


WGRAD = [
    wg("d-t1-coef", "tile 1 (64 co x 128 ci): coefficients only; accumulate = 1", 128, 64, "coef", acc=True),
    wg("d-t1-coef-ring", "tile 1: coefficients + ring", 128, 56, "coef+ring"),
    wg("d-t1-ring", "tile 1: ring only (A = B = NULL, x = z_src, up = 1)", 128, 48, "ring"),
    wg("d-t2-coef", "tile 2 (64 x 64, taps split over two wave groups): coefficients only, zero padding, slope 0.25", 64, 32, "coef", reflect=False, slope=0.25),
    wg("d-t2-coef-ring", "tile 2: coefficients + ring", 64, 24, "coef+ring"),
    wg("d-t2-ring", "tile 2: ring only", 64, 8, "ring"),
    wg("d-t3-coef", "tile 3 (128 co x 64 ci): coefficients only, two ci slices", 128, 96, "coef"),
    wg("d-t3-coef-ring", "tile 3: coefficients + ring, Cout = 136: ragged second co tile", 64, 136, "coef+ring"),
    wg("d-t3-ring", "tile 3: ring only", 64, 128, "ring"),
]


def wgrad_reference(case, cu):
    gen = torch.Generator().manual_seed(seed_of(case["id"]))
    cin, cout, N = case["cin"], case["cout"], case["N"](cu)
    unit = unit_of(case)
    x = ternary(gen, (N, cin, case["H"], case["W"]), 0.5)
    A, B = draw_pro(gen, case, N, cin)
    zl, ring = logical_z(gen, case, x, A, B)
    dy = ternary(gen, (N, cout) + tuple(zl.shape[-2:]), 0.25)
    w0 = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (dw,) = torch.autograd.grad(conv_ref(zl, w0, None, case), [w0], dy)
    (dw_abs,) = torch.autograd.grad(conv_ref(zl.abs(), w0, None, case), [w0], dy.abs())      # sum of |dy z| per weight
    m = {"max_dw": dw.abs().max().item() / unit, "max_sum_abs_dw": dw_abs.max().item() / unit}
    assert m["max_dw"] <= m["max_sum_abs_dw"] < LIMIT, m
    return dict(N=N, x=x, A=A, B=B, ring=ring, dy=dy, dw=dw.float(), unit=unit, maxima=m)


@gpu
@pytest.mark.parametrize("case", WGRAD, ids=lambda c: c["id"])
def test_wgrad_pro_exact(ops, case):
    """D. dei2i_conv2d_wgrad_oihw_pro: dw = sum dy z over the three wgrad_halo tiles with a ConvPro; the last element short of one
    slab returns DEI2I_ERR_WORKSPACE and writes nothing"""
    from de_i2i_gan_amd import _lib as L
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    r = wgrad_reference(case, cu)
    N, cin, cout = r["N"], case["cin"], case["cout"]
    cins, couts = cin, cdiv(cout, 8) * 8
    geom = ops.ConvGeom(cin, cout, 3, 1, 1, case["reflect"], case["up"])
    d = ops._desc(ops.BF16, geom, N, case["H"], case["W"], cins, couts)
    xd, dyd = nhwc(r["x"], cins, torch.bfloat16).to(DEV), nhwc(r["dy"], couts, torch.bfloat16).to(DEV)
    lib = ops._lib_for(xd)
    st = ops._stream()
    assert lib.dei2i_conv2d_wgrad_pro_supported(byref(d)) == 1
    pd, keep = pro_desc(L, case, cins, r["A"], r["B"], r["ring"])
    packed = lib.dei2i_wgrad_slab_elems(byref(d))
    sc_elems = 4 * packed + 1
    scbuf, sc, scg = guarded((sc_elems,), torch.float32)
    dwbuf, dwo, dwg = guarded((cout, cin, 3, 3), torch.float32)
    fails = []
    torch.cuda.synchronize()
    _counts()
    rc = lib.dei2i_conv2d_wgrad_oihw_pro(byref(d), ops._p(xd), ops._p(dyd), ops._p(sc), packed - 1, c_void_p(dwo.data_ptr()), 0, byref(pd), st)
    torch.cuda.synchronize()
    assert rc == WORKSPACE and _counts() == {}, (rc, "a call without room for one slab must launch nothing")
    assert bool(torch.isnan(dwo).all().item()) and bool(torch.isnan(sc).all().item())
    rc = lib.dei2i_conv2d_wgrad_oihw_pro(byref(d), ops._p(xd), ops._p(dyd), ops._p(sc), sc_elems, c_void_p(dwo.data_ptr()), 0, byref(pd), st)
    torch.cuda.synchronize()
    fam = _counts()
    assert rc == 0, (case["id"], rc)
    got = dwo.cpu()
    if not torch.equal(got, r["dw"]):
        fails.append("dw: " + where_report(got, r["dw"]))
    if case.get("acc"):
        base = torch.randint(-3, 4, r["dw"].shape, generator=torch.Generator().manual_seed(7)).float()
        dwo.copy_(base)
        sc.fill_(float("nan"))
        rc = lib.dei2i_conv2d_wgrad_oihw_pro(byref(d), ops._p(xd), ops._p(dyd), ops._p(sc), sc_elems, c_void_p(dwo.data_ptr()), 1, byref(pd), st)
        torch.cuda.synchronize()
        _counts()
        assert rc == 0, ("accumulate", rc)
        got = dwo.cpu()
        if not torch.equal(got, r["dw"] + base):
            fails.append("dw, accumulate = 1: " + where_report(got, r["dw"] + base))
    for nm, (buf, g) in {"dw": (dwbuf, dwg), "slab scratch": (scbuf, scg)}.items():
        if not guards_intact(buf, g):
            fails.append(f"the guard rows of {nm} were written")
    assert not fails, f"{case['id']} ({case['seam']}):\n" + "\n".join(fails)
    assert fam == {"wgrad_halo": 1}, f"{case['id']}: the case is listed for wgrad_halo but ran {fam}"


# ---- E. dgrad_input_norm (FOLD + EPIN) -------------------------------------------------------------------------------------------
# 32 x 64: the smallest FOLD-eligible image (every tile owns a corner); 48 x 96: a 3 x 3 tile grid with a tile without border pixel.
# kind 2: act, group (0: one coefficient row for the batch; 2: N / 2 images per row, the rows differ); kind 1: up (x at half resolution)
def dn(cid, seam, cin, kind, H=32, W=64, **ex):
    tiles = (H // 16) * (W // 32)
    return dict(id=cid, seam=seam, cin=cin, cout=64, H=H, W=W, N=n_halo16(tiles, cin), knd=kind, kind="dgrad_norm", act=ex.pop("act", "none"),
                groups=ex.pop("groups", 0), up=ex.pop("up", False), **ex)


DGRAD_NORM = [
    dn("e-k2-none", "kind 2, act none, one coefficient row", 128, 2),
    dn("e-k2-relu", "kind 2, ReLU", 128, 2, act="relu"),
    dn("e-k2-groups", "kind 2, group_images = N / 2: per-group a / b / mean / rstd rows", 128, 2, groups=2),
    dn("e-k2-groups-relu", "kind 2, ReLU, group_images = N / 2", 128, 2, act="relu", groups=2),
    dn("e-k1-dx128", "kind 1, 128-channel dx: 25 classes, the frame's pixels use their own", 128, 1),
    dn("e-k1-dx128-up", "kind 1 with up = 1: x at half resolution", 128, 1, up=True),
    dn("e-k1-dx64", "kind 1 on the 64-channel dx tile", 64, 1),
    dn("e-k1-dx64-up", "kind 1 on the 64-channel dx tile, up = 1", 64, 1, up=True),
    dn("e-k1-48x96", "kind 1 at 48x96: 3 x 3 tiles per image, one of them without a border pixel", 128, 1, H=48, W=96),
    dn("e-k2-48x96", "kind 2 at 48x96, ReLU", 128, 2, H=48, W=96, act="relu"),
]

_dgrad_cache = {}


def dgrad_data(cin, cout, H, W, N):
    """(w, dy, dx) of the reflect 3x3 dgrad, shared by the cases with the same shape (the newest shape only is kept) and never modified"""
    key = (cin, cout, H, W, N)
    if key not in _dgrad_cache:
        _dgrad_cache.clear()
        gen = torch.Generator().manual_seed(3000 + cin + H)
        w = ternary(gen, (cout, cin, 3, 3), 7.0 / 8.0)
        dy = ternary(gen, (N, cout, H, W), min(0.25, 288.0 / (cout * 9)))
        gframe = F.conv_transpose2d(dy, w)                                      # gradient of the padded frame (N, cin, H + 2, W + 2)
        xr = torch.zeros(N, cin, H, W, dtype=torch.float64, requires_grad=True)
        frame = F.pad(xr, (1, 1, 1, 1), mode="reflect")
        (dx,) = torch.autograd.grad(frame, [xr], gframe, retain_graph=True)
        (fold_abs,) = torch.autograd.grad(frame, [xr], gframe.abs())
        assert dx.abs().max().item() <= 256 and fold_abs.max().item() <= 256 and torch.equal(dx, dx.round())
        _dgrad_cache[key] = (w, dy, dx, {"max_dx": dx.abs().max().item(), "max_fold": fold_abs.max().item()})
    return _dgrad_cache[key]


def border_class(n):
    i = torch.arange(n)
    return torch.where(i < 2, i, torch.where(i >= n - 2, 4 - (n - 1 - i), torch.full_like(i, 2)))


def dgrad_norm_reference(case, cu):
    cin, cout, H, W = case["cin"], case["cout"], case["H"], case["W"]
    N = case["N"](cu)
    w, dy, dz, m = dgrad_data(cin, cout, H, W, N)
    m = dict(m)
    gen = torch.Generator().manual_seed(seed_of(case["id"]))
    sums = lambda t: t.sum(dim=(2, 3))      # noqa: E731
    out = dict(N=N, w=w, dy=dy, dx=dz)
    if case["knd"] == 2:
        G = case["groups"] or 1
        assert N % G == 0
        y1 = ternary(gen, (N, cin, H, W), 0.5)
        a, b = choice(gen, (G, cin), [1.0, 2.0, -1.0]), choice(gen, (G, cin), [0.5, -0.5, 1.5, -1.5])
        mean, rstd = choice(gen, (G, cin), [-1.0, 0.0, 1.0]), choice(gen, (G, cin), [0.5, 1.0, 2.0])
        assert G == 1 or not (torch.equal(a[0], a[1]) or torch.equal(b[0], b[1]) or torch.equal(mean[0], mean[1]) or torch.equal(rstd[0], rstd[1]))
        row = torch.arange(N) // (N // G)                                        # image n takes row n / group_images
        per = lambda t: t[row][:, :, None, None]      # noqa: E731
        z = per(a) * y1 + per(b)
        assert bool((z != 0).all())
        g = dz * ((z > 0).double() if case["act"] == "relu" else 1.0)
        xhat = (y1 - per(mean)) * per(rstd)
        terms = [g, g * xhat]
        units = [1.0, 0.5]
        out.update(x=y1, a=a, b=b, mean=mean, rstd=rstd)
    else:
        hs, ws = (H // 2, W // 2) if case["up"] else (H, W)
        xs = 2 * ternary(gen, (N, cin, hs, ws), 0.5)
        mean, rstd = choice(gen, (N, cin), [-2.0, 0.0, 2.0]), choice(gen, (N, cin), [0.5, 1.0, 2.0])
        g1 = choice(gen, (N, 5, 5, cin), [1.0, 2.0, -1.0])
        beta = choice(gen, (N, 5, 5, cin), [0.5, -0.5, 1.5, -1.5])
        gb = torch.cat([g1 - 1.0, beta], dim=-1)                                 # the (N, 5, 5, 2C) table: gamma | beta
        flat = gb.view(N, 25, 2 * cin)
        assert all(len({tuple(r.tolist()) for r in flat[n]}) == 25 for n in range(N)), "two classes of an image coincide"
        cy, cx = border_class(H), border_class(W)
        g1p = g1[:, cy][:, :, cx].permute(0, 3, 1, 2)                            # per pixel (N, C, H, W)
        bp = beta[:, cy][:, :, cx].permute(0, 3, 1, 2)
        xu = F.interpolate(xs, scale_factor=2, mode="nearest") if case["up"] else xs
        xhat = (xu - mean[:, :, None, None]) * rstd[:, :, None, None]
        assert torch.equal(xhat, xhat.round())
        z = xhat * g1p + bp
        assert bool((z != 0).all())
        gg = dz * (z > 0).double()
        inter = ((cy == 2)[:, None] & (cx == 2)[None, :]).double()
        terms = [gg * g1p, gg * g1p * xhat, gg * xhat * inter, gg * inter]
        units = [1.0, 1.0, 1.0, 1.0]
        out.update(x=xs, mean=mean, rstd=rstd, gb=gb)
    for q, (t, u) in enumerate(zip(terms, units)):
        m[f"sum_abs_q{q}"] = sums(t.abs()).max().item() / u
        assert m[f"sum_abs_q{q}"] < LIMIT, m
    out.update(partial=torch.stack([sums(t) for t in terms], dim=1), maxima=m)       # (N, nq, C)
    return out


@gpu
@pytest.mark.parametrize("case", DGRAD_NORM, ids=lambda c: c["id"])
def test_dgrad_input_norm_exact(ops, case):
    """E. dei2i_conv2d_dgrad_input_norm: the EPIN build of the FOLD epilogue.  dx bit for bit against the reference dgrad and against
    dei2i_conv2d_dgrad_input on the same data; the kind-1 / kind-2 records summed per image == the float64 sums"""
    from de_i2i_gan_amd import _lib as L
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    r = dgrad_norm_reference(case, cu)
    N, cin, cout, H, W = r["N"], case["cin"], case["cout"], case["H"], case["W"]
    geom = ops.ConvGeom(cin, cout, 3, 1, 1, True, False)
    d = ops._desc(ops.BF16, geom, N, H, W, cin, cout)
    dyd = nhwc(r["dy"], cout, torch.bfloat16).to(DEV)
    xd = nhwc(r["x"], cin, torch.bfloat16).to(DEV)
    wd = r["w"].float().to(DEV)
    lib = ops._lib_for(wd)
    st = ops._stream()
    _, wdg = ops.PackedWeights().get(wd, (wd,), ops.BF16, geom, cin, cout, need_dgrad=True)
    assert lib.dei2i_conv2d_dgrad_norm_supported(byref(d)) == 1
    chunks = lib.dei2i_conv2d_dgrad_norm_chunks(byref(d))
    assert chunks == (H // 16) * (W // 32)
    nq = 4 if case["knd"] == 1 else 2
    dxbuf, dxo, dxg = guarded((N, H, W, cin), torch.bfloat16)
    pbuf, part, pg = guarded((N, chunks, nq, cin), torch.float32)      # kind 2: (N * chunks, 2, C), the same memory
    f32 = lambda t: t.float().contiguous().to(DEV)      # noqa: E731
    mean, rstd = f32(r["mean"]), f32(r["rstd"])
    a = b = gb = None
    if case["knd"] == 2:
        a, b = f32(r["a"]), f32(r["b"])
    else:
        gb = r["gb"].to(torch.bfloat16).contiguous().to(DEV)
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    group_images = N // case["groups"] if case["groups"] else 0
    en = L.EpiNormDesc(case["knd"], int(case["up"]), ops.ACT[case["act"]], group_images, ptr(xd), ptr(mean), ptr(rstd), ptr(gb), ptr(a), ptr(b),
                       ptr(part))
    torch.cuda.synchronize()
    _counts()
    rc = lib.dei2i_conv2d_dgrad_input_norm(byref(d), ops._p(dyd), ops._p(wdg), ops._p(dxo), byref(en), st)
    torch.cuda.synchronize()
    fam = _counts()
    assert rc == 0, (case["id"], rc)
    fails = []
    ref = nhwc(r["dx"], cin, torch.bfloat16)
    got = dxo.cpu()
    if not torch.equal(got, ref):
        fails.append("dx: " + where_report(got, ref, band=2))
    pgot = part.double().sum(dim=1).cpu()
    if not torch.equal(pgot, r["partial"]):
        bad = ((pgot != r["partial"]) | torch.isnan(pgot)).nonzero()
        fails.append(f"partial records: {len(bad)} of {pgot.numel()} per-image sums differ ({int(torch.isnan(pgot).sum())} NaN); first (n, q, c): "
                     + "; ".join(f"{tuple(i)}: got {pgot[tuple(i)].item()} want {r['partial'][tuple(i)].item()}" for i in bad[:8].tolist()))
    # the plain entry point on the same data
    ws_elems = cdiv(lib.dei2i_conv2d_workspace_bytes(byref(d)), 4)
    ws = torch.full((ws_elems,), float("nan"), device=DEV)
    ext = torch.full((N, H + 2, W + 2, cin), float("nan"), dtype=torch.bfloat16, device=DEV)
    dx2 = torch.full((N, H, W, cin), float("nan"), dtype=torch.bfloat16, device=DEV)
    rc = lib.dei2i_conv2d_dgrad_input(byref(d), ops._p(dyd), ops._p(wdg), ops._p(ext), ops._p(dx2), ops._p(ws), ws_elems * 4, st)
    torch.cuda.synchronize()
    _counts()
    assert rc == 0, ("conv2d_dgrad_input", rc)
    if not torch.equal(dx2, dxo):
        fails.append("dx differs from dei2i_conv2d_dgrad_input: " + where_report(got, dx2.cpu(), band=2))
    for nm, (buf, g) in {"dx": (dxbuf, dxg), "partial records": (pbuf, pg)}.items():
        if not guards_intact(buf, g):
            fails.append(f"the guard rows of {nm} were written")
    assert not fails, f"{case['id']} ({case['seam']}):\n" + "\n".join(fails)
    assert fam == {"halo16_conv": 1}, f"{case['id']}: the case is listed for halo16_conv but ran {fam}"


# ---- the conditions of every case, without a GPU ------------------------------------------------------------------------------------
ALL_CASES = FORWARD + WGRAD + DGRAD_NORM
REFERENCES = {"fwd": forward_reference, "wgrad": wgrad_reference, "dgrad_norm": dgrad_norm_reference}


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["id"])
def test_reference_conditions(case):
    """every case's float64 reference at the batch of 256 CUs: the conditions for bit-exactness hold (asserted inside), and the
    maxima they are judged by are printed (-s shows them; the module docstring quotes the largest)"""
    r = REFERENCES[case["kind"]](case, 256)
    print(f"{case['id']}: N = {r['N']}, unit = {r.get('unit', 1.0)}, " + ", ".join(f"{k} = {v:g}" for k, v in r["maxima"].items()))


# ---- G. refusals: DEI2I_ERR_BAD_ARG, nothing launched, every output still NaN between intact guards ---------------------------------
REFUSALS = ["fused-pro-cins576", "fused-pro-s2", "ring-up0", "ring-h-below-4", "norm-zero-padding", "norm-kind3", "norm-kind2-up",
            "norm-groups-not-dividing", "wgrad-pro-only-A"]


@gpu
@pytest.mark.parametrize("cid", REFUSALS)
def test_refusals_leave_the_outputs_untouched(ops, cid):
    from de_i2i_gan_amd import _lib as L
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    # the shape each entry point WOULD take, then the one thing that makes it refuse
    cin, cout, k, s, reflect, up, H, W = 64, 128, 3, 1, True, 0, 8, 32
    N = n_halo8(1, 128)(cu)
    if cid == "fused-pro-cins576":
        cin, cout, N = 576, 64, n_halo8(1, 64)(cu)
    elif cid == "fused-pro-s2":
        k, s, H, W, N = 4, 2, 32, 64, n_halo16(1, 128)(cu)
    elif cid == "ring-up0":
        H, W, N = 16, 32, n_halo16(1, 128)(cu)
    elif cid == "ring-h-below-4":
        up, H, W, N = 1, 1, 16, n_halo16(1, 128)(cu)
    elif cid.startswith("norm"):
        cin, cout, H, W, N = 128, 64, 32, 64, n_halo16(4, 128)(cu)
        reflect = cid != "norm-zero-padding"
    elif cid == "wgrad-pro-only-A":
        N = 3
    d = L.ConvDesc(L.BF16, N, H, W, cin, cout, cin, cout, k, k, s, 1, L.PAD_REFLECT if reflect else L.PAD_ZERO, up)
    big = N * ((H << up) + 2) * ((W << up) + 2) * max(cin, cout) + cout * k * k * cin
    src = torch.zeros(big, dtype=torch.bfloat16, device=DEV)                  # stands for x / dy / the packed weights / the ring: never read
    coef = torch.ones(max(N, 25) * 2 * cin, device=DEV)                       # stands for A / B / mean / rstd / a / b / gb
    lib = ops._lib_for(src)
    obuf, out, og = guarded((big,), torch.float32 if cid.startswith("wgrad") else torch.bfloat16)
    rbuf, rec, rg = guarded((N * 64 * 4 * max(cin, cout),), torch.float32)    # statistics / partial records / slab scratch
    st = ops._stream()
    torch.cuda.synchronize()
    _counts()
    if cid.startswith("fused"):
        pd = L.ProDesc(coef.data_ptr(), coef.data_ptr(), 0, 0.0, None)
        assert cid != "fused-pro-s2" or lib.dei2i_conv2d_fused_supported(byref(d), 0) == 1      # without pro the stride-2 form takes it
        rc = lib.dei2i_conv2d_fwd_fused(byref(d), ops._p(src), ops._p(src), None, 0, ops._p(out), byref(pd), ops._p(rec), st)
    elif cid.startswith("ring"):
        rc = lib.dei2i_conv2d_fwd_ring(byref(d), ops._p(src), ops._p(src), ops._p(src), None, 0, ops._p(out), ops._p(rec), st)
    elif cid.startswith("norm"):
        kind = {"norm-kind3": 3, "norm-zero-padding": 2, "norm-kind2-up": 2, "norm-groups-not-dividing": 2}[cid]
        groups = N - 1 if cid == "norm-groups-not-dividing" else 0
        assert groups == 0 or N % groups != 0
        en = L.EpiNormDesc(kind, 1 if cid == "norm-kind2-up" else 0, 0, groups, src.data_ptr(), coef.data_ptr(), coef.data_ptr(), src.data_ptr(),
                           coef.data_ptr(), coef.data_ptr(), rec.data_ptr())
        if cid != "norm-zero-padding":      # the same call is taken once the one thing is put right: the refusal is about that thing
            ok = L.ConvDesc(L.BF16, N, H, W, cin, cout, cin, cout, k, k, s, 1, L.PAD_REFLECT, 0)
            assert lib.dei2i_conv2d_dgrad_norm_supported(byref(ok)) == 1
        rc = lib.dei2i_conv2d_dgrad_input_norm(byref(d), ops._p(src), ops._p(src), ops._p(out), byref(en), st)
    else:
        assert lib.dei2i_conv2d_wgrad_pro_supported(byref(d)) == 1
        pd = L.ProDesc(coef.data_ptr(), None, 0, 0.0, src.data_ptr())
        rc = lib.dei2i_conv2d_wgrad_oihw_pro(byref(d), ops._p(src), ops._p(src), ops._p(rec), rec.numel(), c_void_p(out.data_ptr()), 0, byref(pd), st)
    torch.cuda.synchronize()
    assert rc == BAD_ARG, (cid, rc)
    assert _counts() == {}, "a refused call launched a kernel"
    assert bool(torch.isnan(out.float()).all().item()) and bool(torch.isnan(rec).all().item())
    assert guards_intact(obuf, og) and guards_intact(rbuf, rg)
