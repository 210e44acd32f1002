"""The convolution kernels (csrc/conv_gemm.hip, conv_gemm_v2.hip, conv_halo.hip, conv_halo16.hip, thin_conv.hip, wgrad_v2.hip,
wgrad_thin.hip and the fold / split-K host code of conv_api.hip) BIT-EXACTLY on integer data, at the seams of their dispatch.

Why integers: with x, w, dy and the bias drawn from {-1, 0, 1} every bf16 product is exact, every fp32 partial sum is an integer
below 2^24 and therefore exact in ANY order (MFMA order, split-K slabs, slab reduces, the read-add-store of fold_border_kernel), and
an output of magnitude <= 256 is an exactly representable bf16 value.  So the kernel must equal a float64 reference bit for bit: one
dropped, doubled or mis-addressed product fails the case, where the tolerances of test_ops_gpu.py / test_hot_shapes_gpu.py (1.5e-2 of
the tensor's maximum) let it pass.  The conditions that make this hold are asserted on the REFERENCE of every case and nothing is
masked: max |y| <= 256, max |dx| <= 256, max |dw| < 2^24 -- and, because the reflect / upsample input gradients are folded from a
bf16 frame (fold_pad_kernel, fold_border_kernel, the FOLD epilogue of conv_halo16.hip), also the sum of the MAGNITUDES of the frame
elements that fold onto one pixel <= 256, which bounds every partial sum of every fold order.

Harness (run_case): the C entry points dei2i_conv2d_fwd / dei2i_conv2d_dgrad_input / dei2i_conv2d_wgrad_oihw on the caller's
tensors, with the packed weights of ops.PackedWeights.get (dei2i_pack_weight_both) and the descriptor of ops._desc.  Every output
(y, dx, dw with accumulate = 0, the dgrad frame scratch, the split-K / slab workspace) is filled with NaN before the call -- ops.conv2d
takes them from the caching allocator, where a region a kernel never writes can hold the previous, correct result of the same shape
-- and is carved from a larger allocation with one guard row of a sentinel before and after it.  Comparison: torch.equal on the whole
NHWC tensor (padded channels exactly 0; dw as fp32); a mismatch prints its count, the first indices and whether each lies in a
corner, on a border or in the interior.

Which kernel ran: FAMILIES pins dei2i_launch_counts per case and phase, recorded from a run of the library as it is; the ``must``
entry of a case names the family its section is about -- a case that falls through to gather_v1 / wgrad_v1 is wrong, not the table.
A change to a conv gate, tile size or split rule must move these tables on purpose.  Batch sizes of gated cases
come from the gate's own expression and the device's CU count, so each is the smallest batch its gate admits.

Reference: F.pad (reflect) / zero padding, nearest upsample and F.conv2d on the CPU in float64, gradients from torch.autograd.grad;
a fused activation is max(v, 0) + 0.2f * min(v, 0) in fp32 rounded once to bf16 (act_slope in csrc/common.h; integer pre-activations
leave no ambiguity at the kink).

Wall time of the file on an MI355X box with 16 CPU threads: 25 s for its 98 tests, most of it the float64 references on the CPU
(the largest case, b-s2-ring, takes 2.6 s, 2.4 s of them its reference)."""
import functools
import math
from ctypes import byref, c_void_p

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12288.0             # exact in bf16 and fp32; no integer sum of a case reaches it
from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
OPTION_DEFAULTS = {"halo16": 1, "halo16_fold": 1, "dgrad_s2_ring": 1}      # the library's defaults (include/dei2i_hip.h; it has no getter)


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the gates, with the expressions of the source -------------------------------------------------------------------------------
def n_halo16(tiles_per_image, ldc):
    """halo16_shape_ok / halo16_s2_shape_ok: tiles_m * tn >= num_cu * 7 / 8 (16 x 32 tiles; tn counts 128-channel tiles from 128 channels on)"""
    tn = cdiv(ldc, 128) if ldc >= 128 else 1
    return lambda cu: cdiv((cu * 7) // 8, tiles_per_image * tn)


def n_halo8(tiles_per_image, ldc):
    """halo_conv_shape_ok: tiles_m * ceil(ldc / 128) >= num_cu / 2 from 128 channels on, tiles_m >= num_cu / 2 below (8 x 32 tiles)"""
    tn = cdiv(ldc, 128) if ldc >= 128 else 1
    return lambda cu: cdiv(cu // 2, tiles_per_image * tn)


def n_v2(rows_per_image, ldc):
    """gather_gemm_v2: tiles256 * ntn >= num_cu / 2 (BN = 128 above 64 channels; the 256-wide tile counts ldc / 256)"""
    ntn = ldc // 256 if ldc % 256 == 0 else cdiv(ldc, 128 if ldc > 64 else 64)
    return lambda cu: (cdiv(cu // 2, ntn) - 1) * 256 // rows_per_image + 1


def takes_192(rows_per_image):
    """gather_gemm_v2, BN = 128, one N tile: the 192-row tile is taken when its rounds cost less, c192 < c256"""
    def rule(cu, n):
        t256, t192 = cdiv(n * rows_per_image, 256), cdiv(n * rows_per_image, 192)
        return t256 >= cu // 2 and cdiv(t192, cu) * 192 < cdiv(t256, cu) * 256
    return rule


def n_v2_192(rows_per_image, n_at_256):
    """the batch the <192,128> case is stated for on 256 CUs; on another CU count the smallest batch at which takes_192 holds"""
    rule = takes_192(rows_per_image)
    return lambda cu: n_at_256 if cu == 256 else next(n for n in range(1, 1 << 16) if rule(cu, n))


def n_thin(tiles_per_image, extra=0):
    """thin_cin_conv / thin_cout_conv: 8 x 32 tiles >= num_cu; extra = 1: one workgroup of the persistent loop takes a second tile"""
    return lambda cu: cdiv(cu + extra, tiles_per_image)


def n_s2_ring(H, W, cins):
    """dei2i_conv2d_dgrad_input: N * H * W * CinS >= 48 << 20 sends a stride-2 reflect dgrad to the parity-class ring decomposition"""
    return lambda cu: cdiv(48 << 20, H * W * cins)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (id, seam it reaches, cin, cout, k, stride, pad, reflect, up, H, W (physical input), N, bias, act, extras)
# extras: must = {phase: family the case is listed for}; opt = {option: value} for the call (restored afterwards); phases = subset of
# "fdw" (forward, dgrad, wgrad; default all); expect = rule(cu, N) the batch must satisfy to reach its seam; acc = also accumulate = 1 onto an integer-filled dw; dx / ddy = densities of x / dy
# (default: min(1/2, 576 / K) and min(1/4, 288 / K of the dgrad), which keeps 6 sigma of an output below 160).
V1D, V1W = {"d": "gather_v1"}, {"w": "wgrad_v1"}
GENERIC = [
    # M tile edge (BM = 128) and the GEMM-N tile choice: CoutS 8 -> BN 32, 32 -> BN 32, 40 -> BN 64 ragged
    ("a-m127-co8", "M = 127: one short M tile; K = 72: one partial k-step", 8, 8, 3, 1, 1, False, False, 1, 127, 1, False, "none", {}),
    ("a-m128-co32", "M = 128: exactly one M tile; CoutS = 32 fills the 32-wide tile", 8, 32, 3, 1, 1, False, False, 8, 16, 1, True, "relu", {}),
    ("a-m129-co40", "M = 129: one row in a second M tile; CoutS = 40: ragged 64-wide tile", 8, 40, 3, 1, 1, True, False, 3, 43, 1, False, "leaky_relu", {}),
    # k-steps (bf16: 64 per step; f32: 32) and split-K slices
    ("a-nk3-co64", "K = 144: nk = 3, no split-K; CoutS = 64 fills the 64-wide tile", 16, 64, 3, 1, 1, True, False, 5, 7, 2, False, "none", {}),
    ("a-nk4-co72", "K = 216: a k tail, nk = 4: two slices; CoutS = 72: ragged 128-wide tile", 24, 72, 3, 1, 1, False, False, 6, 10, 2, True, "none", {}),
    ("a-nk5-co136", "K = 288: nk = 5, slices of 3 and 2 k-steps; CoutS = 136: second N tile ragged", 32, 136, 3, 1, 1, True, False, 4, 9, 3, False, "leaky_relu", {}),
    ("a-k4096", "K = 4096 on a 4x4 output, one tile: splits = 2 cu capped by nk / 2 (32 slices in bf16, 64 in f32)", 256, 8, 4, 1, 0, False, False, 7, 7, 1, False, "none", {}),
    # dei2i_conv2d_workspace_bytes holds 16 slabs of max(y, dx) elements: with y and dx of one size (zero padding, Cin = Cout) fit = 16,
    # below nk / 2 = 18 (bf16: K = 2304, nk = 36; f32: nk = 72, nk / 2 = 36); 2 tiles.  A launch that ignored the cap would write the
    # workspace's guard row.  The dgrad is the same GEMM and reaches the cap as well.
    ("a-ws-fit", "256 -> 256 3x3 on a 4x4 image: splits capped by nk / 2, then by the 16 slabs the workspace holds", 256, 256, 3, 1, 1, False, False, 4, 4, 1, False, "none", {}),
    # parity classes of a stride-2 dgrad
    ("a-s2k4-zero", "stride 2, 4x4: four equal parity classes, zero padding", 16, 24, 4, 2, 1, False, False, 8, 12, 2, True, "leaky_relu", {}),
    ("a-s2k4-reflect", "stride 2, 4x4: four classes on the padded frame + fold_pad_kernel", 16, 24, 4, 2, 1, True, False, 8, 12, 2, False, "none", {}),
    ("a-s2k3-zero", "stride 2, 3x3: classes of 2 and 1 taps (one descriptor shorter), zero padding, odd extents", 16, 24, 3, 2, 1, False, False, 9, 11, 2, False, "none", {}),
    ("a-s2k3-reflect", "stride 2, 3x3: unequal classes on the padded frame + fold_pad_kernel", 16, 24, 3, 2, 1, True, False, 9, 11, 2, False, "relu", {}),
    # decomposed stride-1 reflect dgrad: interior + four ring rectangles + fold_border_kernel
    ("a-ring3-h4", "3x3 pad 1 at H = 4 = 2p + 2: no row outside the border rows", 16, 16, 3, 1, 1, True, False, 4, 12, 2, False, "none", {}),
    ("a-ring3-w4", "3x3 pad 1 at W = 4 = 2p + 2 with H = 9", 16, 16, 3, 1, 1, True, False, 9, 4, 2, False, "none", {}),
    ("a-ring7-8x8", "7x7 pad 3 at H = W = 8 = 2p + 2", 8, 16, 7, 1, 3, True, False, 8, 8, 2, False, "none", {}),
    ("a-ring7-8x20", "7x7 pad 3 at 8 x 20: interior columns between the border columns", 8, 16, 7, 1, 3, True, False, 8, 20, 1, False, "none", {}),
    ("a-ring5-p1", "5x5 pad 1 (k != 2p + 1): the ring runs without sub_taps_desc", 16, 16, 5, 1, 1, True, False, 6, 9, 2, False, "none", {}),
    ("a-frame3-h3", "3x3 pad 1 at H = 3 = 2p + 1: the generic frame + fold_pad_kernel path", 16, 16, 3, 1, 1, True, False, 3, 8, 2, False, "none", {}),
    # fold_pad_kernel alone
    ("a-fold7-h4", "7x7 reflect at H = 4: rows with three folded sources", 8, 16, 7, 1, 3, True, False, 4, 9, 2, False, "none", {"ddy": 1 / 32}),
    ("a-fold7-h5", "7x7 reflect at H = 5", 8, 16, 7, 1, 3, True, False, 5, 8, 2, False, "none", {"ddy": 1 / 32}),
    ("a-fold7-h7", "7x7 reflect at H = W = 7 = 2p + 1", 8, 16, 7, 1, 3, True, False, 7, 7, 2, False, "none", {"ddy": 1 / 32}),
    ("a-fold-up-reflect", "fused upsample with reflect padding: 2x2 cells and their reflected images", 16, 16, 3, 1, 1, True, True, 4, 6, 2, False, "none", {}),
    ("a-fold-up-zero", "fused upsample with zero padding: 2x2 cells only", 16, 16, 3, 1, 1, False, True, 4, 6, 2, True, "relu", {}),
    # wgrad_v1
    ("a-wg-co64", "wgrad: Cout = 64 (64-row tile), K = 72, one pixel chunk in bf16: splits clamped to 1", 8, 64, 3, 1, 1, False, False, 8, 8, 1, False, "none", {"acc": True}),
    ("a-wg-co65", "wgrad: Cout = 65 (128-row tile), K = 200, three pixel chunks in bf16", 8, 65, 5, 1, 2, False, False, 8, 24, 1, False, "none", {"acc": True}),
    ("a-wg-slabs", "wgrad: Cout * cblocks < 512 and 11 (f32: 22) slabs: slab_group_sum_kernel with an uneven last group", 8, 8, 3, 1, 1, False, False, 22, 32, 2, False, "none", {"acc": True}),
]

H16F, H16D, H16S2 = {"f": "halo16_conv"}, {"d": "halo16_conv"}, {"f": "halo16_s2"}
TUNED = [
    # ---- B. 16 x 32 halo kernel: tiles * tn >= cu * 7 / 8 ----
    ("b-one-tile-reflect", "one 16x32 tile per image, every tile touches all four borders; one slice of 9 k-steps", 32, 128, 3, 1, 1, True, False, 16, 32, n_halo16(1, 128), False, "none", {"must": H16F}),
    ("b-one-tile-zero", "the same with zero padding", 32, 128, 3, 1, 1, False, False, 16, 32, n_halo16(1, 128), False, "none", {"must": H16F}),
    ("b-slices3-co136", "three 32-channel slices, tn = 2 with a ragged second N tile, bias + ReLU", 96, 136, 3, 1, 1, False, False, 16, 32, n_halo16(1, 136), True, "relu", {"must": H16F}),
    ("b-co72-two-phase", "the 64-channel two-phase instance: tiles_n = 2 while the gate counts 1, LeakyReLU", 64, 72, 3, 1, 1, True, False, 16, 32, n_halo16(1, 72), False, "leaky_relu", {"must": H16F}),
    ("b-up-fwd", "fused upsample forward, source 8x16", 64, 64, 3, 1, 1, True, True, 8, 16, n_halo16(1, 64), False, "none", {"must": H16F}),
    ("b-fold-128", "FOLD: smallest eligible image 32x64, every tile owns a corner", 128, 128, 3, 1, 1, True, False, 32, 64, n_halo16(4, 128), False, "none", {"must": H16D}),
    ("b-fold-128-off", "the same through the separate ring launches (halo16_fold = 0)", 128, 128, 3, 1, 1, True, False, 32, 64, n_halo16(4, 128), False, "none", {"opt": {"halo16_fold": 0}, "phases": "d", "ref": "b-fold-128"}),
    ("b-fold-dx64", "FOLD with a 64-channel dx: the 64-channel tile", 64, 128, 3, 1, 1, True, False, 32, 64, n_halo16(4, 64), False, "none", {"must": H16D}),
    ("b-fold-48x96", "FOLD at 48x96, tn = 2: a 3 x 3 tile grid per image, so corner, edge and interior tiles at the gate's minimum batch (13 images, 117 tiles)", 256, 128, 3, 1, 1, True, False, 48, 96, n_halo16(9, 256), False, "none", {"must": H16D}),
    ("b-s2-reflect", "stride 2 4x4 on 16x32 tiles, reflect + LeakyReLU", 64, 128, 4, 2, 1, True, False, 32, 64, n_halo16(1, 128), False, "leaky_relu", {"must": H16S2}),
    ("b-s2-zero", "stride 2 4x4 on 16x32 tiles, zero padding + bias", 64, 128, 4, 2, 1, False, False, 32, 64, n_halo16(1, 128), True, "none", {"must": H16S2}),
    ("b-s2-ring", "N * H * W * CinS = 48 << 20: the dgrad's parity-class ring decomposition (rows 1, H-2, columns 1, W-2, corners)", 64, 128, 4, 2, 1, True, False, 32, 64, n_s2_ring(32, 64, 64), False, "none", {"must": H16S2}),
    ("b-s2-ring-off", "the same dgrad through the frame + fold path (dgrad_s2_ring = 0)", 64, 128, 4, 2, 1, True, False, 32, 64, n_s2_ring(32, 64, 64), False, "none", {"opt": {"dgrad_s2_ring": 0}, "phases": "d", "ref": "b-s2-ring"}),
    ("b-s2-ring-64x128", "the same threshold at 64x128 (N = 96): the ring-row launch too small for gather_v2 -> gather_v2 + 2 x gather_v1 (64 -> 64)", 64, 64, 4, 2, 1, True, False, 64, 128, n_s2_ring(64, 128, 64), False, "none", {"phases": "d", "must": V1D}),
    # ---- C. 8 x 32 halo kernel: cu / 2, where the 16-row kernel refuses ----
    ("c-one-slice", "one 64-channel slice, one 8x32 tile per image", 64, 128, 3, 1, 1, True, False, 8, 32, n_halo8(1, 128), False, "none", {"must": {"f": "halo_conv"}}),
    ("c-slices3-bn64", "three slices (the halo double buffer ends on an odd slice), a middle tile without top / bottom border, BN = 64", 192, 64, 3, 1, 1, True, False, 24, 32, n_halo8(3, 64), False, "none", {"must": {"f": "halo_conv"}}),
    ("c-co136-zero", "ragged N tile, zero padding + bias", 128, 136, 3, 1, 1, False, False, 8, 64, n_halo8(2, 136), True, "none", {"must": {"f": "halo_conv"}}),
    ("c-h16-halo16-off", "H = 16 on the 8-row kernel (halo16 = 0): two tile rows", 64, 128, 3, 1, 1, True, False, 16, 32, n_halo8(2, 128), False, "none", {"must": {"f": "halo_conv"}, "opt": {"halo16": 0}}),
    # ---- D. LDS-DMA GEMM: tiles256 * ntn >= cu / 2 ----
    ("d-256x128", "<256,128>: 128 -> 128 4x4 s2 at 32x32; dgrad: four parity classes on blockIdx.y", 128, 128, 4, 2, 1, False, False, 32, 32, n_v2(256, 128), False, "none", {"must": {"f": "gather_v2", "d": "gather_v2"}}),
    ("d-256x64-ragged", "<256,64>; 17x15 outputs: every class M = 255 N is no multiple of the tile", 64, 64, 4, 2, 1, False, False, 34, 30, n_v2(255, 64), True, "leaky_relu", {"must": {"f": "gather_v2", "d": "gather_v2"}}),
    ("d-256x256", "<256,256> single round: tiles256 in [cu / 2, cu]", 128, 256, 4, 2, 1, True, False, 32, 32, n_v2(256, 256), False, "none", {"must": {"f": "gather_v2"}}),
    # (the tile variant is not a launch-count family: ``expect`` asserts gather_gemm_v2's own rule for it on this device's CU count)
    ("d-192x128", "<192,128>: M = 76 500 (N = 75), ragged last tile, c192 < c256", 64, 128, 3, 1, 1, False, False, 30, 34, n_v2_192(1020, 75), False, "none", {"must": {"f": "gather_v2"}, "expect": takes_192(1020)}),
    ("d-cin192", "Cin = 192: one 128-column k-tile spans two taps", 192, 128, 4, 2, 1, False, False, 32, 32, n_v2(256, 128), False, "relu", {"must": {"f": "gather_v2"}}),
    # ---- E. thin kernels: 8x32 tiles >= cu ----
    ("e-cin-7x7-persistent", "thin_cin 3 -> 64 7x7 reflect, cu + 1 tiles: one workgroup takes a second tile; dgrad: thin_cout without register weights", 3, 64, 7, 1, 3, True, False, 8, 32, n_thin(1, 1), False, "none", {"must": {"f": "thin_cin", "d": "thin_cout", "w": "wgrad_thin"}}),
    ("e-cin-co24", "thin_cin 3 -> 24: a partial output block", 3, 24, 3, 1, 1, True, False, 8, 32, n_thin(1), False, "none", {"must": {"f": "thin_cin"}}),
    ("e-cin-4x4s2", "thin_cin 3 -> 64 4x4 s2, bias + LeakyReLU, 16x64 -> 8x32", 3, 64, 4, 2, 1, False, False, 16, 64, n_thin(1), True, "leaky_relu", {"must": {"f": "thin_cin"}}),
    ("e-cout-persistent", "thin_cout 64 -> 4 3x3, cu + 1 tiles; dgrad: thin_cin on an 8-channel dY with flipped taps", 64, 4, 3, 1, 1, True, False, 8, 32, n_thin(1, 1), False, "none", {"must": {"f": "thin_cout", "d": "thin_cin"}}),
    ("e-cout-co8", "thin_cout 64 -> 8: every output lane live", 64, 8, 3, 1, 1, False, False, 8, 32, n_thin(1), True, "relu", {"must": {"f": "thin_cout"}}),
    ("e-cout-co1", "thin_cout 64 -> 1", 64, 1, 3, 1, 1, True, False, 8, 32, n_thin(1), False, "none", {"must": {"f": "thin_cout"}}),
    ("e-wthin-64", "wgrad_thin: 64 half-tiles exactly (8x32, N = 32), Cout = 64", 3, 64, 7, 1, 3, True, False, 8, 32, 32, False, "none", {"must": {"w": "wgrad_thin"}, "acc": True}),
    ("e-wthin-66-co24", "wgrad_thin: 66 half-tiles (N = 33): an uneven last split; Cout = 24", 3, 24, 7, 1, 3, True, False, 8, 32, 33, False, "none", {"must": {"w": "wgrad_thin"}}),
    ("e-wthin-63", "63 half-tiles (12x32, N = 21) fall through to wgrad_v1", 3, 64, 7, 1, 3, True, False, 12, 32, 21, False, "none", {"must": V1W}),
    # ---- F. wgrad_v2: Cs % 128 == 0, Cout >= 96, M >= 4096 ----
    ("f-m4096", "M = 4096 exactly: 64 chunks, nchunks / 8 caps splits at 8", 128, 128, 4, 2, 1, False, False, 32, 32, 16, False, "none", {"must": {"w": "wgrad_v2"}, "acc": True}),
    ("f-m4095", "M = 4095 (63 x 65 outputs) falls to wgrad_v1", 128, 128, 4, 2, 1, False, False, 126, 130, 1, False, "none", {"must": V1W, "phases": "w"}),
    ("f-m4100", "M = 4100: a ragged last 64-pixel chunk", 128, 128, 4, 2, 1, True, False, 50, 82, 4, False, "none", {"must": {"w": "wgrad_v2"}, "phases": "w"}),
    ("f-co96", "Cout = 96 is taken", 128, 96, 4, 2, 1, False, False, 32, 32, 16, False, "none", {"must": {"w": "wgrad_v2"}, "phases": "w"}),
    ("f-co95", "Cout = 95 is refused", 128, 95, 4, 2, 1, False, False, 32, 32, 16, False, "none", {"must": V1W, "phases": "w"}),
    ("f-co192", "Cout = 192: the 256-row tile; Cin = 256", 256, 192, 4, 2, 1, False, False, 32, 32, 16, False, "none", {"must": {"w": "wgrad_v2"}, "phases": "w"}),
    ("f-co191", "Cout = 191: the 128-row tile, two row tiles, the second ragged", 128, 191, 4, 2, 1, False, False, 32, 32, 16, False, "none", {"must": {"w": "wgrad_v2"}, "phases": "w"}),
]

# ---- which kernels served each case and phase: dei2i_launch_counts of the library as it is.  A change of dispatch moves this on purpose.
# key: case id (generic cases: "id/bf16", "id/f32"); value: {"f": forward, "d": dgrad, "w": wgrad} launch counts
FAMILIES = {
    "a-m127-co8/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-m127-co8/f32": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-m128-co32/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-m128-co32/f32": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-m129-co40/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-m129-co40/f32": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-nk3-co64/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 2, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-nk3-co64/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-nk4-co72/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-nk4-co72/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-nk5-co136/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-nk5-co136/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-k4096/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-k4096/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-ws-fit/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-ws-fit/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k4-zero/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k4-zero/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k4-reflect/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k4-reflect/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k3-zero/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k3-zero/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k3-reflect/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-s2k3-reflect/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-ring3-h4/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 2}, "w": {"wgrad_v1": 1}},
    "a-ring3-h4/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-ring3-w4/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 2}, "w": {"wgrad_v1": 1}},
    "a-ring3-w4/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-ring7-8x8/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-ring7-8x8/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-ring7-8x20/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-ring7-8x20/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-ring5-p1/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-ring5-p1/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "a-frame3-h3/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-frame3-h3/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold7-h4/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold7-h4/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold7-h5/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold7-h5/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold7-h7/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold7-h7/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold-up-reflect/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-fold-up-reflect/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-fold-up-zero/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-fold-up-zero/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-wg-co64/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-wg-co64/f32": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-wg-co65/bf16": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-wg-co65/f32": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "a-wg-slabs/bf16": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "a-wg-slabs/f32": {"f": {"gather_v1": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "b-one-tile-reflect": {"f": {"halo16_conv": 1}, "d": {"gather_v1": 2, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "b-one-tile-zero": {"f": {"halo16_conv": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "b-slices3-co136": {"f": {"halo16_conv": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "b-co72-two-phase": {"f": {"halo16_conv": 1}, "d": {"gather_v1": 2, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "b-up-fwd": {"f": {"halo16_conv": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v1": 1}},
    "b-fold-128": {"f": {"halo16_conv": 1}, "d": {"halo16_conv": 1}, "w": {"wgrad_halo": 1}},
    "b-fold-128-off": {"d": {"gather_v1": 1, "halo16_conv": 1, "splitk_finalize": 1}},
    "b-fold-dx64": {"f": {"halo16_conv": 1}, "d": {"halo16_conv": 1}, "w": {"wgrad_halo": 1}},
    "b-fold-48x96": {"f": {"halo_conv": 1}, "d": {"halo16_conv": 1}, "w": {"wgrad_halo": 1}},
    "b-s2-reflect": {"f": {"halo16_s2": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v1": 1}},
    "b-s2-zero": {"f": {"halo16_s2": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v1": 1}},
    "b-s2-ring": {"f": {"halo16_s2": 1}, "d": {"gather_v1": 1, "gather_v2": 2, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "b-s2-ring-off": {"d": {"gather_v2": 1}},
    "b-s2-ring-64x128": {"d": {"gather_v1": 2, "gather_v2": 1, "splitk_finalize": 2}},
    "c-one-slice": {"f": {"halo_conv": 1}, "d": {"gather_v1": 1, "halo_conv": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "c-slices3-bn64": {"f": {"halo_conv": 1}, "d": {"gather_v1": 1, "halo_conv": 1}, "w": {"wgrad_v1": 1}},
    "c-co136-zero": {"f": {"halo_conv": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v2": 1}},
    "c-h16-halo16-off": {"f": {"halo_conv": 1}, "d": {"gather_v1": 1, "halo_conv": 1, "splitk_finalize": 1}, "w": {"wgrad_v1": 1}},
    "d-256x128": {"f": {"gather_v2": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v2": 1}},
    "d-256x64-ragged": {"f": {"gather_v2": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v1": 1}},
    "d-256x256": {"f": {"gather_v2": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v2": 1}},
    "d-192x128": {"f": {"gather_v2": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v1": 1}},
    "d-cin192": {"f": {"gather_v2": 1}, "d": {"gather_v2": 1}, "w": {"wgrad_v1": 1}},
    "e-cin-7x7-persistent": {"f": {"thin_cin": 1}, "d": {"gather_v1": 1, "thin_cout": 1}, "w": {"wgrad_thin": 1}},
    "e-cin-co24": {"f": {"thin_cin": 1}, "d": {"gather_v1": 2}, "w": {"wgrad_v1": 1}},
    "e-cin-4x4s2": {"f": {"thin_cin": 1}, "d": {"gather_v1": 1}, "w": {"wgrad_v1": 1}},
    "e-cout-persistent": {"f": {"thin_cout": 1}, "d": {"gather_v1": 1, "thin_cin": 1}, "w": {"wgrad_v1": 1}},
    "e-cout-co8": {"f": {"thin_cout": 1}, "d": {"thin_cin": 1}, "w": {"wgrad_v1": 1}},
    "e-cout-co1": {"f": {"thin_cout": 1}, "d": {"gather_v1": 1, "thin_cin": 1}, "w": {"wgrad_v1": 1}},
    "e-wthin-64": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_thin": 1}},
    "e-wthin-66-co24": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_thin": 1}},
    "e-wthin-63": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 2, "splitk_finalize": 2}, "w": {"wgrad_v1": 1}},
    "f-m4096": {"f": {"gather_v1": 1, "splitk_finalize": 1}, "d": {"gather_v1": 1, "splitk_finalize": 1}, "w": {"wgrad_v2": 1}},
    "f-m4095": {"w": {"wgrad_v1": 1}},
    "f-m4100": {"w": {"wgrad_v2": 1}},
    "f-co96": {"w": {"wgrad_v2": 1}},
    "f-co95": {"w": {"wgrad_v1": 1}},
    "f-co192": {"w": {"wgrad_v2": 1}},
    "f-co191": {"w": {"wgrad_v2": 1}},
}


# ---- data and reference ----------------------------------------------------------------------------------------------------------
def ternary(gen, shape, density):
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    keep = torch.rand(shape, generator=gen) < density
    return (sign * keep).double()


def densities(case):
    _, _, cin, cout, k, s, _, _, _, _, _, _, _, _, ex = case
    dx = ex.get("dx", min(0.5, 576.0 / (cin * k * k)))
    ddy = ex.get("ddy", min(0.25, 288.0 / (cout * k * k / (s * s))))
    return dx, ddy


@functools.lru_cache(maxsize=1)
def reference(key):
    """float64 (x, w, bias, dy, pre-activation y, dx, dw) in NCHW / OIHW; shared by the cases with the same data (an option's A/B pair,
    the two precisions of a generic case) and never modified."""
    cin, cout, k, s, p, reflect, up, H, W, N, bias, dx_density, dy_density, seed = key
    gen = torch.Generator().manual_seed(seed)
    x = ternary(gen, (N, cin, H, W), dx_density)
    w = ternary(gen, (cout, cin, k, k), 7.0 / 8.0)           # dense: every tap, channel and output column counts
    b = ternary(gen, (cout,), 1.0) if bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    xl = F.interpolate(xr, scale_factor=2, mode="nearest") if up else xr
    if reflect and p > 0:
        frame = F.pad(xl, (p, p, p, p), mode="reflect")
        pre = F.conv2d(frame, wr, b, stride=s)
    else:
        frame = xl * 1.0                                    # the dgrad frame is the logical input itself
        pre = F.conv2d(frame, wr, b, stride=s, padding=p)
    dy = ternary(gen, tuple(pre.shape), dy_density)
    dx, gframe, dw = torch.autograd.grad(pre, [xr, frame, wr], dy, retain_graph=True)
    (fold_abs,) = torch.autograd.grad(frame, [xr], gframe.abs())      # sum of the magnitudes that fold onto one input pixel
    pre = pre.detach()
    # the conditions for bit-exactness, on the reference, no element excluded
    assert pre.abs().max().item() <= 256, ("max |y|", pre.abs().max().item())
    assert dx.abs().max().item() <= 256, ("max |dx|", dx.abs().max().item())
    assert fold_abs.max().item() <= 256, ("max sum |frame| per pixel", fold_abs.max().item())
    assert dw.abs().max().item() < 2 ** 24, ("max |dw|", dw.abs().max().item())
    assert torch.equal(pre, pre.round()) and torch.equal(dx, dx.round())
    stats = {"max_y": pre.abs().max().item(), "max_dx": dx.abs().max().item(), "max_fold": fold_abs.max().item(),
             "max_dw": dw.abs().max().item()}
    return x, w, b, dy, pre, dx, dw, stats


def nhwc(t, cs, dtype):
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, cs, dtype=dtype)
    out[..., :c] = t.permute(0, 2, 3, 1).to(dtype)
    return out


def act_ref(pre, act, dtype):
    """max(v, 0) + 0.2f * min(v, 0) in fp32, one rounding to the stored type"""
    v = pre.float()
    if act == "relu":
        v = torch.clamp_min(v, 0.0)
    elif act == "leaky_relu":
        v = torch.clamp_min(v, 0.0) + torch.tensor(0.2, dtype=torch.float32) * torch.clamp_max(v, 0.0)
    return v.to(dtype)


# ---- poisoned, guarded outputs ---------------------------------------------------------------------------------------------------
def guarded(shape, dtype, fill=float("nan")):
    """(whole allocation, view of ``shape`` filled with ``fill``, guard elements): one guard row (an image row, at least 256 bytes,
    a multiple of 256 bytes so the view keeps the alignment of an allocation) of SENTINEL before and after the view"""
    n = math.prod(shape)
    row = math.prod(shape[-2:]) if len(shape) >= 2 else 1
    g = cdiv(max(row, 1), 128) * 128
    buf = torch.empty(n + 2 * g, dtype=dtype, device=DEV)
    buf[:g] = SENTINEL
    buf[g + n:] = SENTINEL
    view = buf[g:g + n].view(shape)
    view.fill_(fill)
    return buf, view, g


def guards_intact(buf, g):
    return bool((buf[:g] == SENTINEL).all().item()) and bool((buf[-g:] == SENTINEL).all().item())


def where_report(got, ref, band=None):
    """count, first indices and -- for an NHWC tensor -- where each lies: within ``band`` pixels of two edges (corner), of one edge
    (border row / border column: a reflect fold lands on rows 1 .. pad and H-1-pad .. H-2, so band = pad + 1 there) or in the interior"""
    nan = torch.isnan(got.float())
    bad = (got != ref) | nan
    lines = [f"{int(bad.sum())} of {bad.numel()} elements differ ({int(nan.sum())} NaN)"]
    for i in bad.nonzero()[:8].tolist():
        pos = "(co, ci, ky, kx)"
        if band is not None:
            _, hh, ww, _ = got.shape
            eh, ew = min(i[1], hh - 1 - i[1]) < band, min(i[2], ww - 1 - i[2]) < band
            pos = "(n, h, w, c), " + ("corner" if eh and ew else ("border row" if eh else ("border column" if ew else "interior")))
        lines.append(f"  {tuple(i)} [{pos}]: got {got[tuple(i)].item()} want {ref[tuple(i)].item()}")
    return "\n".join(lines)


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


@pytest.fixture()
def options(request):
    """dei2i_set_option for one case; every option back at its default afterwards"""
    from de_i2i_gan_amd import _lib
    lib = _lib.load()
    touched = []

    def set_(name, value):
        touched.append(name)
        _lib.check(lib.dei2i_set_option(name.encode(), value), "set_option")

    def restore():
        for name in touched:
            lib.dei2i_set_option(name.encode(), OPTION_DEFAULTS[name])
    request.addfinalizer(restore)
    return set_


def _counts():
    from de_i2i_gan_amd import _lib
    return {k: v for k, v in _lib.launch_counts(reset=True).items() if v}


def run_case(ops, options, case, prec):
    """forward, dgrad and wgrad of one case through the C entry points on poisoned, guarded outputs -> list of failures"""
    cid, seam, cin, cout, k, s, p, reflect, up, H, W, N, bias, act, ex = case
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    N = N(cu) if callable(N) else N
    phases = ex.get("phases", "fdw")
    key = cid if case in TUNED else f"{cid}/{prec.name}"
    seed = 1000 + [c[0] for c in GENERIC + TUNED].index(ex.get("ref", cid))      # ref: the case whose data (and reference) this one shares
    dxd, dyd = densities(case)
    assert "expect" not in ex or ex["expect"](cu, N), f"{cid}: N = {N} does not reach its seam on {cu} CUs"
    x, w, b, dy, pre, dx_ref, dw_ref, _ = reference((cin, cout, k, s, p, reflect, up, H, W, N, bias, dxd, dyd, seed))
    cins, couts = prec.pad(cin), prec.pad(cout)
    geom = ops.ConvGeom(cin, cout, k, s, p, reflect, up)
    xd = nhwc(x, cins, prec.dtype).to(DEV)
    dyd_ = nhwc(dy, couts, prec.dtype).to(DEV)
    wd_ = w.float().to(DEV)
    bd = b.float().to(DEV) if b is not None else None
    lib = ops._lib_for(xd)
    d = ops._desc(prec, geom, N, H, W, cins, couts)
    wf, wdg = ops.PackedWeights().get(wd_, (wd_,), prec, geom, cins, couts, need_dgrad=True)
    for name, value in ex.get("opt", {}).items():
        options(name, value)
    ws_elems = cdiv(lib.dei2i_conv2d_workspace_bytes(byref(d)), 4)
    fails, fam = [], {}
    st = ops._stream()
    torch.cuda.synchronize()
    _counts()

    def check_guards(what, pairs):
        for nm, (buf, g) in pairs.items():
            if not guards_intact(buf, g):
                fails.append(f"{what}: the guard rows of {nm} were written")

    if "f" in phases:
        ho, wo = pre.shape[-2:]
        ybuf, y, yg = guarded((N, ho, wo, couts), prec.dtype)
        wsbuf, ws, wsg = guarded((ws_elems,), torch.float32)
        rc = lib.dei2i_conv2d_fwd(byref(d), ops._p(xd), ops._p(wf), ops._p(bd), ops.ACT[act], ops._p(y), ops._p(ws), ws_elems * 4, st)
        torch.cuda.synchronize()
        fam["f"] = _counts()
        assert rc == 0, ("conv2d_fwd", rc)
        y_ref = nhwc(act_ref(pre, act, prec.dtype), couts, prec.dtype)
        got = y.cpu()
        if not torch.equal(got, y_ref):
            fails.append("forward: " + where_report(got, y_ref, band=1))
        check_guards("forward", {"y": (ybuf, yg), "workspace": (wsbuf, wsg)})
        del ybuf, y, wsbuf, ws
    if "d" in phases:
        dxbuf, dxo, dxg = guarded((N, H, W, cins), prec.dtype)
        wsbuf, ws, wsg = guarded((ws_elems,), torch.float32)
        oh, ow = (H << up) + (2 * p if reflect else 0), (W << up) + (2 * p if reflect else 0)
        extbuf, ext, extg = guarded((N, oh, ow, cins), prec.dtype)
        rc = lib.dei2i_conv2d_dgrad_input(byref(d), ops._p(dyd_), ops._p(wdg), ops._p(ext), ops._p(dxo), ops._p(ws), ws_elems * 4, st)
        torch.cuda.synchronize()
        fam["d"] = _counts()
        assert rc == 0, ("conv2d_dgrad_input", rc)
        ref = nhwc(dx_ref, cins, prec.dtype)
        got = dxo.cpu()
        if not torch.equal(got, ref):
            fails.append("dgrad: " + where_report(got, ref, band=p + 1))
        check_guards("dgrad", {"dx": (dxbuf, dxg), "workspace": (wsbuf, wsg), "frame scratch": (extbuf, extg)})
        del dxbuf, dxo, wsbuf, ws, extbuf, ext
    if "w" in phases:
        packed = lib.dei2i_wgrad_slab_elems(byref(d))
        sc_elems = max(packed * 4, min(max(packed * 4 * 64, 96 << 20), 512 << 20)) // 4 + 1       # ops._wgrad_scratch
        scbuf, sc, scg = guarded((sc_elems,), torch.float32)
        dwbuf, dwo, dwg = guarded((cout, cin, k, k), torch.float32)
        rc = lib.dei2i_conv2d_wgrad_oihw(byref(d), ops._p(xd), ops._p(dyd_), ops._p(sc), sc_elems, c_void_p(dwo.data_ptr()), 0, st)
        torch.cuda.synchronize()
        fam["w"] = _counts()
        assert rc == 0, ("conv2d_wgrad_oihw", rc)
        ref = dw_ref.float()
        got = dwo.cpu()
        if not torch.equal(got, ref):
            fails.append("wgrad: " + where_report(got, ref))
        if ex.get("acc"):
            base = torch.randint(-3, 4, ref.shape, generator=torch.Generator().manual_seed(7)).float()
            dwo.copy_(base)
            sc.fill_(float("nan"))
            rc = lib.dei2i_conv2d_wgrad_oihw(byref(d), ops._p(xd), ops._p(dyd_), ops._p(sc), sc_elems, c_void_p(dwo.data_ptr()), 1, st)
            torch.cuda.synchronize()
            _counts()
            assert rc == 0, ("conv2d_wgrad_oihw accumulate", rc)
            got = dwo.cpu()
            if not torch.equal(got, ref + base):
                fails.append("wgrad accumulate = 1: " + where_report(got, ref + base))
        check_guards("wgrad", {"dw": (dwbuf, dwg), "slab scratch": (scbuf, scg)})
        del scbuf, sc, dwbuf, dwo
    assert not fails, f"{key} ({seam}):\n" + "\n".join(fails)
    for ph, family in ex.get("must", {}).items():
        assert fam[ph].get(family, 0) >= 1, f"{key}: the case is listed for {family} but its {ph} phase ran {fam[ph]}"
    assert fam == FAMILIES.get(key), f"{key}: dispatch moved: ran {fam}, pinned {FAMILIES.get(key)}"


@pytest.mark.parametrize("prec_name", ["bf16", "f32"])
@pytest.mark.parametrize("case", GENERIC, ids=[c[0] for c in GENERIC])
def test_generic_kernels_exact_on_integers(ops, options, case, prec_name):
    """A. gather_v1, the split-K finalize, fold_pad_kernel / fold_border_kernel and wgrad_v1 (+ slab sums) on tiny shapes, both types"""
    run_case(ops, options, case, ops.BF16 if prec_name == "bf16" else ops.F32)


@pytest.mark.parametrize("case", TUNED, ids=[c[0] for c in TUNED])
def test_tuned_kernels_exact_on_integers(ops, options, case):
    """B .. F. every bf16-only family at the smallest batch its gate admits"""
    run_case(ops, options, case, ops.BF16)


# ---- refusals: DEI2I_ERR_BAD_ARG and a poisoned output left untouched ----------------------------------------------------------------
# (id, entry point, cin, cout, k, stride, pad, reflect, H, W, CinS override, null frame scratch)
REFUSALS = [
    ("kh-below-stride", "fwd", 8, 8, 1, 2, 0, False, 8, 8, None, False),
    ("kh-below-stride-dgrad", "dgrad", 8, 8, 1, 2, 0, False, 8, 8, None, False),
    ("reflect-pad-reaches-H", "fwd", 8, 8, 7, 1, 3, True, 3, 8, None, False),
    ("reflect-pad-reaches-H-wgrad", "wgrad", 8, 8, 7, 1, 3, True, 3, 8, None, False),
    ("cins-not-a-vector-multiple", "fwd", 8, 8, 3, 1, 1, False, 8, 8, 12, False),
    ("stride-3-dgrad", "dgrad", 8, 8, 3, 3, 1, False, 9, 9, None, False),
    ("null-frame-scratch", "dgrad", 8, 8, 3, 1, 1, True, 8, 8, None, True),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_leave_the_output_untouched(ops, case):
    from de_i2i_gan_amd import _lib as L
    cid, entry, cin, cout, k, s, p, reflect, H, W, cins_override, null_ext = case
    prec = ops.BF16
    cins, couts = cins_override or prec.pad(cin), prec.pad(cout)
    N = 2
    d = L.ConvDesc(prec.code, N, H, W, cin, cout, cins, couts, k, k, s, p, L.PAD_REFLECT if reflect else L.PAD_ZERO, 0)
    big = 4 * N * (H + 2 * p) * (W + 2 * p) * max(cins, couts) * k * k
    src = torch.zeros(big, dtype=prec.dtype, device=DEV)                     # stands for x / dy / the packed weights: never read
    lib = ops._lib_for(src)
    outbuf, out, og = guarded((big,), prec.dtype if entry != "wgrad" else torch.float32)
    ws = torch.full((1 << 16,), float("nan"), dtype=torch.float32, device=DEV)
    ext = torch.full((big,), float("nan"), dtype=prec.dtype, device=DEV)
    st = ops._stream()
    _counts()
    if entry == "fwd":
        rc = lib.dei2i_conv2d_fwd(byref(d), ops._p(src), ops._p(src), None, 0, ops._p(out), ops._p(ws), ws.numel() * 4, st)
    elif entry == "dgrad":
        rc = lib.dei2i_conv2d_dgrad_input(byref(d), ops._p(src), ops._p(src), None if null_ext else ops._p(ext), ops._p(out), ops._p(ws),
                                          ws.numel() * 4, st)
    else:
        rc = lib.dei2i_conv2d_wgrad_oihw(byref(d), ops._p(src), ops._p(src), ops._p(ws), ws.numel(), c_void_p(out.data_ptr()), 0, st)
    torch.cuda.synchronize()
    assert rc == BAD_ARG, (cid, rc)
    assert _counts() == {}, "a refused call launched a kernel"
    assert bool(torch.isnan(out.float()).all().item()) and bool(torch.isnan(ext.float()).all().item()) and bool(torch.isnan(ws).all().item())
    assert guards_intact(outbuf, og)
