"""Case tables, data builders and float64 references of tests/test_elementwise_edges_gpu.py and tests/test_diffaug_edges_gpu.py, and
the conditions their exactness arguments rest on -- checked here without a GPU, nothing excluded: the integer ranges, that every
bit-exact reference is representable in bf16, that no pre-activation sits on a kink, that every z class meets every vector lane,
that every saturation value is planted in every image, that every DiffAugment record category is in the table, and that the sizes
named for a grid cap equal cap x 256 (+ the stated remainder) with the caps read from the .hip sources as they are written.

The DiffAugment reference (``diffaug_ref``) is the header comment of csrc/diffaug.hip in float64; before it judges the kernel it is
anchored to ``oracle.diff_augment`` from the same seed (test_diffaug_reference_equals_the_oracle)."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import defectgan_oracle as O

CSRC = Path(__file__).resolve().parents[1] / "de-i2i-gan_amd" / "csrc"
DTYPES = ["bf16", "f32"]
VEC = {"bf16": 8, "f32": 4}
TORCH_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
THREADS = 256
EW_CAP = 4096            # elementwise.hip: EW_CAP workgroups of 256 threads
POOL_CAP = 2048          # launch.h: grid_for's default cap, the one the average pool takes
IMG_CAP = 512            # dei2i_affine_act_img_fwd: at most 512 workgroups per image
MAX_CHUNKS = 64          # diffaug.hip: kMaxChunks
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rounded(t, pname):
    return t.to(torch.bfloat16).float() if pname == "bf16" else t.float()


def bf16_exact(t):
    t = t.double()
    return bool((t.to(torch.bfloat16).double() == t).all())


# ---- the average pool -----------------------------------------------------------------------------------------------------------
POOL_SMALL = [(1, 2, 2, 1),        # one item
              (3, 2, 10, 1),       # Ho = 1, Wo odd
              (2, 6, 2, 3),        # Wo = 1, cv = 3
              (2, 10, 14, 5)]      # odd Ho, Wo and cv, several images
POOL_CAPPED = [(2, 1024, 1024, 1),     # N Ho Wo cv = 2 * 512 * 512 = 524 288 = 2048 x 256: the cap reached exactly, one trip
               (29, 202, 358, 1)]      # 29 * 101 * 179 = 524 291 = 2048 x 256 + 3 cv: three items of a second trip


def pool_items(shape):
    n, h, w, cv = shape
    return n * (h // 2) * (w // 2) * cv


@functools.lru_cache(maxsize=2)
def pool_problem(shape, pname):
    """x (N, H, W, C) integers in [-31, 31], dout (N, H/2, W/2, C) integers in [-127, 127], both NHWC in the compute dtype; out and
    dx: float64 F.avg_pool2d and its autograd gradient, cast to the compute dtype (exact: see the conditions test)"""
    n, h, w, cv = shape
    c, dt = cv * VEC[pname], TORCH_DTYPE[pname]
    g = gen(100 + n + h + w + cv)
    x = torch.randint(-31, 32, (n, h, w, c), generator=g).to(dt)
    dout = torch.randint(-127, 128, (n, h // 2, w // 2, c), generator=g).to(dt)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    out64 = F.avg_pool2d(x64, 2)
    (dx64,) = torch.autograd.grad(out64, x64, dout.double().permute(0, 3, 1, 2))
    out64, dx64 = out64.detach().permute(0, 2, 3, 1).contiguous(), dx64.permute(0, 2, 3, 1).contiguous()
    return dict(x=x, dout=dout, out64=out64, dx64=dx64, out=out64.to(dt), dx=dx64.to(dt))


# ---- act_bwd ----------------------------------------------------------------------------------------------------------------------
Z_CLASSES = [-2.0, -0.5, -0.0, 0.0, 0.5, 3.0]
ACT_BWD_NVEC = [1, 255, 256, 257, EW_CAP * THREADS, EW_CAP * THREADS + 3]
LRELU_SLOPE = float(np.float32(0.2))          # common.h act_grad_from_out: the fp32 constant 0.2f


def act_bwd_rotations(nvec):
    """class of element (v, e) is Z_CLASSES[(v + e + rot) % 6]: with >= 6 vectors one rotation shows every class to every lane, below
    that the test calls once per rotation"""
    return [0] if nvec >= len(Z_CLASSES) else list(range(len(Z_CLASSES)))


def act_bwd_problem(nvec, pname, rot=0):
    vec, dt = VEC[pname], TORCH_DTYPE[pname]
    dz = torch.randint(-127, 128, (nvec, vec), generator=gen(nvec % 1000 + rot)).to(dt)
    cls = (torch.arange(nvec).view(-1, 1) + torch.arange(vec).view(1, -1) + rot) % len(Z_CLASSES)
    z = torch.tensor(Z_CLASSES, dtype=torch.float32)[cls].to(dt)
    return dict(dz=dz, z=z, cls=cls)


def act_bwd_ref(P, act, pname):
    """dz * s with s by the kernel's convention (common.h): ReLU z > 0 -> 1 else 0; LeakyReLU z >= 0 -> 1 else float32(0.2); none 1.
    The float64 product of two fp32 values is exact: rounding it to fp32 and then to the compute dtype is the kernel's arithmetic."""
    z, dz = P["z"].double(), P["dz"].double()
    if act == ACT_RELU:
        s = (z > 0).double()
    elif act == ACT_LRELU:
        s = torch.where(z >= 0, torch.ones_like(z), torch.full_like(z, LRELU_SLOPE))
    else:
        s = torch.ones_like(z)
    return (dz * s).float().to(TORCH_DTYPE[pname])


# ---- affine_act_img ---------------------------------------------------------------------------------------------------------------
IMG_SHAPES = [(1, 1, 1), (3, 5, 1), (2, 7, 2), (2, 3, 256),
              (2, 3, 512),         # cv % 256 == 0: 2 workgroups per pixel row
              (2, 171, 768),       # min(3 * 171 + 1, 512) = 512 workgroups rounded down to 510, then 768 vectors of a second trip
              (2, 32769, 4)]       # nvec_img = 131 076 = 512 x 256 + 4: the cap and one ragged trip
IMG_SLOPES = [0.0, 0.25, 1.0]
IMG_A, IMG_B = [1.0, 2.0, -1.0, 0.5], [0.5, -0.5, 1.5, -1.5]


def img_blocks(hw, cv):
    """the launch geometry of dei2i_affine_act_img_fwd, restated"""
    nvec = hw * cv
    blocks = min((nvec + THREADS - 1) // THREADS, IMG_CAP)
    if cv > THREADS:
        blocks = blocks // (cv // THREADS) * (cv // THREADS)
    return max(blocks, cv // THREADS if cv > THREADS else 1), nvec


def act64(v, slope):
    """slope * min(v, 0) + max(v, 0): LeakyReLU for slope 0.2 / 0.25, ReLU for 0 (a +0 for every negative v, as torch.relu gives), v for 1"""
    return v.clamp(min=0) + slope * v.clamp(max=0)


@functools.lru_cache(maxsize=4)
def img_problem(shape, pname, exact=True):
    """x (N, HW, C) in the compute dtype, A / B (N, C) fp32 drawn independently per (image, channel).  exact: x integers in [-8, 8],
    A in IMG_A, B in IMG_B.  The one combination that meets the kink (A = 0.5, x odd, |x| <= 3: 0.5 x + B = 0) has x moved by 2, which
    stays inside [-8, 8]; every other draw is kept."""
    n, hw, cv = shape
    c, dt = cv * VEC[pname], TORCH_DTYPE[pname]
    g = gen(7 + hw + cv)
    if exact:
        x = torch.randint(-8, 9, (n, hw, c), generator=g).float()
        A = torch.tensor(IMG_A)[torch.randint(0, 4, (n, c), generator=g)]
        B = torch.tensor(IMG_B)[torch.randint(0, 4, (n, c), generator=g)]
        on_kink = (A[:, None, :] * x + B[:, None, :]) == 0
        x = torch.where(on_kink, x + 2, x)
    else:
        x = rounded(torch.randn(n, hw, c, generator=g) * 1.7 + 0.3, pname)
        A = 1 + 0.3 * torch.randn(n, c, generator=g)
        B = 0.5 * torch.randn(n, c, generator=g)
    pre64 = A.double()[:, None, :] * x.double() + B.double()[:, None, :]
    return dict(x=x.to(dt), A=A, B=B, pre64=pre64)


# ---- compose ----------------------------------------------------------------------------------------------------------------------
COMPOSE_SHAPES = [(1, 1, 1), (3, 9, 7), (1, 1, EW_CAP * THREADS), (1, 1, EW_CAP * THREADS + 3)]
SAT3, SAT012 = [-100.0, -20.0, 0.0, 20.0, 100.0], [-30.0, 30.0]
PAD_FILL = 3.0e4                   # what the padded channels of ``raw`` hold in the forward: large, finite, bf16-exact after rounding


@functools.lru_cache(maxsize=2)
def compose_problem(shape, pname):
    """raw4 (N, H, W, 4) = randn * 1.5 rounded to the compute dtype, with the saturation values planted in every image that has the
    7 pixels for them (channel 3: SAT3 at pixels 0..4, channels 0..2: SAT012 at pixels 5, 6; the last planted +-100 pixels also carry
    +-30); x_in, d_out, d_prob fp32 NCHW.  References in float64 by autograd: with both cotangents, with d_out = 0 and with d_prob = 0.
    The same formula in fp32 on the CPU gives the reference's own rounding (``f32``)."""
    n, h, w = shape
    hw = h * w
    g = gen(31 + n + hw % 1000)
    raw4 = torch.randn(n, hw, 4, generator=g) * 1.5
    if hw >= 7:
        raw4[:, 0:5, 3] = torch.tensor(SAT3)
        raw4[:, 5, 0:3] = SAT012[0]
        raw4[:, 6, 0:3] = SAT012[1]
        raw4[:, 0, 0:3] = torch.tensor([30.0, -30.0, 30.0])          # p = 0 exactly under a saturated foreground
        raw4[:, 4, 0:3] = torch.tensor([-30.0, 30.0, -30.0])         # p = 1 exactly
    raw4 = rounded(raw4, pname).reshape(n, h, w, 4)
    x = torch.rand(n, 3, h, w, generator=g) * 2 - 1
    go, gp = torch.randn(n, 3, h, w, generator=g), torch.randn(n, 1, h, w, generator=g)

    def run(dtype):
        rr = raw4.to(dtype).permute(0, 3, 1, 2).clone().requires_grad_(True)
        xr = x.to(dtype).clone().requires_grad_(True)
        p = torch.sigmoid(rr[:, 3:4])
        out = xr * (1 - p) + torch.tanh(rr[:, :3]) * p
        R = dict(out=out.detach(), prob=p.detach())
        for key, a, b in (("both", go, gp), ("no_dout", torch.zeros_like(go), gp), ("no_dprob", go, torch.zeros_like(gp))):
            d_raw, d_x = torch.autograd.grad([out, p], [rr, xr], [a.to(dtype), b.to(dtype)], retain_graph=True)
            R[key] = (d_raw.permute(0, 2, 3, 1).contiguous(), d_x)           # d_raw back in NHWC (N, H, W, 4)
        return R

    return dict(raw4=raw4, x=x, go=go, gp=gp, f64=run(torch.float64), f32=run(torch.float32))


def compose_raw(P, cs, pname, pad_value=0.0):
    """(N, H, W, Cs) in the compute dtype: raw4 in channels 0..3, ``pad_value`` (sign alternating) in the padded channels"""
    n, h, w, _ = P["raw4"].shape
    raw = torch.empty(n, h, w, cs)
    raw[..., 4:] = pad_value * (1 - 2 * (torch.arange(cs - 4) % 2)).float()
    raw[..., :4] = P["raw4"]
    return raw.to(TORCH_DTYPE[pname])


# ---- the NaN guard ----------------------------------------------------------------------------------------------------------------
BIG_NVEC = EW_CAP * THREADS + 3
DT_MAX_BITS = {"bf16": 0x7F7F, "f32": 0x7F7FFFFF}
NEG_NAN_BITS = {"bf16": 0xFFC5, "f32": 0xFFC01234}            # sign set, quiet, a payload
SUBNORMAL_BITS = {"bf16": 0x0003, "f32": 0x00000123}
# (size in vectors, placement): where the single NaN goes.  ("vec", v, lane)
NAN_CASES = [
    (1, "element0"), (1, "last_lane"), (1, "negative_payload"),
    (255, "element0"), (255, "thread63"), (255, "last_vector"),
    (257, "last_lane"), (257, "thread255"), (257, "last_vector"), (257, "negative_payload"),
    (BIG_NVEC, "second_trip"), (BIG_NVEC, "last_vector"),
]
NAN_CLEAN_NVEC = [1, 255, 257, BIG_NVEC]


def int_dtype(pname):
    return torch.int16 if pname == "bf16" else torch.int32


def from_bits(pattern, pname):
    if pname == "bf16":
        return torch.tensor([pattern], dtype=torch.int32).to(torch.int16).view(torch.bfloat16)[0]
    return torch.tensor([pattern], dtype=torch.int64).to(torch.int32).view(torch.float32)[0]


def nan_position(nvec, placement, pname):
    vec = VEC[pname]
    return {"element0": 0, "negative_payload": 0 if nvec == 1 else 5 * vec + 2, "last_lane": min(nvec - 1, 100) * vec + vec - 1,
            "thread63": 63 * vec + 1, "thread255": 255 * vec + 2, "last_vector": (nvec - 1) * vec + 1,
            "second_trip": (EW_CAP * THREADS + 1) * vec + vec - 2}[placement]


def nan_guard_data(nvec, pname, placement=None, seed=0):
    """randn in the compute dtype with +inf, -inf, -0.0, a subnormal, +max, -max planted (as many of them, in that order, as the size
    has room for beside the NaN) and one NaN at ``placement`` (None: no NaN).  -> (x, expected): expected is the reference's rule,
    ``torch.nan_to_num(x) if x.isnan().any() else x`` (generator.py:266-267), on the CPU."""
    vec, dt = VEC[pname], TORCH_DTYPE[pname]
    n = nvec * vec
    x = torch.randn(n, generator=gen(nvec % 1000 + seed)).to(dt)
    hold = -1 if placement is None else nan_position(nvec, placement, pname)
    plants = [from_bits(0x7F80 if pname == "bf16" else 0x7F800000, pname), from_bits(0xFF80 if pname == "bf16" else 0xFF800000, pname),
              from_bits(0x8000 if pname == "bf16" else 0x80000000, pname), from_bits(SUBNORMAL_BITS[pname], pname),
              from_bits(DT_MAX_BITS[pname], pname), from_bits(DT_MAX_BITS[pname] | (0x8000 if pname == "bf16" else 0x80000000), pname)]
    spots = [i for i in [1, n - 1, 2, 3, n // 2, n // 2 + 1, 5, 6, 7, 9, 10] if 0 <= i < n and i != hold]
    spots = list(dict.fromkeys(spots))[:len(plants)]
    for i, v in zip(spots, plants):
        x[i] = v
    if placement is not None:
        x[hold] = from_bits(NEG_NAN_BITS[pname], pname) if placement == "negative_payload" else float("nan")
    expected = torch.nan_to_num(x) if bool(x.isnan().any()) else x.clone()
    return x, expected


# ---- DiffAugment ------------------------------------------------------------------------------------------------------------------
GEO_SHAPES = [((3, 12, 16), (6, 6)), ((3, 7, 10), (3, 4)), ((1, 5, 3), (2, 1))]       # (C, H, W), (ch, cw)
GEO_CATEGORIES = ["identity", "tx+4", "tx-4", "tx+1", "tx-3", "tx+6", "ty+2", "ty-2", "ty+(H-1)", "ty-(H-1)", "ty=H", "tx=-W",
                  "hole_inside", "hole_top<0", "hole_left<0", "hole_bottom>H", "hole_right>W", "everything_cut", "no_hole",
                  "translation+hole"]


def records(rows):
    """rows of (a, b, k, beta, ty, tx, top, left) -> int32 (N, 8) in the layout of utils.diffaug.REC_FIELDS (the floats bitwise)"""
    rec = np.zeros((len(rows), 8), dtype=np.int32)
    rec.view(np.float32)[:, :4] = np.array([r[:4] for r in rows], dtype=np.float32)
    rec[:, 4:] = np.array([r[4:] for r in rows], dtype=np.int32)
    return rec


def geo_tables(chw, hole):
    """-> [(ch, cw, names, rows)]: one entry per call (ch and cw belong to the call, every sample carries another record).  A record
    that wants no hole in a call that has one keeps it outside the image (top = H + 2, left = W + 2)."""
    _, H, W = chw
    ch, cw = hole
    out = (H + 2, W + 2)
    left_in = 5 if W >= 12 else 1                                # == 1 mod 4: quads straddle both edges of the hole
    ident = (1.0, 0.0, 0.0, 0.0)
    main = [("identity", 0, 0) + out,
            ("tx+4", 0, 4) + out, ("tx-4", 0, -4) + out,                                     # fast quads (W % 4 == 0)
            ("tx+1", 0, 1) + out, ("tx-3", 0, -3) + out, ("tx+6", 0, 6) + out,               # slow quads, straddling both image edges
            ("ty+2", 2, 0) + out, ("ty-2", -2, 0) + out, ("ty+(H-1)", H - 1, 0) + out, ("ty-(H-1)", -(H - 1), 0) + out,
            ("ty=H", H, 0) + out, ("tx=-W", 0, -W) + out,                                    # everything masked
            ("hole_inside", 0, 0, 1, left_in),
            ("hole_top<0", 0, 0, -((ch + 1) // 2), 2 if W > 3 else 0),
            ("hole_left<0", 0, 0, 1, -((cw + 1) // 2) if cw > 1 else -1),
            ("hole_bottom>H", 0, 0, H - (ch + 1) // 2, 1),
            ("hole_right>W", 0, 0, 1, W - (cw + 1) // 2 if cw > 1 else W - 1),
            ("translation+hole", 2, -3, H - ch + 1, 0)]          # the hole overlaps the bottom band ty vacates and the left band of tx
    cut = [("everything_cut", 0, 0, 0, 0), ("everything_cut", 1, -1, -1, 0)]
    none = [("no_hole", 0, 0, 3, 3), ("no_hole", 1, -1, 2, 2)]

    def pack(rows):
        return [r[0] for r in rows], records([ident + r[1:] for r in rows])

    return [(ch, cw) + pack(main), (H + 1, W) + pack(cut), (0, 0) + pack(none)]


def rec_fields(rec):
    rec = np.ascontiguousarray(rec)
    f = torch.from_numpy(rec.view(np.float32)[:, :4].copy())
    return f, [tuple(int(v) for v in r[4:]) for r in rec]


def diffaug_geometry(L, geo, ch, cw):
    """Cut . Trans of (N, C, H, W): out[n, :, i, j] = L[n, :, i + ty, j + tx] where that is inside, 0 elsewhere and in the hole"""
    _, _, H, W = L.shape
    out = torch.zeros_like(L)
    for n, (ty, tx, top, left) in enumerate(geo):
        i0, i1, j0, j1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(W, W - tx)
        if i0 < i1 and j0 < j1:
            out[n, :, i0:i1, j0:j1] = L[n, :, i0 + ty:i1 + ty, j0 + tx:j1 + tx]
        t0, t1, l0, l1 = max(0, top), min(H, top + ch), max(0, left), min(W, left + cw)
        if t0 < t1 and l0 < l1:
            out[n, :, t0:t1, l0:l1] = 0
    return out


def diffaug_ref(x, rec, ch, cw, mode, g=None, coef=None):
    """csrc/diffaug.hip's header in the dtype of ``x`` (float64: the reference; float32: the reference's own rounding):
    mode 0: y = Cut Trans (L x + beta), L(x)[c] = a x[c] + b mean_c(x) + k mean_chw(x); mode 1: the same with beta = 0;
    mode 2: torch.autograd.grad of mode 1 at the cotangent ``g`` (x then only gives the shape).  ``coef``: (N, 4) a, b, k, beta to
    use in place of the record's fp32 ones."""
    f, geo = rec_fields(rec)
    f = (f if coef is None else coef).to(x.dtype)
    a, b, k, beta = (f[:, i].view(-1, 1, 1, 1) for i in range(4))

    def fwd(t, with_beta):
        L = a * t + b * t.mean(dim=1, keepdim=True) + k * t.mean(dim=(1, 2, 3), keepdim=True)
        return diffaug_geometry(L + beta if with_beta else L, geo, ch, cw)

    if mode < 2:
        return fwd(x, mode == 0)
    t = torch.zeros_like(x).requires_grad_(True)
    y = fwd(t, False)
    if not y.requires_grad:                                           # every pixel of every sample masked: the operator is 0
        return torch.zeros_like(x)
    (gx,) = torch.autograd.grad(y, t, g.to(x.dtype))
    return gx


COLOR_SEAMS = [(1, 1),          # one chunk
               (1, 64),         # 64 chunks of one row
               (1, 65),         # want = 64, rpc = 2: 33 chunks, the last of one row
               (17, 70),        # want = ceil(1024 / 17) = 61, rpc = 2: 35 chunks
               (1025, 4)]       # want = 1: one chunk, N above 1024
COLOR_W = 8
COLOR_CHANNELS = [1, 3, 4]


def chunking(n, h):
    """diffaug.hip chunking(), restated"""
    want = max(1, min(MAX_CHUNKS, (1024 + n - 1) // n))
    want = min(want, h)
    rpc = (h + want - 1) // want
    return rpc, (h + rpc - 1) // rpc


def color_records(n, h, w, first=0):
    """n records cycling, from ``first``, through the 27 corners (ks, kc, beta) in {0, 1, 2} x {0.5, 1, 1.5} x {-0.5, 0, 0.5} (a = kc ks,
    b = kc (1 - ks), k = 1 - kc), each with one of three geometry records; the cycle starts at kc = 1.5 (k = -0.5), ks = 2 so that a
    single-sample case has the mean term.  -> (ch, cw, rec)"""
    ch, cw = max(1, h // 2), w // 2
    geos = [(1, -3, h + 2, w + 2),                 # translation alone (slow quads), no hole
            (0, 0, -1, -2),                        # a hole clipped by the top and the left border
            (-1, 4, min(1, h - 1), 1)]             # fast quads, a hole inside
    corners = [(ks, kc, bt) for kc in (1.5, 0.5, 1.0) for ks in (2.0, 0.0, 1.0) for bt in (-0.5, 0.5, 0.0)]
    rows = []
    for i in range(first, first + n):
        ks, kc, bt = corners[i % 27]
        rows.append((kc * ks, kc * (1 - ks), 1 - kc, bt) + geos[(i + i // 27) % 3])
    return ch, cw, records(rows)


def color_image(n, c, h, w, seed=3):
    return torch.rand(n, c, h, w, generator=gen(seed + h))          # in [0, 1]: the mean of about 0.5 makes a dropped row visible


# =================================================================================================================================
# the conditions
# =================================================================================================================================
def test_caps_are_the_constants_of_the_sources():
    ew = (CSRC / "elementwise.hip").read_text()
    m = re.search(r"EW_CAP = (\d+)u \* (\d+)u;", ew)
    assert int(m.group(1)) * int(m.group(2)) == EW_CAP
    m = re.search(r"grid_for\(size_t work_items, int threads, unsigned cap = (\d+)u \* (\d+)u\)", (CSRC / "launch.h").read_text())
    assert int(m.group(1)) * int(m.group(2)) == POOL_CAP
    assert re.search(r"avgpool2_fwd_kernel<T>, dim3\(grid_for\(total, 256\)\)", ew) and re.search(r"avgpool2_bwd_kernel<T>, dim3\(grid_for\(total, 256\)\)", ew)
    assert re.search(r"std::min<size_t>\(\(nvec_img \+ 255\) / 256, (\d+)\)", ew).group(1) == str(IMG_CAP)
    assert re.search(r"constexpr int kMaxChunks = (\d+);", (CSRC / "diffaug.hip").read_text()).group(1) == str(MAX_CHUNKS)
    assert re.search(r"return z >= 0\.f \? 1\.f : 0\.2f;", (CSRC / "common.h").read_text())        # LeakyReLU takes 1 at z = 0


def test_sizes_named_for_a_cap_sit_on_it():
    assert pool_items(POOL_CAPPED[0]) == POOL_CAP * THREADS == 524288
    assert pool_items(POOL_CAPPED[1]) == POOL_CAP * THREADS + 3 * POOL_CAPPED[1][3]
    assert ACT_BWD_NVEC[-2:] == [EW_CAP * THREADS, EW_CAP * THREADS + 3] and EW_CAP * THREADS == 1048576
    assert [s[1] * s[2] for s in COMPOSE_SHAPES[-2:]] == [EW_CAP * THREADS, EW_CAP * THREADS + 3]
    assert BIG_NVEC == EW_CAP * THREADS + 3
    assert img_blocks(3, 512) == (6, 1536)
    assert img_blocks(171, 768) == (510, 510 * THREADS + 768)        # 512 rounded down to a multiple of 3; 768 vectors left over
    assert all(img_blocks(hw, cv)[0] == min((hw * cv + 255) // 256, IMG_CAP) for _, hw, cv in IMG_SHAPES if (hw, cv) != (171, 768))
    assert img_blocks(32769, 4) == (IMG_CAP, IMG_CAP * THREADS + 4)
    for _, hw, cv in IMG_SHAPES:
        assert (img_blocks(hw, cv)[0] * THREADS) % cv == 0           # a thread keeps one channel vector
    assert [chunking(n, h) for n, h in COLOR_SEAMS] == [(1, 1), (1, 64), (2, 33), (2, 35), (4, 1)]
    assert MAX_CHUNKS == 64 and (1024 + 17 - 1) // 17 == 61


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", POOL_SMALL + POOL_CAPPED, ids=str)
def test_pool_data_makes_the_arithmetic_exact(shape, pname):
    P = pool_problem(shape, pname)
    x, dout = P["x"].double(), P["dout"].double()
    assert x.abs().max() <= 31 and dout.abs().max() <= 127 and torch.equal(x, x.round()) and torch.equal(dout, dout.round())
    assert (4 * P["out64"]).abs().max() <= 124                        # |k| <= 124 < 256: k / 4 has 8 significant bits at most
    assert torch.equal(P["out"].double(), P["out64"]) and torch.equal(P["dx"].double(), P["dx64"])
    assert bf16_exact(P["out64"]) and bf16_exact(P["dx64"])
    assert P["x"].shape[3] == shape[3] * VEC[pname]


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("nvec", ACT_BWD_NVEC)
def test_act_bwd_classes_meet_every_lane(nvec, pname):
    seen = torch.zeros(VEC[pname], len(Z_CLASSES), dtype=torch.bool)
    for rot in act_bwd_rotations(nvec):
        P = act_bwd_problem(nvec, pname, rot)
        assert P["dz"].double().abs().max() <= 127 and torch.equal(P["dz"].double(), P["dz"].double().round())
        for e in range(VEC[pname]):
            seen[e, P["cls"][:, e].unique()] = True
        zb = P["z"].view(int_dtype(pname))
        assert torch.equal(zb[P["cls"] == 2] != 0, torch.ones_like(zb[P["cls"] == 2], dtype=torch.bool))      # -0.0 kept its sign bit
        assert not zb[P["cls"] == 3].any()
        for act in (ACT_NONE, ACT_RELU, ACT_LRELU):
            assert act_bwd_ref(P, act, pname).shape == P["dz"].shape
    assert seen.all()
    P = act_bwd_problem(6, "f32")
    r = act_bwd_ref(P, ACT_LRELU, "f32")
    zero = (P["cls"] == 2) | (P["cls"] == 3)
    assert torch.equal(r[zero], P["dz"][zero])                        # the kernel's convention: slope 1 at z = +-0 (torch takes 0.2)
    assert torch.equal(act_bwd_ref(P, ACT_RELU, "f32")[zero].abs(), torch.zeros(int(zero.sum())))


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", IMG_SHAPES, ids=str)
def test_affine_img_data_is_dyadic_and_off_the_kink(shape, pname):
    P = img_problem(shape, pname)
    x = P["x"].double()
    assert x.abs().max() <= 8 and torch.equal(x, x.round())
    assert set(P["A"].unique().tolist()) <= set(IMG_A) and set(P["B"].unique().tolist()) <= set(IMG_B)
    assert (P["pre64"] != 0).all()
    for slope in IMG_SLOPES:
        assert bf16_exact(act64(P["pre64"], slope))
    if shape[0] >= 2 and shape[2] * VEC[pname] >= 8:
        assert not torch.equal(P["A"][0], P["A"][1]) and not torch.equal(P["B"][0], P["B"][1])     # image 1 has its own row


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", COMPOSE_SHAPES[:3], ids=str)
def test_compose_saturation_values_are_planted_in_every_image(shape, pname):
    P = compose_problem(shape, pname)
    raw4 = P["raw4"].reshape(shape[0], -1, 4)
    if raw4.shape[1] >= 7:
        for n in range(shape[0]):
            assert set(SAT3) <= set(raw4[n, :, 3].tolist())
            for c in range(3):
                assert set(SAT012) <= set(raw4[n, :, c].tolist())
    R = P["f64"]
    assert all(torch.isfinite(t).all() for t in (R["out"], R["prob"], R["both"][0], R["both"][1]))
    raw = compose_raw(P, 2 * VEC[pname], pname, PAD_FILL)
    assert torch.isfinite(raw.float()).all() and (raw[..., 4:].float().abs() > 1e4).all()
    assert torch.equal(raw[..., :4].float(), P["raw4"])


@pytest.mark.parametrize("pname", DTYPES)
def test_nan_guard_data_and_reference(pname):
    bit = lambda t: int(t.view(int_dtype(pname)).item()) & (0xFFFF if pname == "bf16" else 0xFFFFFFFF)      # noqa: E731
    sign = 0x8000 if pname == "bf16" else 0x80000000
    for nvec, placement in NAN_CASES + [(n, None) for n in NAN_CLEAN_NVEC]:
        if nvec == BIG_NVEC and placement not in ("second_trip", None):
            continue
        x, want = nan_guard_data(nvec, pname, placement)
        xb, wb = x.view(int_dtype(pname)), want.view(int_dtype(pname))
        assert int(x.isnan().sum()) == (0 if placement is None else 1)
        assert bool(x.isinf().any())
        if placement is None:
            assert torch.equal(xb, wb)                                # infinities without a NaN stay
            continue
        pos = nan_position(nvec, placement, pname)
        assert 0 <= pos < x.numel() and bit(want[pos]) == 0
        if placement == "negative_payload":
            assert bit(x[pos]) == NEG_NAN_BITS[pname]
        if placement == "second_trip":
            assert pos // VEC[pname] >= EW_CAP * THREADS
        if placement in ("thread63", "thread255"):
            assert pos // VEC[pname] == int(placement[6:])
        if placement == "last_lane":
            assert pos % VEC[pname] == VEC[pname] - 1
        pinf, ninf = x == float("inf"), x == float("-inf")
        assert pinf.any() and ninf.any()
        assert all(v & (sign * 2 - 1) == DT_MAX_BITS[pname] for v in wb[pinf].tolist())
        assert all(v & (sign * 2 - 1) == DT_MAX_BITS[pname] | sign for v in wb[ninf].tolist())
        other = ~(pinf | ninf | x.isnan())
        assert torch.equal(xb[other], wb[other])
        if x.numel() >= 16:
            vals = [v & (sign * 2 - 1) for v in wb.tolist()] if x.numel() < 5000 else None
            if vals is not None:
                assert sign in vals and SUBNORMAL_BITS[pname] in vals          # -0.0 and the subnormal pass through


def test_geometry_tables_hold_every_category():
    for chw, hole in GEO_SHAPES:
        names = [n for _, _, ns, _ in geo_tables(chw, hole) for n in ns]
        assert set(names) == set(GEO_CATEGORIES)
    (C, H, W), hole = GEO_SHAPES[0]
    assert hole == (6, 6) and W % 4 == 0
    ch, cw, names, rec = geo_tables((C, H, W), hole)[0]
    x = torch.ones(len(names), 1, H, W, dtype=torch.float64)
    y = diffaug_ref(x, rec, ch, cw, 1)
    kept = {n: int(y[i].sum()) for i, n in enumerate(names)}
    assert kept["identity"] == H * W and kept["ty=H"] == 0 and kept["tx=-W"] == 0
    assert kept["tx+4"] == H * (W - 4) and kept["tx+6"] == H * (W - 6) and kept["ty+(H-1)"] == W == kept["ty-(H-1)"]
    assert kept["hole_inside"] == H * W - ch * cw
    for n in ("hole_top<0", "hole_left<0", "hole_bottom>H", "hole_right>W"):       # clipped by its border, not gone
        assert H * W - ch * cw < kept[n] < H * W
    i = names.index("hole_inside")
    left = int(rec[i, 7])
    assert left % 4 == 1 and (left + cw) % 4 != 0 and int(rec[i, 6]) > 0 and int(rec[i, 6]) + ch < H and left + cw < W
    i = names.index("translation+hole")
    ty, tx, top, _ = (int(v) for v in rec[i, 4:])
    assert top + ch > H - ty and tx < 0                               # the hole reaches into the band the translation vacates
    ch2, cw2, names2, rec2 = geo_tables((C, H, W), hole)[1]
    assert ch2 >= H and cw2 >= W and not diffaug_ref(x[:2], rec2, ch2, cw2, 1)[0].any()
    ch3, cw3, _, rec3 = geo_tables((C, H, W), hole)[2]
    assert (ch3, cw3) == (0, 0) and torch.equal(diffaug_ref(x[:1], rec3[:1], 0, 0, 1), x[:1])


def test_color_records_reach_the_corners_and_the_mean_term():
    ch, cw, rec = color_records(81, 4, COLOR_W)
    f, geo = rec_fields(rec)
    assert len({tuple(r) for r in f.tolist()}) == 27 and len(set(geo)) == 3
    assert len({(tuple(r), g) for r, g in zip(f.tolist(), geo)}) == 81
    assert set(f[:, 2].tolist()) == {-0.5, 0.0, 0.5} and set(f[:, 3].tolist()) == {-0.5, 0.0, 0.5}
    for first in range(3):
        f1, _ = rec_fields(color_records(1, 64, COLOR_W, first)[2])
        assert abs(float(f1[0, 2])) == 0.5
    # mode 2: where the adjoint's source is masked the output is k M, M the mean of the masked cotangent
    n, c, h, w = 6, 3, 4, COLOR_W
    g = color_image(n, c, h, w, 9).double()
    ch, cw, rec = color_records(n, h, w)
    f, geo = rec_fields(rec)
    gx = diffaug_ref(g, rec, ch, cw, 2, g)
    ident = records([(1.0, 0.0, 0.0, 0.0) + t for t in geo])
    hh = diffaug_ref(g, ident, ch, cw, 2, g)
    reach = diffaug_ref(g, ident, ch, cw, 2, torch.ones_like(g))
    M = hh.mean(dim=(1, 2, 3), keepdim=True)
    want = (f[:, 2].double().view(-1, 1, 1, 1) * M).expand_as(gx)
    assert (reach == 0).any() and float((gx - want)[reach == 0].abs().max()) < 1e-15


def test_diffaug_reference_equals_the_oracle():
    """The float64 reference against oracle.diff_augment from the same seed at (3, 3, 12, 16), "color,translation,cutout".

    The oracle multiplies by the fp32 draws kc and ks one after the other in float64; a record holds a = kc ks and b = kc (1 - ks)
    rounded to fp32 (k and beta are exact in fp32).  So the reference is held to 1e-12 with a and b taken before that rounding, from
    the same draws, and the record is held to them bit for bit: float32(a) and float32(b) ARE the record's, everything else in
    the record is used as it stands.  Fed the record's own a and b the reference is one fp32 rounding of each away: within
    2^-24 (|a x| + |b mean_c x|), asserted as well."""
    from de_i2i_gan_amd.utils import diffaug as DA
    n, c, h, w = 3, 3, 12, 16
    policy = "color,translation,cutout"
    x = torch.rand(n, c, h, w, generator=gen(1)).double()
    for seed in (21, 22, 23):
        torch.manual_seed(seed)
        want = O.diff_augment(x, policy)
        torch.manual_seed(seed)
        rec, meta = DA.draw_params(policy, n, h, w)
        assert rec.shape == (1, n, DA.REC_FIELDS) and len(meta) == 1 and meta[0][0]
        _, ch, cw = meta[0]
        torch.manual_seed(seed)
        rb, rs, rc = (torch.rand(n, 1, 1, 1).view(n) for _ in range(3))           # draw_params' first three draws
        ks, kc = (rs * 2).double(), (rc + 0.5).double()
        coef = torch.stack([kc * ks, kc * (1 - ks), 1 - kc, (rb - 0.5).double()], dim=1)
        f, _ = rec_fields(rec[0])
        assert torch.equal(coef.float(), f)                           # the record is these coefficients, rounded once
        assert torch.equal(coef[:, 2:].float().double(), coef[:, 2:])
        got = diffaug_ref(x, rec[0], ch, cw, 0, coef=coef)
        assert float((got - want).abs().max()) <= 1e-12
        plain = diffaug_ref(x, rec[0], ch, cw, 0)
        a, b = f[:, 0].double().abs().view(-1, 1, 1, 1), f[:, 1].double().abs().view(-1, 1, 1, 1)
        room = 2.0 ** -24 * (a * x.abs().amax(dim=(1, 2, 3), keepdim=True) + b * x.mean(dim=1, keepdim=True).abs().amax(dim=(1, 2, 3), keepdim=True))
        assert ((plain - want).abs() <= room + 1e-15).all()
