"""DiffAugment (Zhao et al. 2020, "Differentiable Augmentation for Data-Efficient GAN Training") as the reference applies it
to the images the discriminator sees (utils/diffaug.py:9-76; call sites defectgan_model.py:200-203,266-270): policies
'color' (brightness, saturation, contrast), 'translation' (random shift by up to 1/8 of the side, zero fill) and 'cutout'
(a random half-size square set to zero), all differentiable w.r.t. the image.  Beyond the reference: 'flip' (mirror left-right)
and 'rot90' (quarter turns), the pixel-blitting augmentations of Karras et al. 2020 that the integer translation lacked -- per
sample one permutation of the pixels (csrc/blit.hip), in runs of their own (``policy_runs``) -- and 'scale', 'rotate' and 'aniso',
their geometric group: per sample one 2x2 matrix, applied as ONE bilinear resampling per run (``warp``, csrc/warp.hip).

NCHW fp32 images.  The policy functions below are plain torch ops and define the semantics (the defectGAN model calls
them); ``ops.diff_augment`` is the same map as fused HIP kernels (csrc/diffaug.hip), differentiable to any order, whose
host half is ``draw_params``.  The per-sample random numbers are drawn with the global torch RNG ON THE HOST in the
reference's order -- a run seeded like the reference's CPU path sees the reference's augmentations -- and uploaded (a few
values per sample).

``opt.diff_aug_rng = "device"`` (opt-in) takes neither half: the defectGAN model then calls ``ops.diff_augment(x, policy,
rng=ops.DiffAugRng)``, whose table is filled on the device by a counter-based generator with the formulas of ``draw_params``
(csrc/diffaug.hip dei2i_diffaug_draw) -- the same distributions, not the reference's draws, and nothing a graph capture would
freeze.  ``policy_runs`` serves both."""
import ctypes

import numpy as np
import torch

from .. import _lib


def _rand(n, x):
    return torch.rand(n, 1, 1, 1).to(device=x.device, dtype=x.dtype)


def _randint(lo, hi, n, x):
    return torch.randint(lo, hi, size=[n, 1, 1]).to(x.device)


def brightness(x):
    return x + (_rand(x.size(0), x) - 0.5)


def saturation(x):
    mean = x.mean(dim=1, keepdim=True)
    return (x - mean) * (_rand(x.size(0), x) * 2) + mean


def contrast(x):
    mean = x.mean(dim=[1, 2, 3], keepdim=True)
    return (x - mean) * (_rand(x.size(0), x) + 0.5) + mean


def translation(x, ratio=0.125):
    """out[n, :, i, j] = x[n, :, i + ty_n, j + tx_n] (zero outside), one integer shift pair per sample."""
    n, _, h, w = x.shape
    max_y, max_x = int(h * ratio + 0.5), int(w * ratio + 0.5)
    ty = _randint(-max_y, max_y + 1, n, x)
    tx = _randint(-max_x, max_x + 1, n, x)
    rows = torch.arange(h, device=x.device).view(1, h, 1) + ty          # source row of every output row, per sample
    cols = torch.arange(w, device=x.device).view(1, 1, w) + tx
    inside = ((rows >= 0) & (rows < h) & (cols >= 0) & (cols < w)).unsqueeze(1).to(x.dtype)
    rows, cols = rows.clamp(0, h - 1), cols.clamp(0, w - 1)
    batch = torch.arange(n, device=x.device).view(n, 1, 1)
    gathered = x.permute(0, 2, 3, 1)[batch, rows, cols]                   # (n, h, w, c)
    return gathered.permute(0, 3, 1, 2) * inside


def cutout(x, ratio=0.5):
    """zero a (ratio*h) x (ratio*w) window centred at a random pixel (the part of it inside the image)"""
    n, _, h, w = x.shape
    ch, cw = int(h * ratio + 0.5), int(w * ratio + 0.5)
    cy = _randint(0, h + (1 - ch % 2), n, x)
    cx = _randint(0, w + (1 - cw % 2), n, x)
    rows = torch.arange(h, device=x.device).view(1, h, 1)
    cols = torch.arange(w, device=x.device).view(1, 1, w)
    top, left = cy - ch // 2, cx - cw // 2
    hole = (rows >= top) & (rows < top + ch) & (cols >= left) & (cols < left + cw)
    return x * (~hole).unsqueeze(1).to(x.dtype)


def flip(x):
    """mirror a sample left-right when its bit is 1 (the x-flip of Karras et al. 2020, one of the pixel-blitting augmentations)"""
    f = _randint(0, 2, x.size(0), x)
    return torch.where(f.unsqueeze(1) == 1, x.flip(3), x)


def rot90(x):
    """k quarter turns per sample, k uniform in {0, 1, 2, 3}: torch.rot90(x[i], k_i, dims=(1, 2)); square images only"""
    k = torch.randint(0, 4, size=[x.size(0), 1, 1]).view(-1).tolist()          # (drawn on the host, as _randint draws)
    return torch.stack([torch.rot90(x[i], k[i], dims=(1, 2)) for i in range(x.size(0))])


# ---- the geometric group (Karras et al. 2020): isotropic scaling, rotation by any angle, anisotropic scaling ----------------------
# One record per sample, the six floats of a dei2i_warp table row (include/dei2i_hip.h): the 2x2 matrix M = A R S that takes an OUTPUT
# pixel to the INPUT position it samples, about the image centre, and a shift (tu, tv) that every draw leaves 0.
#   S = s I, s = 2^(r_s - 0.5);  R = rotation by (2 r_t - 1) pi;  A = diag(l, 1/l), l = 2^(r_l - 0.5);  each r uniform in [0, 1).
# Both singular values of M lie in [1/2, 2] (bounded on purpose -- Karras et al. draw log-normal scales -- so that the adjoint's
# search box has a fixed size, csrc/warp.hip), and the distributions are symmetric under inversion, so drawing the sampling matrix
# is drawing the image transform.
WARP_MAX = 4.0          # the usable gate: every entry of M and of its inverse is at most this in magnitude


def warp_usable(rec):
    """-> bool (n,): which rows of an (n, >= 6) fp32 record table the warp applies; the others are applied as the identity.  A row
    is usable when its six floats are finite, |m| <= 4 for the four matrix entries, and det != 0 and |m| <= 4 |det| for each of them
    (every entry of the inverse is at most 4), det = m00 m11 - m01 m10 in float64 (each product exact, one rounding)."""
    r = np.asarray(rec, dtype=np.float32).reshape(len(rec), -1)[:, :6].astype(np.float64)
    with np.errstate(all="ignore"):
        det = r[:, 0] * r[:, 3] - r[:, 1] * r[:, 2]
        big = np.abs(r[:, :4]).max(axis=1)
        return np.isfinite(r).all(axis=1) & (big <= WARP_MAX) & (det != 0) & (big <= WARP_MAX * np.abs(det))


def warp(x, rec):
    """One bilinear resampling of an (n, c, h, w) fp32 batch, per sample the record rec[k] = (m00, m01, m10, m11, tu, tv) (an
    (n, >= 6) fp32 host table): with cx = (w - 1) / 2, cy = (h - 1) / 2, output pixel (i, j) samples the input at
        u = (m00 (j - cx) + m01 (i - cy)) + (cx + tu),   v = (m10 (j - cx) + m11 (i - cy)) + (cy + tv)
    -- separate fp32 operations in this association -- as ((t0 + t1) + t2) + t3 over the taps (v0, u0), (v0, u0 + 1), (v0 + 1, u0),
    (v0 + 1, u0 + 1), u0 = floor(u), v0 = floor(v), with the weights (1 - fv)(1 - fu), (1 - fv) fu, fv (1 - fu), fv fu; a tap outside
    the image is 0 (zero fill, as ``translation``), and so is the pixel when u or v is not finite or lies outside [-1, w) x [-1, h).
    A row that is not ``warp_usable`` is applied as the identity.  Pixel coordinates, not F.grid_sample's normalised ones (they
    round differently); differentiable in x to any order (the map is linear); csrc/warp.hip is the same map bit for bit."""
    n, _, h, w = x.shape
    rec = np.array(np.asarray(rec, dtype=np.float32).reshape(n, -1)[:, :6])
    rec[~warp_usable(rec)] = (1, 0, 0, 1, 0, 0)
    m00, m01, m10, m11, tu, tv = (torch.from_numpy(rec[:, k].copy()).to(x.device).view(n, 1, 1) for k in range(6))
    cx, cy = (w - 1) / 2, (h - 1) / 2
    dx = torch.arange(w, dtype=torch.float32, device=x.device).view(1, 1, w) - cx
    dy = torch.arange(h, dtype=torch.float32, device=x.device).view(1, h, 1) - cy
    u = (m00 * dx + m01 * dy) + (cx + tu)
    v = (m10 * dx + m11 * dy) + (cy + tv)
    valid = torch.isfinite(u) & torch.isfinite(v) & (u >= -1) & (u < w) & (v >= -1) & (v < h)
    u0, v0 = torch.floor(u), torch.floor(v)
    fu, fv = u - u0, v - v0
    col, row = torch.where(valid, u0, 0).long(), torch.where(valid, v0, 0).long()
    batch = torch.arange(n, device=x.device).view(n, 1, 1)
    pixels = x.permute(0, 2, 3, 1)
    out = None
    for a, b, weight in ((0, 0, (1 - fv) * (1 - fu)), (0, 1, (1 - fv) * fu), (1, 0, fv * (1 - fu)), (1, 1, fv * fu)):
        rr, cc = row + a, col + b
        inside = valid & (rr >= 0) & (rr < h) & (cc >= 0) & (cc < w)
        tap = pixels[batch, rr.clamp(0, h - 1), cc.clamp(0, w - 1)]          # (n, h, w, c)
        term = torch.where(inside.unsqueeze(3), weight.unsqueeze(3) * tap, torch.zeros((), dtype=x.dtype, device=x.device))
        out = term if out is None else out + term
    return out.permute(0, 3, 1, 2).contiguous()


def warp_records(names, n):
    """Draw the records of one warp run: one (n, 1, 1, 1) uniform per policy of ``names`` in list order from the global CPU RNG,
    the matrix in torch fp32 ops; an absent policy contributes its identity exactly.  -> fp32 numpy (n, 8), the last two words 0."""
    one, zero = torch.ones(n), torch.zeros(n)
    s, c, sn, lam = one, one, zero, one
    for name in names:
        r = torch.rand(n, 1, 1, 1).view(n)
        if name == "scale":
            s = torch.exp2(r - 0.5)
        elif name == "rotate":
            theta = (2 * r - 1) * np.pi
            c, sn = torch.cos(theta), torch.sin(theta)
        else:
            lam = torch.exp2(r - 0.5)
    cs, ss = c * s, sn * s
    rec = np.zeros((n, REC_FIELDS), dtype=np.float32)
    for k, entry in enumerate((lam * cs, lam * (-ss), ss / lam, cs / lam)):
        rec[:, k] = entry.numpy()
    return rec


def scale(x):
    """isotropic scaling by 2^(r - 0.5) about the centre, bilinear, zero fill"""
    return warp(x, warp_records(["scale"], x.size(0)))


def rotate(x):
    """rotation by (2 r - 1) pi about the centre, bilinear, zero fill"""
    return warp(x, warp_records(["rotate"], x.size(0)))


def aniso(x):
    """anisotropic scaling diag(l, 1 / l), l = 2^(r - 0.5), about the centre, bilinear, zero fill"""
    return warp(x, warp_records(["aniso"], x.size(0)))


POLICIES = {"color": (brightness, saturation, contrast), "translation": (translation,), "cutout": (cutout,), "flip": (flip,),
            "rot90": (rot90,), "scale": (scale,), "rotate": (rotate,), "aniso": (aniso,)}


def check_policy(policy, h, w):
    """-> the names of ``policy``; an unknown name raises KeyError and rot90 on a non-square image ValueError, before anything is
    drawn"""
    names = policy.split(",") if policy else []
    for name in names:
        if name not in POLICIES:
            raise KeyError(f"DiffAugment policy [{name}] is not defined (color | translation | cutout | flip | rot90 | scale | rotate "
                           "| aniso)")
    if "rot90" in names and h != w:
        raise ValueError(f"DiffAugment policy [rot90] needs square images; these are {h} x {w}")
    return names


def diff_augment(x, policy=""):
    if not policy:
        return x
    check_policy(policy, x.size(2), x.size(3))
    for names in policy_runs(policy):
        if is_warp_run(names):          # one resampling with the product matrix, not one per name
            x = warp(x, warp_records(names, x.size(0)))
            continue
        for name in names:
            for fn in POLICIES[name]:
                x = fn(x)
    return x.contiguous()


# ---- host half of the fused HIP op (ops.diff_augment, csrc/diffaug.hip) ----------------------------------------------------------
CANONICAL = ("color", "translation", "cutout")
BLIT_CANONICAL = ("flip", "rot90")          # the pixel-blitting policies: runs of their own kind (csrc/blit.hip), one code per sample
WARP_CANONICAL = ("scale", "rotate", "aniso")          # the geometric policies: runs of a third kind (csrc/warp.hip), one matrix per sample
REC_FIELDS = ctypes.sizeof(_lib.DiffAugRec) // 4       # 32-bit words of a dei2i_diffaug_rec: a, b, k, beta (fp32), ty, tx, top, left (int32)
BLIT = "blit"           # the entry of a blit run in the run list of draw_params / ops.diffaug_draw
WARP = "warp"           # the entry of a warp run


def is_blit_run(names):
    return names[0] in BLIT_CANONICAL


def is_warp_run(names):
    return names[0] in WARP_CANONICAL


def policy_runs(policy):
    """the policy list split into maximal runs in canonical order (color -> translation -> cutout, flip -> rot90, or scale ->
    rotate -> aniso: a run is never merged with a run of another kind), each launched as one operator; an unknown name raises KeyError before anything is
    drawn"""
    names = check_policy(policy, 0, 0)
    runs = []
    for name in names:
        order = BLIT_CANONICAL if name in BLIT_CANONICAL else WARP_CANONICAL if name in WARP_CANONICAL else CANONICAL
        if runs and runs[-1][-1] in order and order.index(name) > order.index(runs[-1][-1]):
            runs[-1].append(name)
        else:
            runs.append([name])
    return runs


def draw_params(policy, n, h, w, shard=None):
    """Draw the per-sample parameters of ``policy`` for an (n, *, h, w) batch from the global CPU torch RNG, in the order and shapes
    of the policy functions above (one (n,1,1,1) float draw per color function, two (n,1,1) integer draws per translation / cutout).
    Returns (records, runs): records an int32 (len(runs), n, 8) array of struct dei2i_diffaug_rec (the four floats stored bitwise),
    runs a list of (has_color, cut_h, cut_w) -- cut_h = cut_w = 0 when the run has no cutout.  A blit run (flip -> rot90) draws one
    (n,1,1) integer per policy; its entry in runs is ``BLIT`` and its records hold the code f | k << 1 of csrc/blit.hip in word 0,
    zeros elsewhere.  A warp run (scale -> rotate -> aniso) draws one (n,1,1,1) float per policy; its entry is ``WARP`` and its
    records hold the rows of dei2i_warp's table (six floats stored bitwise, two zero words).  rot90 on a non-square image raises ValueError before anything is drawn.

    ``shard=(rank, world)``: n is one rank's share of a global batch of n * world rows.  The parameters of the whole global batch are
    drawn, exactly as the unsharded call for n * world draws them (same RNG consumption), and rows [rank * n, (rank + 1) * n) are
    returned: ranks that hold the same RNG state see the augmentation one process would apply to the global batch."""
    if shard is not None:
        rank, world = shard
        rec, meta = draw_params(policy, n * world, h, w)
        return np.ascontiguousarray(rec[:, rank * n:(rank + 1) * n]), meta
    check_policy(policy, h, w)
    runs = policy_runs(policy)
    rec = np.zeros((len(runs), n, REC_FIELDS), dtype=np.int32)
    f = rec.view(np.float32)
    meta = []
    for r, names in enumerate(runs):
        if is_blit_run(names):
            for name in names:
                draw = torch.randint(0, 2 if name == "flip" else 4, size=[n, 1, 1]).view(n).numpy().astype(np.int32)
                rec[r, :, 0] |= draw if name == "flip" else draw << 1
            meta.append(BLIT)
            continue
        if is_warp_run(names):
            f[r] = warp_records(names, n)
            meta.append(WARP)
            continue
        f[r, :, 0] = 1.0
        ch = cw = 0
        for name in names:
            if name == "color":
                rb, rs, rc = (torch.rand(n, 1, 1, 1).view(n) for _ in range(3))
                ks, kc = rs * 2, rc + 0.5
                f[r, :, 0] = (kc * ks).numpy()
                f[r, :, 1] = (kc * (1 - ks)).numpy()
                f[r, :, 2] = (1 - kc).numpy()
                f[r, :, 3] = (rb - 0.5).numpy()
            elif name == "translation":
                max_y, max_x = int(h * 0.125 + 0.5), int(w * 0.125 + 0.5)
                rec[r, :, 4] = torch.randint(-max_y, max_y + 1, size=[n, 1, 1]).view(n).numpy()
                rec[r, :, 5] = torch.randint(-max_x, max_x + 1, size=[n, 1, 1]).view(n).numpy()
            else:
                ch, cw = int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)
                cy = torch.randint(0, h + (1 - ch % 2), size=[n, 1, 1]).view(n)
                cx = torch.randint(0, w + (1 - cw % 2), size=[n, 1, 1]).view(n)
                rec[r, :, 6] = (cy - ch // 2).numpy()
                rec[r, :, 7] = (cx - cw // 2).numpy()
        meta.append(("color" in names, ch, cw))
    return rec, meta
