"""numpy reference of the geometric DiffAugment policies (scale -> rotate -> aniso; csrc/warp.hip, include/dei2i_hip.h): the bilinear
resampling and its adjoint in fp32, op for op with the kernel's association, tap order and summation order; the usable gate; the run
split; the Philox words of the device draw and a float64 matrix built from them."""
import numpy as np

from embed_reference import philox4x32_10

CANONICAL = ("color", "translation", "cutout")
BLIT_CANONICAL = ("flip", "rot90")
WARP_CANONICAL = ("scale", "rotate", "aniso")
PARAM_BLOCK, GATE_BLOCK = 4, 5          # the block numbers of the warp draw in the counter word run | block << 16
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
F = np.float32


def usable(rec):
    """-> bool (n,): six finite floats, |m| <= 4, det != 0 and |m| <= 4 |det| (det in float64: exact products, one rounding)"""
    r = np.asarray(rec, dtype=F).reshape(len(rec), -1)[:, :6].astype(np.float64)
    with np.errstate(all="ignore"):
        det = r[:, 0] * r[:, 3] - r[:, 1] * r[:, 2]
        big = np.abs(r[:, :4]).max(axis=1)
        return np.isfinite(r).all(axis=1) & (big <= 4.0) & (det != 0) & (big <= 4.0 * np.abs(det))


def effective(rec):
    """the (n, 6) fp32 table a launch applies: rows that are not usable replaced by the identity"""
    rec = np.array(np.asarray(rec, dtype=F).reshape(len(rec), -1)[:, :6])
    rec[~usable(rec)] = IDENTITY
    return rec


def taps(row, h, w):
    """one record -> (valid (h, w) bool, u0, v0 (h, w) int64, the four (h, w) fp32 weights), every step a separate fp32 operation"""
    m00, m01, m10, m11, tu, tv = (F(v) for v in row)
    cx, cy = F(w - 1) * F(0.5), F(h - 1) * F(0.5)
    dx = np.arange(w, dtype=F).reshape(1, w) - cx
    dy = np.arange(h, dtype=F).reshape(h, 1) - cy
    with np.errstate(all="ignore"):
        u = (m00 * dx + m01 * dy) + (cx + tu)
        v = (m10 * dx + m11 * dy) + (cy + tv)
        assert u.dtype == F and v.dtype == F
        valid = (u >= F(-1)) & (u < F(w)) & (v >= F(-1)) & (v < F(h))          # (NaN fails every comparison)
        u, v = np.where(valid, u, F(0)), np.where(valid, v, F(0))
        u0, v0 = np.floor(u), np.floor(v)
        fu, fv = u - u0, v - v0
        weights = ((F(1) - fv) * (F(1) - fu), (F(1) - fv) * fu, fv * (F(1) - fu), fv * fu)
    assert all(wt.dtype == F for wt in weights)
    return valid, u0.astype(np.int64), v0.astype(np.int64), weights


def forward(x, rec):
    """x (n, c, h, w) fp32, rec (n, >= 6) -> ((t0 + t1) + t2) + t3 per pixel, t = weight * tap or 0 for a tap outside the image"""
    x = np.asarray(x, dtype=F)
    n, _, h, w = x.shape
    out = np.zeros_like(x)
    for b, row in enumerate(effective(rec)):
        valid, u0, v0, weights = taps(row, h, w)
        total = None
        for (a, d), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
            rr, cc = v0 + a, u0 + d
            inside = valid & (rr >= 0) & (rr < h) & (cc >= 0) & (cc < w)
            with np.errstate(all="ignore"):
                term = np.where(inside, wt * x[b][:, rr.clip(0, h - 1), cc.clip(0, w - 1)], F(0))
            total = term if total is None else total + term
        out[b] = total
    return out


def adjoint(g, rec):
    """the transpose of ``forward`` with the same weights: every output pixel (i, j), in ascending row-major order, adds
    weight * g[i][j] to each of its taps inside the image (one output pixel reaches one input pixel through at most one tap, so per
    input pixel this is the kernel's sum order), starting from 0"""
    g = np.asarray(g, dtype=F)
    n, _, h, w = g.shape
    out = np.zeros_like(g)
    for b, row in enumerate(effective(rec)):
        valid, u0, v0, weights = taps(row, h, w)
        for i in range(h):
            for j in range(w):
                if not valid[i, j]:
                    continue
                for (a, d), wt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
                    y, x = v0[i, j] + a, u0[i, j] + d
                    if 0 <= y < h and 0 <= x < w:
                        with np.errstate(all="ignore"):
                            out[b, :, y, x] = out[b, :, y, x] + wt[i, j] * g[b, :, i, j]
    return out


def policy_runs(policy):
    """maximal canonical-order runs; runs of different kinds are never merged"""
    runs = []
    for name in policy.split(",") if policy else []:
        order = next(o for o in (BLIT_CANONICAL, WARP_CANONICAL, CANONICAL) if name in o)
        if runs and runs[-1][-1] in order and order.index(name) > order.index(runs[-1][-1]):
            runs[-1].append(name)
        else:
            runs.append([name])
    return runs


def _unit(x):
    return (x >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def draw_words(seed, call, run, n, row0, block):
    key = (seed & 0xFFFFFFFF, seed >> 32)
    rows = np.arange(row0, row0 + n, dtype=np.uint64)
    return philox4x32_10((call & 0xFFFFFFFF, call >> 32, run | block << 16, rows), key)


def warp_runs(policy):
    """[(index in the whole run list, names)] of the warp runs"""
    return [(run, names) for run, names in enumerate(policy_runs(policy)) if names[0] in WARP_CANONICAL]


def gates(seed, call, policy, n, row0, p):
    """-> bool (warp runs, n, 3): whether the scale / rotate / aniso gate of a row passes at ``p`` (block 5: x0, x1, x2)"""
    out = []
    for run, _ in warp_runs(policy):
        x = draw_words(seed, call, run, n, row0, GATE_BLOCK)
        out.append(np.stack([_unit(x[k]) < F(p) for k in range(3)], axis=1))
    return np.stack(out)


def matrix64(seed, call, policy, n, row0, p=None):
    """-> float64 (warp runs, n, 4): m00, m01, m10, m11 from the block-4 words.  The ARGUMENTS of exp2, sin and cos are formed in fp32
    exactly as the device forms them (r - 0.5 and 2 r - 1 are exact; (2 r - 1) * (float)pi is one fp32 multiply); the functions and
    the products are float64, so what separates the device table from this one is the error of exp2f, sinf, cosf and the rounding
    of the entry formulas' fp32 multiplies and divides."""
    out = []
    for b, (run, names) in enumerate(warp_runs(policy)):
        x = draw_words(seed, call, run, n, row0, PARAM_BLOCK)
        on = np.array([[name in names for name in WARP_CANONICAL]] * n)
        if p is not None:
            on &= gates(seed, call, policy, n, row0, p)[b]
        rs, rt, rl = (_unit(x[k]) for k in range(3))
        theta = ((F(2) * rt - F(1)) * F(np.pi)).astype(np.float64)
        s = np.where(on[:, 0], np.exp2((rs - F(0.5)).astype(np.float64)), 1.0)
        c, sn = np.where(on[:, 1], np.cos(theta), 1.0), np.where(on[:, 1], np.sin(theta), 0.0)
        lam = np.where(on[:, 2], np.exp2((rl - F(0.5)).astype(np.float64)), 1.0)
        out.append(np.stack([lam * (c * s), lam * (-(sn * s)), (sn * s) / lam, (c * s) / lam], axis=1))
    return np.stack(out)
