"""numpy reference of the pixel-blitting DiffAugment policies (flip -> rot90; csrc/blit.hip, include/dei2i_hip.h): the index maps
of the eight codes f | k << 1 written out per pixel, the inverse codes, the run split and the device draw words."""
import numpy as np

from embed_reference import philox4x32_10

CANONICAL = ("color", "translation", "cutout")
BLIT_CANONICAL = ("flip", "rot90")
BLIT_STREAM = 3          # the block number of the blit draw in the counter word run | block << 16


def source_index(code, i, j, h, w):
    """the source pixel of output pixel (i, j) under code = f | k << 1: flip first, then k quarter turns (S = h = w for k != 0)"""
    f, k = code & 1, code >> 1
    s = h
    si, sj = ((i, j), (j, s - 1 - i), (s - 1 - i, s - 1 - j), (s - 1 - j, i))[k]      # in the flipped image
    return si, (w - 1 - sj if f else sj)


def blit(x, codes):
    """x (n, c, h, w), codes (n,) -> the blitted batch, pixel by pixel"""
    x = np.asarray(x)
    out = np.empty_like(x)
    n, _, h, w = x.shape
    for b in range(n):
        for i in range(h):
            for j in range(w):
                si, sj = source_index(int(codes[b]), i, j, h, w)
                out[b, :, i, j] = x[b, :, si, sj]
    return out


def inverse_code(code):
    f, k = code & 1, code >> 1
    return code if f else ((4 - k) & 3) << 1


def policy_runs(policy):
    """maximal canonical-order runs; a blit run and a run of the other kind are never merged"""
    runs = []
    for name in policy.split(",") if policy else []:
        order = BLIT_CANONICAL if name in BLIT_CANONICAL else CANONICAL
        if runs and runs[-1][-1] in order and order.index(name) > order.index(runs[-1][-1]):
            runs[-1].append(name)
        else:
            runs.append([name])
    return runs


def _unit(x):
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def draw_words(seed, call, run, n, row0):
    key = (seed & 0xFFFFFFFF, seed >> 32)
    rows = np.arange(row0, row0 + n, dtype=np.uint64)
    return philox4x32_10((call & 0xFFFFFFFF, call >> 32, run | BLIT_STREAM << 16, rows), key)


def draw_codes(seed, call, policy, n, row0, p=None):
    """-> int32 (blit runs, n): f = x0 >> 31, k = mulhi(x1, 4) of the block (call, run | 3 << 16, row0 + i), run the index in the
    whole run list; with ``p`` (a float32) flip applies iff unit(x2) < p and rot90 iff unit(x3) < p"""
    rows = []
    for run, names in enumerate(policy_runs(policy)):
        if names[0] not in BLIT_CANONICAL:
            continue
        x = draw_words(seed, call, run, n, row0)
        f = (x[0] >> np.uint32(31)).astype(np.int32) if "flip" in names else np.zeros(n, np.int32)
        k = ((x[1].astype(np.uint64) * np.uint64(4)) >> np.uint64(32)).astype(np.int32) if "rot90" in names else np.zeros(n, np.int32)
        if p is not None:
            f = np.where(_unit(x[2]) < np.float32(p), f, 0)
            k = np.where(_unit(x[3]) < np.float32(p), k, 0)
        rows.append((f | k << 1).astype(np.int32))
    return np.stack(rows)


def gates(seed, call, policy, n, row0, p):
    """-> bool (blit runs, n, 2): whether the flip / the rot90 gate of a row passes at ``p``"""
    out = []
    for run, names in enumerate(policy_runs(policy)):
        if names[0] in BLIT_CANONICAL:
            x = draw_words(seed, call, run, n, row0)
            out.append(np.stack([_unit(x[2]) < np.float32(p), _unit(x[3]) < np.float32(p)], axis=1))
    return np.stack(out)
