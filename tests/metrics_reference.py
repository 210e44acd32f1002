"""float64 numpy reference of the validation metrics (csrc/metrics.hip, ops.image_metrics / clf_counts / image_scores / clf_scores):
the SSIM window, the valid-mode SSIM map of Wang et al. 2004, the per-image sums, the classifier's confusion counts and the scores
made of them.  Written from the definitions, sharing no code with the package."""
import numpy as np

WINDOW, SIGMA = 11, 1.5


def window_weights():
    """the 11 taps of the Gaussian (sigma 1.5), normalised to sum 1; the 2-D window is their outer product"""
    d = np.arange(WINDOW, dtype=np.float64) - WINDOW // 2
    g = np.exp(-d * d / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def window_mean(a):
    """(..., H, W) -> (..., H-10, W-10): the window-weighted mean at every position where the window lies inside the plane"""
    a = np.asarray(a, dtype=np.float64)
    w2 = np.outer(window_weights(), window_weights())
    h, w = a.shape[-2] - WINDOW + 1, a.shape[-1] - WINDOW + 1
    out = np.zeros(a.shape[:-2] + (h, w), dtype=np.float64)
    for i in range(WINDOW):
        for j in range(WINDOW):
            out += w2[i, j] * a[..., i:i + h, j:j + w]
    return out


def ssim_map(x, y, data_range=2.0):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = window_mean(x), window_mean(y)
    vx, vy, cxy = window_mean(x * x) - mx * mx, window_mean(y * y) - my * my, window_mean(x * y) - mx * my
    return ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def image_sums(x, y, mask=None, data_range=2.0):
    """(N,C,H,W) x 2 [, mask (N,1,H,W)] -> float64 (N, 6): sse, sae, masked sse, masked sae, masked element count, SSIM sum"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    d = x - y
    out = np.zeros((n, 6), dtype=np.float64)
    out[:, 0] = (d * d).reshape(n, -1).sum(1)
    out[:, 1] = np.abs(d).reshape(n, -1).sum(1)
    if mask is not None:
        m = np.broadcast_to(np.asarray(mask) != 0, x.shape)
        out[:, 2] = np.where(m, d * d, 0.0).reshape(n, -1).sum(1)
        out[:, 3] = np.where(m, np.abs(d), 0.0).reshape(n, -1).sum(1)
        out[:, 4] = m.reshape(n, -1).sum(1)
    out[:, 5] = ssim_map(x, y, data_range).reshape(n, -1).sum(1)
    return out


def image_scores(sums, chw, data_range=2.0):
    """-> {"psnr", "ssim", "l1", "psnr_masked"}: means over the images; psnr_masked over those with masked elements (NaN: none)"""
    c, h, w = chw
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 6)
    peak = data_range ** 2

    def psnr(mse):
        return 10.0 * np.log10(peak / np.maximum(mse, 1e-10 * peak))

    has = sums[:, 4] > 0
    return {"psnr": float(psnr(sums[:, 0] / (c * h * w)).mean()),
            "ssim": float((sums[:, 5] / (c * (h - WINDOW + 1) * (w - WINDOW + 1))).mean()),
            "l1": float((sums[:, 1] / (c * h * w)).mean()),
            "psnr_masked": float(psnr(sums[has, 2] / sums[has, 4]).mean()) if has.any() else float("nan")}


def clf_counts(logits, targets, kind):
    """(N,K) x 2 -> int64 (4K+1,): TP | FP | FN | TN per class, then the rows right in every class.  bce / mse: logit > 0 against
    target > 0.5; cce: first argmax against first argmax."""
    logits, targets = np.asarray(logits), np.asarray(targets)
    n, k = logits.shape
    if kind in ("bce", "mse"):
        pred, want = logits > 0, targets > 0.5
    elif kind == "cce":
        pred = np.eye(k, dtype=bool)[logits.argmax(1)]
        want = np.eye(k, dtype=bool)[targets.argmax(1)]
    else:
        raise ValueError(kind)
    rows = [(pred & want).sum(0), (pred & ~want).sum(0), (~pred & want).sum(0), (~pred & ~want).sum(0), [(pred == want).all(1).sum()]]
    return np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])


def clf_scores(counts):
    """-> {"acc": exact-match rate, "f1": macro F1 over the classes with any positive target (NaN: none)}"""
    counts = np.asarray(counts, dtype=np.float64)
    k = (len(counts) - 1) // 4
    tp, fp, fn, tn = counts[:4 * k].reshape(4, k)
    has = tp + fn > 0
    f1 = 2 * tp[has] / (2 * tp[has] + fp[has] + fn[has])
    return {"acc": float(counts[4 * k] / (tp[0] + fp[0] + fn[0] + tn[0])), "f1": float(f1.mean()) if has.any() else float("nan")}
