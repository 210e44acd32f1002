"""tests/metrics_reference.py against closed forms: the float64 reference the GPU tests compare csrc/metrics.hip with is itself
checked where SSIM, the sums and F1 can be written down by hand."""
import numpy as np
import pytest

import metrics_reference as R

L = 2.0
C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2


def test_weights_are_a_normalised_symmetric_gaussian():
    w = R.window_weights()
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15
    assert np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert np.allclose(w[4] / w[5], np.exp(-1 / 4.5), rtol=1e-14, atol=0)


def test_equal_images_give_ssim_one_and_no_error():
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (2, 3, 20, 17))
    s = R.image_sums(x, x)
    assert np.array_equal(s[:, :5], np.zeros((2, 5)))
    assert np.array_equal(R.ssim_map(x, x), np.ones((2, 3, 10, 7)))
    assert np.array_equal(s[:, 5], np.full(2, 3 * 10 * 7))
    got = R.image_scores(s, (3, 20, 17))
    assert got["psnr"] == pytest.approx(100.0, abs=1e-12) and got["ssim"] == 1.0 and got["l1"] == 0.0 and np.isnan(got["psnr_masked"])


@pytest.mark.parametrize("a, b", [(0.5, 0.25), (-1.0, 1.0), (0.0, 0.75), (0.0, 0.0)])
def test_constant_images(a, b):
    x, y = np.full((1, 1, 14, 13), a), np.full((1, 1, 14, 13), b)
    want = (2 * a * b + C1) / (a * a + b * b + C1)         # (the variances vanish: the second factor is C2 / C2)
    got = R.ssim_map(x, y)
    assert got.shape == (1, 1, 4, 3) and np.allclose(got, want, rtol=0, atol=1e-12)
    s = R.image_sums(x, y)[0]
    assert s[0] == pytest.approx((a - b) ** 2 * 14 * 13, rel=1e-15) and s[1] == pytest.approx(abs(a - b) * 14 * 13, rel=1e-15)


def test_impulse_changes_ssim_inside_its_footprint_only():
    h, w, i, j = 40, 37, 17, 20
    x = np.zeros((1, 1, h, w))
    x[0, 0, i, j] = 1.0
    m = R.ssim_map(x, np.zeros_like(x))[0, 0]
    rows, cols = np.nonzero(m != 1.0)
    # the window at position (r, c) covers pixels [r, r + 10] x [c, c + 10]
    assert rows.min() == i - 10 and rows.max() == i and cols.min() == j - 10 and cols.max() == j
    assert len(rows) == 121 and bool((m[i - 10:i + 1, j - 10:j + 1] < 1.0).all())


def test_masked_sums_and_scores():
    rng = np.random.default_rng(1)
    x, y = rng.uniform(-1, 1, (2, 3, 12, 12)), rng.uniform(-1, 1, (2, 3, 12, 12))
    mask = np.zeros((2, 1, 12, 12))
    mask[0, 0, :6] = 1
    s = R.image_sums(x, y, mask)
    d = (x - y)[0, :, :6]
    assert s[0, 4] == 3 * 6 * 12 and s[1, 4] == 0 and np.array_equal(s[1, 2:4], [0, 0])
    assert s[0, 2] == pytest.approx((d * d).sum(), rel=1e-14) and s[0, 3] == pytest.approx(np.abs(d).sum(), rel=1e-14)
    ones = R.image_sums(x, y, np.ones((2, 1, 12, 12)))
    assert np.allclose(ones[:, 2:4], ones[:, 0:2], rtol=1e-15, atol=0) and np.array_equal(ones[:, 4], [432, 432])
    got = R.image_scores(s, (3, 12, 12))
    assert got["psnr_masked"] == pytest.approx(10 * np.log10(4.0 / ((d * d).sum() / (3 * 6 * 12))), rel=1e-12)     # (image 0 alone)
    assert got["l1"] == pytest.approx(np.abs(x - y).mean(), rel=1e-13)


def test_counts_and_f1_on_a_hand_made_table():
    #                  class 0      class 1      class 2
    logits = np.array([[2.0, -1.0, 0.0],        # predicts {0}       (a logit of exactly 0 is a negative)
                       [0.5, 3.0, -2.0],        # predicts {0, 1}
                       [-1.0, -1.0, -0.5],      # predicts {}
                       [1.0, -2.0, 4.0]])       # predicts {0, 2}
    targets = np.array([[1, 0, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0]], dtype=np.float64)
    c = R.clf_counts(logits, targets, "bce")
    assert c.dtype == np.int64
    assert c.tolist() == [2, 1, 0,  1, 0, 1,  0, 1, 0,  1, 2, 3,  1]       # TP | FP | FN | TN | exact rows (row 0 only)
    assert np.array_equal(c, R.clf_counts(logits, targets, "mse"))
    s = R.clf_scores(c)
    # F1: class 0 = 2*2/(4+1+0) = 0.8, class 1 = 2*1/(2+0+1) = 2/3, class 2 has no positive target: left out
    assert s["acc"] == 0.25 and s["f1"] == pytest.approx((0.8 + 2 / 3) / 2, rel=1e-15)
    cce = R.clf_counts(logits, targets, "cce")                     # argmax: 0, 1, 2, 2 against 0, 1, 1, 0
    assert cce.tolist() == [1, 1, 0,  0, 0, 2,  1, 1, 0,  2, 2, 2,  2]
    assert R.clf_scores(cce)["acc"] == 0.5
    assert np.isnan(R.clf_scores(R.clf_counts(logits, np.zeros((4, 3)), "bce"))["f1"])
