"""Float64 reference of class-mode SPADE (gb_mode 1) and the data its GPU tests run on -- plain torch on the CPU, no kernel consulted.

Written from the documents, not from the kernels:
  * normalization.py:24-37 as the oracle states it: z = IN(x) * (1 + gamma) + beta, then ReLU (architecture.py:241-245), behind an
    optional nearest x2 upsample; gamma | beta come out of two zero-padded 3x3 convs on the resized label map.  On a label map that
    is constant over the image the result depends on a pixel only through how much zero padding the two convs see there, i.e. through
    the pixel's distance to each edge as far as 2: the (N, 5, 5, 2C) class table.
  * the class rule: index i of an extent E has class i for i < 2, class 4 - (E - 1 - i) for i >= E - 2, else class 2.
  * csrc/geom.h on the ring order: "rows 0, 1 | rows H-2, H-1 | for rows 2 .. H-3: columns 0, 1, W-2, W-1".
test_spade_class_refs_cpu.py ties each of these to an independent statement (autograd, two real convs, the other tests' ring builders).

Layout: everything is NHWC as the kernels see it -- x (N, Hs, Ws, C) at the source resolution, z / dz (N, H, W, C) at the logical one
(H = Hs << up), mean / rstd (N, C), table (N, 5, 5, 2C) with gamma in [..., :C] and beta in [..., C:].  The functions compute in the dtype
of their inputs: float64 is the reference, the same call on float32 tensors is the "plain fp32 evaluation" the non-exact bounds are
taken from.

Exact data (``exact_problem``, ``prep_problem``; ``ops_problem`` and ``conv_problem`` on ``balanced_x``, whose statistics the kernels
compute themselves: mean 0, rstd 1 / a): mean in {-1, 0, 1}, rstd in {0.5, 1, 2}, integer x and dz, and a table
on a dyadic grid whose 25 classes of all N images are pairwise different in every channel: 1 + gamma = G / 2 with G even and nonzero,
beta = (rstd / 2) b with b odd, so that the pre-activation v = (rstd / 2) ((x - mean) G + b) is an odd multiple of rstd / 2 -- never 0,
at most 8 significant bits -- and xhat, the mask, g, g xhat and every class sum are exact in fp32.  Every builder asserts its own
conditions; test_spade_class_refs_cpu.py runs every shipped case through them without a GPU."""
import functools
import math

import torch

SLOPE_02 = float(torch.tensor(0.2, dtype=torch.float32))          # the slope as the C ABI's `float` carries it
F32_EXACT = float(2 ** 24)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def border_class_of(i, extent):
    if i < 2:
        return i
    if i >= extent - 2:
        return 4 - (extent - 1 - i)
    return 2


def class_map(H, W):
    """(H, W) int64: cy * 5 + cx of every pixel, 0 .. 24; 12 is the interior class (2, 2)"""
    assert H >= 4 and W >= 4
    cy = torch.tensor([border_class_of(h, H) for h in range(H)])
    cx = torch.tensor([border_class_of(w, W) for w in range(W)])
    return cy[:, None] * 5 + cx[None, :]


def ring_coords(H, W):
    """[(y, x)] of the 2-pixel frame in the order of geom.h: rows 0, 1 | rows H-2, H-1 | for rows 2 .. H-3: columns 0, 1, W-2, W-1"""
    assert H >= 4 and W >= 4
    out = []
    for y in (0, 1, H - 2, H - 1):
        out += [(y, x) for x in range(W)]
    for y in range(2, H - 2):
        out += [(y, x) for x in (0, 1, W - 2, W - 1)]
    return out


def upsampled(x, up):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if up else x


def gathered(table, H, W):
    """(N, 5, 5, 2C) -> gamma, beta (N, H, W, C): every pixel's own class"""
    n, c2 = table.shape[0], table.shape[-1]
    gb = table.reshape(n, 25, c2)[:, class_map(H, W).reshape(-1)].reshape(n, H, W, c2)
    return gb[..., :c2 // 2], gb[..., c2 // 2:]


# ---- the operation ----------------------------------------------------------------------------------------------------------------
def preact(x, mean, rstd, table, up):
    """-> (xhat, v, gamma) at the logical resolution: xhat = (x - mean) rstd, v = xhat (1 + gamma) + beta"""
    xl = upsampled(x, up)
    gamma, beta = gathered(table, xl.shape[1], xl.shape[2])
    xh = (xl - mean[:, None, None, :]) * rstd[:, None, None, :]
    return xh, xh * (1 + gamma) + beta, gamma


def forward(x, mean, rstd, table, up):
    """z = relu(IN(up(x)) (1 + gamma) + beta) at the logical resolution"""
    return preact(x, mean, rstd, table, up)[1].clamp_min(0)


def backward(dz, x, mean, rstd, table, up, slope, dskip=None):
    """-> (dx at the source resolution, dtable (N, 5, 5, 2C), s1 / M, s2 / M) of z = act(v), act'(v) = 1 for v > 0 else ``slope``:
         g = dz act'(v);  dgamma = g xhat, dbeta = g, summed over the pixels of each class (an empty class: 0)
         dxhat = g (1 + gamma);  s1 = sum dxhat, s2 = sum dxhat xhat over the M = H W logical pixels of the image
         dx = rstd (dxhat - s1 / M - xhat s2 / M), summed over the 2 x 2 cell of a source pixel behind the upsample, + dskip"""
    xh, v, gamma = preact(x, mean, rstd, table, up)
    n, H, W, c = dz.shape
    g = torch.where(v > 0, dz, slope * dz)
    cls = class_map(H, W).reshape(-1)
    dtable = torch.zeros(n, 25, 2 * c, dtype=dz.dtype)
    dtable[:, :, :c].index_add_(1, cls, (g * xh).reshape(n, H * W, c))
    dtable[:, :, c:].index_add_(1, cls, g.reshape(n, H * W, c))
    dxh = g * (1 + gamma)
    c1 = dxh.sum(dim=(1, 2)) / (H * W)
    c2 = (dxh * xh).sum(dim=(1, 2)) / (H * W)
    dxl = rstd[:, None, None, :] * (dxh - c1[:, None, None, :] - xh * c2[:, None, None, :])
    dx = dxl.reshape(n, H // 2, 2, W // 2, 2, c).sum(dim=(2, 4)) if up else dxl
    if dskip is not None:
        dx = dx + dskip
    return dx, dtable.reshape(n, 5, 5, 2 * c), c1, c2


def cancel_scale(dz, x, mean, rstd, table, up, slope):
    """rstd (|sum_cell dxhat| + cnt |c1| + cnt |xhat c2|) at the source resolution: the size of the terms that cancel in dx, which an
    fp32 evaluation's error is proportional to (the result itself may be arbitrarily smaller)"""
    xh, v, gamma = preact(x, mean, rstd, table, up)
    n, H, W, c = dz.shape
    dxh = torch.where(v > 0, dz, slope * dz) * (1 + gamma)
    c1 = dxh.sum(dim=(1, 2)) / (H * W)
    c2 = (dxh * xh).sum(dim=(1, 2)) / (H * W)
    cell = (lambda t: t.reshape(n, H // 2, 2, W // 2, 2, c).sum(dim=(2, 4))) if up else (lambda t: t)
    return rstd[:, None, None, :] * (cell(dxh).abs() + cell(c1.abs()[:, None, None, :].expand_as(xh))
                                     + cell((xh * c2[:, None, None, :]).abs()))


def class_abs_sums(dz, x, mean, rstd, table, up, slope):
    """(N, 5, 5, 2C): sum |g xhat| | sum |g| per class -- the scale an fp32 summation's error in dtable is proportional to"""
    xh, v, _ = preact(x, mean, rstd, table, up)
    n, H, W, c = dz.shape
    g = torch.where(v > 0, dz, slope * dz).abs()
    out = torch.zeros(n, 25, 2 * c, dtype=dz.dtype)
    cls = class_map(H, W).reshape(-1)
    out[:, :, :c].index_add_(1, cls, (g * xh.abs()).reshape(n, H * W, c))
    out[:, :, c:].index_add_(1, cls, g.reshape(n, H * W, c))
    return out.reshape(n, 5, 5, 2 * c)


def stats_of_records(records, count, eps):
    """(N, chunks, 2, C) records of sum x | sum x^2 -> mean, rstd (N, C): biased variance, clamped at 0"""
    s = records.sum(dim=1)
    mean = s[:, 0] / count
    var = (s[:, 1] / count - mean * mean).clamp_min(0)
    return mean, 1 / torch.sqrt(var + eps)


def prep(x, records, table, up, eps):
    """-> (mean, rstd, A, B, ring): the InstanceNorm statistics from the records, the interior class's z = relu(A x + B) coefficients
    A = rstd (1 + gamma), B = beta - mean A, and z of the frame's pixels (N, ring_pixels, C) in ring order"""
    n, hs, ws, c = x.shape
    mean, rstd = stats_of_records(records, hs * ws, eps)
    A = rstd * (1 + table[:, 2, 2, :c])
    B = table[:, 2, 2, c:] - mean * A
    z = forward(x, mean, rstd, table, up)
    ys, xs = zip(*ring_coords(z.shape[1], z.shape[2]))
    return mean, rstd, A, B, z[:, list(ys), list(xs)]


# ---- data -------------------------------------------------------------------------------------------------------------------------
def fits(t, pname):
    """every element of the float64 tensor is a value of the format"""
    return bool((t.to(torch.bfloat16 if pname == "bf16" else torch.float32).double() == t).all())


def ints(gen, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def choice(gen, shape, values):
    return torch.tensor(values, dtype=torch.float64)[torch.randint(0, len(values), shape, generator=gen)]


def distinct_table(gen, rstd):
    """(N, 5, 5, 2C) for the per-(image, channel) ``rstd`` (N, C): in every channel the 25 N values of 1 + gamma are a shuffle of the
    nonzero even numbers up to +-(25 N + 1) over 2, those of beta a shuffle of 25 N consecutive odd numbers times rstd / 2"""
    n, c = rstd.shape
    k = 25 * n
    half = (k + 1) // 2
    G = torch.tensor([2 * j for j in range(-half, half + 1) if j != 0][:k], dtype=torch.float64)
    b = torch.tensor([2 * j + 1 for j in range(-half, half)][:k], dtype=torch.float64)
    pg = torch.rand(c, k, generator=gen).argsort(dim=1)
    pb = torch.rand(c, k, generator=gen).argsort(dim=1)
    gamma = (G[pg] / 2 - 1).t().reshape(n, 25, c)
    beta = b[pb].t().reshape(n, 25, c) * (rstd / 2)[:, None, :]
    table = torch.cat([gamma, beta], dim=-1).reshape(n, 5, 5, 2 * c)
    assert_distinct(table)
    return table


def assert_distinct(table):
    """all 25 classes of all N images pairwise different, in gamma and in beta, in every channel; the images differ as tables"""
    n, c2 = table.shape[0], table.shape[-1]
    flat = table.reshape(n * 25, c2)
    for ch in range(c2):
        assert flat[:, ch].unique().numel() == n * 25, f"channel {ch} repeats a value"
    assert n >= 2


def exact_sum_ok(terms, unit, dims):
    """any summation order of these terms is exact in fp32: they lie on the grid ``unit`` and sum |term| < 2^24 unit"""
    q = terms / unit
    return bool((q == q.round()).all()) and bool((terms.abs().sum(dim=dims) / unit < F32_EXACT).all())


def every_class_counts(dtable, H, W):
    """every class that has pixels has a non-zero gradient entry in some image and channel (a class whose pixels all carry dz = 0 or a
    closed mask would hide a wrong pixel list)"""
    n = dtable.shape[0]
    empty = torch.bincount(class_map(H, W).reshape(-1), minlength=25) == 0
    dt = dtable.reshape(n, 25, -1)
    return bool((dt[:, empty] == 0).all()) and bool((dt[:, ~empty].abs().sum(dim=(0, 2)) > 0).all())


@functools.lru_cache(maxsize=None)
def exact_problem(N, H, W, C, up, pname, slope=0.0):
    """the first draw (seed 0, 1, ...) of _exact_problem in which every non-empty class carries a gradient: a condition on the
    reference alone"""
    for seed in range(50):
        P = _exact_problem(N, H, W, C, up, pname, slope, seed)
        if every_class_counts(P["dtable"], H, W):
            return P
    raise AssertionError("no draw in which every class carries a gradient")


def _exact_problem(N, H, W, C, up, pname, slope, seed):
    """Inputs of the four C entry points on exact data and the float64 results, for a logical H x W image.  ``exact``: which results
    the conditions below prove to be exact in the kernel's fp32 arithmetic in any order of evaluation."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * H + 13 * W + C + 2 * up)
    hs, ws = (H >> 1, W >> 1) if up else (H, W)
    mean, rstd = choice(gen, (N, C), [-1.0, 0.0, 1.0]), choice(gen, (N, C), [0.5, 1.0, 2.0])
    x = ints(gen, (N, hs, ws, C), -2, 2)
    table = distinct_table(gen, rstd)
    dz = ints(gen, (N, H, W, C), -2, 2) * (torch.rand((N, H, W, C), generator=gen) < 0.75)
    addend = ints(gen, (N, hs, ws, C), -3, 3)
    P = dict(N=N, H=H, W=W, C=C, up=up, slope=slope, x=x, mean=mean, rstd=rstd, table=table, dz=dz, addend=addend)
    xh, v, gamma = preact(x, mean, rstd, table, up)
    P["z"] = v.clamp_min(0)
    P["dx"], P["dtable"], P["c1"], P["c2"] = backward(dz, x, mean, rstd, table, up, slope)
    P["dx_add"] = backward(dz, x, mean, rstd, table, up, slope, addend)[0]
    # ---- the conditions
    assert bool((v != 0).all()), "a pre-activation on the kink"
    assert bool((dz == 0).any()) and bool((dz != 0).float().mean() > 0.5)
    assert bool(((v > 0).float().mean() > 0.2)) and bool(((v < 0).float().mean() > 0.2)), "the mask is one-sided"
    for name in ("x", "mean", "rstd", "table", "dz", "addend", "z"):
        assert fits(P[name], pname), f"{name} is not a {pname} value"
    for t in (xh, 1 + gamma, v):
        assert fits(t, "f32")
    slope_exact = slope in (0.0, 1.0)
    g = torch.where(v > 0, dz, slope * dz)
    dxh = g * (1 + gamma)
    sums_exact = slope_exact and exact_sum_ok(dxh, 0.5, (1, 2)) and exact_sum_ok(dxh * xh, 0.25, (1, 2)) \
        and exact_sum_ok(g * xh, 0.5, (1, 2)) and exact_sum_ok(g, 1.0, (1, 2))
    assert sums_exact or not slope_exact
    M = H * W
    pow2 = M & (M - 1) == 0
    dx_exact = sums_exact and pow2
    if dx_exact:        # every term of rstd (acc - cnt c1 - cnt xhat c2) (+ addend), and either order of the subtractions, is an fp32 value
        cnt = 4.0 if up else 1.0
        cell = (lambda t: t.reshape(N, hs, 2, ws, 2, C).sum(dim=(2, 4))) if up else (lambda t: t)
        xs = (x - mean[:, None, None, :]) * rstd[:, None, None, :]
        acc, t1, t2 = cell(dxh), cnt * P["c1"][:, None, None, :], cnt * xs * P["c2"][:, None, None, :]
        r = rstd[:, None, None, :]
        terms = (P["c1"], P["c2"], acc, t1, xs * P["c2"][:, None, None, :], t2, acc - t1, acc - t2, t1 + t2, acc - t1 - t2,
                 r * (acc - t1 - t2), r * (acc - t1 - t2) + addend)
        dx_exact = all(fits(t, "f32") for t in terms)            # (the partial cell sums of acc: exact_sum_ok(dxh) above)
        assert torch.equal(r * (acc - t1 - t2), P["dx"])
    # sums: dtable (and the records); coef: s1 / M, s2 / M; dx: every term.  The CPU file asserts that every shipped case with slope 0
    # or 1 has exact sums, and exact coefficients and dx wherever H W is a power of two: the data never opts out of an exact check.
    P["exact"] = dict(sums=sums_exact, coef=sums_exact and pow2, dx=dx_exact)
    P["pow2"] = pow2
    return P


def f32_errors(P, dskip=False):
    """the plain fp32 evaluation of ``backward`` on the problem's inputs against float64: (max |dx error| / cancel_scale,
    max |dtable error| / class_abs_sums)"""
    args = [P[k] for k in ("dz", "x", "mean", "rstd", "table")]
    a32 = [t.float() for t in args]
    add = P["addend"] if dskip else None
    dx32, dt32, _, _ = backward(*a32, P["up"], P["slope"], None if add is None else add.float())
    dx64, dt64, _, _ = backward(*args, P["up"], P["slope"], add)
    scale = cancel_scale(*args, P["up"], P["slope"])
    tscale = class_abs_sums(*args, P["up"], P["slope"])
    e_dx = ((dx32.double() - dx64).abs() / scale.clamp_min(1e-30)).max().item()
    e_dt = ((dt32.double() - dt64).abs() / tscale.clamp_min(1e-30)).max().item()
    return e_dx, e_dt


@functools.lru_cache(maxsize=None)
def prep_problem(N, Hs, Ws, C, up, chunks, pname, seed=0):
    """dei2i_spade_prep on hand-made records: ``chunks`` rows of integers whose sums are mean * count and (var + mean^2) * count with
    mean in {-1, 0, 1, 2} and var in {1/4, 1, 4}, so that with eps = 0 mean and rstd in {2, 1, 0.5} are exact.  (The records are not
    the moments of x: the kernel must take its statistics from the records.)"""
    gen = torch.Generator().manual_seed(5000 + 1000 * seed + 7 * Hs + 13 * Ws + C + 2 * up + chunks)
    count = Hs * Ws
    mean, var = choice(gen, (N, C), [-1.0, 0.0, 1.0, 2.0]), choice(gen, (N, C), [0.25, 1.0, 4.0])
    totals = torch.stack([mean * count, (var + mean * mean) * count], dim=1)            # (N, 2, C)
    records = ints(gen, (N, chunks, 2, C), -40, 40)
    records[:, -1] = totals - records[:, :-1].sum(dim=1)
    rstd = 1 / var.sqrt()
    x = ints(gen, (N, Hs, Ws, C), -2, 2) + mean[:, None, None, :].round()
    table = distinct_table(gen, rstd)
    P = dict(N=N, Hs=Hs, Ws=Ws, C=C, up=up, chunks=chunks, x=x, records=records, table=table)
    P["mean"], P["rstd"], P["A"], P["B"], P["ring"] = prep(x, records, table, up, 0.0)
    assert torch.equal(P["mean"], mean) and torch.equal(P["rstd"], rstd), "the records do not give the intended statistics"
    assert fits(records, "f32") and bool((records.abs().sum(dim=1) < F32_EXACT).all())
    assert bool((totals[:, 1] * 4 == (totals[:, 1] * 4).round()).all())
    for name in ("x", "table", "ring"):
        assert fits(P[name], pname), f"{name} is not a {pname} value"
    for name in ("A", "B"):
        assert fits(P[name], "f32")
    _, v, _ = preact(x, mean, rstd, table, up)
    assert bool((v != 0).all()) and fits(v, "f32")
    assert bool((P["ring"] > 0).float().mean() > 0.2) and bool((P["ring"] == 0).float().mean() > 0.2)
    return P


def balanced_x(gen, N, Hs, Ws, C):
    """(x (N, Hs, Ws, C), a (N, C)): per (image, channel) half the pixels +a and half -a in a shuffled order, a in {1, 2, 4}: the mean
    is exactly 0 and the variance exactly a^2, from any summation order of the moments (Hs Ws even); x - mean is an integer, as
    distinct_table's no-kink argument wants"""
    hw = Hs * Ws
    assert hw % 2 == 0
    a = choice(gen, (N, C), [1.0, 2.0, 4.0])
    signs = torch.cat([torch.ones(hw // 2), -torch.ones(hw - hw // 2)]).double()
    order = torch.rand(N, C, hw, generator=gen).argsort(dim=2)
    x = (signs[order] * a[:, :, None]).permute(0, 2, 1).reshape(N, Hs, Ws, C)
    assert bool((x.sum(dim=(1, 2)) == 0).all()) and torch.equal((x * x).sum(dim=(1, 2)) / hw, a * a)
    return x, a


@functools.lru_cache(maxsize=None)
def ops_problem(N, Hs, Ws, C, up, pname, seed=0):
    """ops.spade_relu(x, gb, up, 1, eps = 0, skip = not up) on balanced x: mean = 0, rstd = 1 / a exactly, xhat = +-1, a distinct table
    for that rstd, integer upstream gradients with zeros (and one for the skip output)."""
    gen = torch.Generator().manual_seed(9000 + 1000 * seed + 7 * Hs + 13 * Ws + C + 2 * up)
    H, W = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    x, a = balanced_x(gen, N, Hs, Ws, C)
    mean, rstd = torch.zeros(N, C, dtype=torch.float64), 1 / a
    table = distinct_table(gen, rstd)
    dz = ints(gen, (N, H, W, C), -2, 2) * (torch.rand((N, H, W, C), generator=gen) < 0.75)
    dskip = None if up else ints(gen, (N, Hs, Ws, C), -3, 3)
    P = dict(N=N, H=H, W=W, C=C, up=up, x=x, mean=mean, rstd=rstd, table=table, dz=dz, dskip=dskip, slope=0.0, addend=dskip)
    xh, v, gamma = preact(x, mean, rstd, table, up)
    P["z"] = v.clamp_min(0)
    P["dx"], P["dtable"], P["c1"], P["c2"] = backward(dz, x, mean, rstd, table, up, 0.0, dskip)
    assert bool((v != 0).all()) and bool((xh.abs() == 1).all())
    for name in ("x", "table", "dz", "z"):
        assert fits(P[name], pname), f"{name} is not a {pname} value"
    g = dz * (v > 0)
    dxh = g * (1 + gamma)
    assert exact_sum_ok(dxh, 0.5, (1, 2)) and exact_sum_ok(dxh * xh, 0.5, (1, 2)) and exact_sum_ok(g * xh, 1.0, (1, 2))
    M = H * W
    P["exact_dx"] = M & (M - 1) == 0
    if P["exact_dx"]:
        assert fits(P["c1"], "f32") and fits(P["c2"], "f32") and fits(P["dx"] * 1.0, "f32")
        assert math.log2(M) + 9 < 24        # |dxhat| <= 2 (25 N + 1) / 2 < 2^7 on the grid 1/2: sums over M pixels, divided by M
    return P


@functools.lru_cache(maxsize=2)
def conv_problem(N, Hs, Ws, up, cin, cout, seed=0):
    """ops.spade_conv(x, gb, w, ..., eps = 0) in bf16 on exact data: conv3x3(reflect)(relu(SPADE(up(x)))) and its three gradients.
    The conv gates want N in the hundreds, and one byte of significand holds 50 distinct table values per channel: the images take two
    distinct tables (and two sets of a = 1 / rstd) in turn, so image 1 still differs from image 0 in every class.
      x: balanced +-a, a in {1, 2}: mean 0, rstd 1 / a, xhat = +-1;  w: ternary, density 1/2;  dy: +-1, density 1/16.
    Then z (8 bits), the MFMA sums behind y, dz (a small integer), dw, the class sums and -- H W is a power of two -- every term of dx
    are exact in fp32: y, dz, dgb and dx are the float64 values rounded once to bf16, dw is the float64 value.  All of it is asserted
    here, on the reference."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(7000 + 1000 * seed + 7 * Hs + 13 * Ws + cin + 2 * up)
    H, W = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    hw = Hs * Ws
    a2 = choice(gen, (2, cin), [1.0, 2.0])
    table2 = distinct_table(gen, 1 / a2)
    idx = torch.arange(N) % 2
    a, table = a2[idx], table2[idx]
    signs = torch.cat([torch.ones(hw // 2), -torch.ones(hw - hw // 2)]).double()
    x = (signs[torch.rand(N, cin, hw, generator=gen).argsort(dim=2)] * a[:, :, None]).permute(0, 2, 1).reshape(N, Hs, Ws, cin)
    assert hw % 2 == 0 and bool((x.sum(dim=(1, 2)) == 0).all()) and torch.equal((x * x).sum(dim=(1, 2)) / hw, a * a)
    mean, rstd = torch.zeros(N, cin, dtype=torch.float64), 1 / a
    w = (torch.randint(0, 2, (cout, cin, 3, 3), generator=gen) * 2 - 1).double() * (torch.rand((cout, cin, 3, 3), generator=gen) < 0.5)
    dy = (torch.randint(0, 2, (N, cout, H, W), generator=gen) * 2 - 1).double() * (torch.rand((N, cout, H, W), generator=gen) < 1 / 16)
    xh, v, gamma = preact(x, mean, rstd, table, up)
    assert bool((v != 0).all()) and bool((xh.abs() == 1).all())
    z = v.clamp_min(0)
    zl = z.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    y = F.conv2d(F.pad(zl, (1, 1, 1, 1), mode="reflect"), wg)
    dzl, dw = torch.autograd.grad(y, [zl, wg], dy)
    dz = dzl.permute(0, 2, 3, 1).contiguous()
    y = y.detach().permute(0, 2, 3, 1).contiguous()
    # ---- exactness, on the reference: operands are bf16 values, every fp32 accumulation is exact in any order
    for t, name in ((x, "x"), (table, "table"), (z, "z"), (dz, "dz"), (w, "w"), (dy, "dy")):
        assert fits(t, "bf16"), f"{name} is not a bf16 value"
    unit = 0.25                                                                        # z is a multiple of rstd / 2 >= 1/4
    zabs = F.conv2d(F.pad(z.abs().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect"), w.abs())
    assert bool((zabs / unit < F32_EXACT).all()), "a forward MFMA sum may round"
    assert bool((F.conv_transpose2d(dy.abs(), w.abs()).abs() * 4 < F32_EXACT).all())
    dw_abs = torch.autograd.grad(F.conv2d(F.pad(z.abs().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect"), wg), wg, dy.abs())[0]
    assert bool((dw_abs / unit < F32_EXACT).all()), "a weight-gradient sum may round"
    assert fits(dw, "f32")
    dskip = None
    dx, dtable, c1, c2 = backward(dz, x, mean, rstd, table, up, 0.0, dskip)
    g = dz * (v > 0)
    dxh = g * (1 + gamma)
    assert exact_sum_ok(dxh, 0.5, (1, 2)) and exact_sum_ok(dxh * xh, 0.5, (1, 2)) and exact_sum_ok(g * xh, 1.0, (1, 2))
    M = H * W
    assert M & (M - 1) == 0
    cnt = 4.0 if up else 1.0
    cell = (lambda t: t.reshape(N, Hs, 2, Ws, 2, cin).sum(dim=(2, 4))) if up else (lambda t: t)
    xs = x * rstd[:, None, None, :]
    acc, t1, t2 = cell(dxh), cnt * c1[:, None, None, :], cnt * xs * c2[:, None, None, :]
    for t in (c1, c2, acc, t1, t2, acc - t1, acc - t2, t1 + t2, acc - t1 - t2, rstd[:, None, None, :] * (acc - t1 - t2)):
        assert fits(t, "f32"), "a term of dx needs more than 24 bits"
    assert every_class_counts(dtable[:2], H, W) and not torch.equal(table[0], table[1])
    return dict(N=N, H=H, W=W, up=up, cin=cin, cout=cout, x=x, table=table, w=w, dy=dy.permute(0, 2, 3, 1).contiguous(), z=z, y=y, dz=dz,
                dw=dw, dx=dx, dtable=dtable)


# mode: (Hs, Ws, up, cin, cout, N as a function of the CU count -- the gates of test_conv_exact_gpu.py).  "ring": the conv's dgrad takes the
# SPADE backward records in its epilogue from 32 x 64 logical pixels on (two 16 x 32 tiles each way), so the source is 16 x 32 -- at
# 8 x 16, the smallest the forward admits, only the streaming route would run.  "pro": one 8 x 32 tile per image, streaming route only.
CONV_CASES = {
    "ring": (16, 32, 1, 64, 128, lambda cu: -(-((cu * 7) // 8) // 4)),       # halo16: four 16 x 32 tiles per image, tiles >= 7/8 of the CUs
    "pro": (4, 16, 1, 64, 128, lambda cu: cu // 2),                            # halo_conv: one 8 x 32 tile per image, tiles >= half the CUs
}
MI355X_CUS = 256


PREP_REAL = [(9, 15, 0), (5, 7, 1)]          # (Hs, Ws, up): two moments chunks / a ring behind the upsample


@functools.lru_cache(maxsize=None)
def prep_real_data(N, Hs, Ws, C, up, pname):
    """random x and a generic table with 25 N distinct values per channel, both values of the format (float64 tensors)"""
    gen = torch.Generator().manual_seed(40 + Hs + up)
    dt = torch.bfloat16 if pname == "bf16" else torch.float32
    x = (torch.randn(N, Hs, Ws, C, generator=gen) * 1.3 + 0.4).to(dt).double()
    table = distinct_table(gen, torch.ones(N, C, dtype=torch.float64)) * 0.125 + 0.01 * torch.randn(N, 5, 5, 2 * C, generator=gen).double()
    table = table.to(dt).double()
    assert_distinct(table)
    return x, table


# ---- the shipped cases (the GPU file runs exactly these; the CPU file proves the builders' conditions for each) -------------------
VEC = {"bf16": 8, "f32": 4}
PNAMES = ["f32", "bf16"]
# logical (H, W), up.  4: top and bottom border classes meet, class 2 empty in that dimension; 5: one interior row / column; with up,
# sources 2, 3 and 4: a 2 x 2 cell spans two or four classes, at H = 6 the cell of rows 2 | 3 straddles interior and border
SEAM_HW = [(h, w, 0) for h in (4, 5, 6, 7) for w in (4, 5, 6, 7)] + [(4, 9, 0), (9, 4, 0), (5, 34, 0)] + \
          [(h, w, 1) for h in (4, 6, 8) for w in (4, 6, 8)]
# (H, W, up, cv): the chunking and row-split seams (module docstring of test_spade_class_edges_gpu.py)
SPLIT_CASES = [
    (9, 15, 0, 1),       # HW = 135: two chunks of 68 + 67 rows, the boundary in the middle of image row 4; cv = 1: rpp = 256 > rows
    (9, 15, 0, 3),       # cv = 3: rpp = 85, thread 255 idle; 68 rows = one tail row per thread
    (8, 16, 0, 2),       # HW = 128 = 2^7: two even chunks, coefficients and dx exact
    (8, 16, 1, 2),       # the same behind the upsample (source 4 x 8)
    (6, 8, 0, 256),      # cv = 256: rpp = 1, 48 rows = 24 trips of the two-row loop, no tail (0 rows left)
    (5, 9, 0, 256),      # cv = 256, 45 rows: 22 trips and one tail row
    (4, 4, 0, 16),       # rpp = 16, 16 rows: one row per thread, the two-row loop never runs
    (6, 6, 0, 8),        # rpp = 32, 36 rows: threads 0..3 run the two-row loop once (0 left), the others the tail alone
]
SLOPE_CASES = [(6, 7, 0, SLOPE_02), (6, 8, 1, SLOPE_02), (6, 7, 0, 1.0), (8, 8, 1, 1.0)]
# (Hs, Ws, up, cv, chunks)
PREP_CASES = [
    (4, 4, 0, 1, 1),     # the ring is the whole image; 16 items: one partial trip
    (4, 7, 0, 1, 3),     # H = 4 alone
    (7, 4, 0, 2, 2),     # W = 4 alone
    (5, 5, 0, 1, 1),     # one interior pixel
    (5, 34, 0, 3, 2),    # ring_pixels cv = 140 * 3 = 420: not a multiple of 256, second trip of the grid-stride loop
    (2, 2, 1, 1, 1),     # source 2 x 2 -> 4 x 4: every cell spans four classes
    (3, 4, 1, 2, 2),     # 6 x 8 behind the upsample
    (8, 8, 1, 32, 1),    # 16 x 16: 112 * 32 = 3584 items on two workgroups
]
NC = 2


def exact_cases():
    """every (N, H, W, C, up, pname, slope) the GPU file feeds exact_problem"""
    out = []
    for p in PNAMES:
        out += [(NC, h, w, VEC[p], up, p, 0.0) for h, w, up in SEAM_HW]
        out += [(NC, h, w, cv * VEC[p], up, p, 0.0) for h, w, up, cv in SPLIT_CASES]
        out += [(NC, h, w, VEC[p], up, p, s) for h, w, up, s in SLOPE_CASES]
    return out


def prep_cases():
    return [(NC, hs, ws, cv * VEC[p], up, chunks, p) for p in PNAMES for hs, ws, up, cv, chunks in PREP_CASES]


OPS_CASES = [(4, 4, 0), (8, 8, 0), (5, 6, 0), (2, 2, 1), (4, 8, 1), (3, 4, 1)]       # (Hs, Ws, up)


def ops_cases():
    return [(NC, hs, ws, 2 * VEC[p], up, p) for p in PNAMES for hs, ws, up in OPS_CASES]
