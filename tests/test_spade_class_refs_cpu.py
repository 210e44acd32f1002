"""The float64 reference of class-mode SPADE (spade_class_reference.py) checked against independent statements of the same thing, and
every data builder of test_spade_class_edges_gpu.py run through its own conditions -- no GPU.

  * ``backward`` against torch.autograd through InstanceNorm -> nearest x2 -> a gather of the table by ``class_map`` -> (Leaky)ReLU;
  * ``class_map`` against what two zero-padded 3x3 convs (normalization.py:24-37) make of a constant label map;
  * ``ring_coords`` against the class map, its length, and the ring builders of two other test files;
  * the builders: distinct tables, no pre-activation on the kink, format fits, exact sums -- for every shipped case."""
import pytest
import torch
import torch.nn.functional as F

import spade_class_reference as R

SIZES = [4, 5, 6, 9]


def rand_problem(N, hs, ws, C, up, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = (2 * hs, 2 * ws) if up else (hs, ws)
    x = torch.randn(N, hs, ws, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    table = torch.randn(N, 5, 5, 2 * C, generator=g, dtype=torch.float64) * 0.7
    dz = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    dskip = torch.randn(N, hs, ws, C, generator=g, dtype=torch.float64)
    return x, table, dz, dskip


AUTOGRAD_CASES = [(h, w, up) for up in (0, 1) for h in SIZES + [2, 3] * up for w in SIZES + [2, 3] * up]


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("hs,ws,up", AUTOGRAD_CASES)
def test_backward_equals_autograd(hs, ws, up, slope):
    """hs, ws: the logical size without the upsample, the source size behind it (2 and 3 only there: logical 4 and 6)"""
    N, C, eps = 2, 3, 1e-5
    x, table, dz, dskip = rand_problem(N, hs, ws, C, up, 100 * hs + 10 * ws + up)
    xg, tg = x.clone().requires_grad_(True), table.clone().requires_grad_(True)
    xn = F.instance_norm(xg.permute(0, 3, 1, 2), eps=eps)
    if up:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    H, W = xn.shape[-2:]
    gb = tg.reshape(N, 25, 2 * C)[:, R.class_map(H, W).reshape(-1)].reshape(N, H, W, 2 * C).permute(0, 3, 1, 2)
    v = xn * (1 + gb[:, :C]) + gb[:, C:]
    z = F.leaky_relu(v, slope) if slope else torch.relu(v)
    out = (z.permute(0, 2, 3, 1) * dz).sum() + (xg * dskip).sum()
    dx_ref, dt_ref = torch.autograd.grad(out, [xg, tg])
    mean = x.mean(dim=(1, 2))
    rstd = 1 / torch.sqrt(x.var(dim=(1, 2), unbiased=False) + eps)
    assert torch.allclose(R.forward(x, mean, rstd, table, up), torch.relu(v).permute(0, 2, 3, 1).detach(), rtol=1e-12, atol=1e-12)
    dx, dt, c1, c2 = R.backward(dz, x, mean, rstd, table, up, slope, dskip)
    assert dx.shape == x.shape and dt.shape == table.shape and c1.shape == (N, C) and c2.shape == (N, C)
    assert torch.allclose(dx, dx_ref, rtol=1e-10, atol=1e-11), (dx - dx_ref).abs().max()
    assert torch.allclose(dt, dt_ref, rtol=1e-10, atol=1e-11), (dt - dt_ref).abs().max()      # every class
    empty = torch.bincount(R.class_map(H, W).reshape(-1), minlength=25) == 0
    assert bool((dt.reshape(N, 25, -1)[:, empty] == 0).all()) and bool((dt_ref.reshape(N, 25, -1)[:, empty] == 0).all())
    assert empty.any() == (H == 4 or W == 4)


@pytest.mark.parametrize("H", [4, 5, 6, 7, 9, 34])
@pytest.mark.parametrize("W", [4, 5, 6, 7, 9, 34])
def test_class_map_is_what_two_zero_padded_convs_see(H, W):
    """normalization.py:24-37 on a constant label map, generic weights: pixels of one class get the same gamma | beta, pixels of
    different classes different ones"""
    g = torch.Generator().manual_seed(H * 100 + W)
    labels, hidden, C = 3, 16, 4            # (wide enough that the ReLU leaves generic, non-zero activations in every class)
    seg = torch.randn(1, labels, 1, 1, generator=g, dtype=torch.float64).expand(1, labels, H, W)
    w1, b1 = torch.randn(hidden, labels, 3, 3, generator=g, dtype=torch.float64), torch.randn(hidden, generator=g, dtype=torch.float64)
    w2, b2 = torch.randn(2 * C, hidden, 3, 3, generator=g, dtype=torch.float64), torch.randn(2 * C, generator=g, dtype=torch.float64)
    gb = F.conv2d(torch.relu(F.conv2d(seg, w1, b1, padding=1)), w2, b2, padding=1)[0].permute(1, 2, 0).reshape(H * W, 2 * C)
    cls = R.class_map(H, W).reshape(-1)
    assert cls.min() >= 0 and cls.max() <= 24
    same = cls[:, None] == cls[None, :]
    dist = (gb[:, None, :] - gb[None, :, :]).abs().max(dim=-1).values
    assert bool((dist[same] < 1e-12).all()), "two pixels of one class differ"
    assert bool((dist[~same] > 1e-6).all()), "two classes coincide"
    for h in range(H):
        for w in range(W):
            assert cls[h * W + w] == R.border_class_of(h, H) * 5 + R.border_class_of(w, W)


@pytest.mark.parametrize("H", [4, 5, 6, 7, 9, 16])
@pytest.mark.parametrize("W", [4, 5, 6, 7, 9, 34])
def test_ring_coords(H, W):
    rc = R.ring_coords(H, W)
    assert len(rc) == 4 * W + 4 * (H - 4) and len(set(rc)) == len(rc)
    cls = R.class_map(H, W)
    frame = {(y, x) for y in range(H) for x in range(W) if y < 2 or y >= H - 2 or x < 2 or x >= W - 2}
    assert set(rc) == frame
    border = {(y, x) for y in range(H) for x in range(W) if cls[y, x] != 12}
    assert border <= frame
    assert all(cls[y, x] == 12 for y, x in frame - border)        # (none: a frame pixel has a border class in y or in x, at 4 and 5 too)
    # order: rows 0, 1 | rows H-2, H-1 | rows 2 .. H-3: columns 0, 1, W-2, W-1
    assert rc[0] == (0, 0) and rc[W] == (1, 0) and rc[2 * W] == (H - 2, 0) and rc[4 * W - 1] == (H - 1, W - 1)
    if H > 4:
        assert rc[4 * W:4 * W + 4] == [(2, 0), (2, 1), (2, W - 2), (2, W - 1)]


def test_ring_coords_match_the_other_ring_builders():
    """tests/test_wgrad_halo_rows_gpu.py's ring_coords and tests/test_conv_fused_exact_gpu.py's ring_layout, on the shapes they use"""
    import test_conv_fused_exact_gpu as CF
    import test_wgrad_halo_rows_gpu as WG
    for H, W in [(16, 32), (8, 32), (32, 64), (4, 4), (5, 7)]:
        assert WG.ring_coords(H, W) == R.ring_coords(H, W)
        zl = torch.arange(2 * 3 * H * W, dtype=torch.float64).reshape(2, 3, H, W)
        ys, xs = zip(*R.ring_coords(H, W))
        assert torch.equal(CF.ring_layout(zl), zl.permute(0, 2, 3, 1)[:, list(ys), list(xs)])


# ---- the builders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.exact_cases(), ids=lambda c: "-".join(map(str, c)))
def test_exact_problem_conditions(case):
    N, H, W, C, up, pname, slope = case
    P = R.exact_problem(*case)                    # asserts: distinct table, no kink, format fits, a two-sided mask
    R.assert_distinct(P["table"])
    assert not torch.equal(P["table"][0], P["table"][1])
    M = H * W
    if slope in (0.0, 1.0):
        assert P["exact"]["sums"], "dtable is not exact on this data"
        assert P["exact"]["coef"] == P["exact"]["dx"] == (M & (M - 1) == 0), "a power-of-two case lost its exact check"
    else:
        assert not any(P["exact"].values())
    # the reference itself: the same formulas in fp32 agree with float64 to fp32 accuracy (and bit for bit where exact)
    e_dx, e_dt = R.f32_errors(P)
    assert e_dx < 1e-4 and e_dt < 1e-6       # (dx: relative to the terms of the last line only -- c1 and c2 are themselves sums that cancel)
    if P["exact"]["dx"]:
        assert e_dx == 0 and e_dt == 0
    # every class that has pixels gets a gradient that depends on them; an empty class gets +0
    assert R.every_class_counts(P["dtable"], H, W)
    assert bool((P["dx"] != P["dx_add"]).any())


def test_exact_cases_cover_the_power_of_two_shapes():
    pow2 = {(c[1], c[2], c[4]) for c in R.exact_cases() if (c[1] * c[2]) & (c[1] * c[2] - 1) == 0 and c[6] == 0.0}
    assert {(4, 4, 0), (4, 4, 1), (4, 8, 1), (8, 4, 1), (8, 8, 1), (8, 16, 0), (8, 16, 1)} <= pow2


@pytest.mark.parametrize("case", R.prep_cases(), ids=lambda c: "-".join(map(str, c)))
def test_prep_problem_conditions(case):
    N, Hs, Ws, C, up, chunks, pname = case
    P = R.prep_problem(*case)
    R.assert_distinct(P["table"])
    assert P["records"].shape == (N, chunks, 2, C) and P["ring"].shape == (N, 4 * (Ws << up) + 4 * ((Hs << up) - 4), C)
    assert bool((P["rstd"].log2() == P["rstd"].log2().round()).all())
    # the statistics are the records', not x's
    assert not torch.allclose(P["x"].mean(dim=(1, 2)), P["mean"])
    # fp32 restatement of prep: bit for bit
    m, r, A, B, ring = R.prep(P["x"].float(), P["records"].float(), P["table"].float(), up, 0.0)
    for got, name in ((m, "mean"), (r, "rstd"), (A, "A"), (B, "B"), (ring, "ring")):
        assert torch.equal(got.double(), P[name]), name


@pytest.mark.parametrize("case", R.ops_cases(), ids=lambda c: "-".join(map(str, c)))
def test_ops_problem_conditions(case):
    N, Hs, Ws, C, up, pname = case
    P = R.ops_problem(*case)
    R.assert_distinct(P["table"])
    x = P["x"]
    assert bool((x.mean(dim=(1, 2)) == 0).all())
    var = (x * x).mean(dim=(1, 2))
    assert torch.equal(1 / var.sqrt(), P["rstd"]) and bool((P["rstd"].log2() == P["rstd"].log2().round()).all())
    M = P["H"] * P["W"]
    assert P["exact_dx"] == (M & (M - 1) == 0)
    assert (P["dskip"] is None) == bool(up)


@pytest.mark.parametrize("pname", R.PNAMES)
@pytest.mark.parametrize("Hs,Ws,up", R.PREP_REAL)
def test_prep_real_data_conditions(Hs, Ws, up, pname):
    x, table = R.prep_real_data(2, Hs, Ws, 3 * R.VEC[pname], up, pname)
    R.assert_distinct(table)
    assert R.fits(x, pname) and R.fits(table, pname)


@pytest.mark.parametrize("mode", sorted(R.CONV_CASES))
def test_conv_problem_conditions(mode):
    """the exactness of z, y, dz, dw, dgb and dx of the ops.spade_conv cases, at the batch the gates ask of a 256-CU part; N follows the
    gates of test_conv_exact_gpu.py"""
    from test_conv_exact_gpu import n_halo16, n_halo8
    Hs, Ws, up, cin, cout, n_of = R.CONV_CASES[mode]
    N = n_of(R.MI355X_CUS)
    assert N == (n_halo16(4, cout) if mode == "ring" else n_halo8(1, cout))(R.MI355X_CUS)
    P = R.conv_problem(N, Hs, Ws, up, cin, cout)            # asserts its conditions
    assert P["y"].shape == (N, 2 * Hs, 2 * Ws, cout) and P["dx"].shape == (N, Hs, Ws, cin) and P["dw"].shape == (cout, cin, 3, 3)
    assert P["y"].abs().max() > 4 and P["dz"].abs().max() > 2 and bool((P["dz"] == 0).any())
