"""The kernels of global-norm gradient clipping (csrc/adam.hip): dei2i_grad_sumsq, dei2i_grad_clip_finalize and the ``_clip`` forms of
the Adam update, at the seams of the launch.

dei2i_grad_sumsq runs the Adam launch's grid -- B = min(512, ceil(max_n / 4 / 256)) workgroups of 256 threads per table row, B from
the LONGEST row --, a float4 grid-stride loop (a second trip for n > 524 288), the scalar tail of the n % 4 last elements, and the
scalar loop alone for a row whose gradient is not 16-byte aligned.  Every workgroup stores its partial, so a short row next to a
long one leaves B - 1 workgroups that must store 0.

Exactness.  On integer gradients in [-8, 8] every partial is an integer below 2^24 (asserted here from the launch geometry), so fp32
adds are exact whatever their order, and the partials must equal, workgroup by workgroup, what the geometry assigns to them.

Tolerance on random data (DESIGN.md section 4 has the measured value).  u = 2^-24.  All terms of S = sum g^2 are >= 0, so the relative
error of S is bounded by u times the roundings on the longest path to it: a thread's chain of fused multiply-adds (one rounding per
element, ``chain`` elements: 4 per float4 trip + 1 tail element), 6 shuffle adds across the wave, 3 adds across the four waves; the
double-precision sum of the partials, the square root and the product with grad_scale add nothing at this scale.  The square root
halves the relative error, the conversion to float adds one rounding of at most u:  k = (chain + 9) / 2 + 1.  A CPU restatement of the
same tree in fp32 has to pass the same bound.  out[1] = grad_scale * min(1, max_norm / (out[0] + 1e-6)) is compared with that formula
in float64 on the device's own out[0]: the add 1, the division 2, the product 1 (the rounding counts of test_optim_edges_gpu.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
SIZES = [1, 2, 3, 4, 5, 1023, 524288, 524288 + 4 * 256 + 3]      # the last: a second grid-stride trip of 256 float4 + a 3-element tail
MISALIGNED = 1029                                                 # one more row, its pointer 4 bytes past a 16-byte boundary
GUARD = 64                                                        # floats of NaN between two rows (a multiple of 4: rows stay aligned)
ADAM_SIZES = [5, 1023, 524288 + 4 * 256 + 3]


def note(*a):
    print("[grad-clip]", *a, flush=True)


def f32(x):
    return float(np.float32(x))


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib as L
    from de_i2i_gan_amd import ops
    ops._lib_for(torch.empty(1, device=DEV))
    return L.load()


def stream():
    from de_i2i_gan_amd import ops
    return ops._stream()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def blocks_of(max_n):
    return min(512, max(1, (max_n // 4 + 255) // 256))


class Rows:
    """Gradients laid out in ONE device buffer between NaN guard rows: guard, row 0, guard, row 1, ..., guard; every row starts
    16-byte aligned except the last, which starts one float later."""

    def __init__(self, host_rows, misaligned_last=True):
        self.host = [np.ascontiguousarray(r, dtype=np.float32) for r in host_rows]
        offs, at = [], GUARD
        for i, r in enumerate(self.host):
            if misaligned_last and i == len(self.host) - 1:
                at += 1
            offs.append(at)
            at += (len(r) + 3) // 4 * 4 + GUARD
        flat = np.full(at, np.nan, dtype=np.float32)
        self.is_guard = np.ones(at, dtype=bool)
        for o, r in zip(offs, self.host):
            flat[o:o + len(r)] = r
            self.is_guard[o:o + len(r)] = False
        self.buf = torch.from_numpy(flat).to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[o:o + len(r)] for o, r in zip(offs, self.host)]
        self.aligned = [v.data_ptr() % 16 == 0 for v in self.views]

    def guards_intact(self):
        return bool(torch.isnan(self.buf[torch.from_numpy(self.is_guard).to(DEV)]).all())


def sumsq(lib, views, pad=8):
    """-> (the B x count partials as a float32 array, B): one launch over ``views``, into a NaN-filled buffer with NaN cells on
    both sides that must stay NaN"""
    rows = [(0, v.data_ptr(), 0, 0, v.numel()) for v in views]
    max_n = max(r[4] for r in rows)
    B = lib.dei2i_grad_sumsq_blocks(max_n)
    assert B == blocks_of(max_n)
    tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
    cells = B * len(rows)
    buf = torch.full((cells + 2 * pad,), float("nan"), device=DEV)
    rc = lib.dei2i_grad_sumsq(ptr(tab), len(rows), max_n, ctypes.c_void_p(buf.data_ptr() + 4 * pad), stream())
    assert rc == 0
    host = buf.cpu().numpy()
    assert np.isnan(host[:pad]).all() and np.isnan(host[pad + cells:]).all()
    return host[pad:pad + cells].reshape(len(rows), B), B


def finalize(lib, partials, grad_scale, max_norm):
    part = torch.from_numpy(np.ascontiguousarray(partials, dtype=np.float32).reshape(-1)).to(DEV)
    out = torch.full((4,), float("nan"), device=DEV)
    assert lib.dei2i_grad_clip_finalize(ptr(part), part.numel(), grad_scale, max_norm, ptr(out), stream()) == 0
    host = out.cpu().numpy()
    assert np.isnan(host[2:]).all()
    return host[0], host[1]


# ---- the launch geometry, restated on the CPU -----------------------------------------------------------------------------
def tree(g, B, aligned):
    """The kernel's summation tree in fp32 on the CPU: -> (the B partials of one row, the longest per-thread chain).  A fused
    multiply-add is the float64 sum of the exact float64 square and the accumulator, rounded to fp32."""
    n, stride = len(g), B * 256
    n4 = n // 4 if aligned else 0
    acc = np.zeros(stride, dtype=np.float32)
    sq = g.astype(np.float64) ** 2
    chain = 0
    for k in range(-(-n4 // stride)):
        lo, hi = k * stride, min((k + 1) * stride, n4)
        for e in range(4):
            acc[:hi - lo] = (sq[4 * lo + e:4 * hi:4] + acc[:hi - lo].astype(np.float64)).astype(np.float32)
        chain += 4
    tail = sq[4 * n4:]
    for k in range(-(-len(tail) // stride)):
        part = tail[k * stride:(k + 1) * stride]
        acc[:len(part)] = (part + acc[:len(part)].astype(np.float64)).astype(np.float32)
        chain += 1
    v = acc.reshape(B, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    return ((v[:, 0, 0] + v[:, 1, 0]) + v[:, 2, 0]) + v[:, 3, 0], chain


def norm_of(partials, grad_scale):
    """the finalize launch's out[0] from fp32 partials, in float64 and rounded once"""
    return np.float32(math.sqrt(float(np.sum(partials.astype(np.float64)))) * grad_scale)


def scale_formula(out0, grad_scale, max_norm):
    """out[1] in float64 from the device's out[0] and the fp32 arguments"""
    coef = np.float64(np.float32(max_norm)) / (np.float64(out0) + np.float64(np.float32(1e-6)))
    return np.float64(np.float32(grad_scale)) * (coef if not coef > 1.0 else 1.0)


# ---- exact: integer gradients ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ints():
    rng = np.random.default_rng(17)
    rows = [rng.integers(1, 9, size=n) * rng.choice([-1, 1], size=n) for n in SIZES + [MISALIGNED]]
    r = Rows(rows)
    assert r.aligned == [True] * len(SIZES) + [False]
    return r


def check_exact(lib, rows, idx):
    views = [rows.views[i] for i in idx]
    got, B = sumsq(lib, views)
    assert np.isfinite(got).all()                                   # every one of B x count workgroups stored
    for row, i in zip(got, idx):
        want, chain = tree(rows.host[i], B, rows.aligned[i])
        assert (chain * 256 + 3) * 64 < 2 ** 24                     # a workgroup's partial stays an exactly representable integer
        assert want.max() < 2 ** 24
        assert (row == want).all(), i
    total = int(got.astype(np.int64).sum())
    assert total == sum(int((rows.host[i].astype(np.int64) ** 2).sum()) for i in idx)
    again, _ = sumsq(lib, views)
    assert got.tobytes() == again.tobytes()                         # two launches, equal bits
    assert rows.guards_intact()
    return got


@pytest.mark.parametrize("i", range(len(SIZES) + 1))
def test_sumsq_is_exact_on_integers_one_row(lib, ints, i):
    check_exact(lib, ints, [i])


def test_sumsq_is_exact_on_integers_all_rows_in_one_table(lib, ints):
    """the longest row sizes the grid: the short rows leave 511 workgroups that store 0"""
    got = check_exact(lib, ints, list(range(len(SIZES) + 1)))
    assert got.shape == (len(SIZES) + 1, 512) and (got[0, 1:] == 0).all() and got[0, 0] == ints.host[0][0] ** 2


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_finalize_on_the_integer_partials(lib, ints, grad_scale):
    got, _ = sumsq(lib, ints.views)
    S = sum(int((h.astype(np.int64) ** 2).sum()) for h in ints.host)
    want0 = np.float32(math.sqrt(float(S)) * grad_scale)
    norm = float(finalize(lib, got, grad_scale, 1.0)[0])            # the device's own out[0]
    for regime, max_norm in (("clamped", 2.0 * norm), ("clips", 0.3 * norm), ("at the norm", norm)):
        out0, out1 = finalize(lib, got, grad_scale, max_norm)
        assert float(out0) == norm
        assert abs(norm - float(want0)) <= float(np.spacing(want0)), (regime, out0, want0)          # 1 fp32 ulp
        ref = scale_formula(out0, grad_scale, max_norm)
        note(f"finalize gs={grad_scale} {regime}: out = ({out0!r}, {out1!r}), formula {ref!r}")
        assert abs(float(out1) - ref) <= 4 * U * abs(ref), (regime, out1, ref)
        if regime == "clamped":
            assert out1 == np.float32(grad_scale)
        if regime == "clips":
            assert out1 < np.float32(0.31 * grad_scale)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_finalize_edge_cases(lib, grad_scale):
    """zeros: (0, grad_scale); one inf: (inf, grad_scale * 0); one NaN: (NaN, NaN) -- what the float formula gives"""
    n = 1023
    for kind, bad in (("zero", 0.0), ("inf", float("inf")), ("nan", float("nan"))):
        g = np.zeros(n, dtype=np.float32) if kind == "zero" else np.ones(n, dtype=np.float32)
        g[517] = bad
        rows = Rows([g], misaligned_last=False)
        part, _ = sumsq(lib, rows.views)
        out0, out1 = finalize(lib, part, grad_scale, 1.0)
        if kind == "zero":
            assert out0 == 0 and not np.signbit(out0) and out1 == np.float32(grad_scale)
        elif kind == "inf":
            assert out0 == np.inf and out1 == 0
        else:
            assert np.isnan(out0) and np.isnan(out1)


# ---- random fp32 data against float64 -------------------------------------------------------------------------------------
def test_norm_of_random_gradients_within_the_tree_bound(lib):
    gen = np.random.default_rng(23)
    rows = Rows([gen.standard_normal(n).astype(np.float32) for n in SIZES + [MISALIGNED]])
    worst, ks = {"device": 0.0, "restatement": 0.0}, []
    cases = [[i] for i in range(len(rows.host))] + [list(range(len(rows.host)))]
    for idx in cases:
        got, B = sumsq(lib, [rows.views[i] for i in idx])
        assert np.isfinite(got).all()
        restated, chains = zip(*[tree(rows.host[i], B, rows.aligned[i]) for i in idx])
        k = (max(chains) + 9) / 2 + 1
        ks.append(k)
        exact = math.sqrt(sum(float((rows.host[i].astype(np.float64) ** 2).sum()) for i in idx))
        for gs in (1.0, 0.5):
            out0, _ = finalize(lib, got, gs, 1.0)
            for name, val in (("device", float(out0)), ("restatement", float(norm_of(np.stack(restated), gs)))):
                err = abs(val - exact * gs) / (exact * gs)
                worst[name] = max(worst[name], err / U)
                assert err <= k * U, (name, idx, gs, val, exact * gs, k)
    assert rows.guards_intact()
    note(f"random fp32 norm vs float64: worst relative error {worst['device']:.3f} u on the device, "
         f"{worst['restatement']:.3f} u in the CPU restatement (u = 2^-24; bounds k = {min(ks)} .. {max(ks)} u)")


# ---- the _clip forms of the Adam update -----------------------------------------------------------------------------------
def adam_state(seed):
    gen = torch.Generator().manual_seed(seed)
    return [[(torch.randn(n, generator=gen) * s).to(DEV) if kind != "v" else (torch.rand(n, generator=gen) * 1.5).to(DEV)
             for n in ADAM_SIZES] for kind, s in (("p", 0.5), ("g", 1.0), ("m", 0.3), ("v", 1.0))]


def adam_table(p, g, m, v):
    rows = [(a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), a.numel()) for a, b, c, d in zip(p, g, m, v)]
    return torch.tensor(rows, dtype=torch.int64).to(DEV), max(r[4] for r in rows)


@pytest.mark.parametrize("coupled", [False, True])
@pytest.mark.parametrize("dev", [False, True])
def test_clip_forms_equal_the_by_value_forms_bit_for_bit(lib, coupled, dev):
    """*scale_dev holding exactly grad_scale: dei2i_adam_step_clip == dei2i_adam_step / _l2, dei2i_adam_step_clip_dev == the _dev forms"""
    from de_i2i_gan_amd.optim import _HyperTable
    gs, wd, lr, b1, b2, eps, t = f32(0.37), 3e-2, 1e-2, 0.5, 0.999, 1e-8, 7
    scale = torch.tensor([float("nan"), gs, float("nan")], device=DEV)
    scale_ptr = ctypes.c_void_p(scale.data_ptr() + 4)
    p0, g, m0, v0 = adam_state(31)
    A = [[x.clone() for x in s] for s in (p0, m0, v0)]
    B = [[x.clone() for x in s] for s in (p0, m0, v0)]
    ta, n = adam_table(A[0], g, A[1], A[2])
    tb, _ = adam_table(B[0], g, B[1], B[2])
    c1, c2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    if dev:
        hyper = _HyperTable(torch.device(DEV), t, rows=4)
        hyper.ensure(t, lr, b1, b2, 0.0 if coupled else wd)
        h = (ptr(hyper.table), ptr(hyper.index), hyper.rows)
        if coupled:
            assert lib.dei2i_adam_step_l2_dev(ptr(ta), len(ADAM_SIZES), n, *h, b1, b2, eps, gs, wd, stream()) == 0
        else:
            assert lib.dei2i_adam_step_dev(ptr(ta), len(ADAM_SIZES), n, *h, b1, b2, eps, gs, stream()) == 0
        assert lib.dei2i_adam_step_clip_dev(ptr(tb), len(ADAM_SIZES), n, *h, b1, b2, eps, scale_ptr, int(coupled), wd, stream()) == 0
    else:
        fn = lib.dei2i_adam_step_l2 if coupled else lib.dei2i_adam_step
        assert fn(ptr(ta), len(ADAM_SIZES), n, lr, b1, b2, eps, c1, c2, gs, wd, stream()) == 0
        assert lib.dei2i_adam_step_clip(ptr(tb), len(ADAM_SIZES), n, lr, b1, b2, eps, c1, c2, scale_ptr, int(coupled), wd, stream()) == 0
    torch.cuda.synchronize()
    for name, x, y, before in zip("pmv", A, B, (p0, m0, v0)):
        for a, b, c in zip(x, y, before):
            assert torch.equal(a, b), (name, a.numel())
            assert not torch.equal(a, c), (name, a.numel())          # (the update ran)
