"""Class-mode SPADE (gb_mode 1: gamma | beta from an (N, 5, 5, 2C) table, looked up per pixel with border_class(h, H) * 5 +
border_class(w, W)) on tables whose 25 classes of every image are pairwise different in every channel, against the float64 reference
of spade_class_reference.py -- spade_act_kernel, spade_prep_kernel, spade_bwd_partial / _border / _finalize / _apply_kernel through
their C entry points, then through ops.spade_relu and ops.spade_conv (both fused forms, both routes of ops._spade_backward).  A wrong pixel -> class mapping, a wrong border pixel list, a class never written
or a dropped ``n * 25`` moves a result here; on a replicated table (test_reduce_edges_gpu.py) it does not.

Harness (test_elementwise_edges_gpu.py): every output is carved out of a NaN-sentinel buffer with guards on both sides, the guards are
checked after every call, every element of every output is compared.

Exact data (spade_class_reference.exact_problem: mean in {-1, 0, 1}, rstd in {0.5, 1, 2}, integer x and dz, dyadic tables): z, the table
gradient of all 25 classes (in bf16: the float64 sum rounded once; an empty class: +0.0) and the four records are compared with
``torch.equal``; the coefficients s1 / M, s2 / M and dx too where M = H W is a power of two and the builder shows every term of dx to be an
fp32 value.  Elsewhere (M not a power of two, the slope 0.2f) nothing is fixed in advance: the kernel's error, measured relative to
rstd (|sum_cell dxhat| + cnt |c1| + cnt |xhat c2|) -- the terms that cancel -- must stay within 4x that of the same formulas evaluated
in fp32 by torch on the CPU (both against float64; bf16 adds one rounding of the result, 2^-8 |ref|); a coefficient is the correctly
rounded quotient, within 2^-24 of the reference.  Each such test prints both errors.

Seams (the tables in spade_class_reference.py name what each shape reaches): H, W in {4, 5, 6, 7}, (4, 9), (9, 4), (5, 34); behind the
upsample sources 2, 3, 4; cv = 1, 3, 256 (257 is refused); one and two moments chunks with the boundary inside an image row; 0 and 1 rows
left for the tail of the two-rows-in-flight loop; dgb = NULL; slopes 0, 0.2f and 1 on distinct tables.

Measured on an MI355X (DESIGN.md section 4 has the table): worst kernel error of the non-exact f32 dx cases 2.96e-5 of the cancelling terms,
the fp32 CPU restatement's 2.96e-5, worst kernel : CPU ratio 2.5 (6 x 7, slope 0.2f); the file's 220 tests take 6 s.  Eight in-bounds
mutations of the kernels each fail at least 16 of them."""

import pytest
import torch

import spade_class_reference as R
from test_elementwise_edges_gpu import BAD_ARG, DEV, Guarded, lib, prec_of, ptr, stream, sync  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = torch.float32


def note(*a):
    print("[spade-class-edges]", *a, flush=True)


def tdtype(pname):
    return torch.bfloat16 if pname == "bf16" else torch.float32


def cid(case):
    return "-".join(str(round(v, 3)) if isinstance(v, float) else str(v) for v in case)


def to_dev(t, dtype):
    return t.to(dtype).contiguous().to(DEV)


def stored(ref64, dtype):
    """the float64 reference rounded once to the stored type"""
    return ref64.to(dtype)


def assert_equal(got, ref64, what):
    """every element equals the reference rounded once to the output's type (+-0 alike; a NaN -- the sentinel -- equals nothing)"""
    want = stored(ref64, got.dtype).reshape(got.shape)
    bad = ~(got == want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {bad.nonzero()[:4].tolist()}: " \
                          f"got {got[bad][:4].tolist()} want {want[bad][:4].tolist()}"


def assert_within(got, ref64, scale, e32, what):
    """|got - ref| <= 4 e32 scale (+ 2^-8 |ref| for a bf16 output), element by element; prints the kernel's and the fp32 CPU error"""
    assert not got.isnan().any(), what
    ref = ref64.reshape(got.shape)
    err = (got.double() - ref).abs()
    if got.dtype == torch.bfloat16:
        err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0)
    rel = (err / scale.reshape(got.shape).clamp_min(1e-30)).max().item()
    note(f"{what}: kernel {rel:.3e}, fp32 CPU {e32:.3e} (relative to the cancelling terms)")
    assert rel <= 4 * e32, (what, rel, e32)


class Inputs:
    """the operands of a problem on the device, as the kernels see them"""

    def __init__(self, P, pname):
        dt = tdtype(pname)
        self.x, self.dz, self.table = to_dev(P["x"], dt), to_dev(P["dz"], dt), to_dev(P["table"], dt)
        self.mean, self.rstd = to_dev(P["mean"], F32), to_dev(P["rstd"], F32)
        self.addend = to_dev(P["addend"], dt)
        self.code = prec_of(pname).code
        self.dims = (P["N"], P["H"], P["W"], P["C"], P["up"])


def run_backward(lib, P, pname, want_dgb=True, addend=False):
    """dei2i_spade_bwd_partial + dei2i_spade_bwd_apply as ops._spade_backward calls them -> (records, dgb or None, coef, dx), each from its
    own guarded sentinel buffer"""
    I, dt = Inputs(P, pname), tdtype(pname)
    N, H, W, C, up = I.dims
    chunks = lib.dei2i_moments_chunks(H * W)
    partial, coef = Guarded(N * chunks * 4 * C, F32), Guarded(N * 2 * C, F32)
    dgb = Guarded(N * 25 * 2 * C, dt) if want_dgb else None
    dx = Guarded(P["x"].numel(), dt)
    dgb_p = dgb.ptr if want_dgb else None
    assert lib.dei2i_spade_bwd_partial(I.code, N, H, W, C, up, ptr(I.dz), ptr(I.x), ptr(I.mean), ptr(I.rstd), ptr(I.table), 1, P["slope"],
                                       dgb_p, partial.ptr, stream()) == 0
    assert lib.dei2i_spade_bwd_apply(I.code, N, H, W, C, up, ptr(I.dz), ptr(I.x), ptr(I.mean), ptr(I.rstd), ptr(I.table), 1, P["slope"],
                                     partial.ptr, chunks, dgb_p, coef.ptr, ptr(I.addend) if addend else None, dx.ptr, stream()) == 0
    sync()
    return (partial.values((N, chunks, 4, C)), dgb.values((N, 5, 5, 2 * C)) if want_dgb else None, coef.values((N, 2, C)),
            dx.values(tuple(P["x"].shape)))


def check_dtable(got, P, what):
    N, H, W, C = P["N"], P["H"], P["W"], P["C"]
    if P["exact"]["sums"]:
        assert_equal(got, P["dtable"], what + " dtable")
    else:
        e32 = R.f32_errors(P)[1]
        scale = R.class_abs_sums(*[P[k] for k in ("dz", "x", "mean", "rstd", "table")], P["up"], P["slope"])
        assert_within(got, P["dtable"], scale, e32, what + " dtable")
    empty = torch.bincount(R.class_map(H, W).reshape(-1), minlength=25) == 0
    bits = got.reshape(N, 25, 2 * C)[:, empty].contiguous().view(torch.int16 if got.dtype == torch.bfloat16 else torch.int32)
    assert bool((bits == 0).all()), what + ": an empty class is not +0.0"


def check_dx(got, P, with_addend, what):
    ref = P["dx_add"] if with_addend else P["dx"]
    if P["exact"]["dx"]:
        assert_equal(got, ref, what)
    else:
        e32 = R.f32_errors(P, with_addend)[0]
        scale = R.cancel_scale(*[P[k] for k in ("dz", "x", "mean", "rstd", "table")], P["up"], P["slope"])
        assert_within(got, ref, scale, e32, what)


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.exact_cases() if c[6] == 0.0], ids=cid)
def test_forward_bit_exact(lib, case):
    """dei2i_spade_act_fwd, class mode: z equals the reference in every element"""
    pname = case[5]
    P = R.exact_problem(*case)
    I = Inputs(P, pname)
    N, H, W, C, up = I.dims
    out = Guarded(N * H * W * C, tdtype(pname))
    assert lib.dei2i_spade_act_fwd(I.code, N, H, W, C, up, ptr(I.x), ptr(I.mean), ptr(I.rstd), ptr(I.table), 1, out.ptr, None, 1.0,
                                   stream()) == 0
    sync()
    assert_equal(out.values((N, H, W, C)), P["z"], f"z {cid(case)}")


# ---- backward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.exact_cases(), ids=cid)
def test_backward(lib, case):
    """partial + apply with and without the addend; the border kernel alone, as the hint route of ops._spade_backward launches it"""
    pname = case[5]
    P = R.exact_problem(*case)
    N, H, W, C, up = P["N"], P["H"], P["W"], P["C"], P["up"]
    tag = cid(case)
    records, dgb, coef, dx = run_backward(lib, P, pname)
    check_dtable(dgb, P, tag)
    cref = torch.stack([P["c1"], P["c2"]], dim=1)
    if P["exact"]["coef"]:
        assert_equal(coef, cref, tag + " coef")
    else:           # the correctly rounded quotient of an exact (slope 0, 1) or fp32-summed (0.2f) sum
        assert not coef.isnan().any()
        tol = 2.0 ** -24 * cref.abs() * (1 + 2.0 ** -20)
        if not P["exact"]["sums"]:
            I64 = [P[k] for k in ("dz", "x", "mean", "rstd", "table")]
            xh, v, gamma = R.preact(P["x"], P["mean"], P["rstd"], P["table"], up)
            dxh = (torch.where(v > 0, P["dz"], P["slope"] * P["dz"]) * (1 + gamma)).abs()
            mag = torch.stack([dxh.sum(dim=(1, 2)), (dxh * xh.abs()).sum(dim=(1, 2))], dim=1) / (H * W)
            a32 = R.backward(*[t.float() for t in I64], up, P["slope"])
            e32 = ((torch.stack(a32[2:], dim=1).double() - cref).abs() / mag.clamp_min(1e-30)).max().item()
            got = ((coef.double() - cref).abs() / mag.clamp_min(1e-30)).max().item()
            note(f"{tag} coef: kernel {got:.3e}, fp32 CPU {e32:.3e} (relative to sum |terms| / M)")
            tol = tol + 4 * e32 * mag
        assert bool(((coef.double() - cref).abs() <= tol).all()), tag + " coef"
    if P["exact"]["sums"]:          # the records: the chunks' sums, whatever the split, add up to the exact totals
        xh, v, gamma = R.preact(P["x"], P["mean"], P["rstd"], P["table"], up)
        dxh = torch.where(v > 0, P["dz"], P["slope"] * P["dz"]) * (1 + gamma)
        want = torch.stack([dxh.sum(dim=(1, 2)), (dxh * xh).sum(dim=(1, 2)), P["dtable"][:, 2, 2, :C], P["dtable"][:, 2, 2, C:]], dim=1)
        assert torch.equal(records.double().sum(dim=1), want), tag + " records"
    check_dx(dx, P, False, tag + " dx")
    _, dgb2, coef2, dx_add = run_backward(lib, P, pname, addend=True)
    check_dx(dx_add, P, True, tag + " dx + addend")
    assert torch.equal(dgb2.view(torch.uint8), dgb.view(torch.uint8)) and torch.equal(coef2, coef)
    # the border kernel alone: 24 classes, the interior one left to the finalize kernel
    I, dt = Inputs(P, pname), tdtype(pname)
    alone = Guarded(N * 25 * 2 * C, dt)
    assert lib.dei2i_spade_bwd_border(I.code, N, H, W, C, up, ptr(I.dz), ptr(I.x), ptr(I.mean), ptr(I.rstd), ptr(I.table), P["slope"],
                                      alone.ptr, stream()) == 0
    sync()
    alone.guards_intact()
    got = alone.interior().reshape(N, 25, 2 * C).cpu()
    assert bool((got[:, 12] == alone.sent).all()), "the border kernel wrote class (2, 2)"
    keep = [k for k in range(25) if k != 12]
    assert torch.equal(got[:, keep].view(dt), dgb.reshape(N, 25, 2 * C)[:, keep]), tag + ": the border kernel alone differs"


@pytest.mark.parametrize("case", [c for c in R.exact_cases() if (c[1], c[2]) in ((4, 4), (5, 34), (9, 15), (8, 8))], ids=cid)
def test_backward_without_a_table_gradient(lib, case):
    """dgb = NULL to both entry points (want_dgb False): nothing but records, coefficients and dx is written, and dx is unchanged"""
    P = R.exact_problem(*case)
    _, _, coef, dx = run_backward(lib, P, case[5])
    _, none, coef0, dx0 = run_backward(lib, P, case[5], want_dgb=False)
    assert none is None and torch.equal(coef0, coef) and torch.equal(dx0.view(torch.uint8), dx.view(torch.uint8))
    check_dx(dx0, P, False, cid(case) + " dx, dgb = NULL")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    # (what, H, W, up, cv, which entry points must refuse)
    ("up-odd-h", 5, 6, 1, 1, "pba"), ("up-odd-w", 6, 7, 1, 1, "pba"), ("up-odd-both", 5, 5, 1, 1, "pba"),
    ("h-below-4", 3, 8, 0, 1, "pba"), ("w-below-4", 8, 3, 0, 1, "pba"), ("h-below-4-up", 2, 8, 1, 1, "pba"),
    ("cv-257", 6, 6, 0, 257, "pba"), ("cv-257-up", 6, 6, 1, 257, "pba"),
]


@pytest.mark.parametrize("pname", R.PNAMES)
@pytest.mark.parametrize("what,H,W,up,cv,who", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(lib, what, H, W, up, cv, who, pname):
    """DEI2I_ERR_BAD_ARG and nothing written: an odd H or W behind the upsample (x has H >> 1 rows: row H - 1 would read past it), H or
    W < 4 in class mode, cv > 256.  (The inputs are sized for the rounded-up image, should a refusal ever be missing.)"""
    dt, N = tdtype(pname), 2
    C = cv * R.VEC[pname]
    code = prec_of(pname).code
    big = N * (H + 1) * (W + 1) * C
    src = torch.zeros(big, dtype=dt, device=DEV)
    tab = torch.zeros(N * 25 * 2 * C, dtype=dt, device=DEV)
    stat = torch.ones(N * C, dtype=F32, device=DEV)
    chunks = lib.dei2i_moments_chunks(H * W)
    rec_in = torch.zeros(N * chunks * 4 * C, dtype=F32, device=DEV)
    partial, coef, dgb, dx = Guarded(N * chunks * 4 * C, F32), Guarded(N * 2 * C, F32), Guarded(N * 25 * 2 * C, dt), Guarded(big, dt)
    rcs = {
        "p": lib.dei2i_spade_bwd_partial(code, N, H, W, C, up, ptr(src), ptr(src), ptr(stat), ptr(stat), ptr(tab), 1, 0.0, dgb.ptr,
                                         partial.ptr, stream()),
        "b": lib.dei2i_spade_bwd_border(code, N, H, W, C, up, ptr(src), ptr(src), ptr(stat), ptr(stat), ptr(tab), 0.0, dgb.ptr, stream()),
        "a": lib.dei2i_spade_bwd_apply(code, N, H, W, C, up, ptr(src), ptr(src), ptr(stat), ptr(stat), ptr(tab), 1, 0.0, ptr(rec_in), chunks,
                                       dgb.ptr, coef.ptr, None, dx.ptr, stream()),
    }
    sync()
    for k in who:
        assert rcs[k] == BAD_ARG, (what, k, rcs[k])
    for out in (partial, coef, dgb, dx):
        out.untouched()


@pytest.mark.parametrize("pname", R.PNAMES)
def test_prep_refuses_cv_257_and_a_ring_below_4(lib, pname):
    dt, N = tdtype(pname), 2
    code = prec_of(pname).code
    for Hs, Ws, up, cv in ((6, 6, 0, 257), (3, 8, 0, 1), (1, 4, 1, 1)):
        C = cv * R.VEC[pname]
        x = torch.zeros(N * Hs * Ws * C, dtype=dt, device=DEV)
        tab = torch.zeros(N * 25 * 2 * C, dtype=dt, device=DEV)
        rec = torch.zeros(N * 2 * C, dtype=F32, device=DEV)
        outs = [Guarded(N * C, F32) for _ in range(4)]
        ring = Guarded(N * 4 * ((Hs + Ws) << up) * C, dt)
        rc = lib.dei2i_spade_prep(code, N, Hs, Ws, C, up, ptr(x), ptr(rec), 1, 0.0, ptr(tab), *[o.ptr for o in outs], ring.ptr, stream())
        sync()
        assert rc == BAD_ARG, (Hs, Ws, up, cv, rc)
        for o in outs + [ring]:
            o.untouched()


# ---- dei2i_spade_prep -------------------------------------------------------------------------------------------------------------
def run_prep(lib, pname, x, records, table, up, eps, with_ring=True):
    dt = tdtype(pname)
    N, Hs, Ws, C = x.shape
    chunks = records.shape[1]
    xd, rd, td = to_dev(x, dt), to_dev(records, F32), to_dev(table, dt)
    outs = [Guarded(N * C, F32) for _ in range(4)]
    rp = lib.dei2i_ring_pixels(Hs << up, Ws << up)
    assert rp == len(R.ring_coords(Hs << up, Ws << up))
    ring = Guarded(N * rp * C, dt)
    assert lib.dei2i_spade_prep(prec_of(pname).code, N, Hs, Ws, C, up, ptr(xd), ptr(rd), chunks, eps, ptr(td), *[o.ptr for o in outs],
                                ring.ptr if with_ring else None, stream()) == 0
    sync()
    if not with_ring:
        ring.untouched()
    return [o.values((N, C)) for o in outs] + [ring.values((N, rp, C)) if with_ring else None]


@pytest.mark.parametrize("case", R.prep_cases(), ids=cid)
def test_prep_bit_exact(lib, case):
    """hand-made records with exact statistics, eps = 0: mean, rstd, A, B and every ring pixel equal the reference; with ring = NULL the
    coefficients are written and nothing else"""
    N, Hs, Ws, C, up, chunks, pname = case
    P = R.prep_problem(*case)
    for with_ring in (True, False):
        mean, rstd, A, B, ring = run_prep(lib, pname, P["x"], P["records"], P["table"], up, 0.0, with_ring)
        for got, name in ((mean, "mean"), (rstd, "rstd"), (A, "A"), (B, "B")):
            assert_equal(got, P[name], f"prep {cid(case)} {name} ring={with_ring}")
        if with_ring:
            assert_equal(ring, P["ring"], f"prep {cid(case)} ring")


@pytest.mark.parametrize("pname", R.PNAMES)
@pytest.mark.parametrize("Hs,Ws,up", R.PREP_REAL)
def test_prep_on_real_statistics(lib, Hs, Ws, up, pname):
    """random x, records from dei2i_moments_partial, eps = 1e-5, against float64 on the records the kernel read.  Bound per output: 4x the
    error of the same formulas in fp32 (torch, CPU) plus one fp32 rounding of the stored value, 2^-24 |ref| (2^-8 |ref| for a bf16 ring)."""
    dt, N, C, eps = tdtype(pname), 2, 3 * R.VEC[pname], 1e-5
    x, table = R.prep_real_data(N, Hs, Ws, C, up, pname)
    chunks = lib.dei2i_moments_chunks(Hs * Ws)
    rec = Guarded(N * chunks * 2 * C, F32)
    xd = to_dev(x, dt)
    assert lib.dei2i_moments_partial(prec_of(pname).code, N, Hs * Ws, C, ptr(xd), rec.ptr, stream()) == 0
    sync()
    records = rec.values((N, chunks, 2, C))
    direct = torch.stack([x.sum(dim=(1, 2)), (x ** 2).sum(dim=(1, 2))], dim=1)
    assert torch.allclose(records.double().sum(dim=1), direct, rtol=1e-5, atol=1e-4), "the moment records are not the moments of x"
    ref = R.prep(x, records.double(), table, up, eps)
    f32 = R.prep(x.float(), records, table.float(), up, eps)
    got = run_prep(lib, pname, x, records, table, up, eps)
    for name, g, r64, r32 in zip(("mean", "rstd", "A", "B", "ring"), got, ref, f32):
        e32 = (r32.double() - r64).abs().max().item()
        err = (g.double() - r64).abs()
        bound = 4 * e32 + (2.0 ** -8 if g.dtype == torch.bfloat16 else 2.0 ** -24) * r64.abs()
        note(f"prep real {pname} {Hs}x{Ws} up={up} {name}: kernel max |err| {err.max().item():.3e}, fp32 CPU {e32:.3e}")
        assert not g.isnan().any() and bool((err <= bound).all()), name


# ---- through ops ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ops_cases(), ids=cid)
def test_spade_relu_through_ops(case):
    """ops.spade_relu(x, gb, up, 1, eps = 0, skip = not up) with a leaf table: balanced x gives mean 0 and rstd 1 / a exactly through
    dei2i_moments_partial and dei2i_in_finalize, so out, dgb and (M a power of two) dx with the skip gradient are exact"""
    from de_i2i_gan_amd import ops
    N, Hs, Ws, C, up, pname = case
    P, dt = R.ops_problem(*case), tdtype(pname)
    x = to_dev(P["x"], dt).requires_grad_(True)
    gb = to_dev(P["table"], dt).requires_grad_(True)
    skip = not up
    res = ops.spade_relu(x, gb, bool(up), 1, eps=0.0, skip=skip)
    out, outs, gouts = (res[0], list(res), [to_dev(P["dz"], dt), to_dev(P["dskip"], dt)]) if skip else (res, [res], [to_dev(P["dz"], dt)])
    dx, dgb = torch.autograd.grad(outs, [x, gb], gouts)
    sync()
    tag = "spade_relu " + cid(case)
    assert_equal(out.detach().cpu(), P["z"], tag + " out")
    assert_equal(dgb.cpu(), P["dtable"], tag + " dgb")
    if P["exact_dx"]:
        assert_equal(dx.cpu(), P["dx"], tag + " dx")
    else:
        e32 = R.f32_errors(P, skip)[0]
        scale = R.cancel_scale(*[P[k] for k in ("dz", "x", "mean", "rstd", "table")], up, 0.0)
        assert_within(dx.cpu(), P["dx"], scale, e32, tag + " dx")


@pytest.mark.parametrize("mode", ["ring", "pro"])
def test_spade_conv_through_ops(mode):
    """ops.spade_conv in the two forms ops.spade_conv_supported answers, at the smallest shapes their gates admit (64 -> 128 behind
    the upsample: source 4 x 16 for "pro"; 16 x 32 for "ring", the smallest at which the dgrad epilogue leaves the records), on exact data: y, dw, dgb and dx equal float64 (rounded once where the
    output is bf16) -- dei2i_spade_prep hands the conv a ring tensor and coefficients, the conv's dgrad hands dz (and, with
    ops.fuse_bwd, the backward records: dei2i_spade_bwd_border then runs alone) back to the SPADE kernels.  Both routes of
    ops._spade_backward are run where the dgrad epilogue takes the shape; ops.bwd_fused_counts tells them apart."""
    from ctypes import byref
    from de_i2i_gan_amd import ops
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    Hs, Ws, up, cin, cout, n_of = R.CONV_CASES[mode]
    N = n_of(cu)
    P = R.conv_problem(N, Hs, Ws, up, cin, cout)
    bf = torch.bfloat16
    geom = ops.ConvGeom(cin, cout, 3, 1, 1, True, bool(up))
    lib = ops._lib_for(torch.empty(1, device=DEV))
    d_log = ops._desc(ops.BF16, ops.ConvGeom(cin, cout, 3, 1, 1, True, False), N, P["H"], P["W"], cin, cout)
    epilogue = bool(lib.dei2i_conv2d_dgrad_norm_supported(byref(d_log)))
    assert epilogue or mode != "ring", "the dgrad epilogue refuses the ring shape: the hint route is not tested"
    saved = (ops.fuse_norm, ops.fuse_pro, ops.fuse_ring, ops.fuse_bwd)
    results = {}
    try:
        ops.fuse_norm, ops.fuse_pro, ops.fuse_ring = True, mode == "pro", True
        for fused in (True, False):
            ops.fuse_bwd = fused
            x = to_dev(P["x"], bf).requires_grad_(True)
            gb = to_dev(P["table"], bf).requires_grad_(True)
            w = torch.nn.Parameter(P["w"].float().to(DEV))
            assert ops.spade_conv_supported(x, w, geom, True) == mode
            before = dict(ops.bwd_fused_counts)
            y = ops.spade_conv(x, gb, w, ops.PackedWeights(), geom, eps=0.0, mode=mode)
            dx, dgb, dw = torch.autograd.grad(y, [x, gb, w], to_dev(P["dy"], bf))
            sync()
            took = {k: ops.bwd_fused_counts[k] - before[k] for k in before}
            assert took == ({"epilogue": 1, "taken": 1} if fused and epilogue else {"epilogue": 0, "taken": 0}), (fused, took)
            results[fused] = [t.detach().cpu() for t in (y, dw, dgb, dx)]
    finally:
        ops.fuse_norm, ops.fuse_pro, ops.fuse_ring, ops.fuse_bwd = saved
    for fused, (y, dw, dgb, dx) in results.items():
        tag = f"spade_conv {mode} fuse_bwd={fused}"
        assert_equal(y, P["y"], tag + " y")
        assert_equal(dw, P["dw"], tag + " dw")
        assert_equal(dgb, P["dtable"], tag + " dgb")
        assert_equal(dx, P["dx"], tag + " dx")
    assert torch.equal(results[True][2].view(torch.int16), results[False][2].view(torch.int16)), "the two routes differ in dgb"
