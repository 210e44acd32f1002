"""The element-wise kernels of csrc/elementwise.hip that the layout tests leave out -- the average pool (forward, backward, and as
``ops.upsample2``), ``dei2i_act_bwd``, ``dei2i_affine_act_img_fwd``, the generator's head ``dei2i_compose_fwd / _bwd`` and the NaN
guard in front of it -- through their C entry points, in both compute dtypes, by the method of test_layout_edges_gpu.py: the test owns
every output, carved out of a buffer with 64 spare elements on each side, all pre-filled with a NaN sentinel, and compares the
interior element by element with a float64 CPU reference computed from the operands as the kernel sees them.

Seams: the grid caps and the grid-stride trip behind them (EW_CAP = 4096 workgroups x 256 threads; 2048 for the average pool; 512
per image for affine_act_img, rounded down to a multiple of cv / 256 when cv > 256), odd Ho / Wo / cv, the per-image coefficient row
(N >= 2), the two-vector store loop of compose_bwd (Cs = 2 VEC), its three nullable pointers, saturated sigmoid / tanh arguments,
the NaN flag at the thread, wavefront, workgroup and grid-stride positions and its reset between calls, and every refusal.

Exact where the data makes the arithmetic exact (the pool and act_bwd on integers, affine_act_img on a dyadic grid, the NaN guard
on bit patterns): ``torch.equal`` on bit patterns, nothing excluded.  Elsewhere the project's bound per element: 1e-5 max(1, |ref|)
for an fp32 output, 2^-8 |ref| + 1e-5 for a bf16 one; each such test prints the kernel's and a plain fp32 CPU restatement's worst
error against float64.  LeakyReLU's gradient at z = +-0 is 1 in the kernel (common.h: ``z >= 0``) where torch takes the slope:
test_act_bwd pins the kernel's convention with the +-0 entries.  Data, references and their conditions: test_elementwise_refs_cpu.py."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import test_elementwise_refs_cpu as R
from test_elementwise_refs_cpu import DTYPES, TORCH_DTYPE, VEC

gpu = pytest.mark.gpu
pytestmark = gpu
DEV = "cuda:0"
GUARD = 64
from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
SENTINEL = {"bf16": 0x7FC1, "f32": 0x7FC0ABCD}                        # quiet NaNs with a payload


def note(*a):
    print("[elementwise-edges]", *a, flush=True)


def prec_of(pname):
    from de_i2i_gan_amd import ops
    return ops.BF16 if pname == "bf16" else ops.F32


def itype(dtype):
    return torch.int16 if dtype == torch.bfloat16 else torch.int32


def bits(t):
    return t.contiguous().view(itype(t.dtype))


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib as L
    from de_i2i_gan_amd import ops
    ops._lib_for(torch.empty(1, device=DEV))
    return L.load()


def stream():
    from de_i2i_gan_amd import ops
    return ops._stream()


class Guarded:
    """``numel`` elements of ``dtype`` between two guards of GUARD elements, everything pre-filled with the sentinel (the helper of
    test_layout_edges_gpu.py; ``fill``: the interior starts as this tensor, for a kernel that works in place)"""

    def __init__(self, numel, dtype, fill=None):
        self.numel, self.dtype = numel, dtype
        self.sent = SENTINEL["bf16" if dtype == torch.bfloat16 else "f32"]
        self.flat = torch.full((numel + 2 * GUARD,), self.sent, dtype=itype(dtype), device=DEV)
        self.ptr = ctypes.c_void_p(self.flat.data_ptr() + GUARD * self.flat.element_size())
        assert self.ptr.value % 16 == 0
        if fill is not None:
            self.interior().copy_(bits(fill).reshape(-1))

    def interior(self):
        return self.flat[GUARD:GUARD + self.numel]

    def guards_intact(self):
        assert (self.flat[:GUARD] == self.sent).all() and (self.flat[GUARD + self.numel:] == self.sent).all(), "a write outside the tensor"

    def untouched(self):
        self.guards_intact()
        assert (self.interior() == self.sent).all(), "a refused call wrote to its output"

    def values(self, shape):
        """the interior on the CPU in its own dtype; the guards are checked on the way"""
        self.guards_intact()
        return self.interior().cpu().view(self.dtype).reshape(shape)

    def check(self, ref):
        """every interior element equals ``ref`` (bit patterns), every spare element is still the sentinel"""
        self.guards_intact()
        want = bits(ref).reshape(-1).to(DEV)
        assert want.numel() == self.numel
        assert torch.equal(self.interior(), want), "interior differs (an unwritten lane holds the sentinel)"


def within(got, ref64, what, cpu32=None):
    """per element: |got - ref| <= 1e-5 max(1, |ref|) for an fp32 ``got``, <= 2^-8 |ref| + 1e-5 for a bf16 one (one bf16 rounding of the
    float64 reference on top of the fp32 bound).  Prints the worst error of the kernel and of the fp32 CPU restatement."""
    assert not got.isnan().any(), what
    ref = ref64.double().reshape(got.shape)
    err = (got.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-5 if got.dtype == torch.bfloat16 else 1e-5 * ref.abs().clamp(min=1)
    line = f"{what}: kernel max |err| {float(err.max()):.3e} ({float((err / bound).max()):.3f} of the bound)"
    if cpu32 is not None:
        line += f", fp32 CPU {float((cpu32.double().reshape(got.shape) - ref).abs().max()):.3e}"
    note(line)
    assert (err <= bound).all(), what


def sync():
    torch.cuda.synchronize()


# ---- the average pool -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", R.POOL_SMALL + R.POOL_CAPPED, ids=str)
def test_avgpool_forward_and_backward_bit_exact(lib, shape, pname):
    prec, P = prec_of(pname), R.pool_problem(shape, pname)
    n, h, w, cv = shape
    c = cv * VEC[pname]
    xd, dd = P["x"].to(DEV), P["dout"].to(DEV)
    out, dx = Guarded(P["out"].numel(), prec.dtype), Guarded(P["dx"].numel(), prec.dtype)
    assert lib.dei2i_avgpool2_fwd(prec.code, n, h, w, c, ptr(xd), out.ptr, stream()) == 0
    assert lib.dei2i_avgpool2_bwd(prec.code, n, h, w, c, ptr(dd), dx.ptr, stream()) == 0
    sync()
    out.check(P["out"])
    dx.check(P["dx"])


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", R.POOL_SMALL, ids=str)
def test_upsample2_equals_nearest_interpolation(shape, pname):
    from de_i2i_gan_amd import ops
    x = R.pool_problem(shape, pname)["dout"]                          # (N, H/2, W/2, C) integers
    want = F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1).contiguous().to(x.dtype)
    got = ops.upsample2(x.to(DEV))
    assert got.shape == want.shape and got.dtype == x.dtype
    assert torch.equal(bits(got).cpu(), bits(want))


@pytest.mark.parametrize("pname", DTYPES)
def test_avgpool_refusals(lib, pname):
    prec, vec = prec_of(pname), VEC[pname]
    x = torch.ones(2 * 6 * 6 * 2 * vec, dtype=prec.dtype, device=DEV)
    for n, h, w, c, null in [(1, 3, 4, vec, None), (1, 4, 3, vec, None), (1, 4, 4, vec + 1, None), (1, 4, 4, vec // 2, None),
                             (0, 4, 4, vec, None), (1, 4, 4, vec, "in"), (1, 4, 4, vec, "out")]:
        for fn in (lib.dei2i_avgpool2_fwd, lib.dei2i_avgpool2_bwd):
            dst = Guarded(256, prec.dtype)
            assert fn(prec.code, n, h, w, c, None if null == "in" else ptr(x), None if null == "out" else dst.ptr, stream()) == BAD_ARG
            sync()
            dst.untouched()


# ---- dei2i_act_bwd ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("nvec", R.ACT_BWD_NVEC)
def test_act_bwd_bit_exact(lib, nvec, pname):
    """g = dz * act'(z) on integer dz and z in {-2, -0.5, -0.0, +0.0, 0.5, 3}, every class in every vector lane.  torch's LeakyReLU takes
    the slope 0.2 at z = 0; the kernel takes 1 at +0 AND at -0 (``z >= 0``): the +-0 entries pin that convention."""
    prec = prec_of(pname)
    for rot in R.act_bwd_rotations(nvec):
        P = R.act_bwd_problem(nvec, pname, rot)
        dz, z = P["dz"].to(DEV), P["z"].to(DEV)
        for act in (R.ACT_NONE, R.ACT_RELU, R.ACT_LRELU):
            g = Guarded(dz.numel(), prec.dtype)
            assert lib.dei2i_act_bwd(prec.code, dz.numel(), ptr(dz), ptr(z), act, g.ptr, stream()) == 0
            sync()
            g.check(R.act_bwd_ref(P, act, pname))


@pytest.mark.parametrize("pname", DTYPES)
def test_act_bwd_refusals(lib, pname):
    prec, vec = prec_of(pname), VEC[pname]
    t = torch.ones(4 * vec, dtype=prec.dtype, device=DEV)
    for n, dzp, zp, null_g in [(0, t, t, False), (vec + 1, t, t, False), (vec - 1, t, t, False), (vec, None, t, False), (vec, t, None, False),
                               (vec, t, t, True)]:
        g = Guarded(4 * vec, prec.dtype)
        assert lib.dei2i_act_bwd(prec.code, n, ptr(dzp), ptr(zp), R.ACT_LRELU, None if null_g else g.ptr, stream()) == BAD_ARG
        sync()
        g.untouched()


# ---- dei2i_affine_act_img_fwd -----------------------------------------------------------------------------------------------------
def run_affine_img(lib, prec, P, slope):
    n, hw, c = P["x"].shape
    xd, A, B = P["x"].to(DEV), P["A"].to(DEV), P["B"].to(DEV)
    out = Guarded(xd.numel(), prec.dtype)
    assert lib.dei2i_affine_act_img_fwd(prec.code, n, hw, c, ptr(xd), ptr(A), ptr(B), slope, out.ptr, stream()) == 0
    sync()
    return out


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", R.IMG_SHAPES, ids=str)
def test_affine_act_img_bit_exact_on_dyadic_data(lib, shape, pname):
    """x integers in [-8, 8], A in {1, 2, -1, 0.5}, B in {+-0.5, +-1.5} per (image, channel), slope in {0, 0.25, 1}: every intermediate
    has at most 8 significant bits and none is 0, so the output equals the float64 reference in bf16 and in fp32"""
    prec, P = prec_of(pname), R.img_problem(shape, pname)
    for slope in R.IMG_SLOPES:
        run_affine_img(lib, prec, P, slope).check(R.act64(P["pre64"], slope).to(prec.dtype))


@pytest.mark.parametrize("pname", DTYPES)
def test_affine_act_img_at_the_real_slope(lib, pname):
    prec, shape = prec_of(pname), (2, 7, 2)
    P = R.img_problem(shape, pname, exact=False)
    got = run_affine_img(lib, prec, P, 0.2).values(P["x"].shape)
    pre32 = P["A"][:, None, :] * P["x"].float() + P["B"][:, None, :]
    within(got, R.act64(P["pre64"], 0.2), f"affine_act_img {pname} {shape} slope 0.2", cpu32=R.act64(pre32, 0.2))


@pytest.mark.parametrize("pname", DTYPES)
def test_affine_act_img_refusals(lib, pname):
    prec, vec = prec_of(pname), VEC[pname]
    x = torch.ones(2 * 257 * vec, dtype=prec.dtype, device=DEV)
    co = torch.ones(2 * 257 * vec, dtype=torch.float32, device=DEV)
    for n, hw, c, nulls in [(1, 2, 3 * vec, ()), (1, 1, 257 * vec, ()), (1, 2, vec + 1, ()), (0, 2, vec, ()), (1, 0, vec, ()),
                            (1, 2, vec, ("x",)), (1, 2, vec, ("A",)), (1, 2, vec, ("B",)), (1, 2, vec, ("out",))]:
        out = Guarded(257 * vec, prec.dtype)
        rc = lib.dei2i_affine_act_img_fwd(prec.code, n, hw, c, None if "x" in nulls else ptr(x), None if "A" in nulls else ptr(co),
                                          None if "B" in nulls else ptr(co), 0.2, None if "out" in nulls else out.ptr, stream())
        assert rc == BAD_ARG, (n, hw, c, nulls)
        sync()
        out.untouched()


@pytest.mark.parametrize("pname", DTYPES)
def test_instance_norm_act_with_three_channel_vectors_takes_the_grouped_kernel(pname):
    """C = 3 VEC: cv = 3 neither divides 256 nor is divided by it, dei2i_affine_act_img_fwd refuses it (above) and the wrapper goes
    through dei2i_affine_act_fwd with one group per image; the output still matches float64 at test_reduce_edges_gpu.py's bound"""
    from de_i2i_gan_amd import ops
    from test_reduce_edges_gpu import TOL, relmax
    n, h, w, c = 2, 5, 6, 3 * VEC[pname]
    assert 256 % (c // VEC[pname]) != 0
    x = R.rounded(torch.randn(n, h, w, c, generator=R.gen(17)) * 1.7 + 0.4, pname)
    ref = F.leaky_relu(F.instance_norm(x.double().permute(0, 3, 1, 2), eps=1e-5), 0.2).permute(0, 2, 3, 1)
    got = ops.instance_norm_act(x.to(DEV, TORCH_DTYPE[pname]), "leaky_relu")
    e = relmax(got, ref)
    e32 = relmax(F.leaky_relu(F.instance_norm(x.permute(0, 3, 1, 2), eps=1e-5), 0.2).permute(0, 2, 3, 1), ref)
    note(f"instance_norm_act {pname} C = 3 VEC: kernel {e:.3e}, fp32 CPU {e32:.3e} of the output's max (tol {TOL[pname]:.1e})")
    assert e < TOL[pname]


# ---- the generator's head ---------------------------------------------------------------------------------------------------------
def compose_forward(lib, prec, pname, P, cs):
    n, h, w, _ = P["raw4"].shape
    raw, x = R.compose_raw(P, cs, pname, R.PAD_FILL).to(DEV), P["x"].to(DEV)
    out, prob = Guarded(n * 3 * h * w, torch.float32), Guarded(n * h * w, torch.float32)
    assert lib.dei2i_compose_fwd(prec.code, n, h, w, cs, ptr(raw), ptr(x), out.ptr, prob.ptr, stream()) == 0
    sync()
    return out.values((n, 3, h, w)), prob.values((n, 1, h, w))


def compose_backward(lib, prec, pname, P, cs, d_out=True, d_prob=True, d_x=True):
    n, h, w, _ = P["raw4"].shape
    raw, x = R.compose_raw(P, cs, pname).to(DEV), P["x"].to(DEV)
    go, gp = P["go"].to(DEV), P["gp"].to(DEV)
    d_raw, dx = Guarded(n * h * w * cs, prec.dtype), Guarded(n * 3 * h * w, torch.float32)
    rc = lib.dei2i_compose_bwd(prec.code, n, h, w, cs, ptr(raw), ptr(x), ptr(go) if d_out else None, ptr(gp) if d_prob else None,
                               d_raw.ptr, dx.ptr if d_x else None, stream())
    assert rc == 0
    sync()
    return d_raw.values((n, h, w, cs)), dx


def check_d_raw(d_raw, ref, P, what, cpu32):
    """channels 0..3 within the bound of the compute dtype, the padded channels +0.0 bit for bit; where channel 3 of raw is +-100 the
    sigmoid is exactly 0 or 1 and its gradient exactly 0, and under p = 0 the foreground's gradient as well"""
    assert not bits(d_raw[..., 4:]).any(), what + ": a padded channel of d_raw is not +0.0"
    within(d_raw[..., :4], ref, what + " d_raw", cpu32=cpu32)
    r3 = P["raw4"][..., 3]
    assert (d_raw[..., 3][r3.abs() == 100].float() == 0).all()
    assert (d_raw[..., :3][r3 == -100].float() == 0).all()


@pytest.mark.parametrize("csmul", [1, 2])
@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("shape", R.COMPOSE_SHAPES, ids=str)
def test_compose_forward_and_backward(lib, shape, pname, csmul):
    prec, P = prec_of(pname), R.compose_problem(shape, pname)
    cs, tag = csmul * VEC[pname], f"compose {pname} {shape} Cs = {csmul} VEC"
    out, prob = compose_forward(lib, prec, pname, P, cs)              # the padded channels of raw hold +-3e4: they must not reach out
    within(out, P["f64"]["out"], tag + " out", cpu32=P["f32"]["out"])
    within(prob, P["f64"]["prob"], tag + " prob", cpu32=P["f32"]["prob"])
    r3 = P["raw4"][..., 3].reshape(prob.shape)
    assert (prob[r3 == -100] == 0).all() and (prob[r3 == 100] == 1).all()
    d_raw, dx = compose_backward(lib, prec, pname, P, cs)
    check_d_raw(d_raw, P["f64"]["both"][0], P, tag, P["f32"]["both"][0])
    within(dx.values(P["x"].shape), P["f64"]["both"][1], tag + " d_x", cpu32=P["f32"]["both"][1])


@pytest.mark.parametrize("pname", DTYPES)
def test_compose_backward_nullable_pointers(lib, pname):
    prec, shape = prec_of(pname), (3, 9, 7)
    P = R.compose_problem(shape, pname)
    cs = VEC[pname]
    for key, kw in (("no_dout", dict(d_out=False)), ("no_dprob", dict(d_prob=False))):
        d_raw, dx = compose_backward(lib, prec, pname, P, cs, **kw)
        check_d_raw(d_raw, P["f64"][key][0], P, f"compose {pname} {key}", P["f32"][key][0])
        within(dx.values(P["x"].shape), P["f64"][key][1], f"compose {pname} {key} d_x", cpu32=P["f32"][key][1])
    d_raw, dx = compose_backward(lib, prec, pname, P, cs, d_x=False)
    check_d_raw(d_raw, P["f64"]["both"][0], P, f"compose {pname} no d_x", P["f32"]["both"][0])
    dx.untouched()


@pytest.mark.parametrize("pname", DTYPES)
def test_compose_refusals(lib, pname):
    prec, vec = prec_of(pname), VEC[pname]
    raw = torch.zeros(2 * 2 * 2 * 2 * vec, dtype=prec.dtype, device=DEV)
    f = torch.zeros(64, dtype=torch.float32, device=DEV)
    small = 0 if pname == "f32" else 4                                # Cs < 4 is only reachable with Cs = 0; bf16's 4 fails Cs % VEC
    for n, h, w, cs, null in [(1, 2, 2, small, None), (1, 2, 2, vec + 1, None), (1, 2, 2, vec - 1, None), (0, 2, 2, vec, None),
                              (1, 0, 2, vec, None), (1, 2, 0, vec, None), (1, 2, 2, vec, "raw"), (1, 2, 2, vec, "x_in"),
                              (1, 2, 2, vec, "out"), (1, 2, 2, vec, "prob"), (1, 2, 2, vec, "d_raw")]:
        out, prob = Guarded(64, torch.float32), Guarded(64, torch.float32)
        d_raw, dx = Guarded(128, prec.dtype), Guarded(64, torch.float32)
        rp, xp = (None if null == "raw" else ptr(raw)), (None if null == "x_in" else ptr(f))
        if null != "d_raw":
            rc = lib.dei2i_compose_fwd(prec.code, n, h, w, cs, rp, xp, None if null == "out" else out.ptr,
                                       None if null == "prob" else prob.ptr, stream())
            assert rc == BAD_ARG, (n, h, w, cs, null)
        if null not in ("out", "prob"):
            rc = lib.dei2i_compose_bwd(prec.code, n, h, w, cs, rp, xp, ptr(f), ptr(f), None if null == "d_raw" else d_raw.ptr, dx.ptr, stream())
            assert rc == BAD_ARG, (n, h, w, cs, null)
        sync()
        for g in (out, prob, d_raw, dx):
            g.untouched()


@pytest.mark.parametrize("pname", DTYPES)
def test_compose_through_the_wrapper(pname):
    """ops.compose at (3, 9, 7): the same bounds; an x_in that does not require a gradient gets none"""
    from de_i2i_gan_amd import ops
    shape = (3, 9, 7)
    P = R.compose_problem(shape, pname)
    go, gp = P["go"].to(DEV), P["gp"].to(DEV)
    for x_grad in (True, False):
        raw = R.compose_raw(P, VEC[pname], pname).to(DEV).requires_grad_(True)
        x = P["x"].to(DEV).requires_grad_(x_grad)
        out, prob = ops.compose(raw, x)
        within(out.detach().cpu(), P["f64"]["out"], f"ops.compose {pname} out", cpu32=P["f32"]["out"])
        within(prob.detach().cpu(), P["f64"]["prob"], f"ops.compose {pname} prob", cpu32=P["f32"]["prob"])
        torch.autograd.backward([out, prob], [go, gp])
        check_d_raw(raw.grad.cpu(), P["f64"]["both"][0], P, f"ops.compose {pname} x_grad={x_grad}", P["f32"]["both"][0])
        if x_grad:
            within(x.grad.cpu(), P["f64"]["both"][1], f"ops.compose {pname} d_x", cpu32=P["f32"]["both"][1])
        else:
            assert x.grad is None


# ---- the NaN guard ----------------------------------------------------------------------------------------------------------------
def guard_call(lib, prec, x, flag):
    buf = Guarded(x.numel(), prec.dtype, fill=x)
    assert lib.dei2i_nan_guard(prec.code, x.numel(), buf.ptr, ptr(flag), stream()) == 0
    sync()
    return buf


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("nvec", R.NAN_CLEAN_NVEC)
def test_nan_guard_leaves_infinities_alone_without_a_nan(lib, nvec, pname):
    """the reference applies nan_to_num only if a NaN is present (generator.py:266-267): +-inf, -0.0, a subnormal and +-max pass
    bit-unchanged through a tensor that has none -- also right after a tensor that had one (the flag is reset by every call)"""
    prec = prec_of(pname)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    x, want = R.nan_guard_data(nvec, pname, None)
    assert torch.equal(bits(x), bits(want))
    guard_call(lib, prec, x, flag).check(want)
    dirty, dirty_want = R.nan_guard_data(min(nvec, 257), pname, "element0", seed=1)
    guard_call(lib, prec, dirty, flag).check(dirty_want)
    guard_call(lib, prec, x, flag).check(want)                        # dirty, then clean


@pytest.mark.parametrize("pname", DTYPES)
@pytest.mark.parametrize("case", R.NAN_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_nan_guard_with_one_nan(lib, case, pname):
    """one NaN wherever a thread, wavefront, workgroup or grid-stride trip could lose it: NaN -> +0.0, +-inf -> +-max of the dtype, every
    other element (-0.0 and the subnormal included) bit-unchanged"""
    prec = prec_of(pname)
    nvec, placement = case
    x, want = R.nan_guard_data(nvec, pname, placement)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    guard_call(lib, prec, x, flag).check(want)


@pytest.mark.parametrize("pname", DTYPES)
def test_nan_guard_through_the_wrapper_shares_one_flag(pname):
    from de_i2i_gan_amd import ops
    dirty, dirty_want = R.nan_guard_data(257, pname, "thread255")
    clean, clean_want = R.nan_guard_data(255, pname, None)
    for _ in range(2):
        d, c = dirty.to(DEV), clean.to(DEV)
        assert ops.nan_guard_(d) is d and ops.nan_guard_(c) is c
        assert torch.equal(bits(d).cpu(), bits(dirty_want)) and torch.equal(bits(c).cpu(), bits(clean_want))
    assert len([k for k in ops._nan_flags if k == d.device]) == 1


@pytest.mark.parametrize("pname", DTYPES)
def test_nan_guard_refusals(lib, pname):
    prec, vec = prec_of(pname), VEC[pname]
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    for n, null in [(0, None), (vec + 1, None), (vec - 1, None), (vec, "flag"), (vec, "x")]:
        buf = Guarded(4 * vec, prec.dtype)
        assert lib.dei2i_nan_guard(prec.code, n, None if null == "x" else buf.ptr, None if null == "flag" else ptr(flag), stream()) == BAD_ARG
        sync()
        buf.untouched()
