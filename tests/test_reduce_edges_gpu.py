"""The norm, reduction and loss kernels of csrc/reduce.hip at their structural boundaries, against plain float64 torch on the CPU.

Every kernel there has the same seams: the tensor is viewed as (rows, C) and cut into ``ceil(rows / chunks)``-row chunks
(dei2i_moments_chunks: HW / 64 capped at 64 per image; dei2i_bn_bwd_chunks: pixels / 64 capped at 2048; dei2i_colsum_blocks:
rows / 256 capped at 256), a 256-thread workgroup splits into ``cv = C / VEC`` vector columns (VEC 8 in bf16, 4 in f32) by
``rpp = 256 / cv`` row-threads, the main loop is unrolled (x4 or x2) in front of a tail, the records are combined by a finalize
workgroup of 64 threads -- or 256 when there are more than 256 records -- and the element-wise grids are capped and fall back to
grid-stride loops.  The shape tables below sit ON those seams; the boundary each shape reaches is named beside it.  A change to a
chunk size or a grid cap has to move these tables on purpose.

Conventions: the reference is float64 torch on the CPU, evaluated on operands rounded to the compute dtype (the ``rounded()``
idiom of test_ops_gpu.py) -- never a second GPU path.  Inputs differ per row and per channel and the upstream gradients are
random, so a dropped or doubled row moves a result by more than its tolerance.  Tolerances are the project's: TOL of the tensor's
max for outputs and input gradients, x2 for parameter gradients, 1e-4 (+5e-3 in bf16) for running statistics, test_losses' for the
losses, 2e-5 for the noise weight.  Activation kinks: the backward recomputes the pre-activation in fp32, so an element whose
reference pre-activation lies within 1e-4 of the tensor's max of zero may take the other branch; those elements (asserted to be
fewer than 0.1 %) are left out of the max-error check and stay in a relative-L2 check (1e-3 f32, 3e-2 bf16)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-4, "bf16": 1.5e-2}
L2TOL = {"f32": 1e-3, "bf16": 3e-2}
KINK_BAND, KINK_SHARE = 1e-4, 1e-3
PNAMES = ["f32", "bf16"]


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


def dev():
    return torch.device("cuda:0")


def note(*a):
    print("[reduce-edges]", *a, flush=True)


def _dtype(pname):
    return torch.bfloat16 if pname == "bf16" else torch.float32


def _vec(pname):
    return 8 if pname == "bf16" else 4


def rounded(t, pname):
    return t.to(torch.bfloat16).float() if pname == "bf16" else t


def data(shape, seed, scale=1.7, shift=0.4):
    """(N,H,W,C) -> NCHW fp32: another value per row, another scale and shift per channel"""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, c, h, w, generator=g) * scale + shift
    ch = torch.arange(c, dtype=torch.float32)
    return t * (1 + 0.05 * (ch % 7)).view(1, c, 1, 1) + (0.1 * (ch % 5) - 0.2).view(1, c, 1, 1)


def vecs(c, seed):
    """per-channel weight, bias, running mean, running var -- all different per channel"""
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.2 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g),
            1 + 0.1 * torch.rand(c, generator=g))


def to_dev(t_nchw, pname, cs=None):
    """NCHW fp32 cpu -> NHWC compute-dtype GPU tensor, channels zero-padded to ``cs``"""
    n, c, h, w = t_nchw.shape
    cs = cs or c
    out = torch.zeros(n, h, w, cs)
    out[..., :c] = t_nchw.permute(0, 2, 3, 1)
    return out.to(dev(), _dtype(pname))


def back(t_nhwc, c=None):
    """NHWC GPU tensor -> NCHW float64 cpu (the first ``c`` channels)"""
    t = t_nhwc.detach().double().cpu().permute(0, 3, 1, 2)
    return t if c is None else t[:, :c]


def relmax(got, ref, keep=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = (got - ref).abs()
    if keep is not None:
        d = d[keep]
    return (d.max() / ref.abs().max().clamp_min(1e-12)).item()


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-12)).item()


def kink_keep(pre, act):
    """Elements whose reference pre-activation is clear of the kink (all of them without an activation); the excluded share is a
    condition of the test: below 0.1 %."""
    if act in ("none", None):
        return None
    pre = pre.detach()
    band = pre.abs() < KINK_BAND * pre.abs().max()
    share = band.double().mean().item()
    assert share < KINK_SHARE, f"{share:.2e} of the pre-activations lie in the kink band"
    return ~band


def check_grad(got, ref, keep, pname, what, tol=None):
    tol = TOL[pname] if tol is None else tol
    e, l2 = relmax(got, ref, keep), rel_l2(got, ref)
    note(f"{what}: max {e:.3e} (tol {tol:.1e})  relL2 {l2:.3e}")
    assert e < tol, (what, e)
    assert l2 < L2TOL[pname], (what, l2)
    return e


def act64(v, act):
    return F.leaky_relu(v, 0.2) if act == "leaky_relu" else (torch.relu(v) if act == "relu" else v)


# ======================================================================================================================
# 1. BatchNorm forward and backward
# ======================================================================================================================
# (N, H, W, C): what it reaches
BN_SHAPES = [
    (2, 9, 14, 16),      # HW = 126: one moments chunk per image (the smallest of the three; one row less -- HW 125 -- moves the
                         #           batch mean by |x| / 252 ~ 7e-3 of the output's max: 35x the f32 tolerance)
    (2, 8, 16, 16),      # HW = 128: exactly two chunks of 64 rows
    (2, 10, 13, 16),     # HW = 130: two ragged chunks (65 + 65), 260 pixels = 4 backward chunks
    (1, 3, 5, 8),        # 15 rows: fewer rows than rpp; N = 1; cv = 1 in bf16 (rpp = 256), cv = 2 in f32
    (3, 7, 11, 24),      # cv = 3 in bf16 (rpp = 85, thread 255 idle, bn_bwd_apply_kernel<.., false>); cv = 6 in f32 (rpp = 42)
    (2, 6, 6, 136),      # cv = 17 in bf16 (rpp = 15), 34 in f32 (rpp = 7): neither divides 256
    (5, 64, 64, 8),      # 64 chunks x 5 images = 320 forward records and 20480 pixels = 320 backward chunks: 256-thread combine
    (2, 64, 65, 8),      # HW = 4160: the 64-chunk cap with ragged chunks of 65 rows
    (2, 256, 260, 8),    # 133120 pixels: above the 2048-chunk cap of dei2i_bn_bwd_chunks (65 rows per chunk, ragged last)
]
# the largest C that cv_ok admits (cv = 256, rpp = 1) -- per dtype
BN_WIDEST = {"bf16": (2, 8, 8, 2048), "f32": (2, 8, 8, 1024)}


def _bn_train_cases():
    cases = [pytest.param(p, s, id=f"{p}-{'x'.join(map(str, s))}") for p in PNAMES for s in BN_SHAPES]
    cases += [pytest.param(p, s, id=f"{p}-{'x'.join(map(str, s))}-widest") for p, s in BN_WIDEST.items()]
    return cases


def clear_of_kinks(make, act, seed):
    """make(seed) for the first seed (seed, seed + 100, ...) whose reference pre-activations leave fewer than half the permitted share
    inside the kink band: a condition on the inputs alone (the kernels are not consulted), so that kink_keep's cap holds with margin"""
    for s in range(seed, seed + 2000, 100):
        P = make(s)
        pre = P["pre"]
        if act in ("none", None) or (pre.abs() < KINK_BAND * pre.abs().max()).double().mean().item() < KINK_SHARE / 2:
            return P
    raise AssertionError("no input draw clear of the kink band")


@functools.lru_cache(maxsize=None)
def _bn_problem(pname, shape, act, with_res, training, seed=3):
    """inputs and the float64 reference of one batchnorm_act call (computed once per case, never modified)"""
    return clear_of_kinks(lambda s: _bn_make(pname, shape, act, with_res, training, s), act, seed)


def _bn_make(pname, shape, act, with_res, training, seed):
    n, h, w, c = shape
    y, g = data(shape, seed), data(shape, seed + 2, 1.0, 0.0)
    res = data(shape, seed + 1, 1.0, 0.1) if with_res else None
    wt, bs, rm, rv = vecs(c, seed + 3)
    yr = rounded(y, pname).double().requires_grad_(True)
    rr = rounded(res, pname).double().requires_grad_(True) if with_res else None
    w64, b64 = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    pre = F.batch_norm(yr, rm64, rv64, w64, b64, training, 0.1, 1e-5)       # updates rm64 / rv64 (unbiased variance) in training
    out = act64(pre, act)
    if with_res:
        out = out + rr
    grads = torch.autograd.grad(out, [yr, w64, b64], rounded(g, pname).double())
    return dict(y=y, g=g, res=res, wt=wt, bs=bs, rm=rm, rv=rv, out=out.detach(), pre=pre.detach(), dy=grads[0], dw=grads[1], db=grads[2],
                rm_ref=rm64, rv_ref=rv64)


def _run_bn(ops, pname, shape, act, with_res, training):
    P = _bn_problem(pname, shape, act, with_res, training)
    n, h, w, c = shape
    wg, bg = P["wt"].to(dev()).requires_grad_(True), P["bs"].to(dev()).requires_grad_(True)
    rm, rv = P["rm"].to(dev()), P["rv"].to(dev())
    nbt = torch.zeros((), dtype=torch.int64, device=dev())
    yg = to_dev(P["y"], pname).requires_grad_(True)
    resg = to_dev(P["res"], pname).requires_grad_(True) if with_res else None
    out = ops.batchnorm_act(yg, wg, bg, rm, rv, training, act, resg, num_batches_tracked=nbt)
    gg = to_dev(P["g"], pname)
    out.backward(gg)
    tag = f"bn {pname} {shape} {act} res={with_res} train={training}"
    tol = TOL[pname]
    e = relmax(back(out), P["out"])
    note(f"{tag} out: max {e:.3e} (tol {tol:.1e})")
    assert e < tol
    keep = kink_keep(P["pre"], act)
    check_grad(back(yg.grad), P["dy"], keep, pname, tag + " dy")
    ew, eb = relmax(wg.grad, P["dw"]), relmax(bg.grad, P["db"])
    note(f"{tag} dweight {ew:.3e} dbias {eb:.3e} (tol {2 * tol:.1e})")
    assert wg.grad.shape == (c,) and bg.grad.shape == (c,)
    assert ew < 2 * tol and eb < 2 * tol
    if with_res:
        assert torch.equal(resg.grad, gg)                                 # the residual's gradient is the upstream gradient
    if training:
        rtol = 1e-4 + (5e-3 if pname == "bf16" else 0)
        em, ev = relmax(rm, P["rm_ref"]), relmax(rv, P["rv_ref"])
        note(f"{tag} running mean {em:.3e} var {ev:.3e} (tol {rtol:.1e})")
        assert em < rtol and ev < rtol
        assert int(nbt.item()) == 1
    else:
        assert torch.equal(rm.cpu(), P["rm"]) and torch.equal(rv.cpu(), P["rv"]) and int(nbt.item()) == 0


@pytest.mark.parametrize("pname,shape", _bn_train_cases())
def test_batchnorm_leaky_relu_at_chunk_and_column_boundaries(ops, pname, shape):
    """ops.batchnorm_act, training mode + LeakyReLU: output, dy, dweight, dbias and the running statistics at every shape of the
    table against float64 F.batch_norm on the rounded input."""
    _run_bn(ops, pname, shape, "leaky_relu", False, True)


@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("shape", [(2, 10, 13, 16),      # two ragged moments chunks
                                   (3, 7, 11, 24)])      # cv = 3 / 6: the non-invariant apply kernels, forward and backward
def test_batchnorm_without_activation_with_residual(ops, pname, shape):
    _run_bn(ops, pname, shape, "none", True, True)


@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("shape", [(3, 7, 11, 24),       # cv = 3 / 6: bn_bwd_apply_kernel<.., false> with c2 = c3 = 0
                                   (2, 64, 65, 8)])      # 8320 pixels = 130 backward chunks of 64 rows
def test_batchnorm_eval_mode(ops, pname, shape):
    """Eval mode: running statistics normalise, dy = a * g * act', the running buffers and the counter stay untouched."""
    _run_bn(ops, pname, shape, "leaky_relu", False, False)


@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("shape", [(4, 8, 16, 16),       # two images per group, HW = 128: two chunks per image
                                   (6, 9, 14, 24)])      # three images per group, cv = 3 / 6, one chunk per image
def test_batchnorm_groups_against_float64_per_half(ops, pname, shape):
    """ops.bn_batch_groups(2) against float64 BatchNorm applied to each half of the batch on its own: outputs, dy, dweight / dbias
    summed over the groups, and the running statistics after the two replayed updates."""
    n, h, w, c = shape

    def make(seed):
        y, g = data(shape, seed), data(shape, seed + 1, 1.0, 0.0)
        wt, bs, rm0, rv0 = vecs(c, seed + 2)
        yr = rounded(y, pname).double().requires_grad_(True)
        w64, b64 = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
        rm64, rv64 = rm0.double().clone(), rv0.double().clone()
        pre = torch.cat([F.batch_norm(yr[k * (n // 2):(k + 1) * (n // 2)], rm64, rv64, w64, b64, True, 0.1, 1e-5) for k in range(2)], 0)
        grads = torch.autograd.grad(F.leaky_relu(pre, 0.2), [yr, w64, b64], rounded(g, pname).double())
        return dict(y=y, g=g, vecs=(wt, bs, rm0, rv0), pre=pre.detach(), grads=grads, running=(rm64, rv64))

    P = clear_of_kinks(make, "leaky_relu", 21)
    y, g, pre, (dy, dw, db), (rm64, rv64), (wt, bs, rm0, rv0) = P["y"], P["g"], P["pre"], P["grads"], P["running"], P["vecs"]
    out_ref = F.leaky_relu(pre, 0.2)

    wg, bg = wt.to(dev()).requires_grad_(True), bs.to(dev()).requires_grad_(True)
    rm, rv = rm0.to(dev()), rv0.to(dev())
    yg = to_dev(y, pname).requires_grad_(True)
    with ops.bn_running_deferred() as running:
        with ops.bn_batch_groups(2):
            running.pass_index = (0, 1)
            out = ops.batchnorm_act(yg, wg, bg, rm, rv, True, "leaky_relu")
        running.apply()
    out.backward(to_dev(g, pname))
    tag, tol = f"bn groups {pname} {shape}", TOL[pname]
    e = relmax(back(out), out_ref)
    note(f"{tag} out {e:.3e}")
    assert e < tol
    check_grad(back(yg.grad), dy, kink_keep(pre, "leaky_relu"), pname, tag + " dy")
    ew, eb = relmax(wg.grad, dw), relmax(bg.grad, db)
    note(f"{tag} dweight {ew:.3e} dbias {eb:.3e}")
    assert ew < 2 * tol and eb < 2 * tol
    rtol = 1e-4 + (5e-3 if pname == "bf16" else 0)
    em, ev = relmax(rm, rm64), relmax(rv, rv64)
    note(f"{tag} running mean {em:.3e} var {ev:.3e}")
    assert em < rtol and ev < rtol


@pytest.mark.parametrize("pname", PNAMES)
def test_batchnorm_parameters_used_twice_accumulate(ops, pname):
    """One pair of BatchNorm parameters in two batchnorm_act calls of one graph (the second backward node adds into the first
    one's gradient inside bn_bwd_finalize_kernel), on a chunk-crossing shape: dweight / dbias against the float64 sum."""
    shape = (2, 10, 13, 16)                                  # HW = 130: two ragged chunks; 260 pixels: four backward chunks
    n, h, w, c = shape
    y1, y2, g1, g2 = data(shape, 31), data(shape, 32, 1.1, -0.3), data(shape, 33, 1.0, 0.0), data(shape, 34, 1.0, 0.0)
    wt, bs, rm0, rv0 = vecs(c, 35)
    w64, b64 = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    rm64, rv64 = rm0.double().clone(), rv0.double().clone()
    yr1, yr2 = (rounded(t, pname).double().requires_grad_(True) for t in (y1, y2))
    o1 = F.leaky_relu(F.batch_norm(yr1, rm64, rv64, w64, b64, True, 0.1, 1e-5), 0.2)
    o2 = F.leaky_relu(F.batch_norm(yr2, rm64, rv64, w64, b64, True, 0.1, 1e-5), 0.2)
    loss = (o1 * rounded(g1, pname).double()).sum() + (o2 * rounded(g2, pname).double()).sum()
    dw, db = torch.autograd.grad(loss, [w64, b64])

    wg, bg = wt.to(dev()).requires_grad_(True), bs.to(dev()).requires_grad_(True)
    rm, rv = rm0.to(dev()), rv0.to(dev())
    a1 = ops.batchnorm_act(to_dev(y1, pname).requires_grad_(True), wg, bg, rm, rv, True, "leaky_relu")
    a2 = ops.batchnorm_act(to_dev(y2, pname).requires_grad_(True), wg, bg, rm, rv, True, "leaky_relu")
    torch.autograd.backward([a1, a2], [to_dev(g1, pname), to_dev(g2, pname)])
    ew, eb = relmax(wg.grad, dw), relmax(bg.grad, db)
    note(f"bn accumulate {pname}: dweight {ew:.3e} dbias {eb:.3e}")
    assert ew < 2 * TOL[pname] and eb < 2 * TOL[pname]
    rtol = 1e-4 + (5e-3 if pname == "bf16" else 0)
    assert relmax(rm, rm64) < rtol and relmax(rv, rv64) < rtol


def small_ints(shape, seed, lo=1, hi=8, signed=False):
    """(N,H,W,C) -> NCHW fp32 of integers in [lo, hi] (or +-[lo, hi]): exact in bf16, and every partial sum of them (and of their
    squares) stays an integer below 2^24, i.e. exact in fp32 in ANY summation order"""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, (n, c, h, w), generator=g).float()
    return t * (torch.randint(0, 2, (n, c, h, w), generator=g).float() * 2 - 1) if signed else t


@pytest.mark.parametrize("pname,shape", _bn_train_cases())
def test_batchnorm_statistics_and_dbias_of_integer_data_are_exact(ops, pname, shape):
    """The project's tolerances cannot see ONE dropped or doubled row at the large shapes (one row of 133120 moves the mean by
    1e-6 of it).  Integer data can: y in [1, 8] and an upstream gradient in +-[1, 4] make sum y, sum y^2 and sum g exact in fp32 in
    any order (all below 2^24), so with momentum = 1 the running mean / variance are the float64 statistics rounded once (the
    kernel combines in fp64; bound 2^-22 relative: two roundings) and dbias (no activation) EQUALS sum g.  One row less moves the
    mean by at least 0.5 / pixels, 8e-7 of it at 133120 pixels: 3.5 times the bound; dbias by at least 1."""
    n, h, w, c = shape
    assert 64 * n * h * w < 2 ** 24
    y, g = small_ints(shape, 71), small_ints(shape, 72, 1, 4, signed=True)
    wg, bg = torch.ones(c, device=dev()).requires_grad_(True), torch.zeros(c, device=dev()).requires_grad_(True)
    rm, rv = torch.zeros(c, device=dev()), torch.ones(c, device=dev())
    yg = to_dev(y, pname).requires_grad_(True)
    out = ops.batchnorm_act(yg, wg, bg, rm, rv, True, "none", momentum=1.0)
    out.backward(to_dev(g, pname))
    mean, var = y.double().mean(dim=(0, 2, 3)), y.double().var(dim=(0, 2, 3), unbiased=True)
    em = ((rm.double().cpu() - mean).abs() / mean).max().item()
    ev = ((rv.double().cpu() - var).abs() / var).max().item()
    note(f"bn integers {pname} {shape}: running mean {em:.3e} var {ev:.3e} (bound {2.0 ** -22:.2e})")
    assert em <= 2.0 ** -22 and ev <= 2.0 ** -22
    assert torch.equal(bg.grad.double().cpu(), g.double().sum(dim=(0, 2, 3))), "dbias of integer gradients must be exact"


def _offset_input(shape, seed):
    """mean = 8 * std per channel: E[x^2] - mean^2 loses 6 bits"""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    std = (0.5 + 0.25 * torch.arange(c, dtype=torch.float32)).view(1, c, 1, 1)
    return torch.randn(n, c, h, w, generator=g) * std + 8.0 * std


def test_batchnorm_variance_cancellation_f32(ops):
    """E[x^2] - mean^2 from fp32 partial sums with mean = 8 std, at (2, 64, 65, 8) in f32: rstd, read through the output of an
    act="none" call, against float64 -- allowed 4x the error of torch's own float32 CPU batch_norm on the same input, and never
    less than the project's 2e-4."""
    shape = (2, 64, 65, 8)
    c = shape[3]
    y = _offset_input(shape, 41)
    ref = F.batch_norm(y.double(), None, None, None, None, True, 0.1, 1e-5)
    e32 = relmax(F.batch_norm(y, None, None, None, None, True, 0.1, 1e-5), ref)
    wg, bg = torch.ones(c, device=dev()), torch.zeros(c, device=dev())
    rm, rv = torch.zeros(c, device=dev()), torch.ones(c, device=dev())
    out = ops.batchnorm_act(to_dev(y, "f32"), wg, bg, rm, rv, True, "none")
    e = relmax(back(out), ref)
    note(f"bn cancellation f32: kernel {e:.3e}  torch-f32 {e32:.3e}  ratio {e / max(e32, 1e-30):.2f}")
    # measured on MI355X: independent fp32 (torch CPU, two-pass variance) 1.55e-07, kernel 8.2e-07 -- ratio 5.3, the price of
    # E[x^2] - mean^2 at mean = 8 std (64x amplification of the fp32 partial sums' rounding, cut by the fp64 combine); 4 x 1.55e-07 is
    # below the project's 2e-4, which therefore is the bound: 240x headroom
    assert e < max(TOL["f32"], 4 * e32)


@pytest.mark.parametrize("pname", PNAMES)
def test_more_than_256_channel_vectors_are_refused(ops, pname):
    """cv > 256 is refused by design (DEI2I_ERR_BAD_ARG): the Python side raises, it does not compute garbage."""
    c = _vec(pname) * 257
    x = torch.zeros(1, 4, 4, c, dtype=_dtype(pname), device=dev())
    wg, bg, rm, rv = (torch.ones(c, device=dev()) for _ in range(4))
    with pytest.raises(RuntimeError, match="moments_partial"):
        ops.batchnorm_act(x, wg, bg, rm, rv, True, "none")
    with pytest.raises(RuntimeError, match="moments_partial"):
        ops.in_affine_act(x, torch.zeros(1, c, device=dev()), torch.zeros(1, c, device=dev()))


# ======================================================================================================================
# 2. InstanceNorm family
# ======================================================================================================================
IN_SHAPES = [
    (2, 4, 4, 16),       # class-mode minimum in H and W: top and bottom border classes meet, no interior row or column (one
                         #           pixel less of 16 moves the mean by |x| / 16: far above any tolerance)
    (1, 4, 9, 16),       # H = 4 only; N = 1
    (3, 9, 4, 8),        # W = 4 only; cv = 1 in bf16
    (2, 5, 5, 16),       # exactly one interior row and column
    (2, 5, 12, 16),      # exactly one interior row
    (2, 7, 5, 24),       # cv = 3 in bf16 (6 in f32): the dei2i_affine_act_fwd one-group-per-image fallback of the forward
    (2, 8, 16, 16),      # HW = 128: exactly two chunks
    (2, 9, 15, 16),      # HW = 135: two ragged chunks (68 + 67)
    (2, 64, 65, 8),      # HW = 4160: the 64-chunk cap, ragged chunks of 65 rows
    (1, 16, 16, 512),    # stargan-v2's bottleneck width; cv = 64 in bf16 and 128 in f32
    (3, 6, 10, 40),      # cv = 5 in bf16, 10 in f32: the fallback forward again, HW = 60 < 64
]


def _id(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def _in_problem(pname, shape, act, affine, with_res, cl=None, seed=5):
    """inputs and float64 reference of act(IN(x) * (1 + gamma) + beta) (+ res); ``cl``: logical channels (the rest stay zero)"""
    return clear_of_kinks(lambda s: _in_make(pname, shape, act, affine, with_res, cl, s), act, seed)


def _in_make(pname, shape, act, affine, with_res, cl, seed):
    n, h, w, c = shape
    cl = cl or c
    lshape = (n, h, w, cl)
    x, g = data(lshape, seed), data(lshape, seed + 1, 1.0, 0.0)
    res = data(lshape, seed + 2, 1.0, 0.1) if with_res else None
    gen = torch.Generator().manual_seed(seed + 3)
    gamma, beta = 0.3 * torch.randn(n, cl, generator=gen), 0.2 * torch.randn(n, cl, generator=gen) + 0.1
    xr = rounded(x, pname).double().requires_grad_(True)
    z = F.instance_norm(xr, eps=1e-5)
    P = dict(x=x, g=g, res=res, gamma=gamma, beta=beta)
    wrt = [xr]
    if affine:
        gm, bt = (rounded(t, pname).double().requires_grad_(True) for t in (gamma, beta))     # rounded as the op rounds them
        z = z * (1 + gm[:, :, None, None]) + bt[:, :, None, None]
        wrt += [gm, bt]
    out = act64(z, act)
    if with_res:
        out = out + rounded(res, pname).double()
    grads = torch.autograd.grad(out, wrt, rounded(g, pname).double())
    P.update(out=out.detach(), pre=z.detach(), dx=grads[0])
    if affine:
        P.update(dgamma=grads[1], dbeta=grads[2])
    return P


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("shape", IN_SHAPES, ids=_id)
@pytest.mark.parametrize("pname", PNAMES)
def test_instance_norm_act_at_class_and_chunk_boundaries(ops, pname, shape, with_res):
    """ops.instance_norm_act (LeakyReLU), with and without ``res``: output and dx against float64 F.instance_norm."""
    P = _in_problem(pname, shape, "leaky_relu", False, with_res)
    xg = to_dev(P["x"], pname).requires_grad_(True)
    resg = to_dev(P["res"], pname).requires_grad_(True) if with_res else None
    out = ops.instance_norm_act(xg, "leaky_relu", resg)
    gg = to_dev(P["g"], pname)
    out.backward(gg)
    tag = f"in {pname} {shape} res={with_res}"
    e = relmax(back(out), P["out"])
    note(f"{tag} out {e:.3e}")
    assert e < TOL[pname]
    check_grad(back(xg.grad), P["dx"], kink_keep(P["pre"], "leaky_relu"), pname, tag + " dx")
    if with_res:
        assert torch.equal(resg.grad, gg)


def _run_in_affine(ops, pname, shape, act, cl=None):
    n, h, w, c = shape
    cl = cl or c
    P = _in_problem(pname, shape, act, True, False, cl)
    xg = to_dev(P["x"], pname, c).requires_grad_(True)
    gmg, btg = P["gamma"].to(dev()).requires_grad_(True), P["beta"].to(dev()).requires_grad_(True)
    out = ops.in_affine_act(xg, gmg, btg, act)
    out.backward(to_dev(P["g"], pname, c))
    tag, tol = f"in_affine {pname} {shape} cl={cl} {act}", TOL[pname]
    e = relmax(back(out, cl), P["out"])
    note(f"{tag} out {e:.3e}")
    assert e < tol
    keep = kink_keep(P["pre"], act)
    check_grad(back(xg.grad, cl), P["dx"], keep, pname, tag + " dx")
    assert gmg.grad.shape == (n, cl) and btg.grad.shape == (n, cl)
    eg, eb = relmax(gmg.grad, P["dgamma"]), relmax(btg.grad, P["dbeta"])
    note(f"{tag} dgamma {eg:.3e} dbeta {eb:.3e} (tol {2 * tol:.1e})")
    assert eg < 2 * tol and eb < 2 * tol
    if cl < c:                                                # channel padding stays zero
        assert float(out.detach()[..., cl:].abs().max()) == 0.0 and float(xg.grad[..., cl:].abs().max()) == 0.0


@pytest.mark.parametrize("act", ["leaky_relu", "none", "relu"])
@pytest.mark.parametrize("shape", IN_SHAPES, ids=_id)
@pytest.mark.parametrize("pname", PNAMES)
def test_in_affine_act_at_class_and_chunk_boundaries(ops, pname, shape, act):
    """ops.in_affine_act (AdaIN / affine InstanceNorm of stargan-v2): output, dx, dgamma and dbeta -- the backward goes through
    the 5x5 border-class table (25 class gradients summed back to (N, C))."""
    _run_in_affine(ops, pname, shape, act)


@pytest.mark.parametrize("act", ["leaky_relu", "none", "relu"])
@pytest.mark.parametrize("pname", PNAMES)
def test_in_affine_act_gamma_narrower_than_the_channel_stride(ops, pname, act):
    """36 logical channels (gamma.shape[1] = 36) on a 40-wide activation (ctx.cl < c): the padded channels of out and dx stay
    zero, dgamma / dbeta come back 36 wide."""
    _run_in_affine(ops, pname, (3, 6, 10, 40), act, cl=36)


@pytest.mark.parametrize("shape", IN_SHAPES, ids=_id)
def test_in_affine_act_of_integer_data_f32(ops, shape):
    """The InstanceNorm counterpart of the integer-data BatchNorm test, in f32 (in bf16 the class table's gradient is stored in
    bf16): x in [1, 8], upstream gradient in +-[1, 4], no activation.  sum x and sum x^2 are exact, mean and rstd the float64 ones
    rounded once, so the output is within 16 * 2^-24 of its max of float64 (mean, rstd, A, B, the fma and the store: at most six
    roundings of terms up to |mean * rstd| ~ 2, against max |out| ~ 1.5) -- one row less of the 4160 of the largest shape moves it
    by 3e-5.  dbeta = sum g over the 25 border classes is a sum of integers: it EQUALS the float64 sum (one pixel less: >= 1)."""
    n, h, w, c = shape
    x, g = small_ints(shape, 73), small_ints(shape, 74, 1, 4, signed=True)
    gen = torch.Generator().manual_seed(75)
    gamma, beta = 0.3 * torch.randn(n, c, generator=gen), 0.2 * torch.randn(n, c, generator=gen)
    xg = to_dev(x, "f32").requires_grad_(True)
    gmg, btg = gamma.to(dev()).requires_grad_(True), beta.to(dev()).requires_grad_(True)
    out = ops.in_affine_act(xg, gmg, btg, "none")
    out.backward(to_dev(g, "f32"))
    ref = F.instance_norm(x.double(), eps=1e-5) * (1 + gamma.double()[:, :, None, None]) + beta.double()[:, :, None, None]
    e = relmax(back(out), ref)
    note(f"in_affine integers f32 {shape}: out {e:.3e} (bound {16 * 2.0 ** -24:.2e})")
    assert e <= 16 * 2.0 ** -24
    assert torch.equal(btg.grad.double().cpu(), g.double().sum(dim=(2, 3))), "dbeta of integer gradients must be exact"


@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("shape", [(2, 3, 5, 16), (2, 6, 2, 16)], ids=_id)
def test_in_affine_act_small_images_forward_only(ops, pname, shape):
    """H or W < 4: the forward still matches; the backward (class-mode kernels) raises the documented NotImplementedError."""
    n, h, w, c = shape
    P = _in_problem(pname, shape, "leaky_relu", True, False)
    xg = to_dev(P["x"], pname).requires_grad_(True)
    gmg, btg = P["gamma"].to(dev()).requires_grad_(True), P["beta"].to(dev()).requires_grad_(True)
    out = ops.in_affine_act(xg, gmg, btg, "leaky_relu")
    e = relmax(back(out), P["out"])
    note(f"in_affine small {pname} {shape} out {e:.3e}")
    assert e < TOL[pname]
    with pytest.raises(NotImplementedError, match="H, W >= 4"):
        out.backward(to_dev(P["g"], pname))


@functools.lru_cache(maxsize=None)
def _in_zero_table_problem(pname, shape, seed=61):
    """x, upstream gradient and, per activation, the float64 dgamma / dbeta of act(IN(x) * (1 + gamma) + beta) at gamma = beta = 0"""
    def make(s):
        x, g = data(shape, s), data(shape, s + 1, 1.0, 0.0)
        xr = rounded(x, pname).double()
        n, c = shape[0], shape[3]
        gm, bt = (torch.zeros(n, c, dtype=torch.float64, requires_grad=True) for _ in range(2))
        pre = F.instance_norm(xr, eps=1e-5) * (1 + gm[:, :, None, None]) + bt[:, :, None, None]
        dgb = {act: torch.autograd.grad(act64(pre, act), [gm, bt], rounded(g, pname).double(), retain_graph=True)
               for act in ("relu", "leaky_relu", "none")}
        return dict(x=x, g=g, pre=pre.detach(), dgb=dgb)
    return clear_of_kinks(make, "relu", seed)


@pytest.mark.parametrize("shape", [(2, 4, 4, 16),       # the class-mode minimum: border classes only, no interior
                                   (2, 5, 12, 16),      # one interior row
                                   (1, 9, 15, 16)],     # HW = 135: two ragged chunks
                         ids=_id)
@pytest.mark.parametrize("pname", PNAMES)
def test_instance_norm_family_is_one_path(ops, pname, shape):
    """instance_norm_act, in_affine_act with gamma = beta = 0 and (ReLU) spade_relu with an all-zero class table are the same
    statistics, the same coefficients (A = rstd (1 + 0) = rstd, B = 0 - mean A = -(mean rstd)) and the same backward kernels: out and
    dx are BIT-equal between the first two for every activation, dx of the third is bit-equal for ReLU (its forward is another
    kernel and is not compared).  in_affine_act's dgamma / dbeta at the zero table against float64, at that op's tolerances; the
    module's shared zero table is still all zeros after instance_norm_act's backward."""
    n, h, w, c = shape
    P = _in_zero_table_problem(pname, shape)
    gg = to_dev(P["g"], pname)
    for act in ("relu", "leaky_relu", "none"):
        tag = f"one-path {pname} {shape} {act}"
        xa, xb = (to_dev(P["x"], pname).requires_grad_(True) for _ in range(2))
        gmg, btg = (torch.zeros(n, c, device=dev(), requires_grad=True) for _ in range(2))
        out_a = ops.in_affine_act(xa, gmg, btg, act)
        out_a.backward(gg)
        out_b = ops.instance_norm_act(xb, act)
        out_b.backward(gg)
        table = ops._zero_tables[(dev(), _dtype(pname), n, c)]
        assert table.shape == (n, 5, 5, 2 * c) and int(torch.count_nonzero(table)) == 0, tag + ": the shared zero table was written"
        d_out, d_dx = (out_a.detach().float() - out_b.detach().float()).abs().max().item(), (xa.grad.float() - xb.grad.float()).abs().max().item()
        note(f"{tag}: in_affine_act vs instance_norm_act max |d out| {d_out:.3e} max |d dx| {d_dx:.3e}")
        assert torch.equal(out_a.detach(), out_b.detach()), (tag, "out", d_out)
        assert torch.equal(xa.grad, xb.grad), (tag, "dx", d_dx)
        if act == "relu":
            xc = to_dev(P["x"], pname).requires_grad_(True)
            zeros = torch.zeros(n, 5, 5, 2 * c, dtype=_dtype(pname), device=dev())
            ops.spade_relu(xc, zeros, False, 1).backward(gg)
            d_sp = (xc.grad.float() - xb.grad.float()).abs().max().item()
            note(f"{tag}: spade_relu vs instance_norm_act max |d dx| {d_sp:.3e}")
            assert torch.equal(xc.grad, xb.grad), (tag, "spade dx", d_sp)
        dgm, dbt = P["dgb"][act]
        eg, eb = relmax(gmg.grad, dgm), relmax(btg.grad, dbt)
        note(f"{tag}: dgamma {eg:.3e} dbeta {eb:.3e} (tol {2 * TOL[pname]:.1e})")
        assert eg < 2 * TOL[pname] and eb < 2 * TOL[pname]


def test_instance_norm_variance_cancellation_f32(ops):
    """The InstanceNorm counterpart of test_batchnorm_variance_cancellation_f32 (mean = 8 std per channel, (2, 64, 65, 8), f32)."""
    shape = (2, 64, 65, 8)
    x = _offset_input(shape, 43)
    ref = F.instance_norm(x.double(), eps=1e-5)
    e32 = relmax(F.instance_norm(x, eps=1e-5), ref)
    out = ops.instance_norm_act(to_dev(x, "f32"), "none")
    e = relmax(back(out), ref)
    note(f"in cancellation f32: kernel {e:.3e}  torch-f32 {e32:.3e}  ratio {e / max(e32, 1e-30):.2f}")
    # measured on MI355X: independent fp32 (torch CPU) 1.88e-07, kernel 1.94e-06 -- ratio 10.3, the same one-pass cancellation as in
    # the BatchNorm case; 4 x 1.88e-07 is below the project's 2e-4, which therefore is the bound: 100x headroom
    assert e < max(TOL["f32"], 4 * e32)


@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("shape,up", [((2, 9, 15, 16), False),      # HW = 135: two ragged chunks (smallest: one pixel of 135 less
                                                                   #   moves the mean by |x| / 135 ~ 4e-3 of the max: 20x tol)
                                      ((2, 64, 65, 8), False),     # the 64-chunk cap, ragged
                                      ((2, 10, 16, 16), True)],    # output extents; x is (2, 5, 8, 16): 160 output rows, 2 chunks
                         ids=["9x15", "64x65", "up-10x16"])
def test_spade_relu_dense_table(ops, pname, shape, up):
    """ops.spade_relu with a dense (N, H, W, 2C) gamma | beta tensor (gb_mode 0) -- the partial / finalize / apply kernels without
    the class table -- against relu(IN(up(x)) * (1 + gamma) + beta) in float64: out, dx and the dense dgb."""
    n, h, w, c = shape
    sshape = (n, h // 2, w // 2, c) if up else shape

    def make(seed):
        x, g = data(sshape, seed, 1.3, 0.2), data(shape, seed + 1, 1.0, 0.0)
        gamma, beta = data(shape, seed + 2, 0.3, 0.0), data(shape, seed + 3, 0.3, 0.1)
        xr, gmr, btr = (rounded(t, pname).double().requires_grad_(True) for t in (x, gamma, beta))
        xin = xr.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if up else xr
        pre = F.instance_norm(xin, eps=1e-5) * (1 + gmr) + btr
        grads = torch.autograd.grad(torch.relu(pre), [xr, gmr, btr], rounded(g, pname).double())
        return dict(x=x, g=g, gamma=gamma, beta=beta, pre=pre.detach(), grads=grads)

    P = clear_of_kinks(make, "relu", 51)
    x, g, gamma, beta, pre, (dx, dgm, dbt) = P["x"], P["g"], P["gamma"], P["beta"], P["pre"], P["grads"]
    out_ref = torch.relu(pre)

    xg = to_dev(x, pname).requires_grad_(True)
    gbg = torch.cat([to_dev(gamma, pname), to_dev(beta, pname)], dim=-1).contiguous().requires_grad_(True)
    out = ops.spade_relu(xg, gbg, up, 0)
    out.backward(to_dev(g, pname))
    tag = f"spade dense {pname} {shape} up={up}"
    e = relmax(back(out), out_ref)
    note(f"{tag} out {e:.3e}")
    assert e < TOL[pname]
    keep = kink_keep(pre, "relu")
    keep_src = keep if not up else F.max_pool2d((~keep).double(), 2) == 0          # a source pixel collects its four cells
    check_grad(back(xg.grad), dx, keep_src, pname, tag + " dx")
    check_grad(back(gbg.grad[..., :c]), dgm, keep, pname, tag + " dgamma")
    check_grad(back(gbg.grad[..., c:]), dbt, keep, pname, tag + " dbeta")


# ======================================================================================================================
# 3. Column sums (the bias gradient)
# ======================================================================================================================
COLSUM_ROWS_SMALL = [1,          # one row (the smallest: it IS the sum)
                     255, 256,   # below / at one full trip of rpp = 256 row-threads (cv = 1); one workgroup
                     257,        # one row into the second trip
                     511,        # still one workgroup (511 / 256 = 1)
                     513]        # two workgroups, ragged (257 + 256)
COLSUM_ROWS_LARGE = [65536 + 77,   # 256 workgroups (the cap reached exactly: 65613 / 256 = 256), 257 rows each, ragged last
                     70001]        # above the 256-workgroup cap: 274 rows per workgroup, 131 in the last


def _colsum_cases():
    cases = []
    for p in PNAMES:
        widest = _vec(p) * 256
        for c in (8, 24, 136, widest):     # cv = 1 | 2, 3 | 6, 17 | 34, 256 (bf16 | f32)
            for rows in COLSUM_ROWS_SMALL + (COLSUM_ROWS_LARGE if c == 8 else []):      # <= ~1M elements per case
                cases.append(pytest.param(p, rows, c, id=f"{p}-{rows}x{c}"))
    return cases


def _colsum(ops, pname, g):
    rows, c = g.shape
    lib = ops._lib_for(g)
    blocks = lib.dei2i_colsum_blocks(rows)
    assert 1 <= blocks <= 256
    part = torch.full((blocks * c,), 7.0, dtype=torch.float32, device=dev())     # the kernel promises to need no zero fill
    out = torch.full((c,), 7.0, dtype=torch.float32, device=dev())
    rc = lib.dei2i_colsum(ops.get_precision(pname).code, rows, c, ops._p(g), ops._p(part), ops._p(out), ops._stream())
    torch.cuda.synchronize()
    return rc, out, part


@pytest.mark.parametrize("pname,rows,c", _colsum_cases())
def test_colsum_rows_and_widths(ops, pname, rows, c):
    """dei2i_colsum through the C ABI, scratch and output pre-filled with a sentinel.  Two inputs per case:
    * non-zero integers in [-8, 8]: every partial sum in any order is an integer below 2^24, so fp32 accumulation is exact and the
      result must EQUAL the float64 column sum -- one dropped or doubled row is a difference of at least 1;
    * randn * 1.7 + 0.4 data: |error| <= k * 2^-24 * sum|x| per column with k = 320 additions on the longest chain (2 per thread,
      256 across the row-threads, 32 in the finalize, and the roundings of the stores) -- the a-priori bound of fp32 summation."""
    gen = torch.Generator().manual_seed(rows * 31 + c)
    ints = torch.randint(1, 9, (rows, c), generator=gen).float() * (torch.randint(0, 2, (rows, c), generator=gen).float() * 2 - 1)
    rc, out, _ = _colsum(ops, pname, ints.to(dev(), _dtype(pname)))
    assert rc == 0
    assert torch.equal(out.double().cpu(), ints.double().sum(0)), "integer data: the column sums must be exact"
    x = rounded(torch.randn(rows, c, generator=gen) * 1.7 + 0.4 + 0.1 * (torch.arange(c) % 5), pname)
    rc, out, _ = _colsum(ops, pname, x.to(dev(), _dtype(pname)))
    assert rc == 0
    err = ((out.double().cpu() - x.double().sum(0)).abs() / x.double().abs().sum(0)).max().item()
    note(f"colsum {pname} {rows}x{c}: max error / sum|x| = {err:.3e} (bound {320 * 2.0 ** -24:.1e})")
    assert err < 320 * 2.0 ** -24


@pytest.mark.parametrize("pname", PNAMES)
def test_colsum_refuses_more_than_256_channel_vectors(ops, pname):
    from de_i2i_gan_amd import _lib as L
    g = torch.ones(4, _vec(pname) * 257, dtype=_dtype(pname), device=dev())
    rc, out, part = _colsum(ops, pname, g)
    assert rc != 0
    with pytest.raises(RuntimeError, match="colsum"):
        L.check(rc, "colsum")
    assert float((out - 7.0).abs().max()) == 0.0 and float((part - 7.0).abs().max()) == 0.0      # nothing was launched


# ======================================================================================================================
# 4. Scalar losses and the noise-weight gradient
# ======================================================================================================================
# 262144 = 1024 workgroups x 256 threads (grid_for's cap for the losses): the last workgroup index, the first element of the
# grid-stride second trip, and one past; 1048576 + 3: four full trips and a ragged fifth
LOSS_N = [1, 255, 256, 257, 1023, 262143, 262144, 262145, 1048576 + 3]


@functools.lru_cache(maxsize=None)
def _bce_problem(n, target):
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * 3
    x[::97] = 40.0                                            # saturation of log1p(exp(-|x|))
    x[n - 1] = -40.0
    t = torch.rand(n, generator=gen).round() if target == "tensor" else None
    xr = x.double().requires_grad_(True)
    tt = t.double() if t is not None else torch.full_like(xr, float(target))
    ref = (torch.clamp_min(xr, 0) - xr * tt + torch.log1p(torch.exp(-xr.abs()))).mean()
    (gref,) = torch.autograd.grad(ref * 1.7, xr)
    return x, t, ref.item(), gref


def _check_bce(ops, n, target):
    x, t, ref, gref = _bce_problem(n, target)
    xg = x.to(dev()).requires_grad_(True)
    out = ops.bce_logits(xg, t.to(dev()) if t is not None else float(target))
    (out * 1.7).backward()
    e, eg = abs(out.detach().item() - ref) / max(1.0, abs(ref)), relmax(xg.grad, gref)
    note(f"bce n={n} target={target}: loss {e:.3e} (tol 1e-5)  grad {eg:.3e} (tol 1e-5)")
    assert e < 1e-5 and eg < 1e-5


@pytest.mark.parametrize("target", ["tensor", 1.0, 0.0], ids=["tensor", "ones", "zeros"])
@pytest.mark.parametrize("n", LOSS_N)
def test_bce_logits_across_the_partial_and_grid_stride_boundaries(ops, n, target):
    """n = 1 is the smallest: the loss IS that element.  At the large sizes the per-element gradient covers every index once."""
    _check_bce(ops, n, target)


@functools.lru_cache(maxsize=None)
def _l1_problem(n, with_b):
    gen = torch.Generator().manual_seed(n + 7)
    a, b = torch.randn(n, generator=gen), (torch.randn(n, generator=gen) if with_b else None)
    if with_b:
        b[::53] = a[::53]                                     # exact ties: gradient 0
    else:
        a[::53] = 0.0
    ar = a.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if with_b else None
    ref = (ar - br).abs().mean() if with_b else ar.abs().mean()
    grefs = torch.autograd.grad(ref, [ar] + ([br] if with_b else []))
    return a, b, ref.item(), grefs


def _check_l1(ops, n, with_b):
    a, b, ref, grefs = _l1_problem(n, with_b)
    ag = a.to(dev()).requires_grad_(True)
    bg = b.to(dev()).requires_grad_(True) if with_b else None
    out = ops.l1(ag, bg)
    out.backward()
    e, ea = abs(out.detach().item() - ref), relmax(ag.grad, grefs[0])
    note(f"l1 n={n} b={with_b}: loss {e:.3e} (tol 1e-6)  grad {ea:.3e} (tol 1e-6)")
    assert e < 1e-6 and ea < 1e-6
    assert float(ag.grad[::53].abs().max()) == 0.0            # the ties
    if with_b:
        assert relmax(bg.grad, grefs[1]) < 1e-6


@pytest.mark.parametrize("with_b", [True, False], ids=["b", "none"])
@pytest.mark.parametrize("n", LOSS_N)
def test_l1_across_the_partial_and_grid_stride_boundaries(ops, n, with_b):
    _check_l1(ops, n, with_b)


@pytest.mark.parametrize("n", [262143, 262144, 262145, 1048576 + 3])
def test_l1_of_integer_data_is_exact_to_two_roundings(ops, n):
    """|a - b| of small integers sums exactly in fp32 in any order (the total stays below 2^24), so the loss may differ from float64
    only by the rounding of 1 / n and of the product: 2^-23 relative.  One dropped or doubled element (|a - b| >= 1 of a total of
    at most 3 n) moves it by at least 1 / (3 n) = 3.2e-7 relative at the largest n: 2.7 times the bound."""
    gen = torch.Generator().manual_seed(n)
    a = torch.randint(-4, 5, (n,), generator=gen).float()
    b = a + torch.randint(1, 4, (n,), generator=gen).float() * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
    ref = (a.double() - b.double()).abs().mean().item()
    assert (a - b).abs().sum().item() < 2 ** 24
    out = ops.l1(a.to(dev()), b.to(dev()))
    e = abs(out.item() - ref) / ref
    note(f"l1 integers n={n}: {e:.3e} (bound {2.0 ** -23:.2e})")
    assert e <= 2.0 ** -23 * (1 + 1e-6)                       # (1 + 2^-24)^2 - 1


@pytest.mark.parametrize("first,second", [(1048576 + 3, 257), (262145, 255), (1023, 1)])
def test_losses_called_twice_smaller_after_larger(ops, first, second):
    """The block partials live in one process-wide buffer that is never cleared: a smaller loss right after a larger one must not
    read the larger one's partials."""
    _check_bce(ops, first, "tensor")
    _check_bce(ops, second, "tensor")
    _check_l1(ops, first, True)
    _check_l1(ops, second, True)
    _check_bce(ops, first, 1.0)
    _check_l1(ops, second, False)


# nvec = rows * C / VEC channel vectors; (rows, vectors per row)
NOISE_CASES = [(85, 3),          # nvec = 255: one workgroup, its last thread idle (smallest: one row of 85 less moves dweight by ~1 %)
               (257, 1),         # nvec = 257: one vector into the second workgroup
               (87383, 3)]       # nvec = 262144 + 5: the 1024-workgroup cap and five vectors of the grid-stride second trip


@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("rows,vpr", NOISE_CASES)
def test_noise_inject_weight_gradient_with_the_weight_used_twice(ops, pname, rows, vpr):
    """ops.noise_inject at nvec in {255, 257, 262144 + 5}: output, dx and dweight (weight used twice: the second node accumulates
    inside loss_finalize_kernel) against float64.  The large case uses small non-zero integers for dy and the noise: the sum is
    then exact in fp32 in any order, so the project's 2e-5 holds trivially for a correct kernel while one dropped vector (a term of
    at least 1 in a random-walk total of a few thousand) breaks it; the small cases use randn data."""
    c = vpr * _vec(pname)
    gen = torch.Generator().manual_seed(rows)
    if rows > 1000:
        def ints(*shape):
            return torch.randint(1, 3, shape, generator=gen).float() * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
        nz1, nz2, gy1, gy2 = ints(rows), ints(rows), ints(rows, c), ints(rows, c)
    else:
        nz1, nz2 = torch.randn(rows, generator=gen), torch.randn(rows, generator=gen)
        gy1, gy2 = (rounded(torch.randn(rows, c, generator=gen), pname) for _ in range(2))
    x1, x2 = (rounded(torch.randn(rows, c, generator=gen), pname) for _ in range(2))
    wt = torch.tensor(0.37).reshape(1, 1, 1, 1)
    wr = wt.double().requires_grad_(True)
    y1 = x1.double() + wr.reshape(()) * nz1.double().view(rows, 1)
    y2 = x2.double() + wr.reshape(()) * nz2.double().view(rows, 1)
    ((y1 * gy1.double()).sum() + (y2 * gy2.double()).sum()).backward()

    wg = torch.nn.Parameter(wt.to(dev()))
    shape = (1, rows, 1, c)
    xg1, xg2 = (t.view(shape).to(dev(), _dtype(pname)).requires_grad_(True) for t in (x1, x2))
    o1 = ops.noise_inject(xg1, wg, nz1.view(1, 1, rows, 1).to(dev()))
    o2 = ops.noise_inject(xg2, wg, nz2.view(1, 1, rows, 1).to(dev()))
    g1, g2 = (t.view(shape).to(dev(), _dtype(pname)) for t in (gy1, gy2))
    torch.autograd.backward([o1, o2], [g1, g2])
    assert relmax(o1.view(rows, c), y1) < TOL[pname] and relmax(o2.view(rows, c), y2) < TOL[pname]
    assert torch.equal(xg1.grad, g1) and torch.equal(xg2.grad, g2)
    e = relmax(wg.grad, wr.grad)
    note(f"noise {pname} rows={rows} nvec={rows * vpr}: dweight {e:.3e} (tol 2e-5), |dweight| {abs(wr.grad.item()):.4g}")
    assert wg.grad.shape == wt.shape and e < 2e-5


# ======================================================================================================================
# 5. Statistics records written by another producer (dei2i_affine_act_stats_fwd)
# ======================================================================================================================
STATS_SHAPES = [(2, 9, 14, 16),      # one record per image (smallest: see BN_SHAPES)
                (2, 10, 13, 24),     # two ragged chunks; cv = 3 in bf16, 6 in f32
                (5, 64, 64, 8)]      # 64 records per image, 320 for the batch: BatchNorm's 256-thread combine


@pytest.mark.parametrize("consumer", ["instance_norm", "batchnorm"])
@pytest.mark.parametrize("producer", ["add", "batchnorm"])
@pytest.mark.parametrize("shape", STATS_SHAPES, ids=_id)
@pytest.mark.parametrize("pname", PNAMES)
def test_norm_consumes_the_statistics_its_producer_left(ops, monkeypatch, pname, shape, producer, consumer):
    """ops.add(..., stats=True) and ops.batchnorm_act(..., stats=True) run dei2i_affine_act_stats_fwd: the moments records of their
    own ROUNDED output ride on the tensor, and the norm that follows reads them in place of a dei2i_moments_partial pass.  (a) the
    producer's output is right, (b) the consumer launched no moments pass, (c) its result is the float64 normalisation of the
    stored tensor."""
    n, h, w, c = shape
    x, r = data(shape, 61), data(shape, 62, 1.0, -0.2)
    xg, rg = to_dev(x, pname), to_dev(r, pname)
    xr, rr = rounded(x, pname).double(), rounded(r, pname).double()
    if producer == "add":
        s = ops.add(xg, rg, stats=True)
        s_ref = xr + rr
    else:
        wt, bs, rm0, rv0 = vecs(c, 63)
        s = ops.batchnorm_act(xg, wt.to(dev()), bs.to(dev()), rm0.to(dev()), rv0.to(dev()), True, "leaky_relu", rg, stats=True)
        s_ref = F.leaky_relu(F.batch_norm(xr, None, None, wt.double(), bs.double(), True, 0.1, 1e-5), 0.2) + rr
    tag = f"stats {pname} {shape} {producer}->{consumer}"
    e = relmax(back(s), s_ref)
    note(f"{tag} producer out {e:.3e}")
    assert e < TOL[pname]
    have = ops._stats_of(s, n, h * w, c)
    assert have is not None and have[1] == ops._lib_for(s).dei2i_moments_chunks(h * w)

    lib, calls = ops._lib_for(s), []
    real = lib.dei2i_moments_partial
    monkeypatch.setattr(lib, "dei2i_moments_partial", lambda *a: (calls.append(1), real(*a))[1])
    stored = back(s)                                          # what the consumer reads: the rounded tensor in memory
    if consumer == "instance_norm":
        out = ops.instance_norm_act(s, "none")
        ref = F.instance_norm(stored, eps=1e-5)
    else:
        wt2, bs2, rm2, rv2 = vecs(c, 64)
        rm, rv = rm2.to(dev()), rv2.to(dev())
        out = ops.batchnorm_act(s, wt2.to(dev()), bs2.to(dev()), rm, rv, True, "none")
        rm64, rv64 = rm2.double().clone(), rv2.double().clone()
        ref = F.batch_norm(stored, rm64, rv64, wt2.double(), bs2.double(), True, 0.1, 1e-5)
        rtol = 1e-4 + (5e-3 if pname == "bf16" else 0)
        assert relmax(rm, rm64) < rtol and relmax(rv, rv64) < rtol
    assert calls == [], "the consumer ran its own moments pass"
    e = relmax(back(out), ref)
    note(f"{tag} consumer out {e:.3e}")
    assert e < TOL[pname]
