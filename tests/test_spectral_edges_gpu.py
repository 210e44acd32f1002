"""csrc/spectral.hip at the branches its kernels contain, through ops.spectral_weight / ops.fold_bn_weight against the oracle's
float64 restatement of torch.nn.utils.spectral_norm (oracle.weight_of), as test_ops_gpu.py::test_spectral_weight_op does at round
shapes.  W is weight_orig as a (Cout, K) matrix, K = Cin * kh * kw; the seams:

  sn_wt_u_kernel    64 columns a workgroup (a partial last block when K % 64 != 0), the rows dealt to 16 row groups: group g runs a
                    4x-unrolled loop while r + 48 < Cout, then a remainder loop
  sn_sum_parts      256 threads stride over ceil(K / 64) column-block partials or over Cout row partials: a second trip above 256
  sn_w_v_kernel     pairs (k, k + 256) while k + 256 < K, then one tail element; workgroup r writes ceil(K / Cout) elements of v
  sn_scale_kernel / sn_bwd_dot_kernel      n / 4 float4 groups, then the n % 4 tail (n = Cout * K)
  sn_bwd_apply_kernel<K4>                  K % 4 == 0 picks the float4 form; both sum n / 2048 (<= 1024) partials, 256 at a time

Every shape runs forward and backward with the parameter used TWICE in one pass, so the second backward node adds into the first
one's tensor (accumulate = 0 and 1).  Bounds are the project's: maxrel 2e-5 for w_eff, u, v and 5e-5 for the gradient; the error of a
plain fp32 CPU restatement of the same power iteration is printed beside the kernel's (DESIGN.md section 4 records them)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import defectgan_oracle as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

# (Cout, Cin, kh, kw): what it reaches
SHAPES = [
    (63, 7, 3, 3),        # K = 63: one partial column block; n % 4 = 1; row group 15 runs the remainder loop only
    (65, 16, 2, 2),       # K = 64: one full column block; row group 0 runs the unrolled loop, then ONE remainder row (r = 64)
    (80, 65, 1, 1),       # K = 65: a second column block of one column; every row group: unrolled loop then a remainder row
    (80, 3, 3, 3),        # K = 27 < Cout: one-element v slices, most workgroups write none
    (3, 257, 1, 1),       # the W.v loop: one pair (k = 0, 256), no tail
    (3, 513, 1, 1),       # one pair and the tail element k = 512
    (2, 1025, 1, 1),      # v slices of 513 elements (> 256: a second trip of the slice loop); n % 4 = 2
    (257, 8, 1, 1),       # 257 row partials: sn_sum_parts' second trip (one element)
    (300, 4, 3, 3),       # 300 row partials
    (4, 1028, 4, 4),      # K = 16 448: 257 column-block partials
    (257, 2049, 1, 1),    # 257 backward partials (n / 2048), scalar apply kernel (K % 4 = 1), n % 4 = 1
    (264, 500, 2, 2),     # 257 backward partials, float4 apply kernel (K = 2000)
]
TOL_FWD, TOL_GRAD = 2e-5, 5e-5


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


def dev():
    return torch.device("cuda:0")


def note(*a):
    print("[spectral-edges]", *a, flush=True)


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@functools.lru_cache(maxsize=None)
def inputs(shape, iterate, scale=0.2):
    """(w, u, v, g1, g2) on the CPU.  Training: random unit (u, v), as a fresh module holds.  Eval: (u, v) from three float64 power
    iterations rounded to fp32, as a trained checkpoint holds -- with random vectors sigma = u^T W v can land near zero and the
    comparison would mean nothing; sigma > 0.1 |W|_2 is asserted."""
    gen = torch.Generator().manual_seed(1000 * shape[0] + shape[1] * shape[2] * shape[3])
    w = torch.randn(shape, generator=gen) * scale
    u = F.normalize(torch.randn(shape[0], generator=gen), dim=0)
    v = F.normalize(torch.randn(w[0].numel(), generator=gen), dim=0)
    g1, g2 = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    if not iterate:
        wm, ud = w.double().flatten(1), u.double()
        for _ in range(3):
            vd = F.normalize(wm.t() @ ud, dim=0)
            ud = F.normalize(wm @ vd, dim=0)
        u, v = ud.float(), vd.float()
        sigma = torch.dot(u.double(), wm @ v.double()).item()
        assert sigma > 0.1 * torch.linalg.matrix_norm(wm, 2).item(), (shape, sigma)
    return w, u, v, g1, g2


@functools.lru_cache(maxsize=None)
def reference(shape, iterate):
    """float64 through the oracle: two successive forwards, like two calls of the module in one step -> (r1, r2, u, v, grad)"""
    w, u, v, g1, g2 = inputs(shape, iterate)
    S = {"c.weight_orig": w.double().requires_grad_(True), "c.weight_u": u.double().clone(), "c.weight_v": v.double().clone()}
    r1 = O.weight_of(S, "c.weight", iterate)
    r2 = O.weight_of(S, "c.weight", iterate)
    ((r1 * g1.double()).sum() + (r2 * g2.double()).sum()).backward()
    return r1.detach(), r2.detach(), S["c.weight_u"], S["c.weight_v"], S["c.weight_orig"].grad


def fp32_cpu(shape, iterate):
    """The same two forwards as plain fp32 torch on the CPU -> (r1, r2, u, v)"""
    w, u, v, _, _ = inputs(shape, iterate)
    wm, u, v = w.flatten(1), u.clone(), v.clone()
    outs = []
    for _ in range(2):
        if iterate:
            v = F.normalize(torch.mv(wm.t(), u), dim=0, eps=1e-12)
            u = F.normalize(torch.mv(wm, v), dim=0, eps=1e-12)
        outs.append(w / torch.dot(u, torch.mv(wm, v)))
    return outs[0], outs[1], u, v


def run_gpu(ops, shape, iterate, scale=1.0):
    w, u, v, g1, g2 = inputs(shape, iterate)
    wg = torch.nn.Parameter((w * scale).to(dev()))
    ug, vg = u.to(dev()), v.to(dev())
    o1 = ops.spectral_weight(wg, ug, vg, iterate)
    o2 = ops.spectral_weight(wg, ug, vg, iterate)
    ((o1 * g1.to(dev())).sum() + (o2 * g2.to(dev())).sum()).backward()
    torch.cuda.synchronize()
    return o1.detach().cpu(), o2.detach().cpu(), ug.cpu(), vg.cpu(), wg.grad.cpu()


# ---- a, b, c: every shape, training and eval -----------------------------------------------------------------------------------
@pytest.mark.parametrize("iterate", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_spectral_weight_at_the_seams(ops, shape, iterate):
    w, u0, v0, _, _ = inputs(shape, iterate)
    r1, r2, ur, vr, gr = reference(shape, iterate)
    o1, o2, ug, vg, grad = run_gpu(ops, shape, iterate)
    c1, c2, uc, vc = fp32_cpu(shape, iterate)
    got = dict(w_eff1=maxrel(o1, r1), w_eff2=maxrel(o2, r2), u=maxrel(ug, ur), v=maxrel(vg, vr), grad=maxrel(grad, gr))
    cpu = dict(w_eff1=maxrel(c1, r1), w_eff2=maxrel(c2, r2), u=maxrel(uc, ur), v=maxrel(vc, vr))
    note(shape, "iterate" if iterate else "eval", "kernel", {k: f"{e:.2e}" for k, e in got.items()}, "fp32 cpu",
         {k: f"{e:.2e}" for k, e in cpu.items()})
    if not iterate:
        assert torch.equal(ug, u0) and torch.equal(vg, v0)             # eval mode leaves the stored vectors alone
    assert got["w_eff1"] < TOL_FWD and got["w_eff2"] < TOL_FWD
    assert got["u"] < TOL_FWD and got["v"] < TOL_FWD
    assert grad.shape == w.shape and got["grad"] < TOL_GRAD


# ---- d: fixed-order reductions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterate", [True, False])
@pytest.mark.parametrize("shape", [(257, 2049, 1, 1), (80, 65, 1, 1)])
def test_two_runs_are_bit_identical(ops, shape, iterate):
    a = run_gpu(ops, shape, iterate)
    b = run_gpu(ops, shape, iterate)
    for x, y, name in zip(a, b, ("w_eff1", "w_eff2", "u", "v", "grad")):
        assert torch.equal(x, y), (shape, name)


# ---- e: every step scales exactly under a power of two --------------------------------------------------------------------------
@pytest.mark.parametrize("iterate", [True, False])
def test_power_of_two_scale_invariance(ops, iterate):
    shape = (65, 16, 2, 2)
    a = run_gpu(ops, shape, iterate)
    b = run_gpu(ops, shape, iterate, scale=1024.0)
    for x, y, name in zip(a[:4], b[:4], ("w_eff1", "w_eff2", "u", "v")):
        assert torch.equal(x, y), name


# ---- f: fold_bn_weight ----------------------------------------------------------------------------------------------------------
# v_rsq_f32 is not correctly rounded.  RSQRT_ULPS = its measured error against float64 rsqrt on the running_var + eps of these
# cases, rounded up to a whole ulp, plus one (the test measures it again through the kernel itself -- W = bn_weight = 1 makes w_eff
# the bare rsqrtf -- prints it and asserts it has not grown).  One ulp is two units u = 2^-24.  Roundings:
#   a = bn_w * rsqrtf(rv + eps)       the sum 1, rsqrtf 2 * RSQRT_ULPS, the product 1           k_a = 2 + 2 * RSQRT_ULPS
#   w_eff = W * a                     + 1 product                                                k_w = k_a + 1   on |W a|
#   b_eff = bn_b - rm * a             + 1 product + 1 difference                                 k_b = k_a + 2   on |bn_b| + |rm a|
RSQRT_ULPS = 2
FOLD_SHAPES = [(1, 5, 1, 1), (257, 3, 3, 3), (300, 7, 1, 1)]           # the last two: the bias loop strides past 256


@pytest.mark.parametrize("shape", FOLD_SHAPES)
def test_fold_bn_weight(ops, shape):
    gen = torch.Generator().manual_seed(77 + shape[0])
    cout, eps = shape[0], 1e-5
    w = torch.randn(shape, generator=gen) * 0.3
    bn_w = 1 + 0.3 * torch.randn(cout, generator=gen)
    bn_b = 0.2 * torch.randn(cout, generator=gen)
    rm = 0.5 * torch.randn(cout, generator=gen)
    rv = 1e-3 + (4 - 1e-3) * torch.rand(cout, generator=gen)
    eps32 = torch.tensor(eps, dtype=torch.float32)
    d = dev()
    # the device's rsqrtf on these inputs, in ulps of the exact value
    ones = torch.ones(cout, device=d)
    r_dev, zero_b = ops.fold_bn_weight(torch.ones(shape, device=d), ones, torch.zeros(cout, device=d), torch.zeros(cout, device=d), rv.to(d), eps)
    r_dev = r_dev.cpu().flatten(1)
    assert torch.equal(r_dev, r_dev[:, :1].expand_as(r_dev)) and not zero_b.cpu().any()
    x = (rv + eps32).double()                                          # the fp32 sum the kernel forms
    exact = x.rsqrt()
    ulp = torch.exp2(torch.floor(torch.log2(exact)) - 23)
    measured = ((r_dev[:, 0].double() - exact).abs() / ulp).max().item()
    note(shape, "rsqrtf error in ulps", round(measured, 3), "allowed", RSQRT_ULPS)
    assert measured <= RSQRT_ULPS - 1
    # the op
    w_eff, b_eff = ops.fold_bn_weight(w.to(d), bn_w.to(d), bn_b.to(d), rm.to(d), rv.to(d), eps)
    w_eff, b_eff = w_eff.cpu(), b_eff.cpu()
    a64 = bn_w.double() / (rv.double() + float(eps32)).sqrt()
    w_ref, S_w = w.double() * a64.view(-1, 1, 1, 1), (w.double() * a64.view(-1, 1, 1, 1)).abs()
    b_ref, S_b = bn_b.double() - rm.double() * a64, bn_b.double().abs() + (rm.double() * a64).abs()
    k_a = 2 + 2 * RSQRT_ULPS
    a32 = bn_w * torch.rsqrt(rv + eps32)                               # the plain fp32 CPU restatement
    for tag, gw, gb in (("kernel", w_eff, b_eff), ("fp32 cpu", w * a32.view(-1, 1, 1, 1), bn_b - rm * a32)):
        ew = ((gw.double() - w_ref).abs() / (U * S_w.clamp_min(1e-300))).max().item()
        eb = ((gb.double() - b_ref).abs() / (U * S_b.clamp_min(1e-300))).max().item()
        note(shape, tag, "worst error / (2^-24 * S): w_eff", round(ew, 3), "of", k_a + 1, "b_eff", round(eb, 3), "of", k_a + 2)
        assert ew <= k_a + 1 and eb <= k_a + 2, (tag, ew, eb)
