"""The ops that stargan-v2's R1 penalty differentiates TWICE (create_graph=True; ops.py "double backward"): _Conv2d.backward's
second-order branch, _ConvDgradFn (whose own backward swaps the operand roles: dg is the FORWARD conv of the incoming gradient, dW the
wgrad kernel on (x := incoming, dy := g)), _ActBwd, _AvgPool2 / _AvgPool2Bwd, _Scale, _AffineAdd, _ToNHWC / _ToNCHW -- one op at a
time and as one discriminator block, against plain torch (F.conv2d, F.leaky_relu(., 0.2), F.avg_pool2d) in float64 on the CPU with the
operands rounded to the compute dtype.  The whole-discriminator test (tests/test_starganv2_gpu.py) bounds them at 2e-3 relative L2 per
parameter in f32 only; here a wrong role or geometry of ONE op shows.

Per conv: g = d<y, seed>/dx with create_graph=True (seed a leaf), S = <g, r> for a fixed r (or the R1 form 0.5 mean_n |g|^2), and g,
dS/dW, dS/dseed, dS/dbias (None or zero: g does not depend on the bias) against the reference, at the bounds of
tests/test_ops_gpu.py test_conv2d_fwd_bwd: 2e-4 (f32) and 1.5e-2 (bf16) of the tensor's max."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = {"f32": 2e-4, "bf16": 1.5e-2}          # tests/test_ops_gpu.py TOL


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rounded(t, pname):
    return t.bfloat16().float() if pname == "bf16" else t


def nhwc(t, cs):
    """NCHW -> (N, H, W, cs), channels zero-padded"""
    n, c, h, w = t.shape
    out = torch.zeros(n, h, w, cs, dtype=t.dtype)
    out[..., :c] = t.permute(0, 2, 3, 1)
    return out


def nchw(t, c):
    return t[..., :c].permute(0, 3, 1, 2)


# ---- B1: one conv at a time ------------------------------------------------------------------------------------------------------
N = 3
# (cin, cout, k, stride, pad, bias, fused act, H, W, layout of the leaves)
CONV_CASES = [
    (3, 16, 3, 1, 1, True, "none", 8, 12, "nchw"),            # NCHW fp32 leaf -> to_nhwc (3 channels padded) -> conv -> to_nchw
    (16, 32, 3, 1, 1, True, "leaky_relu", 8, 12, "nhwc"),
    (16, 32, 1, 1, 0, False, "none", 8, 12, "nhwc"),
    (32, 32, 4, 1, 0, True, "leaky_relu", 4, 4, "nhwc"),      # the discriminator's 4x4 valid conv: 4 x 4 -> 1 x 1
    (32, 6, 1, 1, 0, True, "none", 1, 1, "nhwc"),             # its 1x1 head on 1 x 1
    (8, 16, 4, 2, 1, False, "leaky_relu", 8, 12, "nhwc"),     # stride 2, zero padding
    # cin == cout at one size: the only geometry at which _ConvDgradFn.backward's wgrad call with its operands SWAPPED still passes the
    # library's argument check (everywhere else it is refused) -- there only the numbers tell
    (16, 16, 3, 1, 1, False, "none", 8, 12, "nhwc"),
]
# seeds (checked on the CPU) for which no pre-activation of the reference lies within 1e-4 of its max magnitude of zero: no
# LeakyReLU mask can then legitimately differ, and the max-error bounds hold for the fused-activation cases too
SEEDS = {(1, "f32"): 16, (1, "bf16"): 3, (3, "f32"): 0, (3, "bf16"): 0, (5, "f32"): 1, (5, "bf16"): 1}     # margins 1.2e-4 ... 5.9e-3


def conv_data(ci, pname):
    cin, cout, k, s, pad, has_bias, act, H, W, _ = CONV_CASES[ci]
    gen = torch.Generator().manual_seed(100 + 1000 * SEEDS.get((ci, pname), 0) + ci)
    ho, wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    d = {"x": torch.randn(N, cin, H, W, generator=gen), "w": torch.randn(cout, cin, k, k, generator=gen) * math.sqrt(2.0 / (cin * k * k)),
         "seed": torch.randn(N, cout, ho, wo, generator=gen), "r": torch.randn(N, cin, H, W, generator=gen)}
    d = {key: rounded(v, pname) for key, v in d.items()}
    d["b"] = torch.randn(cout, generator=gen) * 0.3 if has_bias else None         # fp32 in the product: not rounded
    return d


def penalty(g, form, r=None):
    if form == "dot":
        return (g * r).sum()
    return 0.5 * g.pow(2).reshape(g.shape[0], -1).sum(1).mean()                    # solver.py r1_reg


def conv_reference(ci, d, form):
    """float64 -> (pre-activation, g, dS/dW, dS/dseed, dS/dbias or None)"""
    cin, cout, k, s, pad, has_bias, act, H, W, _ = CONV_CASES[ci]
    x, w, seed = (d[key].double().requires_grad_(True) for key in ("x", "w", "seed"))
    b = d["b"].double().requires_grad_(True) if has_bias else None
    z = F.conv2d(x, w, b, stride=s, padding=pad)
    y = F.leaky_relu(z, 0.2) if act == "leaky_relu" else z
    (g,) = torch.autograd.grad((y * seed).sum(), x, create_graph=True)
    S = penalty(g, form, d["r"].double())
    grads = torch.autograd.grad(S, [w, seed] + ([b] if has_bias else []), allow_unused=True)
    return z.detach(), g.detach(), grads[0], grads[1], (grads[2] if has_bias else None)


def mask_margin(z):
    """smallest |pre-activation| relative to the largest"""
    return float(z.abs().min() / z.abs().max())


def conv_product(ops, pname, ci, d, form):
    cin, cout, k, s, pad, has_bias, act, H, W, layout = CONV_CASES[ci]
    prec = ops.get_precision(pname)
    w = d["w"].to(DEV).requires_grad_(True)
    b = d["b"].to(DEV).requires_grad_(True) if has_bias else None
    geom = ops.ConvGeom(cin, cout, k, s, pad, False, False)
    if layout == "nchw":
        x, seed, r = d["x"].to(DEV).requires_grad_(True), d["seed"].to(DEV).requires_grad_(True), d["r"].to(DEV)
        y = ops.to_nchw(ops.conv2d(ops.to_nhwc(x, prec), w, b, ops.PackedWeights(), geom, act), cout)
    else:
        x = nhwc(d["x"], prec.pad(cin)).to(prec.dtype).to(DEV).requires_grad_(True)
        seed = nhwc(d["seed"], prec.pad(cout)).to(prec.dtype).to(DEV).requires_grad_(True)
        r = nhwc(d["r"], prec.pad(cin)).to(DEV)
        y = ops.conv2d(x, w, b, ops.PackedWeights(), geom, act)
    (g,) = torch.autograd.grad((y * seed).sum(), x, create_graph=True)
    assert g.requires_grad
    S = penalty(g.float(), form, r)
    grads = torch.autograd.grad(S, [w, seed] + ([b] if has_bias else []), allow_unused=True)
    torch.cuda.synchronize()
    g, dseed = g.detach(), grads[1]
    if layout == "nhwc":
        assert float(g[..., cin:].abs().max()) == 0.0 if g.shape[-1] > cin else True
        g, dseed = nchw(g, cin), nchw(dseed, cout)
    return g, grads[0], dseed, (grads[2] if has_bias else None)


@pytest.mark.parametrize("pname", ["f32", "bf16"])
@pytest.mark.parametrize("ci,form", [(0, "dot"), (1, "dot"), (1, "r1"), (2, "dot"), (3, "dot"), (4, "dot"), (5, "dot"), (6, "dot")])
def test_conv_double_backward_matches_float64(ops, pname, ci, form):
    """Bounds: test_conv2d_fwd_bwd's 2e-4 (f32) / 1.5e-2 (bf16) of the tensor's max, for g, dS/dW and dS/dseed alike."""
    d = conv_data(ci, pname)
    z, g_ref, dw_ref, dseed_ref, db_ref = conv_reference(ci, d, form)
    if CONV_CASES[ci][6] != "none":
        assert mask_margin(z) > 1e-4, mask_margin(z)         # on the reference alone: the masks are unambiguous
    assert db_ref is None or float(db_ref.abs().max()) == 0.0
    g, dw, dseed, db = conv_product(ops, pname, ci, d, form)
    err = {"g": maxrel(g, g_ref), "dS/dW": maxrel(dw, dw_ref), "dS/dseed": maxrel(dseed, dseed_ref)}
    print("conv double backward", pname, CONV_CASES[ci], form, {k: f"{v:.2e}" for k, v in err.items()})
    assert db is None or float(db.abs().max()) == 0.0
    # measured worst over the cases, f32: g 4.2e-7, dS/dW 2.2e-7, dS/dseed 2.6e-7; bf16: g 3.1e-3, dS/dW 1.5e-3 (the R1 form, behind two
    # bf16 stores: it fits the bound of the others), dS/dseed 2.9e-3
    assert err["g"] < TOL[pname], err
    assert err["dS/dW"] < TOL[pname], err
    assert err["dS/dseed"] < TOL[pname], err


# ---- B2: the linear ops, exact on small integers -----------------------------------------------------------------------------------
def ints(gen, shape, lo=-4, hi=4, nonzero=False):
    t = torch.randint(lo, hi + 1, shape, generator=gen).float()
    if nonzero:
        t = torch.where(t == 0, torch.full_like(t, float(hi)), t)
    return t


def aslist(o):
    return list(o) if isinstance(o, (tuple, list)) else [o]


def twice(fn, xs, seeds, rs, device, use=None):
    """ys = fn(*xs); g_i = d sum_k <y_k, seed_k> / d x_i with create_graph=True; -> (ys, gs, d sum_i <g_i, r_i> / d seed_k).
    On the CPU everything is float64; on the device the leaves keep their dtypes.  ``use``: the outputs that enter the sum."""
    ref = device == "cpu"
    conv = (lambda t: t.double()) if ref else (lambda t: t.to(device))
    xs = [conv(x).requires_grad_(True) for x in xs]
    ys = aslist(fn(*xs))
    use = range(len(ys)) if use is None else use
    seeds = {k: conv(seeds[k]).requires_grad_(True) for k in use}
    acc = torch.float64 if ref else torch.float32
    total = sum((ys[k].to(acc) * seeds[k].to(acc)).sum() for k in use)
    gs = torch.autograd.grad(total, xs, create_graph=True)
    S = sum((g.to(acc) * conv(r).to(acc)).sum() for g, r in zip(gs, rs))
    ds = torch.autograd.grad(S, [seeds[k] for k in use])
    if not ref:
        torch.cuda.synchronize()
    return [y.detach() for y in ys], [g.detach() for g in gs], list(ds)


def agree(got, want, tol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if tol == 0:
        return torch.equal(got, want)
    return bool(((got - want).abs() <= tol * want.abs()).all())


def linear_cases(ops, prec):
    """name -> (product fn, reference fn on float64 tensors of the same layout, input shapes/kinds, used outputs, tolerance)"""
    c3, c20 = prec.pad(3), prec.pad(20)
    act = "a"            # an NHWC activation in the compute dtype
    img = "i"            # an NCHW fp32 image
    pool = lambda x: x.reshape(x.shape[0], x.shape[1] // 2, 2, x.shape[2] // 2, 2, x.shape[3]).mean((2, 4))
    up = lambda x: x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    return {
        "avgpool2": (ops.avgpool2, pool, [(act, (2, 4, 6, 8))], None, 0),
        "upsample2": (ops.upsample2, up, [(act, (2, 3, 5, 8))], None, 0),
        "scale_half": (lambda x: ops.scale(x, 0.5), lambda x: x * 0.5, [(act, (2, 3, 5, 8))], None, 0),
        "scale_4": (lambda x: ops.scale(x, 4.0), lambda x: x * 4.0, [(act, (2, 3, 5, 8))], None, 0),
        "add": (ops.add, lambda x, y: x + y, [(act, (2, 3, 5, 8)), (act, (2, 3, 5, 8))], None, 0),
        "to_nhwc_3": (lambda x: ops.to_nhwc(x, prec), lambda x: F.pad(x.permute(0, 2, 3, 1), (0, c3 - 3)), [(img, (2, 3, 4, 6))], None, 0),
        "to_nhwc_20": (lambda x: ops.to_nhwc(x, prec), lambda x: F.pad(x.permute(0, 2, 3, 1), (0, c20 - 20)), [(img, (2, 20, 3, 5))], None, 0),
        "to_nchw_3": (lambda x: ops.to_nchw(x, 3), lambda x: x[..., :3].permute(0, 3, 1, 2), [(act, (2, 4, 6, c3))], None, 0),
        "to_nchw_20": (lambda x: ops.to_nchw(x, 20), lambda x: x[..., :20].permute(0, 3, 1, 2), [(act, (2, 3, 5, c20))], None, 0),
        # three row blocks, the middle one unused: its gradient is the zero block of the concatenation
        "split_rows": (lambda x: ops.split_rows(x, [2, 1, 3]), lambda x: x.split([2, 1, 3], 0), [(act, (6, 2, 3, 8))], (0, 2), 0),
        # _ActBwd: 0.2 is not a bf16 (or fp32) number -- relative 2^-8 in bf16 (one rounding of 0.2 x to 8 bits), 2^-22 in fp32
        "leaky_relu": (ops.leaky_relu, lambda x: F.leaky_relu(x, 0.2), [(act, (2, 3, 5, 8), "nonzero")], None, 2.0 ** -8 if prec.name == "bf16" else 2.0 ** -22),
    }


LINEAR_NAMES = ["avgpool2", "upsample2", "scale_half", "scale_4", "add", "to_nhwc_3", "to_nhwc_20", "to_nchw_3", "to_nchw_20", "split_rows",
                "leaky_relu"]


@pytest.mark.parametrize("pname", ["f32", "bf16"])
@pytest.mark.parametrize("name", LINEAR_NAMES)
def test_linear_ops_first_and_second_order_on_integers(ops, pname, name):
    """Small-integer data: the op, its input gradient and the gradient of <input gradient, r> with respect to the seed are exact in
    either dtype (sums of at most four integers, divided by 4 or scaled by a power of two) and must EQUAL the float64 reference.
    leaky_relu: the second-order result r * act'(z) does not depend on the seed and doubling the seed doubles g exactly (linearity);
    the values carry the rounding of 0.2 x."""
    prec = ops.get_precision(pname)
    fn, ref_fn, inputs, use, tol = linear_cases(ops, prec)[name]
    gen = torch.Generator().manual_seed(7 + LINEAR_NAMES.index(name))
    xs = [ints(gen, spec[1], nonzero=len(spec) > 2).to(prec.dtype if spec[0] == "a" else torch.float32) for spec in inputs]
    rs = [ints(gen, spec[1]).to(x.dtype) for spec, x in zip(inputs, xs)]
    with torch.no_grad():
        shapes = [(tuple(y.shape), y.dtype) for y in aslist(fn(*[x.to(DEV) for x in xs]))]
    seeds = [ints(gen, s).to(dt) for s, dt in shapes]
    y_ref, g_ref, ds_ref = twice(ref_fn, xs, seeds, rs, "cpu", use)
    y, g, ds = twice(fn, xs, seeds, rs, DEV, use)
    for k in (range(len(y)) if use is None else use):
        assert agree(y[k], y_ref[k], tol), (name, "forward", k)
    for a, b in zip(g, g_ref):
        assert agree(a, b, tol), (name, "input gradient")
    for a, b in zip(ds, ds_ref):
        assert agree(a, b, tol), (name, "second order")
    if name == "leaky_relu":
        _, g2, ds2 = twice(fn, xs, [2 * s for s in seeds], rs, DEV, use)
        assert torch.equal(g2[0], 2 * g[0]) and torch.equal(ds2[0], ds[0])


# ---- B3: one discriminator block ---------------------------------------------------------------------------------------------------
class _Round(torch.autograd.Function):
    """round to bf16 (kept in fp32), twice differentiable: the gradient is rounded as well -- a tensor the product STORES"""

    @staticmethod
    def forward(ctx, x):
        return x.bfloat16().float()

    @staticmethod
    def backward(ctx, g):
        return _Round.apply(g)


class _RoundBwd(torch.autograd.Function):
    """identity whose gradient is rounded to bf16: a gradient the product stores where the forward pass stores nothing"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _Round.apply(g)


BLOCK_SHAPES = {"w0": (16, 3, 3, 3), "b0": (16,), "w1": (16, 16, 3, 3), "b1": (16,), "w2": (32, 16, 3, 3), "b2": (32,), "wsc": (32, 16, 1, 1),
                "w3": (32, 32, 4, 4), "b3": (32,), "w4": (2, 32, 1, 1), "b4": (2,)}
SQRT1_2 = 1.0 / math.sqrt(2.0)


def block_data(pname):
    gen = torch.Generator().manual_seed(21)
    P = {}
    for k, s in BLOCK_SHAPES.items():
        P[k] = rounded(torch.randn(s, generator=gen) * math.sqrt(2.0 / (s[1] * s[2] * s[3])), pname) if len(s) == 4 else torch.randn(s, generator=gen) * 0.2
    return rounded(torch.randn(4, 3, 8, 8, generator=gen), pname), P


def block_torch(x, P, st=lambda t: t, bw=lambda t: t):
    """The block in plain torch.  ``st``: wherever the product stores a tensor (the forward value and, through st's backward, the
    gradient that arrives there); ``bw``: where only the backward pass stores one (a branch's own input gradient before autograd
    sums the branches; the gradient between a fused activation and its conv)."""
    lrelu = lambda t: F.leaky_relu(t, 0.2)
    h0 = st(F.conv2d(st(x), P["w0"], P["b0"], padding=1))                              # to_nhwc, conv 3x3
    h = st(lrelu(bw(h0)))
    h = st(F.conv2d(h, P["w1"], P["b1"], padding=1))
    h = st(lrelu(st(F.avg_pool2d(h, 2))))
    h = st(F.conv2d(h, P["w2"], P["b2"], padding=1))
    sc = st(F.avg_pool2d(st(F.conv2d(bw(h0), P["wsc"])), 2))
    h = st(st(sc + h) * SQRT1_2)
    h = st(lrelu(h))
    h = st(lrelu(bw(F.conv2d(h, P["w3"], P["b3"]))))                                   # 4x4 valid conv, LeakyReLU in its epilogue
    return st(F.conv2d(h, P["w4"], P["b4"]))                                           # conv 1x1 (to_nchw then writes fp32)


def block_hip(ops, prec, x, P):
    G = ops.ConvGeom
    conv = lambda t, w, b, geom, act="none": ops.conv2d(t, P[w], P[b] if b else None, ops.PackedWeights(), geom, act)
    h0 = conv(ops.to_nhwc(x, prec), "w0", "b0", G(3, 16, 3, 1, 1, False, False))
    h = conv(ops.leaky_relu(h0), "w1", "b1", G(16, 16, 3, 1, 1, False, False))
    h = conv(ops.leaky_relu(ops.avgpool2(h)), "w2", "b2", G(16, 32, 3, 1, 1, False, False))
    sc = ops.avgpool2(conv(h0, "wsc", None, G(16, 32, 1, 1, 0, False, False)))
    h = ops.scale(ops.add(sc, h), SQRT1_2)
    h = conv(ops.leaky_relu(h), "w3", "b3", G(32, 32, 4, 1, 0, False, False), "leaky_relu")
    return ops.to_nchw(conv(h, "w4", "b4", G(32, 2, 1, 1, 0, False, False)), 2)


def r1_of(block, x, P):
    """-> (penalty, {weight name: d penalty / d weight}); the biases get no gradient (the input gradient does not depend on them)"""
    out = block(x, P)
    (g,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    pen = penalty(g, "r1")
    names = [k for k in P if k.startswith("w")]
    grads = torch.autograd.grad(pen, [P[k] for k in P], allow_unused=True)
    for k, gr in zip(P, grads):
        assert k.startswith("w") or gr is None or float(gr.abs().max()) == 0.0, k
    return pen.detach(), {k: gr.detach() for k, gr in zip(P, grads) if k in names}


def on(P, x, device, dtype):
    return x.to(device=device, dtype=dtype).requires_grad_(True), {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in P.items()}


def test_block_r1_penalty_f32(ops):
    """to_nhwc, conv 3x3 | LeakyReLU, conv 3x3, average pool, LeakyReLU, conv 3x3 || conv 1x1, average pool | add, / sqrt 2, LeakyReLU,
    conv 4x4 valid + LeakyReLU, conv 1x1, to_nchw on 4 x 3 x 8 x 8 (channels 3 -> 16 -> 32): the R1 penalty and its gradient with
    respect to every weight against float64 at the bounds of test_r1_penalty_double_backward_matches_the_oracle (value 1e-4, gradients
    2e-3 relative L2)."""
    x, P = block_data("f32")
    pen_ref, g_ref = r1_of(block_torch, *on(P, x, "cpu", torch.float64))
    xd, Pd = on(P, x, DEV, torch.float32)
    pen, g = r1_of(lambda a, b: block_hip(ops, ops.F32, a, b), xd, Pd)
    torch.cuda.synchronize()
    worst = {k: rel_l2(g[k], g_ref[k]) for k in g_ref}
    print("block R1 f32: value", float(pen), float(pen_ref), {k: f"{v:.2e}" for k, v in worst.items()})
    assert abs(float(pen) - float(pen_ref)) < 1e-4 * abs(float(pen_ref))               # measured 1.2e-8
    assert max(worst.values()) < 2e-3, worst                                           # measured at most 2.6e-7


def test_block_r1_penalty_bf16_within_three_times_the_emulated_rounding(ops):
    """The same block in bf16: every stored activation and gradient is rounded to 8 bits, so the bound is MEASURED, not guessed -- on a
    CPU emulation of the product: the same torch graph in fp32 with a twice-differentiable round-to-bf16 (its backward rounds too)
    wherever the product stores a tensor.  Bound per tensor (and for the value): 3 x the emulation's distance from float64 (relative
    L2); the factor covers the summation order and the masks taken from rounded outputs.  The emulation's distance sets the bound, not
    the kernels'.

    Measured, emulation / product:  w0 1.77e-2 / 2.95e-3,  w1 2.80e-2 / 3.98e-3,  w2 2.56e-2 / 3.86e-3,  wsc 2.25e-2 / 3.39e-3,
    w3 1.50e-2 / 4.06e-3,  w4 4.62e-3 / 1.94e-3,  value 1.47e-3 / 1.51e-3.  The emulation's own figures are dominated by LeakyReLU masks
    that flip under ITS forward rounding (a handful among the block's few thousand pre-activations; the product's roundings differ in
    the last bit and flip others or none); with the gradient roundings alone it sits 2.2e-3 ... 2.5e-3 from float64 (w4 1.6e-3), and
    the product is within 3 x that as well."""
    x, P = block_data("bf16")
    pen_ref, g_ref = r1_of(block_torch, *on(P, x, "cpu", torch.float64))
    pen_emu, g_emu = r1_of(lambda a, b: block_torch(a, b, _Round.apply, _RoundBwd.apply), *on(P, x, "cpu", torch.float32))
    xd, Pd = on(P, x, DEV, torch.float32)
    pen, g = r1_of(lambda a, b: block_hip(ops, ops.BF16, a, b), xd, Pd)
    torch.cuda.synchronize()
    emu = {k: rel_l2(g_emu[k], g_ref[k]) for k in g_ref}
    got = {k: rel_l2(g[k], g_ref[k]) for k in g_ref}
    emu["value"] = abs(float(pen_emu) - float(pen_ref)) / abs(float(pen_ref))
    got["value"] = abs(float(pen) - float(pen_ref)) / abs(float(pen_ref))
    print("block R1 bf16 (emulation, product):", {k: (f"{emu[k]:.2e}", f"{got[k]:.2e}") for k in emu})
    assert all(e > 0 for e in emu.values()), emu
    bad = {k: (emu[k], got[k]) for k in emu if not got[k] < 3 * emu[k]}
    assert not bad, bad


# ---- B4: geometry the double backward does not build --------------------------------------------------------------------------------
@pytest.mark.parametrize("reflect,up", [(True, False), (False, True)])
def test_double_backward_refuses_reflect_and_upsample_convs(ops, reflect, up):
    """a reflect-padded or upsample-fused conv under create_graph=True raises; it must not return numbers"""
    prec = ops.BF16
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 8, 8, 16, generator=gen).to(prec.dtype).to(DEV).requires_grad_(True)
    w = (torch.randn(16, 16, 3, 3, generator=gen) * 0.1).to(DEV).requires_grad_(True)
    y = ops.conv2d(x, w, None, ops.PackedWeights(), ops.ConvGeom(16, 16, 3, 1, 1, reflect, up))
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(y.float().sum(), x, create_graph=True)
    torch.cuda.synchronize()
