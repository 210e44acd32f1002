"""Shared by tests/test_starganv2_store_emulation.py (CPU) and the stargan-v2 bf16 GPU tests: the round-to-bf16 store hook of
oracle/starganv2_oracle.py, the block cases and network problems the tests run, and their float64 references -- computed once per
process and never modified.

The bf16 rule of every comparison here ("3 x the store emulation + floor"):
    d_emul = relative L2 of the float64 oracle WITH the rounding hook from the float64 oracle without it, same operands;
    d_prod = the same for the HIP product in bf16 mode;
    d_prod <= 3 * d_emul + 1e-3.
The factor and the form are tests/test_second_order_gpu.py's (a bf16 block against a rounding emulation: summation order, LeakyReLU
masks taken from rounded outputs, a branch's gradient rounded before autograd sums the branches); the floor is the f32-mode forward
bound, for tensors the emulation gets exactly (the mapping network: fp32 linears, nothing stored).  The emulation's distance sets the
bound, never the kernels'."""
import contextlib
import functools
import math

import torch

from oracle import starganv2_oracle as O

FACTOR, FLOOR = 3.0, 1e-3
COS_FLOOR = 1e-4
F32_FWD, F32_GRAD = 1e-3, 2e-3            # tests/test_starganv2_gpu.py: forward 1e-3 of the tensor's max, gradients 2e-3 relative L2
KINK_BAND, KINK_SHARE = 1e-4, 1e-3        # tests/test_reduce_edges_gpu.py: |pre| < 1e-4 max|pre| for fewer than 0.1 % of the elements
STYLE_DIM = 16


# ---- the hook ------------------------------------------------------------------------------------------------------------------------
def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _Round(torch.autograd.Function):
    """round to bf16, straight through; the backward rounds the arriving gradient the same way (and is differentiable again: the R1
    penalty differentiates it)"""

    @staticmethod
    def forward(ctx, t):
        return _bf16(t)

    @staticmethod
    def backward(ctx, g):
        return _Round.apply(g)


class _RoundForward(torch.autograd.Function):
    """round to bf16, gradient untouched: a conv weight (the kernels read PackedWeights' bf16 copy and write the gradient in fp32)"""

    @staticmethod
    def forward(ctx, t):
        return _bf16(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _LReluOneAtZero(torch.autograd.Function):
    """LeakyReLU(0.2) with the kernels' derivative at an exact 0: 1 (csrc/common.h act_grad_from_out, ``z >= 0``), not torch's 0.2"""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.nn.functional.leaky_relu(x, 0.2)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return torch.where(x >= 0, g, 0.2 * g)


class Bf16Store:
    """the product's bf16 mode as a hook of the oracle: ``store(t)`` an activation or gradient store, ``store.weight(w)`` a conv's
    packed weight copy, ``store.lrelu(x)`` LeakyReLU with the kernels' derivative at 0"""

    def __call__(self, t):
        return _Round.apply(t)

    @staticmethod
    def weight(w):
        return _RoundForward.apply(w)

    @staticmethod
    def lrelu(x):
        return _LReluOneAtZero.apply(x)


BF16_STORE = Bf16Store()
STORES = {"ref": O._same, "emul": BF16_STORE}


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def bf16_bound(d_emul):
    return FACTOR * d_emul + FLOOR


@contextlib.contextmanager
def recorded_preactivations(sink):
    """every tensor the oracle hands to its LeakyReLU while the block runs, appended to ``sink``"""
    plain = O.lrelu

    def recording(x):
        sink.append(x.detach())
        return plain(x)
    O.lrelu = recording
    try:
        yield
    finally:
        O.lrelu = plain


def kink_share(pres):
    """share of the pre-activations inside the kink band of their own tensor"""
    inside = sum(int((p.abs() < KINK_BAND * p.abs().max()).sum()) for p in pres)
    return inside / max(1, sum(p.numel() for p in pres))


# ---- initialisation ------------------------------------------------------------------------------------------------------------------
def he_state(shapes, gen):
    """The reference's he_init (kaiming normal, fan_in, relu gain: conv and linear weights, tests/test_stargan_ddp_gpu.py::_he_init),
    then every bias ~ N(0, 0.1) and every InstanceNorm weight ~ 1 + N(0, 0.1) -- the product's gamma = weight - 1 is then N(0, 0.1)
    like AdaIN's -- so that a dropped bias or affine term shows.  fp32, as the product holds its parameters."""
    S = {}
    for k, shape in shapes.items():
        if len(shape) >= 2:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            S[k] = torch.randn(shape, generator=gen) * math.sqrt(2.0 / fan_in)
        else:
            S[k] = torch.randn(shape, generator=gen) * 0.1 + (1.0 if k.endswith("weight") else 0.0)
    return S


def bf16_valued(shape, gen, scale=1.0):
    return _bf16(torch.randn(shape, generator=gen) * scale)


# ---- part 1: the blocks --------------------------------------------------------------------------------------------------------------
# (id, kind, normalize | -, downsample | upsample, din, dout, H = W): every structural branch of ResBlk and AdainResBlk at N = 2, 8 x 8
# (an interior and a border at both resolutions), and the first and sixth at 64 -> 128 / 128 -> 64 channels, 16 x 16 (more than one
# vector group, a second K block)
BLOCKS = [
    ("res-norm-down-16-32", "res", True, True, 16, 32, 8),       # learned 1x1 shortcut then pool; IN -> conv -> pool -> IN -> conv
    ("res-norm-32-32", "res", True, False, 32, 32, 8),           # identity shortcut, no pool
    ("res-plain-down-16-32", "res", False, True, 16, 32, 8),     # stand-alone leaky_relu feeding both branches (trunk block)
    ("res-plain-down-32-32", "res", False, True, 32, 32, 8),     # identity shortcut through the pool
    ("res-plain-16-16", "res", False, False, 16, 16, 8),         # conv1 with the activation in its epilogue
    ("adain-up-32-16", "adain", None, True, 32, 16, 8),          # x2 upsample fused into the 1x1 shortcut and into conv1
    ("adain-up-32-32", "adain", None, True, 32, 32, 8),          # ops.upsample2 on the shortcut
    ("adain-32-32", "adain", None, False, 32, 32, 8),            # bottleneck
    ("res-norm-down-64-128", "res", True, True, 64, 128, 16),
    ("adain-up-128-64", "adain", None, True, 128, 64, 16),
]
BLOCK_IDS = [b[0] for b in BLOCKS]


def _block_draw(case, seed):
    name, kind, normalize, resample, din, dout, hw = case
    gen = torch.Generator().manual_seed(seed)
    shapes = O._resblk_shapes("", din, dout, normalize) if kind == "res" else O._adain_resblk_shapes("", din, dout, STYLE_DIM)
    S = he_state(shapes, gen)
    x = bf16_valued((2, din, hw, hw), gen)
    s = torch.randn(2, STYLE_DIM, generator=gen) if kind == "adain" else None
    ho = hw // 2 if (kind == "res" and resample) else (hw * 2 if (kind == "adain" and resample) else hw)
    gy = bf16_valued((2, dout, ho, ho), gen)
    return dict(case=case, seed=seed, S=S, x=x, s=s, gy=gy)


def block_oracle(P, store, s=None):
    """-> {"out", "dx", ["ds"], parameter gradients} of the block in float64 under ``store``; the block input passes a store first, as
    the tensor a neighbouring op (or to_nhwc) wrote"""
    name, kind, normalize, resample, din, dout, hw = P["case"]
    S = {k: v.double().requires_grad_(True) for k, v in P["S"].items()}
    x = P["x"].double().requires_grad_(True)
    s = (P["s"] if s is None else s)
    leaves = [x] + list(S.values())
    if kind == "res":
        out = O.resblk(S, "", store(x), normalize, resample, store)
    else:
        s = s.double().requires_grad_(True)
        leaves.append(s)
        out = O.adain_resblk(S, "", store(x), s, resample, store)
    grads = torch.autograd.grad(out, leaves, P["gy"].double())
    res = {"out": out.detach(), "dx": grads[0]}
    res.update({k: g for k, g in zip(S, grads[1:])})
    if kind == "adain":
        res["ds"] = grads[-1]
    return res


@functools.lru_cache(maxsize=None)
def block_problem(name):
    """The case's draw for the first seed whose float64 reference leaves fewer than 3/4 of the permitted share of its LeakyReLU
    pre-activations inside the kink band -- a condition on the reference alone (the share is a density: about 0.8 x band / sigma for a
    normal pre-activation, more behind an AdaIN whose 1 + gamma is small for some channels) -- with the reference and the emulation."""
    case = BLOCKS[BLOCK_IDS.index(name)]
    for seed in range(11 + BLOCK_IDS.index(name), 2000, 100):
        P = _block_draw(case, seed)
        pres = []
        with recorded_preactivations(pres):
            ref = block_oracle(P, O._same)
        if kink_share(pres) < 0.75 * KINK_SHARE:
            break
    else:
        raise AssertionError("no draw clear of the kink band")
    P["ref"], P["pres"] = ref, pres
    P["emul"] = block_oracle(P, BF16_STORE)
    return P


# ---- part 2: the networks and the loss graphs at the reference's init ------------------------------------------------------------------
NETS = ("generator", "mapping_network", "style_encoder", "discriminator")
SHAPES = {"generator": O.generator_state_shapes, "mapping_network": O.mapping_state_shapes, "style_encoder": O.style_encoder_state_shapes,
          "discriminator": O.discriminator_state_shapes}
BATCH = 2


@functools.lru_cache(maxsize=None)
def net_problem():
    """O.Cfg() (img 64), batch 2: He init + random biases, images uniform in [-1, 1], z ~ N(0, 1), y_org != y_trg for both samples"""
    cfg = O.Cfg()
    gen = torch.Generator().manual_seed(2024)
    N = {n: he_state(SHAPES[n](cfg), gen) for n in NETS}
    img = lambda: torch.rand(BATCH, 3, cfg.img_size, cfg.img_size, generator=gen) * 2.0 - 1.0
    x_real, x_ref, x_ref2 = img(), img(), img()
    z_trg, z_trg2 = torch.randn(BATCH, cfg.latent_dim, generator=gen), torch.randn(BATCH, cfg.latent_dim, generator=gen)
    y_org, y_trg = torch.tensor([0, 1]), torch.tensor([1, 0])
    return dict(cfg=cfg, N=N, x_real=x_real, x_ref=x_ref, x_ref2=x_ref2, z_trg=z_trg, z_trg2=z_trg2, y_org=y_org, y_trg=y_trg)


def _states64(P, grad):
    return {n: {k: v.double().requires_grad_(grad) for k, v in S.items()} for n, S in P["N"].items()}


@functools.lru_cache(maxsize=None)
def forwards(mode):
    """-> {"s_map", "s_enc", "x_fake", "d_out"} in float64 under STORES[mode]"""
    P, store = net_problem(), STORES[mode]
    cfg, N = P["cfg"], _states64(P, False)
    with torch.no_grad():
        s_map = O.mapping_network(N["mapping_network"], P["z_trg"].double(), P["y_trg"], cfg)
        return {"s_map": s_map,
                "s_enc": O.style_encoder(N["style_encoder"], P["x_ref"].double(), P["y_trg"], cfg, store),
                "x_fake": O.generator(N["generator"], P["x_real"].double(), s_map, cfg, store),
                "d_out": O.discriminator(N["discriminator"], P["x_real"].double(), P["y_org"], cfg, store)}


GRAPHS = {"d_latent": ("discriminator",), "g_latent": ("generator", "mapping_network", "style_encoder"),
          "g_ref": ("generator", "style_encoder")}


@functools.lru_cache(maxsize=None)
def loss_graph(graph, mode):
    """-> ({term: value}, {net: {key: gradient}}) of compute_d_loss (latent) / compute_g_loss (latent, reference) in float64 under
    STORES[mode], lambda_ds = lambda_cyc = 1 (the diversity term included)"""
    P, store = net_problem(), STORES[mode]
    cfg, N = P["cfg"], _states64(P, True)
    assert cfg.lambda_ds == 1.0 and cfg.lambda_cyc == 1.0
    d = lambda k: P[k].double()
    if graph == "d_latent":
        loss, terms = O.compute_d_loss(N, d("x_real"), P["y_org"], P["y_trg"], cfg, z_trg=d("z_trg"), store=store)
    elif graph == "g_latent":
        loss, terms = O.compute_g_loss(N, d("x_real"), P["y_org"], P["y_trg"], cfg, z_trgs=(d("z_trg"), d("z_trg2")), store=store)
    else:
        loss, terms = O.compute_g_loss(N, d("x_real"), P["y_org"], P["y_trg"], cfg, x_refs=(d("x_ref"), d("x_ref2")), store=store)
    return terms, {n: {k: g.detach() for k, g in O.grads_of(loss, N[n]).items() if g is not None} for n in GRAPHS[graph]}


def style_codes(graph):
    """the two style codes of the diversity term on the float64 reference"""
    P = net_problem()
    cfg, N = P["cfg"], _states64(P, False)
    with torch.no_grad():
        if graph == "g_latent":
            return [O.mapping_network(N["mapping_network"], P[k].double(), P["y_trg"], cfg) for k in ("z_trg", "z_trg2")]
        return [O.style_encoder(N["style_encoder"], P[k].double(), P["y_trg"], cfg) for k in ("x_ref", "x_ref2")]


def flat(grads, keys=None):
    return torch.cat([grads[k].detach().double().cpu().flatten() for k in (keys or grads)])


def cosine(a, b):
    return float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-300))
