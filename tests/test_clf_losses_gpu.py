"""ops.cce_logits and ops.mse (csrc/reduce.hip: cce_*_kernel, mse_*_kernel) against float64 torch on the CPU.

The reference is F.cross_entropy (float class-weight targets) / F.mse_loss in float64; the loss is multiplied by 1.7 before
backward(), as test_reduce_edges_gpu.py's _check_bce does.  Error measures, each bounded by 1e-5 -- the bound that file applies to
the fp32 bce / l1 kernels against float64:
    e_loss = |out - ref| / max(1, |ref|)
    e_rel  = max|dx - ref| / max|ref|
    e_abs  = max|dx - ref| / (1.7 / rows * max(1, max_r S_r)),  S_r = sum_c t[r][c]: the error in units of the largest gradient a row of
             that weight can have -- used where the logits are so peaked that the true gradient is ~0 and e_rel would only measure
             cancellation.
Where the float64 gradient is identically zero (one class; all-zero targets) e_rel is 0 / 0: there the kernel's loss and gradient
must be exactly 0, which is what its arithmetic gives (S * 1 - t with S = t, and every term scaled by S = 0).

Seams of the cce kernels: one wavefront per row and lane l owns classes l, l + 64, ... (63 / 64 / 65 classes: the last lane idle, every
lane once, a second trip; 256 and 1000: four trips, sixteen ragged ones); four rows per workgroup (1, 2, 3, 5 rows: ragged quads; 4:
exactly one); one partial per workgroup, summed by a 256-thread finalize (257 rows: 65 partials; 1025 rows: 257 partials, one past
the finalize's first trip); at most 1024 workgroups (4096 rows: the cap reached exactly; 4101: a grid-stride second trip with a ragged
quad).  `classes` has no cap.  mse follows l1: 256 elements per workgroup, 1024 workgroups (262149 = 262144 + 5: five elements of the
second trip)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 1e-5
CCE_SHAPES = [(1, 1), (1, 2), (2, 6), (32, 6), (64, 6), (3, 7), (257, 5), (1025, 6), (5, 63), (5, 64), (5, 65), (4, 256), (3, 1000),
              (4096, 3), (4101, 3)]            # the last two: the 1024-workgroup cap of this kernel (see the docstring)
CCE_TARGETS = ["onehot", "multihot", "soft", "onehot_row0_zero"]
CCE_SCALES = [3.0, 30.0, 1e4]
MSE_N = [1, 3, 4, 255, 256, 257, 262149]


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


def dev():
    return torch.device("cuda:0")


def note(*a):
    print("[clf-losses]", *a, flush=True)


@functools.lru_cache(maxsize=None)
def _cce_inputs(rows, classes):
    """unit-scale logits and the four targets of one shape, from one generator seeded rows * 1000 + classes"""
    g = torch.Generator().manual_seed(rows * 1000 + classes)
    x = torch.randn(rows, classes, generator=g)
    index = torch.randint(0, classes, (rows,), generator=g)
    onehot = F.one_hot(index, classes).float()
    multihot = (torch.rand(rows, classes, generator=g) < 0.4).float()
    soft = torch.softmax(torch.randn(rows, classes, generator=g), dim=1)
    zeroed = onehot.clone()
    zeroed[0] = 0
    return x, index, {"onehot": onehot, "multihot": multihot, "soft": soft, "onehot_row0_zero": zeroed}


@functools.lru_cache(maxsize=None)
def _cce_problem(rows, classes, target, scale):
    """logits, target and the float64 reference (loss, gradient of 1.7 * loss); computed once, never modified"""
    x, _, targets = _cce_inputs(rows, classes)
    x, t = x * scale, targets[target]
    xr = x.double().requires_grad_(True)
    ref = F.cross_entropy(xr, t.double())
    (gref,) = torch.autograd.grad(ref * 1.7, xr)
    return x, t, ref.item(), gref


def _check_cce(ops, rows, classes, target, scale):
    x, t, ref, gref = _cce_problem(rows, classes, target, scale)
    xg = x.to(dev()).requires_grad_(True)
    out = ops.cce_logits(xg, t.to(dev()))
    (out * 1.7).backward()
    assert out.shape == () and out.dtype == torch.float32 and xg.grad.shape == x.shape
    got, dx = out.detach().item(), xg.grad.double().cpu()
    tag = f"cce ({rows},{classes}) {target} scale {scale:g}"
    assert torch.isfinite(out).item() and bool(torch.isfinite(xg.grad).all()), tag
    e_loss = abs(got - ref) / max(1.0, abs(ref))
    err = (dx - gref).abs().max().item()
    e_abs = err / (1.7 / rows * max(1.0, t.sum(1).max().item()))
    if gref.abs().max().item() == 0.0:            # one class, or no target weight at all: exact zeros
        note(f"{tag}: zero gradient; loss {got!r} max|dx| {dx.abs().max().item()!r}")
        assert dx.abs().max().item() == 0.0, tag
        if classes == 1 or t.sum().item() == 0.0:
            assert got == 0.0, tag
        e_rel = 0.0
    else:
        e_rel = err / gref.abs().max().item()
    note(f"{tag}: e_loss {e_loss:.3e} e_rel {e_rel:.3e} e_abs {e_abs:.3e} (bound {BOUND:.0e})")
    assert e_loss < BOUND, (tag, e_loss)
    if scale <= 3.0:
        assert e_rel < BOUND, (tag, e_rel)
    else:
        assert e_abs < BOUND, (tag, e_abs)
    return out.detach(), xg.grad


@pytest.mark.parametrize("target", CCE_TARGETS)
@pytest.mark.parametrize("shape", CCE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cce_logits_against_float64(ops, shape, target):
    """Every shape of the table with every target kind at the three logit scales: randn * 3 (e_loss, e_rel), randn * 30 and
    randn * 1e4 (e_loss, e_abs, everything finite)."""
    for scale in CCE_SCALES:
        _check_cce(ops, shape[0], shape[1], target, scale)


def test_cce_single_class_is_exactly_zero(ops):
    """(1, 1): lse = x, softmax = 1 -- loss 0 and gradient 0 exactly, for a weight of 1 and of 2.5"""
    for w in (1.0, 2.5):
        xg = torch.tensor([[0.37]], device=dev(), requires_grad=True)
        out = ops.cce_logits(xg, torch.tensor([[w]], device=dev()))
        (out * 1.7).backward()
        assert out.item() == 0.0 and xg.grad.item() == 0.0


def test_cce_onehot_equals_the_class_index_form(ops):
    for rows, classes in [(32, 6), (5, 65), (1025, 6)]:
        x, index, targets = _cce_inputs(rows, classes)
        x = x * 3
        ref = F.cross_entropy(x.double(), index).item()
        out = ops.cce_logits(x.to(dev()), targets["onehot"].to(dev())).item()
        e = abs(out - ref) / max(1.0, abs(ref))
        note(f"cce ({rows},{classes}) one-hot vs F.cross_entropy(x, index): {e:.3e}")
        assert e < BOUND


def test_cce_accepts_rank4_and_bf16_logits_and_refuses_spatial_ones(ops):
    rows, classes = 32, 6
    x, t, ref, gref = _cce_problem(rows, classes, "onehot", 3.0)
    x4 = x.view(rows, classes, 1, 1).to(dev()).requires_grad_(True)
    out = ops.cce_logits(x4, t.view(rows, classes, 1, 1).to(dev()))
    (out * 1.7).backward()
    assert x4.grad.shape == (rows, classes, 1, 1)
    flat = ops.cce_logits(x.to(dev()), t.to(dev()))
    assert torch.equal(out.detach(), flat)                       # the same kernel on the same bytes
    assert abs(out.item() - ref) / max(1.0, abs(ref)) < BOUND
    assert ((x4.grad.double().cpu().view(rows, classes) - gref).abs().max() / gref.abs().max()).item() < BOUND
    assert torch.equal(ops.cce_logits(x.to(dev()), t.view(-1).to(dev())), flat)       # the target's element count is what matters

    xb = x.to(torch.bfloat16)                                    # bf16 logits: converted to fp32, so the reference is on the rounded values
    xbg = xb.to(dev()).requires_grad_(True)
    outb = ops.cce_logits(xbg, t.to(dev()))
    (outb * 1.7).backward()
    xr = xb.double().requires_grad_(True)
    refb = F.cross_entropy(xr, t.double())
    (grefb,) = torch.autograd.grad(refb * 1.7, xr)
    assert outb.dtype == torch.float32 and xbg.grad.dtype == torch.bfloat16
    assert abs(outb.item() - refb.item()) / max(1.0, abs(refb.item())) < BOUND
    # the gradient comes back rounded to bf16 (2^-9 relative per element)
    assert ((xbg.grad.double().cpu() - grefb).abs().max() / grefb.abs().max()).item() < 2.0 ** -8

    for bad in [torch.zeros(4, 6, 2, 2), torch.zeros(6), torch.zeros(0, 6)]:
        with pytest.raises(ValueError, match="cce_logits"):
            ops.cce_logits(bad.to(dev()), torch.zeros(max(bad.numel(), 1)).to(dev()))
    with pytest.raises(ValueError, match="target size"):
        ops.cce_logits(torch.zeros(4, 6, device=dev()), torch.zeros(4, 5, device=dev()))
    with pytest.raises(ValueError, match="cce_logits"):
        ops.cce_logits(torch.zeros(4, 6, device=dev()), 1.0)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.cce_logits(torch.zeros(4, 6), torch.zeros(4, 6))


# ---- mse --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mse_problem(n, kind):
    """kind: 'tensor' | 'const' | 'grad' (b requires a gradient)"""
    g = torch.Generator().manual_seed(n + 11)
    a = torch.randn(n, generator=g) * 1.5 + 0.2
    b = None if kind == "const" else torch.randn(n, generator=g)
    ar = a.double().requires_grad_(True)
    br = b.double().requires_grad_(kind == "grad") if b is not None else torch.full_like(ar, 0.25)
    ref = F.mse_loss(ar, br)
    grefs = torch.autograd.grad(ref * 1.7, [ar] + ([br] if kind == "grad" else []))
    return a, b, ref.item(), grefs


def _check_mse(ops, n, kind):
    a, b, ref, grefs = _mse_problem(n, kind)
    ag = a.to(dev()).requires_grad_(True)
    bg = 0.25 if b is None else b.to(dev()).requires_grad_(kind == "grad")
    out = ops.mse(ag, bg)
    (out * 1.7).backward()
    assert out.shape == () and out.dtype == torch.float32
    e_loss = abs(out.item() - ref) / max(1.0, abs(ref))
    e_rel = ((ag.grad.double().cpu() - grefs[0]).abs().max() / grefs[0].abs().max()).item()
    note(f"mse n={n} b={kind}: e_loss {e_loss:.3e} e_rel {e_rel:.3e} (bound {BOUND:.0e})")
    assert e_loss < BOUND and e_rel < BOUND
    if kind == "grad":
        assert torch.equal(bg.grad, -ag.grad), "db must be -da bit for bit"
        assert ((bg.grad.double().cpu() - grefs[1]).abs().max() / grefs[1].abs().max()).item() < BOUND
    elif b is not None:
        assert bg.grad is None
    return out.detach(), ag.grad


@pytest.mark.parametrize("kind", ["tensor", "const", "grad"])
@pytest.mark.parametrize("n", MSE_N)
def test_mse_against_float64(ops, n, kind):
    _check_mse(ops, n, kind)


@pytest.mark.parametrize("n", MSE_N)
def test_mse_of_integer_data_is_exact_to_two_roundings(ops, n):
    """(a - b)^2 of small integers with |a - b| <= 3 sums exactly in fp32 in any order (the total stays below 2^24), so the loss
    may differ from float64 only by the rounding of 1 / n and of the product: 2^-22 relative.  One dropped or doubled element (a
    term of at least 1 in a total of at most 9 n) moves it by at least 1 / (9 n) = 4.2e-7 at the largest n: 1.8 times the bound."""
    g = torch.Generator().manual_seed(n)
    a = torch.randint(-4, 5, (n,), generator=g).float()
    b = a + torch.randint(1, 4, (n,), generator=g).float() * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)
    assert (a - b).pow(2).sum().item() < 2 ** 24
    ref = (a.double() - b.double()).pow(2).mean().item()
    out = ops.mse(a.to(dev()), b.to(dev()))
    e = abs(out.item() - ref) / ref
    note(f"mse integers n={n}: {e:.3e} (bound {2.0 ** -22:.2e})")
    assert e <= 2.0 ** -22


def test_mse_target_forms_and_refusals(ops):
    a = torch.arange(6, dtype=torch.float32, device=dev()).view(2, 3)
    assert ops.mse(a, 1).item() == ops.mse(a, torch.ones_like(a)).item()
    assert ops.mse(a).item() == ops.mse(a, 0.0).item() == ops.mse(a, None).item()
    with pytest.raises(ValueError, match="target size"):
        ops.mse(a, torch.ones(5, device=dev()))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.mse(torch.zeros(4), 0.0)


def test_l1_refuses_a_shorter_target(ops):
    """A ``b`` of fewer elements than ``a`` is refused (the kernel would read ``a.numel()`` elements of it); without ``b``, and with
    one of ``a``'s size, the value is float64's: small integers and n = 8, so every sum and the 1 / n are exact in fp32."""
    a = (torch.arange(8, dtype=torch.float32) - 3).view(2, 4)
    b = torch.ones(8).view(2, 4)
    with pytest.raises(ValueError, match="target size"):
        ops.l1(a.to(dev()), torch.ones(4, device=dev()))
    assert ops.l1(a.to(dev()), None).item() == a.double().abs().mean().item()
    assert ops.l1(a.to(dev()), b.to(dev())).item() == (a.double() - b.double()).abs().mean().item()


# ---- state and reproducibility ----------------------------------------------------------------------------------------------
def test_smaller_call_after_larger_does_not_read_stale_partials(ops):
    """The block partials live in one process-wide buffer that is never cleared: (1025, 6) leaves 257 partials, (2, 6) must read one;
    mse of 262149 leaves 1024, mse of 3 must read one."""
    _check_cce(ops, 1025, 6, "onehot", 3.0)
    _check_cce(ops, 2, 6, "onehot", 3.0)
    _check_mse(ops, 262149, "tensor")
    _check_mse(ops, 3, "tensor")
    _check_cce(ops, 2, 6, "soft", 3.0)


def test_two_calls_give_the_same_bits(ops):
    for args in [(1025, 6, "multihot", 3.0), (3, 1000, "soft", 30.0), (4101, 3, "onehot", 3.0)]:
        (o1, g1), (o2, g2) = _check_cce(ops, *args), _check_cce(ops, *args)
        assert torch.equal(o1, o2) and torch.equal(g1, g2), args
    (o1, g1), (o2, g2) = _check_mse(ops, 262149, "tensor"), _check_mse(ops, 262149, "tensor")
    assert torch.equal(o1, o2) and torch.equal(g1, g2)
