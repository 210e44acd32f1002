"""GPU: ops.diff_augment (csrc/diffaug.hip) against the oracle's DiffAugment from the same seed -- forward, the input gradient (VJP)
and the second-order gradient the R1 penalty takes through it -- plus run-to-run bit reproducibility and the empty policy."""
import pytest
import torch

from oracle import defectgan_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POLICIES = ["color", "translation", "cutout", "color,translation,cutout", "translation,color"]
SHAPES = [(2, 3, 64, 64), (8, 3, 256, 256), (3, 3, 33, 47)]


def _image(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("policy", POLICIES)
def test_forward_matches_the_oracle(policy, shape):
    from de_i2i_gan_amd import ops
    x = _image(shape, 1)
    torch.manual_seed(21)
    ref = O.diff_augment(x, policy)
    after = torch.rand(1)
    torch.manual_seed(21)
    got = ops.diff_augment(x.to(DEV), policy)
    assert torch.equal(torch.rand(1), after)           # the same host draws
    assert got.shape == ref.shape and got.is_contiguous()
    assert float((got.cpu() - ref).abs().max()) <= 1e-5


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (3, 3, 33, 47)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("policy", POLICIES)
def test_first_and_second_order_gradients_match_the_oracle(policy, shape):
    """the VJP, and d/dx of <w, (dL/dx)^2> with dL/dx taken with create_graph=True (the R1 pattern: the adjoint differentiated again)
    -- through a nonlinear consumer, so the second-order term is not zero"""
    from de_i2i_gan_amd import ops
    x = _image(shape, 2) * 2 - 1
    gy = _image(shape, 3) - 0.5
    w = _image(shape, 4)

    def run(aug, xx, gyy, ww):
        y = aug(xx)
        loss = (y * gyy).sum() + 0.25 * (y * y * gyy).sum()
        (gx,) = torch.autograd.grad(loss, xx, create_graph=True)
        (ggx,) = torch.autograd.grad((ww * gx * gx).sum(), xx)
        return gx, ggx

    torch.manual_seed(33)
    xo = x.clone().double().requires_grad_(True)
    ref_gx, ref_ggx = run(lambda t: O.diff_augment(t, policy), xo, gy.double(), w.double())
    torch.manual_seed(33)
    xd = x.to(DEV).requires_grad_(True)
    gx, ggx = run(lambda t: ops.diff_augment(t, policy), xd, gy.to(DEV), w.to(DEV))
    assert _rel_l2(gx, ref_gx) < 1e-5, _rel_l2(gx, ref_gx)
    assert _rel_l2(ggx, ref_ggx) < 1e-5, _rel_l2(ggx, ref_ggx)


def test_vjp_of_a_linear_loss_matches_the_oracle_at_the_default_size():
    from de_i2i_gan_amd import ops
    shape = (8, 3, 256, 256)
    x, gy = _image(shape, 5), _image(shape, 6) - 0.5
    policy = "color,translation,cutout"
    torch.manual_seed(44)
    xo = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad((O.diff_augment(xo, policy) * gy).sum(), xo)
    torch.manual_seed(44)
    xd = x.to(DEV).requires_grad_(True)
    (got,) = torch.autograd.grad((ops.diff_augment(xd, policy) * gy.to(DEV)).sum(), xd)
    assert _rel_l2(got, ref) < 1e-5


@pytest.mark.parametrize("shape", [(8, 3, 256, 256), (3, 3, 33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_same_seed_runs_are_bit_identical(shape):
    from de_i2i_gan_amd import ops
    x = _image(shape, 7).to(DEV)
    gy = _image(shape, 8).to(DEV)
    outs = []
    for _ in range(2):
        torch.manual_seed(55)
        xx = x.clone().requires_grad_(True)
        y = ops.diff_augment(xx, "color,translation,cutout")
        (gx,) = torch.autograd.grad((y * gy).sum(), xx)
        outs.append((y.detach(), gx))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_empty_policy_returns_the_input_object_without_a_draw():
    from de_i2i_gan_amd import ops
    x = torch.rand(2, 3, 8, 8, device=DEV)
    torch.manual_seed(9)
    expect = torch.rand(1)
    torch.manual_seed(9)
    assert ops.diff_augment(x, "") is x
    assert torch.equal(torch.rand(1), expect)


def test_unknown_policy_raises_key_error():
    from de_i2i_gan_amd import ops
    with pytest.raises(KeyError):
        ops.diff_augment(torch.rand(2, 3, 8, 8, device=DEV), "color,zoom")
