"""GPU: scale, rotate and aniso through ops.diff_augment -- host draws against the torch-op functions of utils/diffaug.py on the CPU from
one RNG state (bit for bit where the policy holds warp runs only; the 1e-5 bound of tests/test_blit_op_gpu.py where other runs are
mixed in), first- and second-order gradients in the R1 pattern, device draws against the table-fed launch, and two ranks on their
rows against one process on the batch."""
import numpy as np
import pytest
import torch

import warp_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
ALL = "scale,rotate,aniso"
MIXED = "color,rotate,scale,aniso,flip"


def _image(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _cpu(x, policy):
    from de_i2i_gan_amd.utils.diffaug import diff_augment
    return diff_augment(x, policy)


@pytest.mark.parametrize("policy, shape", [(ALL, (6, 3, 33, 33)), ("rotate,scale", (4, 1, 5, 12)), ("scale", (3, 2, 9, 7)),
                                           ("aniso,rotate,rotate", (3, 3, 16, 16))])
def test_warp_policies_equal_the_cpu_functions_from_one_seed_bit_for_bit(policy, shape):
    from de_i2i_gan_amd import ops
    x = _image(shape, 1) - 0.5
    torch.manual_seed(21)
    ref = _cpu(x, policy)
    after = torch.rand(1)
    torch.manual_seed(21)
    got = ops.diff_augment(x.to(DEV), policy)
    assert torch.equal(torch.rand(1), after)                          # the same host draws
    assert got.is_contiguous() and torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32)) and not torch.equal(ref, x)


@pytest.mark.parametrize("policy", [MIXED, "translation,scale,cutout,rot90,aniso"])
def test_mixed_policies_match_the_cpu_functions(policy):
    from de_i2i_gan_amd import ops
    x = _image((3, 3, 33, 33), 2)
    torch.manual_seed(22)
    ref = _cpu(x, policy)
    after = torch.rand(1)
    torch.manual_seed(22)
    got = ops.diff_augment(x.to(DEV), policy)
    assert torch.equal(torch.rand(1), after)
    assert float((got.cpu() - ref).abs().max()) <= 1e-5


def _r1(aug, xx, gyy, ww):
    """the VJP, and d/dx of <w, (dL/dx)^2> with dL/dx taken with create_graph=True, through a loss quadratic in the output"""
    y = aug(xx)
    loss = (y * gyy).sum() + 0.25 * (y * y * gyy).sum()
    (gx,) = torch.autograd.grad(loss, xx, create_graph=True)
    (ggx,) = torch.autograd.grad((ww * gx * gx).sum(), xx)
    return gx.detach(), ggx.detach()


@pytest.mark.parametrize("policy", [ALL, "rotate,scale", MIXED])
def test_first_and_second_order_gradients_match_the_cpu_functions(policy):
    from de_i2i_gan_amd import ops
    shape = (3, 3, 17, 19) if "flip" not in policy else (3, 3, 17, 17)
    x, gy, w = _image(shape, 3) * 2 - 1, _image(shape, 4) - 0.5, _image(shape, 5)
    torch.manual_seed(34)
    ref = _r1(lambda t: _cpu(t, policy), x.clone().double().requires_grad_(True), gy.double(), w.double())
    torch.manual_seed(34)
    got = _r1(lambda t: ops.diff_augment(t, policy), x.to(DEV).requires_grad_(True), gy.to(DEV), w.to(DEV))
    assert float(ref[1].abs().max()) > 0
    assert _rel_l2(got[0], ref[0]) < 1e-5 and _rel_l2(got[1], ref[1]) < 1e-5, (_rel_l2(got[0], ref[0]), _rel_l2(got[1], ref[1]))


def test_the_gradient_of_a_linear_loss_is_the_reference_adjoint_bit_for_bit():
    from de_i2i_gan_amd import ops
    from de_i2i_gan_amd.utils.diffaug import draw_params
    shape = (3, 2, 9, 11)
    x, gy = _image(shape, 6), _image(shape, 7) - 0.5
    torch.manual_seed(35)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.diff_augment(xd, ALL)
    (gx,) = torch.autograd.grad((y * gy.to(DEV)).sum(), xd)
    torch.manual_seed(35)
    rec = draw_params(ALL, 3, 9, 11)[0].view(F)[0]
    assert np.array_equal(gx.cpu().numpy().view(np.int32), R.adjoint(gy.numpy(), rec).view(np.int32))
    assert np.array_equal(y.detach().cpu().numpy().view(np.int32), R.forward(x.numpy(), rec).view(np.int32))


def test_the_adjoints_gradient_is_the_forward():
    """_WarpAdjoint's backward is _Warp: differentiating <W^T g, v> with respect to g gives W v, bit for bit the forward launch"""
    from de_i2i_gan_amd import ops
    shape = (2, 2, 8, 9)
    v, g = _image(shape, 8).to(DEV), (_image(shape, 9) - 0.5).to(DEV).requires_grad_(True)
    rng = ops.DiffAugRng(9, DEV)
    mats = ops.warp_draw(rng, ALL, 2)
    adj = ops._WarpAdjoint.apply(g, mats[0])
    (wv,) = torch.autograd.grad((adj * v).sum(), g)
    assert torch.equal(wv, ops._warp_run(v, mats[0], 0)) and torch.equal(adj.detach(), ops._warp_run(g.detach(), mats[0], 1))


@pytest.mark.parametrize("p", [None, 0.5], ids=["p=1", "p=0.5"])
def test_device_draws_equal_the_table_fed_launches(p):
    from de_i2i_gan_amd import ops
    x = _image((8, 2, 9, 12), 10) - 0.5
    gate = None if p is None else torch.tensor([p], dtype=torch.float32, device=DEV)
    rng = ops.DiffAugRng(5, DEV)
    rng.set_state((5, 2))
    got = ops.diff_augment(x.to(DEV), "rotate,scale", rng=rng, p=gate)
    assert rng.state() == (5, 3)                                      # one draw launch for the two warp runs
    rng.set_state((5, 2))
    mats = ops.warp_draw(rng, "rotate,scale", 8, p=gate)
    want = ops._warp_run(ops._warp_run(x.to(DEV), mats[0], 0), mats[1], 0)
    assert torch.equal(got, want)
    m = mats.cpu().numpy().view(F)
    ref = R.forward(R.forward(x.numpy(), m[0]), m[1])
    assert np.array_equal(got.cpu().numpy().view(np.int32), ref.view(np.int32)) and not np.array_equal(ref, x.numpy())


def test_two_ranks_on_their_rows_equal_one_process_on_the_batch():
    from de_i2i_gan_amd import ops
    x = (_image((8, 3, 16, 16), 11) - 0.5).to(DEV)
    for policy in (ALL, MIXED):
        torch.manual_seed(6)
        whole = ops.diff_augment(x, policy)
        after = torch.rand(1)
        for rank in range(2):
            torch.manual_seed(6)
            with ops.diffaug_sharded(rank, 2):
                part = ops.diff_augment(x[4 * rank:4 * rank + 4].contiguous(), policy)
            assert torch.equal(torch.rand(1), after) and torch.equal(part, whole[4 * rank:4 * rank + 4])
        rng = ops.DiffAugRng(77, DEV)
        gate = torch.tensor([0.5], dtype=torch.float32, device=DEV)
        for p in (None, gate):
            rng.set_state((77, 3))
            whole = ops.diff_augment(x, policy, rng=rng, p=p)
            assert rng.state() == (77, 3 + (3 if policy == MIXED else 1))      # MIXED: an affine, a blit and a warp draw
            for rank in range(2):
                rng.set_state((77, 3))
                with ops.diffaug_sharded(rank, 2):
                    assert torch.equal(ops.diff_augment(x[4 * rank:4 * rank + 4].contiguous(), policy, rng=rng, p=p), whole[4 * rank:4 * rank + 4])
