"""GPU: flip and rot90 through the stack -- ops.diff_augment with host draws against the torch-op policy functions on the CPU from
one seed (exact for pure blits; the 1e-5 bounds of tests/test_diffaug_op_gpu.py where a color / translation / cutout run is mixed
in), first- and second-order gradients in the R1 pattern, the sharded call, the defectGAN trainer eager against graph_step and
stopped-and-resumed against uninterrupted (train_state), and stargan-v2's compute_d_loss through DiffAugment = "flip,rot90"."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C32 = dict(image_size=32, batch=2, num_layers=3, ngf=8, ndf=8, hidden_nc=16)
ALL = "flip,rot90,color,translation,cutout"


def _arange(n, c, h, w):
    return torch.arange(n * c * h * w, dtype=torch.float32).view(n, c, h, w)


def _image(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _cpu(x, policy):
    from de_i2i_gan_amd.utils.diffaug import diff_augment
    return diff_augment(x, policy)


# ---- the op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy, shape", [("flip,rot90", (16, 3, 33, 33)), ("rot90,flip", (16, 1, 32, 32)), ("flip", (8, 3, 5, 12)),
                                           ("rot90", (8, 2, 65, 65))])
def test_pure_blits_equal_the_cpu_functions_from_one_seed(policy, shape):
    from de_i2i_gan_amd import ops
    x = _arange(*shape)
    torch.manual_seed(21)
    ref = _cpu(x, policy)
    after = torch.rand(1)
    torch.manual_seed(21)
    got = ops.diff_augment(x.to(DEV), policy)
    assert torch.equal(torch.rand(1), after)           # the same host draws
    assert got.is_contiguous() and torch.equal(got.cpu(), ref) and not torch.equal(ref, x)


@pytest.mark.parametrize("policy", ["flip,color,translation", "rot90,cutout,flip", ALL])
def test_mixed_policies_match_the_cpu_functions(policy):
    from de_i2i_gan_amd import ops
    x = _image((3, 3, 33, 33), 1)
    torch.manual_seed(22)
    ref = _cpu(x, policy)
    after = torch.rand(1)
    torch.manual_seed(22)
    got = ops.diff_augment(x.to(DEV), policy)
    assert torch.equal(torch.rand(1), after)
    assert float((got.cpu() - ref).abs().max()) <= 1e-5


def _r1(aug, xx, gyy, ww):
    """the VJP, and d/dx of <w, (dL/dx)^2> with dL/dx taken with create_graph=True, through a nonlinear consumer"""
    y = aug(xx)
    loss = (y * gyy).sum() + 0.25 * (y * y * gyy).sum()
    (gx,) = torch.autograd.grad(loss, xx, create_graph=True)
    (ggx,) = torch.autograd.grad((ww * gx * gx).sum(), xx)
    return gx.detach(), ggx.detach()


def test_gradients_of_pure_blits_are_exact():
    """small integers: every value of the loss graph is an integer far below 2^24 on either device, so the CPU functions' autograd
    and the kernels' inverse launches agree bit for bit"""
    from de_i2i_gan_amd import ops
    gen = torch.Generator().manual_seed(5)
    shape = (16, 2, 33, 33)
    x, gy, w = (torch.randint(-3, 4, shape, generator=gen).float() for _ in range(3))
    gy = gy * 4                                              # (0.25 y y gy stays an integer)
    torch.manual_seed(33)
    ref = _r1(lambda t: _cpu(t, "flip,rot90"), x.clone().requires_grad_(True), gy, w)
    torch.manual_seed(33)
    got = _r1(lambda t: ops.diff_augment(t, "flip,rot90"), x.to(DEV).requires_grad_(True), gy.to(DEV), w.to(DEV))
    for name, a, b in zip(("gradient", "second-order gradient"), got, ref):
        assert torch.equal(a.cpu(), b), name
    assert float(got[1].abs().max()) > 0


@pytest.mark.parametrize("policy", ["flip,color,translation", "rot90,cutout,flip"])
def test_gradients_of_mixed_policies_match_the_cpu_functions(policy):
    from de_i2i_gan_amd import ops
    shape = (3, 3, 33, 33)
    x, gy, w = _image(shape, 2) * 2 - 1, _image(shape, 3) - 0.5, _image(shape, 4)
    torch.manual_seed(34)
    ref = _r1(lambda t: _cpu(t, policy), x.clone().double().requires_grad_(True), gy.double(), w.double())
    torch.manual_seed(34)
    got = _r1(lambda t: ops.diff_augment(t, policy), x.to(DEV).requires_grad_(True), gy.to(DEV), w.to(DEV))
    assert _rel_l2(got[0], ref[0]) < 1e-5 and _rel_l2(got[1], ref[1]) < 1e-5, (_rel_l2(got[0], ref[0]), _rel_l2(got[1], ref[1]))


def test_sharded_calls_equal_the_slices():
    from de_i2i_gan_amd import ops
    x = _arange(8, 3, 16, 16).to(DEV)
    torch.manual_seed(6)
    whole = ops.diff_augment(x, "flip,rot90")
    after = torch.rand(1)
    for rank in range(2):
        torch.manual_seed(6)
        with ops.diffaug_sharded(rank, 2):
            part = ops.diff_augment(x[4 * rank:4 * rank + 4].contiguous(), "flip,rot90")
        assert torch.equal(torch.rand(1), after) and torch.equal(part, whole[4 * rank:4 * rank + 4])
    rng = ops.DiffAugRng(77, DEV)
    gate = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    for p in (None, gate):
        rng.set_state((77, 3))
        whole = ops.diff_augment(x, ALL, rng=rng, p=p)
        assert rng.state() == (77, 5)
        rng.set_state((77, 3))
        with ops.diffaug_sharded(1, 2):
            assert torch.equal(ops.diff_augment(x[4:8].contiguous(), ALL, rng=rng, p=p), whole[4:8])


def test_device_drawn_blits_apply_the_drawn_codes():
    from de_i2i_gan_amd import ops
    import blit_reference as R
    x = _arange(8, 2, 9, 9)
    rng = ops.DiffAugRng(5, DEV)
    rng.set_state((5, 2))
    got = ops.diff_augment(x.to(DEV), "flip,rot90", rng=rng)
    codes = R.draw_codes(5, 2, "flip,rot90", 8, 0)[0]
    assert torch.equal(got.cpu(), torch.from_numpy(R.blit(x.numpy(), codes))) and len(set(codes.tolist())) > 2


# ---- the defectGAN trainer ---------------------------------------------------------------------------------------------------
def test_model_refuses_rot90_on_non_square_images_before_a_draw():
    from de_i2i_gan_amd.models.defectgan_model import DefectGanModel
    from helpers import make_opt
    for over in ({}, dict(diff_aug_rng="device", diff_aug_seed=3)):
        model = DefectGanModel(make_opt(C32, DEV, "bf16", diff_aug="flip,rot90", **over))
        host = torch.get_rng_state()
        with pytest.raises(ValueError, match="rot90"):
            model._diff_augment(torch.zeros(2, 3, 32, 16, device=DEV), "flip,rot90")
        assert torch.equal(torch.get_rng_state(), host)
        assert model.diffaug_rng is None or model.diffaug_rng.state() == (3, 0)


@pytest.mark.parametrize("gated", [False, True], ids=["p=1", "p=0.5"])
def test_graph_step_equals_eager_with_all_five_policies(gated):
    from test_graph_step_gpu import compare
    over = dict(diff_aug_p=0.5) if gated else {}
    tr = compare(C32, steps=5, warmup=2, diff_aug=ALL, diff_aug_rng="device", diff_aug_seed=1234, **over)
    assert tr.model.diffaug_rng.state() == (1234, 5 * 6 * 2)        # six calls per step, an affine and a blit draw each


def test_a_resumed_run_is_the_uninterrupted_run():
    from test_train_state_gpu import check_resume
    want, _ = check_resume(k=2, diff_aug=ALL, diff_aug_rng="device", diff_aug_seed=1234)
    assert want["diffaug_rng"] == (1234, 4 * 6 * 2)


# ---- stargan-v2 --------------------------------------------------------------------------------------------------------------
def test_stargan_d_loss_with_blits_and_r1_through_them_matches_the_cpu_functions():
    from oracle import starganv2_oracle as O
    from test_starganv2_gpu import build
    from test_starganv2_oracle_goldens import load, states
    from de_i2i_gan_amd.stargan import compute_d_loss
    policy = "flip,rot90"
    meta, arr, cfg = load()
    args, nets, _ = build(cfg, "f32")
    args.DiffAugment = policy
    x_real, y_org, y_trg, _, _, z_trg, _ = O.synthetic_inputs(cfg, meta["batch"])
    torch.manual_seed(123)
    loss, ls = compute_d_loss(nets, args, x_real.to(DEV), y_org.to(DEV), y_trg.to(DEV), z_trg=z_trg.to(DEV))
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(p.grad).all()) for p in nets.discriminator.parameters())
    _, N = states(cfg)
    O.require_grad(N["discriminator"], True)
    torch.manual_seed(123)
    xr = x_real.detach().requires_grad_(True)
    out = O.discriminator(N["discriminator"], _cpu(xr, policy), y_org, cfg)
    want = {"real": float(O.adv_loss(out, 1).detach()), "reg": float(O.r1_reg(out, xr).detach())}
    with torch.no_grad():
        x_fake = O.generator(N["generator"], xr, O.style_code(N, y_trg, cfg, None, z_trg), cfg)
    want["fake"] = float(O.adv_loss(O.discriminator(N["discriminator"], _cpu(x_fake, policy), y_trg, cfg), 0))
    for k in ("real", "fake", "reg"):
        assert abs(getattr(ls, k) - want[k]) < 1e-4 * abs(want[k]), (k, getattr(ls, k), want[k])
