"""GPU: the stargan-v2 iteration pieces this port adds on top of the reference's networks -- DiffAugment at the reference's three call
sites (core/solver.py:472,481,510) with the R1 penalty through it, the lambda_ds decay (solver.py:311-313), the fused EMA and Adam's
coupled weight decay inside the kernel -- on the sg0 fixture configuration in exact-f32 mode, against the oracle."""
import copy

import pytest
import torch

from oracle import defectgan_oracle as DO
from oracle import starganv2_oracle as O
from test_starganv2_gpu import build, rel_l2
from test_starganv2_oracle_goldens import load, states

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POLICY = "color,translation,cutout"


def _oracle_d_loss(N, x_real, y_org, y_trg, cfg, z_trg):
    """O.compute_d_loss with DiffAugment on x_real and x_fake (solver.py:472,481): real drawn first, then fake"""
    x_real = x_real.detach().requires_grad_(True)
    out = O.discriminator(N["discriminator"], DO.diff_augment(x_real, POLICY), y_org, cfg)
    loss_real = O.adv_loss(out, 1)
    loss_reg = O.r1_reg(out, x_real)
    with torch.no_grad():
        x_fake = O.generator(N["generator"], x_real, O.style_code(N, y_trg, cfg, None, z_trg), cfg)
    loss_fake = O.adv_loss(O.discriminator(N["discriminator"], DO.diff_augment(x_fake, POLICY), y_trg, cfg), 0)
    return loss_real + loss_fake + cfg.lambda_reg * loss_reg, {"real": float(loss_real), "fake": float(loss_fake), "reg": float(loss_reg)}


def _oracle_g_loss(N, x_real, y_org, y_trg, cfg, z_trgs):
    """O.compute_g_loss with DiffAugment on the x_fake the discriminator sees (solver.py:510)"""
    z_trg, z_trg2 = z_trgs
    s_trg = O.style_code(N, y_trg, cfg, None, z_trg)
    x_fake = O.generator(N["generator"], x_real, s_trg, cfg)
    loss_adv = O.adv_loss(O.discriminator(N["discriminator"], DO.diff_augment(x_fake, POLICY), y_trg, cfg), 1)
    loss_sty = torch.mean(torch.abs(O.style_encoder(N["style_encoder"], x_fake, y_trg, cfg) - s_trg))
    x_fake2 = O.generator(N["generator"], x_real, O.style_code(N, y_trg, cfg, None, z_trg2), cfg).detach()
    loss_ds = torch.mean(torch.abs(x_fake - x_fake2))
    x_rec = O.generator(N["generator"], x_fake, O.style_encoder(N["style_encoder"], x_real, y_org, cfg), cfg)
    loss_cyc = torch.mean(torch.abs(x_rec - x_real))
    loss = loss_adv + cfg.lambda_sty * loss_sty - cfg.lambda_ds * loss_ds + cfg.lambda_cyc * loss_cyc
    return loss, {"adv": float(loss_adv), "sty": float(loss_sty), "ds": float(loss_ds), "cyc": float(loss_cyc)}


def test_d_loss_with_diffaugment_and_r1_through_it_matches_the_oracle():
    from de_i2i_gan_amd.stargan import compute_d_loss
    meta, arr, cfg = load()
    args, nets, _ = build(cfg, "f32")
    args.DiffAugment = POLICY
    x_real, y_org, y_trg, _, _, z_trg, _ = O.synthetic_inputs(cfg, meta["batch"])
    torch.manual_seed(123)
    loss, ls = compute_d_loss(nets, args, x_real.to(DEV), y_org.to(DEV), y_trg.to(DEV), z_trg=z_trg.to(DEV))
    loss.backward()
    _, N = states(cfg)
    O.require_grad(N["discriminator"], True)
    torch.manual_seed(123)
    o_loss, o_ls = _oracle_d_loss(N, x_real, y_org, y_trg, cfg, z_trg)
    o_grads = O.grads_of(o_loss, N["discriminator"])
    for k in ("real", "fake", "reg"):
        assert abs(getattr(ls, k) - o_ls[k]) < 1e-4 * abs(o_ls[k]), (k, getattr(ls, k), o_ls[k])
    worst = {k: rel_l2(p.grad, o_grads[k]) for k, p in nets.discriminator.state_dict(keep_vars=True).items()}
    assert max(worst.values()) < 2e-3, worst


def test_g_loss_with_diffaugment_matches_the_oracle():
    """lambda_ds = lambda_cyc = 0 for the gradients: the reasons of test_starganv2_gpu's generator test (one generator pass on the
    gradient path, the diversity term is fp32 noise on this fill); the four loss values are compared all the same"""
    from de_i2i_gan_amd.stargan import compute_g_loss
    meta, arr, cfg = load()
    cfg.lambda_ds, cfg.lambda_cyc = 0.0, 0.0
    args, nets, _ = build(cfg, "f32")
    args.DiffAugment = POLICY
    x_real, y_org, y_trg, _, _, z_trg, z_trg2 = O.synthetic_inputs(cfg, meta["batch"])
    torch.manual_seed(321)
    loss, ls = compute_g_loss(nets, args, x_real.to(DEV), y_org.to(DEV), y_trg.to(DEV), z_trgs=[z_trg.to(DEV), z_trg2.to(DEV)])
    loss.backward()
    _, N = states(cfg)
    for S in N.values():
        O.require_grad(S, True)
    torch.manual_seed(321)
    o_loss, o_ls = _oracle_g_loss(N, x_real, y_org, y_trg, cfg, (z_trg, z_trg2))
    for k in ("adv", "sty", "cyc"):
        assert abs(getattr(ls, k) - o_ls[k]) < 1e-4 * max(abs(o_ls[k]), 1e-2), (k, getattr(ls, k), o_ls[k])
    assert abs(ls.ds - o_ls["ds"]) < 1e-5
    bad = {}
    for name in ("generator", "mapping_network", "style_encoder"):
        og = O.grads_of(o_loss, N[name])
        scale = max(float(v.norm()) for v in og.values() if v is not None)
        for k, ref in og.items():
            p = getattr(nets, name).state_dict(keep_vars=True)[k]
            if ref is None or float(ref.norm()) < 1e-3 * scale:
                continue
            if rel_l2(p.grad, ref) > 2e-2:
                bad[name + "." + k] = rel_l2(p.grad, ref)
    assert not bad, bad


def test_lambda_ds_decays_linearly_to_zero_over_ds_iter():
    from de_i2i_gan_amd.stargan import Solver
    meta, arr, cfg = load()
    args, nets, nets_ema = build(cfg, "f32")
    args.DiffAugment, args.ds_iter, args.lambda_ds = POLICY, 4, 1.0
    solver = Solver(args, nets, nets_ema, DEV)
    inputs = [t.to(DEV) for t in O.synthetic_inputs(cfg, meta["batch"])]
    torch.manual_seed(0)
    seen = []
    for _ in range(5):
        out = solver.train_iteration(*inputs)
        assert all(torch.isfinite(torch.tensor(list(vars(v).values()))).all() for v in out.values()), out
        seen.append(args.lambda_ds)
    assert seen == [0.75, 0.5, 0.25, 0.0, 0.0]


def test_fused_ema_matches_lerp_and_invalidates_the_packed_weights():
    from de_i2i_gan_amd.stargan import build_model, moving_average
    meta, arr, cfg = load()
    args, nets, nets_ema = build(cfg, "f32")
    G, G_ema = nets.generator, nets_ema.generator
    with torch.no_grad():
        for p in G.parameters():
            p.add_(0.1 * torch.randn_like(p))
    x_real, _, y_trg, _, _, z_trg, _ = [t.to(DEV) for t in O.synthetic_inputs(cfg, meta["batch"])]
    with torch.no_grad():
        s = nets_ema.mapping_network(z_trg, y_trg)
        G_ema(x_real, s)                                     # packs the EMA generator's conv weights
        expect = [torch.lerp(p, e, 0.999) for p, e in zip(G.parameters(), G_ema.parameters())]
        moving_average(G, G_ema, beta=0.999)
        for e, ref in zip(G_ema.parameters(), expect):
            assert float((e - ref).abs().max()) <= 1e-6 * max(float(ref.abs().max()), 1e-30)
        got = G_ema(x_real, s)
        fresh, _ = build_model(copy.copy(args))
        fresh.generator.to(DEV).load_state_dict(G_ema.state_dict())
        assert torch.equal(got, fresh.generator(x_real, s))


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_coupled_weight_decay_adam_matches_torch_and_leaves_grads(grad_scale):
    from de_i2i_gan_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(4)
    shapes = [(64,), (3, 5, 7), (1001,), (16, 8, 3, 3)]
    ps = [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in shapes]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    wd, lr = 1e-2, 1e-3
    mine = FusedAdam(ps, lr=lr, betas=(0.5, 0.99), weight_decay=wd, decoupled=False, grad_scale=grad_scale)
    ref = torch.optim.Adam(qs, lr=lr, betas=(0.5, 0.99), weight_decay=wd)
    for it in range(3):
        grads = [torch.randn(s, generator=g).to(DEV) for s in shapes]
        for p, q, gr in zip(ps, qs, grads):
            p.grad = gr.clone()
            q.grad = gr * grad_scale
        mine.step()
        ref.step()
        for p, gr in zip(ps, grads):
            assert torch.equal(p.grad, gr)                   # the caller's gradient is not written
        for p, q in zip(ps, qs):
            assert float((p - q).abs().max()) < 1e-6, (it, float((p - q).abs().max()))
