"""GPU: the four stargan-v2 networks and both loss graphs at the reference's initialisation, against oracle/starganv2_oracle.py in
float64 (tests/stargan_emulation.py::net_problem: O.Cfg() -- img 64 -- batch 2, He init + N(0, 0.1) biases and affine parameters, images
uniform in [-1, 1], z ~ N(0, 1), y_org != y_trg for both samples, so the per-domain heads matter).

  * forwards of mapping_network, style_encoder, generator, discriminator: f32 mode 1e-3 of the tensor's max; bf16 mode
    d_prod <= 3 * d_emul + 1e-3 (relative L2; d_emul: the float64 oracle under the round-to-bf16 store hook);
  * compute_d_loss (latent branch: the R1 penalty's double backward included) and compute_g_loss (latent and reference branches) in
    bf16 with lambda_ds = lambda_cyc = 1 -- the diversity term is IN the gradient: with real style codes (they differ by 0.66 / 0.20
    relative, asserted on the CPU) sign(x_fake - x_fake2) is well defined.  Per loss term |prod - ref| / |ref| <= 3 x the emulation's
    + 1e-3.  Per network, on the full gradient: 1 - cos_prod <= 3 * (1 - cos_emul) + 1e-4, and | |g_prod| / |g_ref| - 1 | <= 3 * d_emul
    + 1e-3 with d_emul the emulated full gradient's relative L2 (| |a| / |b| - 1 | <= |a - b| / |b| for any a: the relative L2 bounds the
    ratio, whereas the emulation's own ratio is a signed number that can pass through 1 by chance).  Per tensor whose reference norm is
    above 1e-3 of the network's largest: relative L2 by the same rule; the others (a conv bias in front of an instance norm) by their
    norm against that largest one.

Every bf16 comparison prints d_emul and d_prod; the measured values are in DESIGN.md section 3d."""
from types import SimpleNamespace

import pytest
import torch

import stargan_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _build(pname):
    from de_i2i_gan_amd.stargan import build_model
    P = E.net_problem()
    cfg = P["cfg"]
    args = SimpleNamespace(img_size=cfg.img_size, style_dim=cfg.style_dim, latent_dim=cfg.latent_dim, num_domains=cfg.num_domains,
                           max_conv_dim=cfg.max_conv_dim, w_hpf=0, norm_type="adain", num_embeds=1, lambda_reg=cfg.lambda_reg,
                           lambda_sty=cfg.lambda_sty, lambda_ds=cfg.lambda_ds, lambda_cyc=cfg.lambda_cyc, compute_dtype=pname)
    nets, _ = build_model(args)
    for name, net in vars(nets).items():
        net.load_state_dict(P["N"][name])
        net.to(DEV)
    return P, args, nets


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("pname", ["f32", "bf16"])
def test_network_forwards_at_the_reference_init(pname):
    P, _, nets = _build(pname)
    d = lambda k: P[k].to(DEV)
    with torch.no_grad():
        s_map = nets.mapping_network(d("z_trg"), d("y_trg"))
        got = {"s_map": s_map, "s_enc": nets.style_encoder(d("x_ref"), d("y_trg")), "x_fake": nets.generator(d("x_real"), s_map),
               "d_out": nets.discriminator(d("x_real"), d("y_org"))}
    torch.cuda.synchronize()
    ref, emu = E.forwards("ref"), E.forwards("emul")
    bad = {}
    for k in ref:
        assert got[k].shape == ref[k].shape, k
        if pname == "f32":
            err = E.maxrel(got[k], ref[k])
            print(f"forward f32 {k}: {err:.2e} of max")
            if not err < E.F32_FWD:
                bad[k] = err
        else:
            d_emul, d_prod = E.rel_l2(emu[k], ref[k]), E.rel_l2(got[k], ref[k])
            print(f"forward bf16 {k}: d_emul {d_emul:.2e} d_prod {d_prod:.2e}")
            if not d_prod <= E.bf16_bound(d_emul):
                bad[k] = (d_emul, d_prod)
    assert not bad, bad


@pytest.mark.parametrize("graph", list(E.GRAPHS))
def test_loss_graph_bf16_within_three_times_the_store_emulation(graph):
    from de_i2i_gan_amd.stargan import compute_d_loss, compute_g_loss
    P, args, nets = _build("bf16")
    d = lambda k: P[k].to(DEV)
    if graph == "d_latent":
        loss, terms = compute_d_loss(nets, args, d("x_real"), d("y_org"), d("y_trg"), z_trg=d("z_trg"))
    elif graph == "g_latent":
        loss, terms = compute_g_loss(nets, args, d("x_real"), d("y_org"), d("y_trg"), z_trgs=[d("z_trg"), d("z_trg2")])
    else:
        loss, terms = compute_g_loss(nets, args, d("x_real"), d("y_org"), d("y_trg"), x_refs=[d("x_ref"), d("x_ref2")])
    loss.backward()
    torch.cuda.synchronize()
    torch.set_num_threads(16)
    (t_ref, g_ref), (t_emu, g_emu) = E.loss_graph(graph, "ref"), E.loss_graph(graph, "emul")
    bad = {}
    for k, v in t_ref.items():
        d_emul, d_prod = _rel(t_emu[k], v), _rel(getattr(terms, k), v)
        print(f"{graph} loss {k}: ref {v:.6f} d_emul {d_emul:.2e} d_prod {d_prod:.2e}")
        if not d_prod <= E.bf16_bound(d_emul):
            bad["loss " + k] = (d_emul, d_prod)
    for net in E.GRAPHS[graph]:
        ref, emu = g_ref[net], g_emu[net]
        params = getattr(nets, net).state_dict(keep_vars=True)
        assert set(ref) == set(params), net              # every parameter of the network is in this graph
        got = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().cpu() for k, p in params.items()}
        keys = list(ref)
        a_ref, a_emu, a_got = E.flat(ref, keys), E.flat(emu, keys), E.flat(got, keys)
        c_emul, c_prod = E.cosine(a_emu, a_ref), E.cosine(a_got, a_ref)
        d_emul, d_prod = E.rel_l2(a_emu, a_ref), E.rel_l2(a_got, a_ref)
        r_emul, r_prod = float(a_emu.norm() / a_ref.norm()), float(a_got.norm() / a_ref.norm())
        print(f"{graph} {net} full gradient: 1-cos emul {1 - c_emul:.2e} prod {1 - c_prod:.2e}; rel L2 emul {d_emul:.2e} prod {d_prod:.2e}; "
              f"norm ratio emul {r_emul:.4f} prod {r_prod:.4f}")
        if not 1 - c_prod <= E.FACTOR * (1 - c_emul) + E.COS_FLOOR:
            bad[net + " cosine"] = (1 - c_emul, 1 - c_prod)
        if not abs(r_prod - 1) <= E.bf16_bound(d_emul):
            bad[net + " norm ratio"] = (d_emul, r_prod)
        scale = max(float(v.norm()) for v in ref.values())
        worst = (0.0, 0.0, None)
        for k in keys:
            if float(ref[k].norm()) > 1e-3 * scale:
                t_emul, t_prod = E.rel_l2(emu[k], ref[k]), E.rel_l2(got[k], ref[k])
            else:                                        # structurally zero: its size against the largest tensor's
                t_emul, t_prod = float(emu[k].norm()) / scale, float(got[k].norm()) / scale
            print(f"{graph} {net}.{k}: d_emul {t_emul:.2e} d_prod {t_prod:.2e}")
            if t_prod > worst[1]:
                worst = (t_emul, t_prod, k)
            if not t_prod <= E.bf16_bound(t_emul):
                bad[net + "." + k] = (t_emul, t_prod)
        print(f"{graph} {net} worst tensor {worst[2]}: d_emul {worst[0]:.2e} d_prod {worst[1]:.2e}")
    assert not bad, bad
