"""CPU: the stargan-v2 oracle (oracle/starganv2_oracle.py) against the fixture captured from the reference's own core.model /
core.solver (tests/golden/gen_starganv2_golden.py): forward passes of the four networks, the four loss graphs of one training
iteration (incl. the R1 penalty: a double backward through the discriminator), gradient norms, post-Adam parameter norms, EMA."""
import json
from pathlib import Path

import numpy as np
import torch

from oracle import starganv2_oracle as O

GOLD = Path(__file__).resolve().parent / "golden"
NAME = "sg0_img64_b2"


def load():
    meta = json.loads((GOLD / f"{NAME}.json").read_text())
    arr = np.load(GOLD / f"{NAME}.npz")
    cfg = O.Cfg(**meta["config"])
    return meta, arr, cfg


def states(cfg):
    shapes = {"generator": O.generator_state_shapes(cfg), "mapping_network": O.mapping_state_shapes(cfg),
              "style_encoder": O.style_encoder_state_shapes(cfg), "discriminator": O.discriminator_state_shapes(cfg)}
    return shapes, {n: O.make_state(s, n + ".") for n, s in shapes.items()}


def test_state_manifest_is_the_references():
    meta, arr, cfg = load()
    shapes, _ = states(cfg)
    for n in shapes:
        assert list(shapes[n]) == meta["keys"][n], n


def test_one_training_iteration_matches_the_reference_fixture():
    meta, arr, cfg = load()
    torch.set_num_threads(8)
    shapes, N = states(cfg)
    N_ema = {n: {k: v.clone() for k, v in N[n].items()} for n in ("generator", "mapping_network", "style_encoder")}
    inputs = O.synthetic_inputs(cfg, meta["batch"])
    x_real, y_org, y_trg, x_ref, x_ref2, z_trg, z_trg2 = inputs
    with torch.no_grad():
        s_map = O.mapping_network(N["mapping_network"], z_trg, y_trg, cfg)
        assert np.abs(s_map.numpy() - arr["s_map"]).max() < 1e-5
        assert np.abs(O.style_encoder(N["style_encoder"], x_ref, y_trg, cfg).numpy() - arr["s_enc"]).max() < 1e-5
        # the generator's fp32 output moves by up to 2.5e-4 with the host's CPU kernels (oneDNN / ATen ISA, thread count): the
        # fixture, itself an fp32 run, sits 9.2e-5 from the exact result -- so compare the oracle evaluated in float64
        G64 = {k: v.double() for k, v in N["generator"].items()}
        assert np.abs(O.generator(G64, x_real.double(), s_map.double(), cfg).numpy() - arr["x_fake"]).max() < 1.2e-4
        assert np.abs(O.discriminator(N["discriminator"], x_real, y_org, cfg).numpy() - arr["d_out"]).max() < 1e-6
    opt = {n: O.AdamState() for n in N}
    losses, grads = O.train_iteration(N, N_ema, opt, inputs, cfg)
    # Two kinds of numbers below.  Everything up to the generator update is well conditioned and pinned tightly.  The diversity
    # loss ds = mean|G(x, s1) - G(x, s2)| is not: at init the two styles barely move the image, so ds is fp32 rounding noise
    # (exact value 2.4e-7, fixture 1.5e-6), its gradient is the sign of that noise, and Adam turns it into full lr-sized steps of
    # the generator.  The generator's new weights and every g_ref loss computed with them therefore depend on the host's CPU
    # kernels (oneDNN / ATen ISA, thread count): over float64 and 12 fp32 kernel / thread variants of this oracle they spread
    # g_ref adv 4.4e-3, cyc 0.11 relative, sty 0.029, ds 5.6e-5 absolute, the generator's per-tensor norms 6e-3 relative
    # (its total norm 6.4e-6, the median tensor 1.3e-5).  Those are bounded at about 3x that spread.
    order = {"d_latent": ("real", "fake", "reg"), "d_ref": ("real", "fake", "reg"), "g_latent": ("adv", "sty", "ds", "cyc")}
    for tag, keys in order.items():
        got, ref = np.array([losses[tag][k] for k in keys]), arr["losses_" + tag]
        rel = (np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6))[[k != "ds" for k in keys]]
        assert np.max(rel) < (1e-5 if tag == "d_latent" else 5e-3), (tag, got, ref)
    assert abs(losses["g_latent"]["ds"] - arr["losses_g_latent"][2]) < 5e-6, (losses["g_latent"], arr["losses_g_latent"])
    got, ref = np.array([losses["g_ref"][k] for k in ("adv", "sty", "ds", "cyc")]), arr["losses_g_ref"]
    assert abs(got[0] - ref[0]) < 1.5e-2 * ref[0] and abs(got[3] - ref[3]) < 0.3 * ref[3], (got, ref)
    assert abs(got[1] - ref[1]) < 0.1 and abs(got[2] - ref[2]) < 2e-4, (got, ref)
    g0 = grads["d_latent"]["main.0.weight"].numpy()                 # carries the R1 term (lambda_reg 2e5 in the fixture)
    assert np.abs(g0 - arr["d_latent_grad::main.0.weight"]).max() < 1e-4 * np.abs(arr["d_latent_grad::main.0.weight"]).max()
    for n in N:
        mine = np.array([float(N[n][k].detach().double().norm()) for k in shapes[n]])
        ref = arr["post_norm_" + n]
        rel = np.abs(mine - ref) / np.maximum(ref, 1e-9)
        if n == "generator":
            total = abs(np.linalg.norm(mine) - np.linalg.norm(ref)) / np.linalg.norm(ref)
            assert rel.max() < 2e-2 and np.median(rel) < 1e-4 and total < 1e-4, (n, rel.max(), np.median(rel), total)
        else:
            assert rel.max() < 1e-4, n
    for n in N_ema:
        mine = np.array([float(N_ema[n][k].double().norm()) for k in shapes[n]])
        # (the generator's EMA takes 1e-3 of its noise-driven update)
        assert np.max(np.abs(mine - arr["ema_norm_" + n]) / np.maximum(arr["ema_norm_" + n], 1e-9)) < (3e-5 if n == "generator" else 1e-5), n
