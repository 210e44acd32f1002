"""CPU: the store hook of oracle/starganv2_oracle.py and every condition the stargan-v2 bf16 GPU tests rely on (tests/test_stargan_blocks_gpu.py,
tests/test_stargan_nets_bf16_gpu.py), on the references alone:

  * an identity hook leaves every hooked function bit for bit what the un-hooked call returns (values and gradients);
  * the rounding hook (tests/stargan_emulation.py) is the identity on bf16-valued tensors, rounds the gradient that arrives at a store,
    leaves a conv weight's gradient alone, takes LeakyReLU'(0) = 1 as the kernels do, and can be differentiated twice (the R1 penalty);
  * every block case: the emulation differs from float64 (the hook is in the graph), the share of LeakyReLU pre-activations in the kink
    band is below 0.1 %, no bias or affine parameter is zero, and -- AdaIN blocks -- swapping the two style rows moves the reference
    by far more than the bf16 bound;
  * the network problem: y_org != y_trg for both samples, images in [-1, 1], and the two style codes of the diversity term differ by
    more than 1e-2 relative on both branches (its gradient sign(x_fake - x_fake2) / numel is then well defined)."""
import pytest
import torch

import stargan_emulation as E
from oracle import starganv2_oracle as O

identity = lambda t: t          # an explicit hook: not the module's own default object


def _same_tree(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same_tree(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_tree(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return a == b


@pytest.mark.parametrize("name", E.BLOCK_IDS[:8])
def test_identity_hook_leaves_the_blocks_bit_for_bit(name):
    P = E.block_problem(name)
    _, kind, normalize, resample, _, _, _ = P["case"]

    def run(*hook):
        S = {k: v.clone().requires_grad_(True) for k, v in P["S"].items()}
        x = P["x"].clone().requires_grad_(True)
        if kind == "res":
            out, leaves = O.resblk(S, "", x, normalize, resample, *hook), [x] + list(S.values())
        else:
            s = P["s"].clone().requires_grad_(True)
            out, leaves = O.adain_resblk(S, "", x, s, resample, *hook), [x, s] + list(S.values())
        return [out.detach()] + list(torch.autograd.grad(out, leaves, P["gy"]))
    assert _same_tree(run(), run(identity))


def test_identity_hook_leaves_the_networks_and_loss_graphs_bit_for_bit():
    P = E.net_problem()
    cfg = P["cfg"]

    def states():
        return {n: {k: v.clone().requires_grad_(True) for k, v in S.items()} for n, S in P["N"].items()}

    def nets(*hook):
        N = states()
        with torch.no_grad():
            s = O.mapping_network(N["mapping_network"], P["z_trg"], P["y_trg"], cfg)
            return [O.generator(N["generator"], P["x_real"], s, cfg, *hook), O._trunk(N["style_encoder"], "shared.", P["x_ref"], cfg, *hook),
                    O.style_encoder(N["style_encoder"], P["x_ref"], P["y_trg"], cfg, *hook),
                    O.discriminator(N["discriminator"], P["x_real"], P["y_org"], cfg, *hook)]

    def d_loss(**hook):
        N = states()
        loss, terms = O.compute_d_loss(N, P["x_real"], P["y_org"], P["y_trg"], cfg, z_trg=P["z_trg"], **hook)
        return loss.detach(), terms, O.grads_of(loss, N["discriminator"])

    def g_loss(**hook):
        N = states()
        loss, terms = O.compute_g_loss(N, P["x_real"], P["y_org"], P["y_trg"], cfg, x_refs=(P["x_ref"], P["x_ref2"]), **hook)
        return loss.detach(), terms, [O.grads_of(loss, N[n]) for n in ("generator", "style_encoder")]
    assert _same_tree(nets(), nets(identity))
    assert _same_tree(d_loss(), d_loss(store=identity))
    assert _same_tree(g_loss(), g_loss(store=identity))


def test_rounding_hook_is_the_identity_on_bf16_values_and_rounds_the_gradient():
    gen = torch.Generator().manual_seed(1)
    st = E.BF16_STORE
    t = E.bf16_valued((64, 33), gen).double()
    assert torch.equal(st(t), t) and torch.equal(st.weight(t), t)
    raw = torch.randn(64, 33, generator=gen, dtype=torch.float64)
    assert not torch.equal(st(raw), raw) and torch.equal(st(raw), raw.to(torch.bfloat16).double())
    assert torch.equal(st(st(raw)), st(raw))
    x = raw.clone().requires_grad_(True)
    g = torch.randn(64, 33, generator=gen, dtype=torch.float64)
    (gx,) = torch.autograd.grad(st(x), x, g)
    assert torch.equal(gx, g.to(torch.bfloat16).double())                       # straight through, rounded the same way
    (gw,) = torch.autograd.grad(st.weight(x), x, g)
    assert torch.equal(gw, g)                                                   # a weight gradient is written in fp32: untouched
    # LeakyReLU: torch's values, the kernels' derivative 1 at an exact 0 (csrc/common.h act_grad_from_out), differentiable again
    z = torch.tensor([-1.5, -0.0, 0.0, 2.0], dtype=torch.float64, requires_grad=True)
    assert torch.equal(st.lrelu(z), O.lrelu(z))
    assert torch.autograd.grad(st.lrelu(z).sum(), z)[0].tolist() == [0.2, 1.0, 1.0, 1.0]
    assert torch.autograd.grad(O.lrelu(z).sum(), z)[0].tolist() == [0.2, 0.2, 0.2, 1.0]
    # twice differentiable: d/dw of |d sum(st(st(w x) ^ 2)) / dx|^2 exists and is finite
    w = torch.tensor(0.75, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(st(st(w * x) ** 2).sum(), x, create_graph=True)
    (gww,) = torch.autograd.grad(gx.pow(2).sum(), w)
    assert torch.isfinite(gww) and float(gww) != 0.0


@pytest.mark.parametrize("name", E.BLOCK_IDS)
def test_block_cases_meet_the_conditions_of_the_gpu_tests(name):
    P = E.block_problem(name)
    _, kind, _, _, _, _, _ = P["case"]
    share = E.kink_share(P["pres"])
    print(f"{name}: seed {P['seed']}, kink share {share:.2e}")
    assert len(P["pres"]) == 2 and share < E.KINK_SHARE
    assert all(float(v.abs().min()) > 0.0 for k, v in P["S"].items() if v.dim() == 1), "a zero bias / affine parameter would hide its term"
    assert torch.equal(P["x"], P["x"].to(torch.bfloat16).float()) and torch.equal(P["gy"], P["gy"].to(torch.bfloat16).float())
    d_out = E.rel_l2(P["emul"]["out"], P["ref"]["out"])
    assert 1e-3 < d_out < 2e-2, d_out             # the hook rounds (2^-9 per store, a handful of stores) and does nothing worse
    if kind == "adain":
        assert float((P["s"][0] - P["s"][1]).norm() / P["s"].norm()) > 0.5
        swapped = E.block_oracle(P, O._same, s=P["s"].flip(0))
        moved = E.rel_l2(swapped["out"], P["ref"]["out"])
        print(f"{name}: style rows swapped moves the reference by {moved:.2e}; bf16 bound {E.bf16_bound(d_out):.2e}")
        assert moved > 10 * E.bf16_bound(d_out), (moved, d_out)


def test_network_problem_meets_the_conditions_of_the_gpu_tests():
    P = E.net_problem()
    assert bool((P["y_org"] != P["y_trg"]).all())
    for k in ("x_real", "x_ref", "x_ref2"):
        assert float(P[k].min()) >= -1.0 and float(P[k].max()) <= 1.0 and float(P[k].std()) > 0.5
    assert all(float(v.abs().min()) > 0.0 for S in P["N"].values() for v in S.values() if v.dim() == 1)
    for graph in ("g_latent", "g_ref"):
        s1, s2 = E.style_codes(graph)
        dist = float((s1 - s2).norm() / s1.norm())
        print(f"{graph}: the diversity term's style codes differ by {dist:.2e} relative")
        assert dist > 1e-2, (graph, dist)
