"""GPU: ResBlk and AdainResBlk of de_i2i_gan_amd/stargan/model.py, one block at a time, against oracle/starganv2_oracle.py's resblk /
adain_resblk in float64 -- the forward output, the input gradient, the style gradient and every parameter gradient under a random
upstream gradient, in both precisions, on every structural branch of the two classes (tests/stargan_emulation.py::BLOCKS: the case
table, the data, the seed choice and the references; tests/test_starganv2_store_emulation.py asserts their conditions on the CPU).

  * f32 mode: forward 1e-3 of the tensor's max, gradients 2e-3 relative L2 per tensor (tests/test_starganv2_gpu.py's bounds);
  * bf16 mode: per tensor d_prod <= 3 * d_emul + 1e-3, d_emul the float64 oracle with the round-to-bf16 store hook against the float64
    oracle without it (stargan_emulation's docstring).  No element is excluded: the seed keeps the LeakyReLU kink band below 0.1 %.
  * a gradient that is structurally zero (a conv bias in front of an instance norm: the norm removes the shift; the reference holds
    1e-17-scale noise there) is judged by its size against the block's largest parameter gradient: below 2e-3 of it in f32 mode (the
    existing rule of test_generator_loss_and_gradients_match_the_oracle), below 3 x the emulation's + 1e-3 of it in bf16 mode.

Measured (emulation / product, worst tensor of each case) is printed by every bf16 case and recorded in DESIGN.md section 3d."""
import pytest
import torch

import stargan_emulation as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run_product(P, pname):
    from de_i2i_gan_amd import ops
    from de_i2i_gan_amd.stargan.model import AdainResBlk, ResBlk
    _, kind, normalize, resample, din, dout, _ = P["case"]
    prec = ops.get_precision(pname)
    if kind == "res":
        blk = ResBlk(din, dout, normalize=normalize, downsample=resample)
    else:
        blk = AdainResBlk(din, dout, style_dim=E.STYLE_DIM, w_hpf=0, upsample=resample)
    blk.load_state_dict(P["S"])
    blk.to(DEV)
    x = P["x"].to(DEV).requires_grad_(True)
    h = ops.to_nhwc(x, prec)
    if kind == "res":
        y, s = blk(h), None
    else:
        s = P["s"].to(DEV).requires_grad_(True)
        y = blk(h, s)
    out = ops.to_nchw(y, dout)
    out.backward(P["gy"].to(DEV))
    torch.cuda.synchronize()
    got = {"out": out.detach(), "dx": x.grad}
    got.update({k: p.grad for k, p in blk.state_dict(keep_vars=True).items()})
    if s is not None:
        got["ds"] = s.grad
    return got


def _split(P):
    """-> (compared tensors, structurally zero ones, the scale those are judged by)"""
    ref = P["ref"]
    scale = max(float(ref[k].norm()) for k in P["S"])
    live = [k for k in ref if k in ("out", "dx", "ds") or float(ref[k].norm()) > 1e-3 * scale]
    return live, [k for k in ref if k not in live], scale


@pytest.mark.parametrize("name", E.BLOCK_IDS)
def test_block_f32_matches_float64(name):
    P = E.block_problem(name)
    got = _run_product(P, "f32")
    ref = P["ref"]
    assert set(got) == set(ref)
    live, dead, scale = _split(P)
    assert got["out"].shape == ref["out"].shape
    assert E.maxrel(got["out"], ref["out"]) < E.F32_FWD, E.maxrel(got["out"], ref["out"])
    worst = {k: E.rel_l2(got[k], ref[k]) for k in live if k != "out"}
    print(f"{name} f32: out {E.maxrel(got['out'], ref['out']):.2e} of max; worst gradient {max(worst.values()):.2e}")
    assert max(worst.values()) < E.F32_GRAD, worst
    for k in dead:
        assert float(got[k].norm()) < 2e-3 * scale, k


@pytest.mark.parametrize("name", E.BLOCK_IDS)
def test_block_bf16_within_three_times_the_store_emulation(name):
    P = E.block_problem(name)
    got = _run_product(P, "bf16")
    ref, emu = P["ref"], P["emul"]
    assert set(got) == set(ref)
    live, dead, scale = _split(P)
    bad = {}
    for k in live:
        d_emul, d_prod = E.rel_l2(emu[k], ref[k]), E.rel_l2(got[k], ref[k])
        print(f"{name} bf16 {k}: d_emul {d_emul:.2e} d_prod {d_prod:.2e}")
        if not d_prod <= E.bf16_bound(d_emul):
            bad[k] = (d_emul, d_prod)
    for k in dead:
        n_emul, n_prod = float(emu[k].norm()) / scale, float(got[k].norm()) / scale
        print(f"{name} bf16 {k} (structurally zero, of the largest gradient): emul {n_emul:.2e} prod {n_prod:.2e}")
        if not n_prod <= E.bf16_bound(n_emul):
            bad[k] = (n_emul, n_prod)
    assert not bad, bad
