"""Device-drawn DiffAugment parameters (csrc/diffaug.hip dei2i_diffaug_draw, ops.DiffAugRng, opt.diff_aug_rng='device').

Everything here is compared bit for bit; nothing needs a tolerance.  The reference is a numpy Philox4x32-10 and a numpy
``draw_reference`` written from the formulas of include/dei2i_hip.h and utils.diffaug.draw_params: the generator is checked
against the Random123 known answers and for coverage of every integer value on the CPU, the device table against the
reference over policies, batch sizes (257 crosses the 256-thread stride), image sizes (odd ones exercise the 1 - ch % 2 term),
call counts (2^32 + 5 reaches the high counter word) and row offsets; the op against the existing ``_DiffAug`` path fed the table
read back from the device (output, gradient, second-order gradient); the captured step against the eager step after every step."""
import ctypes
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import make_opt

gpu = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5DEECE66D1234567          # (checked below: at 8x8, N = 4096 every translation and cutout value occurs)
from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
POLICIES = ["color", "translation", "cutout", "color,translation,cutout", "translation,color", "color,color"]
CANONICAL = ("color", "translation", "cutout")

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def policy_runs(policy):
    """maximal canonical-order runs of the policy list (utils.diffaug.policy_runs, restated)"""
    runs = []
    for name in policy.split(","):
        if runs and CANONICAL.index(name) > CANONICAL.index(runs[-1][-1]):
            runs[-1].append(name)
        else:
            runs.append([name])
    return runs


def _unit(x):
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _below(x, rng):
    return ((x.astype(np.uint64) * np.uint64(rng)) >> np.uint64(32)).astype(np.int64)


def draw_uniforms(seed, call, run, rows, block):
    key = (seed & 0xFFFFFFFF, seed >> 32)
    return philox4x32_10((call & 0xFFFFFFFF, call >> 32, run | block << 16, rows), key)


def draw_reference(seed, call, policy, n, row0, h, w):
    """the int32 (runs, n, 8) table of struct dei2i_diffaug_rec (a, b, k, beta stored bitwise; ty, tx, top, left)"""
    runs = policy_runs(policy)
    rec = np.zeros((len(runs), n, 8), dtype=np.int32)
    f = rec.view(np.float32)
    rows = np.arange(row0, row0 + n, dtype=np.uint64)
    one, half, two = np.float32(1), np.float32(0.5), np.float32(2)
    for r, names in enumerate(runs):
        f[r, :, 0] = 1.0
        if "color" in names:
            x = draw_uniforms(seed, call, r, rows, 0)
            rb, rs, rc = _unit(x[0]), _unit(x[1]), _unit(x[2])
            ks, kc = two * rs, rc + half
            f[r, :, 0] = kc * ks
            f[r, :, 1] = kc * (one - ks)
            f[r, :, 2] = one - kc
            f[r, :, 3] = rb - half
        if "translation" in names or "cutout" in names:
            x = draw_uniforms(seed, call, r, rows, 1)
        if "translation" in names:
            max_y, max_x = int(h * 0.125 + 0.5), int(w * 0.125 + 0.5)
            rec[r, :, 4] = -max_y + _below(x[0], 2 * max_y + 1)
            rec[r, :, 5] = -max_x + _below(x[1], 2 * max_x + 1)
        if "cutout" in names:
            ch, cw = int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)
            rec[r, :, 6] = _below(x[2], h + (1 - ch % 2)) - ch // 2
            rec[r, :, 7] = _below(x[3], w + (1 - cw % 2)) - cw // 2
    return rec


# ---- 1. the reference itself (CPU) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
], ids=["zeros", "ones", "pi"])
def test_reference_philox_reproduces_the_random123_known_answers(ctr, key, want):
    assert tuple(int(v) for v in philox4x32_10(ctr, key)) == want


def test_reference_draws_cover_every_value():
    rec = draw_reference(SEED, 0, "color,translation,cutout", 4096, 0, 8, 8)[0]
    assert set(rec[:, 4].tolist()) == {-1, 0, 1} and set(rec[:, 5].tolist()) == {-1, 0, 1}
    assert set((rec[:, 6] + 2).tolist()) == set(range(9)) and set((rec[:, 7] + 2).tolist()) == set(range(9))      # cy = top + ch // 2
    rows = np.arange(4096, dtype=np.uint64)
    for u in draw_uniforms(SEED, 0, 0, rows, 0)[:3]:
        v = _unit(u)
        assert v.dtype == np.float32 and (v >= 0).all() and (v < 1).all()
    assert policy_runs("translation,color") == [["translation"], ["color"]] and policy_runs("color,color") == [["color"], ["color"]]
    assert policy_runs("color,translation,cutout") == [["color", "translation", "cutout"]]


def test_options_io_round_trips_the_new_attributes(tmp_path):
    from de_i2i_gan_amd.utils import options_io
    opt = SimpleNamespace(ckpt_dir=tmp_path, name="run", diff_aug="color,cutout", diff_aug_rng="device", diff_aug_seed=2 ** 62 + 3)
    options_io.save_options(opt)
    fresh = SimpleNamespace(ckpt_dir=tmp_path, name="run", continue_training=True, diff_aug="", diff_aug_rng=None, diff_aug_seed=None)
    options_io.update_options_from_file(fresh)
    assert (fresh.diff_aug, fresh.diff_aug_rng, fresh.diff_aug_seed) == ("color,cutout", "device", 2 ** 62 + 3)
    assert "diff_aug_rng: device" in (tmp_path / "run" / "opt.txt").read_text()
    assert pickle.loads((tmp_path / "run" / "opt.pkl").read_bytes()).diff_aug_seed == 2 ** 62 + 3


# ---- 2. the device table ---------------------------------------------------------------------------------------------------
def _table(ops, rng, policy, n, h, w, row0=0):
    tab, runs = ops.diffaug_draw(rng, policy, n, h, w, row0=row0)
    return tab.cpu().numpy(), runs


@gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_table_matches_the_reference_bit_for_bit(policy):
    from de_i2i_gan_amd import ops
    rng = ops.DiffAugRng(SEED, DEV)
    assert rng.state() == (SEED, 0)
    for call in (0, 1, 2 ** 32 + 5):
        for h, w in ((8, 8), (9, 7), (256, 256)):
            for n in (1, 5, 257):
                for row0 in (0, 3):
                    rng.set_state((SEED, call))
                    got, runs = _table(ops, rng, policy, n, h, w, row0)
                    assert rng.state() == (SEED, call + 1), (call, h, w, n, row0)
                    want = draw_reference(SEED, call, policy, n, row0, h, w)
                    assert got.dtype == np.int32 and got.shape == want.shape
                    assert np.array_equal(got, want), (call, h, w, n, row0, np.argwhere(got != want)[:4])
                    cut = [(int(h * 0.5 + 0.5), int(w * 0.5 + 0.5)) if "cutout" in names else (0, 0) for names in policy_runs(policy)]
                    assert runs == [("color" in names, ch, cw) for names, (ch, cw) in zip(policy_runs(policy), cut)]


@gpu
def test_rows_are_a_slice_of_the_whole_batch_and_calls_differ():
    from de_i2i_gan_amd import ops
    policy = "color,translation,cutout"
    rng = ops.DiffAugRng(SEED, DEV)
    rng.set_state((SEED, 7))
    whole, _ = _table(ops, rng, policy, 5, 9, 7)
    nxt, _ = _table(ops, rng, policy, 5, 9, 7)                       # the next call: count 8
    assert rng.state() == (SEED, 9)
    assert not np.array_equal(whole, nxt) and np.array_equal(nxt, draw_reference(SEED, 8, policy, 5, 0, 9, 7))
    rng.set_state((SEED, 7))
    part, _ = _table(ops, rng, policy, 2, 9, 7, row0=3)
    assert np.array_equal(part, whole[:, 3:5])
    other = ops.DiffAugRng(SEED + 1, DEV)
    other.set_state((SEED + 1, 7))
    assert not np.array_equal(_table(ops, other, policy, 5, 9, 7)[0], whole)


@gpu
def test_draw_refuses_bad_arguments():
    from de_i2i_gan_amd import _lib, ops
    rng = ops.DiffAugRng(SEED, DEV)
    tab = torch.zeros(2, 4, 8, dtype=torch.int32, device=DEV)
    lib = ops._lib_for(tab)
    c, t, st = ctypes.c_void_p(rng.counter.data_ptr()), ctypes.c_void_p(tab.data_ptr()), ops._stream()

    def draw(counter=c, runs=1, flags=7, n=4, row0=0, h=8, w=8, table=t):
        return lib.dei2i_diffaug_draw(SEED, counter, runs, flags, n, row0, h, w, table, st)

    assert draw() == 0
    for bad in (dict(counter=None), dict(table=None), dict(runs=0), dict(runs=_lib.DIFFAUG_MAX_RUNS + 1), dict(n=0), dict(row0=-1),
                dict(h=0), dict(w=0), dict(flags=0), dict(flags=7 | 1 << 3), dict(runs=2, flags=7), dict(n=2, row0=2 ** 31 - 1)):
        assert draw(**bad) == BAD_ARG, bad
    assert rng.state() == (SEED, 1)                                 # the refused calls launched nothing
    with pytest.raises(ValueError):
        ops.diffaug_draw(rng, ",".join(["color"] * (_lib.DIFFAUG_MAX_RUNS + 1)), 2, 8, 8)
    with pytest.raises(ValueError):
        ops.DiffAugRng(1, "cpu")


# ---- 3. the op -------------------------------------------------------------------------------------------------------------
def _image(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _first_and_second_order(aug, x, gy, w):
    """the output, the VJP, and d/dx of <w, (dL/dx)^2> through create_graph=True (the nonlinear consumer keeps it non-zero)"""
    x = x.clone().requires_grad_(True)
    y = aug(x)
    loss = (y * gy).sum() + 0.25 * (y * y * gy).sum()
    (gx,) = torch.autograd.grad(loss, x, create_graph=True)
    (ggx,) = torch.autograd.grad((w * gx * gx).sum(), x)
    return y.detach(), gx.detach(), ggx


@gpu
@pytest.mark.parametrize("shape", [(2, 3, 16, 16), (3, 3, 9, 7)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("policy", ["color,translation,cutout", "translation,color", "cutout"])
def test_op_equals_the_table_fed_path_bit_for_bit(policy, shape):
    from de_i2i_gan_amd import ops
    n, _, h, w = shape
    x, gy, wt = (_image(shape, 2) * 2 - 1).to(DEV), (_image(shape, 3) - 0.5).to(DEV), _image(shape, 4).to(DEV)
    rng = ops.DiffAugRng(SEED, DEV)
    rng.set_state((SEED, 11))
    tab, runs = ops.diffaug_draw(rng, policy, n, h, w)
    assert np.array_equal(tab.cpu().numpy(), draw_reference(SEED, 11, policy, n, 0, h, w))

    def table_fed(t):
        for i, run in enumerate(runs):
            t = ops._DiffAug.apply(t, tab[i], run, 0, None)
        return t

    want = _first_and_second_order(table_fed, x, gy, wt)
    rng.set_state((SEED, 11))
    host_state = torch.get_rng_state()
    got = _first_and_second_order(lambda t: ops.diff_augment(t, policy, rng=rng), x, gy, wt)
    assert torch.equal(torch.get_rng_state(), host_state)
    assert rng.state() == (SEED, 12)
    for name, a, b in zip(("output", "gradient", "second-order gradient"), got, want):
        assert torch.equal(a, b), name
    assert not torch.equal(got[0], x) and got[2].abs().max().item() > 0


@gpu
def test_sharded_rows_equal_the_rows_of_the_unsharded_call():
    from de_i2i_gan_amd import ops
    policy = "color,translation,cutout"
    x = (_image((4, 3, 16, 16), 5) * 2 - 1).to(DEV)
    rng = ops.DiffAugRng(SEED, DEV)
    rng.set_state((SEED, 3))
    whole = ops.diff_augment(x, policy, rng=rng)
    rng.set_state((SEED, 3))
    with ops.diffaug_sharded(1, 2):
        part = ops.diff_augment(x[2:4].contiguous(), policy, rng=rng)
    assert torch.equal(part, whole[2:4])
    rng.set_state((SEED, 3))
    with ops.diffaug_sharded(0, 2):
        assert not torch.equal(ops.diff_augment(x[2:4].contiguous(), policy, rng=rng), whole[2:4])


# ---- 4. the trainer: graph against eager -----------------------------------------------------------------------------------
def _graph_against_eager(**over):
    from test_graph_step_gpu import SMALL, compare
    seen, trainers = [], []

    def watch(tr):
        if not any(t is tr for t in trainers):
            trainers.append(tr)
        seen.append((tr.model.diffaug_rng.state(), tr.iters, torch.get_rng_state()))

    tr = compare(SMALL, steps=8, hooks={i: watch for i in range(8)}, diff_aug="color,translation,cutout", diff_aug_rng="device",
                 diff_aug_seed=1234, **over)
    assert len(trainers) == 2 and trainers[1] is tr and len(seen) == 16
    for (state, iters, _), i in zip(seen, list(range(8)) * 2):      # four D-step calls and two G-step calls per step
        assert state == (1234, 6 * i) and iters == i
    assert [t.model.diffaug_rng.state() for t in trainers] == [(1234, 48), (1234, 48)]
    return seen


@gpu
def test_graph_step_equals_eager_with_device_drawn_diff_aug():
    seen = _graph_against_eager()
    assert all(torch.equal(host, seen[0][2]) for _, _, host in seen)          # no step drew from the host RNG
    assert torch.equal(torch.get_rng_state(), seen[0][2])


@gpu
def test_graph_step_equals_eager_with_the_recipe_options():
    _graph_against_eager(use_spectral=True, add_noise=True)


# ---- 5. refusals and defaults ----------------------------------------------------------------------------------------------
@gpu
def test_host_drawn_diff_aug_is_still_refused_and_the_message_names_the_option():
    from test_graph_step_gpu import SMALL, batch, build
    for over in ({}, {"diff_aug_rng": "host"}):
        tr = build(SMALL, "bf16", graph_step=True, diff_aug="color,translation", **over)
        assert tr.model.diffaug_rng is None
        bg, lab, df = batch(SMALL, 0)
        with pytest.raises(NotImplementedError, match="graph_step") as err:
            tr.step(bg.to(DEV), lab.to(DEV), df.to(DEV))
        assert "diff_aug_rng" in str(err.value)
        assert tr.iters == 0


@gpu
def test_device_rng_needs_a_gpu_device_and_a_known_value():
    from de_i2i_gan_amd.models.defectgan_model import DefectGanModel
    from test_graph_step_gpu import SMALL
    with pytest.raises(ValueError, match="diff_aug_rng"):
        DefectGanModel(make_opt(SMALL, "cpu", "f32", diff_aug="color", diff_aug_rng="device"))
    with pytest.raises(ValueError, match="diff_aug_rng"):
        DefectGanModel(make_opt(SMALL, DEV, "bf16", diff_aug="color", diff_aug_rng="gpu"))


@gpu
def test_default_is_the_host_path_unchanged():
    from test_graph_step_gpu import SMALL, build, run
    losses = []
    for over in ({}, {"diff_aug_rng": "host"}):
        tr = build(SMALL, "bf16", diff_aug="color,translation,cutout", **over)
        assert tr.model.diffaug_rng is None
        torch.manual_seed(5)
        for _ in run(tr, SMALL, 2):
            pass
        tr.flush_losses()
        losses.append({kind: {k: list(v) for k, v in d.items()} for kind, d in tr.losses.items()})
    assert losses[0] == losses[1] and len(losses[0]["gan"]["D"]) == 2


@gpu
def test_seed_defaults_to_one_draw_from_the_host_rng_and_survives_a_load():
    from test_graph_step_gpu import SMALL, batch, build
    tr = build(SMALL, "bf16", diff_aug="color", diff_aug_rng="device")
    again = build(SMALL, "bf16", diff_aug="color", diff_aug_rng="device")
    seed, calls = tr.model.diffaug_rng.state()
    assert 0 <= seed < 2 ** 63 and calls == 0 and again.model.diffaug_rng.state() == (seed, 0)      # (build seeds the host RNG)
    bg, lab, df = batch(SMALL, 0)
    tr.step(bg.to(DEV), lab.to(DEV), df.to(DEV))
    rng = tr.model.diffaug_rng
    tr.save_latest(1)
    tr.opt.load_model_name = tr.opt.name
    tr.model.load("latest")
    tr.release_graphs()
    assert tr.model.diffaug_rng is rng and rng.state() == (seed, 6)
