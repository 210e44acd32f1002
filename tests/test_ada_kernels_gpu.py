"""The kernels of adaptive discriminator augmentation: the gated draw (csrc/diffaug.hip dei2i_diffaug_draw_p), the op on a gated
table, and the controller's two launches (csrc/ada.hip dei2i_ada_measure / dei2i_ada_apply).

Everything is compared bit for bit against numpy: the gated table against the Philox reference of tests/test_diffaug_dev_gpu.py
extended by the gate block (counter word run | 2 << 16; x0 / x1 / x2 gate color / translation / cutout; applies iff
(x >> 8) * 2^-24 < p), the measured pair against integer sums, p against a float32 model of the update (a power-of-two inv_images
makes every step exact).  Only rt = (float)sum / (float)n is allowed 1 ulp, and the sequence keeps every rt at least 0.1 away from
the target, so that ulp cannot change a decision."""
import ctypes

import numpy as np
import pytest
import torch

from test_diffaug_dev_gpu import BAD_ARG, DEV, SEED, _unit, draw_reference, draw_uniforms, policy_runs

gpu = pytest.mark.gpu
H = W = 8
POLICIES = ["color", "translation,cutout", "color,translation,cutout", "cutout,color"]
PS = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0]
SEED_HALF, N_HALF = SEED, 64        # (test_ada_args_cpu.py checks on the CPU: all-on, all-off and mixed rows at p = 0.5)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def gate_reference(seed, call, policy, n, row0, p):
    """bool (runs, n, 3): whether color / translation / cutout would apply to the row (whatever the run holds)"""
    rows = np.arange(row0, row0 + n, dtype=np.uint64)
    out = np.zeros((len(policy_runs(policy)), n, 3), dtype=bool)
    for r in range(out.shape[0]):
        x = draw_uniforms(seed, call, r, rows, 2)
        for j in range(3):
            out[r, :, j] = _unit(x[j]) < np.float32(p)
    return out


def gated_reference(seed, call, policy, n, row0, h, w, p):
    rec = draw_reference(seed, call, policy, n, row0, h, w).copy()
    gates = gate_reference(seed, call, policy, n, row0, p)
    one = np.float32(1).view(np.int32)
    for r, names in enumerate(policy_runs(policy)):
        if "color" in names:
            off = ~gates[r, :, 0]
            rec[r, off, 0], rec[r, off, 1:4] = one, 0
        if "translation" in names:
            rec[r, ~gates[r, :, 1], 4:6] = 0
        if "cutout" in names:
            off = ~gates[r, :, 2]
            rec[r, off, 6], rec[r, off, 7] = h, w
    return rec


def identity_table(policy, n, h, w):
    rec = np.zeros((len(policy_runs(policy)), n, 8), dtype=np.int32)
    rec[:, :, 0] = np.float32(1).view(np.int32)
    for r, names in enumerate(policy_runs(policy)):
        if "cutout" in names:
            rec[r, :, 6], rec[r, :, 7] = h, w
    return rec


def _word(p):
    return torch.tensor([p], dtype=torch.float32, device=DEV)


# ---- 1. the gated table ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("policy", POLICIES)
def test_gated_table_matches_the_reference_bit_for_bit(policy):
    from de_i2i_gan_amd import ops
    rng, plain = ops.DiffAugRng(SEED, DEV), ops.DiffAugRng(SEED, DEV)
    seen = set()
    for h, w in ((H, W), (9, 7)):
        for n in (1, 5, 257):
            for row0 in (0, 3):
                for p in PS:
                    rng.set_state((SEED, 6))
                    for call in (6, 7):                     # two consecutive calls: the launch advances the counter by exactly 1
                        tab, runs = ops.diffaug_draw(rng, policy, n, h, w, row0=row0, p=_word(p))
                        got = tab.cpu().numpy()
                        assert rng.state() == (SEED, call + 1), (n, row0, p, call)
                        want = gated_reference(SEED, call, policy, n, row0, h, w, p)
                        assert got.dtype == np.int32 and got.shape == want.shape
                        assert np.array_equal(got, want), (h, w, n, row0, p, call, np.argwhere(got != want)[:4])
                        if p == 1.0:
                            plain.set_state((SEED, call))
                            ungated, plain_runs = ops.diffaug_draw(plain, policy, n, h, w, row0=row0)
                            assert torch.equal(tab, ungated) and runs == plain_runs
                            assert np.array_equal(got, draw_reference(SEED, call, policy, n, row0, h, w))
                        if p == 0.0:
                            assert np.array_equal(got, identity_table(policy, n, h, w))
                        if n == 257:
                            seen.add((p, bool((got != identity_table(policy, n, h, w)).any())))
    assert (0.5, True) in seen and (0.0, False) in seen


@gpu
def test_a_rows_parameters_do_not_depend_on_its_gates():
    from de_i2i_gan_amd import ops
    policy, n = "color,translation,cutout", N_HALF
    rng = ops.DiffAugRng(SEED_HALF, DEV)
    half = ops.diffaug_draw(rng, policy, n, H, W, p=_word(0.5))[0].cpu().numpy()[0]
    full = draw_reference(SEED_HALF, 0, policy, n, 0, H, W)[0]
    gates = gate_reference(SEED_HALF, 0, policy, n, 0, 0.5)[0]
    for j, cols in enumerate((slice(0, 4), slice(4, 6), slice(6, 8))):
        assert np.array_equal(half[gates[:, j]][:, cols], full[gates[:, j]][:, cols])
    assert gates.any(axis=0).all() and (~gates).any(axis=0).all()


# ---- 2. the op on a gated table --------------------------------------------------------------------------------------------
def _image(shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV)


def _out_and_grad(aug, x, cot):
    x = x.clone().requires_grad_(True)
    y = aug(x)
    (gx,) = torch.autograd.grad(y, x, cot)
    return y.detach(), gx


@gpu
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 3, 5, 7)], ids=["float4", "scalar"])
@pytest.mark.parametrize("policy", ["color", "translation", "cutout", "color,translation,cutout"])
def test_p_zero_is_the_identity_forward_and_backward(policy, shape):
    from de_i2i_gan_amd import ops
    x, cot = _image(shape, 2), _image(shape, 3)
    rng = ops.DiffAugRng(SEED, DEV)
    y, gx = _out_and_grad(lambda t: ops.diff_augment(t, policy, rng=rng, p=_word(0.0)), x, cot)
    assert y.data_ptr() != x.data_ptr() and rng.state() == (SEED, 1)          # (the kernels ran)
    assert torch.equal(y, x) and torch.equal(gx, cot)


@gpu
def test_p_half_rows_follow_their_gates():
    from de_i2i_gan_amd import ops
    policy, n = "color,translation,cutout", N_HALF
    gates = gate_reference(SEED_HALF, 0, policy, n, 0, 0.5)[0]
    on = gates.sum(axis=1)
    all_on, all_off = torch.from_numpy(on == 3).to(DEV), torch.from_numpy(on == 0).to(DEV)
    assert (on == 3).any() and (on == 0).any() and ((on > 0) & (on < 3)).any()
    x, cot = _image((n, 3, H, W), 4), _image((n, 3, H, W), 5)
    rng = ops.DiffAugRng(SEED_HALF, DEV)
    y, gx = _out_and_grad(lambda t: ops.diff_augment(t, policy, rng=rng, p=_word(0.5)), x, cot)
    rng.set_state((SEED_HALF, 0))
    y_full, gx_full = _out_and_grad(lambda t: ops.diff_augment(t, policy, rng=rng), x, cot)
    assert torch.equal(y[all_off], x[all_off]) and torch.equal(gx[all_off], cot[all_off])
    assert torch.equal(y[all_on], y_full[all_on]) and torch.equal(gx[all_on], gx_full[all_on])
    assert not torch.equal(y[all_on], x[all_on]) and not torch.equal(y, y_full)


@gpu
def test_p_needs_an_rng_and_a_device_word():
    from de_i2i_gan_amd import ops
    x = _image((2, 3, 8, 8), 1)
    with pytest.raises(ValueError, match="rng"):
        ops.diff_augment(x, "color", p=_word(0.5))
    rng = ops.DiffAugRng(SEED, DEV)
    for bad in (0.5, torch.tensor([0.5]), torch.tensor([0.5, 0.5], device=DEV), torch.tensor([0.5], dtype=torch.float64, device=DEV)):
        with pytest.raises(ValueError, match="p is"):
            ops.diff_augment(x, "color", rng=rng, p=bad)
    assert rng.state() == (SEED, 0)


# ---- 3. the controller -----------------------------------------------------------------------------------------------------
def _logits(n):
    g = np.random.default_rng(n)
    x = g.standard_normal(n).astype(np.float32)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39], dtype=np.float32)
    idx = g.permutation(n)[:special.size]
    x[idx] = special[:idx.size]
    return x


def _sign_sum(x):
    return int((x > 0).sum()) - int((x < 0).sum())


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_measure_counts_signs_exactly(n):
    from de_i2i_gan_amd import ops
    x, more = _logits(n), -_logits(n + 1)[:n]
    st = ops.AdaState(DEV)
    st.pair.fill_(-12345)                                   # (accumulate = 0 overwrites)
    st.measure(torch.from_numpy(x).to(DEV))
    assert st.pair.tolist() == [_sign_sum(x), n]
    lib = ops._lib_for(st.pair)
    t = torch.from_numpy(more).to(DEV)
    assert lib.dei2i_ada_measure(ctypes.c_void_p(t.data_ptr()), n, ctypes.c_void_p(st.pair.data_ptr()), 1, ops._stream()) == 0
    assert st.pair.tolist() == [_sign_sum(x) + _sign_sum(more), 2 * n]
    if n == 1000:                                           # the extremes, and AdaState.measure over several tensors
        st.measure(torch.ones(n, device=DEV), torch.full((7,), -1.0, device=DEV).to(torch.bfloat16))
        assert st.pair.tolist() == [n - 7, n + 7]
        whole = torch.from_numpy(x).to(DEV)
        st.measure(*whole.split([300, 700]))                # consecutive slices of one buffer: one launch over both
        assert st.pair.tolist() == [_sign_sum(x), n]


def _ulp_apart(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, b) == b


@gpu
def test_apply_follows_the_float32_model_for_twelve_calls():
    """interval 3, inv_images 2^-10, p from 0.25 with p_max 0.75: up by 48 rows (rt 0.9), up into p_max by 768 rows (rt 0.8), down by
    48 rows (rt 0.1), down into 0 by 1536 rows (rt -1); the last call of each interval carries the odd row counts"""
    from de_i2i_gan_amd import ops
    target, interval, p_max = 0.6, 3, 0.75
    st = ops.AdaState(DEV, p=0.25, target=target, interval=interval, kimg=2.0 ** 10 / 1000.0, p_max=p_max)
    inv = np.float32(2.0 ** -10)
    assert st.inv_images == float(inv) and st.state()["p"] == 0.25
    calls = ([(90, 100, 16)] * 3 + [(70, 100, 5), (80, 100, 250), (90, 100, 513)] + [(10, 100, 16)] * 3
             + [(-100, 100, 512), (-7, 7, 1), (-1, 1, 1023)])
    assert len(calls) == 12
    p, rt, acc, trail = np.float32(0.25), np.float32(0.0), np.zeros(4, dtype=np.int64), []
    for s, n, rows in calls:
        st.pair.copy_(torch.tensor([s, n], dtype=torch.int64))
        st.apply(rows)
        acc = acc + np.array([s, n, rows, 1], dtype=np.int64)
        if acc[3] == interval:
            rt = np.float32(acc[0]) / np.float32(acc[1])
            assert abs(float(rt) - target) >= 0.1            # (a last-bit difference of the division cannot change the decision)
            step = np.float32(acc[2]) * inv
            p = np.float32(p + (step if rt > np.float32(target) else -step if rt < np.float32(target) else np.float32(0)))
            p = np.float32(min(max(p, np.float32(0)), np.float32(p_max)))
            acc = np.zeros(4, dtype=np.int64)
        got = st.state()
        assert np.float32(got["p"]).view(np.int32) == p.view(np.int32), (got, p)
        assert _ulp_apart(got["rt"], rt), (got, rt)
        assert [got[k] for k in ("sum_sign", "n_logits", "rows", "calls")] == acc.tolist(), got
        assert st.pair.tolist() == [s, n]                   # (the pair is read, not consumed)
        trail.append(float(p))
    assert trail == [0.25] * 2 + [0.296875] * 3 + [0.75] * 3 + [0.703125] * 3 + [0.0]
    assert acc.tolist() == [0, 0, 0, 0]


@gpu
def test_state_round_trips():
    from de_i2i_gan_amd import ops
    st = ops.AdaState(DEV, p=0.3)
    assert st.state() == dict(p=float(np.float32(0.3)), rt=0.0, sum_sign=0, n_logits=0, rows=0, calls=0)
    want = dict(p=float(np.float32(0.7)), rt=float(np.float32(-0.25)), sum_sign=-5, n_logits=2 ** 40, rows=9, calls=2)
    st.set_state(want)
    assert st.state() == want and st.p.data_ptr() == st.p_rt.data_ptr() and st.rt.item() == want["rt"]
    with pytest.raises(ValueError):
        ops.AdaState("cpu")


# ---- 4. refused arguments --------------------------------------------------------------------------------------------------
@gpu
def test_entry_points_refuse_bad_arguments():
    from de_i2i_gan_amd import ops
    rng, st = ops.DiffAugRng(SEED, DEV), ops.AdaState(DEV, p=0.5)
    tab = torch.zeros(2, 4, 8, dtype=torch.int32, device=DEV)
    x = torch.ones(8, device=DEV)
    lib, s = ops._lib_for(tab), ops._stream()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731

    def draw(counter=ptr(rng.counter), runs=1, flags=7, n=4, row0=0, h=8, w=8, p=ptr(st.p), table=ptr(tab)):
        return lib.dei2i_diffaug_draw_p(SEED, counter, runs, flags, n, row0, h, w, p, table, s)

    assert draw() == 0
    for bad in (dict(p=None), dict(counter=None), dict(table=None), dict(runs=0), dict(n=0), dict(row0=-1), dict(h=0), dict(w=0),
                dict(flags=0), dict(flags=7 | 1 << 3), dict(runs=2, flags=7), dict(n=2, row0=2 ** 31 - 1)):
        assert draw(**bad) == BAD_ARG, bad
    assert rng.state() == (SEED, 1)                         # the refused calls launched nothing

    def measure(logits=ptr(x), n=8, pair=ptr(st.pair), accumulate=0):
        return lib.dei2i_ada_measure(logits, n, pair, accumulate, s)

    assert measure() == 0 and st.pair.tolist() == [8, 8]
    for bad in (dict(logits=None), dict(pair=None), dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(n=2 ** 40)):
        assert measure(**bad) == BAD_ARG, bad

    def apply(pair=ptr(st.pair), rows=4, p_rt=ptr(st.p_rt), acc=ptr(st.acc), interval=4, target=0.6, inv=2.0 ** -10, p_max=1.0):
        return lib.dei2i_ada_apply(pair, rows, p_rt, acc, interval, target, inv, p_max, s)

    assert apply() == 0
    for bad in (dict(pair=None), dict(p_rt=None), dict(acc=None), dict(interval=0), dict(interval=-1), dict(rows=0), dict(rows=-4),
                dict(p_max=-0.5), dict(p_max=1.5), dict(p_max=float("nan")), dict(target=1.0), dict(target=-1.0),
                dict(target=float("nan")), dict(inv=-1.0)):
        assert apply(**bad) == BAD_ARG, bad
    assert st.state() == dict(p=0.5, rt=0.0, sum_sign=8, n_logits=8, rows=4, calls=1)
