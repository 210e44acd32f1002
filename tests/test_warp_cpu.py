"""CPU: the geometric DiffAugment policies scale, rotate and aniso (utils/diffaug.py) -- the run split, the host draws, and the
torch-op resampler ``warp`` against the numpy reference of tests/warp_reference.py bit for bit; the reference adjoint against the
transpose of the reference forward."""
import numpy as np
import pytest
import torch

import warp_reference as R

F = np.float32


def _rotation(deg, s=1.0, lam=1.0):
    t = np.deg2rad(deg)
    c, sn = np.cos(t) * s, np.sin(t) * s
    return [lam * c, -lam * sn, sn / lam, c / lam, 0.0, 0.0]


def _random_usable(n, seed):
    """matrices U diag(a, b) V with a, b in {1/2, 2}: singular values 1/2 and 2, every entry and inverse entry at most 2"""
    g = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        t1, t2 = g.uniform(-np.pi, np.pi, 2)
        u = np.array([[np.cos(t1), -np.sin(t1)], [np.sin(t1), np.cos(t1)]])
        v = np.array([[np.cos(t2), -np.sin(t2)], [np.sin(t2), np.cos(t2)]])
        m = u @ np.diag(g.choice([0.5, 2.0], 2)) @ v
        rows.append([m[0, 0], m[0, 1], m[1, 0], m[1, 1], 0.0, 0.0])
    return np.array(rows, dtype=F)


GARBAGE = np.array([[np.nan, 0, 0, 1, 0, 0], [1, 0, 0, 1, np.inf, 0], [1, 0, 0, -np.inf, 0, 0], [0, 0, 0, 0, 0, 0],
                    [1e30, 0, 0, 1e30, 0, 0], [1e-40, 0, 0, 1e-40, 0, 0], [1, 2, 2, 4, 0, 0], [1, 0, 0, 1, 0, np.nan],
                    [0.1, 0, 0, 1, 0, 0], [5, 0, 0, 1, 0, 0]], dtype=F)


def test_policy_runs_group_and_split_warp_runs():
    from de_i2i_gan_amd.utils.diffaug import policy_runs
    assert policy_runs("scale,rotate,aniso") == [["scale", "rotate", "aniso"]]
    assert policy_runs("scale,aniso") == [["scale", "aniso"]]
    assert policy_runs("rotate,scale") == [["rotate"], ["scale"]]
    assert policy_runs("aniso,aniso") == [["aniso"], ["aniso"]]
    assert policy_runs("color,scale,rotate,flip,aniso,scale") == [["color"], ["scale", "rotate"], ["flip"], ["aniso"], ["scale"]]
    assert policy_runs("flip,scale,rot90") == [["flip"], ["scale"], ["rot90"]]
    assert policy_runs("translation,rotate,cutout") == [["translation"], ["rotate"], ["cutout"]]
    assert policy_runs("color,translation,cutout") == [["color", "translation", "cutout"]]
    for policy in ("scale", "color,scale,rotate,flip,aniso,scale", "rot90,aniso,color", "scale,rotate,aniso,flip,rot90,color,cutout"):
        assert policy_runs(policy) == R.policy_runs(policy)


@pytest.mark.parametrize("policy", ["scale", "rotate", "aniso", "scale,rotate,aniso", "rotate,scale", "color,rotate,scale,aniso,flip"])
def test_draw_params_consumes_one_uniform_per_policy_in_list_order(policy):
    from de_i2i_gan_amd.utils.diffaug import WARP, draw_params, policy_runs
    n = 6
    torch.manual_seed(11)
    rec, runs = draw_params(policy, n, 8, 8)
    after = torch.get_rng_state()
    torch.manual_seed(11)
    want = np.zeros((len(runs), n, 4), dtype=F)
    for r, names in enumerate(policy_runs(policy)):
        if names[0] not in R.WARP_CANONICAL:
            if names == ["color"]:
                torch.rand(n, 1, 1, 1), torch.rand(n, 1, 1, 1), torch.rand(n, 1, 1, 1)
            else:
                torch.randint(0, 2, size=[n, 1, 1])
            continue
        assert runs[r] == WARP
        s = c = lam = torch.ones(n)
        sn = torch.zeros(n)
        for name in names:
            u = torch.rand(n, 1, 1, 1).view(n)
            if name == "scale":
                s = torch.exp2(u - 0.5)
            elif name == "rotate":
                c, sn = torch.cos((2 * u - 1) * np.pi), torch.sin((2 * u - 1) * np.pi)
            else:
                lam = torch.exp2(u - 0.5)
        want[r] = torch.stack([lam * (c * s), lam * (-(sn * s)), (sn * s) / lam, (c * s) / lam], dim=1).numpy()
    assert torch.equal(torch.get_rng_state(), after)                  # the same consumption of the CPU RNG
    got = rec.view(F)
    for r, run in enumerate(runs):
        if run == WARP:
            assert np.array_equal(got[r, :, :4], want[r]) and not rec[r, :, 4:].any()
            sv = np.linalg.svd(got[r, :, :4].astype(np.float64).reshape(n, 2, 2), compute_uv=False)
            assert sv.min() >= 0.5 - 1e-6 and sv.max() <= 2 + 1e-6


def test_identities_of_absent_policies_are_exact():
    from de_i2i_gan_amd.utils.diffaug import draw_params
    torch.manual_seed(3)
    m = draw_params("scale", 32, 8, 8)[0].view(F)[0]
    assert (m[:, 1] == 0).all() and (m[:, 2] == 0).all() and np.array_equal(m[:, 0], m[:, 3]) and (m[:, 0] != 1).any()
    m = draw_params("aniso", 32, 8, 8)[0].view(F)[0]
    assert (m[:, 1] == 0).all() and (m[:, 2] == 0).all() and np.array_equal(m[:, 3], F(1) / m[:, 0]) and (m[:, 0] != m[:, 3]).any()
    m = draw_params("rotate", 32, 8, 8)[0].view(F)[0]
    assert np.array_equal(m[:, 0], m[:, 3]) and np.array_equal(m[:, 1], -m[:, 2])


@pytest.mark.parametrize("policy", ["scale,rotate", "color,rotate,scale,aniso,flip"])
def test_shard_slices_equal_the_whole_batch_rows(policy):
    from de_i2i_gan_amd.utils.diffaug import draw_params
    torch.manual_seed(5)
    whole, runs = draw_params(policy, 8, 8, 8)
    after = torch.get_rng_state()
    for rank in range(4):
        torch.manual_seed(5)
        part, part_runs = draw_params(policy, 2, 8, 8, shard=(rank, 4))
        assert part_runs == runs and np.array_equal(part, whole[:, 2 * rank:2 * rank + 2])
        assert torch.equal(torch.get_rng_state(), after)


@pytest.mark.parametrize("policy, error", [("scale,zoom", KeyError), ("zoom,rotate", KeyError), ("aniso,rot90", ValueError)])
def test_unknown_names_and_non_square_rot90_raise_before_any_draw(policy, error):
    from de_i2i_gan_amd.utils.diffaug import diff_augment, draw_params
    torch.manual_seed(0)
    before = torch.get_rng_state()
    for call in (lambda: diff_augment(torch.zeros(2, 1, 4, 6), policy), lambda: draw_params(policy, 2, 4, 6)):
        with pytest.raises(error) as err:
            call()
        assert torch.equal(torch.get_rng_state(), before)
        if error is KeyError:
            for name in ("color", "translation", "cutout", "flip", "rot90", "scale", "rotate", "aniso"):
                assert name in str(err.value)


def _check(x, rec):
    from de_i2i_gan_amd.utils.diffaug import warp
    got = warp(torch.from_numpy(x), rec).numpy()
    want = R.forward(x, rec)
    assert got.dtype == F and np.array_equal(got, want)
    return got


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 1, 33, 65)])
def test_warp_equals_the_numpy_reference_bit_for_bit(shape):
    g = np.random.default_rng(7)
    x = g.standard_normal(shape).astype(F)
    n = shape[0]
    for seed in range(3):
        _check(x, _random_usable(n, seed))
    for deg in (0, 45, 90, 180, 270, 33):
        _check(x, np.array([_rotation(deg)] * n, dtype=F))
    _check(x, np.array([_rotation(20, s=2.0, lam=1.0)] * n, dtype=F))
    _check(x, np.array([_rotation(-70, s=0.5, lam=2.0 ** 0.5)] * n, dtype=F))
    shifted = np.array([[1, 0, 0, 1, 0.25, -1.5]] * n, dtype=F)
    _check(x, shifted)
    outside = np.array([[1, 0, 0, 1, 1000, 0]] * n, dtype=F)
    assert not _check(x, outside).any()                               # a sample mapped wholly outside
    assert np.array_equal(_check(x, np.array([R.IDENTITY] * n, dtype=F)), x)


def test_unusable_records_are_the_identity():
    from de_i2i_gan_amd.utils.diffaug import warp_usable
    g = np.random.default_rng(8)
    x = g.standard_normal((len(GARBAGE), 2, 5, 7)).astype(F)
    assert not R.usable(GARBAGE).any() and not warp_usable(GARBAGE).any()
    assert np.array_equal(_check(x, GARBAGE), x)
    edge = np.array([[4, 0, 0, 0.25, 0, 0], [0.25, 0, 0, 0.25, 0, 0], [2, 0, 0, 2, 1e30, 0]], dtype=F)      # on the gate: usable
    assert R.usable(edge).all() and warp_usable(edge).all()
    assert np.array_equal(R.adjoint(x, GARBAGE), x)


def test_warp_is_twice_differentiable_and_linear():
    from de_i2i_gan_amd.utils.diffaug import warp
    rec = _random_usable(2, 4)
    x = torch.randn(2, 2, 5, 7, dtype=torch.float32, requires_grad=True)
    gy = torch.randn(2, 2, 5, 7)
    y = warp(x, rec)
    (gx,) = torch.autograd.grad((y * y * gy).sum(), x, create_graph=True)
    (ggx,) = torch.autograd.grad(gx.square().sum(), x)
    assert torch.isfinite(ggx).all() and ggx.abs().sum() > 0
    # the first-order gradient is the transpose applied to 2 y gy
    want = R.adjoint((2 * y * gy).detach().numpy(), rec)
    assert np.allclose(gx.detach().numpy(), want, rtol=1e-5, atol=1e-6)


def test_reference_adjoint_is_the_transpose_of_the_reference_forward():
    h, w = 5, 7
    for rec in (_random_usable(1, 1), np.array([_rotation(45)], dtype=F), np.array([[0.5, 0, 0, 2, 0.5, -0.25]], dtype=F)):
        fwd = np.zeros((h * w, h * w), dtype=F)          # column k: the forward of basis image k
        adj = np.zeros((h * w, h * w), dtype=F)          # column k: the adjoint of basis image k
        for k in range(h * w):
            e = np.zeros((1, 1, h, w), dtype=F)
            e.reshape(-1)[k] = 1
            fwd[:, k] = R.forward(e, rec).reshape(-1)
            adj[:, k] = R.adjoint(e, rec).reshape(-1)
        assert fwd.any() and np.array_equal(adj, fwd.T)


def test_diff_augment_applies_a_warp_run_as_one_warp():
    from de_i2i_gan_amd.utils.diffaug import diff_augment, draw_params, warp
    x = torch.randn(3, 2, 9, 9)
    torch.manual_seed(21)
    got = diff_augment(x, "scale,rotate,aniso")
    torch.manual_seed(21)
    rec, _ = draw_params("scale,rotate,aniso", 3, 9, 9)
    assert torch.equal(got, warp(x, rec.view(F)[0]))
    torch.manual_seed(21)
    two = diff_augment(x, "rotate,scale")                             # two runs: two resamplings
    torch.manual_seed(21)
    rec, _ = draw_params("rotate,scale", 3, 9, 9)
    assert torch.equal(two, warp(warp(x, rec.view(F)[0]), rec.view(F)[1]))
