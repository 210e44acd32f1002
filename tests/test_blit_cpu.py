"""CPU: the pixel-blitting DiffAugment policies flip and rot90 (utils/diffaug.py) -- the torch-op functions against the numpy index
maps of tests/blit_reference.py for all eight codes, draw_params against the functions' RNG consumption and draws, its shards, the
run split, and the refusals that must come before any draw.  Everything is compared exactly."""
import numpy as np
import pytest
import torch

import blit_reference as R

POLICIES = ["flip", "rot90", "flip,rot90", "rot90,flip", "flip,color,translation", "rot90,cutout,flip",
            "flip,rot90,color,translation,cutout"]


def _arange(n, c, h, w):
    return torch.arange(n * c * h * w, dtype=torch.float32).view(n, c, h, w)


def test_reference_index_maps_are_torch_rot90_and_flip():
    x = _arange(8, 2, 5, 5)
    got = R.blit(x.numpy(), np.arange(8))
    for code in range(8):
        f, k = code & 1, code >> 1
        want = torch.rot90(x[code].flip(2) if f else x[code], k, dims=(1, 2))
        assert np.array_equal(got[code], want.numpy()), code
        back = R.blit(got[code:code + 1], [R.inverse_code(code)])
        assert np.array_equal(back[0], x[code].numpy()), code


def _codes_of_the_next_draws(policy, n):
    """what the policy functions will draw from the current CPU RNG state, read without disturbing the caller's comparison"""
    state = torch.get_rng_state()
    out = [torch.randint(0, 2 if name == "flip" else 4, size=[n, 1, 1]).view(n).numpy() for name in policy.split(",")]
    torch.set_rng_state(state)
    return out


@pytest.mark.parametrize("policy", ["flip", "rot90", "flip,rot90", "rot90,flip"])
def test_policy_functions_match_the_reference_for_all_codes(policy):
    from de_i2i_gan_amd.utils.diffaug import diff_augment
    x = _arange(64, 2, 6, 6)
    torch.manual_seed(3)
    draws = _codes_of_the_next_draws(policy, 64)
    got = diff_augment(x, policy)
    want, seen = x.numpy(), set()
    for name, d in zip(policy.split(","), draws):
        codes = d if name == "flip" else d << 1
        want = R.blit(want, codes)
        seen |= set(int(c) for c in codes)
    assert np.array_equal(got.numpy(), want) and got.is_contiguous()
    assert seen == ({0, 1} if policy == "flip" else {0, 2, 4, 6} if policy == "rot90" else {0, 1, 2, 4, 6})


def test_flip_takes_non_square_images_and_one_run_is_one_code():
    from de_i2i_gan_amd.utils.diffaug import diff_augment, draw_params
    x = _arange(16, 3, 5, 12)
    torch.manual_seed(8)
    got = diff_augment(x, "flip")
    torch.manual_seed(8)
    rec, runs = draw_params("flip", 16, 5, 12)
    assert np.array_equal(got.numpy(), R.blit(x.numpy(), rec[0, :, 0]))
    y = _arange(64, 1, 4, 4)
    torch.manual_seed(9)
    got = diff_augment(y, "flip,rot90")
    torch.manual_seed(9)
    rec, runs = draw_params("flip,rot90", 64, 4, 4)
    assert runs == ["blit"] and set(rec[0, :, 0].tolist()) == set(range(8)) and not rec[:, :, 1:].any()
    assert np.array_equal(got.numpy(), R.blit(y.numpy(), rec[0, :, 0]))          # c = f | k << 1: flip first, then k turns


@pytest.mark.parametrize("policy", POLICIES)
def test_draw_params_consumes_the_rng_like_the_functions(policy):
    from de_i2i_gan_amd.utils.diffaug import diff_augment, draw_params
    x = torch.rand(3, 3, 12, 12)
    torch.manual_seed(7)
    diff_augment(x, policy)
    after = torch.rand(1)
    torch.manual_seed(7)
    rec, runs = draw_params(policy, 3, 12, 12)
    assert torch.equal(torch.rand(1), after)
    assert rec.shape == (len(runs), 3, 8) and rec.dtype == np.int32
    assert [run == "blit" for run in runs] == [names[0] in R.BLIT_CANONICAL for names in R.policy_runs(policy)]


@pytest.mark.parametrize("policy", ["flip,rot90", "rot90,translation,flip"])
def test_draw_params_shards_are_slices_of_the_global_draw(policy):
    from de_i2i_gan_amd.utils.diffaug import draw_params
    torch.manual_seed(5)
    whole, runs = draw_params(policy, 6, 8, 8)
    after = torch.rand(1)
    for rank in range(3):
        torch.manual_seed(5)
        part, part_runs = draw_params(policy, 2, 8, 8, shard=(rank, 3))
        assert torch.equal(torch.rand(1), after)
        assert part_runs == runs and np.array_equal(part, whole[:, 2 * rank:2 * rank + 2])


def test_policy_runs_keep_blit_runs_apart():
    from de_i2i_gan_amd.utils.diffaug import policy_runs
    assert policy_runs("flip,rot90,color,cutout") == [["flip", "rot90"], ["color", "cutout"]]
    assert policy_runs("rot90,flip") == [["rot90"], ["flip"]]
    assert policy_runs("color,flip,translation") == [["color"], ["flip"], ["translation"]]
    assert policy_runs("flip,flip,rot90") == [["flip"], ["flip", "rot90"]]
    assert policy_runs("color,translation,cutout") == [["color", "translation", "cutout"]]
    assert policy_runs("translation,color") == [["translation"], ["color"]]
    assert policy_runs("") == []
    for policy in POLICIES:
        assert policy_runs(policy) == R.policy_runs(policy)


@pytest.mark.parametrize("policy, error", [("flip,rot90", ValueError), ("color,rot90", ValueError), ("flip,zoom", KeyError),
                                           ("zoom,rot90", KeyError)])
def test_non_square_rot90_and_unknown_names_raise_before_any_draw(policy, error):
    from de_i2i_gan_amd.utils.diffaug import diff_augment, draw_params
    torch.manual_seed(5)
    expect = torch.rand(1)
    for call in (lambda: draw_params(policy, 2, 8, 12), lambda: draw_params(policy, 1, 8, 12, shard=(0, 2)),
                 lambda: diff_augment(torch.zeros(2, 3, 8, 12), policy)):
        torch.manual_seed(5)
        with pytest.raises(error) as err:
            call()
        assert torch.equal(torch.rand(1), expect)
        if error is KeyError:
            assert "flip" in str(err.value) and "rot90" in str(err.value) and "color" in str(err.value)


def test_reference_draws_cover_every_code():
    codes = R.draw_codes(0x5DEECE66D1234567, 0, "flip,rot90", 1024, 0)
    assert codes.shape == (1, 1024) and set(codes[0].tolist()) == set(range(8))
    assert set(R.draw_codes(0x5DEECE66D1234567, 0, "flip", 256, 0)[0].tolist()) == {0, 1}
    assert set(R.draw_codes(0x5DEECE66D1234567, 0, "rot90", 256, 0)[0].tolist()) == {0, 2, 4, 6}
