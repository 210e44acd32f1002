"""GPU: the device-drawn code table of the blit runs (csrc/blit.hip dei2i_blit_draw / dei2i_blit_draw_p, ops.blit_draw) against the
numpy Philox reference of tests/blit_reference.py, bit for bit: the counter-word layout (run = the index in the whole run list,
block 3), the gates, slices of the global batch, the call count, and the launches a policy without blit names must not gain."""
import ctypes

import numpy as np
import pytest
import torch

import blit_reference as R
from test_diffaug_dev_gpu import draw_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5DEECE66D1234567
from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
MIXED = "flip,color,rot90"          # runs [flip] [color] [rot90]: blit runs at index 0 and 2


def _p(value):
    return torch.tensor([value], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("policy", [MIXED, "flip,rot90", "rot90,flip", "cutout,flip,rot90"])
def test_table_matches_the_reference_bit_for_bit(policy):
    from de_i2i_gan_amd import ops
    rng = ops.DiffAugRng(SEED, DEV)
    for call in (0, 2 ** 32 + 5):
        for n, row0 in ((5, 3), (257, 0)):
            rng.set_state((SEED, call))
            got = ops.blit_draw(rng, policy, n, row0=row0)
            assert rng.state() == (SEED, call + 1)
            want = R.draw_codes(SEED, call, policy, n, row0)
            assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (call, n, row0)


def test_mixed_policy_draws_affine_then_blit_and_both_are_the_references():
    from de_i2i_gan_amd import ops
    rng = ops.DiffAugRng(SEED, DEV)
    rng.set_state((SEED, 9))
    tab, runs = ops.diffaug_draw(rng, MIXED, 5, 16, 16, row0=3)
    assert rng.state() == (SEED, 10) and runs == ["blit", (True, 0, 0), "blit"]
    assert np.array_equal(tab.cpu().numpy(), draw_reference(SEED, 9, "color", 5, 3, 16, 16))
    codes = ops.blit_draw(rng, MIXED, 5, row0=3)
    assert rng.state() == (SEED, 11)
    assert np.array_equal(codes.cpu().numpy(), R.draw_codes(SEED, 10, MIXED, 5, 3))
    tab, runs = ops.diffaug_draw(rng, "flip,rot90", 5, 16, 16)
    assert tab is None and runs == ["blit"] and rng.state() == (SEED, 11)          # no affine run: no launch


def test_gates():
    from de_i2i_gan_amd import ops
    rng = ops.DiffAugRng(SEED, DEV)
    n, row0 = 256, 3

    def draw(p):
        rng.set_state((SEED, 4))
        out = ops.blit_draw(rng, MIXED + ",flip,rot90", n, row0=row0, p=None if p is None else _p(p))
        assert rng.state() == (SEED, 5)
        return out.cpu().numpy()

    policy = MIXED + ",flip,rot90"                                   # blit runs at 0, 2 and 3; the last holds both policies
    plain = draw(None)
    assert np.array_equal(plain, R.draw_codes(SEED, 4, policy, n, row0)) and plain.shape == (3, n)
    assert np.array_equal(draw(1.0), plain)
    assert not draw(0.0).any()
    half = draw(0.5)
    assert np.array_equal(half, R.draw_codes(SEED, 4, policy, n, row0, p=0.5))
    passes = R.gates(SEED, 4, policy, n, row0, 0.5)
    assert np.array_equal(half & 1, np.where(passes[:, :, 0], plain & 1, 0))       # a passing gate keeps the ungated bits
    assert np.array_equal(half >> 1, np.where(passes[:, :, 1], plain >> 1, 0))
    assert 0.3 < passes.mean() < 0.7 and (half != plain).any() and half.any()


def test_rows_are_a_slice_of_the_whole_batch_and_calls_differ():
    from de_i2i_gan_amd import ops
    rng = ops.DiffAugRng(SEED, DEV)
    for p in (None, 0.5):
        gate = None if p is None else _p(p)
        rng.set_state((SEED, 7))
        whole = ops.blit_draw(rng, MIXED, 64, p=gate)
        nxt = ops.blit_draw(rng, MIXED, 64, p=gate)
        assert rng.state() == (SEED, 9) and not torch.equal(whole, nxt)
        rng.set_state((SEED, 7))
        assert torch.equal(ops.blit_draw(rng, MIXED, 16, row0=32, p=gate), whole[:, 32:48])


def test_existing_policies_draw_and_count_as_before():
    """one draw launch per call, the table of the affine reference, and blit_draw refuses a policy it has nothing to draw for"""
    from de_i2i_gan_amd import ops
    rng = ops.DiffAugRng(SEED, DEV)
    policy = "color,translation,cutout"
    rng.set_state((SEED, 2))
    tab, runs = ops.diffaug_draw(rng, policy, 5, 9, 7, row0=3)
    assert rng.state() == (SEED, 3) and runs == [(True, 5, 4)]
    assert np.array_equal(tab.cpu().numpy(), draw_reference(SEED, 2, policy, 5, 3, 9, 7))
    x = torch.rand(5, 3, 9, 7, device=DEV)
    ops.diff_augment(x, policy, rng=rng)
    assert rng.state() == (SEED, 4)
    ops.diff_augment(x[:, :, :7], "flip,color,rot90", rng=rng)
    assert rng.state() == (SEED, 6)                                  # one extra launch for a call with blit runs
    ops.diff_augment(x, "flip", rng=rng)
    assert rng.state() == (SEED, 7)
    with pytest.raises(ValueError):
        ops.blit_draw(rng, policy, 5)
    with pytest.raises(ValueError):
        ops.diffaug_draw(rng, "rot90,color", 5, 9, 7)                # not square: before any launch
    with pytest.raises(ValueError):
        ops.diff_augment(x, "color,rot90", rng=rng)
    assert rng.state() == (SEED, 7)


def test_draw_refuses_bad_arguments():
    from de_i2i_gan_amd import _lib, ops
    rng = ops.DiffAugRng(SEED, DEV)
    codes = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    gate = _p(0.5)
    lib = ops._lib_for(codes)
    c, t, st = ctypes.c_void_p(rng.counter.data_ptr()), ctypes.c_void_p(codes.data_ptr()), ops._stream()

    def draw(counter=c, runs=1, flags=3, n=4, row0=0, table=t):
        return lib.dei2i_blit_draw(SEED, counter, runs, flags, n, row0, table, st)

    assert draw() == 0
    for bad in (dict(counter=None), dict(table=None), dict(runs=0), dict(runs=_lib.DIFFAUG_MAX_RUNS + 1), dict(n=0), dict(row0=-1),
                dict(flags=0), dict(flags=3 | 1 << 2), dict(runs=2, flags=0), dict(n=2, row0=2 ** 31 - 1), dict(runs=16, n=2 ** 20)):
        assert draw(**bad) == BAD_ARG, bad
    assert lib.dei2i_blit_draw_p(SEED, c, 1, 3, 4, 0, None, t, st) == BAD_ARG
    assert lib.dei2i_blit_draw_p(SEED, c, 1, 3, 4, 0, ctypes.c_void_p(gate.data_ptr()), t, st) == 0
    assert draw(runs=2, flags=2 << 2) == 0                            # (a list whose first run is not a blit run)
    assert rng.state() == (SEED, 3)                                  # the refused calls launched nothing
    with pytest.raises(ValueError):
        ops.blit_draw(rng, ",".join(["flip"] * (_lib.DIFFAUG_MAX_RUNS + 1)), 2)
