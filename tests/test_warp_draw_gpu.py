"""GPU: the device-drawn matrix table of the warp runs (csrc/warp.hip dei2i_warp_draw / dei2i_warp_draw_p, ops.warp_draw) against the
Philox reference of tests/warp_reference.py: exact identities, the entries within a closed-form tolerance of a float64 matrix built
from the same words, the gates bit for bit, slices of the global batch, the call count and the launch order of a diff_augment call."""
import ctypes

import numpy as np
import pytest
import torch

import warp_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x5DEECE66D1234567
F = np.float32
ALL = "scale,rotate,aniso"
MIXED = "scale,color,rotate,flip,aniso"          # runs [scale] [color] [rotate] [flip] [aniso]: warp runs at index 0, 2 and 4
IDENT = np.array([1, 0, 0, 1, 0, 0, 0, 0], dtype=F)

# The tolerance of an entry, in closed form.  exp2f, sinf and cosf are the device library's accurate functions; the library documents
# that they meet the OpenCL full-profile limits, which are 3 ulp for exp2 and 4 ulp for sin and cos.  Their arguments are formed
# exactly as the reference forms them, so an entry such as m00 = l * (c * s) carries the error of one cos or sin (4 ulp), two exp2
# (3 ulp each; 1 / l has l's relative error) and two fp32 multiplies or divides (half an ulp each): 4 + 2 * 3 + 2 * 0.5 = 11 ulp,
# an ulp being at most 2^-23 of the value, the value at most 2 (s, l <= sqrt 2); the factor 1 + 2^-10 covers the products of errors.
ULP_EXP2, ULP_SINCOS = 3.0, 4.0
TOL = 2.0 * (ULP_SINCOS + 2 * ULP_EXP2 + 2 * 0.5) * 2.0 ** -23 * (1 + 2.0 ** -10)          # 2.63e-6


def _p(value):
    return torch.tensor([value], dtype=torch.float32, device=DEV)


def _draw(rng, policy, n, call, row0=0, p=None):
    from de_i2i_gan_amd import ops
    rng.set_state((SEED, call))
    tab = ops.warp_draw(rng, policy, n, row0=row0, p=None if p is None else _p(p))
    assert rng.state() == (SEED, call + 1)                            # exactly one per launch
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (len(R.warp_runs(policy)), n, 8)
    return tab.cpu().numpy().view(F)


@pytest.fixture(scope="module")
def rng():
    from de_i2i_gan_amd import ops
    return ops.DiffAugRng(SEED, DEV)


def test_identities_of_absent_policies_are_exact(rng):
    m = _draw(rng, "scale", 512, 3)[0]
    assert (m[:, 1] == 0).all() and (m[:, 2] == 0).all() and np.array_equal(m[:, 0], m[:, 3]) and len(set(m[:, 0].tolist())) > 400
    m = _draw(rng, "scale,aniso", 512, 3)[0]                          # rotate absent: cos = 1, sin = 0
    assert (m[:, 1] == 0).all() and (m[:, 2] == 0).all() and (m[:, 0] != m[:, 3]).any()
    m = _draw(rng, "scale,rotate", 512, 3)[0]                         # aniso absent: l = 1
    assert np.array_equal(m[:, 0], m[:, 3]) and np.array_equal(m[:, 1], -m[:, 2]) and (m[:, 1] != 0).any()
    m = _draw(rng, "rotate", 512, 3)[0]                               # scale and aniso absent
    assert np.array_equal(m[:, 0], m[:, 3]) and np.array_equal(m[:, 1], -m[:, 2])
    assert np.abs(m[:, 0].astype(np.float64) ** 2 + m[:, 2].astype(np.float64) ** 2 - 1).max() < 1e-6
    m = _draw(rng, "aniso", 512, 3)[0]
    assert (m[:, 1] == 0).all() and (m[:, 2] == 0).all() and np.array_equal(m[:, 3], F(1) / m[:, 0])
    assert not _draw(rng, ALL, 512, 3)[0, :, 4:].view(np.int32).any()          # tu = tv = 0 and the pad words


@pytest.mark.parametrize("policy", [ALL, MIXED, "rotate,scale", "aniso,aniso,cutout,scale,aniso"])
def test_entries_are_within_the_closed_form_tolerance_of_the_float64_matrix(rng, policy):
    """TOL = 2 * (4 + 2 * 3 + 2 * 0.5) * 2^-23 * (1 + 2^-10) = 2.63e-6 (derivation above; not tuned to what is observed)"""
    worst = 0.0
    for call in (0, 2 ** 32 + 5):
        for n, row0 in ((5, 3), (4096, 0)):
            got = _draw(rng, policy, n, call, row0)
            want = R.matrix64(SEED, call, policy, n, row0)
            worst = max(worst, float(np.abs(got[:, :, :4].astype(np.float64) - want).max()))
    print(f"[warp-draw] {policy}: max |device entry - float64 entry| = {worst:.3e} (tolerance {TOL:.3e})", flush=True)
    assert worst <= TOL


def test_gates(rng):
    n, row0, call = 4096, 3, 4
    plain = _draw(rng, MIXED, n, call, row0)
    assert np.array_equal(_draw(rng, MIXED, n, call, row0, p=1.0).view(np.int32), plain.view(np.int32))      # p = 1: bit for bit
    none = _draw(rng, MIXED, n, call, row0, p=0.0)
    assert (none == IDENT).all()                                      # p = 0: identity records only
    half = _draw(rng, MIXED, n, call, row0, p=0.5)
    passes = R.gates(SEED, call, MIXED, n, row0, 0.5)                 # (warp runs, n, 3): block 5, x0 scale, x1 rotate, x2 aniso
    for b, k in enumerate((0, 1, 2)):                                 # run b holds the one policy k
        gate = passes[b, :, k]
        assert 0.4 < gate.mean() < 0.6
        assert np.array_equal(half[b][gate].view(np.int32), plain[b][gate].view(np.int32))      # parameters unchanged by gating
        assert (half[b][~gate] == IDENT).all() and (plain[b][~gate] != IDENT).any(axis=1).all()
    # one run with all three policies: all gates passing is the ungated row, none passing the identity, the rest within tolerance
    plain, half = _draw(rng, ALL, n, call, row0)[0], _draw(rng, ALL, n, call, row0, p=0.5)[0]
    passes = R.gates(SEED, call, ALL, n, row0, 0.5)[0]
    every, no = passes.all(axis=1), ~passes.any(axis=1)
    assert every.sum() > 300 and no.sum() > 300
    assert np.array_equal(half[every].view(np.int32), plain[every].view(np.int32)) and (half[no] == IDENT).all()
    assert np.abs(half[:, :4].astype(np.float64) - R.matrix64(SEED, call, ALL, n, row0, p=0.5)[0]).max() <= TOL
    assert np.array_equal(_draw(rng, ALL, n, call, row0, p=1.0)[0].view(np.int32), plain.view(np.int32))


def test_rows_are_a_slice_of_the_whole_batch_and_calls_differ(rng):
    from de_i2i_gan_amd import ops
    for p in (None, 0.5):
        whole = _draw(rng, MIXED, 64, 7, p=p)
        gate = None if p is None else _p(p)
        nxt = ops.warp_draw(rng, MIXED, 64, p=gate).cpu().numpy().view(F)          # the count the first launch left
        assert rng.state() == (SEED, 9) and not np.array_equal(whole, nxt)
        assert np.array_equal(_draw(rng, MIXED, 16, 7, row0=32, p=p).view(np.int32), whole[:, 32:48].view(np.int32))


def test_a_diff_augment_call_draws_affine_then_blit_then_warp(rng):
    from de_i2i_gan_amd import ops
    policy = "color,flip,rotate"
    x = torch.rand(5, 3, 9, 9, device=DEV)
    rng.set_state((SEED, 20))
    got = ops.diff_augment(x, policy, rng=rng)
    assert rng.state() == (SEED, 23)
    rng.set_state((SEED, 20))
    tab, runs = ops.diffaug_draw(rng, policy, 5, 9, 9)
    assert rng.state() == (SEED, 21) and runs == [(True, 0, 0), "blit", "warp"]
    codes = ops.blit_draw(rng, policy, 5)
    assert rng.state() == (SEED, 22)
    mats = ops.warp_draw(rng, policy, 5)
    assert rng.state() == (SEED, 23)
    want = ops._Warp.apply(ops._Blit.apply(ops._DiffAug.apply(x, tab[0], runs[0], 0, None), codes[0], None), mats[0], None)
    assert torch.equal(got, want)
    m = mats.cpu().numpy().view(F)
    assert np.abs(m[:, :, :4].astype(np.float64) - R.matrix64(SEED, 22, policy, 5, 0)).max() <= TOL          # the warp draw saw call + 2
    assert np.abs(m[:, :, :4].astype(np.float64) - R.matrix64(SEED, 20, policy, 5, 0)).max() > 1e-3
    # a policy without warp names launches what it launched
    for pol, step in (("color", 1), ("color,flip", 2), ("flip", 1), ("rotate", 1), ("flip,scale", 2), ("color,aniso", 2)):
        before = rng.state()[1]
        ops.diff_augment(x, pol, rng=rng)
        assert rng.state() == (SEED, before + step), pol
    with pytest.raises(ValueError):
        ops.warp_draw(rng, "color,flip", 5)
    with pytest.raises(KeyError):
        ops.diff_augment(x, "rotate,zoom", rng=rng)
    tab, runs = ops.diffaug_draw(rng, "scale,rotate", 5, 9, 9)
    assert tab is None and runs == ["warp"]                           # no affine run: no launch
    assert rng.state() == (SEED, 23 + 9)


def test_singular_values_of_drawn_matrices_lie_between_a_half_and_two(rng):
    m = _draw(rng, ALL, 4096, 11)[0, :, :4].astype(np.float64).reshape(4096, 2, 2)
    sv = np.linalg.svd(m, compute_uv=False)
    # an entry is within TOL of the exact matrix, whose singular values lie in [1/2, 2]; they move by at most the Frobenius norm 2 TOL
    assert sv.min() >= 0.5 - 2 * TOL and sv.max() <= 2 + 2 * TOL and sv.min() < 0.6 and sv.max() > 1.8
    inv = np.linalg.inv(m)
    assert np.abs(m).max() <= 2 + TOL and np.abs(inv).max() <= 2 + 1e-5          # far inside the usable gate


def test_draw_refuses_bad_arguments(rng):
    from de_i2i_gan_amd import _lib, ops
    rng.set_state((SEED, 0))
    tab = torch.zeros(2, 4, 8, dtype=torch.int32, device=DEV)
    gate = _p(0.5)
    lib = ops._lib_for(tab)
    c, t, st = ctypes.c_void_p(rng.counter.data_ptr()), ctypes.c_void_p(tab.data_ptr()), ops._stream()

    def draw(counter=c, runs=1, flags=7, n=4, row0=0, table=t):
        return lib.dei2i_warp_draw(SEED, counter, runs, flags, n, row0, table, st)

    assert draw() == 0
    for bad in (dict(counter=None), dict(table=None), dict(runs=0), dict(runs=_lib.DIFFAUG_MAX_RUNS + 1), dict(n=0), dict(row0=-1),
                dict(flags=0), dict(flags=7 | 1 << 3), dict(runs=2, flags=0), dict(n=2, row0=2 ** 31 - 1), dict(runs=16, n=2 ** 20)):
        assert draw(**bad) == _lib.ERR_BAD_ARG, bad
    assert lib.dei2i_warp_draw_p(SEED, c, 1, 7, 4, 0, None, t, st) == _lib.ERR_BAD_ARG
    assert lib.dei2i_warp_draw_p(SEED, c, 1, 7, 4, 0, ctypes.c_void_p(gate.data_ptr()), t, st) == 0
    assert draw(runs=2, flags=2 << 3) == 0                            # (a list whose first run is not a warp run)
    assert rng.state() == (SEED, 3)                                   # the refused calls launched nothing
    with pytest.raises(ValueError):
        ops.warp_draw(rng, ",".join(["scale"] * (_lib.DIFFAUG_MAX_RUNS + 1)), 2)
