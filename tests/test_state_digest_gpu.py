"""ops.state_digest (csrc/adam.hip: state_digest_kernel + its one-workgroup sum) against the numpy reference of the definition
(tests/digest_reference.py): equality of the 64-bit word, nothing needs a tolerance -- the digest is integer arithmetic mod 2^64.

Sizes: around the 16-byte vector width (1, 3, 4, 5), around one workgroup's 256 lanes and 4 words a lane (255 .. 1025), one past the
grid's cap of 512 workgroups x 256 lanes x 4 words (every lane then strides), a view that starts one element into its buffer (the
word-by-word path), a 0-dim int64, a table whose rows differ in length by 1000x (workgroups with no word store 0) and a list that
goes out in two launches (row0)."""
import numpy as np
import pytest
import torch

import digest_reference as R

DEV = "cuda:0"
GRID_CAP_WORDS = 512 * 256 * 4
M64 = 2 ** 64 - 1


def test_reference_known_answers():
    """CPU: the reference itself, on the two values the definition is published with"""
    assert int(R.splitmix64(0)) == R.SPLITMIX64_OF_ZERO == 0xE220A8397B1DCDAF
    assert R.digest([np.zeros(1, np.float32)]) == R.DIGEST_OF_ONE_FP32_ZERO == 0xA706DD2F4D197E6F
    # by hand: one word 0 at (k, i) = (0, 0) is splitmix64(splitmix64(0) + 0)
    assert R.digest([np.zeros(1, np.float32)]) == int(R.splitmix64(R.splitmix64(0)))
    assert R.digest([np.zeros(1, np.float32)], row0=1) == int(R.splitmix64(R.splitmix64(1 << 32)))
    a, b = np.arange(5, dtype=np.float32), np.arange(7, dtype=np.int64)
    assert R.digest([a, b]) == (R.digest([a]) + R.digest([b], row0=1)) & M64
    assert R.digest([a, b]) != R.digest([b, a])


def got(tensors, **kw):
    from de_i2i_gan_amd import ops
    out = ops.state_digest(tensors, **kw)
    assert out.shape == (1,) and out.dtype == torch.int64 and out.is_cuda
    return int(out.item()) & M64


def rand(n, seed):
    """n fp32 words of every exponent (random bits, NaNs included)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32).to(DEV)


@pytest.mark.gpu
def test_known_answers():
    assert got([torch.zeros(1, device=DEV)]) == 0xA706DD2F4D197E6F
    assert got([torch.zeros(1, dtype=torch.int32, device=DEV)]) == int(R.splitmix64(R.splitmix64(0)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, GRID_CAP_WORDS + 5])
def test_word_counts(n):
    t = rand(n, n)
    assert t.data_ptr() % 16 == 0
    assert got([t]) == R.of_tensors([t])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257, 1025])
def test_unaligned_view_takes_the_scalar_path(n):
    buf = rand(n + 1, 7 * n)
    view = buf[1:]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert got([view]) == R.of_tensors([view])
    assert got([view]) == got([view.clone()])            # (the same words through the 16-byte path)


@pytest.mark.gpu
def test_zero_dim_int64_and_mixed_dtypes():
    tensors = [torch.tensor(-3, dtype=torch.int64, device=DEV), rand(9, 1), torch.arange(6, device=DEV, dtype=torch.int64),
               torch.randn(5, 4, device=DEV).bfloat16(), torch.zeros(0, device=DEV), torch.ones(3, dtype=torch.float64, device=DEV)]
    assert got(tensors[:1]) == R.of_tensors(tensors[:1])
    assert got(tensors) == R.of_tensors(tensors)


@pytest.mark.gpu
def test_rows_that_differ_in_length_by_1000x():
    tensors = [rand(3, 1), rand(3000, 2), rand(1, 3), rand(300_000, 4), rand(300, 5)]
    assert got(tensors) == R.of_tensors(tensors)


@pytest.mark.gpu
def test_a_list_split_over_two_launches():
    tensors = [rand(n, n) for n in (5, 1030, 1, 64, 257)]
    want = R.of_tensors(tensors)
    assert got(tensors) == want
    assert got(tensors, rows_per_launch=3) == want       # rows 0..2, then rows 3..4 with row0 = 3 added into the same word
    assert got(tensors, rows_per_launch=1) == want
    assert R.of_tensors(tensors[3:], row0=3) == (want - R.of_tensors(tensors[:3])) & M64


@pytest.mark.gpu
def test_non_contiguous_inputs_are_made_contiguous():
    t = rand(48, 3).view(6, 8)
    assert got([t.t()]) == R.of_tensors([t.t().contiguous()]) != got([t])


@pytest.mark.gpu
def test_sensitivity():
    a, b = rand(100, 1), rand(100, 2)
    base = got([a, b])
    assert base == got([a.clone(), b.clone()])
    swapped = a.clone()
    swapped[[3, 70]] = swapped[[70, 3]]
    assert not torch.equal(swapped.view(torch.int32), a.view(torch.int32))
    assert got([swapped, b]) != base                     # two elements swapped
    assert got([b, a]) != base                           # two tensors swapped
    z = torch.zeros(8, device=DEV)
    neg = z.clone()
    neg[5] = -0.0
    assert torch.equal(z, neg) and got([z]) != got([neg])                         # the sign of a zero
    nan = torch.full((8,), float("nan"), device=DEV)
    other = nan.clone()
    other.view(torch.int32)[2] ^= 1                      # one payload bit
    assert bool(other.isnan().all()) and got([nan]) != got([other])
    for x, y in ((z, neg), (nan, other)):
        assert got([x]) == R.of_tensors([x]) and got([y]) == R.of_tensors([y])


@pytest.mark.gpu
def test_no_host_wait():
    """the call only queues work: torch's synchronisation check (every blocking call of its own raises) stays silent"""
    from de_i2i_gan_amd import ops
    t = [rand(1024, 9), rand(7, 10)[1:]]
    ops.state_digest(t)                                  # (library initialisation, the first pinned buffer)
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.state_digest(t)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out.item()) & M64 == R.of_tensors(t)


def test_refusals_cpu():
    from de_i2i_gan_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.state_digest([torch.zeros(4)])
    with pytest.raises(ValueError):
        ops.state_digest([])


@pytest.mark.gpu
def test_refusals():
    from de_i2i_gan_amd import ops
    with pytest.raises(ValueError, match="32-bit words"):
        ops.state_digest([torch.zeros(3, dtype=torch.bfloat16, device=DEV)])
    with pytest.raises(ValueError, match="32-bit words"):
        ops.state_digest([torch.zeros(4, device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.state_digest([torch.zeros(4, device=DEV), torch.zeros(4)])
    with pytest.raises(ValueError):
        ops.state_digest([torch.zeros(4, device=DEV)], rows_per_launch=0)
