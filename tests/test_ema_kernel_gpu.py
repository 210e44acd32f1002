"""dei2i_ema_lerp_dev (csrc/adam.hip): the EMA update with its weight read from device memory, weight = weights_dev[*index_dev] --
the form a captured graph replays -- against dei2i_ema_lerp with the same float passed by value (bit for bit: the two kernels
share the element's formula) and against float64.

One table of tensors whose sizes straddle the workgroup (256 threads, one element each per pass) and the launch's grid; a second
one long enough for the grid-stride loop (more than 1024 workgroups of elements).  Weight rows 0 (an exact copy), 0.3, 0.5 (where
torch.lerp's two-sided formula changes sides) and 0.999.

The float64 bound: the formula rounds four times (the difference, 1 - w, the product, the sum), each time a quantity of at most
2 max(|p|, |e|), so the result is within 4 * 2^-24 * 2 max(|p|, |e|) = 8 * 2^-24 * max(|p|, |e|) of w e + (1 - w) p."""
import ctypes

import pytest
import torch

from de_i2i_gan_amd import _lib as L
from de_i2i_gan_amd import ops
from de_i2i_gan_amd.optim import _PointerTable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 255, 256, 257, 1023, 1024, 1025, 4099]
LONG = [5, 1024 * 256 + 257]
WEIGHTS = [0.0, 0.3, 0.5, 0.999]


def tensors(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(n, generator=g) * 2 - 1) * 10 ** float(torch.randint(-3, 3, (1,), generator=g))).to(DEV) for n in sizes]


class Case:
    def __init__(self, sizes):
        self.p = tensors(sizes, 11)
        self.e0 = tensors(sizes, 12)
        self.weights = torch.tensor(WEIGHTS, dtype=torch.float32, device=DEV)
        self.index = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.lib = ops._lib_for(self.p[0])

    def start(self):
        """-> fresh copies of the EMA tensors, and the launch arguments (device table, count, max_n) that update them from p"""
        e = [t.clone() for t in self.e0]
        table = _PointerTable("test", [(a, b, None, None) for a, b in zip(e, self.p)])
        self.table_dev = table.upload()           # (kept until the launch has run)
        return e, table.args(self.table_dev)

    def by_value(self, weight):
        e, args = self.start()
        L.check(self.lib.dei2i_ema_lerp(*args, weight, ops._stream()), "ema_lerp")
        torch.cuda.synchronize()
        return e

    def from_device(self, index=None, rows=len(WEIGHTS)):
        if index is not None:
            self.index.fill_(index)
        e, args = self.start()
        L.check(self.lib.dei2i_ema_lerp_dev(*args, ctypes.c_void_p(self.weights.data_ptr()), ctypes.c_void_p(self.index.data_ptr()),
                                            rows, ops._stream()), "ema_lerp_dev")
        torch.cuda.synchronize()
        return e

    def advance(self):
        L.check(self.lib.dei2i_index_advance(ctypes.c_void_p(self.index.data_ptr()), ops._stream()), "index_advance")


@pytest.fixture(scope="module")
def case():
    return Case(SIZES)


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("row", range(len(WEIGHTS)))
def test_device_weight_equals_the_weight_by_value_and_float64(case, row):
    got = case.from_device(row)
    want = case.by_value(WEIGHTS[row])
    w = float(torch.tensor(WEIGHTS[row], dtype=torch.float32).double())          # the float both kernels computed with
    for n, g, v, p, e0 in zip(SIZES, got, want, case.p, case.e0):
        assert torch.equal(g, v), (n, row)
        ref = w * e0.double() + (1.0 - w) * p.double()
        err = (g.double() - ref).abs()
        bound = 8 * 2.0 ** -24 * torch.maximum(p.abs(), e0.abs()).double()
        print(f"numel {n} weight {WEIGHTS[row]}: max err / bound = {(err / bound).max().item():.3f}")
        assert bool((err <= bound).all()), (n, row, (err / bound).max().item())
    if WEIGHTS[row] != 0.0:
        assert not same(got, case.e0) and not same(got, case.p)


def test_weight_zero_is_an_exact_copy(case):
    assert same(case.from_device(0), case.p)


@pytest.mark.parametrize("index", [-1, len(WEIGHTS)])
def test_an_index_outside_the_rows_changes_nothing(case, index):
    assert same(case.from_device(index), case.e0)


def test_fewer_rows_than_the_index_changes_nothing(case):
    assert same(case.from_device(2, rows=2), case.e0)


def test_index_advance_moves_the_next_launch_to_the_next_row(case):
    case.index.fill_(1)
    case.advance()
    assert same(case.from_device(), case.by_value(WEIGHTS[2]))
    case.advance()
    assert same(case.from_device(), case.by_value(WEIGHTS[3]))
    assert case.index.item() == 3


def test_grid_stride_loop():
    long = Case(LONG)
    for row in (1, 3):
        assert same(long.from_device(row), long.by_value(WEIGHTS[row])), row
    assert same(long.from_device(0), long.p)


def test_bad_arguments_are_refused(case):
    e, args = case.start()
    w, i = ctypes.c_void_p(case.weights.data_ptr()), ctypes.c_void_p(case.index.data_ptr())
    assert case.lib.dei2i_ema_lerp_dev(*args, None, i, 4, ops._stream()) != 0
    assert case.lib.dei2i_ema_lerp_dev(*args, w, None, 4, ops._stream()) != 0
    assert case.lib.dei2i_ema_lerp_dev(*args, w, i, 0, ops._stream()) != 0
    torch.cuda.synchronize()
    assert same(e, case.e0)
