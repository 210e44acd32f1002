"""``dei2i_diffaug`` (the reduce and apply kernels of csrc/diffaug.hip) driven directly with hand-written record tables, so that what a
seeded draw meets by luck is met on purpose: the float4 fast path (all four lanes taken and ``sx % 4 == 0``) and the per-lane slow
path, quads that straddle the image edge and the hole edge, a hole clipped by each border, everything masked, everything cut, no
hole, the scalar fallback (W % 4 != 0, or a pointer 4 bytes off 16-byte alignment) and the seams of ``chunking()`` (64 chunks at
most).  Every sample of a batch carries another record, so N is also the case table.  All three modes -- forward, its linear part,
the adjoint, each with its own masking rule -- into outputs the test owns (64 sentinel elements on each side).

The float64 reference is the header comment of diffaug.hip (test_elementwise_refs_cpu.diffaug_ref, anchored to the oracle there);
mode 2 is torch.autograd.grad of mode 1's reference, not a second formula.  Colour off (a = 1, b = k = beta = 0) the kernel computes
1 q + 0 mc + 0: bit-equal to the reference for any finite data.  Colour on: 1e-5 max(1, |ref|) per element, the forward test's bound,
in all three modes (the existing gradient tests hold a relative L2 that one wrong border pixel does not move)."""
import ctypes

import numpy as np
import pytest
import torch

import test_elementwise_refs_cpu as R
from test_elementwise_edges_gpu import BAD_ARG, DEV, GUARD, SENTINEL, bits, itype, lib, ptr, stream, sync  # noqa: F401

gpu = pytest.mark.gpu
pytestmark = gpu
F32 = torch.float32


def note(*a):
    print("[diffaug-edges]", *a, flush=True)


class GuardedF32:
    """fp32 output between two sentinel guards; ``off``: the interior starts ``off`` floats past a 16-byte boundary"""

    def __init__(self, numel, off=0):
        self.numel, self.sent, self.lo = numel, SENTINEL["f32"], GUARD + off
        self.flat = torch.full((numel + 2 * GUARD + off,), self.sent, dtype=torch.int32, device=DEV)
        self.ptr = ctypes.c_void_p(self.flat.data_ptr() + 4 * self.lo)
        assert self.ptr.value % 16 == 4 * off

    def interior(self):
        return self.flat[self.lo:self.lo + self.numel]

    def guards_intact(self):
        assert (self.flat[:self.lo] == self.sent).all() and (self.flat[self.lo + self.numel:] == self.sent).all(), "a write outside the tensor"

    def untouched(self):
        self.guards_intact()
        assert (self.interior() == self.sent).all(), "a refused call wrote to its output"

    def values(self, shape):
        self.guards_intact()
        return self.interior().cpu().view(F32).reshape(shape)


def run(lib, mode, src, rec, ch, cw, color, src_off=0, dst_off=0):
    """one dei2i_diffaug call on a CPU fp32 (N, C, H, W) ``src`` -> CPU fp32 output (guards checked)"""
    n, c, h, w = src.shape
    hold = torch.zeros(src.numel() + 8, dtype=F32, device=DEV)
    assert hold.data_ptr() % 16 == 0
    sd = hold[src_off:src_off + src.numel()]
    sd.copy_(src.reshape(-1))
    tab = torch.from_numpy(np.ascontiguousarray(rec)).to(DEV)
    assert tab.shape == (n, 8) and tab.dtype == torch.int32
    partial = torch.full((lib.dei2i_diffaug_partial_floats(n),), float("nan"), dtype=F32, device=DEV) if color else None
    dst = GuardedF32(src.numel(), dst_off)
    assert lib.dei2i_diffaug(mode, n, c, h, w, ch, cw, int(color), ptr(sd), ptr(tab), ptr(partial), dst.ptr, stream()) == 0
    sync()
    return dst.values(src.shape)


def same_bits(got, want64):
    want = want64.float()
    assert torch.equal(want.double(), want64)
    return torch.equal(bits(got), bits(want))


# ---- geometry, colour off: bit-exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GEO_SHAPES, ids=lambda c: "x".join(map(str, c[0])))
def test_geometry_bit_exact_in_all_three_modes(lib, case):
    """randn data (a wrong source pixel shows), one record per sample; (3, 7, 10) and (1, 5, 3) take the scalar kernel (W % 4 != 0)"""
    (c, h, w), hole = case
    for ch, cw, names, rec in R.geo_tables((c, h, w), hole):
        n = len(names)
        x = torch.randn(n, c, h, w, generator=R.gen(11 + h))
        g = torch.randn(n, c, h, w, generator=R.gen(12 + h))
        for mode, src in ((0, x), (1, x), (2, g)):
            got = run(lib, mode, src, rec, ch, cw, 0)
            want = R.diffaug_ref(src.double(), rec, ch, cw, mode, g.double())
            for i, name in enumerate(names):
                assert same_bits(got[i], want[i]), (name, mode, (c, h, w))
            if mode < 2:
                for name in ("ty=H", "tx=-W", "everything_cut"):
                    for i in [i for i, nm in enumerate(names) if nm == name]:
                        assert not bits(got[i]).any(), (name, mode)          # all +0.0


def test_misaligned_pointers_take_the_scalar_path_with_equal_bits(lib):
    (c, h, w), hole = R.GEO_SHAPES[0]
    ch, cw, names, rec = R.geo_tables((c, h, w), hole)[0]
    x = torch.randn(len(names), c, h, w, generator=R.gen(13))
    for mode in (0, 1, 2):
        aligned = run(lib, mode, x, rec, ch, cw, 0)
        assert torch.equal(bits(run(lib, mode, x, rec, ch, cw, 0, src_off=1)), bits(aligned))
        assert torch.equal(bits(run(lib, mode, x, rec, ch, cw, 0, dst_off=1)), bits(aligned))
    # colour on, where the reduce kernel has a scalar form as well: the same sums in another order, so the bound and not the bits
    ch, cw, crec = R.color_records(len(names), h, w)
    xc = R.color_image(len(names), c, h, w)
    for mode in (0, 2):
        want = R.diffaug_ref(xc.double(), crec, ch, cw, mode, xc.double())
        for kw in (dict(src_off=1), dict(dst_off=1)):
            got = run(lib, mode, xc, crec, ch, cw, 1, **kw)
            assert ((got.double() - want).abs() <= 1e-5 * want.abs().clamp(min=1)).all(), (mode, kw)


@pytest.mark.parametrize("case", R.GEO_SHAPES, ids=lambda c: "x".join(map(str, c[0])))
def test_adjoint_is_the_transpose_on_integers(lib, case):
    """<g, mode1(x)> and <mode2(g), x> on integers in [-3, 3], colour off: sums of integer products of the device outputs, summed in
    float64 -- they must be EQUAL, sample by sample, for the whole table"""
    (c, h, w), hole = case
    for ch, cw, names, rec in R.geo_tables((c, h, w), hole):
        n = len(names)
        x = torch.randint(-3, 4, (n, c, h, w), generator=R.gen(21)).float()
        g = torch.randint(-3, 4, (n, c, h, w), generator=R.gen(22)).float()
        y, gx = run(lib, 1, x, rec, ch, cw, 0), run(lib, 2, g, rec, ch, cw, 0)
        lhs = (g.double() * y.double()).sum(dim=(1, 2, 3))
        rhs = (gx.double() * x.double()).sum(dim=(1, 2, 3))
        assert torch.equal(lhs, rhs), [nm for nm, a, b in zip(names, lhs.tolist(), rhs.tolist()) if a != b]
        if "identity" in names:
            assert lhs[names.index("identity")] != 0                   # (the sums are not trivially zero)


# ---- colour on: 1e-5 max(1, |ref|) per element ------------------------------------------------------------------------------------------
def color_check(lib, x, rec, ch, cw, tag):
    g = x                                                              # the cotangent is an image in [0, 1] as well
    worst, worst32 = 0.0, 0.0
    for mode, src in ((0, x), (1, x), (2, g)):
        got = run(lib, mode, src, rec, ch, cw, 1)
        want = R.diffaug_ref(src.double(), rec, ch, cw, mode, g.double())
        cpu32 = R.diffaug_ref(src, rec, ch, cw, mode, g)
        err = (got.double() - want).abs()
        worst, worst32 = max(worst, float(err.max())), max(worst32, float((cpu32.double() - want).abs().max()))
        assert (err <= 1e-5 * want.abs().clamp(min=1)).all(), (tag, mode, float(err.max()))
        if mode == 2:
            # where the adjoint's source is masked the output is k M, M the mean of the MASKED cotangent
            f, geo = R.rec_fields(rec)
            ident = R.records([(1.0, 0.0, 0.0, 0.0) + t for t in geo])
            hh = R.diffaug_ref(g.double(), ident, ch, cw, 2, g.double())
            reach = R.diffaug_ref(g.double(), ident, ch, cw, 2, torch.ones_like(g).double())
            kM = (f[:, 2].double().view(-1, 1, 1, 1) * hh.mean(dim=(1, 2, 3), keepdim=True)).expand_as(want)
            assert ((got.double() - kM)[reach == 0].abs() <= 1e-5).all(), (tag, "masked pixels of the adjoint")
    note(f"{tag}: kernel max |err| {worst:.3e}, fp32 CPU {worst32:.3e} (bound 1e-5 max(1, |ref|))")


@pytest.mark.parametrize("seam", R.COLOR_SEAMS, ids=lambda s: f"N{s[0]}-H{s[1]}")
def test_color_at_the_chunking_seams(lib, seam):
    # One row dropped from (or doubled in) the reduce moves mean_chw by about 0.5 / H and the output by |k| 0.5 / H = 0.25 / H at |k| = 0.5:
    #   H = 1: the whole mean (0.25); H = 64: 3.9e-3; H = 65: 3.8e-3; H = 70: 3.6e-3; H = 4: 6.3e-2 -- 360x the 1e-5 bound at the least.
    n, h = seam
    assert 0.25 / h >= 1e-3
    for first in (range(3) if n == 1 else [0]):                       # a single sample: once per geometry record, each with |k| = 0.5
        ch, cw, rec = R.color_records(n, h, R.COLOR_W, first)
        color_check(lib, R.color_image(n, 3, h, R.COLOR_W), rec, ch, cw, f"diffaug colour N = {n} H = {h} chunks = {R.chunking(n, h)[1]}")


@pytest.mark.parametrize("c", R.COLOR_CHANNELS)
def test_color_by_channel_count(lib, c):
    n, h, w = 81, 6, 12                                               # every colour corner with every geometry record; W % 4 == 0
    ch, cw, rec = R.color_records(n, h, w)
    color_check(lib, R.color_image(n, c, h, w), rec, ch, cw, f"diffaug colour C = {c} (81 records, 6 x 12)")
    ch, cw, rec = R.color_records(n, 5, 7)                            # and the scalar kernels
    color_check(lib, R.color_image(n, c, 5, 7), rec, ch, cw, f"diffaug colour C = {c} (81 records, 5 x 7, scalar)")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(lib):
    n, c, h, w = 2, 3, 4, 8
    src = torch.rand(n, c, h, w, device=DEV)
    tab = torch.from_numpy(R.color_records(n, h, w)[2]).to(DEV)
    partial = torch.zeros(lib.dei2i_diffaug_partial_floats(n), dtype=F32, device=DEV)
    ok = dict(mode=0, n=n, ch=2, cw=4, color=1, src=src, tab=tab, partial=partial)
    for change in (dict(mode=3), dict(mode=-1), dict(n=0), dict(ch=-1), dict(cw=-1), dict(tab=None), dict(src=None), dict(partial=None)):
        a = dict(ok, **change)
        dst = GuardedF32(src.numel())
        rc = lib.dei2i_diffaug(a["mode"], a["n"], c, h, w, a["ch"], a["cw"], a["color"], ptr(a["src"]), ptr(a["tab"]), ptr(a["partial"]),
                               dst.ptr, stream())
        assert rc == BAD_ARG, change
        sync()
        dst.untouched()
    assert lib.dei2i_diffaug(0, n, c, h, w, 2, 4, 1, ptr(src), ptr(tab), ptr(partial), None, stream()) == BAD_ARG
    dst = GuardedF32(src.numel())                                     # colour off needs no partial buffer
    assert lib.dei2i_diffaug(0, n, c, h, w, 2, 4, 0, ptr(src), ptr(tab), None, dst.ptr, stream()) == 0
    sync()
    dst.guards_intact()
