"""The host-side caches of the hot path, the part that needs no GPU: the facts of torch their keys rest on, the keys' own logic, and
the integer cases tests/test_host_caches_gpu.py runs (DESIGN.md section 4 has the table of caches, keys and writers).

Almost every host-side speed-up of ops.py, optim.py, networks/architecture.py and models/defectgan_model.py memoises on tensor
identity, the autograd version counter or the hand-written ``_dei2i_epoch`` stamp (``ops.mark_written``).  A cache that misses an
invalidation does not crash: it feeds a correct kernel the operand of an earlier call.  This file pins

* which writes move ``Tensor._version`` and which do not (a torch upgrade that changes the table fails here, not in training),
* that ``BaseNetwork.init_weights`` -- which writes through ``.data`` -- stamps what it wrote,
* the hand-over attributes of activations (``_dei2i_stats``, ``_dei2i_fp8``) against an in-place write, on host tensors,
* ``_NormBwdHint.take``, ``DefectGanModel._paired_label_sets``, ``SPADE._table_key`` / ``_class_table`` (the table convs stubbed out),
  the ``> 4096`` clear of ``ops._descs`` and the ``> 16`` clear of ``ops._zero_tables``,
* the POWER CONDITION of the integer cases of the GPU file, for the seeds it uses: x, dy and both weight sets W0, W1 are drawn from
  {-1, 0, 1}, every sum is an exact small integer (|y|, |dx| <= 256, |dw| < 2^24), and the float64 references on W0 and on W1 differ
  in at least half of their elements -- a kernel served W0's packed copy cannot pass by accident.
"""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from helpers import load_golden, make_opt

# ---- the integer cases shared with tests/test_host_caches_gpu.py -------------------------------------------------------------
# name -> (N, cin, cout, k, pad, H, W, density of x, density of dy); zero padding, stride 1
INT_CASES = {
    "plain": (2, 16, 16, 3, 1, 8, 8, 1.0, 1.0),                # the smallest conv that reaches the packed layouts: K = 144
    "splitk": (2, 24, 72, 3, 1, 6, 10, 1.0, 1.0),              # test_conv_exact_gpu.py's a-nk4-co72: gather_v1 with split-K
    "grow": (1, 256, 256, 3, 1, 16, 20, 0.25, 0.25),           # 16 slabs of 320 x 256 outputs: more than the 4 MB a slot starts with
}
Y_MAX, DW_MAX = 256, 2 ** 24                                    # test_conv_exact_gpu.py's bounds


def ints(shape, seed, density=1.0):
    """fp32 tensor of values from {-1, 0, 1}, uniform, thinned to ``density``"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-1, 2, shape, generator=g).float()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density).float()
    return t


def differ(a, b):
    """share of the elements in which two references differ"""
    return (a != b).double().mean().item()


@functools.lru_cache(maxsize=None)
def integer_case(name):
    """-> dict(x, gy, W0, W1 fp32 NCHW / OIHW; y0, dx0, y1, dx1, dw float64 references) of one integer case, the conditions that
    make bit-equality the right comparison and the power condition asserted on the references.  Computed once, never modified."""
    n, cin, cout, k, pad, h, w, dx_, dy_ = INT_CASES[name]
    seed = 1000 * (1 + sorted(INT_CASES).index(name))
    x, gy = ints((n, cin, h, w), seed, dx_), ints((n, cout, h + 2 * pad - k + 1, w + 2 * pad - k + 1), seed + 1, dy_)
    out = dict(x=x, gy=gy, W0=ints((cout, cin, k, k), seed + 2), W1=ints((cout, cin, k, k), seed + 3))
    for i in (0, 1):
        xr, wr = x.double().requires_grad_(True), out[f"W{i}"].double().requires_grad_(True)
        y = F.conv2d(xr, wr, padding=pad)
        dx, dw = torch.autograd.grad(y, [xr, wr], gy.double())
        assert y.abs().max() <= Y_MAX and dx.abs().max() <= Y_MAX and dw.abs().max() < DW_MAX, name
        out[f"y{i}"], out[f"dx{i}"] = y.detach(), dx
        assert i == 0 or torch.equal(dw, out["dw"])              # (dw is linear in x and dy alone: no weight in it)
        out["dw"] = dw
    # the power condition: a result computed from W0's packed copies is wrong in at least half of its elements
    assert differ(out["y0"], out["y1"]) >= 0.5 and differ(out["dx0"], out["dx1"]) >= 0.5, name
    return out


@pytest.mark.parametrize("name", sorted(INT_CASES))
def test_integer_cases_are_exact_and_discriminate(name):
    c = integer_case(name)
    share = differ(c["y0"], c["y1"]), differ(c["dx0"], c["dx1"])
    print(f"[host-caches] {name}: max |y| {c['y1'].abs().max().item():.0f}, max |dx| {c['dx1'].abs().max().item():.0f}, "
          f"max |dw| {c['dw'].abs().max().item():.0f}; W0 / W1 references differ in {share[0]:.3f} (y), {share[1]:.3f} (dx)")
    assert min(share) >= 0.5
    assert differ(c["W0"], c["W1"]) >= 0.5


# ---- C. facts of torch the stamps rest on ---------------------------------------------------------------------------------------
def _stamp(t):
    from de_i2i_gan_amd import ops
    return ops.PackedWeights._stamp(t)


def test_writes_that_move_the_version_counter():
    w = torch.nn.Parameter(torch.zeros(4, 3))
    assert w._version == 0
    with torch.no_grad():
        w.mul_(2)
    assert w._version == 1                                                     # an in-place op under no_grad
    lin = torch.nn.Linear(3, 2)
    before = lin.weight._version
    lin.load_state_dict({"weight": torch.ones(2, 3), "bias": torch.ones(2)})
    assert lin.weight._version > before                                        # load_state_dict
    before = lin.weight._version
    lin.weight.grad = torch.ones(2, 3)
    torch.optim.Adam([lin.weight], lr=0.5).step()
    assert lin.weight._version > before                                        # torch.optim.Adam.step
    before = lin.weight._version
    torch.optim.SGD([lin.weight], lr=0.5).step()
    assert lin.weight._version > before                                        # torch.optim.SGD.step
    before = w._version
    w.detach().add_(1)
    assert w._version == before + 1                                            # an in-place op on w.detach(): the counter is shared


def test_writes_through_data_move_nothing():
    """The hole init_weights fell into: ``.data`` is a detached alias with a version counter of its own."""
    w = torch.nn.Parameter(torch.zeros(4, 3))
    stamp = _stamp(w)
    torch.nn.init.normal_(w.data, 0.0, 0.5)
    w.data.add_(1)
    w.data.copy_(torch.ones(4, 3))
    assert w._version == 0 and _stamp(w) == stamp and w.eq(1).all()


def test_assigning_data_moves_the_pointer_and_not_the_version():
    w = torch.nn.Parameter(torch.zeros(4, 3))
    ptr, new = w.data_ptr(), torch.ones(4, 3)
    w.data = new
    assert w.data_ptr() == new.data_ptr() != ptr and w._version == 0
    assert _stamp(w)[0] == new.data_ptr()


def test_mark_written_adds_exactly_one_to_the_epoch():
    from de_i2i_gan_amd import ops
    a, b = torch.nn.Parameter(torch.zeros(3)), torch.zeros(2)
    assert _stamp(a)[2] == 0
    ops.mark_written(a, b)
    assert (a._dei2i_epoch, b._dei2i_epoch) == (1, 1) and _stamp(a) == (a.data_ptr(), 0, 1)
    ops.mark_written(a)
    assert (a._dei2i_epoch, b._dei2i_epoch) == (2, 1) and a._version == 0


@pytest.mark.parametrize("net", ["generator", "discriminator"])
@pytest.mark.parametrize("init_type", ["normal", "xavier", "none"])
def test_init_weights_moves_the_stamp_of_everything_it_wrote(net, init_type):
    """Hole 1 in its CPU form: a network that ran a forward and is then (re-)initialised must not keep its packed copies.  Every
    parameter whose VALUES init_weights changed carries another ``PackedWeights._stamp`` afterwards -- and so another
    ``SPADE._table_key`` -- and every conv weight is among them."""
    from de_i2i_gan_amd.networks.discriminator import DefectGanDiscriminator
    from de_i2i_gan_amd.networks.generator import DefectGanGenerator
    _, _, c, _ = load_golden("t0_img32_b2")
    torch.manual_seed(3)
    model = (DefectGanGenerator if net == "generator" else DefectGanDiscriminator)(make_opt(c, "cpu"))
    before = {k: (p.detach().clone(), _stamp(p)) for k, p in model.named_parameters()}
    keys = [m._table_key(torch.zeros(1, 6, 1, 1), _prec()) for m in model.modules() if hasattr(m, "_table_key")]
    model.init_weights(init_type, 0.5)
    wrote = [k for k, p in model.named_parameters() if not torch.equal(p.detach(), before[k][0])]
    assert {k for k, p in model.named_parameters() if p.dim() == 4} <= set(wrote)
    stale = [k for k, p in model.named_parameters() if k in wrote and _stamp(p) == before[k][1]]
    assert not stale, f"{len(stale)} of {len(wrote)} written parameters kept their stamp, e.g. {stale[:4]}"
    seg = torch.zeros(1, 6, 1, 1)
    mods = [m for m in model.modules() if hasattr(m, "_table_key")]
    assert len(mods) == len(keys) and (net == "discriminator" or mods)
    for m, old in zip(mods, keys):
        assert m._table_key(seg, _prec())[2:] != old[2:]                       # (position 0 is the id of the label tensor)


def _prec():
    from de_i2i_gan_amd import ops
    return ops.BF16


# ---- hand-over attributes of activations ----------------------------------------------------------------------------------------
def _handed_over(shape=(2, 4, 4, 8), chunks=1):
    """a host tensor carrying statistics records the way a producer's public wrapper leaves them"""
    from de_i2i_gan_amd import ops
    y = torch.arange(2 * 4 * 4 * 8, dtype=torch.float32).reshape(shape)
    partial = torch.zeros(shape[0], chunks, 2, shape[-1])
    ops._handover.clear()
    ops._handover["_dei2i_stats"] = (partial, chunks)
    assert ops._attach(y) is y and not ops._handover
    return y, partial


def test_statistics_records_are_read_while_the_tensor_is_as_its_producer_wrote_it():
    from de_i2i_gan_amd import ops
    y, partial = _handed_over()
    have = ops._stats_of(y, 2, 16, 8)
    assert have is not None and have[0] is partial and have[1] == 1
    assert y.contiguous() is y and ops._stats_of(y.contiguous(), 2, 16, 8) is not None     # a no-op: the same tensor, the same data
    assert ops._stats_of(y, 2, 16, 16) is None and ops._stats_of(y, 3, 16, 8) is None      # records of another shape


@pytest.mark.parametrize("write", ["mul_", "add_", "copy_", "detach_mul_", "view_mul_"])
def test_statistics_records_are_ignored_after_an_in_place_write(write):
    """Hole 2 in its CPU form: the records describe a tensor that no longer exists."""
    from de_i2i_gan_amd import ops
    y, _ = _handed_over()
    if write == "mul_":
        y.mul_(2)
    elif write == "add_":
        y.add_(torch.ones_like(y))
    elif write == "copy_":
        y.copy_(torch.ones_like(y))
    elif write == "detach_mul_":
        y.detach().mul_(2)                       # (shares the version counter)
    else:
        y[:1].mul_(2)                            # through a view of a part
    assert ops._stats_of(y, 2, 16, 8) is None


def test_views_and_copies_do_not_inherit_the_records():
    from de_i2i_gan_amd import ops
    y, _ = _handed_over()
    for other in (y[:], y.view(2, 4, 4, 8), y.clone(), y.detach(), y * 1):
        assert other is not y and ops._stats_of(other, 2, 16, 8) is None
    assert ops._stats_of(y, 2, 16, 8) is not None


def test_the_fp8_copy_is_bound_to_the_version_too():
    from de_i2i_gan_amd import ops
    y = torch.zeros(2, 4, 4, 8)
    ops._handover.clear()
    ops._handover["_dei2i_fp8"] = xq = torch.zeros(y.numel(), dtype=torch.uint8)
    ops._attach(y)
    assert ops._handed(y, "_dei2i_fp8") is xq and ops._handed(y, "_dei2i_stats") is None
    y.add_(1)
    assert ops._handed(y, "_dei2i_fp8") is None
    plain = torch.zeros(3)
    assert ops._attach(plain) is plain and not hasattr(plain, "_dei2i_at_version")           # nothing handed over: nothing attached


# ---- _NormBwdHint.take ------------------------------------------------------------------------------------------------------
def _hint():
    from de_i2i_gan_amd import ops
    x = torch.zeros(2, 4, 4, 8)
    hint = ops._NormBwdHint(2, x, torch.zeros(1, 8), torch.ones(1, 8), a=torch.ones(1, 8), b=torch.zeros(1, 8))
    dz, partial = torch.ones(2, 4, 4, 8), torch.zeros(2, 3, 2, 8)
    hint.give(partial, 3, dz)
    return hint, dz, partial


def _dropped(hint):
    return hint.partial is None and hint.chunks is None and hint.dz is None and hint.dz_version is None


def test_hint_take_returns_the_records_for_the_very_dz():
    from de_i2i_gan_amd import ops
    hint, dz, partial = _hint()
    taken = ops.bwd_fused_counts["taken"]
    got = hint.take(dz)
    assert got is not None and got[0] is partial and got[1] == 3 and ops.bwd_fused_counts["taken"] == taken + 1
    assert _dropped(hint)
    assert hint.take(dz) is None and _dropped(hint)                           # a second take: one consumer only


@pytest.mark.parametrize("case", ["bumped", "other", "strided", "never_given"])
def test_hint_take_refuses_every_other_dz(case):
    from de_i2i_gan_amd import ops
    hint, dz, _ = _hint()
    taken = ops.bwd_fused_counts["taken"]
    if case == "bumped":
        dz.add_(1)                                                            # same storage, autograd added a second gradient into it
        asked = dz
    elif case == "other":
        asked = torch.ones(2, 4, 4, 8)                                        # equal shape and content, another tensor
    elif case == "strided":
        big = torch.ones(2, 4, 4, 16)
        hint.give(hint.partial, 3, big[..., ::2])
        asked = big[..., ::2]                                                 # the tensor given, but not contiguous
        assert not asked.is_contiguous()
    else:
        hint.drop()
        asked = dz
    assert hint.take(asked) is None and _dropped(hint) and ops.bwd_fused_counts["taken"] == taken


# ---- DefectGanModel._paired_label_sets ------------------------------------------------------------------------------------------
def test_paired_label_sets_are_memoised_per_label_tensor_and_version():
    from de_i2i_gan_amd.models.defectgan_model import DefectGanModel
    me = SimpleNamespace()
    sets = lambda lab, nm, df: DefectGanModel._paired_label_sets(me, lab, nm, df)          # noqa: E731 (it only concatenates)
    labels = torch.tensor([[0., 1., 0.], [0., 0., 1.]])
    nm, df = torch.zeros(2, 3, 1, 1), labels.view(2, 3, 1, 1).clone()
    head, tail, same = sets(labels, nm, df)
    assert not same and torch.equal(head, torch.cat([df, nm])) and torch.equal(tail, torch.cat([nm, df]))
    head2, tail2, same = sets(labels, nm, df)
    assert same and head2 is head and tail2 is tail                            # the very tensors: the SPADE tables are keyed on them
    labels[0, 0] = 1.0                                                         # an in-place change (a graph replay copies into it)
    df2 = labels.view(2, 3, 1, 1).clone()
    head3, tail3, same = sets(labels, nm, df2)
    assert not same and head3 is not head and torch.equal(head3, torch.cat([df2, nm])) and torch.equal(tail3, torch.cat([nm, df2]))
    twin = labels.clone()                                                      # another tensor of equal content
    head4, _, same = sets(twin, nm, df2)
    assert not same and head4 is not head3
    assert sets(twin, nm, df2)[2] and not sets(labels, nm, df2)[2]             # one slot: the last tensor only
    me._label_sets = None                                                      # what graph_step's capture does
    assert not sets(labels, nm, df2)[2]


# ---- SPADE._table_key / _class_table, the table convs stubbed ---------------------------------------------------------------------
@pytest.fixture
def spade(monkeypatch):
    from de_i2i_gan_amd.networks.architecture import SPADE
    torch.manual_seed(5)
    m = SPADE(label_nc=6, norm_nc=16, hidden_nc=8)
    calls = []

    def gamma_beta(segmap, prec, class_mode, h, w, seg=None, actv=None):
        calls.append(segmap)
        out = torch.full((segmap.shape[0], 5, 5, 32), float(len(calls)))
        return out.requires_grad_(True) * 1 if torch.is_grad_enabled() else out
    monkeypatch.setattr(m, "_gamma_beta", gamma_beta)
    m.calls = calls
    return m


def _labels(seed, n=2):
    lab = torch.zeros(n, 6, 1, 1)
    for j in range(n):
        lab[j, (seed + j) % 6] = 1
    return lab


def test_spade_table_key_moves_with_every_writer(spade):
    from de_i2i_gan_amd import ops
    lab = _labels(0)
    key = spade._table_key(lab, ops.BF16)
    assert spade._table_key(lab, ops.BF16) == key
    assert spade._table_key(lab, ops.F32) != key                               # precision
    with torch.no_grad():
        assert spade._table_key(lab, ops.BF16) != key                          # grad mode
        assert spade._table_key(lab, ops.BF16, grad=True) == key
    assert spade._table_key(_labels(0), ops.BF16) != key                       # another tensor of equal content
    lab.copy_(_labels(1))
    moved = spade._table_key(lab, ops.BF16)
    assert moved != key and moved[0] == key[0]                                 # an in-place label change: the version
    for p in spade.parameters():
        k0 = spade._table_key(lab, ops.BF16)
        ops.mark_written(p)                                                    # a raw-pointer writer (FusedAdam)
        k1 = spade._table_key(lab, ops.BF16)
        assert k1 != k0, "a parameter that is not part of the key"
        with torch.no_grad():
            p.mul_(1.0)                                                        # a torch writer
        assert spade._table_key(lab, ops.BF16) != k1
    k0 = spade._table_key(lab, ops.BF16)
    spade.mlp_gamma.weight.requires_grad_(False)
    assert spade._table_key(lab, ops.BF16) != k0                               # a table without history must not serve a trained pass


def test_spade_class_table_hits_and_misses(spade):
    from de_i2i_gan_amd import ops
    lab, other = _labels(0), _labels(3)
    t1 = spade._class_table(lab, ops.BF16, 8, 8)
    assert spade._class_table(lab, ops.BF16, 8, 8) is t1 and len(spade.calls) == 1          # the same label tensor: a hit
    with torch.no_grad():
        assert spade._class_table(lab, ops.BF16, 8, 8) is t1 and len(spade.calls) == 1      # no-grad after grad: the grad table serves
    lab.copy_(other)
    t2 = spade._class_table(lab, ops.BF16, 8, 8)
    assert t2 is not t1 and len(spade.calls) == 2                                           # in-place label change: a miss
    ops.mark_written(spade.mlp_beta.bias)
    t3 = spade._class_table(lab, ops.BF16, 8, 8)
    assert t3 is not t2 and len(spade.calls) == 3                                           # a parameter written through raw pointers
    fresh = _labels(4)
    with torch.no_grad():
        t4 = spade._class_table(fresh, ops.BF16, 8, 8)
    assert len(spade.calls) == 4 and not t4.requires_grad
    t5 = spade._class_table(fresh, ops.BF16, 8, 8)
    assert t5 is not t4 and t5.requires_grad and len(spade.calls) == 5                      # grad after no-grad: needs its own history


def test_spade_cache_holds_the_label_tensor_so_its_id_stays_unique(spade):
    from de_i2i_gan_amd import ops
    lab = _labels(0)
    spade._class_table(lab, ops.BF16, 8, 8)
    old_id = id(lab)
    del lab
    assert [id(seg) for seg, _ in spade._gb_cache.values()] == [old_id]
    later = [_labels(0) for _ in range(64)]                                    # allocated while the cache holds the old one
    assert all(id(t) != old_id for t in later)
    spade._class_table(later[0], ops.BF16, 8, 8)
    assert len(spade.calls) == 2


def test_spade_prime_serves_the_single_calls(spade):
    from de_i2i_gan_amd import ops
    a, b = _labels(0), _labels(2, n=3)
    assert spade.wants_prime((a, b), ops.BF16)
    spade.prime((a, b), ops.BF16)
    assert len(spade.calls) == 1 and spade.calls[0].shape[0] == 5              # one pass over the concatenation
    ta, tb = spade._class_table(a, ops.BF16, 8, 8), spade._class_table(b, ops.BF16, 8, 8)
    assert len(spade.calls) == 1 and ta.shape[0] == 2 and tb.shape[0] == 3
    assert not spade.wants_prime((a, b), ops.BF16)
    a.copy_(_labels(1))
    assert spade.wants_prime((a, b), ops.BF16)                                 # a changed label tensor: prime again


# ---- the small process-wide tables ------------------------------------------------------------------------------------------------
def test_descriptor_cache_survives_its_own_clear():
    """ops._descs is cleared when it passes 4096 entries; a descriptor handed out before the clear is still the caller's (ctypes
    structures are Python objects: the clear only drops the cache's reference)."""
    from de_i2i_gan_amd import ops
    saved = dict(ops._descs)
    try:
        ops._descs.clear()
        g = ops.ConvGeom(16, 24, 3, 1, 1, True, False)
        first = ops._desc(ops.BF16, g, 2, 8, 12, 16, 24)
        assert ops._desc(ops.BF16, g, 2, 8, 12, 16, 24) is first
        for n in range(1, 4200):
            d = ops._desc(ops.F32, g, n, 7, 9, 16, 24)
            assert (d.dtype, d.N, d.H, d.W) == (ops.F32.code, n, 7, 9)
        assert len(ops._descs) < 4096, "the cache was never cleared"
        fields = [getattr(first, name) for name, _ in first._fields_]
        assert fields == [ops.BF16.code, 2, 8, 12, 16, 24, 16, 24, 3, 3, 1, 1, 1, 0]
        again = ops._desc(ops.BF16, g, 2, 8, 12, 16, 24)
        assert again is not first and [getattr(again, name) for name, _ in again._fields_] == fields
    finally:
        ops._descs.clear()
        ops._descs.update(saved)


def test_zero_tables_and_constant_vectors_key_on_everything_they_depend_on():
    from de_i2i_gan_amd import ops
    saved, saved_c = dict(ops._zero_tables), dict(ops._const_vecs)
    try:
        ops._zero_tables.clear()
        first = ops._zero_table("cpu", torch.float32, 2, 8)
        assert ops._zero_table("cpu", torch.float32, 2, 8) is first and first.shape == (2, 5, 5, 16)
        assert ops._zero_table("cpu", torch.bfloat16, 2, 8).dtype == torch.bfloat16
        for c in range(9, 40):
            t = ops._zero_table("cpu", torch.float32, 3, c)
            assert t.shape == (3, 5, 5, 2 * c) and not t.any()
        assert len(ops._zero_tables) <= 17, "the cache was never cleared"
        assert not first.any() and ops._zero_table("cpu", torch.float32, 2, 8).shape == first.shape
        one, half = ops._const_vec("cpu", 8, 1.0), ops._const_vec("cpu", 8, 0.5)
        assert ops._const_vec("cpu", 8, 1.0) is one and one.eq(1).all() and half.eq(0.5).all()
        assert ops._const_vec("cpu", 16, 1.0).shape == (16,)
    finally:
        ops._zero_tables.clear()
        ops._zero_tables.update(saved)
        ops._const_vecs.clear()
        ops._const_vecs.update(saved_c)
