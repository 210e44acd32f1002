"""The kernels of csrc/adam.hip (Adam / AdamW in four forms, SGD, RMSprop, the EMA lerp) at the seams the small round shapes of
test_ops_gpu.py / test_adam_dev_gpu.py do not reach, one step from a pre-set state against the header comment's formula in float64.

Seams: Adam's grid is min(512, ceil(n / 4 / 256)) workgroups of 256 threads of float4 -- the grid-stride trip runs for
n > 524 288 --, followed by the scalar tail of the n % 4 last elements, and the whole tensor takes the scalar loop (n4 = 0) when any
of p, g, m, v is not 16-byte aligned; SGD / RMSprop cap at 2048 workgroups (n > 524 288), the EMA lerp at 1024 (n > 262 144) and its
formula switches at |w| = 0.5; the ``_dev`` forms read row ``*index`` of a hyper-parameter table and leave everything untouched for
an index outside [0, rows).

Tolerances (DESIGN.md section 4 has the measured values).  With u = 2^-24 the unit
roundoff of fp32, every output is bounded ELEMENTWISE by k * u * S: S the sum of the magnitudes of the terms the formula combines,
k the number of roundings on the longest path to the output -- a correctly rounded operation counts 1, ``sqrtf`` and a division 2
(1 ulp allowed), a fused multiply-add only removes roundings.  m and v are compared with the formula on the INPUTS, p with the formula
on the inputs and the m, v the same run produced ("separately"), so each k counts its own formula only.  A plain fp32 restatement
on the CPU (torch ops, one rounding each, the kernel's order) has to pass the same bounds: they are neither vacuous nor too tight."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
T_STEP = 7
SIZES = [1, 2, 3, 4, 5, 1023, 524288, 524288 + 4 * 256 + 3]      # the last: a second grid-stride trip of 256 float4 + a 3-element tail
FORMS = ["adam", "adam_l2", "adam_dev", "adam_l2_dev", "sgd", "rmsprop"]

# roundings per output (see the module docstring), gv = g * grad_scale [+ wd * p]: 1 [3] roundings
#   m' = m + (1 - b1) * (gv - m)                  gv, sub, mul, add                           (1 - b1, 1 - b2 are exact: Sterbenz)
#   v' = b2 * v + (1 - b2) * gv * gv              gv twice, two products, b2 * v, add
#   p' = p * keep - (lr / c1) * (m' / (sqrt(v') * (1 / c2) + eps))
#        sqrt 2, 1 / c2 2, product 1, + eps 1, m' / denom 2, lr / c1 2, product 1, final sub 1 = 12 on the update term;
#        keep = 1 - lr * wd (2, host) and p * keep (1) and the sub (1) = 4 on the p term -- k = 12 covers both
#   sgd     p' = p - lr * gv                      gv, product, sub
#   rmsprop sq' = alpha * sq + (1 - alpha) gv gv  as v';   p' = p - lr * (gv / (sqrt(sq') + eps)): gv 1, sqrt 2, + eps 1, div 2, product 1, sub 1
K_ROUND = {"adam": dict(m=4, v=6, p=12), "adam_l2": dict(m=6, v=10, p=12), "sgd": dict(p=3), "rmsprop": dict(m=6, p=8)}
# ema: start + w * diff: diff, product, add = 3;  end - diff * (1 - w): diff, 1 - w, product, sub = 4
K_EMA = {False: 3, True: 4}


def note(*a):
    print("[optim-edges]", *a, flush=True)


def f32(x):
    return float(np.float32(x))


@pytest.fixture(scope="module")
def lib():
    from de_i2i_gan_amd import _lib as L
    from de_i2i_gan_amd import ops
    ops._lib_for(torch.empty(1, device=DEV))
    return L.load()


def stream():
    from de_i2i_gan_amd import ops
    return ops._stream()


def hyper_of(form):
    """The scalar arguments as the fp32 values the C ABI receives (ctypes rounds a Python float to c_float)"""
    b1, b2 = 0.5, 0.999
    h = dict(lr=f32(1e-2), b1=f32(b1), b2=f32(b2), eps=f32(1e-8), c1=f32(1.0 - b1 ** T_STEP), c2=f32(math.sqrt(1.0 - b2 ** T_STEP)),
             gs=0.5, wd=f32(3e-2), alpha=f32(0.99))
    h["coupled"] = form.startswith("adam_l2")
    return h


@pytest.fixture(scope="module")
def state():
    """One set of fp32 inputs (p, g, m, v per size) shared by every form: m random, v random >= 0"""
    gen = torch.Generator().manual_seed(11)
    out = []
    for n in SIZES:
        out.append((torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.3,
                    torch.rand(n, generator=gen) * 1.5))
    return out


def table(ps, gs, ms, vs):
    rows = [(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()) for p, g, m, v in zip(ps, gs, ms, vs)]
    return torch.tensor(rows, dtype=torch.int64).to(DEV), max(r[4] for r in rows)


# ---- the formula: float64 = the reference, float32 = the CPU restatement ------------------------------------------------
def scalars(h, dt, keep_row=None):
    """Derived scalars in the arithmetic of ``dt``; keep: the host's 1.f - lr * wd for the argument form, the table's value for
    the ``_dev`` form (``keep_row``), 1 for coupled decay"""
    c = np.float64 if dt == torch.float64 else np.float32
    one = c(1)
    if h["coupled"]:
        keep = one
    elif keep_row is not None:
        keep = c(keep_row)
    else:
        keep = one - c(h["lr"]) * c(h["wd"])
    return dict(a1=one - c(h["b1"]), a2=one - c(h["b2"]), step=c(h["lr"]) / c(h["c1"]), inv_c2=one / c(h["c2"]), keep=keep,
                aa=one - c(h["alpha"]))


def adam_mv(p, g, m, v, h, dt, keep_row=None):
    s = scalars(h, dt, keep_row)
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    gv = g * h["gs"] + h["wd"] * p if h["coupled"] else g * h["gs"]
    m1 = m + float(s["a1"]) * (gv - m)
    v1 = h["b2"] * v + float(s["a2"]) * gv * gv
    G = g.abs() * h["gs"] + (h["wd"] * p.abs() if h["coupled"] else 0)
    return m1, v1, m.abs() + float(s["a1"]) * (G + m.abs()), h["b2"] * v.abs() + float(s["a2"]) * G * G


def adam_p(p, m1, v1, h, dt, keep_row=None):
    s = scalars(h, dt, keep_row)
    p, m1, v1 = p.to(dt), m1.to(dt), v1.to(dt)
    denom = v1.sqrt() * float(s["inv_c2"]) + h["eps"]
    upd = float(s["step"]) * (m1 / denom)
    return p * float(s["keep"]) - upd, p.abs() * float(s["keep"]) + upd.abs()


def plain_sq(g, m, h, dt):
    s = scalars(h, dt)
    g, m = g.to(dt), m.to(dt)
    gv = g * h["gs"]
    return h["alpha"] * m + float(s["aa"]) * gv * gv, h["alpha"] * m.abs() + float(s["aa"]) * gv * gv


def plain_p(p, g, sq1, h, dt, kind):
    p, g = p.to(dt), g.to(dt)
    gv = g * h["gs"]
    upd = h["lr"] * gv if kind == 0 else h["lr"] * (gv / (sq1.to(dt).sqrt() + h["eps"]))
    return p - upd, p.abs() + upd.abs()


def worst(got, ref, S):
    """max over the elements of |got - ref| / (u * S): the error in units of one rounding of the combined magnitudes"""
    assert torch.isfinite(got).all() and torch.isfinite(ref).all()
    S = S.clamp_min(1e-300)
    return ((got.double() - ref).abs() / (U * S)).max().item()


def check_adam(tag, inp, out, h, worst_of, keep_row=None):
    """out = (p', m', v') of one run (kernel or fp32 CPU) on inp = (p, g, m, v), all CPU tensors"""
    p, g, m, v = inp
    k = K_ROUND["adam_l2" if h["coupled"] else "adam"]
    m_ref, v_ref, S_m, S_v = adam_mv(p, g, m, v, h, torch.float64, keep_row)
    p_ref, S_p = adam_p(p, out[1], out[2], h, torch.float64, keep_row)
    for name, got, ref, S in (("m", out[1], m_ref, S_m), ("v", out[2], v_ref, S_v), ("p", out[0], p_ref, S_p)):
        e = worst(got, ref, S)
        worst_of[name] = max(worst_of.get(name, 0.0), e)
        assert e <= k[name], (tag, name, p.numel(), e, k[name])       # |got - ref| <= k * 2^-24 * S, every element


def cpu_adam(inp, h, keep_row=None):
    p, g, m, v = inp
    m1, v1, _, _ = adam_mv(p, g, m, v, h, torch.float32, keep_row)
    p1, _ = adam_p(p, m1, v1, h, torch.float32, keep_row)
    return p1, m1, v1


def hyper_table(h, rows, live):
    """(rows, 4) fp32 rows (lr, c1, c2, keep), every row different; row ``live`` holds h's values"""
    tab = np.empty((rows, 4), dtype=np.float32)
    for r in range(rows):
        tab[r] = (h["lr"] * (1 + 0.25 * (r - live)), h["c1"] * (1 + 0.01 * (r - live)), h["c2"] * (1 + 0.02 * (r - live)),
                  np.float32(1) - np.float32(h["lr"]) * np.float32(h["wd"]) * np.float32(1 + r - live))
    return tab


def launch(lib, form, tab, count, max_n, h, hyper=None, index=None, rows=0):
    t = ctypes.c_void_p(tab.data_ptr())
    if form == "adam":
        rc = lib.dei2i_adam_step(t, count, max_n, h["lr"], h["b1"], h["b2"], h["eps"], h["c1"], h["c2"], h["gs"], h["wd"], stream())
    elif form == "adam_l2":
        rc = lib.dei2i_adam_step_l2(t, count, max_n, h["lr"], h["b1"], h["b2"], h["eps"], h["c1"], h["c2"], h["gs"], h["wd"], stream())
    elif form == "adam_dev":
        rc = lib.dei2i_adam_step_dev(t, count, max_n, ctypes.c_void_p(hyper.data_ptr()), ctypes.c_void_p(index.data_ptr()), rows,
                                     h["b1"], h["b2"], h["eps"], h["gs"], stream())
    elif form == "adam_l2_dev":
        rc = lib.dei2i_adam_step_l2_dev(t, count, max_n, ctypes.c_void_p(hyper.data_ptr()), ctypes.c_void_p(index.data_ptr()), rows,
                                        h["b1"], h["b2"], h["eps"], h["gs"], h["wd"], stream())
    else:
        rc = lib.dei2i_sgd_rmsprop_step(t, count, max_n, 0 if form == "sgd" else 1, h["lr"], h["alpha"], h["eps"], h["gs"], stream())
    assert rc == 0, (form, rc)


def run_form(lib, form, inputs, h, rows=3, live=1):
    """One launch over a table of ``inputs`` (CPU (p, g, m, v) tuples) -> CPU (p', m', v') per tensor and the table's keep value"""
    dev = [[t.to(DEV) for t in inp] for inp in inputs]
    tab, max_n = table(*zip(*dev))
    hyper = index = None
    keep_row = None
    if form.endswith("_dev"):
        ht = hyper_table(h, rows, live)
        hyper = torch.from_numpy(ht.reshape(-1)).to(DEV)
        index = torch.tensor([live], dtype=torch.int32, device=DEV)
        keep_row = float(ht[live, 3])
        assert ht[live, 0] == np.float32(h["lr"]) and ht[live, 1] == np.float32(h["c1"]) and ht[live, 2] == np.float32(h["c2"])
    launch(lib, form, tab, len(dev), max_n, h, hyper, index, rows)
    torch.cuda.synchronize()
    return [(d[0].cpu(), d[2].cpu(), d[3].cpu()) for d in dev], keep_row


# ---- a. grid-stride trips and tails -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_grid_stride_and_tails(lib, state, form):
    h = hyper_of(form)
    if form == "rmsprop":                                              # its square average lives in rec.m: the state's v >= 0 goes there
        state = [(p, g, v, m) for p, g, m, v in state]
    outs, keep_row = run_form(lib, form, state, h)
    wk, wc = {}, {}
    for inp, out in zip(state, outs):
        p, g, m, v = inp
        if form.startswith("adam"):
            check_adam("kernel", inp, out, h, wk, keep_row)
            check_adam("fp32 cpu", inp, cpu_adam(inp, h, keep_row), h, wc, keep_row)
            continue
        kind = 0 if form == "sgd" else 1
        k = K_ROUND[form]
        assert torch.equal(out[2], v)                                  # rec.v is not touched by either kind
        if kind == 0:
            assert torch.equal(out[1], m)
        sq_cpu = plain_sq(g, m, h, torch.float32)[0] if kind == 1 else m
        runs = [("kernel", wk, out[0], out[1]), ("fp32 cpu", wc, plain_p(p, g, sq_cpu, h, torch.float32, kind)[0], sq_cpu)]
        for tag, w, p1, sq1 in runs:
            if kind == 1:
                sq_ref, S_sq = plain_sq(g, m, h, torch.float64)
                e = worst(sq1, sq_ref, S_sq)
                w["m"] = max(w.get("m", 0.0), e)
                assert e <= k["m"], (tag, "sq", p.numel(), e)          # |got - ref| <= k * 2^-24 * S, every element
            p_ref, S_p = plain_p(p, g, sq1, h, torch.float64, kind)
            e = worst(p1, p_ref, S_p)
            w["p"] = max(w.get("p", 0.0), e)
            assert e <= k["p"], (tag, "p", p.numel(), e)
    note(form, "worst error / (2^-24 * S): kernel", {a: round(b, 3) for a, b in wk.items()}, "fp32 cpu",
         {a: round(b, 3) for a, b in wc.items()}, "bound k", K_ROUND[form.replace("_dev", "")])


# ---- b. the n4 = 0 path of a tensor that is not 16-byte aligned ----------------------------------------------------------------
@pytest.mark.parametrize("form", ["adam", "adam_l2"])
def test_misaligned_tensors_equal_aligned_bit_for_bit(lib, form):
    """The scalar loop and the float4 loop perform the same operations (both call adam_update, whose roundings are written out),
    so where a tensor lies must not change a bit of the result.  Left to the compiler's contraction the two loops had differed in
    the last bit of p (adam) and v (adam_l2)."""
    n = 1027
    h = hyper_of(form)
    gen = torch.Generator().manual_seed(23)
    vals = [torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.3,
            torch.rand(n, generator=gen) * 1.5]

    def run(misaligned):
        """each of p, g, m, v carved from a flat buffer of its own at element offset 1 (4-byte, not 16-byte aligned) or 0"""
        flats = [torch.zeros(n + 8, device=DEV) for _ in range(4)]
        views = []
        for i, (flat, val) in enumerate(zip(flats, vals)):
            off = 1 if i in misaligned else 0
            view = flat[off:off + n]
            view.copy_(val)
            assert view.data_ptr() % 16 == (4 if off else 0)
            views.append(view)
        tab, max_n = table(*[[t] for t in views])
        launch(lib, form, tab, 1, max_n, h)
        torch.cuda.synchronize()
        for flat, view in zip(flats, views):                           # nothing outside the carved range was written
            off = (view.data_ptr() - flat.data_ptr()) // 4
            assert not flat[:off].any() and not flat[off + n:].any()
        return views[0].cpu(), views[2].cpu(), views[3].cpu()

    aligned = run(())
    check_adam("aligned", vals, aligned, h, {})
    for mis in ((0,), (1,), (2,), (3,), (0, 1, 2, 3)):
        got = run(mis)
        for a, b, name in zip(got, aligned, "pmv"):
            assert torch.equal(a, b), (form, mis, name)


# ---- c. the device index of the _dev forms -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["adam_dev", "adam_l2_dev"])
def test_dev_index_edges(lib, form):
    h = hyper_of(form)
    rows = 5
    gen = torch.Generator().manual_seed(31)
    inputs = [(torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.3,
               torch.rand(n, generator=gen) * 1.5) for n in (1027, 5)]
    # the last row: the update with THAT row's values (every row of the table differs)
    outs, keep_row = run_form(lib, form, inputs, h, rows=rows, live=rows - 1)
    for inp, out in zip(inputs, outs):
        check_adam("row rows-1", inp, out, h, {}, keep_row)
    other, _ = run_form(lib, form, inputs, h, rows=rows, live=0)       # (row 0 holding h: rows - 1 holds other values there)
    assert torch.equal(other[0][0], outs[0][0])
    ht = hyper_table(h, rows, 0)
    for idx in (-1, rows):
        dev = [[t.to(DEV) for t in inp] for inp in inputs]
        tab, max_n = table(*zip(*dev))
        hyper = torch.from_numpy(ht.reshape(-1)).to(DEV)
        index = torch.tensor([idx], dtype=torch.int32, device=DEV)
        launch(lib, form, tab, len(dev), max_n, h, hyper, index, rows)
        torch.cuda.synchronize()
        for d, inp in zip(dev, inputs):
            for got, was in zip(d, inp):
                assert torch.equal(got.cpu(), was), (form, idx)
        assert int(index.item()) == idx


def test_index_advance_adds_exactly_one(lib):
    buf = torch.tensor([7, -1, 9], dtype=torch.int32, device=DEV)      # the counter between two neighbours
    mid = ctypes.c_void_p(buf.data_ptr() + 4)
    for want in (0, 1, 2):
        assert lib.dei2i_index_advance(mid, stream()) == 0
        torch.cuda.synchronize()
        assert buf.tolist() == [7, want, 9]
    buf[1] = 2 ** 31 - 2
    assert lib.dei2i_index_advance(mid, stream()) == 0
    torch.cuda.synchronize()
    assert buf.tolist() == [7, 2 ** 31 - 1, 9]


# ---- d. the EMA lerp -----------------------------------------------------------------------------------------------------------
EMA_SIZES = [1, 7, 262144, 262144 + 259]                               # 1024 workgroups x 256: the last takes a second trip


@pytest.fixture(scope="module")
def ema_state():
    gen = torch.Generator().manual_seed(41)
    return [(torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.7 + 0.1) for n in EMA_SIZES]      # (ema, param)


@pytest.mark.parametrize("w", [0.0, 0.25, 0.4999, 0.5, 0.999, 1.0])
def test_ema_lerp(lib, ema_state, w):
    from de_i2i_gan_amd.optim import ema_lerp_
    emas = [e.to(DEV) for e, _ in ema_state]
    params = [p.to(DEV) for _, p in ema_state]
    for i, e in enumerate(emas):
        e._dei2i_epoch = 10 * i
    ema_lerp_(emas, params, w)
    torch.cuda.synchronize()
    w32 = f32(w)
    hi = abs(w32) >= 0.5
    wk = wc = 0.0
    for i, (e, p, (e0, p0)) in enumerate(zip(emas, params, ema_state)):
        assert e._dei2i_epoch == 10 * i + 1
        assert torch.equal(p.cpu(), p0)                                # the parameter is read only
        got = e.cpu()
        ref = torch.lerp(p0.double(), e0.double(), w32)
        d = (e0.double() - p0.double()).abs()
        S = e0.double().abs() + d * (1 - w32) if hi else p0.double().abs() + w32 * d
        diff = e0 - p0
        one_minus_w = float(np.float32(1) - np.float32(w32))
        cpu = e0 - diff * one_minus_w if hi else p0 + w32 * diff       # fp32 restatement of the kernel's line
        ek, ec = worst(got, ref, S), worst(cpu, ref, S)
        wk, wc = max(wk, ek), max(wc, ec)
        assert ek <= K_EMA[hi] and ec <= K_EMA[hi], (w, e0.numel(), ek, ec)       # |got - ref| <= k * 2^-24 * S, every element
        if w == 1.0:
            assert torch.equal(got, e0)                                # end - diff * 0: the EMA tensor keeps its bits
        if w == 0.0:
            assert torch.equal(got, p0)                                # start + 0 * diff: the parameter's bits
    note("ema_lerp w", w, "worst error / (2^-24 * S): kernel", round(wk, 3), "fp32 cpu", round(wc, 3), "bound k", K_EMA[hi])


# ---- f. three FusedAdam steps across the grid-stride trip ----------------------------------------------------------------------
def test_fused_adam_three_steps_large_tensor():
    from de_i2i_gan_amd.optim import FusedAdam
    n = 524288 + 1027
    gen = torch.Generator().manual_seed(53)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (10.0 ** (s - 1)) for s in range(3)]
    ref = p0.double().clone().requires_grad_(True)
    topt = torch.optim.Adam([ref], lr=2e-4, betas=(0.5, 0.999), eps=1e-8)
    gp = torch.nn.Parameter(p0.to(DEV))
    opt = FusedAdam([gp], lr=2e-4, betas=(0.5, 0.999), eps=1e-8)
    for g in grads:
        ref.grad = g.double()
        topt.step()
        gp.grad = g.to(DEV)
        opt.step()
    got, want = gp.detach().double().cpu(), ref.detach()
    maxrel = ((got - want).abs().max() / want.abs().max().clamp_min(1e-12)).item()
    note("FusedAdam 3 steps n =", n, "maxrel", maxrel)
    assert maxrel < 2e-6                                               # (a skipped element is 3 * lr = 6e-4 away: 1e-4 of the max)
