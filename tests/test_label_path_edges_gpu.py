"""SPADE's batched label path (csrc/label_path.hip: pack, forward, input gradient, weight + bias gradient) against float64 at the seams
of the file: hidden = 96 (three 32-channel blocks in the wgrad, two dead waves in the dgrad's second workgroup), N around LP_IMG = 4 and
LP_G = 3, 2C that is no multiple of 128, the 16-module limit, dead modules in every position, an activation tensor wider than
modules x hidden with slices out of order, and every refusal of the host code.

Reference of every case, float64 on the CPU: per module F.conv2d(actv slice, cat(gamma.weight, beta.weight), cat(gamma.bias, beta.bias),
padding=1) on the bf16-rounded activation and filters (the kernels read bf16) and the unrounded fp32 biases; dactv / dW / dbias from
torch.autograd.grad with the bf16 table gradients.  A dead module (its table got no gradient) contributes nothing: its slice of dactv
is zero, its parameters get None.

  * random data: the bounds of the existing label-path and hot-shape tests (tests/test_fused_norm_gpu.py
    test_label_path_batched_equals_the_per_module_convs) -- the tables and dactv are bf16 stores of fp32 sums, dW / dbias are fp32 sums
    in another order;
  * small integers: every product and partial sum is an integer far below 2^24 and every bf16 output an integer of magnitude <= 256,
    so EVERY output equals the reference exactly -- one dropped pixel, tap or sample shows."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
from de_i2i_gan_amd._lib import ERR_BAD_ARG as BAD_ARG
SENT = 4096.0                    # exact in bf16 and fp32, and no result of the integer cases reaches it
GUARD = 64                       # elements on either side of a guarded buffer (a multiple of 8: the payload stays 16-byte aligned)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def same(a, b):
    return torch.equal(a.detach().double().cpu(), b.detach().double().cpu())


def draw(gen, N, hidden, Cs, ctot, integer):
    """-> actv (N, 5, 5, ctot) bf16, per module (gamma.weight, gamma.bias, beta.weight, beta.bias) fp32 and the table gradient bf16"""
    def sparse(shape):           # {-1, 0, 1}, one in eight non-zero
        return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float() * (torch.rand(shape, generator=gen) < 0.125).float()

    if integer:
        actv = torch.randint(0, 3, (N, 5, 5, ctot), generator=gen).float()
    else:
        actv = torch.relu(torch.randn(N, 5, 5, ctot, generator=gen))
    params, gys = [], []
    for C in Cs:
        if integer:
            ws = [sparse((C, hidden, 3, 3)) for _ in range(2)]
            bs = [torch.randint(-3, 4, (C,), generator=gen).float() for _ in range(2)]
            gys.append(sparse((N, 5, 5, 2 * C)).bfloat16())
        else:
            ws = [torch.randn(C, hidden, 3, 3, generator=gen) * (9 * hidden) ** -0.5 for _ in range(2)]
            bs = [torch.randn(C, generator=gen) * 0.3 for _ in range(2)]
            gys.append(torch.randn(N, 5, 5, 2 * C, generator=gen).bfloat16())
        params.append((ws[0], bs[0], ws[1], bs[1]))
    return actv.bfloat16(), params, gys


def reference(actv, hidden, offs, params, gys):
    """float64 -> (tables, dactv, per module (d gamma.weight, d gamma.bias, d beta.weight, d beta.bias) or None); gys[i] None: dead"""
    N, _, _, ctot = actv.shape
    tabs, grads = [], []
    dactv = torch.zeros(N, 5, 5, ctot, dtype=torch.float64)
    for (gw, gbias, bw, bbias), off, gy in zip(params, offs, gys):
        C = gw.shape[0]
        a = actv[..., off:off + hidden].permute(0, 3, 1, 2).double().requires_grad_(True)
        w = torch.cat([gw, bw], 0).bfloat16().double().requires_grad_(True)
        b = torch.cat([gbias, bbias], 0).double().requires_grad_(True)
        y = F.conv2d(a, w, b, padding=1)
        tabs.append(y.detach().permute(0, 2, 3, 1))
        if gy is None:
            grads.append(None)
            continue
        da, dw, db = torch.autograd.grad(y, [a, w, b], gy.permute(0, 3, 1, 2).double())
        dactv[..., off:off + hidden] = da.permute(0, 2, 3, 1)
        grads.append((dw[:C], db[:C], dw[C:], db[C:]))
    return tabs, dactv, grads


def run_ops(actv, hidden, params, gys):
    """ops.label_gamma_beta forward + backward -> (tables, dactv, parameter gradients or None per module, the packed filter pairs)"""
    from de_i2i_gan_amd import ops
    dev_p = [tuple(t.to(DEV).requires_grad_(True) for t in p) for p in params]
    convs = [(SimpleNamespace(weight=p[0], bias=p[1]), SimpleNamespace(weight=p[2], bias=p[3])) for p in dev_p]
    a = actv.to(DEV).requires_grad_(True)
    assert ops.label_gamma_beta_supported(a, hidden, convs)
    cache = {}
    tabs = ops.label_gamma_beta(a, hidden, convs, cache)
    live = [i for i, g in enumerate(gys) if g is not None]
    torch.autograd.backward([tabs[i] for i in live], [gys[i].to(DEV) for i in live])
    torch.cuda.synchronize()
    grads = [None if all(t.grad is None for t in p) else tuple(t.grad for t in p) for p in dev_p]
    return [t.detach() for t in tabs], a.grad, grads, cache["packed"]


CYCLE16 = [(16, 32, 48, 64)[i % 4] for i in range(16)]
RANDOM_CASES = [(1, 32, [16], ()), (2, 96, [16, 80, 48], ()), (3, 128, [144], ()), (4, 64, [32, 32], ()), (5, 128, [256, 16], (0,)),
                (7, 64, CYCLE16, (3, 9)), (10, 96, [64], ())]


@pytest.mark.parametrize("N,hidden,Cs,dead", RANDOM_CASES, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, list) else f"m{len(v)}")
def test_label_path_random_data_against_float64(N, hidden, Cs, dead):
    """Random data through ops.label_gamma_beta.  Bounds: those of test_label_path_batched_equals_the_per_module_convs (the same error
    sources: a bf16 store of an fp32 sum for the tables and dactv, summation order for the fp32 dW / dbias)."""
    gen = torch.Generator().manual_seed(11)
    nm = len(Cs)
    actv, params, gys = draw(gen, N, hidden, Cs, nm * hidden, integer=False)
    gys = [None if i in dead else g for i, g in enumerate(gys)]
    offs = [i * hidden for i in range(nm)]
    r_tabs, r_da, r_grads = reference(actv.float(), hidden, offs, params, gys)
    tabs, da, grads, _ = run_ops(actv, hidden, params, gys)
    worst = {"tab_l2": 0.0, "tab_max": 0.0, "dw": 0.0, "db": 0.0}
    for i in range(nm):
        worst["tab_l2"] = max(worst["tab_l2"], rel_l2(tabs[i], r_tabs[i]))
        worst["tab_max"] = max(worst["tab_max"], maxrel(tabs[i], r_tabs[i]))
        if i in dead:
            assert grads[i] is None and r_grads[i] is None
            assert float(da[..., offs[i]:offs[i] + hidden].abs().max()) == 0.0
            continue
        assert grads[i] is not None and all(g is not None for g in grads[i]), i
        for k in (0, 2):
            worst["dw"] = max(worst["dw"], rel_l2(grads[i][k], r_grads[i][k]))
            worst["db"] = max(worst["db"], rel_l2(grads[i][k + 1], r_grads[i][k + 1]))
    worst["da"] = rel_l2(da, r_da)
    print("label path vs float64", (N, hidden, Cs if nm < 16 else "cycle16", dead), {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["tab_l2"] < 3e-3 and worst["tab_max"] < 2e-2, worst     # measured over the cases: at most 1.7e-3 and 2.9e-3
    assert worst["da"] < 4e-3, worst                                     # measured: at most 1.8e-3
    assert worst["dw"] < 2e-4, worst                                     # measured: at most 5.9e-8
    assert worst["db"] < 1e-5, worst                                     # measured: at most 1.0e-8


INTEGER_CASES = [(7, 128, [256, 16, 80], ()), (5, 96, [48, 64], ()), (1, 32, [16], ()), (2, 64, [32, 144], ()), (5, 96, [48, 64], (0,))]


@pytest.mark.parametrize("N,hidden,Cs,dead", INTEGER_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_label_path_is_exact_on_small_integers(N, hidden, Cs, dead):
    """actv in {0, 1, 2}, filters and table gradients in {-1, 0, 1} with one in eight non-zero, integer biases in [-3, 3]: every sum is
    a small integer in fp32 and in bf16 (|tables|, |dactv| <= 256, asserted on the reference), so the tables, dactv, dW, dbias and the
    packed filters ([2C][9][hidden] forward, [hidden][9][2C] input gradient) equal the float64 reference bit for bit."""
    gen = torch.Generator().manual_seed(12)
    nm = len(Cs)
    actv, params, gys = draw(gen, N, hidden, Cs, nm * hidden, integer=True)
    gys = [None if i in dead else g for i, g in enumerate(gys)]
    offs = [i * hidden for i in range(nm)]
    r_tabs, r_da, r_grads = reference(actv.float(), hidden, offs, params, gys)
    assert max(float(t.abs().max()) for t in r_tabs) <= 256 and float(r_da.abs().max()) <= 256      # (these draws: at most 67 and 37)
    tabs, da, grads, packed = run_ops(actv, hidden, params, gys)
    assert same(da, r_da)
    for i, C in enumerate(Cs):
        assert same(tabs[i], r_tabs[i]), ("table", i)
        w = torch.cat([params[i][0], params[i][2]], 0).reshape(2 * C, hidden, 9)
        assert same(packed[i][0].view(2 * C, 9, hidden), w.permute(0, 2, 1)), ("packed forward filters", i)
        assert same(packed[i][1].view(hidden, 9, 2 * C), w.permute(1, 2, 0)), ("packed input-gradient filters", i)
        if i in dead:
            assert grads[i] is None
            continue
        for k, name in enumerate(("d gamma.weight", "d gamma.bias", "d beta.weight", "d beta.bias")):
            assert same(grads[i][k], r_grads[i][k]), (name, i)


# ---- the C ABI directly ------------------------------------------------------------------------------------------------------
def guarded(n, dtype, fill=SENT):
    """-> (whole buffer, payload view of n elements) with GUARD sentinel elements on either side"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all())


def ptr(t):
    return None if t is None else t.data_ptr()


class Buffers:
    """device operands and sentinel-filled, guarded outputs of the four entry points for modules of Cs at in_offs"""

    def __init__(self, N, hidden, ctot, Cs, offs, seed):
        from de_i2i_gan_amd import _lib
        self.lib = _lib.load()
        self.L = _lib
        self.N, self.hidden, self.ctot, self.Cs, self.offs = N, hidden, ctot, Cs, offs
        gen = torch.Generator().manual_seed(seed)
        self.actv, self.params, self.gys = draw(gen, N, hidden, Cs, ctot, integer=True)
        self.d_actv = self.actv.to(DEV)
        self.d_params = [tuple(t.to(DEV).contiguous() for t in p) for p in self.params]
        self.d_gys = [g.to(DEV) for g in self.gys]
        bf, f32 = torch.bfloat16, torch.float32
        self.wf = [guarded(self.lib.dei2i_label_gb_packed_elems(C, hidden), bf) for C in Cs]
        self.wd = [guarded(self.lib.dei2i_label_gb_packed_elems(C, hidden), bf) for C in Cs]
        self.tab = [guarded(N * 25 * 2 * C, bf) for C in Cs]
        self.dactv = guarded(N * 25 * ctot, bf)
        self.dw = [(guarded(C * hidden * 9, f32), guarded(C * hidden * 9, f32)) for C in Cs]
        self.db = [(guarded(C, f32), guarded(C, f32)) for C in Cs]

    def outputs(self):
        return ([b for b, _ in self.wf + self.wd + self.tab] + [self.dactv[0]] + [b for pair in self.dw + self.db for b, _ in pair])

    def mods(self, forward, n=None, **over):
        """the module table of pack / forward (``forward``) or of the two gradient launches; ``over``: field -> (module, value)"""
        n = len(self.Cs) if n is None else n
        arr = (self.L.LabelMod * max(n, 1))()
        for j in range(n):
            i = j % len(self.Cs)
            p = self.d_params[i]
            if forward:
                f = dict(gamma_weight=ptr(p[0]), beta_weight=ptr(p[2]), gamma_bias=ptr(p[1]), beta_bias=ptr(p[3]), packed_fwd=ptr(self.wf[i][1]),
                         packed_dgrad=ptr(self.wd[i][1]), gb=ptr(self.tab[i][1]))
            else:
                f = dict(packed_fwd=ptr(self.wf[i][1]), packed_dgrad=ptr(self.wd[i][1]), gb=ptr(self.d_gys[i]), d_gamma_weight=ptr(self.dw[i][0][1]),
                         d_beta_weight=ptr(self.dw[i][1][1]), d_gamma_bias=ptr(self.db[i][0][1]), d_beta_bias=ptr(self.db[i][1][1]))
            f.update(C=self.Cs[i], in_off=self.offs[i], live=1, reserved=0)
            for k, (mod, v) in over.items():
                if mod == j:
                    f[k] = v
            arr[j] = self.L.LabelMod(**f)
        return arr


def test_label_path_c_abi_with_a_wide_activation_and_slices_out_of_order():
    """ops always passes in_off = i * hidden and ctot = n * hidden; the kernels take more: hidden 64 in a 200-channel activation tensor,
    module 0 (C = 32) on channels [136, 200), module 1 (C = 16) on [0, 64), N = 5, integer data.  Every output sits between sentinel
    guards and dactv is pre-filled with the sentinel: results exact, channels [64, 136) of dactv and all guards untouched."""
    from de_i2i_gan_amd import ops
    N, hidden, ctot, Cs, offs = 5, 64, 200, [32, 16], [136, 0]
    B = Buffers(N, hidden, ctot, Cs, offs, seed=13)
    r_tabs, r_da, r_grads = reference(B.actv.float(), hidden, offs, B.params, B.gys)
    assert max(float(t.abs().max()) for t in r_tabs) <= 256 and float(r_da.abs().max()) <= 256
    lib, st = B.lib, ops._stream()
    fwd, bwd = B.mods(True), B.mods(False)
    assert lib.dei2i_label_gb_pack(fwd, 2, hidden, st) == 0
    assert lib.dei2i_label_gb_fwd(fwd, 2, hidden, ctot, N, ptr(B.d_actv), st) == 0
    assert lib.dei2i_label_gb_dgrad(bwd, 2, hidden, ctot, N, ptr(B.dactv[1]), st) == 0
    assert lib.dei2i_label_gb_wgrad(bwd, 2, hidden, ctot, N, ptr(B.d_actv), st) == 0
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in B.outputs())
    da = B.dactv[1].view(N, 5, 5, ctot)
    assert bool((da[..., 64:136] == SENT).all())
    for i, (C, off) in enumerate(zip(Cs, offs)):
        assert same(da[..., off:off + hidden], r_da[..., off:off + hidden]), ("dactv", i)
        assert same(B.tab[i][1].view(N, 5, 5, 2 * C), r_tabs[i]), ("table", i)
        w = torch.cat([B.params[i][0], B.params[i][2]], 0).reshape(2 * C, hidden, 9)
        assert same(B.wf[i][1].view(2 * C, 9, hidden), w.permute(0, 2, 1)) and same(B.wd[i][1].view(hidden, 9, 2 * C), w.permute(1, 2, 0))
        assert same(B.dw[i][0][1].view(C, hidden, 3, 3), r_grads[i][0]) and same(B.dw[i][1][1].view(C, hidden, 3, 3), r_grads[i][2]), ("dW", i)
        assert same(B.db[i][0][1], r_grads[i][1]) and same(B.db[i][1][1], r_grads[i][3]), ("dbias", i)


def test_label_path_refusals_launch_nothing():
    """Host code: every malformed call returns DEI2I_ERR_BAD_ARG and leaves the (sentinel-filled) outputs alone."""
    from de_i2i_gan_amd import ops
    N, hidden, ctot, Cs, offs = 3, 64, 128, [16, 32], [0, 64]
    B = Buffers(N, hidden, ctot, Cs, offs, seed=14)
    lib, st = B.lib, ops._stream()
    actv, dactv = ptr(B.d_actv), ptr(B.dactv[1])

    def all_four(fwd, bwd, n=2, hidden=hidden, ctot=ctot, N=N, actv=actv, dactv=dactv, which="pfdw"):
        rcs = {}
        if "p" in which:
            rcs["pack"] = lib.dei2i_label_gb_pack(fwd, n, hidden, st)
        if "f" in which:
            rcs["fwd"] = lib.dei2i_label_gb_fwd(fwd, n, hidden, ctot, N, actv, st)
        if "d" in which:
            rcs["dgrad"] = lib.dei2i_label_gb_dgrad(bwd, n, hidden, ctot, N, dactv, st)
        if "w" in which:
            rcs["wgrad"] = lib.dei2i_label_gb_wgrad(bwd, n, hidden, ctot, N, actv, st)
        return rcs

    calls = {}
    for h in (16, 48, 160):
        calls[f"hidden={h}"] = all_four(B.mods(True), B.mods(False), hidden=h, ctot=2 * h + 64)
    for C in (8, 24):
        calls[f"C={C}"] = all_four(B.mods(True, C=(1, C)), B.mods(False, C=(1, C)))
    calls["n=0"] = all_four(B.mods(True), B.mods(False), n=0)
    calls["n=17"] = all_four(B.mods(True, n=17), B.mods(False, n=17), n=17)
    calls["in_off=4"] = all_four(B.mods(True, in_off=(1, 4)), B.mods(False, in_off=(1, 4)), which="fdw")
    calls["in_off+hidden>ctot"] = all_four(B.mods(True, in_off=(1, 72)), B.mods(False, in_off=(1, 72)), which="fdw")
    calls["ctot=100"] = all_four(B.mods(True), B.mods(False), n=1, ctot=100, which="fdw")
    calls["N=0"] = all_four(B.mods(True), B.mods(False), N=0, which="fdw")
    calls["null actv / dactv"] = all_four(B.mods(True), B.mods(False), actv=None, dactv=None, which="fdw")
    calls["live module without gb"] = all_four(None, B.mods(False, gb=(0, None)), which="dw")
    calls["pack without packed_fwd"] = all_four(B.mods(True, packed_fwd=(1, None)), None, which="pf")
    calls["pack without packed_dgrad"] = all_four(B.mods(True, packed_dgrad=(0, None)), None, which="p")
    calls["null module table"] = all_four(None, None)
    torch.cuda.synchronize()
    bad = {k: v for k, v in calls.items() if any(rc != BAD_ARG for rc in v.values())}
    assert not bad, bad
    for b in B.outputs():
        assert bool((b == SENT).all())
    # the same tables, unbroken, are accepted: the refusals above are due to the one field each of them changes
    fwd, bwd = B.mods(True), B.mods(False)
    assert lib.dei2i_label_gb_pack(fwd, 2, hidden, st) == 0 and lib.dei2i_label_gb_fwd(fwd, 2, hidden, ctot, N, actv, st) == 0
    assert lib.dei2i_label_gb_dgrad(bwd, 2, hidden, ctot, N, dactv, st) == 0 and lib.dei2i_label_gb_wgrad(bwd, 2, hidden, ctot, N, actv, st) == 0
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in B.outputs()) and not bool((B.dactv[1] == SENT).any())
