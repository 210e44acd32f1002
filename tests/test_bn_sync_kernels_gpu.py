"""The staged BatchNorm kernels of a batch sharded over processes (csrc/reduce.hip dei2i_bn_sync_*, ops.bn_sync) in ONE process, no
process group: a batch is cut into W shards, every shard runs stage 1, the message buffers are added with torch (the stand-in for the
all-reduce) and every shard runs stage 2 -- forward and backward -- against float64 torch BatchNorm + activation on the CPU over the
WHOLE batch, on operands rounded to the compute dtype.  Conventions, helpers and tolerances are those of test_reduce_edges_gpu.py
(TOL of the tensor's max for outputs and dy, x2 for parameter gradients, 1e-4 (+5e-3 in bf16) for the statistics, the kink band
with its < 0.1 % condition asserted; seeds are taken by clear_of_kinks, on the reference alone).

How the shards are interleaved.  ``exchange`` is called from inside one autograd function, so a single process cannot hold shard A
between its two stages while shard B runs its stage 1.  The shards' passes are therefore REPEATED: the exchange of pass k + 1 returns
the sum of the messages the shards recorded in pass k.  The message of an exchange depends only on the exchanges before it (forward
statistics on nothing, the backward sums on the forward statistics), so with M exchanges per shard the pass M + 1 ran every stage 2 on
the true sums; the kernels use no atomics, so the recorded messages of the last two passes are asserted to be the same bits.  Every
pass starts from fresh parameters and running buffers; only the last one is checked."""
import math

import pytest
import torch
import torch.nn.functional as F

import test_reduce_edges_gpu as E
from test_reduce_edges_gpu import TOL, back, check_grad, clear_of_kinks, data, dev, kink_keep, relmax, rounded, to_dev, vecs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from de_i2i_gan_amd import ops as _ops
    return _ops


def note(*a):
    print("[bn-sync]", *a, flush=True)


class Replay:
    """the exchange functions of W shards (module docstring): record this pass's message, hand out the sum of the last pass's"""

    def __init__(self, shards):
        self.prev, self.cur = None, [[] for _ in range(shards)]

    def next_pass(self):
        self.prev, self.cur = self.cur, [[] for _ in self.cur]

    def of(self, shard):
        def exchange(msg):
            i = len(self.cur[shard])
            self.cur[shard].append(msg.clone())
            if self.prev is not None and all(len(p) > i for p in self.prev):
                total = self.prev[0][i].clone()
                for p in self.prev[1:]:
                    total += p[i]
                msg.copy_(total)
        return exchange

    def settled(self):
        return all(len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)) for a, b in zip(self.prev, self.cur))


def run_passes(shards, exchanges, one_shard):
    """one_shard(s, exchange) for every shard, exchanges + 1 times -> the last pass's results"""
    rp = Replay(shards)
    out = None
    for k in range(exchanges + 1):
        if k:
            rp.next_pass()
        out = [one_shard(s, rp.of(s)) for s in range(shards)]
    assert all(len(m) == exchanges for m in rp.cur), [len(m) for m in rp.cur]
    assert rp.settled(), "the messages of the last two passes differ: the staged kernels are not bit-reproducible"
    return out, rp.cur


# (shards, N per shard, H, W, C, groups, residual): what it reaches
CASES = [
    (2, 1, 5, 7, 24, 1, False),        # 35 rows: one chunk; cv = 3 in bf16 (the non-invariant apply kernel), 6 in f32
    (2, 2, 16, 32, 64, 1, False),      # 8 chunks per image
    (3, 2, 9, 13, 40, 2, True),        # three shards, groups = 2 (one image per group and shard), a residual
    (2, 1, 40, 40, 32, 1, False),      # HW = 1600: 25 chunks
    (2, 2, 8, 8, 20, 1, False),        # nf = 20 in a padded stride of 24 (bf16); a plain 20-channel layer in f32
]


def _reference(pname, case, seed):
    """float64 BatchNorm + LeakyReLU (+ residual) over the WHOLE batch: global group g = group g of every shard"""
    W, N, h, w, c, groups, with_res = case
    shape = (W * N, h, w, c)
    y, g = data(shape, seed), data(shape, seed + 2, 1.0, 0.0)
    res = data(shape, seed + 1, 1.0, 0.1) if with_res else None
    wt, bs, rm, rv = vecs(c, seed + 3)
    yr = rounded(y, pname).double().requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    ng = N // groups
    rows = [[s * N + k * ng + i for s in range(W) for i in range(ng)] for k in range(groups)]      # images of global group k
    pres, mean, rstd = [], [], []
    for k in range(groups):                                   # running buffers: the groups' updates in pass order
        yk = yr[rows[k]]
        pres.append(F.batch_norm(yk, rm64, rv64, w64, b64, True, 0.1, 1e-5))
        mean.append(yk.detach().mean(dim=(0, 2, 3)))
        rstd.append(1.0 / torch.sqrt(yk.detach().var(dim=(0, 2, 3), unbiased=False) + 1e-5))
    order = torch.tensor([i for k in range(groups) for i in rows[k]])
    pre = torch.cat(pres, 0)[torch.argsort(order)]
    out = F.leaky_relu(pre, 0.2)
    if with_res:
        out = out + rounded(res, pname).double()
    gr = rounded(g, pname).double()
    dy, dw, db = torch.autograd.grad(out, [yr, w64, b64], gr, retain_graph=True)
    # one shard's OWN share of dweight / dbias: the sum over its rows only (the statistics do not depend on the parameters)
    local = [torch.autograd.grad((out[s * N:(s + 1) * N] * gr[s * N:(s + 1) * N]).sum(), [w64, b64], retain_graph=True) for s in range(W)]
    return dict(y=y, g=g, res=res, wt=wt, bs=bs, rm=rm, rv=rv, pre=pre.detach(), out=out.detach(), dy=dy, dw=dw, db=db, local=local,
                rm_ref=rm64, rv_ref=rv64, mean=torch.stack(mean), rstd=torch.stack(rstd))


@pytest.mark.parametrize("pname", E.PNAMES)
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c[:5])) + f"-g{c[5]}" + ("-res" if c[6] else "") for c in CASES])
def test_staged_batchnorm_over_shards_equals_float64_over_the_whole_batch(ops, pname, case):
    W, N, h, w, c, groups, with_res = case
    P = clear_of_kinks(lambda s: _reference(pname, case, s), "leaky_relu", 7)
    prec = ops.BF16 if pname == "bf16" else ops.F32
    cs = prec.pad(c)
    assert (cs > c) == (pname == "bf16" and c == 20)

    def one_shard(s, exchange):
        sl = slice(s * N, (s + 1) * N)
        wg, bg = P["wt"].to(dev()).requires_grad_(True), P["bs"].to(dev()).requires_grad_(True)
        rm, rv = P["rm"].to(dev()), P["rv"].to(dev())
        nbt = torch.zeros((), dtype=torch.int64, device=dev())
        yg = to_dev(P["y"][sl], pname, cs).requires_grad_(True)
        resg = to_dev(P["res"][sl], pname, cs) if with_res else None
        with ops.bn_sync(exchange, rank=s, world=W):
            if groups > 1:
                with ops.bn_running_deferred() as running, ops.bn_batch_groups(groups):
                    running.pass_index = tuple(range(groups))
                    out = ops.batchnorm_act(yg, wg, bg, rm, rv, True, "leaky_relu", resg, num_batches_tracked=nbt)
                    running.apply()
            else:                              # the module's own buffers and counter, updated inside stage 2
                out = ops.batchnorm_act(yg, wg, bg, rm, rv, True, "leaky_relu", resg, num_batches_tracked=nbt)
        saved = out.grad_fn.saved_tensors                              # (y, a, b, mean, rstd)
        out.backward(to_dev(P["g"][sl], pname, cs))                    # (outside the scope: the layer kept it)
        return dict(out=back(out, c), dy=back(yg.grad, c), dw=wg.grad.double().cpu(), db=bg.grad.double().cpu(), rm=rm.cpu(), rv=rv.cpu(),
                    nbt=int(nbt.item()), mean=saved[3][:, :c].double().cpu(), rstd=saved[4][:, :c].double().cpu(),
                    pad=float(out[..., c:].abs().max()) if cs > c else 0.0)

    R, msgs = run_passes(W, 2, one_shard)
    assert tuple(msgs[0][0].shape) == (groups, 2 * cs + 1) and tuple(msgs[0][1].shape) == (groups, 2, cs)     # one message per direction
    assert msgs[0][0].dtype == msgs[0][1].dtype == torch.float64
    assert msgs[0][0][:, 2 * cs].tolist() == [float(N // groups * h * w)] * groups                             # this shard's count
    tag, tol = f"{pname} {case}", TOL[pname]
    stol = 1e-4 + (5e-3 if pname == "bf16" else 0)
    keep = kink_keep(P["pre"], "leaky_relu")
    for s, r in enumerate(R):
        sl = slice(s * N, (s + 1) * N)
        e = relmax(r["out"], P["out"][sl])
        note(f"{tag} shard {s} out: max {e:.3e} (tol {tol:.1e})")
        assert e < tol
        em, es = relmax(r["mean"], P["mean"]), relmax(r["rstd"], P["rstd"])
        note(f"{tag} shard {s} mean {em:.3e} rstd {es:.3e} (tol {stol:.1e})")
        assert em < stol and es < stol
        er, ev = relmax(r["rm"], P["rm_ref"]), relmax(r["rv"], P["rv_ref"])          # unbiased, with the GLOBAL count
        note(f"{tag} shard {s} running mean {er:.3e} var {ev:.3e} (tol {stol:.1e})")
        assert er < stol and ev < stol
        assert r["nbt"] == groups and r["pad"] == 0.0
        check_grad(r["dy"], P["dy"][sl], None if keep is None else keep[sl], pname, f"{tag} shard {s} dy")
        # one shard's dweight / dbias: ITS rows' sum, not the global one (the gradient exchange totals them afterwards)
        lw, lb = relmax(r["dw"], P["local"][s][0]), relmax(r["db"], P["local"][s][1])
        note(f"{tag} shard {s} local dweight {lw:.3e} dbias {lb:.3e} (tol {2 * tol:.1e})")
        assert r["dw"].shape == (c,) and lw < 2 * tol and lb < 2 * tol
    ew, eb = relmax(sum(r["dw"] for r in R), P["dw"]), relmax(sum(r["db"] for r in R), P["db"])
    note(f"{tag} dweight {ew:.3e} dbias {eb:.3e} summed over the shards (tol {2 * tol:.1e})")
    assert ew < 2 * tol and eb < 2 * tol
    # the shards' shares differ from the total by far more than the tolerance: the local check above discriminates
    assert relmax(R[0]["dw"], P["dw"]) > 10 * tol


def test_resblock_shaped_conv_bn_conv_with_epilogue_records(ops):
    """Forward records from a conv epilogue, backward records from the dgrad epilogue: bf16 conv -> batchnorm_act(LeakyReLU) -> conv,
    3x3 reflect, 256 channels at 32 x 64, 28 images per shard -- the smallest batch at which the 16 x 32 tile kernel takes the input
    gradient with its norm epilogue (N * 2 * 2 tiles x 2 channel blocks >= 7/8 of the CUs) -- two shards, run through ``ops`` inside a
    ``bn_sync`` scope whose exchange is the torch sum of the two shards' buffers (the repeated passes of the module docstring: the
    autograd functions themselves ran, the staged helpers were not driven by hand).  The kernel families are asserted the way
    test_hot_shapes_gpu.py does, and ops.bwd_fused_counts that the BatchNorm backward TOOK the epilogue's records.  Reference: float64
    BatchNorm + LeakyReLU on the CPU over both shards' conv outputs (the bf16 tensors the first conv stored) with the upstream gradient the
    second conv's input-gradient kernel produced -- the convs are not under test here."""
    from de_i2i_gan_amd import _lib
    W, N, h, w, c = 2, 28, 32, 64, 256
    pname, tol = "bf16", TOL["bf16"]
    torch.manual_seed(11)
    x = (torch.randn(W * N, h, w, c) * 1.3 + 0.2).bfloat16().to(dev())
    w1 = (torch.randn(c, c, 3, 3) * math.sqrt(2.0 / (c * 9))).to(dev())
    w2 = (torch.randn(c, c, 3, 3) * math.sqrt(2.0 / (c * 9))).to(dev())
    gy = torch.randn(W * N, h, w, c).bfloat16().to(dev())
    wt, bs, rm0, rv0 = vecs(c, 12)
    geom = ops.ConvGeom(c, c, 3, 1, 1, True, False)
    caches = (ops.PackedWeights(), ops.PackedWeights())
    fams = []

    def counts():
        return {k: v for k, v in _lib.launch_counts(reset=True).items() if v and k != "splitk_finalize"}

    def shard_pass(s, exchange):
        sl = slice(s * N, (s + 1) * N)
        wg, bg = wt.to(dev()).requires_grad_(True), bs.to(dev()).requires_grad_(True)
        rm, rv = rm0.to(dev()), rv0.to(dev())
        counts()
        y1 = ops.conv2d(x[sl], w1, None, caches[0], geom, "none", stats=True)
        records = y1._dei2i_stats                                          # the moments records of the conv epilogue ...
        y1 = y1.detach().requires_grad_(True)
        y1._dei2i_stats, y1._dei2i_at_version = records, y1._version       # ... travel with the leaf the BatchNorm is given
        with ops.bn_sync(exchange, rank=s, world=W):
            z = ops.batchnorm_act(y1, wg, bg, rm, rv, True, "leaky_relu")
            y2 = ops.conv2d(z, w2, None, caches[1], geom, "none")
        f_fwd = counts()
        dz = []
        z.register_hook(lambda g_: dz.append(g_.detach().clone()))
        before = dict(ops.bwd_fused_counts)
        y2.backward(gy[sl])
        torch.cuda.synchronize()
        took = {k: ops.bwd_fused_counts[k] - before[k] for k in before}
        fams.append((f_fwd, counts(), took))
        note(f"epilogue case shard {s}: forward {fams[-1][0]} backward {fams[-1][1]} {took}")
        return dict(y1=y1.detach(), z=z.detach(), dz=dz[0], dy1=y1.grad.detach(), dw=wg.grad.double().cpu(), db=bg.grad.double().cpu(),
                    rm=rm.cpu(), rv=rv.cpu())

    R, _ = run_passes(W, 2, shard_pass)
    for f_fwd, f_bwd, took in fams:
        assert f_fwd == {"halo16_conv": 2}, ("forward convs were served by", f_fwd)
        assert f_bwd == {"halo16_conv": 1}, ("the input gradient was served by", f_bwd)
        assert took == {"epilogue": 1, "taken": 1}, took                   # the dgrad epilogue's records fed the staged backward

    # ---- float64 reference of the BatchNorm alone, over both shards ----
    y64 = torch.cat([r["y1"] for r in R], 0).double().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    g64 = torch.cat([r["dz"] for r in R], 0).double().cpu().permute(0, 3, 1, 2)
    w64, b64 = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    rm64, rv64 = rm0.double().clone(), rv0.double().clone()
    pre = F.batch_norm(y64, rm64, rv64, w64, b64, True, 0.1, 1e-5)
    out = F.leaky_relu(pre, 0.2)
    dy, dw, db = torch.autograd.grad(out, [y64, w64, b64], g64)
    pre = pre.detach()
    band = pre.abs() < E.KINK_BAND * pre.abs().max()
    share = band.double().mean().item()
    note(f"epilogue case: {share:.2e} of the pre-activations in the kink band")
    assert share < E.KINK_SHARE
    stol = 1e-4 + 5e-3
    for s, r in enumerate(R):
        sl = slice(s * N, (s + 1) * N)
        e = relmax(back(r["z"]), out.detach()[sl])
        note(f"epilogue case shard {s} out: max {e:.3e} (tol {tol:.1e})")
        assert e < tol
        check_grad(back(r["dy1"]), dy[sl], ~band[sl], pname, f"epilogue case shard {s} dy")
        er, ev = relmax(r["rm"], rm64), relmax(r["rv"], rv64)
        note(f"epilogue case shard {s} running mean {er:.3e} var {ev:.3e} (tol {stol:.1e})")
        assert er < stol and ev < stol
    ew, eb = relmax(sum(r["dw"] for r in R), dw), relmax(sum(r["db"] for r in R), db)
    note(f"epilogue case dweight {ew:.3e} dbias {eb:.3e} summed over the shards (tol {2 * tol:.1e})")
    assert ew < 2 * tol and eb < 2 * tol
