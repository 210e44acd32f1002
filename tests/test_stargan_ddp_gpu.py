"""GPU: data-parallel stargan-v2 -- ``parallel.attach_ddp(solver)`` + ``Solver.train_iteration`` under the reducer -- against one process
on the global batch (what the reference's nn.DataParallel computes).

Two ranks on cuda:0 over gloo (the test box has one GPU; RCCL refuses two ranks on one device), each holding rows [rank * 2, rank * 2 + 2)
of a global batch of 4, on the sg0 configuration (64², max_conv_dim 64) with DiffAugment ``color,translation,cutout``, lambda_ds > 0
(decaying), beta1 = 0 and coupled weight decay.  The networks get the reference's He initialisation from a seed, not the formula fill:
on that fill the two style codes of the diversity term differ by 1e-6 and the term is rounding noise, and with torch's
default initialisation x_fake and x_fake2 still differ by ~5e-4, so the L1 sign of a percent of the pixels is rounding noise; here every
loss term is a real function of the weights.  The ranks are built from DIFFERENT seeds: attach_ddp must bring rank 1 to rank 0's networks and
CPU RNG state.  The single-process runs are spawned in a process of their own; at most three processes hold the GPU at once."""
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import starganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POLICY = "color,translation,cutout"
GLOBAL, ITERS, SEED = 4, 2, 100
# The two-rank comparison runs with lr = 0: the Adam kernel still forms exp_avg = g * grad_scale + wd * p (beta1 = 0: the last
# effective gradient of each network) but no parameter moves, so every update's exchanged gradient, every reported loss and the EMA
# are compared at the same point and differ by the summation order only.  With moving parameters two correct runs part by percents
# within an iteration at He initialisation (one update changes the sty loss from 0.81 to 0.24, and beta1 = 0 makes Adam a sign step),
# so the moving runs are compared bit for bit instead: the two ranks with each other, and one rank with forced collectives against no
# reducer (the reference's lr).
EXACT_LR = 1e-4
NETS = ("generator", "mapping_network", "style_encoder", "discriminator")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _config(pname, lr):
    cfg = O.Cfg(img_size=64, style_dim=16, latent_dim=8, num_domains=2, max_conv_dim=64)
    args = SimpleNamespace(img_size=64, style_dim=16, latent_dim=8, num_domains=2, max_conv_dim=64, w_hpf=0, norm_type="adain",
                           num_embeds=1, lambda_reg=1.0, lambda_sty=1.0, lambda_ds=1.0, lambda_cyc=1.0, lr=lr, f_lr=lr, beta1=0.0,
                           beta2=0.99, weight_decay=1e-4, compute_dtype=pname, DiffAugment=POLICY, ds_iter=4)
    return cfg, args


def _he_init(net):
    """the reference's initialisation of the trained networks (core/utils.py he_init, applied in core/solver.py): kaiming normal
    (fan_in, relu) conv / linear weights, zero biases; the instance norms keep weight 1, bias 0"""
    with torch.no_grad():
        for m in net.modules():
            w = getattr(m, "weight", None)
            if isinstance(w, torch.nn.Parameter) and w.dim() >= 2:
                torch.nn.init.kaiming_normal_(w, mode="fan_in", nonlinearity="relu")
                if getattr(m, "bias", None) is not None:
                    m.bias.zero_()


def _run(pname, lr, rank, world, seed, attach_kw, path):
    """build from ``seed``, optionally attach the reducer, run ITERS iterations on this rank's rows; save everything compared"""
    from de_i2i_gan_amd.parallel import attach_ddp
    from de_i2i_gan_amd.stargan import Solver, build_model
    cfg, args = _config(pname, lr)
    torch.manual_seed(seed)
    nets, nets_ema = build_model(args)
    for net in vars(nets).values():
        _he_init(net)
    solver = Solver(args, nets, nets_ema, DEV)
    red = attach_ddp(solver, **attach_kw) if attach_kw is not None else None
    consumed = [0]                       # fp32 bytes of the gradients the optimizers' step() calls read

    def counting(opt):
        step = opt.step

        def counted(*a, **k):
            consumed[0] += sum(p.grad.numel() * 4 for g in opt.param_groups for p in g["params"] if p.grad is not None)
            return step(*a, **k)
        return counted

    for opt in vars(solver.optims).values():
        opt.step = counting(opt)
    init = {"nets": {n: {k: v.detach().cpu().clone() for k, v in getattr(nets, n).state_dict().items()} for n in NETS},
            "ema": {n: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()} for n, net in vars(nets_ema).items()}}
    per = GLOBAL // world
    rows = [t[rank * per:(rank + 1) * per].to(DEV) for t in O.synthetic_inputs(cfg, GLOBAL)]
    losses = []
    for _ in range(ITERS):
        out = solver.train_iteration(*rows)
        losses.append({k: dict(vars(v)) for k, v in out.items()})
    torch.cuda.synchronize()
    adam = {}
    for name in NETS:
        opt = getattr(solver.optims, name)
        adam[name] = [(opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu(), opt.state[p]["step"]) if p in opt.state else None
                      for p in getattr(nets, name).parameters()]
    torch.save({"losses": losses, "lambda_ds": args.lambda_ds, "consumed": consumed[0], "stats": dict(red.stats) if red else None,
                "nets": {n: {k: v.cpu() for k, v in getattr(nets, n).state_dict().items()} for n in NETS},
                "ema": {n: {k: v.cpu() for k, v in net.state_dict().items()} for n, net in vars(nets_ema).items()},
                "init": init, "adam": adam, "param_bytes": {n: sum(p.numel() * 4 for p in getattr(nets, n).parameters()) for n in NETS}}, path)


def _single_worker(_, pname, port, out_dir):
    """one process, global batch: without a reducer (lr 0 and EXACT_LR), then attached on a ONE-rank group with force_collectives"""
    _run(pname, 0.0, 0, 1, SEED, None, os.path.join(out_dir, "single.pt"))
    _run(pname, EXACT_LR, 0, 1, SEED, None, os.path.join(out_dir, "plain.pt"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    _run(pname, EXACT_LR, 0, 1, SEED, dict(force_collectives=True), os.path.join(out_dir, "forced.pt"))
    dist.destroy_process_group()


def _rank_worker(rank, world, pname, port, out_dir):
    """at lr 0 (compared with one process) and at EXACT_LR (the ranks must move in lockstep)"""
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    # small thresholds: buckets AND in-place messages
    kw = dict(bucket_bytes=1 << 18, direct_bytes=1 << 16)
    _run(pname, 0.0, rank, world, SEED + rank, kw, os.path.join(out_dir, f"r{rank}.pt"))
    _run(pname, EXACT_LR, rank, world, SEED + rank, kw, os.path.join(out_dir, f"m{rank}.pt"))
    dist.destroy_process_group()


_cache = {}


def _results(pname, tmp_path_factory):
    if pname not in _cache:
        d = tmp_path_factory.mktemp(f"sgddp_{pname}")
        mp.spawn(_single_worker, args=(pname, _free_port(), str(d)), nprocs=1, join=True)
        mp.spawn(_rank_worker, args=(2, pname, _free_port(), str(d)), nprocs=2, join=True)
        _cache[pname] = {k: torch.load(d / f"{k}.pt", weights_only=False) for k in ("single", "plain", "forced", "r0", "r1", "m0", "m1")}
    return _cache[pname]


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _equal_trees(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_equal_trees(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal_trees(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return a == b


# Against the single process on the global batch, at the same parameters: relative L2 per tensor of the last effective gradient
# (exp_avg), with FLOOR x the network's largest as the denominator's floor (a bias in front of an instance norm has a gradient of
# rounding noise; in bf16 the rounding depends on the batch shape), per network, and the relative difference of every reported loss.
# Measured on an MI355X, the same values run to run: f32 exp_avg 3.1e-3 (mapping network), losses 2.1e-6; bf16 exp_avg G 0.32, M 0.21,
# S 0.12, D 0.17, losses 7.9e-3 (the R1 term) -- bf16 kernels round batch 2 and batch 4 differently and the instance norms amplify it
# (the bf16 generator forward sits 0.35 from the fp32 reference in test_starganv2_gpu.py).
FLOOR = {"f32": 1e-3, "bf16": 1e-2}
EXP_AVG = {"f32": dict.fromkeys(NETS, 1e-2),
           "bf16": {"generator": 0.45, "mapping_network": 0.3, "style_encoder": 0.2, "discriminator": 0.25}}
LOSS = {"f32": 1e-5, "bf16": 2e-2}


@pytest.mark.parametrize("pname", ["f32", "bf16"])
def test_two_ranks_compute_what_one_process_computes_on_the_global_batch(pname, tmp_path_factory):
    R = _results(pname, tmp_path_factory)
    one, r0, r1 = R["single"], R["r0"], R["r1"]
    # the ranks end identical: networks, EMA networks, Adam state, reported losses, lambda_ds
    for key in ("nets", "ema", "adam", "losses", "lambda_ds"):
        assert _equal_trees(r0[key], r1[key]), key
    assert r0["lambda_ds"] == one["lambda_ds"] == 0.5
    errs = {"exp_avg": [], "loss": []}
    # exp_avg = (1 - beta1) * (g * grad_scale + wd * p) = the last effective gradient (beta1 = 0): a direct check of the exchanged
    # gradients of D (second D update), G (reference-guided update), M and S (latent update)
    for name in NETS:
        ref = [s for s in one["adam"][name] if s is not None]
        got = [s for s in r0["adam"][name] if s is not None]
        assert len(ref) == len(got) and [s[2] for s in ref] == [s[2] for s in got], name
        scale = max(float(s[0].norm()) for s in ref)
        for i, (g, e) in enumerate(zip(got, ref)):
            denom = max(float(e[0].norm()), FLOOR[pname] * scale)
            errs["exp_avg"].append((float((g[0].double() - e[0].double()).norm()) / denom, name, i))
    # lr = 0: the networks and the EMA networks (lerp of equal values) stay at rank 0's initial point, on every rank and in one process
    for tree in ("nets", "ema"):
        assert _equal_trees(r0[tree], one[tree]) and _equal_trees(r0["init"][tree], one["init"][tree]), tree
    for it in range(ITERS):
        for tag, ns in one["losses"][it].items():
            for k, v in ns.items():
                errs["loss"].append((abs(r0["losses"][it][tag][k] - v) / abs(v), it, tag, k))
    worst = {name: max(e for e in errs["exp_avg"] if e[1] == name) for name in NETS}
    worst["loss"] = max(errs["loss"])
    print(f"\n[stargan ddp {pname}] worst relative errors against one process:", worst)
    for name in NETS:
        assert worst[name][0] < EXP_AVG[pname][name], (worst[name], EXP_AVG[pname][name])
    assert worst["loss"][0] < LOSS[pname], (worst["loss"], LOSS[pname])
    # what travels: exactly the fp32 gradients the five step() calls of each iteration consume -- 2 D + (G + M + S) + G
    pb = r0["param_bytes"]
    per_iter = 2 * pb["discriminator"] + 2 * pb["generator"] + pb["mapping_network"] + pb["style_encoder"]
    for r in (r0, r1):
        assert r["stats"]["bytes"] == r["consumed"] == ITERS * per_iter, (r["stats"], r["consumed"], ITERS * per_iter)


@pytest.mark.parametrize("pname", ["f32", "bf16"])
def test_two_ranks_move_in_lockstep(pname, tmp_path_factory):
    """two iterations at the reference's lr from different seeds: the ranks stay bit-identical -- networks, EMA networks, Adam state,
    losses -- while the parameters move"""
    R = _results(pname, tmp_path_factory)
    m0, m1 = R["m0"], R["m1"]
    for key in ("init", "nets", "ema", "adam", "losses", "lambda_ds"):
        assert _equal_trees(m0[key], m1[key]), key
    moved = [not torch.equal(v, m0["init"]["nets"][n][k]) for n in NETS for k, v in m0["nets"][n].items()]
    assert sum(moved) > 0.9 * len(moved), (sum(moved), len(moved))
    assert not _equal_trees(m0["ema"], m0["init"]["ema"])


@pytest.mark.parametrize("pname", ["f32", "bf16"])
def test_one_rank_with_forced_collectives_is_bit_identical_to_no_reducer(pname, tmp_path_factory):
    """the freezing, the reduce calls, the loss all-reduce and the sharded draw (world 1) change nothing but the exchange"""
    R = _results(pname, tmp_path_factory)
    one, forced = R["plain"], R["forced"]
    for key in ("nets", "ema", "adam", "losses", "lambda_ds"):
        assert _equal_trees(forced[key], one[key]), key
    assert forced["stats"]["collectives"] > 0 and forced["stats"]["bytes"] == forced["consumed"] == one["consumed"]
