"""stargan-v2 throughput: eager ``Solver.train_iteration`` (two D updates, two G updates, EMA) on one GPU, one JSON line.

Setup: the reference's AFHQ settings (img_size 256, 3 domains, style_dim 64, latent_dim 16, max_conv_dim 512, lambda_reg / sty / ds /
cyc 1, w_hpf 0, lr 1e-4, f_lr 1e-6, Adam (0, 0.99), weight decay 1e-4), batch 8 per GPU, bf16, with DiffAugment
``color,translation,cutout`` and with it empty.  Each iteration is timed host-side between device synchronisations (the iteration
reads its losses back four times anyway); the line carries the median ms per iteration and images/s after the warm-up.

``--force-collectives``: each configuration is also run with ``parallel.attach_ddp(solver, force_collectives=True)`` on a ONE-rank
RCCL group (as ``bench.py --gpus 1 --force-collectives`` does for defectGAN): hooks, buckets, the side-stream all-reduces and the loss
all-reduce at full size, no xGMI traffic.  Reported: collectives and MB per iteration and the time difference against the same
iterations without the reducer, in the same process (timed without the reducer's event brackets; the side-stream spans come from
--measure-steps further iterations).

    python tools/bench_stargan.py [--steps 10] [--warmup 3] [--batch 8] [--dtype bf16] [--force-collectives]
"""
import argparse
import json
import os
import socket
import statistics
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

POLICIES = ("color,translation,cutout", "")


def afhq_args(img_size, dtype, policy):
    return SimpleNamespace(img_size=img_size, style_dim=64, latent_dim=16, num_domains=3, max_conv_dim=512, w_hpf=0, norm_type="adain",
                           num_embeds=1, lambda_reg=1.0, lambda_sty=1.0, lambda_ds=1.0, ds_iter=100000, lambda_cyc=1.0, lr=1e-4,
                           f_lr=1e-6, beta1=0.0, beta2=0.99, weight_decay=1e-4, compute_dtype=dtype, DiffAugment=policy)


def batch(args, n, device):
    g = torch.Generator().manual_seed(7)
    img = lambda: (torch.rand(n, 3, args.img_size, args.img_size, generator=g) * 2 - 1).to(device)      # noqa: E731
    y_org = torch.randint(0, args.num_domains, (n,), generator=g).to(device)
    y_trg = torch.randint(0, args.num_domains, (n,), generator=g).to(device)
    z = lambda: torch.randn(n, args.latent_dim, generator=g).to(device)                                 # noqa: E731
    return img(), y_org, y_trg, img(), img(), z(), z()


def run(opts, policy, reducer_kw, device):
    """median ms per iteration of a fresh Solver (optionally with the reducer attached) after the warm-up"""
    from de_i2i_gan_amd.parallel import attach_ddp
    from de_i2i_gan_amd.stargan import Solver, build_model
    args = afhq_args(opts.img_size, opts.dtype, policy)
    torch.manual_seed(0)
    nets, nets_ema = build_model(args)
    solver = Solver(args, nets, nets_ema, device)
    red = attach_ddp(solver, **reducer_kw) if reducer_kw is not None else None
    inputs = batch(args, opts.batch, device)
    for _ in range(opts.warmup):
        solver.train_iteration(*inputs)
    torch.cuda.synchronize()
    before = dict(red.stats) if red is not None else None
    times = []
    for _ in range(opts.steps):
        t0 = time.perf_counter()
        out = solver.train_iteration(*inputs)
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    ms = statistics.median(times)
    overlap = None
    if red is not None:
        # the collectives' side-stream spans, from extra iterations after the timed ones (measure=True adds a wait and two events per
        # collective: not in the timed region)
        red.measure = True
        for _ in range(opts.measure_steps):
            solver.train_iteration(*inputs)
        torch.cuda.synchronize()
        overlap = red.overlap_report()
    res = {"diffaug": policy, "ms_per_iter": round(ms, 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
           "images_per_s": round(opts.batch * 1e3 / ms, 2),
           "losses_last": {k: {n: round(v, 6) for n, v in vars(ns).items()} for k, ns in out.items()}}
    if red is not None:
        res["ddp"] = {"collectives_per_iter": (red.stats["collectives"] - before["collectives"]) / (opts.steps + opts.measure_steps),
                      "MB_per_iter": round((red.stats["bytes"] - before["bytes"]) / (opts.steps + opts.measure_steps) / 2 ** 20, 2),
                      "overlap": overlap, "overlap_iterations": opts.measure_steps}
    del solver, nets, nets_ema, red
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU")
    ap.add_argument("--img-size", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--diffaug", action="append", default=None,
                    help="DiffAugment policy to time (repeatable; '' = none); default: color,translation,cutout and none")
    ap.add_argument("--measure-steps", type=int, default=3,
                    help="--force-collectives: untimed iterations after the timed ones that record the collectives' stream spans")
    ap.add_argument("--force-collectives", action="store_true",
                    help="also run every configuration with the data-parallel reducer attached on a one-rank RCCL group")
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stargan.py needs a GPU (the HIP path has no CPU fallback)")
    device = "cuda:0"
    torch.cuda.set_device(0)
    if opts.force_collectives:
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
        sk.close()
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(device))
    runs = []
    for policy in (opts.diffaug if opts.diffaug is not None else POLICIES):
        res = run(opts, policy, None, device)
        if opts.force_collectives:
            red = run(opts, policy, dict(force_collectives=True), device)
            res["ddp"] = dict(red["ddp"], ranks=1, ms_per_iter_with_reducer=red["ms_per_iter"],
                              reducer_cost_ms_per_iter=round(red["ms_per_iter"] - res["ms_per_iter"], 3),
                              note="one-rank RCCL group (--force-collectives): the reducer's host and stream work at full size, "
                                   "no xGMI traffic")
        runs.append(res)
        print("[bench_stargan]", json.dumps(res), file=sys.stderr, flush=True)
    print(json.dumps({"workload": "stargan-v2 Solver.train_iteration (eager)", "device": torch.cuda.get_device_name(0),
                      "gpus": 1, "img_size": opts.img_size, "batch_per_gpu": opts.batch, "dtype": opts.dtype, "steps": opts.steps,
                      "warmup": opts.warmup, "runs": runs}))
    if opts.force_collectives:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
