"""What synchronised BatchNorm (parallel.attach_ddp(..., sync_bn=True)) costs on ONE GPU: the reducer on a one-rank RCCL group with forced
collectives, the same D+G steps timed with the mode off and with it on, in the same process; plus the statistics messages per step
(GradReducer.stats).  A comparison of two runs of this script's own loop -- not bench.py's number, and no statement about N > 1:
on one rank the all-reduces move nothing over xGMI, what is priced is the three-stage finalize and the per-layer host work.

    python tools/bench_sync_bn.py [--stage defectgan|mae] [--dtype bf16|f32] [--image-size 256] [--batch 16] [--steps 10] [--warmup 3]
prints one JSON line."""
import argparse
import json
import os
import socket
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", default="defectgan", choices=["defectgan", "mae"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import torch.distributed as dist
    import bench
    from de_i2i_gan_amd.parallel import attach_ddp
    device = "cuda:0"
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
    sk.close()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(device))
    bg, lab, df = (t.to(device) for t in bench.synthetic_batch(args.batch, args.image_size, seed=7))
    out = {"stage": args.stage, "dtype": args.dtype, "image_size": args.image_size, "batch": args.batch, "steps": args.steps, "ranks": 1}
    for sync_bn in (False, True):
        torch.manual_seed(123)
        if args.stage == "mae":
            from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer
            tr = MAETrainer(bench.make_opt(args, device))
            step = lambda: tr.step(bg, lab)                      # noqa: E731
        else:
            from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
            tr = DefectGanTrainer(bench.make_opt(args, device))
            step = lambda: tr.step(bg, lab, df)                  # noqa: E731
        red = attach_ddp(tr, force_collectives=True, sync_bn=sync_bn)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        before = dict(red.stats)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / args.steps
        per = {k: (red.stats[k] - before[k]) / args.steps for k in ("collectives", "bytes", "sync_bn_collectives", "sync_bn_bytes")}
        out["sync_bn_on" if sync_bn else "sync_bn_off"] = dict(ms_per_step=round(ms, 3), **per)
        del tr, red, step
    out["sync_bn_cost_ms_per_step"] = round(out["sync_bn_on"]["ms_per_step"] - out["sync_bn_off"]["ms_per_step"], 3)
    out["note"] = "one-rank RCCL group, forced collectives: the same loop with sync_bn off and on; no multi-GPU traffic is measured"
    dist.destroy_process_group()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
