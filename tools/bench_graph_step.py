"""defectGAN (or, ``--stage mae``, MAE pre-training) step time with the recipe options, eager against ``opt.graph_step``, in one
process: one JSON line.

Setup: the trainer of ``bench.py``'s defaults (256x256, batch 16, bf16, its synthetic batch and seed) with the given option set,
once per requested mode.  After the warm-up (which, in graph mode, covers the eager warm-up calls and the capture) ``--steps``
steps are enqueued back to back with nothing awaited, an event recorded after each: ``ms_per_step`` is the median distance of
consecutive events (the rate the device finishes steps at, whichever of host and GPU bounds it), ``host_enqueue_ms`` the median
host time of a ``step()`` call, ``wall_ms_per_step`` the whole timed region divided by the steps.

    python tools/bench_graph_step.py --use-spectral --add-noise --diff-aug color,translation,cutout --diff-aug-rng device \\
        [--mode eager --mode graph] [--steps 20] [--warmup 8]

    python tools/bench_graph_step.py --stage mae --mask-rng device [--mode eager --mode graph]

    python tools/bench_graph_step.py --ema-beta 0.999 [--ema-start-iter N]

    python tools/bench_graph_step.py --max-grad-norm 1.0 --clip off --clip torch --clip fused [--repeat 2]

    python tools/bench_graph_step.py --sean --use-spectral --add-noise --embed-rng host --embed-rng device [--repeat 2]

``--diff-aug-rng host`` draws DiffAugment's parameters on the host like the reference (graph mode refuses it), ``device`` on the
GPU (``ops.DiffAugRng``).  ``--stage mae`` runs ``MAETrainer`` (bench.py's MAE option set) on the background batch and its labels;
``--mask-rng host`` draws its patch masks on the host like the reference (graph mode refuses it), ``device`` on the GPU
(``ops.mask_draw``).  ``--ema-beta B`` keeps the EMA copies of the generator side (``opt.ema_beta``: one more multi-tensor launch and the
buffer copies per G update), averaging from the first update unless ``--ema-start-iter`` delays it.  ``--clip`` (repeatable) is how
``--max-grad-norm X`` is applied: ``fused`` is ``opt.max_grad_norm`` (the norm and the clip inside the fused Adam, eager or captured),
``torch`` is what a user would write without it -- ``torch.nn.utils.clip_grad_norm_(params, X, foreach=True)`` right before every
``optimizer.step()``, eager only --, ``off`` no clipping.  Every (clip, mode) pair is one column; ``--repeat N`` runs the columns N
times in turn, so that a run shows its own spread.  ``--sean`` is the README's SEAN recipe: ``style_norm_block_type = "sean"`` on a
synthetic embeddings file (``--embeds-per-label`` N(0, 1) embeddings of ``embed_nc`` = 768 for every label combination with one or two
labels set, ``--num-embeds`` drawn per sample); ``--embed-rng`` (repeatable) is where they are drawn: ``host`` with python's
``random.choices`` like the reference (eager only: graph mode refuses it), ``device`` on the GPU (``ops.embed_draw``)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402


def clip_before_step(optimizer, max_norm):
    """the yardstick: clip_grad_norm_ over the optimizer's parameters right before each of its steps"""
    params = [p for group in optimizer.param_groups for p in group["params"]]
    step = optimizer.step

    def clipped_step(*args, **kwargs):
        torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], max_norm, foreach=True)
        return step(*args, **kwargs)
    optimizer.step = clipped_step


def synthetic_embeddings_file(opts):
    """{label tuple: [embedding (768,), ...]} for the combinations with one or two labels set, as a file -> its path"""
    import itertools
    import tempfile
    from pathlib import Path
    g = torch.Generator().manual_seed(99)
    emb = {}
    for key in itertools.product((0, 1), repeat=6):
        emb[key] = list(torch.randn(opts.embeds_per_label, 768, generator=g).unbind(0)) if 1 <= sum(key) <= 2 else []
    path = Path(tempfile.mkdtemp()) / "embeds.pth"
    torch.save(emb, path)
    return path


def run(opts, mode, device, clip="off", embed_rng=None):
    from de_i2i_gan_amd.trainers.defectgan_trainer import DefectGanTrainer
    from de_i2i_gan_amd.trainers.mae_trainer import MAETrainer
    mae = opts.stage == "mae"
    opt = bench.make_opt(opts, device)
    opt.diff_aug = opts.diff_aug
    if opts.diff_aug_rng is not None:
        opt.diff_aug_rng = opts.diff_aug_rng
        opt.diff_aug_seed = opts.diff_aug_seed
    if opts.diff_aug_p is not None:
        opt.diff_aug_p = opts.diff_aug_p
    if opts.ada_target:
        opt.ada_target = opts.ada_target
    if opts.mask_rng is not None:
        opt.mask_rng = opts.mask_rng
        opt.mask_seed = opts.mask_seed
    if opts.ema_beta:
        opt.ema_beta, opt.ema_start_iter = opts.ema_beta, opts.ema_start_iter
    if opts.sean:
        opt.style_norm_block_type, opt.num_embeds, opt.embed_path = "sean", opts.num_embeds, opts.embed_path
        opt.embed_rng, opt.embed_seed = embed_rng, opts.embed_seed
    if clip == "fused":
        opt.max_grad_norm = opts.max_grad_norm
    if mode == "graph":
        opt.graph_step, opt.graph_warmup = True, 3
    torch.manual_seed(123)
    tr = (MAETrainer if mae else DefectGanTrainer)(opt)
    if clip == "torch":          # (after the MAE trainer has added the mask token's group)
        for optimizer in tr.optimizers.values():
            clip_before_step(optimizer, opts.max_grad_norm)
    bg, lab, df = (t.to(device) for t in bench.synthetic_batch(opts.batch, opts.image_size, seed=7))
    inputs = (bg, lab) if mae else (bg, lab, df)
    for _ in range(opts.warmup):
        tr.step(*inputs)
    torch.cuda.synchronize()
    events = [torch.cuda.Event(enable_timing=True) for _ in range(opts.steps + 1)]
    host = []
    events[0].record()
    t_start = time.perf_counter()
    for i in range(opts.steps):
        t0 = time.perf_counter()
        tr.step(*inputs)
        host.append(1e3 * (time.perf_counter() - t0))
        events[i + 1].record()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t_start) / opts.steps
    gaps = [events[i].elapsed_time(events[i + 1]) for i in range(opts.steps)]
    tr.flush_losses()
    res = {"mode": mode, "clip": clip, "embed_rng": embed_rng, "ms_per_step": round(statistics.median(gaps), 3), "ms_min": round(min(gaps), 3), "ms_max": round(max(gaps), 3),
           "wall_ms_per_step": round(wall, 3), "host_enqueue_ms": round(statistics.median(host), 3),
           "graphs": len(tr._graphs.graphs) if tr._graphs is not None else 0,
           "d_gan_last": round(tr.losses["gan"]["D"][-1], 6)}
    if clip == "fused":
        res["grad_norm_last"] = {name: round(v[-1], 6) for name, v in tr.losses["grad_norm"].items()}
    tr.release_graphs()
    del tr
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=20, help="timed steps (at least 20: the figure is a median)")
    ap.add_argument("--warmup", type=int, default=8, help="untimed steps before them (graph mode: 3 eager calls and the capture are among them)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--stage", default="defectgan", choices=["defectgan", "mae"], help="mae: MAETrainer.step on (bg, labels)")
    ap.add_argument("--mask-rng", dest="mask_rng", default=None, choices=["host", "device"], help="--stage mae: where the masks are drawn")
    ap.add_argument("--mask-seed", dest="mask_seed", type=int, default=4321)
    ap.add_argument("--use-spectral", dest="use_spectral", action="store_true")
    ap.add_argument("--add-noise", dest="add_noise", action="store_true")
    ap.add_argument("--diff-aug", dest="diff_aug", default="", metavar="POLICY", help="e.g. color,translation,cutout ('' = none)")
    ap.add_argument("--diff-aug-rng", dest="diff_aug_rng", default=None, choices=["host", "device"])
    ap.add_argument("--diff-aug-seed", dest="diff_aug_seed", type=int, default=1234)
    ap.add_argument("--diff-aug-p", dest="diff_aug_p", type=float, default=None, help="opt.diff_aug_p (needs --diff-aug-rng device)")
    ap.add_argument("--ada-target", dest="ada_target", type=float, default=None, help="opt.ada_target (the controller; 0 / absent = off)")
    ap.add_argument("--ema-beta", dest="ema_beta", type=float, default=0.0, help="opt.ema_beta (0 = no EMA, the default)")
    ap.add_argument("--ema-start-iter", dest="ema_start_iter", type=int, default=0, help="opt.ema_start_iter")
    ap.add_argument("--max-grad-norm", dest="max_grad_norm", type=float, default=None, help="the global gradient norm --clip torch / fused clip to")
    ap.add_argument("--clip", action="append", default=None, choices=["off", "torch", "fused"],
                    help="repeatable; how --max-grad-norm is applied (torch: clip_grad_norm_ before every optimizer.step, eager only; "
                         "fused: opt.max_grad_norm); default: off")
    ap.add_argument("--sean", action="store_true", help="the SEAN generator on a synthetic embeddings file (the README's SEAN recipe with --use-spectral --add-noise)")
    ap.add_argument("--embed-rng", dest="embed_rng", action="append", default=None, choices=["host", "device"],
                    help="--sean, repeatable: where the style embeddings are drawn (host: eager only); default: host")
    ap.add_argument("--embed-seed", dest="embed_seed", type=int, default=5678)
    ap.add_argument("--num-embeds", dest="num_embeds", type=int, default=3, help="--sean: embeddings drawn per sample")
    ap.add_argument("--embeds-per-label", dest="embeds_per_label", type=int, default=64, help="--sean: embeddings stored per label combination")
    ap.add_argument("--repeat", type=int, default=1, help="run every (clip, mode) column this many times, in turn")
    ap.add_argument("--mode", action="append", default=None, choices=["eager", "graph"], help="repeatable; default: eager, then graph")
    opts = ap.parse_args()
    if opts.steps < 20:
        ap.error("--steps must be >= 20")
    if opts.warmup < 5:
        ap.error("--warmup must be >= 5 (graph mode warms up and captures inside it)")
    if not torch.cuda.is_available():
        raise SystemExit("bench_graph_step.py needs a GPU (the HIP path has no CPU fallback)")
    clips = opts.clip or ["off"]
    if any(c != "off" for c in clips) and not (opts.max_grad_norm and opts.max_grad_norm > 0):
        ap.error("--clip torch / fused need --max-grad-norm X with X > 0")
    # (clip_grad_norm_ between backward and step is host code a capture would freeze: the yardstick is eager only)
    if opts.embed_rng and not opts.sean:
        ap.error("--embed-rng needs --sean")
    draws = (opts.embed_rng or ["host"]) if opts.sean else [None]
    # (... and so are host-drawn style embeddings: graph mode refuses them)
    columns = [(c, m, e) for e in draws for c in clips for m in (opts.mode or ["eager", "graph"])
               if not (c == "torch" and m == "graph") and not (e == "host" and m == "graph")]
    if not columns or opts.repeat < 1:
        ap.error("nothing to run (--clip torch and --embed-rng host are eager only)")
    torch.cuda.set_device(0)
    opts.embed_path = synthetic_embeddings_file(opts) if opts.sean else None
    runs = []
    for _ in range(opts.repeat):
        for clip, mode, embed_rng in columns:
            res = run(opts, mode, "cuda:0", clip, embed_rng)
            runs.append(res)
            print("[bench_graph_step]", json.dumps(res), file=sys.stderr, flush=True)
    print(json.dumps({"workload": "MAE-GAN MAETrainer.step" if opts.stage == "mae" else "defectGAN DefectGanTrainer.step", "device": torch.cuda.get_device_name(0), "image_size": opts.image_size,
                      "batch": opts.batch, "dtype": opts.dtype, "use_spectral": opts.use_spectral, "add_noise": opts.add_noise,
                      "diff_aug": opts.diff_aug, "diff_aug_rng": opts.diff_aug_rng or "host", "mask_rng": opts.mask_rng or "host", "sean": opts.sean, "ema_beta": opts.ema_beta,
                      "ema_start_iter": opts.ema_start_iter, "max_grad_norm": opts.max_grad_norm, "steps": opts.steps,
                      "warmup": opts.warmup, "runs": runs}))


if __name__ == "__main__":
    main()
