"""Time of ops.image_metrics (csrc/metrics.hip: two launches) against the same per-image quantities from torch ops, measured back to
back in the same process on the same device: one JSON line.

    python tools/bench_metrics.py [--shape 16 3 256 256] [--reps 50] [--rounds 7] [--buffers 12]

Columns: ``fused`` (ops.image_metrics, eager calls), ``fused_graph`` (the same calls replayed from one captured graph of ``--reps``
of them: no host time between the launches, the kernels' own rate) and ``torch_ops`` -- the yardstick: a depthwise ``conv2d`` with
the 11 x 11 Gaussian window per moment map (x, y, x^2, y^2, xy), the SSIM formula in element-wise ops and ``.mean()`` reductions
per image for SSIM, the squared and the absolute error.  ``--buffers`` pairs of image batches are used in turn (default 12 x 2 x
12.6 MB, more than the 256 MB last-level cache).  Before anything is timed the two formulations are compared on one pair.  A round
times ``--reps`` calls of every column in turn between two device events; the figure is the median over ``--rounds`` rounds, the
spread their min and max.  ``TB_per_s`` is bytes read (x and y once: what the fused kernel needs) over the time, to hold against
the HBM rate of MI355X_MICROARCH.md (8.0 TB/s peak, 6.29 TB/s measured for a float4 copy)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda:0"
HBM_TB_PER_S = {"peak": 8.0, "float4_copy": 6.29}


def torch_metrics(x, y, window, data_range=2.0):
    """-> (N, 3): per image the mean squared error, the mean absolute error and the mean SSIM, from torch ops"""
    c = x.shape[1]
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = F.conv2d(x, window, groups=c), F.conv2d(y, window, groups=c)
    vx = F.conv2d(x * x, window, groups=c) - mx * mx
    vy = F.conv2d(y * y, window, groups=c) - my * my
    cxy = F.conv2d(x * y, window, groups=c) - mx * my
    ssim = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    d = x - y
    return torch.stack([(d * d).mean(dim=(1, 2, 3)), d.abs().mean(dim=(1, 2, 3)), ssim.mean(dim=(1, 2, 3))], 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=4, default=[16, 3, 256, 256], metavar=("N", "C", "H", "W"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--buffers", type=int, default=12)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs a GPU (the HIP path has no CPU fallback)")
    from de_i2i_gan_amd import ops
    n, c, h, w = opts.shape
    torch.cuda.set_device(0)
    gen = torch.Generator().manual_seed(1)
    xs = [(torch.rand(n, c, h, w, generator=gen) * 2 - 1).to(DEV) for _ in range(opts.buffers)]
    ys = [(x + 0.1 * torch.randn(n, c, h, w, generator=gen).to(DEV)).clamp(-1, 1) for x in xs]
    g = torch.exp(-(torch.arange(11, dtype=torch.float64) - 5) ** 2 / (2 * 1.5 ** 2))
    g = g / g.sum()
    window = torch.outer(g, g).float().expand(c, 1, 11, 11).contiguous().to(DEV)

    sums, ref = ops.image_metrics(xs[0], ys[0]), torch_metrics(xs[0], ys[0], window).double()      # the yardstick computes the same
    elems, positions = c * h * w, c * (h - 10) * (w - 10)
    got = torch.stack([sums[:, 0] / elems, sums[:, 1] / elems, sums[:, 5] / positions], 1)
    worst = ((got - ref).abs() / ref.abs().clamp_min(1e-6)).max().item()
    assert worst < 1e-3, f"image_metrics and the torch-op formulation disagree (relative {worst:.2e})"

    columns = {"fused": lambda i: ops.image_metrics(xs[i], ys[i]), "torch_ops": lambda i: torch_metrics(xs[i], ys[i], window)}
    for fn in columns.values():                              # warm-up: every column on every buffer pair
        for i in range(opts.buffers):
            fn(i)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = [columns["fused"](i % opts.buffers) for i in range(opts.reps)]
    graph.replay()
    torch.cuda.synchronize()

    def eager(fn):
        def run():
            for i in range(opts.reps):
                fn(i % opts.buffers)
        return run

    runs = {"fused": eager(columns["fused"]), "fused_graph": graph.replay, "torch_ops": eager(columns["torch_ops"])}
    times = {name: [] for name in runs}
    for _ in range(opts.rounds):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / opts.reps)
    del held
    nbytes = 2 * 4 * n * c * h * w
    res = {name: {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                  "TB_per_s": round(nbytes / statistics.median(v) / 1e6, 3)} for name, v in times.items()}
    print(json.dumps({"workload": "ops.image_metrics against torch ops", "device": torch.cuda.get_device_name(0), "shape": opts.shape,
                      "bytes_read": nbytes, "reps": opts.reps, "rounds": opts.rounds, "buffers": opts.buffers,
                      "hbm_TB_per_s": HBM_TB_PER_S, "agreement_relative": worst, "columns": res,
                      "torch_ops_over_fused": round(statistics.median(times["torch_ops"]) / statistics.median(times["fused"]), 2)}))


if __name__ == "__main__":
    main()
