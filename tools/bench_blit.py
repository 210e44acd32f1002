"""Kernel rate of dei2i_blit (csrc/blit.hip) per code class on one fp32 NCHW batch, against same-byte yardsticks on the same device in
the same process: one JSON line.

    python tools/bench_blit.py [--shape 16 3 256 256] [--reps 500] [--rounds 5] [--buffers 12] [--naive-lib PATH]

Columns: ``blit_even_k`` (codes 0, 1, 4, 5: row copies), ``blit_odd_k`` (codes 2, 3, 6, 7: LDS-tiled transposes), ``blit_mixed`` (the
eight codes in turn), ``naive_even_k`` / ``naive_odd_k`` (tools/microbench/blit_naive.hip: one thread per output pixel, a plain
gather), ``clone`` (torch's copy of the tensor) and ``translation`` (the existing dei2i_diffaug launch of a translation-only run).
Every column reads and writes the tensor once.  ``--buffers`` source / destination pairs are used in turn (default 12 x 2 x 12.6 MB,
more than the 256 MB last-level cache) so that the figures are memory rates; ``--buffers 1`` gives the cache-resident rate.  A round
times one replay of a captured graph of ``--reps`` launches (no host time between them) of every column in turn between two events; the figure is the median over ``--rounds`` rounds, the
spread their min and max.  Before anything is timed the naive kernel's output is compared with dei2i_blit's for all eight codes,
both directions.  Without ``--naive-lib`` the yardstick is compiled with hipcc into a temporary directory."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

DEV = "cuda:0"


def naive_library(path):
    if path is None:
        path = os.path.join(tempfile.mkdtemp(), "libblit_naive.so")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", path,
                               os.path.join(REPO, "tools", "microbench", "blit_naive.hip")])
    lib = ctypes.CDLL(path)
    lib.blit_naive.restype = ctypes.c_int
    lib.blit_naive.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=4, default=[16, 3, 256, 256], metavar=("N", "C", "H", "W"))
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--buffers", type=int, default=12)
    ap.add_argument("--naive-lib", dest="naive_lib", default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_blit.py needs a GPU (the HIP path has no CPU fallback)")
    from de_i2i_gan_amd import ops
    n, c, h, w = opts.shape
    torch.cuda.set_device(0)
    lib, naive, st, p = ops._lib_for(torch.zeros(1, device=DEV)), naive_library(opts.naive_lib), ops._stream, ops._p
    gen = torch.Generator().manual_seed(1)
    srcs = [torch.rand(n, c, h, w, generator=gen).to(DEV) for _ in range(opts.buffers)]
    dsts = [torch.empty_like(s) for s in srcs]

    def codes(values):
        return torch.tensor([values[i % len(values)] for i in range(n)], dtype=torch.int32, device=DEV)

    even, odd, mixed = codes([0, 1, 4, 5]), codes([2, 3, 6, 7]), codes(list(range(8)))
    for inverse in (0, 1):                                   # the yardstick computes the same map
        want, got = torch.empty_like(srcs[0]), torch.empty_like(srcs[0])
        assert lib.dei2i_blit(n, c, h, w, p(mixed), inverse, p(srcs[0]), p(want), st()) == 0
        assert naive.blit_naive(n, c, h, w, mixed.data_ptr(), inverse, srcs[0].data_ptr(), got.data_ptr(), st()) == 0
        torch.cuda.synchronize()
        assert torch.equal(want, got), "blit_naive and dei2i_blit disagree"
    tab = torch.zeros(n, 8, dtype=torch.int32, device=DEV)      # translation-only records: a = 1, ty = tx = the largest shift
    tab.view(torch.float32)[:, 0] = 1.0
    tab[:, 4], tab[:, 5] = int(h * 0.125 + 0.5), -int(w * 0.125 + 0.5)

    def blit(table):
        return lambda s, d: lib.dei2i_blit(n, c, h, w, p(table), 0, p(s), p(d), st())

    def gather(table):
        return lambda s, d: naive.blit_naive(n, c, h, w, table.data_ptr(), 0, s.data_ptr(), d.data_ptr(), st())

    columns = {"blit_even_k": blit(even), "blit_odd_k": blit(odd), "blit_mixed": blit(mixed), "naive_even_k": gather(even),
               "naive_odd_k": gather(odd), "clone": lambda s, d: d.copy_(s),
               "translation": lambda s, d: lib.dei2i_diffaug(0, n, c, h, w, 0, 0, 0, p(s), p(tab), None, p(d), st())}
    for fn in columns.values():                              # warm-up: every column on every buffer pair
        for s, d in zip(srcs, dsts):
            fn(s, d)
    torch.cuda.synchronize()
    graphs = {}
    for name, fn in columns.items():                         # one graph of --reps launches per column: no host time between them
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for i in range(opts.reps):
                fn(srcs[i % opts.buffers], dsts[i % opts.buffers])
        graphs[name].replay()
    torch.cuda.synchronize()
    times = {name: [] for name in columns}
    for _ in range(opts.rounds):
        for name in columns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name].replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / opts.reps)
    nbytes = 2 * 4 * n * c * h * w
    res = {name: {"us": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                  "TB_per_s": round(nbytes / statistics.median(v) / 1e6, 3)} for name, v in times.items()}
    print(json.dumps({"workload": "dei2i_blit kernel rate", "device": torch.cuda.get_device_name(0), "shape": opts.shape,
                      "bytes_per_launch": nbytes, "reps": opts.reps, "rounds": opts.rounds, "buffers": opts.buffers, "columns": res}))


if __name__ == "__main__":
    main()
