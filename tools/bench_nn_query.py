#!/usr/bin/env python3
"""Median time of the cross-set nearest-neighbour search (`metrics.nearest`) on uniform and clustered clouds, beside the
existing self-search on the same target cloud (`regularizers.knn(targets, 1, method="grid")`) and `torch.cdist(...).min()`
both ways where its matrix fits.  Device events round every call, warm-up first, clocks as found.

    python tools/bench_nn_query.py > profiles/nn_query_timing.txt
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((3000, 4000), (5000, 5000), (8000, 8000), (12000, 12000), (3000, 40000), (10000, 70000), (100000, 100000),
         (500000, 500000))
CDIST_MAX_BYTES = 8 << 30


def clustered(n, g):
    """Points along a few segments + faint floaters through the volume (what a trained model looks like)."""
    t = torch.rand(n, 1, generator=g)
    seg = torch.randint(0, 6, (n,), generator=g)
    a, b = torch.rand(6, 3, generator=g), torch.rand(6, 3, generator=g)
    pts = a[seg] * (1 - t) + b[seg] * t + 0.003 * torch.randn(n, 3, generator=g)
    pts[n // 2:] = torch.rand(n - n // 2, 3, generator=g) * 1.3 - 0.15
    return pts


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main():
    from edgegaussians_amd import metrics, regularizers
    print(f"# {torch.cuda.get_device_name(0)}; median ms per call, device events, warm-up 5, 50 calls (10 above 10^10 pairs)")
    print(f"{'cloud':10s} {'Q':>7s} {'M':>7s} {'grid':>9s} {'exhaustive':>11s} {'self-knn K=1 (M)':>17s} {'cdist+min x2':>13s}")
    for kind in ("uniform", "clustered"):
        for Q, M in SIZES:
            g = torch.Generator().manual_seed(Q + M)
            make = (lambda n: torch.rand(n, 3, generator=g)) if kind == "uniform" else (lambda n: clustered(n, g))
            qs, ts = make(Q).cuda(), make(M).cuda()
            reps = 50 if Q * M <= 10 ** 10 else 10
            grid = median_ms(lambda: metrics.nearest(qs, ts, method="grid"), 5, reps)
            exh = median_ms(lambda: metrics.nearest(qs, ts, method="exhaustive"), 2 if reps == 10 else 5, reps)
            self_knn = median_ms(lambda: regularizers.knn(ts, 1, method="grid"), 5, 50)
            cd = "-"
            if Q * M * 4 <= CDIST_MAX_BYTES:
                def both():
                    d = torch.cdist(qs, ts)
                    return d.min(1).values, d.min(0).values
                cd = f"{median_ms(both, 3, 10):.3f}"
            print(f"{kind:10s} {Q:7d} {M:7d} {grid:9.3f} {exh:11.3f} {self_knn:17.3f} {cd:>13s}", flush=True)


if __name__ == "__main__":
    main()
