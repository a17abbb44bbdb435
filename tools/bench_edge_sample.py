#!/usr/bin/env python3
"""Device time of edgegaussians_amd.edges.sample: HIP events around the call (which ends in its one read-back and the
emission), a warm-up, the median of --reps repetitions.

    python tools/bench_edge_sample.py [--reps 50] [--cpu-ms-synthetic X] [--cpu-ms-mixed Y] [--out FILE]

Inputs: 200 seeded curves + 200 seeded lines in the unit cube at 0.005, and the mixed case of
tests/golden/edge_sampling.npz.  The reference function's CPU time on the same inputs is measured where the reference
exists and passed in with --cpu-ms-*; this tool never imports it (blank when not given).
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic(n_curves=200, n_lines=200, seed=0):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.3, 0.7, (n_curves, 1, 3))
    return centre + rng.uniform(-0.3, 0.3, (n_curves, 4, 3)), rng.uniform(0.0, 1.0, (n_lines, 2, 3))


def time_sample(edges, pair, reps, warmup=5):
    for _ in range(warmup):
        pts, _ = edges.sample(pair, 0.005)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pts, _ = edges.sample(pair, 0.005)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms), int(pts.shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--cpu-ms-synthetic", type=float, default=None)
    ap.add_argument("--cpu-ms-mixed", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20
    from edgegaussians_amd import edges
    g = np.load(os.path.join(ROOT, "tests", "golden", "edge_sampling.npz"))
    cases = [("200 curves + 200 lines", synthetic(), args.cpu_ms_synthetic),
             ("fixture mixed case (7 curves + 7 lines)", (g["mixed_curves"], g["mixed_lines"]), args.cpu_ms_mixed)]
    lines = [f"edges.sample at 0.005 on {torch.cuda.get_device_name(0)}: HIP events around the whole call (upload, count, "
             f"read-back of the total, emission), median of {args.reps} after 5 warm-up calls",
             f"{'case':42s} {'samples':>8s} {'median ms':>10s} {'min':>8s} {'max':>8s} {'reference on the CPU, ms':>26s}"]
    for name, pair, cpu in cases:
        med, lo, hi, n = time_sample(edges, pair, args.reps)
        lines.append(f"{name:42s} {n:8d} {med:10.3f} {lo:8.3f} {hi:8.3f} {'' if cpu is None else format(cpu, '26.1f'):>26s}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
