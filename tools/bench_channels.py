"""Forward + backward time of ONE `rasterization` call on colours of D channels, next to the same render done three
channels at a time (ceil(D / 3) calls and a torch.cat: projection, binning, the sort and every alpha evaluation repeated
per call), which is the only way to get it without the wide compositing kernels.

    python tools/bench_channels.py [--gaussians 30000] [--size 512] [--steps 50] [--warmup 10] [--widths 4 8 16 32 64]

Prints one JSON line per width; times are HIP-event milliseconds per call over a window of `--steps` calls after
`--warmup` untimed ones, the colours requiring grad.  `bwd_ms` is the share of `loss.backward()` inside `one_call_ms`.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK = 32  # gsplat's default channel_chunk, and the widest single launch


def _window(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=30000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--widths", type=int, nargs="+", default=[4, 8, 16, 32, 64])
    args = ap.parse_args()

    from edgegaussians_amd import rasterization, synth
    dev = torch.device("cuda")
    sc = synth.make_scene(args.gaussians, 1, args.size, args.size, seed=0, anisotropy=5.0, spread_opacity=True)
    N = sc.means.shape[0]
    params = [t.to(dev).requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    vm, Ks = sc.viewmats[:1].to(dev), sc.Ks[:1].to(dev)
    g = torch.Generator().manual_seed(1)

    def render(col, **kw):
        return rasterization(params[0], params[1], torch.exp(params[2]), torch.sigmoid(params[3]).squeeze(-1), col, vm, Ks,
                             args.size, args.size, packed=False, **kw)

    for D in args.widths:
        colors = (0.2 + 0.8 * torch.rand(N, D, generator=g)).to(dev).requires_grad_(True)
        wr = torch.rand(1, args.size, args.size, D, generator=g).to(dev)
        bwd_ms = [0.0]

        def clear():
            for t in params + [colors]:
                t.grad = None

        def one_call():
            clear()
            r, a, _ = render(colors, channel_chunk=CHUNK)
            loss = (r * wr).sum() + a.sum()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss.backward()
            e1.record()
            events.append((e0, e1))

        def three_at_a_time():
            clear()
            parts, a = [], None
            for c0 in range(0, D, 3):
                col = colors[:, c0:c0 + 3]
                if col.shape[1] == 2:  # (the three-channel path has no two-channel kernel: pad the last call)
                    col = torch.cat([col, col[:, :1]], dim=1)
                r, a, _ = render(col)
                parts.append(r[..., :min(3, D - c0)])
            loss = (torch.cat(parts, dim=-1) * wr).sum() + a.sum()
            loss.backward()

        events = []
        one = _window(one_call, args.steps, args.warmup)
        bwd = sum(e0.elapsed_time(e1) for e0, e1 in events[-args.steps:]) / args.steps
        events = []
        old = _window(three_at_a_time, args.steps, args.warmup)
        line = {"D": D, "gaussians": N, "size": args.size, "channel_chunk": CHUNK,
                "launches_per_direction": math.ceil(D / CHUNK), "one_call_ms": round(one, 4),
                "bwd_ms": round(bwd, 4), "three_channel_calls": math.ceil(D / 3), "three_channel_calls_ms": round(old, 4),
                "speedup": round(old / one, 3), "steps": args.steps, "warmup": args.warmup}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
