"""Time of the three kernel-backed operations of edgegaussians_amd.strategy next to the same operations written as
eager torch expressions (gsplat's own formulation), in one process.  The feature has no predecessor to compare with.

    python tools/bench_strategy.py [--gaussians 100000 1000000] [--cameras 1 4] [--reps 50] [--warmup 10]

  stats_dense / stats_packed   DefaultStrategy's per-step running statistics (eg_strategy_update / _packed; the packed
                               time includes the torch.searchsorted that builds the camera segments) vs. scale, norm,
                               nonzero and index_add_
  inject_noise                 MCMCStrategy's per-step position noise WITHOUT the draw (both sides get the same z):
                               eg_inject_noise vs. quat -> covariance, sigmoid gate, einsum
  compute_relocation           eg_compute_relocation on N / 20 rows (what a refinement relocates or adds) with ratios
                               1..10 vs. the double sum as torch expressions over the same rows

Prints one JSON line per case: medians of `--reps` HIP-event timings in milliseconds after `--warmup` untimed calls.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    times.sort()
    return times[len(times) // 2]


def _covars(quats, scales):
    w, x, y, z = torch.unbind(F.normalize(quats, dim=-1), dim=-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    M = R * scales[:, None, :]
    return torch.bmm(M, M.transpose(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--cameras", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert args.reps >= 50 and args.warmup >= 10

    from edgegaussians_amd.relocation import compute_relocation
    from edgegaussians_amd.strategy import MCMCStrategy, ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    W, H = 800, 800
    binoms = MCMCStrategy().initialize_state()["binoms"].to(dev)
    print("# " + " ".join([os.path.basename(sys.argv[0])] + sys.argv[1:]), flush=True)

    def emit(case, N, C, kernel_ms, torch_ms, **kw):
        print(json.dumps({"case": case, "gaussians": N, "cameras": C, "kernel_ms": round(kernel_ms, 4),
                          "torch_ms": round(torch_ms, 4), "speedup": round(torch_ms / kernel_ms, 2), "reps": args.reps,
                          "warmup": args.warmup, **kw}), flush=True)

    for N in args.gaussians:
        for C in args.cameras:
            grads = torch.randn(C, N, 2, device=dev, generator=g) * 1e-4
            radii = torch.randint(0, 30, (C, N), device=dev, generator=g, dtype=torch.int32)
            radii[torch.rand(C, N, device=dev, generator=g) < 0.4] = 0
            grad2d, count, rstate = (torch.zeros(N, device=dev) for _ in range(3))
            cam, gid = torch.nonzero(radii > 0, as_tuple=True)
            pg, pr = grads[cam, gid].contiguous(), radii[cam, gid].contiguous()

            def k_dense():
                ops._update_grad_stats(grad2d, count, rstate, grads, radii, W, H, C)

            def t_dense():     # gsplat's DefaultStrategy._update_state, packed=False
                gg = grads.clone()
                gg[..., 0] *= W / 2.0 * C
                gg[..., 1] *= H / 2.0 * C
                sel = radii > 0
                ids = torch.where(sel)[1]
                grad2d.index_add_(0, ids, gg[sel].norm(dim=-1))
                count.index_add_(0, ids, torch.ones_like(ids, dtype=torch.float32))
                rstate[ids] = torch.maximum(rstate[ids], radii[sel] / float(max(W, H)))

            def k_packed():
                ops._update_grad_stats(grad2d, count, rstate, pg, pr, W, H, C, gaussian_ids=gid, camera_ids=cam)

            def t_packed():     # gsplat's DefaultStrategy._update_state, packed=True
                gg = pg.clone()
                gg[..., 0] *= W / 2.0 * C
                gg[..., 1] *= H / 2.0 * C
                grad2d.index_add_(0, gid, gg.norm(dim=-1))
                count.index_add_(0, gid, torch.ones_like(gid, dtype=torch.float32))
                rstate[gid] = torch.maximum(rstate[gid], pr / float(max(W, H)))

            emit("stats_dense", N, C, _median_ms(k_dense, args.reps, args.warmup), _median_ms(t_dense, args.reps, args.warmup))
            emit("stats_packed", N, C, _median_ms(k_packed, args.reps, args.warmup), _median_ms(t_packed, args.reps, args.warmup),
                 pairs=int(gid.numel()))

        params = {"means": torch.randn(N, 3, device=dev, generator=g),
                  "quats": torch.randn(N, 4, device=dev, generator=g),
                  "scales": torch.rand(N, 3, device=dev, generator=g) * 4 - 6,
                  "opacities": torch.randn(N, device=dev, generator=g) * 3 - 3}
        z = torch.randn(N, 3, device=dev, generator=g)
        real = torch.randn_like

        def k_noise():
            torch.randn_like = lambda t: z     # (the draw is outside both timings)
            try:
                ops.inject_noise_to_position(params, {}, {}, 1e-3)
            finally:
                torch.randn_like = real

        def t_noise():     # gsplat's inject_noise_to_position
            opac = torch.sigmoid(params["opacities"])
            cov = _covars(params["quats"], torch.exp(params["scales"]))
            gate = 1 / (1 + torch.exp(-100 * ((1 - opac) - 0.995)))
            noise = z * gate[:, None] * 1e-3
            params["means"].add_(torch.einsum("bij,bj->bi", cov, noise))

        emit("inject_noise", N, 0, _median_ms(k_noise, args.reps, args.warmup), _median_ms(t_noise, args.reps, args.warmup))

        n = max(1, N // 20)
        o = torch.rand(n, device=dev, generator=g) * 0.9 + 0.005
        s = torch.rand(n, 3, device=dev, generator=g) * 0.1
        r = torch.randint(1, 11, (n,), device=dev, generator=g)

        def k_reloc():
            compute_relocation(o, s, r, binoms)

        def t_reloc():     # the double sum up to the largest ratio present (10), masked per row
            x = 1 - torch.pow(1 - o, 1.0 / r)
            den = torch.zeros_like(o)
            for i in range(1, 11):
                act = r >= i
                xp = x.clone()
                for k in range(i):
                    den += torch.where(act, binoms[i - 1, k] * (-1) ** k * xp / (k + 1) ** 0.5, 0.0)
                    xp = xp * x
            return x, (o / den)[:, None] * s

        emit("compute_relocation", n, 0, _median_ms(k_reloc, args.reps, args.warmup), _median_ms(t_reloc, args.reps, args.warmup),
             max_ratio=10)


if __name__ == "__main__":
    main()
