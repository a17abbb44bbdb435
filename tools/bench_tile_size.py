"""Stage times of rasterization(tile_size=8 | 16 | 32) ("Tile sizes 8 and 32"): binning, compositing forward
and compositing backward, on 30 000 Gaussians at 512 x 512, three random colour channels, one camera, packed=False.

    python tools/bench_tile_size.py [--gaussians N] [--size S] [--calls K] [--warmup W] [--packed]

Every native call of a whole rasterization + backward is bracketed by two torch.cuda.Events on the current stream and
its time is added to its stage; the figure of a stage is the median over the timed calls.  The 16 row is the existing
path (tile counting fused into the projection, compositing by eg_composite_fwd_cams / eg_composite_bwd_colors).
--packed: the same call with packed=True (binning by eg_packed_bin at 16, compositing by the modes kernels)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = {
    "binning": ("eg_tile_count_ts", "eg_tile_offsets_cams", "eg_tile_emit_sort_ts", "eg_tile_emit_sort_cams", "eg_packed_bin"),
    "composite_fwd": ("eg_composite_fwd_ts_cams", "eg_composite_fwd_cams", "eg_composite_fwd_modes_cams",
                      "eg_composite_fwd_wide_cams"),
    "composite_bwd": ("eg_composite_bwd_ts_cams", "eg_composite_bwd_colors", "eg_composite_bwd_modes_cams",
                      "eg_composite_bwd_wide_cams"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=30000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--packed", action="store_true")
    a = ap.parse_args()
    from edgegaussians_amd import rasterization, synth
    from edgegaussians_amd import rasterizer as R
    sc = synth.make_scene(a.gaussians, 1, a.size, a.size, seed=0, spread_opacity=True)
    N = sc.means.shape[0]
    colors = (0.2 + 0.8 * torch.rand(N, 3, generator=torch.Generator().manual_seed(11))).cuda()
    p = [t.cuda().requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    vm, Ks = sc.viewmats[:1].cuda(), sc.Ks[:1].cuda()
    spans = []
    real_call = R.call

    def timed_call(name, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real_call(name, *args)
        e1.record()
        spans.append((name, e0, e1))

    R.call = timed_call
    try:
        for ts in (8, 16, 32):
            per_call = {k: [] for k in STAGES}
            M = 0
            for it in range(a.warmup + a.calls):
                spans.clear()
                for t in p:
                    t.grad = None
                render, alpha, info = rasterization(p[0], p[1], torch.exp(p[2]), torch.sigmoid(p[3]).squeeze(-1), colors, vm, Ks,
                                                    a.size, a.size, packed=a.packed, tile_size=ts)
                (render.sum() + alpha.sum()).backward()
                torch.cuda.synchronize()
                M = int(info["flatten_ids"].shape[0])
                if it >= a.warmup:
                    for stage, names in STAGES.items():
                        per_call[stage].append(sum(e0.elapsed_time(e1) for n, e0, e1 in spans if n in names))
            row = {"tile_size": ts, "packed": a.packed, "gaussians": N, "size": a.size, "intersections": M,
                   "tiles": info["tile_width"] * info["tile_height"],
                   **{f"{k}_us": round(1e3 * statistics.median(v), 1) for k, v in per_call.items()}}
            print(json.dumps(row), flush=True)
    finally:
        R.call = real_call


if __name__ == "__main__":
    main()
