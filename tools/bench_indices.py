"""Times the per-pixel intersection lists (functional.rasterize_to_indices_in_range + accumulate, csrc/indices.hip)
next to rasterize_to_pixels on the same inputs and writes profiles/indices_timing.txt.

    python tools/bench_indices.py [--out profiles/indices_timing.txt] [--runs 20] [--tile-size 16] [--pixels-only]

Two scenes through the public functions, projection and binning done once outside the timed region:
  tile scene   tests/tile_util.SCENE_ARGS (2500 Gaussians, 204 x 140), cameras 0 and 2
  config 1     a scene of the bench's config-1 size (30 000 Gaussians, 512 x 512, synthetic look-at pose), view 0
Per scene, D = 3 colours and random cotangents; every figure is the median of `--runs` runs, each between two device
events, after a warm-up:
  lists        one full-range rasterize_to_indices_in_range call (count, scan, ONE host read-back, write)
  accumulate   accumulate forward + backward on those lists (gathers, kernel pair, torch's scatter-adds)
  lists + acc  both, as a caller runs them
  pixels       rasterize_to_pixels forward + backward: the yardstick (it runs none of the new code)
--pixels-only times the yardstick alone (the form that also runs on a tree without the two functions)."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def measure(G, label, sc, cams, ts, runs, pixels_only=False):
    Wd, Hd = sc.width, sc.height
    Cn, N = len(cams), sc.means.shape[0]
    tw, th = math.ceil(Wd / ts), math.ceil(Hd / ts)
    with torch.no_grad():
        radii, m2d, depths, conics, _ = G.fully_fused_projection(
            sc.means.cuda(), None, sc.quats.cuda(), torch.exp(sc.log_scales).cuda(), sc.viewmats[cams].cuda(),
            sc.Ks[cams].cuda(), Wd, Hd)
        _tpg, isect_ids, flat = G.isect_tiles(m2d, radii, depths, ts, tw, th)
        offs = G.isect_offset_encode(isect_ids, Cn, tw, th)
    op = torch.sigmoid(sc.logit_opacities).reshape(1, N).expand(Cn, N).contiguous().cuda()
    gen = torch.Generator().manual_seed(1)
    col = (0.2 + 0.8 * torch.rand(Cn, N, 3, generator=gen)).cuda()
    wr, wa = torch.rand(Cn, Hd, Wd, 3, generator=gen).cuda(), torch.rand(Cn, Hd, Wd, 1, generator=gen).cuda()
    ones = torch.ones(Cn, Hd, Wd, device="cuda")
    p = [t.detach().clone().requires_grad_(True) for t in (m2d, conics, op, col)]
    state = {}

    def lists():
        state["ids"] = G.rasterize_to_indices_in_range(0, 10 ** 10, ones, p[0], p[1], p[2], Wd, Hd, ts, offs, flat)

    def backward(r, a):
        for t in p:
            t.grad = None
        ((r * wr).sum() + (a * wa).sum()).backward()

    def acc():
        backward(*G.accumulate(p[0], p[1], p[2], p[3], *state["ids"], Wd, Hd))

    def both():
        lists()
        acc()

    def pixels():
        backward(*G.rasterize_to_pixels(p[0], p[1], p[3], p[2], Wd, Hd, ts, offs, flat))

    fns = {"pixels": pixels} if pixels_only else {"lists": lists, "accumulate": acc, "lists + acc": both, "pixels": pixels}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(runs):  # (alternated run by run: a drift of the machine hits them alike)
        for k, fn in fns.items():
            t[k].append(timed(fn))
    lines = [f"{label}: N = {N}, C = {Cn}, {Wd} x {Hd}, tile_size {ts}, {int(flat.numel())} intersections"]
    if not pixels_only:
        rows = int(state["ids"][0].numel())
        lines[0] += f", {rows} (pixel, Gaussian) rows = {rows / (Cn * Wd * Hd):.1f} per pixel"
    for k in fns:
        xs = t[k]
        lines.append(f"  {k:12s} {statistics.median(xs):10.1f} us  ({min(xs):.1f} .. {max(xs):.1f})")
    if not pixels_only:
        lines.append(f"  (lists + acc) / pixels = {statistics.median(t['lists + acc']) / statistics.median(t['pixels']):.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indices_timing.txt"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--tile-size", type=int, default=16)
    ap.add_argument("--pixels-only", action="store_true")
    args = ap.parse_args()
    from edgegaussians_amd import _lib, synth
    _lib.load()  # raises without the library or the GPU: no fallback
    import gsplat as G
    from tests.tile_util import SCENE_ARGS as A
    lines = [f"per-pixel intersection lists against rasterize_to_pixels, D = 3, fwd + bwd, fp32, {torch.cuda.get_device_name(0)}; "
             f"microseconds per run, median of {args.runs} runs between device events (min .. max)"]
    sc = synth.make_scene(A["n_gauss"], A["n_views"], A["width"], A["height"], seed=A["seed"], spread_opacity=A["spread_opacity"],
                          scale=A["scale"], anisotropy=A["anisotropy"])
    lines += measure(G, "tile scene", sc, [0, 2], args.tile_size, args.runs, args.pixels_only)
    sc = synth.make_scene(30_000, 2, 512, 512, seed=0)
    lines += measure(G, "config-1 size", sc, [0], args.tile_size, args.runs, args.pixels_only)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
