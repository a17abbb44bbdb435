"""python -m edgegaussians_amd.eval -- the one-scan core of the reference's `eval.py`, on the device.

    python -m edgegaussians_amd.eval --pred parametric_edges.json --gt 00004926_0.005.ply [--json]
    python -m edgegaussians_amd.eval --pred gaussians_filtered.ply --gt 00004926_0.005.ply

--pred is a `.json` of parametric edges (sampled at --sample_resolution, `eval.py:114-120`) or a `.ply` of points;
--gt is a `.ply` of ground-truth points.  Prints accuracy, completeness, chamfer and precision / recall / F-score / IoU
per threshold (`eval.py:130-137`), plus n_pred.

Out of scope: the reference's directory conventions (scan lists, output folders, `--use_parametric_edges` switches),
its metrics pickles, `get_gt_points` (the yml feature parser behind the ground-truth files) and visualisation.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np
import torch

from . import edges, io, metrics


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(prog="python -m edgegaussians_amd.eval", description=__doc__.split("\n\n")[0])
    ap.add_argument("--pred", required=True, help="parametric edges (.json) or points (.ply)")
    ap.add_argument("--gt", required=True, help="ground-truth points (.ply)")
    ap.add_argument("--sample_resolution", type=float, default=0.005, help="spacing of the samples on parametric edges")
    ap.add_argument("--scale_points", type=float, default=1.0, help="scale applied to the predicted points")
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.005, 0.01, 0.02])
    ap.add_argument("--save_sampled_points", metavar="OUT.ply", help="write the (unscaled) predicted points")
    ap.add_argument("--json", action="store_true", help="print the metrics as one JSON line")
    args = ap.parse_args(argv)

    gt = torch.from_numpy(io.read_points_ply(args.gt).astype(np.float32)).cuda()
    thresholds = tuple(args.thresholds)
    if args.pred.lower().endswith(".json"):
        with open(args.pred, "r") as f:
            data = json.load(f)
        if args.save_sampled_points:
            io.write_points_ply(edges.sample(data, args.sample_resolution)[0], args.save_sampled_points)
        out = edges.evaluate_edges(data, gt, thresholds, args.sample_resolution, args.scale_points)
    else:
        pts = torch.from_numpy(io.read_points_ply(args.pred).astype(np.float32)).cuda()
        if pts.shape[0] == 0:
            raise ValueError("No points found")
        if args.save_sampled_points:
            io.write_points_ply(pts, args.save_sampled_points)
        if args.scale_points != 1.0:
            pts = pts * args.scale_points
        out = metrics.evaluate(pts, gt, thresholds)
        out["n_pred"] = int(pts.shape[0])
    if args.json:
        print(json.dumps(out))
    else:
        for k, v in out.items():
            print(f"{k}: {v}")
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
