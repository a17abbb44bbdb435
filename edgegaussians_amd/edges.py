"""Parametric edges (line end points and cubic-Bezier control points) to points, and their score, on the device.

The reference's headline evaluation (`eval.py --use_parametric_edges`) first turns `parametric_edges.json` into points
at a 0.005 spacing with `eval_utils.get_pred_points_and_directions[_from_dict]` (`eval_utils.py:120-398`), in
interpreted Python; `fit_edges.py --save_sampled_points` does the same.  Here that is two native calls
(`eg_edge_sample_count`, `eg_edge_sample_emit`: csrc/edges.hip) in float64, with the reference's rules restated:

    pts, n_curve = edges.sample(json.load(open("parametric_edges.json")))      # float32 [S,3] on the device
    m = edges.evaluate_edges(json.load(open("parametric_edges.json")), gt)      # metrics.evaluate + "n_pred"

Out of scope: clustering and fitting (what writes the json), `get_gt_points` and `downsample_point_cloud_average`.
"""
from __future__ import annotations

import ctypes
import json
from typing import Dict, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import metrics
from ._lib import call, load, ptr, stream

TANGENTS = {"reference": 0, "exact": 1}  # EG_EDGE_TANGENT_*
ERR_CAPACITY = -4  # EG_ERR_CAPACITY


def _as_f64(a, tail: Tuple[int, int], name: str) -> np.ndarray:
    """The reference's reshape (`eval_utils.py:290-292`) of a list, array or tensor, checked."""
    if isinstance(a, Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a, dtype=np.float64)
    per = tail[0] * tail[1]
    if a.size % per != 0 or (a.ndim >= 2 and a.shape[-1] not in (3, per)):
        raise ValueError(f"{name} must have shape (n, {tail[0]}, 3), or rows of 3 or {per} that flatten to it, got {a.shape}")
    a = np.ascontiguousarray(a.reshape(-1, *tail))
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds non-finite control points")
    return a


def _split(edges) -> Tuple[np.ndarray, np.ndarray]:
    if isinstance(edges, dict):
        curves, lines = edges["curves_ctl_pts"], edges["lines_end_pts"]
    else:
        curves, lines = edges
    return _as_f64(curves, (4, 3), "curves_ctl_pts"), _as_f64(lines, (2, 3), "lines_end_pts")


def _check_args(sample_resolution: float, tangent: str, device) -> torch.device:
    if not (isinstance(sample_resolution, (int, float)) and 0 < sample_resolution < float("inf")):
        raise ValueError(f"sample_resolution must be a positive number, got {sample_resolution!r}")
    if tangent not in TANGENTS:
        raise ValueError(f"tangent must be 'reference' or 'exact', got {tangent!r}")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"device must be a GPU (got {dev}); edgegaussians_amd has no CPU path")
    return dev


def sample_tables(edges, sample_resolution: float = 0.005, tangent: str = "reference", return_directions: bool = False,
                  return_ids: bool = False, device="cuda", capacity: int = None) -> Dict[str, Tensor]:
    """`sample` with everything the kernels leave: "points" [S,3] float32, "n_curve_points", "lengths" float64 [P],
    "counts" int32 [P], "offsets" int32 [P + 1] (P primitives: all curves, then all lines), and "directions" [S,3]
    float32 / "prim_ids" [S] int32 when asked for."""
    dev = _check_args(sample_resolution, tangent, device)
    curves, lines = _split(edges)
    Nc, Nl = len(curves), len(lines)
    P = Nc + Nl
    if capacity is not None and capacity < 0:
        raise ValueError(f"capacity must be >= 0, got {capacity}")
    with torch.cuda.device(dev):
        dc, dl = torch.from_numpy(curves).to(dev), torch.from_numpy(lines).to(dev)
        lengths = torch.empty(P, dtype=torch.float64, device=dev)
        counts = torch.empty(P, dtype=torch.int32, device=dev)
        offsets = torch.empty(P + 1, dtype=torch.int32, device=dev)
        total = torch.empty(2, dtype=torch.int32, device=dev)
        pc, pl = (ptr(dc) if Nc else None), (ptr(dl) if Nl else None)
        plen, pcnt = (ptr(lengths) if P else None), (ptr(counts) if P else None)
        mode = TANGENTS[tangent]

        def outputs(rows):
            return (torch.empty(rows, 3, device=dev), torch.empty(rows, 3, device=dev) if return_directions else None,
                    torch.empty(rows, dtype=torch.int32, device=dev) if return_ids else None)

        if capacity is None:
            call("eg_edge_sample_count", pc, Nc, pl, Nl, float(sample_resolution), -1, plen, pcnt, ptr(offsets),
                 ptr(total), stream())
            # the one read-back: the total sizes the output (with it, where the lines' samples start)
            S, overflow, n_curve = torch.cat([total, offsets[Nc:Nc + 1]]).tolist()
            if overflow:
                raise RuntimeError(f"the edges give more than 2^31 - 1 samples at resolution {sample_resolution}")
            points, directions, ids = outputs(S)
            if S:
                call("eg_edge_sample_emit", pc, Nc, pl, Nl, pcnt, ptr(offsets), ptr(total), S, mode, ptr(points),
                     ptr(directions), ptr(ids), stream())
        else:
            points, directions, ids = outputs(capacity)
            host = (ctypes.c_int32 * 2)()
            lib = load()
            rc = lib.eg_edge_sample(pc, Nc, pl, Nl, float(sample_resolution), capacity, mode, plen, pcnt, ptr(offsets),
                                    ptr(total), ptr(points) if capacity else None, ptr(directions), ptr(ids), host,
                                    stream())
            if rc != 0:
                raise RuntimeError(f"eg_edge_sample failed (code {rc}): {lib.eg_last_error_string().decode()}")
            S = host[0]
            points = points[:S]
            directions = directions[:S] if return_directions else None
            ids = ids[:S] if return_ids else None
            n_curve = int(offsets[Nc])
    out = {"points": points, "n_curve_points": n_curve, "lengths": lengths, "counts": counts, "offsets": offsets}
    if return_directions:
        out["directions"] = directions
    if return_ids:
        out["prim_ids"] = ids
    return out


def sample(edges, sample_resolution: float = 0.005, tangent: str = "reference", return_directions: bool = False,
           return_ids: bool = False, device="cuda", capacity: int = None):
    """Points on parametric edges at `sample_resolution`, as `get_pred_points_and_directions_from_dict` lays them out.

    edges: the reference's dict {"curves_ctl_pts": [...], "lines_end_pts": [...]} (reshaped as it does, to (-1, 4, 3)
    and (-1, 2, 3)), or a pair (curves, lines) of arrays / tensors.  Returns (points, n_curve_points[, directions]
    [, prim_ids]): points float32 [S,3] on `device`, the samples of all curves first (points[:n_curve_points]), then
    those of all lines (`eval.py:116`); directions float32 [S,3]; prim_ids int32 [S] (curve i -> i, line j -> Nc + j).

    A primitive of length L gives int(L // sample_resolution) samples at np.linspace(0, 1, n) (none when it is shorter
    than the resolution, one at t = 0 below twice the resolution), L being the reference's composite Simpson sum for a
    curve.  Everything is evaluated in float64 and rounded once to float32.

    tangent: the direction of curve samples.  "reference" reproduces the reference's formula exactly as written
    (`eval_utils.py:322-368`): A (3 t^2) + B (2 t) + C, normalised, where A t^2 + B t + C is the derivative -- the
    t^2 and t coefficients carry an extra factor 3 and 2, so it is NOT the true tangent except at t = 0.  "exact" is the
    normalised true derivative.  Line directions are (p1 - p0) / (|p1 - p0| + 1e-6) (`:389-391`) in both modes.  A zero
    direction gives nan, as dividing by its norm does in the reference.

    One host read-back, of the total, sizes the output.  With `capacity` the call is one native entry
    (`eg_edge_sample`) into buffers of that many rows and raises when the samples do not fit.  Empty input gives a
    [0,3] tensor."""
    t = sample_tables(edges, sample_resolution, tangent, return_directions, return_ids, device, capacity)
    out = [t["points"], t["n_curve_points"]]
    if return_directions:
        out.append(t["directions"])
    if return_ids:
        out.append(t["prim_ids"])
    return tuple(out)


def get_pred_points_and_directions_from_dict(json_data, sample_resolution: float = 0.005):
    """The reference's function of this name (`eval_utils.py:285-398`) with its return shapes: (curve_points [Sc,3]
    ndarray, line_points [Sl,3] ndarray, curve_directions list of [3] arrays, line_directions list of [3] arrays) --
    float64 arrays holding the float32 samples.  For `fit_edges.py:130` to call instead."""
    pts, n_curve, dirs = sample(json_data, sample_resolution, "reference", return_directions=True)
    pts, dirs = pts.cpu().numpy().astype(np.float64), dirs.cpu().numpy().astype(np.float64)
    return pts[:n_curve], pts[n_curve:], list(dirs[:n_curve]), list(dirs[n_curve:])


def get_pred_points_and_directions(json_path, sample_resolution: float = 0.005):
    """`eval_utils.py:168-283`: the same from a `parametric_edges.json` path.  For `eval.py:114` to call instead."""
    with open(json_path, "r") as f:
        return get_pred_points_and_directions_from_dict(json.load(f), sample_resolution)


def evaluate_edges(edges, gt: Tensor, thresholds: Sequence[float] = (0.005, 0.01, 0.02),
                   sample_resolution: float = 0.005, scale_points: float = 1.0) -> Dict[str, float]:
    """`eval.py:114-137` for one scan with parametric edges: sample, scale (`:120`; applied to the float32 samples),
    `metrics.evaluate` against gt (float32 [M,3] on the device), plus "n_pred", the number of samples.  Raises the
    reference's "No points found" (`:118`) as a ValueError."""
    metrics._check_points(gt, "gt")
    pts, _ = sample(edges, sample_resolution, device=gt.device)
    if pts.shape[0] == 0:
        raise ValueError("No points found")
    if scale_points != 1.0:
        pts = pts * scale_points
    out = metrics.evaluate(pts, gt, thresholds)
    out["n_pred"] = int(pts.shape[0])
    return out
