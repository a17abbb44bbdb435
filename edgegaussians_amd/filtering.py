"""Post-hoc Gaussian filters of the edge-extraction stage, on device.

Host-side mirror of `/root/reference/edgegaussians/edge_extraction/filtering.py`:
    filter_by_projection   :80-123   -> eg_project_visibility (one N x V kernel instead of a V-iteration
                                        numpy loop with a Python list round trip per view)
    filter_by_opacity      :71-77    -> one comparison
    filter_stat_outliers   :59-69    -> the existing exact kNN (eg_knn_small / eg_knn_auto) + a few reductions;
                                        the reference calls Open3D's remove_statistical_outlier

Same argument meaning and return value as the reference: a boolean inlier mask of shape [N] from the first two, the
ascending int64 INDICES of the inliers from `filter_stat_outliers` (the reference applies it first, fit_edges.py:20-45).
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from ._lib import call, ptr, stream
from .regularizers import knn


def pack_cameras(cameras: Sequence[Dict], device) -> torch.Tensor:
    """[V,21] = K (9) | R (9) | t (3) from the reference's camera dicts (filtering.py:42-56)."""
    rows = [np.concatenate([np.asarray(c["K"], np.float32).reshape(9), np.asarray(c["R"], np.float32).reshape(9),
                            np.asarray(c["t"], np.float32).reshape(3)]) for c in cameras]
    return torch.from_numpy(np.stack(rows)).to(device).contiguous()


def filter_by_projection(gaussian_means, edge_images, cameras: Sequence[Dict], visib_thresh: float = 0.1,
                         device="cuda") -> np.ndarray:
    """filtering.py:80-123: keep Gaussians whose mean, projected into every view and rounded to a
    pixel, sees an average edge strength above `visib_thresh` (views it falls outside of count as 0)."""
    means = torch.as_tensor(np.asarray(gaussian_means, np.float32)).to(device).contiguous()
    V = len(edge_images)
    if V == 0 or means.shape[0] == 0:
        return np.zeros(means.shape[0], dtype=bool)
    h, w = int(cameras[0]["h"]), int(cameras[0]["w"])
    maps = torch.stack([torch.as_tensor(e).to(device=device, dtype=torch.float32) for e in edge_images]).contiguous()
    if tuple(maps.shape) != (V, h, w):
        raise ValueError(f"edge_images must be {V} maps of {h}x{w}, got {tuple(maps.shape)}")
    visib = torch.zeros(means.shape[0], dtype=torch.float64, device=device)  # numpy's accumulator type there
    call("eg_project_visibility", ptr(means), means.shape[0], ptr(pack_cameras(cameras, device)), V, ptr(maps), w, h,
         ptr(visib), stream())
    return (visib.cpu().numpy() / float(V) > visib_thresh).reshape(-1)


def filter_by_opacity(opacities, min_opacity: float) -> np.ndarray:
    """filtering.py:71-77."""
    return (np.asarray(opacities) > min_opacity).reshape(-1)


def filter_stat_outliers(means, num_nn: int = 10, std_multiplier: float = 3.0) -> np.ndarray:
    """filtering.py:59-69: statistical outlier removal, the ascending int64 indices of the inliers.

    `means`: float32 [N,3] DEVICE tensor (there is no CPU path).  The semantics are those of Open3D 0.18's
    `PointCloud::RemoveStatisticalOutliers`, RESTATED from knowledge of its public source: Open3D is not a dependency
    of this package and the restatement could not be pinned against it (tests compare with a float64 restatement of
    the same formulas):
        avg_i     = mean of the distances (not squared) from point i to its num_nn nearest points, i itself among them
                    at distance 0: the num_nn - 1 nearest others, summed and divided by num_nn (by the number that
                    exist when the cloud has fewer than num_nn points)
        mean, std = over all avg_i, std with the N - 1 divisor
        inlier    iff avg_i > 0 and avg_i < mean + std_multiplier * std
    The neighbours come from `regularizers.knn` (exact, num_nn - 1 <= 32); mean / std / threshold are float64."""
    if not isinstance(means, torch.Tensor) or not means.is_cuda:
        dev = means.device if isinstance(means, torch.Tensor) else type(means).__name__
        raise ValueError(f"means must be a device tensor (got {dev}); edgegaussians_amd has no CPU path")
    if means.dtype != torch.float32:
        raise TypeError(f"means must be {torch.float32}, got {means.dtype}")
    if means.dim() != 2 or means.shape[1] != 3:
        raise ValueError(f"means must have shape (n, 3), got {tuple(means.shape)}")
    if not 2 <= num_nn <= 33:
        raise ValueError(f"num_nn must be in [2, 33] (the kNN kernels list up to 32 other points), got {num_nn}")
    if std_multiplier <= 0:
        raise ValueError("std_multiplier must be positive")
    N = means.shape[0]
    if N == 0:
        return np.zeros(0, dtype=np.int64)
    idx, dist = knn(means, num_nn - 1, want_dist=True)
    found = idx >= 0  # (a cloud of fewer than num_nn points: the missing neighbours are listed as -1)
    total = torch.where(found, dist, torch.zeros_like(dist)).double().sum(dim=1)
    avg = total / (found.sum(dim=1) + 1).double()
    mean = avg.mean()
    std = ((avg - mean) ** 2).sum().div(max(N - 1, 1)).sqrt()
    keep = (avg > 0) & (avg < mean + std_multiplier * std)
    return torch.nonzero(keep).view(-1).cpu().numpy().astype(np.int64)
