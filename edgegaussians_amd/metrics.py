"""Edge-point metrics on device: how far a set of predicted points is from the ground truth, both ways.

Host-side mirror of the reference's evaluation (`eval.py:130-137`, `eval_utils.py:400-509`): accuracy, completeness
and chamfer distance, and precision / recall / F-score / IoU at a list of thresholds.  The reference builds two CPU
KD-trees per threshold (point_cloud_utils); here both nearest-neighbour searches are ONE exact search each on the
GPU (`eg_nn_query_small` / `eg_nn_query_auto`: the queries are a different point set from the targets, which the
self-search of `regularizers.knn` cannot answer), the distances stay on the device and the scalars are read back once.

    m = metrics.evaluate(pred, gt)          # {"acc", "comp", "chamfer", "precision_0.02", "recall_0.02", ...}
"""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import torch
from torch import Tensor

from ._lib import call, load, ptr, stream

# up to this many (query, target) pairs the exhaustive search (eg_nn_query_small: one launch, every pair) beats the grid
# search (bounding box + two counting sorts + the walk: nine small launches).  Read off profiles/nn_query_timing.txt:
# the exhaustive search costs ~0.02 ms + 0.4 ms per 10^9 pairs (0.045 ms at 8 k x 8 k, 0.07 at 12 k x 12 k, 0.31 at
# 10 k x 70 k), the grid search 0.05 ms on small uniform clouds and 0.08-0.16 on clustered ones: they cross at
# 0.8 * 10^8 pairs (uniform) and 3 * 10^8 (clustered)
NN_EXHAUSTIVE_MAX_PAIRS = 100_000_000
_scratch: Dict = {}


def _check_points(t: Tensor, name: str) -> None:
    if not isinstance(t, Tensor) or not t.is_cuda:
        dev = t.device if isinstance(t, Tensor) else type(t).__name__
        raise ValueError(f"{name} must be a device tensor (got {dev}); edgegaussians_amd has no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be {torch.float32}, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must have shape (n, 3), got {tuple(t.shape)}")


def _query_buffers(Q: int, M: int, ncell: int, dev):
    """cell_of [max(Q, M)], counts [ncell] (zero between calls), start [ncell + 1], targets and queries in cell order
    [M,4] / [Q,4], 64 bytes of grid scratch -- cached per (Q, M, device)."""
    key = (Q, M, str(dev))
    b = _scratch.get(key)
    if b is None:
        if len(_scratch) > 8:
            _scratch.clear()
        b = (torch.empty(max(Q, M), dtype=torch.int32, device=dev), torch.zeros(ncell, dtype=torch.int32, device=dev),
             torch.empty(ncell + 1, dtype=torch.int32, device=dev), torch.empty(M, 4, device=dev),
             torch.empty(Q, 4, device=dev), torch.zeros(16, dtype=torch.int32, device=dev))
        _scratch[key] = b
    return b


def nearest(queries: Tensor, targets: Tensor, method: str = "auto", squared: bool = False) -> Tuple[Tensor, Tensor]:
    """For each query [Q,3] the nearest target [M,3]: (distance [Q] float32, index [Q] int32) -- exact, on the device
    and without a host sync.  Self is not excluded; among targets at the same fp32 squared distance the lowest index
    wins.  method "auto" = exhaustive search up to NN_EXHAUSTIVE_MAX_PAIRS pairs, else the search on a uniform grid
    over the targets that the device chooses; "exhaustive" / "grid" force one (same bits either way).  `squared`: the
    squared distances the kernels order by, instead of their roots."""
    _check_points(queries, "queries")
    _check_points(targets, "targets")
    if method not in ("auto", "exhaustive", "grid"):
        raise ValueError(f"method must be 'auto', 'exhaustive' or 'grid', got {method!r}")
    if queries.device != targets.device:
        raise ValueError(f"queries and targets must be on one device, got {queries.device} and {targets.device}")
    Q, M = queries.shape[0], targets.shape[0]
    if M < 1:
        raise ValueError("targets must hold at least one point")
    dev = queries.device
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    d2 = torch.empty(Q, device=dev)
    if Q == 0:
        return d2, idx
    qs, ts = queries.detach().contiguous(), targets.detach().contiguous()
    with torch.cuda.device(dev):
        if method == "exhaustive" or (method == "auto" and Q * M <= NN_EXHAUSTIVE_MAX_PAIRS):
            call("eg_nn_query_small", ptr(qs), Q, ptr(ts), M, ptr(idx), ptr(d2), stream())
        else:
            D = int(load().eg_knn_auto_dims(M, 1))
            cell_of, counts, start, tsorted, qsorted, gs = _query_buffers(Q, M, D * D * D, dev)
            call("eg_nn_query_auto", ptr(qs), Q, ptr(ts), M, ptr(cell_of), ptr(counts), ptr(start), ptr(tsorted),
                 ptr(qsorted), ptr(gs), ptr(idx), ptr(d2), stream())
    return (d2 if squared else d2.sqrt()), idx


def _summary_tensor(d_pred_to_gt: Tensor, d_gt_to_pred: Tensor, thresholds: Sequence[float]) -> Tensor:
    """[2 + 2 T] float64 on the distances' device: the two means, then the two counts per threshold."""
    a, b = d_pred_to_gt.reshape(-1).double(), d_gt_to_pred.reshape(-1).double()
    rows = [a.mean(), b.mean()]
    for t in thresholds:
        rows += [(a < t).sum().double(), (b < t).sum().double()]
    return torch.stack(rows)


def summarize(d_pred_to_gt: Tensor, d_gt_to_pred: Tensor, thresholds: Sequence[float]) -> Dict[str, float]:
    """The reference's figures from the two nearest-neighbour distance vectors (pure arithmetic: CPU or device
    tensors), `eval_utils.py:400-438` and `:456-494` restated with their quirks:
        acc = mean(d_pred_to_gt), comp = mean(d_gt_to_pred), chamfer = acc + comp          (sums in float64)
        per threshold t, strict <:  precision_t = #(d_pred_to_gt < t) / Q,  recall_t = #(d_gt_to_pred < t) / M,
        fscore_t = 2 P R / (P + R)  (nan when P + R = 0, as numpy gives),
        IOU_t = min(cp, cg) / (Q + M - max(cp, cg)) with the two counts cp, cg -- the reference's definition, not a
        set IoU.
    One read-back of 2 + 2 T scalars when the distances are on the device."""
    Q, M = d_pred_to_gt.numel(), d_gt_to_pred.numel()
    vals = _summary_tensor(d_pred_to_gt, d_gt_to_pred, thresholds).tolist()
    out = {"acc": vals[0], "comp": vals[1], "chamfer": vals[0] + vals[1]}
    for k, t in enumerate(thresholds):
        cp, cg = int(vals[2 + 2 * k]), int(vals[3 + 2 * k])
        p = cp / Q if Q else float("nan")
        r = cg / M if M else float("nan")
        union = Q + M - max(cp, cg)
        out[f"precision_{t}"] = p
        out[f"recall_{t}"] = r
        out[f"fscore_{t}"] = 2 * p * r / (p + r) if p + r > 0 else float("nan")
        out[f"IOU_{t}"] = min(cp, cg) / union if union else float("nan")
    return out


def evaluate(pred: Tensor, gt: Tensor, thresholds: Sequence[float] = (0.005, 0.01, 0.02)) -> Dict[str, float]:
    """`eval.py:130-137` for one scan: two searches (pred -> gt, gt -> pred), `summarize`, one read-back.  (The
    reference repeats both searches per threshold.)  Default thresholds: eval.py:137."""
    d_pred_to_gt, _ = nearest(pred, gt)
    d_gt_to_pred, _ = nearest(gt, pred)
    return summarize(d_pred_to_gt, d_gt_to_pred, thresholds)
