"""Scalar image losses on the device: weighted / masked L1 and L2 (csrc/losses.hip: eg_loss_fwd / eg_loss_bwd) and the
3DGS loss ``(1 - lambda) L1 + lambda (1 - SSIM)`` (csrc/ssim.hip: eg_photometric_fwd / eg_photometric_bwd).  Two
launches forward (partial sums, finalize), one backward, no atomics: the same bits on every run.  No CPU path, no torch
fall-back.

Semantics (tests/losses_util.py states exactly this in float64):

* Pointwise family.  ``input``, ``target``, ``weights``: fp32 device tensors of 1 to 4 dimensions, left-padded to
  ``[B, C, H, W]``; ``target`` and ``weights`` broadcast to ``input``; only ``input`` receives a gradient.  The term of
  element p is ``t_p = w_p |c(x_p) - y_p|^q``: q = 1 (``kind="l1"``) or 2 (``"l2"``), ``c = clamp(., 0, 1)`` with
  ``clamp=True``, ``w_p`` = 1, an fp32 weight, or a ``torch.bool`` mask (read as bytes).  The value is ``sum_p t_p / D``:
  ``reduction="sum"``: D = 1; ``"mean"``: D = numel -- or, with a mask, the number of selected elements (counted as an
  integer on the device), which is ``F.l1_loss(input[mask], target[mask])``: nan with a zero gradient when nothing is
  selected.
* Backward, for a cotangent v: ``g_p = (v / D) w_p q |c(x_p) - y_p|^(q - 1) sign(c(x_p) - y_p)``, times the clamp's
  gate ``0 <= x_p <= 1`` (closed, as ``torch.clamp``), ``sign(0) = 0``, and exactly 0.0 where the mask is false or the
  weight is 0.  v and D stay on the device.
* ``photometric_loss``: shapes, layouts and checks of ``ssim.fused_ssim``; the value is
  ``(1 - lambda) mean|img1 - img2| + lambda (1 - mean(ssim_map(img1, img2, padding)))``.  No SSIM map and no cotangent
  map is written; the three derivative maps only when a gradient is needed.

Layouts: every operand is read through its own element strides.  Work is assigned by the logical index, so the value's
bits do not depend on the strides.  ``input`` is read in place -- and its gradient, ``empty_like(input)``, written
through strides -- when it is dense (``ssim._dense``) or dense up to one skipped stride, which is what selecting a
channel of ``rasterization``'s ``[1, H, W, 3]`` render leaves: ``render[0, ..., 0]``.  Broadcast dimensions of ``target``
and ``weights`` have stride 0 (an ``expand``, no memory).  Any other stride pattern takes one ``.contiguous()``.

Checks, before any launch, structure first so that every one of them can be met without a device: unknown
``reduction`` / ``kind`` / ``padding``, more than 4 dimensions, not broadcastable, an empty ``input`` (ValueError); a
wrong dtype -- fp32 everywhere, weights fp32, a mask ``torch.bool`` -- (TypeError); ``target`` or ``weights`` requiring
grad (ValueError); a CPU tensor (ValueError, "no CPU path").

When ``input`` needs no gradient, or under ``no_grad``, nothing is saved, no derivative map is allocated, and the value
is bit-equal to the training-mode value."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import ssim as _ssim
from ._lib import call, stream
from .ssim import TILE_H, TILE_W, _dense

WG_ELEMS = 1024   # logical indices per workgroup of the pointwise kernels (csrc/losses.hip: kPerWG = kThreads * kQuad)
FIN_LANES = 64    # lanes of the finalize kernels (csrc/losses.hip, csrc/ssim.hip: kFinLanes)
MAX_NUMEL = 2 ** 31 - 1

_KINDS = {"l1": 1, "l2": 2}
_W_NONE, _W_FLOAT, _W_MASK = 0, 1, 2
_SUM, _MEAN, _MASK_MEAN = 0, 1, 2


def _dense_but_one_stride(t: Tensor) -> bool:
    """dense and non-overlapping once ONE stride is divided out: a dense tensor of which an index was selected"""
    expect, skipped = 1, False
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            if skipped or stride < expect or stride % expect:
                return False
            skipped = True
        expect = stride * size
    return True


def _in_place(t: Tensor, broadcast: bool = False) -> Tensor:
    """t itself when the kernels may read it through its strides, else its contiguous copy; `broadcast`: dimensions
    of stride 0 (an expand) are left out of the question"""
    if t.is_contiguous():  # (the common case, decided without a look at the strides)
        return t
    core = t[tuple(0 if st == 0 and s > 1 else slice(None) for s, st in zip(t.shape, t.stride()))] if broadcast else t
    return t if _dense(core) or _dense_but_one_stride(core) else t.contiguous()


def _operand(t: Tensor, shape4, broadcast: bool = False) -> Tensor:
    """t as the 4-D problem sees it: left-padded and, for target and weights, expanded (stride 0, no memory)"""
    if t.dim() < 4:
        t = t.reshape((1,) * (4 - t.dim()) + tuple(t.shape))
    t = _in_place(t, broadcast)
    return t if t.shape == shape4 else t.expand(shape4)


def _strides(t: Tensor):
    return (C.c_int64 * 4)(*t.stride())


class _PointwiseLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, w, q, clamp, reduction, train):
        B, Cn, H, W = x.shape
        w_kind = _W_NONE if w is None else _W_MASK if w.dtype == torch.bool else _W_FLOAT
        G = -(-x.numel() // WG_ELEMS)
        words = 2 * G if w_kind == _W_MASK else G
        slab = torch.empty(words, dtype=torch.float32, device=x.device)
        out = torch.empty(3, dtype=torch.float32, device=x.device)
        head = (x.data_ptr(), y.data_ptr(), w.data_ptr() if w is not None else None, w_kind, B, Cn, H, W, _strides(x),
                _strides(y), _strides(w) if w is not None else None, q, int(clamp))
        call("eg_loss_fwd", *head, reduction, slab.data_ptr(), words, out.data_ptr(), stream())
        if train:
            ctx.head = head
            ctx.save_for_backward(x, y, w, out)
        return out[0]

    @staticmethod
    def backward(ctx, v):
        x, y, w, out = ctx.saved_tensors
        v = v.contiguous()
        g = torch.empty_like(x)  # (dense x: its strides; x with a skipped stride: the same order, packed)
        call("eg_loss_bwd", *ctx.head, v.data_ptr(), out.data_ptr(), g.data_ptr(), _strides(g), stream())
        return g, None, None, None, None, None, None


def _check_pointwise(input: Tensor, target: Tensor, weights: Optional[Tensor], kind: str, reduction: str,
                     weights_dtype=None) -> None:
    if reduction not in ("mean", "sum"):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    if kind not in _KINDS:
        raise ValueError(f"kind must be 'l1' or 'l2', got {kind!r}")
    named = [(input, "input"), (target, "target")] + ([(weights, "weights")] if weights is not None else [])
    for t, name in named:
        if not 1 <= t.dim() <= 4:
            raise ValueError(f"{name} must have 1 to 4 dimensions, got {tuple(t.shape)}")
    for t, name in named[1:]:
        if t.shape != input.shape and not (t.dim() <= input.dim() and all(
                a == b or a == 1 for a, b in zip(reversed(t.shape), reversed(input.shape)))):
            raise ValueError(f"{name} {tuple(t.shape)} is not broadcastable to input {tuple(input.shape)}")
    if input.numel() == 0:
        raise ValueError(f"input must not be empty, got {tuple(input.shape)}")
    if input.numel() > MAX_NUMEL:
        raise ValueError(f"input must have fewer than 2^31 elements, got {input.numel()}")
    for t, name in named[:2]:
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if weights is not None:
        allowed = (torch.float32, torch.bool) if weights_dtype is None else (weights_dtype,)
        if weights.dtype not in allowed:
            raise TypeError(f"weights must be {' or '.join(str(d) for d in allowed)}, got {weights.dtype}")
    for t, name in named[1:]:
        if t.requires_grad:
            raise ValueError(f"{name} must not require grad: only input receives a gradient")
    for t, name in named:
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (got {t.device}); edgegaussians_amd has no CPU path")


def _pointwise(input, target, weights, kind, clamp, reduction, weights_dtype=None) -> Tensor:
    _check_pointwise(input, target, weights, kind, reduction, weights_dtype)
    shape4 = (1,) * (4 - input.dim()) + tuple(input.shape)
    x = _operand(input, shape4)
    y = _operand(target, shape4, True)
    w = _operand(weights, shape4, True) if weights is not None else None
    masked = w is not None and w.dtype == torch.bool
    red = _SUM if reduction == "sum" else _MASK_MEAN if masked else _MEAN
    if torch.is_grad_enabled() and input.requires_grad:
        return _PointwiseLoss.apply(x, y, w, _KINDS[kind], clamp, red, True)
    with torch.no_grad():
        return _PointwiseLoss.apply(x, y, w, _KINDS[kind], clamp, red, False)


def image_loss(input: Tensor, target: Tensor, weights: Optional[Tensor] = None, *, kind: str = "l1",
               clamp: bool = False, reduction: str = "mean") -> Tensor:
    """The general form (module docstring): ``sum_p w_p |c(input_p) - target_p|^q / D`` as a 0-dim tensor,
    differentiable in ``input``.  ``weights``: None, fp32 weights, or a ``torch.bool`` mask -- with a mask
    ``reduction="mean"`` divides by the number of selected elements."""
    return _pointwise(input, target, weights, kind, clamp, reduction)


def l1_loss(input: Tensor, target: Tensor) -> Tensor:
    """``F.l1_loss(input, target)``: the reference's "whole" strategy."""
    return _pointwise(input, target, None, "l1", False, "mean")


def mse_loss(input: Tensor, target: Tensor) -> Tensor:
    """``F.mse_loss(input, target)``: the "whole" strategy with ``loss_type="l2"``."""
    return _pointwise(input, target, None, "l2", False, "mean")


def weighted_l1_loss(input: Tensor, target: Tensor, weights: Tensor) -> Tensor:
    """The reference's ``WeightedL1Loss``: ``mean(weights * |input - target|)``, fp32 weights."""
    return _pointwise(input, target, weights, "l1", False, "mean", torch.float32)


def masked_l1_loss(input: Tensor, target: Tensor, mask: Tensor) -> Tensor:
    """The reference's ``MaskedL1Loss``: ``F.l1_loss(input[mask], target[mask])`` = ``sum mask |.| / sum mask`` with a
    ``torch.bool`` mask; nan with a zero gradient when the mask is all false."""
    return _pointwise(input, target, mask, "l1", False, "mean", torch.bool)


def projection_loss(render: Tensor, gt: Tensor, weight_map: Tensor, clamp: bool = True) -> Tensor:
    """The trainer's projection loss ``sum_p w_p |clamp(render_p, 0, 1) - gt_p|`` for the weight maps of
    ``synth.weight_map`` (every strategy of the reference's ``compute_projection_loss``).  ``render[0, ..., 0]`` of
    ``rasterization``'s ``[1, H, W, 3]`` output is read in place."""
    return _pointwise(render, gt, weight_map, "l1", clamp, "sum", torch.float32)


class _Photometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2, lam, valid, train):
        a, b = _ssim._strided(img1), _ssim._strided(img2)
        B, Cn, H, W = a.shape
        G = -(-W // TILE_W) * -(-H // TILE_H) * B * Cn
        slab = torch.empty(2 * G, dtype=torch.float32, device=a.device)
        out = torch.empty(3, dtype=torch.float32, device=a.device)
        maps = [torch.empty(B, Cn, H, W, device=a.device) for _ in range(3)] if train else [None] * 3
        head = (a.data_ptr(), b.data_ptr(), B, Cn, H, W, _ssim._strides(a), _ssim._strides(b), int(valid), lam)
        call("eg_photometric_fwd", *head, *[m.data_ptr() if m is not None else None for m in maps], slab.data_ptr(),
             2 * G, out.data_ptr(), stream())
        if train:
            ctx.head = head
            ctx.save_for_backward(a, b, *maps)
        terms = out[1:]
        ctx.mark_non_differentiable(terms)
        return out[0], terms

    @staticmethod
    def backward(ctx, v, _):
        a, b, d_m1, d_s1, d_s12 = ctx.saved_tensors
        v = v.contiguous()
        v_img1 = torch.empty_like(a)  # (a is dense: its strides are kept)
        call("eg_photometric_bwd", *ctx.head, v.data_ptr(), d_m1.data_ptr(), d_s1.data_ptr(), d_s12.data_ptr(),
             v_img1.data_ptr(), stream())
        return v_img1, None, None, None, None


def photometric_loss(img1: Tensor, img2: Tensor, lambda_dssim: float = 0.2, padding: str = "same",
                     return_terms: bool = False):
    """``(1 - lambda_dssim) * mean|img1 - img2| + lambda_dssim * (1 - mean(ssim_map(img1, img2, padding)))`` as a 0-dim
    tensor, differentiable in ``img1``; shapes, layouts and checks of ``ssim.fused_ssim``.  With ``return_terms`` also
    the detached L1 mean and SSIM mean: ``(loss, l1, ssim)``."""
    _ssim._check(img1, img2, padding)
    lam = float(lambda_dssim)
    if torch.is_grad_enabled() and img1.requires_grad:
        loss, terms = _Photometric.apply(img1, img2, lam, padding == "valid", True)
    else:
        with torch.no_grad():
            loss, terms = _Photometric.apply(img1, img2, lam, padding == "valid", False)
    return (loss, terms[0], terms[1]) if return_terms else loss
