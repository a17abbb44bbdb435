"""Fused SSIM: the ``fused_ssim`` operation of gsplat's and every 3DGS trainer's ``0.8 * L1 + 0.2 * (1 - SSIM)`` loss on
the two kernels of csrc/ssim.hip (eg_ssim_fwd / eg_ssim_bwd: one launch each, LDS tiles, no atomics).  No CPU path, no
torch fall-back.

Semantics (tests/ssim_util.py states exactly this in float64):

* ``img1``, ``img2``: ``[B, C, H, W]``, fp32, on the device.  ``img1`` is the prediction and receives the gradient;
  ``img2`` is a constant.
* The window is ``g[k] = exp(-(k - 5)^2 / (2 * 1.5^2))``, k = 0..10, normalised to sum 1 in float64, then rounded to fp32.
* The blur ``G*x`` is ``g`` along W, then ``g`` along H, with zero padding of 5 on every side, per ``(b, c)`` plane.
* ``C1 = 0.01^2``, ``C2 = 0.03^2``.
* Moments: ``m1 = G*img1``, ``m2 = G*img2``, ``e11 = G*img1^2``, ``e22 = G*img2^2``, ``e12 = G*(img1 img2)``;
  ``s1 = e11 - m1^2``, ``s2 = e22 - m2^2``, ``s12 = e12 - m1 m2``.
* ``A1 = 2 m1 m2 + C1``, ``A2 = 2 s12 + C2``, ``B1 = m1^2 + m2^2 + C1``, ``B2 = s1 + s2 + C2``; the map is
  ``S = A1 A2 / (B1 B2)``.
* Backward, for a cotangent ``v`` of ``S``: ``d_s1 = -A1 A2 / (B1 B2^2)``, ``d_s12 = 2 A1 / (B1 B2)``,
  ``d_m1 = 2 m2 A2 / (B1 B2) - 2 m1 A1 A2 / (B1^2 B2) - 2 m1 d_s1 - m2 d_s12``, and
  ``v_img1 = G*(v d_m1) + 2 img1 G*(v d_s1) + img2 G*(v d_s12)`` with the same zero-padded blur.
* ``padding="same"``: the map is ``[B, C, H, W]``.  ``padding="valid"``: the same map cropped by 5 on every side (a view;
  H, W >= 11).  Interior windows never see the padding, so this is the valid convolution; its backward is the same
  kernel on ``v`` zero-padded back.

Layouts: each input is read through its own element strides, without a copy, when it is dense and non-overlapping --
contiguous NCHW, and the ``permute(0, 3, 1, 2)`` view of a contiguous ``[B, H, W, C]`` that ``rasterization``'s render
gives, among others.  The gradient is ``empty_like(img1)`` written through the same strides.  Any other stride pattern
takes one ``.contiguous()``.  The map and the derivative maps are contiguous NCHW.

Checks, before any launch, structure first so that every one of them can be met without a device: unknown ``padding``,
not 4-D, shapes that differ, an empty tensor, ``valid`` below 11 (ValueError); a dtype other than fp32 (TypeError);
``img2.requires_grad`` (ValueError); a CPU tensor (ValueError, "no CPU path")."""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from ._lib import call, stream

TILE_H, TILE_W = 32, 32  # the output tile of a workgroup (csrc/ssim.hip: kTH, kTW)
RADIUS = 5               # the window is 2 * RADIUS + 1 taps


def _dense(t: Tensor) -> bool:
    """dense and non-overlapping: some permutation of the dimensions is contiguous"""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def _strided(t: Tensor) -> Tensor:
    return t if _dense(t) else t.contiguous()


def _strides(t: Tensor):
    return (C.c_int64 * 4)(*t.stride())


class _SSIMMap(torch.autograd.Function):
    """S [B, C, H, W] (padding "same") of img1 against img2; `train`: the three derivative maps are written and kept
    for the backward, otherwise they are neither allocated nor computed."""

    @staticmethod
    def forward(ctx, img1, img2, train):
        a, b = _strided(img1), _strided(img2)
        B, Cn, H, W = a.shape
        S = torch.empty(B, Cn, H, W, device=a.device)
        maps = [torch.empty_like(S) for _ in range(3)] if train else [None] * 3
        call("eg_ssim_fwd", a.data_ptr(), b.data_ptr(), B, Cn, H, W, _strides(a), _strides(b), S.data_ptr(),
             *[m.data_ptr() if m is not None else None for m in maps], stream())
        if train:
            ctx.save_for_backward(a, b, *maps)
        return S

    @staticmethod
    def backward(ctx, v):
        a, b, d_m1, d_s1, d_s12 = ctx.saved_tensors
        B, Cn, H, W = a.shape
        v = v.contiguous()
        v_img1 = torch.empty_like(a)  # (a is dense: its strides are kept)
        call("eg_ssim_bwd", a.data_ptr(), b.data_ptr(), B, Cn, H, W, _strides(a), _strides(b), v.data_ptr(),
             d_m1.data_ptr(), d_s1.data_ptr(), d_s12.data_ptr(), v_img1.data_ptr(), stream())
        return v_img1, None, None


def _check(img1: Tensor, img2: Tensor, padding: str) -> None:
    if padding not in ("same", "valid"):
        raise ValueError(f"padding must be 'same' or 'valid', got {padding!r}")
    if img1.dim() != 4 or img2.dim() != 4:
        raise ValueError(f"img1 and img2 must be [B, C, H, W], got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.shape != img2.shape:
        raise ValueError(f"img1 and img2 must have one shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.numel() == 0:
        raise ValueError(f"img1 and img2 must not be empty, got {tuple(img1.shape)}")
    if padding == "valid" and min(img1.shape[2], img1.shape[3]) < 2 * RADIUS + 1:
        raise ValueError(f"padding='valid' needs H, W >= {2 * RADIUS + 1}, got {tuple(img1.shape)}")
    for t, name in ((img1, "img1"), (img2, "img2")):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if img2.requires_grad:
        raise ValueError("img2 must not require grad: SSIM is symmetric, pass the tensor that needs the gradient first")
    for t, name in ((img1, "img1"), (img2, "img2")):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (got {t.device}); edgegaussians_amd has no CPU path")


def _map(img1: Tensor, img2: Tensor, padding: str, train: bool) -> Tensor:
    _check(img1, img2, padding)
    if train and torch.is_grad_enabled() and img1.requires_grad:
        S = _SSIMMap.apply(img1, img2, True)
    else:
        with torch.no_grad():
            S = _SSIMMap.apply(img1, img2, False)
    return S if padding == "same" else S[:, :, RADIUS:-RADIUS, RADIUS:-RADIUS]


def ssim_map(img1: Tensor, img2: Tensor, padding: str = "same") -> Tensor:
    """The SSIM map of ``img1`` against ``img2`` (module docstring): ``[B, C, H, W]``, or with ``padding="valid"`` its
    crop by 5 on every side.  Differentiable in ``img1``."""
    return _map(img1, img2, padding, True)


def fused_ssim(img1: Tensor, img2: Tensor, padding: str = "same", train: bool = True) -> Tensor:
    """``fused_ssim.fused_ssim``: the scalar ``ssim_map(img1, img2, padding).mean()``, differentiable in ``img1``.  With
    ``train=False`` -- or when ``img1`` needs no gradient, or under ``no_grad`` -- the derivative maps are neither
    allocated nor written and the result has no ``grad_fn``; its value is bit-equal to the ``train=True`` value."""
    return _map(img1, img2, padding, train).mean()
