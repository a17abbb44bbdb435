"""Bilateral grid of gsplat's trainers (``--use_bilateral_grid``: ``lib_bilagrid.py`` / the ``fused_bilagrid``
package) on the kernels of csrc/bilagrid.hip: ``slice`` -- the trilinear slice of a per-image lattice of 3x4 affine
colour transforms, applied to the render in the same pass --, ``total_variation_loss`` and the ``BilateralGrid``
module.  No CPU path, no torch fall-back.

Neither ``fused_bilagrid`` nor gsplat's ``lib_bilagrid.py`` was at hand when this was written: the semantics below are
restated from memory of both and defined here in closed form, so nothing depends on that memory being exact.
tests/bilagrid_util.py states exactly this in float64.

Inputs

* ``grids``: ``[N, 12, L, Hg, Wg]``, fp32, contiguous, on the device; every size >= 1.  (Or a ``BilateralGrid``.)
* ``rgb``: ``[B, ..., 3]`` fp32; ``xy``: the same leading shape with a last dimension of 2, fp32, nominally in [0, 1];
  ``x`` indexes ``Wg``, ``y`` indexes ``Hg``.
* ``grid_idx``: integer (int32 / int64) ``[B]`` or ``[B, 1]``, or ``None`` when ``B == N``: image ``b`` uses
  ``grids[grid_idx[b]]``.  Indices may repeat (their grid gradients add) and may leave grids unused (their gradient is
  exactly 0).  The range check is one device reduction read back to the host with nothing else: a HOST SYNC.
  ``check_idx=False`` skips it; the kernels then clamp an index outside ``[0, N)`` into it.

Forward

* ``gray = 0.299 r + 0.587 g + 0.114 b`` with fp32 constants, added in that order.
* ``u = clamp(x (Wg - 1), 0, Wg - 1)``, ``v = clamp(y (Hg - 1), 0, Hg - 1)``, ``w = clamp(gray (L - 1), 0, L - 1)``:
  in exact arithmetic ``grid_sample(grids, cat(2 xy - 1, 2 gray - 1), mode="bilinear", align_corners=True,
  padding_mode="border")``, coordinates outside [-1, 1] included.
* Along each axis of size n: ``i0 = min(floor(u), n - 2)`` (0 when n == 1), ``t = u - i0``, weights ``(1 - t, t)``.
* ``A`` = the sum over the 8 corners of ``w_corner * grids[g, :, l, j, i]``: 12 numbers, a row-major 3x4.
  ``out_c = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3]``.
* ``slice(...)`` returns ``{"rgb": out}``, ``out`` contiguous in the shape of ``rgb``.  The ``[..., 3, 4]`` matrices are
  never materialised: the key ``"rgb_affine_mats"`` of the original is ABSENT.
* The kernel evaluates ``A`` as nested lerps ``a + t (b - a)``, so grids that are constant over their cells -- the
  identity initialisation -- give ``out == rgb`` bit for bit.

Backward, for a cotangent ``v`` of ``out``

* ``v_A[c,k] = v_c (r, g, b, 1)_k``; ``v_grids[g, :, corner] += w_corner v_A``.
* ``v_rgb_k = sum_c v_c A[c,k] + gw_k (L - 1) gate sum_{c,k'} v_A[c,k'] dA[c,k']/dw``: ``dA/dw`` the bilinear xy blend of
  ``grids[l0 + 1] - grids[l0]``, ``gw = (0.299, 0.587, 0.114)``, ``gate = 1`` exactly when ``0 < gray (L - 1) < L - 1``
  (torch's border rule: no gradient at and beyond both ends); 0 for ``L == 1``.
* ``xy`` receives no gradient: ``xy.requires_grad`` is a ValueError.  ``rgb`` and ``grids`` each receive one only if
  they require it; the scatter into ``v_grids`` does not run when ``grids`` do not.
* ``v_rgb`` is a pure map: the same bits every run.  ``v_grids`` is summed with float atomics (in LDS per workgroup,
  then one flush per non-zero word; csrc/bilagrid.hip): it is NOT bit-reproducible, the sums differ in their last bits
  with the order of arrival.  ``scatter_path`` says which of the two scatter kernels a grid size takes.

``total_variation_loss(grids)``: the scalar sum over the axes a of (L, Hg, Wg) with ``n_a > 1`` of
``mean((x[.. i + 1 ..] - x[.. i ..])^2)``, the mean over all ``N * 12 * (n_a - 1) * (the other two sizes)`` differences.
An axis of size 1 contributes 0 (the torch original divides 0 by 0 there).  Backward:
``v_x = v sum_a (2 / count_a) ((x - x_prev) [if prev exists] - (x_next - x) [if next exists])``.  Partial sums in a slab
and a one-wave finalize forward, one gather pass backward: no atomics, the same bits every run.

Layouts: ``rgb`` and ``xy`` are read through their element strides (the convention of ``losses``: four host strides of
the logical ``[B, H, W, last]`` problem), without a copy, when the last stride is 1 or the tensor is dense: the
contiguous ``[C, H, W, 3]`` render of ``rasterization``, ``render[..., :3]`` of an ``RGB+D`` render, one mesh grid
``expand``ed over the batch (stride 0).  Anything else takes one ``.contiguous()``.

Checks, before any launch, structure first so that every one of them can be met without a device: ``grids`` not 5-D
with 12 channels, last dimensions other than 3 and 2, leading shapes that differ, a ``grid_idx`` that is not ``[B]`` /
``[B, 1]`` (or ``None`` with ``B != N``), an empty tensor, 2^31 samples or more (ValueError -- a count is structure, and
here, before the device check, it can be met without a device: by an ``expand``ed CPU tensor); a dtype other than fp32,
a ``grid_idx`` that is not int32 / int64 (TypeError); ``xy.requires_grad`` (ValueError); a CPU tensor (ValueError, "no
CPU path").  Then the range of ``grid_idx`` (ValueError; the host sync).

Under ``no_grad``, or when neither ``rgb`` nor ``grids`` requires grad, nothing is saved and no derivative work is
done; the values are bit-equal to the training-mode values."""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch import Tensor, nn

from ._lib import call, stream
from .losses import _strides
from .ssim import _dense

LDS_BUDGET_BYTES = 96 * 1024   # EG_BILAGRID_LDS_BUDGET (include/edgegs.h)
MAP_THREADS = 1024             # lanes per persistent workgroup of the forward and v_rgb kernels (csrc/bilagrid.hip: kMapThreads)
SCATTER_THREADS = 1024         # lanes per workgroup of the LDS scatter (kScatterThreads)
TV_WG_ELEMS = 1024             # cells per workgroup of the TV forward (kTvPerWG)
FIN_LANES = 64                 # lanes of the TV finalize kernel (kFinLanes)
MAX_SAMPLES = 2 ** 31 - 1
MAX_WORKGROUPS = 256           # persistent workgroups of the LDS kernels over all images (kPersistentWGs: one per CU); a
                               # smaller value makes one workgroup walk more blocks of samples and changes no bit of
                               # out or v_rgb (tests lower it to run the loops of the persistent kernels at small sizes)


def scatter_path(L: int, Hg: int, Wg: int) -> str:
    """"lds" while one grid's gradient (48 L Hg Wg bytes) fits LDS_BUDGET_BYTES, else "global": the kernel the
    backward's scatter into ``v_grids`` takes (csrc/bilagrid.hip)."""
    return "lds" if 48 * L * Hg * Wg <= LDS_BUDGET_BYTES else "global"


class BilateralGrid(nn.Module):
    """``num`` grids ``[12, grid_W, grid_Y, grid_X]`` (guidance, y, x), initialised to the identity transform
    (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0) in every cell."""

    def __init__(self, num: int, grid_X: int = 16, grid_Y: int = 16, grid_W: int = 8):
        super().__init__()
        self.grid_width, self.grid_height, self.grid_guidance = grid_X, grid_Y, grid_W
        eye = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0], dtype=torch.float32)
        self.grids = nn.Parameter(eye.view(1, 12, 1, 1, 1).repeat(num, 1, grid_W, grid_Y, grid_X))

    def tv_loss(self) -> Tensor:
        return total_variation_loss(self.grids)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("BilateralGrid.forward returns the per-pixel affine matrices in the original; the fused "
                                  "slice exists so that they are never built: call bilagrid.slice(grid, xy, rgb, grid_idx)")


def _samples4(t: Tensor) -> Tensor:
    """[B, ..., k] as the logical [B, H, W, k] problem, in place when the last stride is 1 or t is dense.  (The strides
    travel as in ``losses`` -- ``_strides``, four host strides, 0 allowed -- but ``losses._in_place`` cannot make this
    decision: it asks for density up to ONE skipped stride, and ``render[..., :3]`` of a ``[C, H, W, 4]`` render skips a
    stride that is no multiple of the extent below it, 4 against 3, while an ``expand``ed ``xy`` has stride 0 on top.
    The kernels only read through these strides, one lane per sample, so a last stride of 1 is all they need.)"""
    if not (t.stride(-1) == 1 or _dense(t)):
        t = t.contiguous()
    if t.dim() == 4:
        return t
    if t.dim() < 4:
        return t.reshape((t.shape[0],) + (1,) * (4 - t.dim()) + tuple(t.shape[1:]))
    return t.flatten(1, -3)  # (a view where the strides allow it)


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, rgb, xy, idx, train):
        N, _, L, Hg, Wg = grids.shape
        B, H, W, _ = rgb.shape
        out = torch.empty((B, H, W, 3), dtype=torch.float32, device=rgb.device)
        head = (grids.data_ptr(), N, L, Hg, Wg, rgb.data_ptr(), xy.data_ptr(), idx.data_ptr() if idx is not None else None,
                int(idx is not None and idx.dtype == torch.int64), B, H, W, _strides(rgb), _strides(xy), MAX_WORKGROUPS)
        call("eg_bilagrid_slice_fwd", *head, out.data_ptr(), stream())
        if train:
            ctx.head = head
            ctx.save_for_backward(grids, rgb, xy, idx)
        return out

    @staticmethod
    def backward(ctx, v):
        grids, rgb, xy, idx = ctx.saved_tensors
        need_grids, need_rgb = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_grids or need_rgb):
            return None, None, None, None, None
        v = v.contiguous()
        v_rgb = torch.empty(rgb.shape, dtype=torch.float32, device=rgb.device) if need_rgb else None
        v_grids = torch.zeros_like(grids) if need_grids else None
        call("eg_bilagrid_slice_bwd", *ctx.head, v.data_ptr(), v_rgb.data_ptr() if need_rgb else None,
             v_grids.data_ptr() if need_grids else None, stream())
        return v_grids, v_rgb, None, None, None


def _check_slice(grids: Tensor, xy: Tensor, rgb: Tensor, grid_idx: Optional[Tensor]) -> None:
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"grids must be [N, 12, L, Hg, Wg], got {tuple(grids.shape)}")
    if not grids.is_contiguous():
        raise ValueError(f"grids must be contiguous, got strides {tuple(grids.stride())}")
    if rgb.dim() < 2 or rgb.shape[-1] != 3:
        raise ValueError(f"rgb must be [B, ..., 3], got {tuple(rgb.shape)}")
    if xy.dim() < 2 or xy.shape[-1] != 2:
        raise ValueError(f"xy must be [B, ..., 2], got {tuple(xy.shape)}")
    if xy.shape[:-1] != rgb.shape[:-1]:
        raise ValueError(f"xy and rgb must share their leading shape, got {tuple(xy.shape)} and {tuple(rgb.shape)}")
    B, N = rgb.shape[0], grids.shape[0]
    if grid_idx is None:
        if B != N:
            raise ValueError(f"grid_idx may be None only when B == N, got B = {B} and N = {N}")
    elif tuple(grid_idx.shape) not in ((B,), (B, 1)):
        raise ValueError(f"grid_idx must be [B] or [B, 1] with B = {B}, got {tuple(grid_idx.shape)}")
    for t, name in ((grids, "grids"), (rgb, "rgb")):
        if t.numel() == 0:
            raise ValueError(f"{name} must not be empty, got {tuple(t.shape)}")
    if rgb.numel() // 3 > MAX_SAMPLES:
        raise ValueError(f"rgb must have fewer than 2^31 samples, got {rgb.numel() // 3}")
    for t, name in ((grids, "grids"), (rgb, "rgb"), (xy, "xy")):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if grid_idx is not None and grid_idx.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"grid_idx must be torch.int32 or torch.int64, got {grid_idx.dtype}")
    if xy.requires_grad:
        raise ValueError("xy must not require grad: the slice has no gradient of the coordinates")
    for t, name in ((grids, "grids"), (rgb, "rgb"), (xy, "xy")) + (((grid_idx, "grid_idx"),) if grid_idx is not None else ()):
        if not t.is_cuda:
            raise ValueError(f"{name} must be a device tensor (got {t.device}); edgegaussians_amd has no CPU path")


def slice(bil_grids: Union[BilateralGrid, Tensor], xy: Tensor, rgb: Tensor, grid_idx: Optional[Tensor] = None, *,
          check_idx: bool = True) -> dict:
    """``{"rgb": out}``: ``rgb`` under the affine transform sliced from image ``b``'s grid at ``(x, y, luminance)``
    (module docstring); differentiable in ``rgb`` and the grids.  With ``check_idx`` (the default) the range of
    ``grid_idx`` is checked, which is a host sync."""
    grids = bil_grids.grids if isinstance(bil_grids, BilateralGrid) else bil_grids
    _check_slice(grids, xy, rgb, grid_idx)
    idx = None
    if grid_idx is not None:
        idx = grid_idx.detach().reshape(-1).contiguous()
        if check_idx:
            lo, hi = torch.stack(torch.aminmax(idx)).tolist()  # (one reduction, one read-back: the host sync)
            if lo < 0 or hi >= grids.shape[0]:
                raise ValueError(f"grid_idx must lie in [0, {grids.shape[0]}), got values from {lo} to {hi}")
    rgb4, xy4 = _samples4(rgb), _samples4(xy)
    if torch.is_grad_enabled() and (rgb.requires_grad or grids.requires_grad):
        out = _Slice.apply(grids, rgb4, xy4, idx, True)
    else:
        with torch.no_grad():
            out = _Slice.apply(grids, rgb4, xy4, idx, False)
    return {"rgb": out.view(rgb.shape)}


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, train):
        N, _, L, Hg, Wg = grids.shape
        G = -(-grids.numel() // TV_WG_ELEMS)
        slab = torch.empty(G, dtype=torch.float32, device=grids.device)
        out = torch.empty(1, dtype=torch.float32, device=grids.device)
        call("eg_bilagrid_tv_fwd", grids.data_ptr(), N, L, Hg, Wg, slab.data_ptr(), G, out.data_ptr(), stream())
        if train:
            ctx.save_for_backward(grids)
        return out[0]

    @staticmethod
    def backward(ctx, v):
        grids, = ctx.saved_tensors
        N, _, L, Hg, Wg = grids.shape
        v = v.contiguous()
        g = torch.empty_like(grids)
        call("eg_bilagrid_tv_bwd", grids.data_ptr(), N, L, Hg, Wg, v.data_ptr(), g.data_ptr(), stream())
        return g, None


def total_variation_loss(grids: Tensor) -> Tensor:
    """The total variation of all grids as a 0-dim tensor (module docstring), differentiable in ``grids``."""
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"grids must be [N, 12, L, Hg, Wg], got {tuple(grids.shape)}")
    if grids.numel() == 0:
        raise ValueError(f"grids must not be empty, got {tuple(grids.shape)}")
    if grids.numel() > MAX_SAMPLES:
        raise ValueError(f"grids must have fewer than 2^31 elements, got {grids.numel()}")
    if grids.dtype != torch.float32:
        raise TypeError(f"grids must be torch.float32, got {grids.dtype}")
    if not grids.is_cuda:
        raise ValueError(f"grids must be a device tensor (got {grids.device}); edgegaussians_amd has no CPU path")
    x = grids if grids.is_contiguous() else grids.contiguous()
    if torch.is_grad_enabled() and grids.requires_grad:
        return _TotalVariation.apply(x, True)
    with torch.no_grad():
        return _TotalVariation.apply(x, False)
