"""gsplat 1.0.0's stage-by-stage API over the kernels `rasterization` runs: ``fully_fused_projection``,
``quat_scale_to_covar_preci``, ``isect_tiles``, ``isect_offset_encode``, ``rasterize_to_pixels``,
``rasterize_to_indices_in_range``, ``accumulate``, ``world_to_cam``, ``persp_proj`` and ``proj``, with gsplat's signatures and
return orders.

Callers use the stages when they change something between them -- shift ``means2d``, substitute their own conics or
opacities, render Gaussians that exist only as covariances, re-bin with another tile grid.  The projection from
``quats`` + ``scales``, the binning and the compositing are the very kernels behind ``rasterization(packed=False)``;
the projection from ``covars``, ``quat_scale_to_covar_preci`` and ``isect_offset_encode`` have kernels of their own
(csrc/functional.hip), and so have the per-pixel intersection lists -- ``rasterize_to_indices_in_range``, which walks a
range of every tile's list exactly as the compositing does and returns the (pixel, Gaussian) pairs it takes, and
``accumulate``, which composites such pairs (csrc/indices.hip).  ``world_to_cam``, ``persp_proj`` and ``proj`` are plain
differentiable torch expressions (not a hot path; they work on CPU tensors too).  Everything else needs device
tensors: there is no CPU path.

``fully_fused_projection`` and ``proj`` take gsplat's ``camera_model``: "pinhole" (the default) or "ortho" (the
orthographic camera of ``rasterization(camera_model="ortho")``, in both forms of the projection); "fisheye" is a
NotImplementedError, anything else a ValueError.

Not supported, each a NotImplementedError: ``packed=True`` (use ``rasterization(packed=True)``), ``sparse_grad=True``,
``sort=False``, ``masks``, and a ``viewmats`` that requires grad together with ``covars``."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import rasterizer as _R
from ._lib import call, ptr, stream
from . import _lib
from .rasterizer import TILE, TILE_SIZES, _check, _is_ortho

__all__ = ["fully_fused_projection", "quat_scale_to_covar_preci", "isect_tiles", "isect_offset_encode",
           "rasterize_to_pixels", "rasterize_to_indices_in_range", "accumulate", "world_to_cam", "persp_proj", "proj"]


def _no_packed(packed, what):
    if packed:
        raise NotImplementedError(f"{what}: packed=True is not available in the functional stages; use rasterization(packed=True)")


def _tile_size(tile_size):
    if isinstance(tile_size, bool) or tile_size not in TILE_SIZES:
        raise NotImplementedError(f"tile_size must be 8, 16 or 32, got {tile_size!r}")
    return int(tile_size)


# ----------------------------------------------------------------------------------------------------------------
class _QuatScaleToCovarPreci(torch.autograd.Function):
    """eg_quat_scale_to_covar_preci_fwd / _bwd: one lane per Gaussian."""

    @staticmethod
    def forward(ctx, quats, scales, compute_covar, compute_preci, triu):
        N, dev = quats.shape[0], quats.device
        q, s = quats.contiguous(), scales.contiguous()
        shape = (N, 6) if triu else (N, 3, 3)
        covars = torch.empty(shape, device=dev) if compute_covar else None
        precis = torch.empty(shape, device=dev) if compute_preci else None
        call("eg_quat_scale_to_covar_preci_fwd", ptr(q), ptr(s), N, int(triu), ptr(covars), ptr(precis), stream())
        ctx.save_for_backward(q, s)
        ctx.cfg = (bool(triu), compute_covar, compute_preci)
        # (an output that is not computed is a placeholder autograd never differentiates; the wrapper returns None)
        empty = torch.empty(0, device=dev)
        if not compute_covar or not compute_preci:
            ctx.mark_non_differentiable(empty)
        return (covars if compute_covar else empty), (precis if compute_preci else empty)

    @staticmethod
    def backward(ctx, v_covars, v_precis):
        q, s = ctx.saved_tensors
        triu, compute_covar, compute_preci = ctx.cfg
        N, dev = q.shape[0], q.device
        vc = v_covars.contiguous() if (compute_covar and v_covars is not None) else None
        vp = v_precis.contiguous() if (compute_preci and v_precis is not None) else None
        v_quats = torch.empty(N, 4, device=dev)
        v_scales = torch.empty(N, 3, device=dev)
        call("eg_quat_scale_to_covar_preci_bwd", ptr(q), ptr(s), N, int(triu), ptr(vc), ptr(vp), ptr(v_quats), ptr(v_scales),
             stream())
        return v_quats, v_scales, None, None, None


def quat_scale_to_covar_preci(quats: Tensor, scales: Tensor, compute_covar: bool = True, compute_preci: bool = True,
                              triu: bool = False) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """gsplat ``quat_scale_to_covar_preci``: ``covars = R diag(s^2) R^T`` and ``precis = R diag(1 / s^2) R^T`` from
    ``quats`` [N,4] (w, x, y, z; normalised inside) and ``scales`` [N,3]; ``[N,3,3]``, or with ``triu`` the upper
    triangle ``[N,6]`` = (00, 01, 02, 11, 12, 22).  An output that is not computed is ``None``."""
    N = quats.shape[0]
    _check(quats, (N, 4), "quats")
    _check(scales, (N, 3), "scales")
    if not compute_covar and not compute_preci:
        return None, None
    covars, precis = _QuatScaleToCovarPreci.apply(quats, scales, bool(compute_covar), bool(compute_preci), bool(triu))
    return (covars if compute_covar else None), (precis if compute_preci else None)


# ----------------------------------------------------------------------------------------------------------------
def fully_fused_projection(means: Tensor, covars: Optional[Tensor], quats: Optional[Tensor], scales: Optional[Tensor],
                           viewmats: Tensor, Ks: Tensor, width: int, height: int, eps2d: float = 0.3,
                           near_plane: float = 0.01, far_plane: float = 1e10, radius_clip: float = 0.0,
                           packed: bool = False, sparse_grad: bool = False, calc_compensations: bool = False,
                           camera_model: str = "pinhole"):
    """gsplat ``fully_fused_projection`` (packed=False): ``(radii [C,N] int32, means2d [C,N,2], depths [C,N], conics
    [C,N,3], compensations [C,N] | None)``; a culled pair has radius 0 and zeros in every float output.

    Exactly one of ``covars`` [N,6] (upper triangle) and ``quats`` [N,4] + ``scales`` [N,3] must be given (ValueError).
    With ``quats`` + ``scales`` this is the projection node of ``rasterization`` -- the same kernels, the same bits, and
    ``viewmats`` receives its gradient when it requires one.  With ``covars`` a kernel pair of its own; ``viewmats``
    must not require grad there (NotImplementedError): the pose gradient of the covariance form is reachable through
    ``rasterization(covars=[N, 3, 3])``, as are ``packed=True`` and ``sparse_grad``.

    ``camera_model``: "pinhole" or "ortho" (``means2d = (fx x + cx, fy y + cy)``, the constant Jacobian ``[[fx, 0, 0],
    [0, fy, 0]]``, no fov clamp; see ``rasterization``), in both forms; checked before any tensor is looked at."""
    ortho = _is_ortho(camera_model)
    _no_packed(packed, "fully_fused_projection")
    if sparse_grad:
        raise NotImplementedError("fully_fused_projection: sparse_grad=True needs packed=True; use rasterization(packed=True, sparse_grad=True)")
    have_qs = quats is not None or scales is not None
    if (covars is None) == (not have_qs) or (have_qs and (quats is None or scales is None)):
        raise ValueError("fully_fused_projection: give either covars, or quats and scales (exactly one of the two forms)")
    N, Cn = means.shape[0], viewmats.shape[0]
    _check(means, (N, 3), "means")
    _check(viewmats, (Cn, 4, 4), "viewmats")
    _check(Ks, (Cn, 3, 3), "Ks")
    width, height = int(width), int(height)
    cfg = (float(eps2d), float(near_plane), float(far_plane), float(radius_clip))
    if covars is None:
        _check(quats, (N, 4), "quats")
        _check(scales, (N, 3), "scales")
        dummy = torch.ones(N, device=means.device)  # (the record's opacity: nobody reads the record here)
        radii, means2d, depths, conics, comps = _R._Projection.apply(
            means, quats, scales, dummy, viewmats, Ks, width, height, *cfg, bool(calc_compensations), TILE, ortho)[:5]
        return radii, means2d, depths, conics, (comps if calc_compensations else None)
    _check(covars, (N, 6), "covars")
    if viewmats.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("fully_fused_projection: the gradient of viewmats is not available with covars; pass quats and scales")
    # (the dense covariance node of `rasterization`, as a stage: no record, no tile counts, [N, 6] in and out)
    radii, means2d, depths, conics, comps = _R._CovarProjection.apply(
        means, covars, None, viewmats, Ks, width, height, *cfg, bool(calc_compensations), TILE, ortho, True)[:5]
    return radii, means2d, depths, conics, (comps if calc_compensations else None)


# ----------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def isect_tiles(means2d: Tensor, radii: Tensor, depths: Tensor, tile_size: int, tile_width: int, tile_height: int,
                sort: bool = True, packed: bool = False, n_cameras: Optional[int] = None,
                camera_ids: Optional[Tensor] = None, gaussian_ids: Optional[Tensor] = None):
    """gsplat ``isect_tiles`` (packed=False, sort=True): ``(tiles_per_gauss [C,N] int32, isect_ids [M] int64,
    flatten_ids [M] int32)`` for ``means2d`` [C,N,2], ``radii`` [C,N] int32 and ``depths`` [C,N] on a grid of
    ``tile_width`` x ``tile_height`` tiles of ``tile_size`` (8, 16 or 32) pixels.  ``isect_ids`` = camera << (32 +
    tile_bits) | tile << 32 | depth bits, sorted; ``flatten_ids`` = c * N + n.  One host read-back (the M_c)."""
    _no_packed(packed, "isect_tiles")
    if not sort:
        raise NotImplementedError("isect_tiles: sort=False is not available (the emission and the sort are one native call)")
    tile_size = _tile_size(tile_size)
    if means2d.dim() != 3:
        raise ValueError(f"means2d must have shape (C, N, 2), got {tuple(means2d.shape)}")
    Cn, N = means2d.shape[0], means2d.shape[1]
    _check(means2d, (Cn, N, 2), "means2d")
    _check(radii, (Cn, N), "radii", torch.int32)
    _check(depths, (Cn, N), "depths")
    tw, th = int(tile_width), int(tile_height)
    if tw < 1 or th < 1:
        raise ValueError(f"tile_width and tile_height must be positive, got {tile_width!r}, {tile_height!r}")
    if n_cameras is not None and int(n_cameras) != Cn:
        raise ValueError(f"n_cameras is {n_cameras}, means2d holds {Cn} cameras")
    dev = means2d.device
    width, height = tw * tile_size, th * tile_size
    T = tw * th
    m2, rd, dp = means2d.detach().contiguous(), radii.contiguous(), depths.detach().contiguous()
    tpg = torch.zeros(Cn, N, dtype=torch.int32, device=dev)
    if N == 0:
        return tpg, torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    counts = torch.zeros(Cn, T, dtype=torch.int32, device=dev)
    ranges = [c * N for c in range(Cn + 1)]
    _R.count_tiles(m2, rd, ranges, width, height, tile_size, tpg, counts)
    info = _R.bin_tiles(m2, rd, dp, ranges, counts, width, height, tile_size, packed=False).info
    return tpg, info["isect_ids"], info["flatten_ids"]


@torch.no_grad()
def isect_offset_encode(isect_ids: Tensor, n_cameras: int, tile_width: int, tile_height: int) -> Tensor:
    """gsplat ``isect_offset_encode``: ``offsets [C, tile_height, tile_width]`` int32 from SORTED ``isect_ids`` [M]
    int64, ``offsets[c, i, j]`` = the number of entries whose (camera, tile) is below (c, i * tile_width + j).  No host
    read-back (eg_isect_offset_encode)."""
    if isect_ids.dim() != 1:
        raise ValueError(f"isect_ids must have shape (M,), got {tuple(isect_ids.shape)}")
    M = isect_ids.shape[0]
    _check(isect_ids, (M,), "isect_ids", torch.int64)
    Cn, tw, th = int(n_cameras), int(tile_width), int(tile_height)
    if Cn < 1 or tw < 1 or th < 1:
        raise ValueError(f"n_cameras, tile_width and tile_height must be positive, got {n_cameras!r}, {tile_width!r}, {tile_height!r}")
    offsets = torch.empty(Cn, th, tw, dtype=torch.int32, device=isect_ids.device)
    ids = isect_ids.contiguous()
    call("eg_isect_offset_encode", ptr(ids) if M > 0 else None, M, Cn, tw, th, ptr(offsets), stream())
    return offsets


# ----------------------------------------------------------------------------------------------------------------
def rasterize_to_pixels(means2d: Tensor, conics: Tensor, colors: Tensor, opacities: Tensor, image_width: int,
                        image_height: int, tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor,
                        backgrounds: Optional[Tensor] = None, masks: Optional[Tensor] = None, packed: bool = False,
                        absgrad: bool = False) -> Tuple[Tensor, Tensor]:
    """gsplat ``rasterize_to_pixels`` (packed=False): ``(render_colors [C,H,W,D], render_alphas [C,H,W,1])`` from
    ``means2d`` [C,N,2], ``conics`` [C,N,3], ``colors`` [C,N,D] (any D >= 1), ``opacities`` [C,N], ``isect_offsets``
    [C,th,tw] int32 and ``flatten_ids`` [M] int32 (c * N + n) as ``isect_tiles`` / ``isect_offset_encode`` return them.

    The record the compositing kernels read is built here from the caller's tensors (they may have changed since the
    projection), the global offsets become the kernels' per-camera form in torch (no host read-back), and the
    compositing is the kernel family ``rasterization`` takes for this (tile_size, D).  ``means2d`` receives
    ``.absgrad`` [C,N,2] in the backward with ``absgrad=True``."""
    _no_packed(packed, "rasterize_to_pixels")
    if masks is not None:
        raise NotImplementedError("rasterize_to_pixels: masks are not available")
    tile_size = _tile_size(tile_size)
    if means2d.dim() != 3:
        raise ValueError(f"means2d must have shape (C, N, 2), got {tuple(means2d.shape)}")
    Cn, N = means2d.shape[0], means2d.shape[1]
    width, height = int(image_width), int(image_height)
    tw, th = math.ceil(width / tile_size), math.ceil(height / tile_size)
    T = tw * th
    _check(means2d, (Cn, N, 2), "means2d")
    _check(conics, (Cn, N, 3), "conics")
    _check(opacities, (Cn, N), "opacities")
    if colors.dim() != 3 or colors.shape[-1] < 1:
        raise ValueError(f"colors must have shape (C, N, D) with D >= 1, got {tuple(colors.shape)}")
    D = colors.shape[-1]
    _check(colors, (Cn, N, D), "colors")
    if backgrounds is not None:
        _check(backgrounds, (Cn, D), "backgrounds")
    _check(isect_offsets, (Cn, th, tw), "isect_offsets", torch.int32)
    if flatten_ids.dim() != 1:
        raise ValueError(f"flatten_ids must have shape (M,), got {tuple(flatten_ids.shape)}")
    M = flatten_ids.shape[0]
    _check(flatten_ids, (M,), "flatten_ids", torch.int32)
    dev = means2d.device
    if N == 0:  # (nothing to composite: the backgrounds under a transmittance of one, on their graph)
        alphas = torch.zeros(Cn, height, width, 1, device=dev)
        render = (backgrounds[:, None, None, :].expand(Cn, height, width, D) if backgrounds is not None
                  else torch.zeros(Cn, height, width, D, device=dev))
        return render + colors.sum() * 0.0, alphas
    with torch.no_grad():
        # (x y a b c opacity | depth radius): the last two are read by kernels this path never runs
        splat = torch.cat([means2d, conics, opacities[..., None], torch.zeros(Cn, N, 2, device=dev)], dim=-1).contiguous()
        first = isect_offsets.reshape(Cn, T)
        ends = torch.cat([first[1:, 0], torch.full((1,), M, dtype=torch.int32, device=dev)])
        flat = (flatten_ids % N) if M > 0 else torch.zeros(1, dtype=torch.int32, device=dev)
        # the cameras' lists one after the other, every row of offsets local to its camera's list
        # (clamped into the list: offsets outside it must not send a kernel outside `flatten_ids`)
        local = torch.cat([first - first[:, :1], (ends - first[:, 0])[:, None]], dim=1).clamp_(0, M).contiguous()
    opac = opacities.contiguous()
    if tile_size != TILE or D not in (1, 3):
        render, alphas, _ = _R._TileCompositing.apply(means2d, conics, colors, opac, None, backgrounds, width, height, local,
                                                      flat, bool(absgrad), splat, False, 32, tile_size)
    elif backgrounds is not None:
        render, alphas, _ = _R._ModeCompositing.apply(means2d, conics, colors, opac, None, backgrounds, width, height, local,
                                                      flat, bool(absgrad), splat, False)
    else:
        # the per-camera entry takes one list per camera: the whole list with the GLOBAL offsets of that camera's tiles
        with torch.no_grad():
            glob = torch.cat([first, ends[:, None]], dim=1).clamp_(0, M).contiguous()
        render, alphas, _ = _R._Compositing.apply(means2d, conics, colors, opac, width, height,
                                                  tuple(glob[c] for c in range(Cn)), (flat,) * Cn, bool(absgrad), False,
                                                  (None,) * Cn, (None,) * Cn, (0,) * Cn, splat)
    return render, alphas


# ----------------------------------------------------------------------------------------------------------------
_RANGE_MAX = 2 ** 31 - 1  # (more batches than any int32-indexed list has)


def _clamp_range(range_start, range_end):
    """The batch range as the entries take it (int32): negative bounds are a ValueError, huge ones are clamped."""
    rs, re = int(range_start), int(range_end)
    if rs < 0 or re < 0:
        raise ValueError(f"range_start and range_end must not be negative, got {range_start!r}, {range_end!r}")
    return min(rs, _RANGE_MAX), min(re, _RANGE_MAX)


@torch.no_grad()
def rasterize_to_indices_in_range(range_start: int, range_end: int, transmittances: Tensor, means2d: Tensor,
                                  conics: Tensor, opacities: Tensor, image_width: int, image_height: int,
                                  tile_size: int, isect_offsets: Tensor, flatten_ids: Tensor
                                  ) -> Tuple[Tensor, Tensor, Tensor]:
    """gsplat ``rasterize_to_indices_in_range``: which Gaussians reach which pixel, in depth order.  Returns
    ``(gaussian_ids [M], pixel_ids [M], camera_ids [M])``, all int64, one row per (pixel, Gaussian) pair the walk of
    ``rasterize_to_pixels`` composites, in ascending ``(camera, pixel_id = i * W + j)`` order and in list order inside
    a pixel; ``gaussian_ids = flatten_id % N``.

    ``transmittances`` [C,H,W], ``means2d`` [C,N,2], ``conics`` [C,N,3], ``opacities`` [C,N] fp32; ``isect_offsets``
    [C,th,tw] int32 and ``flatten_ids`` int32 as ``isect_tiles`` / ``isect_offset_encode`` return them.

    Per call: a tile's sorted list is cut into batches of ``tile_size ** 2`` entries, and the call looks only at the
    batches ``b`` with ``range_start <= b < range_end`` (``range_end`` may be huge).  Pixel (i, j) of camera c starts
    with ``T = transmittances[c, i, j]`` and walks those batches of its own tile: centre (j + 0.5, i + 0.5), ``alpha
    = min(0.999, opacity * exp(-sigma))``, an entry with ``sigma < 0`` or ``alpha < 1/255`` is skipped, the walk stops
    for the rest of THIS CALL before an entry that would give ``T (1 - alpha) <= 1e-4``, every other entry is recorded
    and ``T <- T (1 - alpha)``.  The stop is not remembered between calls: a later call with a larger ``range_start``
    resumes the walk from the ``T`` it is given (as in gsplat), so a caller who slices the list carries ``T`` forward
    with ``accumulate`` (``T <- T (1 - alphas)``).

    Two passes of one kernel (count, int64 scan, write), no atomics: the same bits every run.  One host read-back
    (the number of rows)."""
    tile_size = _tile_size(tile_size)
    rs, re = _clamp_range(range_start, range_end)
    if means2d.dim() != 3:
        raise ValueError(f"means2d must have shape (C, N, 2), got {tuple(means2d.shape)}")
    Cn, N = means2d.shape[0], means2d.shape[1]
    width, height = int(image_width), int(image_height)
    if width < 0 or height < 0:
        raise ValueError(f"image_width and image_height must not be negative, got {image_width!r}, {image_height!r}")
    tw, th = math.ceil(width / tile_size), math.ceil(height / tile_size)
    T = tw * th
    _check(transmittances, (Cn, height, width), "transmittances")
    _check(means2d, (Cn, N, 2), "means2d")
    _check(conics, (Cn, N, 3), "conics")
    _check(opacities, (Cn, N), "opacities")
    _check(isect_offsets, (Cn, th, tw), "isect_offsets", torch.int32)
    if flatten_ids.dim() != 1:
        raise ValueError(f"flatten_ids must have shape (M,), got {tuple(flatten_ids.shape)}")
    M = flatten_ids.shape[0]
    _check(flatten_ids, (M,), "flatten_ids", torch.int32)
    dev = means2d.device
    P = Cn * height * width
    empty = tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(3))
    if P == 0 or N == 0 or M == 0 or re <= rs:
        return empty
    # the cameras' lists one after the other, every row of offsets local to its camera's list and clamped into the
    # list, the ids as Gaussian indices: what rasterize_to_pixels hands its kernels
    first = isect_offsets.reshape(Cn, T)
    ends = torch.cat([first[1:, 0], torch.full((1,), M, dtype=torch.int32, device=dev)])
    local = torch.cat([first - first[:, :1], (ends - first[:, 0])[:, None]], dim=1).clamp_(0, M).contiguous()
    flat = flatten_ids % N
    m2, con, op, tr = (t.detach().contiguous() for t in (means2d, conics, opacities, transmittances))
    args = (Cn, N, ptr(m2), ptr(con), ptr(op), ptr(tr), ptr(local), ptr(flat), M, width, height, tile_size, rs, re)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    call("eg_indices_count", *args, ptr(counts), stream())
    csum = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(csum[-1].item())  # the one read-back
    if total < 0 or total >= 2 ** 62:
        raise RuntimeError(f"rasterize_to_indices_in_range: the number of rows ({total}) does not fit")
    if total == 0:
        return empty
    starts = csum - counts
    gaussian_ids = torch.empty(total, dtype=torch.int64, device=dev)
    pixel_ids = torch.empty(total, dtype=torch.int64, device=dev)
    camera_ids = torch.empty(total, dtype=torch.int64, device=dev)
    call("eg_indices_write", *args, ptr(starts), total, ptr(gaussian_ids), ptr(pixel_ids), ptr(camera_ids), stream())
    return gaussian_ids, pixel_ids, camera_ids


_ACC_CHUNK = 32  # channels per launch of the segmented sums (the chunk width of the wide compositing)


class _Accumulate(torch.autograd.Function):
    """eg_accumulate_fwd / eg_accumulate_bwd: per pixel p, over the entries [starts[p], starts[p] + counts[p]) in order,
    renders[p] = sum_k alpha_k T_k feat_k and alphas[p] = sum_k alpha_k T_k with T_k the product of (1 - alpha) over the
    segment's earlier entries.  One lane per pixel, no atomics; D in chunks of 32 channels."""

    @staticmethod
    def forward(ctx, alpha, feat, starts, counts, P):
        M, D = feat.shape
        dev = feat.device
        a, f = alpha.contiguous(), feat.contiguous()
        renders = torch.empty(P, D, device=dev)
        alphas = torch.empty(P, device=dev)
        T_k = torch.empty(M, device=dev)
        for c0 in range(0, D, _ACC_CHUNK):
            head = c0 == 0
            call("eg_accumulate_fwd", ptr(a), ptr(f) + 4 * c0, D, min(_ACC_CHUNK, D - c0), ptr(starts), ptr(counts), P, M,
                 ptr(renders) + 4 * c0, D, ptr(alphas) if head else None, ptr(T_k) if head else None, stream())
        ctx.save_for_backward(a, f, starts, counts, T_k)
        ctx.P = P
        return renders, alphas

    @staticmethod
    def backward(ctx, v_renders, v_alphas):
        a, f, starts, counts, T_k = ctx.saved_tensors
        M, D = f.shape
        P, dev = ctx.P, f.device
        vr = v_renders.contiguous() if v_renders is not None else torch.zeros(P, D, device=dev)
        va = v_alphas.contiguous() if v_alphas is not None else None
        v_alpha = torch.empty(M, device=dev)
        v_feat = torch.empty(M, D, device=dev)
        for c0 in range(0, D, _ACC_CHUNK):
            head = c0 == 0
            call("eg_accumulate_bwd", ptr(a), ptr(f) + 4 * c0, D, min(_ACC_CHUNK, D - c0), ptr(starts), ptr(counts), P, M,
                 ptr(T_k), ptr(vr) + 4 * c0, D, ptr(va) if head else None, ptr(v_alpha), 0 if head else 1,
                 ptr(v_feat) + 4 * c0, stream())
        return v_alpha, v_feat, None, None, None


def accumulate(means2d: Tensor, conics: Tensor, opacities: Tensor, colors: Tensor, gaussian_ids: Tensor,
               pixel_ids: Tensor, camera_ids: Tensor, image_width: int, image_height: int) -> Tuple[Tensor, Tensor]:
    """gsplat ``accumulate``: alpha-composite the (pixel, Gaussian) pairs of ``rasterize_to_indices_in_range``.
    Returns ``(renders [C,H,W,D], alphas [C,H,W,1])``; differentiable in ``means2d`` [C,N,2], ``conics`` [C,N,3],
    ``opacities`` [C,N] and ``colors`` [C,N,D] (any D >= 1).  ``gaussian_ids`` / ``pixel_ids`` / ``camera_ids`` [M]
    int64.

    For entry k, ``alpha_k = min(0.999, opacity * exp(-sigma))`` of its (camera, Gaussian, pixel); there is NO 1/255
    skip and NO transmittance stop here.  Inside each (camera, pixel), in the order given, ``w_k = alpha_k * prod over
    the earlier k' of (1 - alpha_k')``; ``renders = sum w_k colors``, ``alphas = sum w_k``; pixels without entries are
    zero.

    PRECONDITION, not checked (checking would cost a host read-back): the entries are sorted by ``camera_ids * H * W +
    pixel_ids``, as ``rasterize_to_indices_in_range`` returns them, and every id is in range.  Unsorted entries give a
    wrong image (a pixel then walks a segment of its own LENGTH somewhere in the list), never an out-of-bounds access.

    The gathers and the per-entry alpha are torch operations on the autograd graph; the segmented products and sums
    are one kernel pair without atomics.  The gradients' scatter-adds (the backward of the gathers) are torch's
    atomics: the gradient bits may vary from run to run."""
    if means2d.dim() != 3:
        raise ValueError(f"means2d must have shape (C, N, 2), got {tuple(means2d.shape)}")
    Cn, N = means2d.shape[0], means2d.shape[1]
    width, height = int(image_width), int(image_height)
    if width < 0 or height < 0:
        raise ValueError(f"image_width and image_height must not be negative, got {image_width!r}, {image_height!r}")
    _check(means2d, (Cn, N, 2), "means2d")
    _check(conics, (Cn, N, 3), "conics")
    _check(opacities, (Cn, N), "opacities")
    if colors.dim() != 3 or colors.shape[-1] < 1:
        raise ValueError(f"colors must have shape (C, N, D) with D >= 1, got {tuple(colors.shape)}")
    D = colors.shape[-1]
    _check(colors, (Cn, N, D), "colors")
    if gaussian_ids.dim() != 1:
        raise ValueError(f"gaussian_ids must have shape (M,), got {tuple(gaussian_ids.shape)}")
    M = gaussian_ids.shape[0]
    _check(gaussian_ids, (M,), "gaussian_ids", torch.int64)
    _check(pixel_ids, (M,), "pixel_ids", torch.int64)
    _check(camera_ids, (M,), "camera_ids", torch.int64)
    dev = means2d.device
    P = Cn * height * width
    if M == 0 or P == 0:  # (nothing to sum: zeros, on the inputs' graph)
        zero = (means2d.sum() + conics.sum() + opacities.sum() + colors.sum()) * 0.0
        return (torch.zeros(Cn, height, width, D, device=dev) + zero, torch.zeros(Cn, height, width, 1, device=dev) + zero)
    with torch.no_grad():
        key = camera_ids * (height * width) + pixel_ids
        counts = torch.bincount(key, minlength=P)[:P].contiguous()  # a pixel's segment has ITS OWN length, whatever the order
        starts = (torch.cumsum(counts, 0) - counts).contiguous()
        px = (pixel_ids % width).to(torch.float32) + 0.5
        py = torch.div(pixel_ids, width, rounding_mode="floor").to(torch.float32) + 0.5
        row = camera_ids * N + gaussian_ids
    # (index_select, not t[row]: its backward is one index_add, where advanced indexing sorts the M indices first)
    xy = means2d.reshape(Cn * N, 2).index_select(0, row)
    con = conics.reshape(Cn * N, 3).index_select(0, row)
    dx, dy = xy[:, 0] - px, xy[:, 1] - py
    sigma = 0.5 * (con[:, 0] * dx * dx + con[:, 2] * dy * dy) + con[:, 1] * dx * dy
    alpha = torch.clamp(opacities.reshape(Cn * N).index_select(0, row) * torch.exp(-sigma), max=0.999)
    feat = colors.reshape(Cn * N, D).index_select(0, row)
    renders, alphas = _Accumulate.apply(alpha, feat, starts, counts, P)
    return renders.reshape(Cn, height, width, D), alphas.reshape(Cn, height, width, 1)


# ----------------------------------------------------------------------------------------------------------------
def world_to_cam(means: Tensor, covars: Tensor, viewmats: Tensor) -> Tuple[Tensor, Tensor]:
    """gsplat ``world_to_cam``: ``means`` [N,3], ``covars`` [N,3,3], ``viewmats`` [C,4,4] -> ``(means_c [C,N,3],
    covars_c [C,N,3,3])``, ``means_c = R means + t``, ``covars_c = R covars R^T``.  Plain torch, any device."""
    R = viewmats[:, :3, :3]
    t = viewmats[:, :3, 3]
    means_c = torch.einsum("cij,nj->cni", R, means) + t[:, None, :]
    covars_c = torch.einsum("cij,njk,clk->cnil", R, covars, R)
    return means_c, covars_c


def persp_proj(means: Tensor, covars: Tensor, Ks: Tensor, width: int, height: int) -> Tuple[Tensor, Tensor]:
    """gsplat ``persp_proj``: camera-space ``means`` [C,N,3] and ``covars`` [C,N,3,3], ``Ks`` [C,3,3] -> ``(means2d
    [C,N,2], covars2d [C,N,2,2])`` with the 1.3 tan-fov clamp on the Jacobian's x / z and y / z (``means2d`` is not
    clamped) and WITHOUT eps2d on the diagonal.  Plain torch, any device."""
    tx, ty, tz = means.unbind(-1)
    fx, fy = Ks[:, 0, 0, None], Ks[:, 1, 1, None]
    cx, cy = Ks[:, 0, 2, None], Ks[:, 1, 2, None]
    lim_x = 1.3 * (0.5 * width / fx)
    lim_y = 1.3 * (0.5 * height / fy)
    rz = 1.0 / tz
    cxz = tz * torch.minimum(lim_x, torch.maximum(-lim_x, tx * rz))
    cyz = tz * torch.minimum(lim_y, torch.maximum(-lim_y, ty * rz))
    zero = torch.zeros_like(tz)
    J = torch.stack([fx * rz, zero, -fx * cxz * rz * rz, zero, fy * rz, -fy * cyz * rz * rz], dim=-1).reshape(means.shape[:-1] + (2, 3))
    covars2d = J @ covars @ J.transpose(-1, -2)
    means2d = torch.stack([fx * tx * rz + cx, fy * ty * rz + cy], dim=-1)
    return means2d, covars2d


def proj(means: Tensor, covars: Tensor, Ks: Tensor, width: int, height: int,
         camera_model: str = "pinhole") -> Tuple[Tensor, Tensor]:
    """gsplat ``proj`` (1.4): camera-space ``means`` [C,N,3] and ``covars`` [C,N,3,3], ``Ks`` [C,3,3] -> ``(means2d
    [C,N,2], covars2d [C,N,2,2])`` under ``camera_model``.  "pinhole" is ``persp_proj``.  "ortho": ``means2d = (fx x +
    cx, fy y + cy)`` and ``covars2d = J covars J^T`` with the constant ``J = [[fx, 0, 0], [0, fy, 0]]`` (``width`` and
    ``height`` play no part), WITHOUT eps2d on the diagonal.  Plain torch, any device."""
    if not _is_ortho(camera_model):
        return persp_proj(means, covars, Ks, width, height)
    fx, fy = Ks[:, 0, 0, None], Ks[:, 1, 1, None]
    cx, cy = Ks[:, 0, 2, None], Ks[:, 1, 2, None]
    tx, ty, _tz = means.unbind(-1)
    f = torch.stack([fx, fy], dim=-1)  # [C,1,2]: J scales rows / columns 0 and 1, and drops the third
    covars2d = covars[..., :2, :2] * f[..., :, None] * f[..., None, :]
    means2d = torch.stack([fx * tx + cx, fy * ty + cy], dim=-1)
    return means2d, covars2d
