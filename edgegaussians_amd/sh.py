"""Spherical-harmonics colours: gsplat 1.0.0's ``spherical_harmonics`` and the ``sh_degree`` branch of
``rasterization`` on the kernels of csrc/sh.hip (eg_sh_fwd / eg_sh_bwd: one lane per Gaussian, the cameras in a loop
inside it, coefficient rows through LDS, no atomics).  No CPU path, no torch fall-back."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from ._lib import call, ptr, stream

MAX_DEGREE = 4


def check_degree(degree, K: int) -> int:
    """gsplat asserts these; here they are ValueErrors."""
    if isinstance(degree, bool) or not isinstance(degree, int) or not 0 <= degree <= MAX_DEGREE:
        raise ValueError(f"sh_degree must be an int in 0..{MAX_DEGREE}, got {degree!r}")
    if (degree + 1) ** 2 > K:
        raise ValueError(f"sh_degree {degree} needs {(degree + 1) ** 2} coefficient rows, coeffs has K = {K}")
    return degree


class _SH(torch.autograd.Function):
    """colors [C, N, 3] of `coeffs` ([N, K, 3] shared by the cameras, or [C, N, K, 3]).  The directions are `dirs`
    [C, N, 3] (then `means` / `campos` are None and `dirs` receives a gradient) or means[n] - campos[c] (then `means`
    receives it, summed over the cameras; `campos` receives none).  `masks` [C, N] bool or None; `clamp`: + 0.5, clamp_min 0."""

    @staticmethod
    def forward(ctx, degree, dirs, means, campos, coeffs, masks, clamp):
        Cn, N = (dirs.shape[0], dirs.shape[1]) if dirs is not None else (campos.shape[0], means.shape[0])
        K = coeffs.shape[-2]
        per_cam = int(coeffs.dim() == 4)
        dirs_c, means_c, campos_c = (t.contiguous() if t is not None else None for t in (dirs, means, campos))
        coeffs_c = coeffs.contiguous()
        masks_c = masks.contiguous() if masks is not None else None
        colors = torch.empty(Cn, N, 3, device=coeffs.device)
        call("eg_sh_fwd", degree, K, Cn, N, ptr(dirs_c), ptr(means_c), ptr(campos_c), ptr(coeffs_c), per_cam, ptr(masks_c),
             int(clamp), ptr(colors), stream())
        ctx.save_for_backward(*[t for t in (dirs_c, means_c, campos_c, coeffs_c, masks_c) if t is not None])
        ctx.cfg = (degree, K, Cn, N, per_cam, int(clamp), dirs is not None, masks is not None)
        return colors

    @staticmethod
    def backward(ctx, v_colors):
        degree, K, Cn, N, per_cam, clamp, has_dirs, has_masks = ctx.cfg
        saved = list(ctx.saved_tensors)
        dirs = saved.pop(0) if has_dirs else None
        means, campos = (None, None) if has_dirs else (saved.pop(0), saved.pop(0))
        coeffs = saved.pop(0)
        masks = saved.pop(0) if has_masks else None
        v_coeffs = torch.empty_like(coeffs)  # (written in full by the kernel, zeros included)
        v_dirs = torch.empty_like(dirs) if has_dirs and ctx.needs_input_grad[1] else None
        v_means = torch.empty_like(means) if not has_dirs and ctx.needs_input_grad[2] else None
        v_colors = v_colors.contiguous()
        call("eg_sh_bwd", degree, K, Cn, N, ptr(dirs), ptr(means), ptr(campos), ptr(coeffs), per_cam, ptr(masks), clamp,
             ptr(v_colors), ptr(v_coeffs), ptr(v_dirs), ptr(v_means), stream())
        return None, v_dirs, v_means, None, v_coeffs if ctx.needs_input_grad[4] else None, None, None


def _device_f32(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor (got {t.device}); edgegaussians_amd has no CPU path")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be torch.float32, got {t.dtype}")


def spherical_harmonics(degrees_to_use: int, dirs: Tensor, coeffs: Tensor, masks: Optional[Tensor] = None) -> Tensor:
    """gsplat 1.0.0 ``spherical_harmonics``: ``dirs`` [..., 3] (any length: normalised in the kernel), ``coeffs``
    [..., K, 3] with ``(degrees_to_use + 1) ** 2 <= K``, ``masks`` [...] bool or None.  Returns [..., 3]: the plain sum
    over the basis (no ``+ 0.5``, no clamp -- those belong to ``rasterization``), 0 where masked, with gradients to
    ``dirs`` and ``coeffs`` (rows above the degree's and masked entries get zeros)."""
    if dirs.dim() < 1 or dirs.shape[-1] != 3:
        raise ValueError(f"dirs must be [..., 3], got {tuple(dirs.shape)}")
    lead = tuple(dirs.shape[:-1])
    if coeffs.dim() != len(lead) + 2 or tuple(coeffs.shape[:-2]) != lead or coeffs.shape[-1] != 3:
        raise ValueError(f"coeffs must be {lead + ('K', 3)}, got {tuple(coeffs.shape)}")
    check_degree(degrees_to_use, coeffs.shape[-2])
    _device_f32(dirs, "dirs")
    _device_f32(coeffs, "coeffs")
    if masks is not None:
        if tuple(masks.shape) != lead or masks.dtype != torch.bool or not masks.is_cuda:
            raise ValueError(f"masks must be a bool device tensor of shape {lead}")
        masks = masks.reshape(1, -1)
    K = coeffs.shape[-2]
    out = _SH.apply(degrees_to_use, dirs.reshape(1, -1, 3), None, None, coeffs.reshape(-1, K, 3), masks, False)
    return out.reshape(lead + (3,))


def check_view_coeffs(coeffs: Tensor, sh_degree, Cn: int, N: int) -> int:
    """The checks of ``rasterization(colors=coeffs, sh_degree=L)``."""
    if coeffs.dim() not in (3, 4):
        raise ValueError(f"with sh_degree, colors must be [N, K, 3] or [C, N, K, 3], got {tuple(coeffs.shape)}")
    if coeffs.shape[-1] != 3:
        raise ValueError(f"with sh_degree, the last dimension of colors must be 3, got {tuple(coeffs.shape)}")
    want = (N,) if coeffs.dim() == 3 else (Cn, N)
    if tuple(coeffs.shape[:-2]) != want:
        raise ValueError(f"with sh_degree, colors must be {want + ('K', 3)}, got {tuple(coeffs.shape)}")
    _device_f32(coeffs, "colors")
    return check_degree(sh_degree, coeffs.shape[-2])


class _CameraDirs(torch.autograd.Function):
    """dirs [C, N, 3] = means[n] - campos[c], for the call whose `campos` needs a gradient.  Backward: `means` receives
    the sum over the cameras in camera order -- the order, hence the bits, of eg_sh_bwd's own sum in its means / campos
    form -- and `campos` minus the sum over the Gaussians."""

    @staticmethod
    def forward(ctx, means, campos):
        return means[None] - campos[:, None]

    @staticmethod
    def backward(ctx, v_dirs):
        v_means = v_dirs[0].clone()
        for c in range(1, v_dirs.shape[0]):
            v_means += v_dirs[c]
        return v_means, -v_dirs.sum(1)


def view_colors(means: Tensor, viewmats: Tensor, coeffs: Tensor, radii: Tensor, sh_degree: int) -> Tensor:
    """The colours ``rasterization`` composites with ``sh_degree``: [C, N, 3] =
    clamp_min(SH(means - campos[c]) + 0.5, 0) where radii [C, N] > 0, else 0.  campos = inverse(viewmats)[:, :3, 3],
    on the device without a host sync.  ``viewmats`` that require grad receive the directions' gradient through
    ``campos`` (the `dirs` form of `_SH` behind `_CameraDirs`); otherwise the kernels form the directions themselves."""
    pose_grad = torch.is_grad_enabled() and viewmats.requires_grad
    with torch.set_grad_enabled(pose_grad):
        campos = torch.linalg.inv_ex(viewmats)[0][:, :3, 3]  # (torch.linalg.inv without its host read of `info`)
    with torch.no_grad():
        masks = radii > 0
    if pose_grad:
        return _SH.apply(sh_degree, _CameraDirs.apply(means, campos), None, None, coeffs, masks, True)
    return _SH.apply(sh_degree, None, means, campos, coeffs, masks, True)
