"""gsplat's ``gsplat.relocation.compute_relocation``: the opacity and scale a Gaussian takes when the MCMC strategy
splits it into ``ratio`` copies (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", eq. 9).

One launch of ``eg_compute_relocation`` (csrc/strategy.hip), one lane per Gaussian.  gsplat is not available here: the
formula is restated from gsplat 1.4's kernel from memory and is not pinned against gsplat's own build.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor

from . import _lib
from .rasterizer import _check


@torch.no_grad()
def compute_relocation(opacities: Tensor, scales: Tensor, ratios: Tensor, binoms: Tensor) -> Tuple[Tensor, Tensor]:
    """``opacities [N]``, ``scales [N,3]`` (both activated, fp32), ``ratios [N]`` (any integer dtype; clamped to
    ``[1, n_max]`` and taken as int32), ``binoms [n_max, n_max]`` fp32 with ``binoms[n, k] = C(n, k)``.
    Returns ``(new_opacities [N], new_scales [N,3])``:

        r = clamp(ratio, 1, n_max);  x = 1 - (1 - o)^(1 / r)
        den = sum_{i=1..r} sum_{k=0..i-1} binoms[i-1, k] (-1)^k x^(k+1) / sqrt(k+1)
        new_opacity = x;  new_scales = (o / den) scales

    Device tensors only (ValueError for a CPU tensor, TypeError for a wrong dtype): there is no torch fallback.
    ``N == 0`` returns empty tensors without a launch."""
    if not isinstance(opacities, Tensor) or opacities.dim() != 1:
        raise ValueError("opacities must be a tensor of shape [N]")
    N = opacities.shape[0]
    _check(opacities, (N,), "opacities")
    _check(scales, (N, 3), "scales")
    if not isinstance(binoms, Tensor) or binoms.dim() != 2 or binoms.shape[0] != binoms.shape[1] or binoms.shape[0] < 1:
        raise ValueError("binoms must be a square table [n_max, n_max]")
    n_max = binoms.shape[0]
    _check(binoms, (n_max, n_max), "binoms")
    if not ratios.is_cuda:
        raise ValueError(f"ratios must be a device tensor (got {ratios.device}); edgegaussians_amd has no CPU path")
    if ratios.dtype.is_floating_point or ratios.dtype.is_complex or ratios.dtype == torch.bool:
        raise TypeError(f"ratios must be an integer tensor, got {ratios.dtype}")
    if tuple(ratios.shape) != (N,):
        raise ValueError(f"ratios must have shape {(N,)}, got {tuple(ratios.shape)}")
    new_opacities = torch.empty(N, dtype=torch.float32, device=opacities.device)
    new_scales = torch.empty(N, 3, dtype=torch.float32, device=opacities.device)
    if N == 0:
        return new_opacities, new_scales
    r = ratios.clamp(1, n_max).to(torch.int32).contiguous()
    o, s, b = opacities.contiguous(), scales.contiguous(), binoms.contiguous()
    _lib.call("eg_compute_relocation", _lib.ptr(o), _lib.ptr(s), _lib.ptr(r), _lib.ptr(b), N, n_max,
              _lib.ptr(new_opacities), _lib.ptr(new_scales), _lib.stream())
    return new_opacities, new_scales
