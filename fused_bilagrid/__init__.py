"""Drop-in for the ``fused_bilagrid`` package: ``from fused_bilagrid import BilateralGrid, slice, total_variation_loss``
in a trainer resolves to edgegaussians_amd.bilagrid (csrc/bilagrid.hip).  ``color_correct``, the evaluation-time torch
routine of the original, is ABSENT: it has no kernel in it and is out of scope here, so gsplat's import line
``from fused_bilagrid import BilateralGrid, color_correct, slice, total_variation_loss`` has to drop that one name
(or take it from ``lib_bilagrid``).  ``slice`` returns ``{"rgb": ...}`` only: the per-pixel affine matrices are never
built."""
from edgegaussians_amd.bilagrid import BilateralGrid, slice, total_variation_loss

__all__ = ["BilateralGrid", "slice", "total_variation_loss"]
