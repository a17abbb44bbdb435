"""Drop-in shim: ``from gsplat import rasterization`` (reference edgegaussians/models/edge_gs.py:8)
resolves to the MI355X-native implementation, so the reference's model class runs unchanged.

The reference imports ``rasterization`` alone; ``spherical_harmonics`` is there for the other callers of gsplat, whose
``rasterization(..., sh_degree=L)`` calls it serves as well.  ``rasterization`` takes gsplat's defaults, ``packed=True``
included (only the visible (camera, Gaussian) pairs are kept; ``info["camera_ids"]`` / ``info["gaussian_ids"]`` name
them), and ``sparse_grad=True`` on top of it; ``viewmats`` that require grad receive their ``[C, 4, 4]`` gradient (pose
optimisation); ``tile_size`` may be 8, 16 or 32 (16 is the reference's); ``camera_model`` (gsplat 1.4's argument, appended
last) may be "pinhole" or "ortho" (the orthographic camera of CAD views); ``covars`` [N, 3, 3] (a keyword in front of
``channel_chunk``; restated from memory of gsplat >= 1.3) gives the full 3-D covariances in place of ``quats`` +
``scales``, which may then be None: only the upper triangle is read, ``covars.grad`` is [N, 3, 3] with zeros below the diagonal (sparse with
``sparse_grad``), and every other argument -- ``packed``, the render modes, ``sh_degree``, both camera models, the
``viewmats`` gradient -- works with it.

The stage-by-stage API -- ``fully_fused_projection`` (from ``quats`` + ``scales`` or from ``covars``),
``quat_scale_to_covar_preci``, ``isect_tiles``, ``isect_offset_encode``, ``rasterize_to_pixels``,
``rasterize_to_indices_in_range``, ``accumulate``, ``world_to_cam``, ``persp_proj``, ``proj`` -- is
edgegaussians_amd/functional.py: the same kernels, for callers that change something between the stages
(``packed=False`` only; see that module for the unsupported corners); ``fully_fused_projection`` and ``proj`` take
``camera_model`` as well.

The densification strategies of gsplat's training scripts -- ``Strategy``, ``DefaultStrategy``, ``MCMCStrategy`` (also
``gsplat.strategy``, with ``gsplat.strategy.ops``) and ``compute_relocation`` (also ``gsplat.relocation``) -- are
edgegaussians_amd/strategy and edgegaussians_amd/relocation.py; the optimizers are ``gsplat.optimizers``."""
from edgegaussians_amd.rasterizer import rasterization  # noqa: F401
from edgegaussians_amd.sh import spherical_harmonics  # noqa: F401
from edgegaussians_amd.functional import (  # noqa: F401
    accumulate, fully_fused_projection, isect_offset_encode, isect_tiles, persp_proj, proj, quat_scale_to_covar_preci,
    rasterize_to_indices_in_range, rasterize_to_pixels, world_to_cam)
from edgegaussians_amd.relocation import compute_relocation  # noqa: F401
from edgegaussians_amd.strategy import DefaultStrategy, MCMCStrategy, Strategy  # noqa: F401

__version__ = "1.0.0+edgegaussians_amd"
__all__ = ["rasterization", "spherical_harmonics", "fully_fused_projection", "quat_scale_to_covar_preci", "isect_tiles",
           "isect_offset_encode", "rasterize_to_pixels", "rasterize_to_indices_in_range", "accumulate", "world_to_cam",
           "persp_proj", "proj", "Strategy", "DefaultStrategy", "MCMCStrategy", "compute_relocation"]
