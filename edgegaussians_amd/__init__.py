"""edgegaussians_amd -- MI355X-native edge-Gaussian rasterizer (the hot path of
kunalchelani/EdgeGaussians) behind the reference's own operator surface.

    from edgegaussians_amd import rasterization      # == the reference's gsplat.rasterization call
    from edgegaussians_amd import spherical_harmonics  # == gsplat.spherical_harmonics (degrees 0..4)
    from edgegaussians_amd import functional         # gsplat's stage-by-stage API (fully_fused_projection, isect_tiles, ...)
    from edgegaussians_amd import strategy           # gsplat.strategy: DefaultStrategy, MCMCStrategy and their ops
    from edgegaussians_amd.ssim import fused_ssim    # == fused_ssim.fused_ssim (the SSIM term of the 3DGS loss)
    from edgegaussians_amd import losses             # scalar image losses: projection_loss, photometric_loss, ...
    from edgegaussians_amd import bilagrid           # == fused_bilagrid: BilateralGrid, slice, total_variation_loss
    from edgegaussians_amd import EdgeTrainer        # fused per-view training step (train_gaussians.py:71-106)
"""
from .rasterizer import rasterization  # noqa: F401
from .sh import spherical_harmonics  # noqa: F401
from .trainer import EdgeTrainer, LRSchedule, train_steps_multi  # noqa: F401
from .train_loop import train, train_epoch  # noqa: F401
from . import edges  # noqa: F401  (parametric edges -> points -> metrics)
from . import functional  # noqa: F401  (gsplat's functional API over the same kernels)
from . import strategy  # noqa: F401  (gsplat's densification strategies: DefaultStrategy, MCMCStrategy, ops)
from . import ssim  # noqa: F401  (fused SSIM: ssim_map, fused_ssim -- the `fused_ssim` package's operation)
from . import losses  # noqa: F401  (scalar image losses on the device: weighted / masked L1, L1 + D-SSIM)
from . import bilagrid  # noqa: F401  (bilateral grid: fused slice + apply, TV loss -- the `fused_bilagrid` package's operations)

__all__ = ["rasterization", "spherical_harmonics", "EdgeTrainer", "LRSchedule", "train", "train_epoch", "train_steps_multi", "edges", "functional", "strategy", "ssim", "losses", "bilagrid"]
