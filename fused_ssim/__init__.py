"""Drop-in for the ``fused_ssim`` package: ``from fused_ssim import fused_ssim`` in an unchanged trainer resolves to
edgegaussians_amd.ssim.fused_ssim (csrc/ssim.hip)."""
from edgegaussians_amd.ssim import fused_ssim

__all__ = ["fused_ssim"]
