"""``gsplat.strategy``: re-exports of edgegaussians_amd/strategy (DefaultStrategy, MCMCStrategy and their ops)."""
from edgegaussians_amd.strategy import DefaultStrategy, MCMCStrategy, Strategy  # noqa: F401
from . import ops  # noqa: F401

__all__ = ["Strategy", "DefaultStrategy", "MCMCStrategy", "ops"]
