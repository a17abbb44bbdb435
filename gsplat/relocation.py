"""``gsplat.relocation``: re-export of edgegaussians_amd/relocation.py."""
from edgegaussians_amd.relocation import compute_relocation  # noqa: F401

__all__ = ["compute_relocation"]
