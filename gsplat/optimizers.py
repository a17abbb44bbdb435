"""``from gsplat.optimizers import SelectiveAdam`` (gsplat >= 1.4): the MI355X-native class of edgegaussians_amd/optim.py.
``step(visibility)`` steps the rows a bool mask names, e.g. ``(info["radii"] > 0).any(0)`` of a ``packed=False`` call."""
from edgegaussians_amd.optim import SelectiveAdam  # noqa: F401

__all__ = ["SelectiveAdam"]
