"""``gsplat.strategy.ops``: re-exports of edgegaussians_amd/strategy/ops.py."""
from edgegaussians_amd.strategy.ops import (  # noqa: F401
    _multinomial_sample, _update_param_with_optimizer, duplicate, inject_noise_to_position, relocate, remove, reset_opa,
    sample_add, split)

__all__ = ["duplicate", "remove", "split", "reset_opa", "relocate", "sample_add", "inject_noise_to_position"]
