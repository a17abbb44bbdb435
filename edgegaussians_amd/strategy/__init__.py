"""gsplat's densification strategies (``gsplat.strategy``): ``DefaultStrategy`` (Kerbl et al.'s clone / split / prune /
opacity-reset schedule) and ``MCMCStrategy`` (Kheradmand et al.: relocate dead Gaussians, grow to a cap, perturb
positions), over the operations of ``edgegaussians_amd.strategy.ops``.

    strategy = DefaultStrategy()
    strategy.check_sanity(params, optimizers)
    state = strategy.initialize_state(scene_scale=1.0)
    for step in range(max_steps):
        render, alpha, info = rasterization(...)
        strategy.step_pre_backward(params, optimizers, state, step, info)
        loss.backward()
        strategy.step_post_backward(params, optimizers, state, step, info, packed=...)
        for opt in optimizers.values(): opt.step(); opt.zero_grad()

``params`` is a dict or ``ParameterDict`` of leaf ``nn.Parameter`` s: ``means [N,3]``, ``scales [N,3]`` (logs), ``quats
[N,4]`` (unnormalised), ``opacities [N]`` (logits) and any further ``[N, ...]`` keys; ``optimizers`` a dict with the same
keys, each optimizer with one param group of one parameter.

What runs on every step is one launch each: the running statistics of ``DefaultStrategy`` (``eg_strategy_update`` /
``eg_strategy_update_packed``) and the position noise of ``MCMCStrategy`` (``eg_inject_noise``).  Not provided: gsplat's
``distributed`` handling, its visualisation hooks, and ``verbose`` beyond one printed line per refinement.  gsplat is
not available here: the schedules and formulas are restated from gsplat 1.4 from memory, not pinned against its build.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, Tuple, Union

import torch
from torch import Tensor

from . import ops  # noqa: F401
from .ops import (_update_grad_stats, duplicate, inject_noise_to_position, relocate, remove, reset_opa, sample_add,
                  split)

__all__ = ["Strategy", "DefaultStrategy", "MCMCStrategy", "ops"]

Params = Union[Dict[str, torch.nn.Parameter], torch.nn.ParameterDict]


@dataclass
class Strategy:
    """Base class: the sanity check of ``params`` / ``optimizers`` and the two no-op hooks."""

    def check_sanity(self, params: Params, optimizers: Dict[str, torch.optim.Optimizer]) -> None:
        for key in ("means", "scales", "quats", "opacities"):
            assert key in params, f"{key} is required in params but missing"
        trainable = set(name for name, p in params.items() if p.requires_grad)
        assert trainable == set(optimizers.keys()), (
            f"trainable parameters and optimizers must have the same keys, got {trainable} and {set(optimizers.keys())}")
        for name, optimizer in optimizers.items():
            assert len(optimizer.param_groups) == 1, (
                f"the optimizer of {name} must have exactly one param group, got {len(optimizer.param_groups)}")
            assert len(optimizer.param_groups[0]["params"]) == 1, (
                f"the param group of {name} must hold exactly one parameter")
            assert optimizer.param_groups[0]["params"][0] is params[name], (
                f"the optimizer of {name} must hold params[{name!r}]")

    def step_pre_backward(self, *args, **kwargs) -> None:
        pass

    def step_post_backward(self, *args, **kwargs) -> None:
        pass


@dataclass
class DefaultStrategy(Strategy):
    """gsplat's ``DefaultStrategy``.  Every ``refine_every`` steps after ``refine_start_iter``: Gaussians whose mean
    image-plane gradient exceeds ``grow_grad2d`` are duplicated (3-D scale <= ``grow_scale3d * scene_scale``) or split
    (larger; also those whose screen radius exceeds ``grow_scale2d`` while ``step < refine_scale2d_stop_iter``), then those
    with opacity below ``prune_opa`` (and, after the first reset, too large in 3-D or on screen) are removed; every
    ``reset_every`` steps the opacities are clamped to ``2 prune_opa``.  ``absgrad`` reads ``info[key].absgrad``
    (``rasterization(absgrad=True)``); a ``grow_grad2d`` of 0.0008 suits it."""

    prune_opa: float = 0.005
    grow_grad2d: float = 0.0002
    grow_scale3d: float = 0.01
    grow_scale2d: float = 0.05
    prune_scale3d: float = 0.1
    prune_scale2d: float = 0.15
    refine_scale2d_stop_iter: int = 0
    refine_start_iter: int = 500
    refine_stop_iter: int = 15_000
    reset_every: int = 3000
    refine_every: int = 100
    pause_refine_after_reset: int = 0
    absgrad: bool = False
    revised_opacity: bool = False
    verbose: bool = False
    key_for_gradient: str = "means2d"

    def initialize_state(self, scene_scale: float = 1.0) -> Dict[str, Any]:
        """The running state; the tensors are created on the first ``step_post_backward`` (``N`` is not known here)."""
        state = {"grad2d": None, "count": None, "scene_scale": scene_scale}
        if self.refine_scale2d_stop_iter > 0:
            state["radii"] = None
        return state

    def step_pre_backward(self, params: Params, optimizers, state: Dict[str, Any], step: int, info: Dict[str, Any]) -> None:
        assert self.key_for_gradient in info, "The 2D means of the Gaussians is required but missing."
        info[self.key_for_gradient].retain_grad()

    def step_post_backward(self, params: Params, optimizers, state: Dict[str, Any], step: int, info: Dict[str, Any],
                           packed: bool = False) -> None:
        if step >= self.refine_stop_iter:
            return
        self._update_state(params, state, info, packed=packed)
        if (step > self.refine_start_iter and step % self.refine_every == 0
                and step % self.reset_every >= self.pause_refine_after_reset):
            n_dupli, n_split = self._grow_gs(params, optimizers, state, step)
            if self.verbose:
                print(f"Step {step}: {n_dupli} GSs duplicated, {n_split} GSs split. "
                      f"Now having {len(params['means'])} GSs.")
            n_prune = self._prune_gs(params, optimizers, state, step)
            if self.verbose:
                print(f"Step {step}: {n_prune} GSs pruned. Now having {len(params['means'])} GSs.")
            state["grad2d"].zero_()
            state["count"].zero_()
            if self.refine_scale2d_stop_iter > 0:
                state["radii"].zero_()
        if step % self.reset_every == 0:
            reset_opa(params=params, optimizers=optimizers, state=state, value=self.prune_opa * 2.0)

    def _update_state(self, params: Params, state: Dict[str, Any], info: Dict[str, Any], packed: bool = False) -> None:
        for key in ("width", "height", "n_cameras", "radii", "gaussian_ids", self.key_for_gradient):
            assert key in info, f"{key} is required but missing."
        grads = info[self.key_for_gradient].absgrad if self.absgrad else info[self.key_for_gradient].grad
        n_gaussian = len(next(iter(params.values())))
        device = grads.device
        if state["grad2d"] is None:
            state["grad2d"] = torch.zeros(n_gaussian, device=device)
        if state["count"] is None:
            state["count"] = torch.zeros(n_gaussian, device=device)
        if self.refine_scale2d_stop_iter > 0 and state["radii"] is None:
            state["radii"] = torch.zeros(n_gaussian, device=device)
        _update_grad_stats(state["grad2d"], state["count"], state.get("radii"), grads, info["radii"], info["width"],
                           info["height"], info["n_cameras"], gaussian_ids=info["gaussian_ids"] if packed else None,
                           camera_ids=info.get("camera_ids") if packed else None)

    @torch.no_grad()
    def _grow_gs(self, params: Params, optimizers, state: Dict[str, Any], step: int) -> Tuple[int, int]:
        grads = state["grad2d"] / state["count"].clamp_min(1)
        device = grads.device
        is_grad_high = grads > self.grow_grad2d
        is_small = torch.exp(params["scales"]).max(dim=-1).values <= self.grow_scale3d * state["scene_scale"]
        is_dupli = is_grad_high & is_small
        n_dupli = int(is_dupli.sum().item())
        is_split = is_grad_high & ~is_small
        if step < self.refine_scale2d_stop_iter:
            is_split |= state["radii"] > self.grow_scale2d
        n_split = int(is_split.sum().item())
        if n_dupli > 0:
            duplicate(params=params, optimizers=optimizers, state=state, mask=is_dupli)
        # the duplicated rows are not split
        is_split = torch.cat([is_split, torch.zeros(n_dupli, dtype=torch.bool, device=device)])
        if n_split > 0:
            split(params=params, optimizers=optimizers, state=state, mask=is_split, revised_opacity=self.revised_opacity)
        return n_dupli, n_split

    @torch.no_grad()
    def _prune_gs(self, params: Params, optimizers, state: Dict[str, Any], step: int) -> int:
        is_prune = torch.sigmoid(params["opacities"].flatten()) < self.prune_opa
        if step > self.reset_every:
            is_too_big = torch.exp(params["scales"]).max(dim=-1).values > self.prune_scale3d * state["scene_scale"]
            if step < self.refine_scale2d_stop_iter:
                is_too_big |= state["radii"] > self.prune_scale2d
            is_prune = is_prune | is_too_big
        n_prune = int(is_prune.sum().item())
        if n_prune > 0:
            remove(params=params, optimizers=optimizers, state=state, mask=is_prune)
        return n_prune


@dataclass
class MCMCStrategy(Strategy):
    """gsplat's ``MCMCStrategy``.  Every ``refine_every`` steps between ``refine_start_iter`` and ``refine_stop_iter``: the
    Gaussians with opacity <= ``min_opacity`` are relocated onto alive ones, then 5 % more are added up to ``cap_max``;
    on every step the positions receive noise scaled by ``lr * noise_lr`` (``lr`` is the means' learning rate)."""

    cap_max: int = 1_000_000
    noise_lr: float = 5e5
    refine_start_iter: int = 500
    refine_stop_iter: int = 25_000
    refine_every: int = 100
    min_opacity: float = 0.005
    verbose: bool = False

    def initialize_state(self) -> Dict[str, Any]:
        n_max = 51
        binoms = torch.zeros((n_max, n_max))
        for n in range(n_max):
            for k in range(n + 1):
                binoms[n, k] = math.comb(n, k)
        return {"binoms": binoms}

    def step_post_backward(self, params: Params, optimizers, state: Dict[str, Any], step: int, info: Dict[str, Any],
                           lr: float) -> None:
        binoms = state["binoms"] = state["binoms"].to(params["means"].device)
        if self.refine_start_iter < step < self.refine_stop_iter and step % self.refine_every == 0:
            n_relocated = self._relocate_gs(params, optimizers, binoms)
            if self.verbose:
                print(f"Step {step}: Relocated {n_relocated} GSs.")
            n_new = self._add_new_gs(params, optimizers, binoms)
            if self.verbose:
                print(f"Step {step}: Added {n_new} GSs. Now having {len(params['means'])} GSs.")
        inject_noise_to_position(params=params, optimizers=optimizers, state={}, scaler=lr * self.noise_lr)

    @torch.no_grad()
    def _relocate_gs(self, params: Params, optimizers, binoms: Tensor) -> int:
        dead_mask = torch.sigmoid(params["opacities"].flatten()) <= self.min_opacity
        n_dead = int(dead_mask.sum().item())
        if n_dead > 0:
            relocate(params=params, optimizers=optimizers, state={}, mask=dead_mask, binoms=binoms,
                     min_opacity=self.min_opacity)
        return n_dead

    @torch.no_grad()
    def _add_new_gs(self, params: Params, optimizers, binoms: Tensor) -> int:
        current = len(params["means"])
        n_new = max(0, min(self.cap_max, int(1.05 * current)) - current)
        if n_new > 0:
            sample_add(params=params, optimizers=optimizers, state={}, n=n_new, binoms=binoms,
                       min_opacity=self.min_opacity)
        return n_new
