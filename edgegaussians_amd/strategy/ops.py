"""gsplat's ``gsplat.strategy.ops``: the operations that change the set of Gaussians, on a ``params`` dict (or
``ParameterDict``) of leaf ``nn.Parameter`` s and one single-parameter optimizer per key.

Every op mutates ``params``, ``optimizers`` and ``state`` in place.  ``duplicate``, ``remove``, ``split`` and ``reset_opa``
are torch indexing and run wherever the tensors live (CPU included).  ``relocate``, ``sample_add`` (through
``compute_relocation``), ``inject_noise_to_position`` and the running statistics of ``DefaultStrategy``
(``_update_grad_stats``) are HIP kernels (csrc/strategy.hip): device fp32 tensors only -- ``ValueError`` for a CPU
tensor, ``TypeError`` for a wrong dtype, never a torch fallback.

RNG calls, one per op, from the global generator of the tensors' device: ``split`` ``torch.randn(2, n_sel, 3)``;
``relocate`` and ``sample_add`` one ``torch.multinomial`` (above 2**24 categories, which ``torch.multinomial`` refuses:
one ``torch.rand`` searched in the cumulative sum); ``inject_noise_to_position`` ``torch.randn_like(means)``; the others none.

gsplat is not available here: the semantics are restated from gsplat 1.4 from memory, not pinned against its build.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Union

import torch
import torch.nn.functional as F
from torch import Tensor

from .. import _lib
from ..rasterizer import _check
from ..relocation import compute_relocation

Params = Union[Dict[str, torch.nn.Parameter], torch.nn.ParameterDict]
_MULTINOMIAL_MAX = 2 ** 24  # torch.multinomial's limit on the number of categories


def _multinomial_sample(weights: Tensor, n: int, replacement: bool = True) -> Tensor:
    """``n`` indices drawn with probabilities proportional to ``weights [K]``: ``torch.multinomial`` up to 2**24
    categories; above (``torch.multinomial`` raises there) ONE ``torch.rand(n)`` searched in the normalised cumulative
    sum -- with replacement only, and a different stream of draws than ``torch.multinomial`` would give."""
    K = weights.numel()
    if K <= _MULTINOMIAL_MAX:
        return torch.multinomial(weights, n, replacement=replacement)
    if not replacement:
        raise NotImplementedError("sampling without replacement above 2**24 categories is not implemented")
    cdf = torch.cumsum(weights.double(), 0)
    u = torch.rand(n, device=weights.device, dtype=torch.float64) * cdf[-1]
    return torch.searchsorted(cdf, u, right=True).clamp_(max=K - 1)


@torch.no_grad()
def _update_param_with_optimizer(param_fn: Callable[[str, Tensor], Tensor], optimizer_fn: Callable[[str, Tensor], Tensor],
                                 params: Params, optimizers: Dict[str, torch.optim.Optimizer],
                                 names: Optional[List[str]] = None) -> None:
    """For each name: ``params[name] = param_fn(name, old)`` (an ``nn.Parameter`` with the old ``requires_grad``); the
    optimizer of that name has its state for ``old`` taken out, every entry except ``"step"`` replaced by
    ``optimizer_fn(key, value)``, and put back under the new parameter, which becomes the only parameter of the param
    group.  An optimizer without state for the parameter keeps none.  Works with ``torch.optim.Adam`` and with
    ``edgegaussians_amd.optim.Adam`` / ``SparseAdam`` / ``SelectiveAdam``, which keep nothing keyed on the old tensor
    outside ``optimizer.state``."""
    if names is None:
        names = list(params.keys())
    for name in names:
        old = params[name]
        new = param_fn(name, old)
        params[name] = new
        if name not in optimizers:
            assert not old.requires_grad, f"parameter {name} requires grad and has no optimizer"
            continue
        optimizer = optimizers[name]
        for i in range(len(optimizer.param_groups)):
            st = optimizer.state.pop(old, None)
            if st:
                for key in list(st.keys()):
                    if key != "step":
                        st[key] = optimizer_fn(key, st[key])
                optimizer.state[new] = st
            optimizer.param_groups[i]["params"] = [new]


def _param(t: Tensor, like: Tensor) -> torch.nn.Parameter:
    return torch.nn.Parameter(t, requires_grad=like.requires_grad)


@torch.no_grad()
def duplicate(params: Params, optimizers, state: Dict, mask: Tensor) -> None:
    """Appends a copy of the rows where ``mask`` is true; zero optimizer moments for the new rows."""
    sel = torch.where(mask)[0]

    def param_fn(name, p):
        return _param(torch.cat([p, p[sel]]), p)

    def optimizer_fn(key, v):
        return torch.cat([v, torch.zeros((len(sel), *v.shape[1:]), dtype=v.dtype, device=v.device)])

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = torch.cat([v, v[sel]])


@torch.no_grad()
def remove(params: Params, optimizers, state: Dict, mask: Tensor) -> None:
    """Drops the rows where ``mask`` is true."""
    sel = torch.where(~mask)[0]

    def param_fn(name, p):
        return _param(p[sel], p)

    def optimizer_fn(key, v):
        return v[sel]

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = v[sel]


def _quat_to_rotmat(quats: Tensor) -> Tensor:
    w, x, y, z = torch.unbind(F.normalize(quats, dim=-1), dim=-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1)
    return R.reshape(quats.shape[:-1] + (3, 3))


@torch.no_grad()
def split(params: Params, optimizers, state: Dict, mask: Tensor, revised_opacity: bool = False) -> None:
    """Replaces every row where ``mask`` is true by two rows sampled from its Gaussian: means ``p + R (s * z)`` with
    ``z = torch.randn(2, n_sel, 3)`` (the only RNG call), scales ``log(s / 1.6)``, opacities copied or, with
    ``revised_opacity``, ``logit(1 - sqrt(1 - sigmoid(p)))``.  The kept rows come first, then copy 0 of every selected
    row, then copy 1."""
    device = mask.device
    sel = torch.where(mask)[0]
    rest = torch.where(~mask)[0]
    scales = torch.exp(params["scales"][sel])
    rotmats = _quat_to_rotmat(params["quats"][sel])
    z = torch.randn(2, len(sel), 3, device=device)
    samples = torch.einsum("nij,nj,bnj->bni", rotmats, scales, z.to(scales.dtype))  # [2, n_sel, 3]

    def param_fn(name, p):
        if name == "means":
            p_split = (p[sel] + samples).reshape(-1, 3)
        elif name == "scales":
            p_split = torch.log(scales / 1.6).repeat(2, 1)
        elif name == "opacities" and revised_opacity:
            new_opacities = 1.0 - torch.sqrt(1.0 - torch.sigmoid(p[sel]))
            p_split = torch.logit(new_opacities).repeat(2, *([1] * (p.dim() - 1)))
        else:
            p_split = p[sel].repeat(2, *([1] * (p.dim() - 1)))
        return _param(torch.cat([p[rest], p_split]), p)

    def optimizer_fn(key, v):
        return torch.cat([v[rest], torch.zeros((2 * len(sel), *v.shape[1:]), dtype=v.dtype, device=v.device)])

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = torch.cat([v[rest], v[sel].repeat(2, *([1] * (v.dim() - 1)))])


@torch.no_grad()
def reset_opa(params: Params, optimizers, state: Dict, value: float) -> None:
    """Clamps the opacities from above at ``value`` (a probability; the parameter holds logits) and zeroes the moments
    of the opacity optimizer."""

    def param_fn(name, p):
        if name != "opacities":
            raise ValueError(f"Unexpected parameter name: {name}")
        return _param(torch.clamp(p, max=torch.logit(torch.tensor(value)).item()), p)

    def optimizer_fn(key, v):
        return torch.zeros_like(v)

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers, names=["opacities"])


def _relocation_update(params: Params, sampled: Tensor, binoms: Tensor, min_opacity: float):
    """(logit of the new opacity, log of the new scale) of the rows ``sampled`` (duplicates carry equal values)."""
    opacities = torch.sigmoid(params["opacities"].detach())
    _check(opacities, (opacities.shape[0],), "opacities")
    new_opacities, new_scales = compute_relocation(
        opacities[sampled], torch.exp(params["scales"].detach())[sampled],
        torch.bincount(sampled, minlength=opacities.shape[0])[sampled] + 1, binoms)
    new_opacities = torch.clamp(new_opacities, max=1.0 - torch.finfo(torch.float32).eps, min=min_opacity)
    return torch.logit(new_opacities), torch.log(new_scales)


@torch.no_grad()
def relocate(params: Params, optimizers, state: Dict, mask: Tensor, binoms: Tensor, min_opacity: float = 0.005) -> None:
    """Moves the dead rows (``mask`` true) onto alive ones drawn with probability proportional to their opacity
    (one ``torch.multinomial`` with replacement, see ``_multinomial_sample`` above 2**24 alive rows): the drawn rows take
    ``compute_relocation``'s opacity (clamped to ``[min_opacity, 1 - eps]``) and scale for ``1 +`` the number of times they
    were drawn, then every key copies ``p[dead] = p[sampled]``; moments and state rows at ``sampled`` are zeroed."""
    dead = mask.nonzero(as_tuple=True)[0]
    alive = (~mask).nonzero(as_tuple=True)[0]
    n = len(dead)
    probs = torch.sigmoid(params["opacities"].detach())[alive].flatten()
    sampled = alive[_multinomial_sample(probs, n, replacement=True)]
    new_logits, new_log_scales = _relocation_update(params, sampled, binoms, min_opacity)

    def param_fn(name, p):
        if name == "opacities":
            p[sampled] = new_logits
        elif name == "scales":
            p[sampled] = new_log_scales
        p[dead] = p[sampled]
        return _param(p, p)

    def optimizer_fn(key, v):
        v[sampled] = 0
        return v

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            v[sampled] = 0


@torch.no_grad()
def sample_add(params: Params, optimizers, state: Dict, n: int, binoms: Tensor, min_opacity: float = 0.005) -> None:
    """Appends ``n`` copies of rows drawn with probability proportional to their opacity (the draw of ``relocate``, over
    all rows), after the drawn rows took ``compute_relocation``'s opacity and scale.  Moments at ``sampled`` are zeroed
    and ``n`` zero rows appended; state tensors get ``n`` zero rows."""
    probs = torch.sigmoid(params["opacities"].detach()).flatten()
    sampled = _multinomial_sample(probs, n, replacement=True)
    new_logits, new_log_scales = _relocation_update(params, sampled, binoms, min_opacity)

    def param_fn(name, p):
        if name == "opacities":
            p[sampled] = new_logits
        elif name == "scales":
            p[sampled] = new_log_scales
        return _param(torch.cat([p, p[sampled]]), p)

    def optimizer_fn(key, v):
        v[sampled] = 0
        return torch.cat([v, torch.zeros((len(sampled), *v.shape[1:]), dtype=v.dtype, device=v.device)])

    _update_param_with_optimizer(param_fn, optimizer_fn, params, optimizers)
    for k, v in state.items():
        if isinstance(v, Tensor):
            state[k] = torch.cat([v, torch.zeros((len(sampled), *v.shape[1:]), dtype=v.dtype, device=v.device)])


@torch.no_grad()
def inject_noise_to_position(params: Params, optimizers, state: Dict, scaler: float) -> None:
    """``means += Sigma (z * g * scaler)`` in one launch (``eg_inject_noise``): ``Sigma = R diag(exp(scales)^2) R^T`` of the
    normalised ``quats``, ``z = torch.randn_like(means)`` (the only RNG call),
    ``g = 1 / (1 + exp(-100 ((1 - sigmoid(opacities)) - 0.995)))``: only nearly transparent Gaussians move.  ``means`` is
    written in place; no optimizer state and no ``state`` entry is touched."""
    means = params["means"]
    if not isinstance(means, Tensor) or means.dim() != 2:
        raise ValueError("means must be a tensor of shape [N, 3]")
    N = means.shape[0]
    _check(means, (N, 3), "means")
    _check(params["quats"], (N, 4), "quats")
    _check(params["scales"], (N, 3), "scales")
    _check(params["opacities"], (N,), "opacities")
    if not means.is_contiguous():
        raise ValueError("means must be contiguous (it is updated in place)")
    noise = torch.randn_like(means)
    if N == 0:
        return
    q, s, o = (params[k].detach().contiguous() for k in ("quats", "scales", "opacities"))
    _lib.call("eg_inject_noise", _lib.ptr(means.detach()), _lib.ptr(q), _lib.ptr(s), _lib.ptr(o), _lib.ptr(noise),
              float(scaler), N, _lib.stream())


@torch.no_grad()
def _update_grad_stats(grad2d: Tensor, count: Tensor, radii_state: Optional[Tensor], grads: Tensor, radii: Tensor,
                       width: int, height: int, n_cameras: int, gaussian_ids: Optional[Tensor] = None,
                       camera_ids: Optional[Tensor] = None) -> None:
    """DefaultStrategy's running statistics in one launch.  For every visible pair (``radii > 0``) of Gaussian ``n``:
    ``grad2d[n] += |(gx width / 2 C, gy height / 2 C)|``, ``count[n] += 1``, ``radii_state[n] = max(radii_state[n],
    radii / max(width, height))`` (``radii_state`` may be None).  Dense (``gaussian_ids is None``): ``grads [C,N,2]``,
    ``radii [C,N]`` int32 (``eg_strategy_update``).  Packed: ``grads [nnz,2]``, ``radii [nnz]``, ``gaussian_ids`` /
    ``camera_ids [nnz]`` int64 IN ``camera * N + gaussian`` ORDER, as ``rasterization(packed=True)`` returns them -- not
    checked; another order gives wrong sums (``eg_strategy_update_packed``; the camera segments come from one
    ``torch.searchsorted`` on the device, no host read-back).  The cameras are added in ascending order by one lane per
    Gaussian: the same bits every run and in both forms."""
    if not isinstance(grad2d, Tensor) or grad2d.dim() != 1:
        raise ValueError("grad2d must be a tensor of shape [N]")
    N, C = grad2d.shape[0], int(n_cameras)
    _check(grad2d, (N,), "grad2d")
    _check(count, (N,), "count")
    if radii_state is not None:
        _check(radii_state, (N,), "radii")
    if not (grad2d.is_contiguous() and count.is_contiguous() and (radii_state is None or radii_state.is_contiguous())):
        raise ValueError("the state tensors must be contiguous (they are updated in place)")
    if C < 1 or width < 1 or height < 1:
        raise ValueError("n_cameras, width and height must be at least 1")
    if gaussian_ids is None:
        _check(grads, (C, N, 2), "grads")
        _check(radii, (C, N), "radii", torch.int32)
        if N == 0:
            return
        g, r = grads.contiguous(), radii.contiguous()
        _lib.call("eg_strategy_update", _lib.ptr(g), _lib.ptr(r), C, N, int(width), int(height), _lib.ptr(grad2d),
                  _lib.ptr(count), _lib.ptr(radii_state), _lib.stream())
        return
    nnz = gaussian_ids.shape[0]
    _check(grads, (nnz, 2), "grads")
    _check(radii, (nnz,), "radii", torch.int32)
    _check(gaussian_ids, (nnz,), "gaussian_ids", torch.int64)
    if N == 0 or nnz == 0:
        return
    indptr = None
    if C > 1:
        if camera_ids is None:
            raise ValueError("camera_ids is needed with more than one camera")
        _check(camera_ids, (nnz,), "camera_ids", torch.int64)
        indptr = torch.searchsorted(camera_ids.contiguous(), torch.arange(C + 1, device=camera_ids.device))
    g, r, ids = grads.contiguous(), radii.contiguous(), gaussian_ids.contiguous()
    _lib.call("eg_strategy_update_packed", _lib.ptr(g), _lib.ptr(r), _lib.ptr(ids), _lib.ptr(indptr), nnz, C, N,
              int(width), int(height), _lib.ptr(grad2d), _lib.ptr(count), _lib.ptr(radii_state), _lib.stream())
