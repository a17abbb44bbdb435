"""Drop-ins for the reference's and gsplat's optimizers: `edgegaussians_amd.optim.Adam` in place of `torch.optim.Adam`,
`SparseAdam` in place of `torch.optim.SparseAdam`, and gsplat's `SelectiveAdam`.

Adam.  The reference keeps FOUR single-tensor `torch.optim.Adam` instances (train_utils.py:50-60: means, scales, quats,
opacities; betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad) and steps them one after the other after every
backward (train_gaussians.py:104-106, and 116-118 / 128-130 for the regulariser iterations).  On this host a
`torch.optim.Adam.step()` costs ~0.11 ms of Python and dispatch per call -- 0.44 ms per training step, half of what the
whole drop-in protocol costs here -- for an update that takes the GPU 2 us.  This class keeps torch's interface and
STATE LAYOUT (`state[p] = {"step", "exp_avg", "exp_avg_sq"}`, `param_groups[i]["lr"]`), so the schedulers of
train_utils.py and the model's densification code, which edits `optimizer.state` and `param_groups[0]["params"]` in
place (edge_gs.py:384-402, 431-451), work unchanged; `step()` is one native launch per tensor (`eg_adam_tensor`, the
arithmetic of `eg_adam_multi`).

Not supported by Adam (the reference uses none of them): weight decay, amsgrad, maximize, closures that re-evaluate the
loss, sparse gradients (SparseAdam below steps those), non-fp32 or non-contiguous parameters, step pre / post hooks --
each raises instead of falling back.

Rounding: the native kernel forms 1 / (sqrt(v_hat) + eps) with the hardware square root and reciprocal (1 ulp each),
torch's with IEEE sqrt and a division: the two agree to ~2e-7 relative per step (tests: 2e-6 over 31 steps incl. the
reference's in-place state surgery), NOT bit for bit.

SparseAdam steps the `torch.sparse_coo_tensor` gradients that `rasterization(packed=True, sparse_grad=True)` hands
`means`, `quats` and `scales`: only the rows a gradient names move, and the moments of every other row do not decay
(torch/optim/_functional.py: sparse_adam).  The same state layout as torch's class (`"step"` is an int there), so
`state_dict()` / `load_state_dict()` go both ways.  A coalesced gradient (one camera) is ONE native launch
(`eg_adam_sparse_rows`) and nothing else on the device; an uncoalesced one (several cameras, or two backward calls) has
its int64 indices sorted first -- a stable `torch.sort`, plumbing -- and the launch adds the values of a row in the order
of the values tensor before it steps the row once: no float atomics, the same bits every run.  The sort is shared: the
gradients of one `step()` whose indices are ONE storage are sorted once, and those that are copies of each other --
autograd's AccumulateGrad clones the three gradients of one backward, indices included, so that is how they arrive --
go through one batched sort call per index count, never one per tensor.  No host read-back.  A row that occurs
thousands of times is summed by one thread (csrc/adam_sparse.hip): slow, correct.

SelectiveAdam (gsplat >= 1.4's optimizer for packed=False callers) steps the rows of dense gradients that a bool mask
names, without bias correction: `eg_adam_masked_rows`.  gsplat is not at hand here: the update is restated from its
kernel from memory, like the rasterizer's arithmetic it is not pinned against gsplat's own build.

Both refuse what they do not do (listed at each class) instead of falling back to torch arithmetic.
"""
from __future__ import annotations

import torch

from . import _lib


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if weight_decay != 0 or amsgrad:
            raise NotImplementedError("edgegaussians_amd.optim.Adam: weight_decay / amsgrad are not implemented "
                                      "(the reference uses neither: train_utils.py:50-60)")
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    # (no torch.no_grad(): nothing below is recorded by autograd -- the update runs on raw device pointers)
    def step(self, closure=None, zero_grad: bool = False):
        """One Adam step on every parameter that has a gradient.  `zero_grad=True` clears the gradients in the same
        launch (what `opt.step(); opt.zero_grad(set_to_none=False)` does in two)."""
        if closure is not None:
            raise NotImplementedError("edgegaussians_amd.optim.Adam.step: closures are not supported")
        _lib.load()  # fails loudly without the HIP library: there is no torch fallback
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse or p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_cuda:
                    raise NotImplementedError("edgegaussians_amd.optim.Adam: dense fp32 device tensors only")
                if not (p.is_contiguous() and g.is_contiguous()):
                    raise NotImplementedError("edgegaussians_amd.optim.Adam: contiguous parameters and gradients only")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)  # torch's layout: a CPU scalar tensor
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                m, v = st["exp_avg"], st["exp_avg_sq"]
                if m.shape != p.shape or v.shape != p.shape or not (m.is_contiguous() and v.is_contiguous()):
                    raise RuntimeError("edgegaussians_amd.optim.Adam: optimizer state does not match its parameter")
                _lib.call("eg_adam_tensor", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                          float(group["lr"]), float(b1), float(b2), float(group["eps"]), int(st["step"]),
                          1 if zero_grad else 0, _lib.stream())
        return None

    # torch.optim.Optimizer wraps `step` of every subclass in a profiler range + pre/post-hook dispatch unless it is
    # marked as hooked already: ~25 us of host time per call, four calls per training step.  This class has no step hooks.
    step.hooked = True

    def register_step_pre_hook(self, hook):
        raise NotImplementedError("edgegaussians_amd.optim.Adam: step hooks are not dispatched (step() skips torch's "
                                  "hook wrapper); use torch.optim.Adam if you need them")

    def register_step_post_hook(self, hook):
        raise NotImplementedError("edgegaussians_amd.optim.Adam: step hooks are not dispatched (step() skips torch's "
                                  "hook wrapper); use torch.optim.Adam if you need them")

    def zero_grad(self, set_to_none: bool = True):
        """torch's semantics (gradients dropped, or zeroed in place with set_to_none=False) without its profiler range
        and foreach grouping: ~3 us instead of ~20 per call."""
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.requires_grad_(False)
                    p.grad.zero_()


class _RowAdam(torch.optim.Optimizer):
    """What SparseAdam and SelectiveAdam share with Adam above: no step hooks (step() skips torch's wrapper) and a
    zero_grad without the profiler range.  A sparse gradient is emptied by `zero_()` (nnz 0), as torch's zero_grad does."""

    def register_step_pre_hook(self, hook):
        raise NotImplementedError(f"edgegaussians_amd.optim.{type(self).__name__}: step hooks are not dispatched (step() "
                                  "skips torch's hook wrapper); use torch's class if you need them")

    def register_step_post_hook(self, hook):
        raise NotImplementedError(f"edgegaussians_amd.optim.{type(self).__name__}: step hooks are not dispatched (step() "
                                  "skips torch's hook wrapper); use torch's class if you need them")

    def zero_grad(self, set_to_none: bool = True):
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_()
                    p.grad.requires_grad_(False)
                    p.grad.zero_()

    def _moments(self, p, st):
        m, v = st["exp_avg"], st["exp_avg_sq"]
        if not (m.shape == p.shape and v.shape == p.shape and m.dtype == p.dtype and v.dtype == p.dtype
                and m.device == p.device and v.device == p.device and m.is_contiguous() and v.is_contiguous()):
            raise RuntimeError(f"edgegaussians_amd.optim.{type(self).__name__}: optimizer state does not match its parameter")
        return m, v


def _stable_sort(rows: torch.Tensor):
    """[k, nnz] int64 index lists -> (sorted, permutation), each row sorted on its own; equal indices keep their order."""
    return torch.sort(rows, dim=1, stable=True)


class SparseAdam(_RowAdam):
    """torch.optim.SparseAdam on fp32 device parameters with gradients of sparse_dim() == 1 and any dense dims.
    Raises: a dense gradient RuntimeError (torch's wording); maximize, a tensor lr, a closure, step hooks, other dtypes
    or devices, non-contiguous parameters, sparse_dim() != 1 NotImplementedError; a state that does not match its
    parameter RuntimeError.  Nothing is stepped when any parameter of the call is refused."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, maximize=False):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("edgegaussians_amd.optim.SparseAdam: a tensor lr is not supported")
        if maximize:
            raise NotImplementedError("edgegaussians_amd.optim.SparseAdam: maximize is not implemented")
        if not 0.0 < lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, maximize=maximize))
        for group in self.param_groups:
            for p in group["params"]:
                if p.is_sparse or p.is_complex():
                    raise ValueError("SparseAdam requires dense, real parameter tensors")

    def _checked(self):
        """[(group, p, grad)] of the parameters that have a gradient; raises before anything is stepped."""
        name = "edgegaussians_amd.optim.SparseAdam"
        work = []
        for group in self.param_groups:
            if group.get("maximize", False) or isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError(f"{name}: maximize / a tensor lr are not supported")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not g.is_sparse:
                    raise RuntimeError("SparseAdam does not support dense gradients, please consider Adam instead")
                if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_cuda or not g.is_cuda:
                    raise NotImplementedError(f"{name}: fp32 device tensors only")
                if g.sparse_dim() != 1:
                    raise NotImplementedError(f"{name}: gradients with sparse_dim() == 1 only (one row index per value row)")
                if not p.is_contiguous():
                    raise NotImplementedError(f"{name}: contiguous parameters only")
                if len(self.state[p]) != 0:
                    self._moments(p, self.state[p])
                work.append((group, p, g))
        return work

    @staticmethod
    def _sorted_indices(grads):
        """{id(grad): (sorted indices [nnz], permutation [nnz] or None)} for the gradients that have entries.  Coalesced:
        the gradient's own indices, no sort.  The others: one sort per distinct index storage, and the distinct
        storages of one length share one batched call."""
        out, key_of, by_storage, by_len = {}, {}, {}, {}
        for g in grads:
            nnz = g._nnz()
            if nnz == 0:
                continue
            idx = g._indices()  # [1, nnz]: its data pointer is the index list's
            if not idx.is_contiguous():
                idx = idx.contiguous()
            if g.is_coalesced():
                out[id(g)] = (idx, None)
                continue
            key_of[id(g)] = key = (idx.data_ptr(), nnz)
            if key not in by_storage:
                by_storage[key] = idx
                by_len.setdefault(nnz, []).append(key)
        done = {}
        for keys in by_len.values():
            rows = by_storage[keys[0]] if len(keys) == 1 else torch.cat([by_storage[k] for k in keys])
            srt, perm = _stable_sort(rows)
            for i, k in enumerate(keys):
                done[k] = (srt[i], perm[i])
        out.update({i: done[k] for i, k in key_of.items()})
        return out

    def step(self, closure=None):
        """One SparseAdam step on every parameter that has a gradient.  `step` advances also for a gradient without
        entries; nothing else happens then."""
        if closure is not None:
            raise NotImplementedError("edgegaussians_amd.optim.SparseAdam.step: closures are not supported")
        _lib.load()  # fails loudly without the HIP library: there is no torch fallback
        work = self._checked()
        plan = self._sorted_indices([g for _, _, g in work])
        for group, p, g in work:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = 0  # torch.optim.SparseAdam's layout: a Python int
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            if id(g) not in plan:
                continue
            m, v = st["exp_avg"], st["exp_avg_sq"]  # (checked above, or just made)
            srt, perm = plan[id(g)]
            values = g._values()
            if not values.is_contiguous():
                values = values.contiguous()
            N = p.shape[0]
            b1, b2 = group["betas"]
            _lib.call("eg_adam_sparse_rows", p.data_ptr(), m.data_ptr(), v.data_ptr(), values.data_ptr(), srt.data_ptr(),
                      None if perm is None else perm.data_ptr(), g._nnz(), N, p.numel() // N if N else 1,
                      float(group["lr"]), float(b1), float(b2), float(group["eps"]), int(st["step"]), _lib.stream())
        return None

    step.hooked = True


class SelectiveAdam(_RowAdam):
    """gsplat's SelectiveAdam: `step(visibility)` with a bool device tensor [N] (e.g. `(info["radii"] > 0).any(0)`) steps
    the rows -- M = numel / N components each -- where it is true:

        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr m / (sqrt(v) + eps)

    and leaves p, m and v of every other row bit for bit.  No bias correction: `state["step"]` is created as the float
    tensor 0.0 and never advanced.  One parameter per group, dense fp32 device gradients.  (Restated from gsplat's
    kernel from memory: gsplat is not at hand, this is not pinned against its build.)"""

    def __init__(self, params, eps, betas, lr=1e-3):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("edgegaussians_amd.optim.SelectiveAdam: a tensor lr is not supported")
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    def step(self, visibility, closure=None):
        name = "edgegaussians_amd.optim.SelectiveAdam"
        if closure is not None:
            raise NotImplementedError(f"{name}.step: closures are not supported")
        _lib.load()  # fails loudly without the HIP library: there is no torch fallback
        if not (isinstance(visibility, torch.Tensor) and visibility.dtype == torch.bool and visibility.is_cuda
                and visibility.dim() == 1 and visibility.is_contiguous()):
            raise NotImplementedError(f"{name}: visibility is a contiguous bool device tensor [N]")
        N = visibility.numel()
        work = []
        for group in self.param_groups:
            if len(group["params"]) != 1:
                raise ValueError(f"{name}: one parameter per group")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError(f"{name}: a tensor lr is not supported")
            p = group["params"][0]
            g = p.grad
            if g is None:
                continue
            if g.is_sparse or p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_cuda or not g.is_cuda:
                raise NotImplementedError(f"{name}: dense fp32 device tensors only")
            if not (p.is_contiguous() and g.is_contiguous()):
                raise NotImplementedError(f"{name}: contiguous parameters and gradients only")
            if p.numel() == 0 and N == 0:
                continue
            if N == 0 or p.numel() % N != 0 or p.numel() == 0:
                raise ValueError(f"{name}: {p.numel()} elements are not rows of a visibility of {N}")
            if len(self.state[p]) != 0:
                self._moments(p, self.state[p])
            work.append((group, p, g))
        for group, p, g in work:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = self._moments(p, st)
            b1, b2 = group["betas"]
            _lib.call("eg_adam_masked_rows", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), visibility.data_ptr(),
                      N, p.numel() // N, float(group["lr"]), float(b1), float(b2), float(group["eps"]), _lib.stream())
        return None

    step.hooked = True
