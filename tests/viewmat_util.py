"""References for the camera-pose gradient of the projection (csrc/viewmat_grad.hip), shared by
tests/test_viewmat_grad_host.py and tests/test_gpu_viewmat_grad.py.

The reference is oracle.ref_torch.project in float64 with autograd with respect to viewmat[c], one output's N(0,1)
cotangent at a time, on the scenes of tests.util.PROJ_CASES (the cotangents are those of tests.util.projection_reference).
Next to the gradient itself the tests need the contribution of every pair, G[c, n, 3, 4]: one Gaussian per `project`
call, once per process.  For the first n rows the reference is G[:, :n].sum(1), its scale S = |G|[:, :n].sum(1), and the
bound is entrywise, |got - ref64| <= TAU * S, with exact zeros where S == 0: a bound relative to the largest of the
twelve entries would hide a wrong small entry.

TAU is set on the references alone: the fp32 `project` against the float64 one, worst |g32 - g64| / S (measured by the
host test and recorded with tests.util.record_cpu), times 8 -- the device chains hardware rcp / rsqrt (1 ulp each)
through about ten roundings per term and sums in another tree than torch's CPU reduction -- rounded up to a power of
two.  The host test keeps the fp32 oracle within an eighth of the bound.

Two constants come out of that rule, because the oracle's own ratio depends on the number of pairs.  One entry of one
pair, v_t[i] mean[j] + sum_k vW[3i+k] M[j][k], is a sum of terms that cancel: its rounding error is ~1e-7 of the TERMS,
up to 2.8e-6 of |G| itself.  Over the thousands of pairs of a whole scene those errors are independent and S grows
faster than their sum -- 6.4e-8 at worst on the four scenes (TAU) -- while on the first 1 / 63 / 257 / 1000 rows the
oracle measures 2.8e-6 / 4.4e-7 / 1.3e-7 / 8.7e-8.  TAU_SMALL, from the worst of those, is the bound for any number of
pairs; TAU holds on the whole scenes."""
import numpy as np
import torch

from tests import util as U

W, H = U.PROJ_SIZE
CASES = ("defaults", "defaults_comp", "fov_cam1", "three_cams_eps1")
RAGGED_CASE = "three_cams_eps1"
RAGGED_N = (1, 63, 257, 1000)     # one lane, less than a wave, one workgroup + one lane, a ragged last workgroup
FP32_WORST = 6.4e-8               # worst |g32 - g64| / S of the fp32 oracle on the whole scenes (the host test measures it)
TAU = 2.0 ** -20                  # the smallest power of two >= 8 * FP32_WORST (5.1e-7 <= 9.5e-7)
FP32_WORST_SMALL = 2.84e-6        # the same on the first n rows, n in RAGGED_N (the worst: the conic cotangent at n = 1)
TAU_SMALL = 2.0 ** -15            # the smallest power of two >= 8 * FP32_WORST_SMALL (2.3e-5 <= 3.1e-5)


def tau_for(case, n):
    """the bound of a run on the first n rows of `case`: TAU on the whole scene, TAU_SMALL on a part of it"""
    N = U.projection_scene(U.PROJ_CASES[case]["kind"], U.PROJ_CASES[case]["scene_cam"])[0].shape[0]
    return TAU if n is None or n == N else TAU_SMALL


def case_sizes(case):
    """the n the tests use on `case`: every row, and the ragged sizes on RAGGED_CASE"""
    N = U.projection_scene(U.PROJ_CASES[case]["kind"], U.PROJ_CASES[case]["scene_cam"])[0].shape[0]
    return ((N,) + RAGGED_N) if case == RAGGED_CASE else (N,)


def contributions(means, quats, scales, viewmats, Ks, width, height, args, cots, todo):
    """({cotangent: float64 G [C, N, 3, 4]}, vis bool [C, N], largest |bottom-row entry| autograd returned): the gradient
    of sum(out[n] * cots[name][c, n]) with respect to viewmats[c], one Gaussian per oracle.ref_torch.project call in
    float64, for the pairs of `todo` (bool [C, N]) that the call keeps; zero elsewhere (a culled pair contributes
    exactly nothing)."""
    from oracle import ref_torch as O
    C, N = todo.shape
    G = {k: torch.zeros(C, N, 3, 4, dtype=torch.float64) for k in cots}
    vis = torch.zeros(C, N, dtype=torch.bool)
    bottom = 0.0
    p = [t.detach().double() for t in (means, quats, scales)]
    cots = {k: v.detach().double() for k, v in cots.items()}
    for c in range(C):
        for n in np.nonzero(np.asarray(todo[c]))[0].tolist():
            vm = viewmats[c].detach().double().clone().requires_grad_(True)
            out = O.project(p[0][n:n + 1], p[1][n:n + 1], p[2][n:n + 1], vm, Ks[c], width, height, args["near_plane"],
                            args["far_plane"], args["eps2d"], args["radius_clip"])
            if int(out[0][0]) <= 0:
                continue
            vis[c, n] = True
            for k in cots:
                y = out[1 + U.PROJ_OUTPUTS.index(k)]
                g = torch.autograd.grad(y, vm, cots[k][c, n].reshape(y.shape), retain_graph=True, allow_unused=True)[0]
                if g is not None:
                    G[k][c, n] = g[:3]
                    bottom = max(bottom, float(g[3].abs().max()))
    return G, vis, bottom


def pair_contributions(case):
    """dict(G, vis, bottom) of `contributions` on a tests.util.PROJ_CASES entry with the cotangents of
    tests.util.projection_reference, computed once per process."""
    key = ("viewmat_pairs", case)
    if key not in U._proj_cache:
        ref = U.projection_reference(case)
        G, vis, bottom = contributions(ref["means"], ref["quats"], ref["scales"], ref["viewmats"], ref["Ks"], W, H,
                                       ref["spec"]["args"], ref["cots"], ref["vis"])
        U._proj_cache[key] = dict(G=G, vis=vis, bottom=bottom)
    return U._proj_cache[key]


def whole_call_gradient(case, cot, n, dtype, drop=None):
    """([C, 4, 4] `dtype` gradient of oracle.ref_torch.project on the first n rows with respect to the viewmats, one
    call per camera, all rows at once; radii [C, n]).  The cotangent rows of the pairs in `drop` are zeroed."""
    from oracle import ref_torch as O
    ref = U.projection_reference(case)
    a = ref["spec"]["args"]
    C = ref["vis"].shape[0]
    p = [ref[k][:n].to(dtype) for k in ("means", "quats", "scales")]
    grads, radii = [], []
    for c in range(C):
        vm = ref["viewmats"][c].to(dtype).clone().requires_grad_(True)
        out = O.project(p[0], p[1], p[2], vm, ref["Ks"][c], W, H, a["near_plane"], a["far_plane"], a["eps2d"], a["radius_clip"])
        y = out[1 + U.PROJ_OUTPUTS.index(cot)]
        ct = ref["cots"][cot][c, :n].to(dtype).reshape(y.shape)
        if drop is not None:
            ct = ct * (~torch.as_tensor(drop[c])).to(dtype).reshape([n] + [1] * (y.dim() - 1))
        g = torch.autograd.grad(y, vm, ct, allow_unused=True)[0]
        grads.append(g if g is not None else torch.zeros(4, 4, dtype=dtype))
        radii.append(out[0])
    return torch.stack(grads), torch.stack(radii)


def reference(case, cot, n=None, drop=None, mode="antialiased"):
    """(ref64 [C, 3, 4], S [C, 3, 4]) for the first n rows, without the pairs of `drop` (bool [C, n]).  In classic mode
    the compensation is no output of the projection: its cotangent reaches nothing, the reference is zero."""
    pc = pair_contributions(case)
    C, N = pc["vis"].shape
    n = N if n is None else n
    if cot == "compensations" and mode == "classic":
        z = torch.zeros(C, 3, 4, dtype=torch.float64)
        return z, z.clone()
    g = pc["G"][cot][:, :n]
    if drop is not None:
        g = g * (~torch.as_tensor(drop))[:, :, None, None]
    return g.sum(1), g.abs().sum(1)


def bound_ratio(got, ref64, S):
    """(largest |got - ref64| / S over the entries with S > 0, number of entries with S == 0 where `got` is not exactly
    zero); `got` [C, 3, 4] or [C, 4, 4] (the bottom row is the caller's to check)."""
    got = torch.as_tensor(got).detach().cpu().double()[:, :3]
    live = S > 0
    ratio = float(((got - ref64).abs()[live] / S[live]).max()) if live.any() else 0.0
    return ratio, int((got[~live] != 0).sum())


def check(got, ref64, S, name, tau):
    """The comparison every device test makes: [C, 4, 4] fp32, bottom row exactly zero, exact zeros where S == 0, every
    other entry within tau * S.  Returns the worst ratio |got - ref64| / S."""
    got = torch.as_tensor(got).detach().cpu()
    assert tuple(got.shape) == (ref64.shape[0], 4, 4) and got.dtype == torch.float32, (got.shape, got.dtype)
    assert not got[:, 3].any(), f"{name}: the bottom row is not exactly zero"
    ratio, nonzero = bound_ratio(got, ref64, S)
    assert nonzero == 0, f"{name}: {nonzero} entries are not exactly zero where no pair contributes"
    assert ratio <= tau, f"{name}: |got - ref64| / S = {ratio:.3e} exceeds {tau:.3e}"
    return ratio
