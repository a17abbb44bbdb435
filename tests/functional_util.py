"""References and scene discipline of the functional-API tests (tests/test_functional_host.py on the CPU,
tests/test_gpu_functional.py on the device): the projection from covariances restated from oracle.ref_torch.project,
its per-case float64 reference with per-row kappa and the integer-borderline set, and the float64 reference of
quat_scale_to_covar_preci.  Every reference is computed once per process and never modified."""
import numpy as np
import torch

from tests import util as U

W, H = U.PROJ_SIZE
COVAR_CASES = ("defaults", "defaults_comp", "fov_cam1", "args_eps0.05", "args_eps1", "three_cams_eps1")
COVAR_GRADS = ("means", "covars")
TRIU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def triu6(mats):
    """[..., 3, 3] -> [..., 6]: the upper triangle (00, 01, 02, 11, 12, 22)"""
    return torch.stack([mats[..., i, j] for i, j in TRIU], dim=-1)


def sym_from6(c6):
    """[..., 6] -> [..., 3, 3]: the six numbers placed into the symmetric matrix (an off-diagonal one twice)"""
    c00, c01, c02, c11, c12, c22 = c6.unbind(-1)
    return torch.stack([c00, c01, c02, c01, c11, c12, c02, c12, c22], dim=-1).reshape(c6.shape[:-1] + (3, 3))


def _internals(means, covars6, viewmat, K, width, height, near_plane, far_plane, eps2d):
    """oracle.ref_torch.project up to the determinant, with the world covariance given as its six numbers"""
    from oracle import ref_torch as O
    dt = means.dtype
    Rv, tv = viewmat[:3, :3].to(dt), viewmat[:3, 3].to(dt)
    fx, fy, cx, cy = K[0, 0].to(dt), K[1, 1].to(dt), K[0, 2].to(dt), K[1, 2].to(dt)
    mean_c = means @ Rv.T + tv
    x, y, z = mean_c.unbind(-1)
    in_z = (z >= near_plane) & (z <= far_plane)
    zs = torch.where(in_z, z, torch.ones_like(z))
    covar_c = Rv @ sym_from6(covars6) @ Rv.T
    lim_x = O.FOV_CLAMP * (0.5 * width / fx)
    lim_y = O.FOV_CLAMP * (0.5 * height / fy)
    rz = 1.0 / zs
    rz2 = rz * rz
    tx = zs * torch.minimum(lim_x, torch.maximum(-lim_x, x * rz))
    ty = zs * torch.minimum(lim_y, torch.maximum(-lim_y, y * rz))
    zero = torch.zeros_like(rz)
    J = torch.stack([fx * rz, zero, -fx * tx * rz2, zero, fy * rz, -fy * ty * rz2], dim=-1).reshape(-1, 2, 3)
    cov2d = J @ covar_c @ J.transpose(-1, -2)
    mean2d = torch.stack([fx * x * rz + cx, fy * y * rz + cy], dim=-1)
    c00, c01, c10, c11 = cov2d[:, 0, 0], cov2d[:, 0, 1], cov2d[:, 1, 0], cov2d[:, 1, 1]
    det0 = c00 * c11 - c01 * c10
    b00, b11 = c00 + eps2d, c11 + eps2d
    det1 = b00 * b11 - c01 * c10
    return dict(z=z, in_z=in_z, mean2d=mean2d, cov2d=cov2d, c01=c01, det0=det0, b00=b00, b11=b11, det1=det1)


def ref_project_covars(means, covars6, viewmat, K, width, height, near_plane=0.01, far_plane=1e10, eps2d=0.3,
                       radius_clip=0.0):
    """oracle.ref_torch.project restated with the covariance given as six numbers [N, 6] instead of quats + scales:
    (radii i32 [N], means2d [N, 2], depths [N], conics [N, 3], compensations [N]); autograd supplies the VJP."""
    from oracle import ref_torch as O
    q = _internals(means, covars6, viewmat, K, width, height, near_plane, far_plane, eps2d)
    det_ok = q["det1"] > 0
    det1s = torch.where(det_ok, q["det1"], torch.ones_like(q["det1"]))
    comp = O._Compensation.apply(q["det0"] / det1s)
    inv = 1.0 / det1s
    conic = torch.stack([q["b11"] * inv, -q["c01"] * inv, q["b00"] * inv], dim=-1)
    mean2d = q["mean2d"]
    with torch.no_grad():
        bh = 0.5 * (q["b00"] + q["b11"])
        v1 = bh + torch.sqrt(torch.clamp(bh * bh - q["det1"], min=O.RADIUS_DET_FLOOR))
        radius = torch.ceil(O.RADIUS_SIGMAS * torch.sqrt(v1))
        ok = q["in_z"] & det_ok & (radius > radius_clip)
        ok &= ~((mean2d[:, 0] + radius <= 0) | (mean2d[:, 0] - radius >= width)
                | (mean2d[:, 1] + radius <= 0) | (mean2d[:, 1] - radius >= height))
        radii = torch.where(ok, radius, torch.zeros_like(radius)).to(torch.int32)
    z = q["z"]
    return (radii, torch.where(ok[:, None], mean2d, torch.zeros_like(mean2d)), torch.where(ok, z, torch.zeros_like(z)),
            torch.where(ok[:, None], conic, torch.zeros_like(conic)), torch.where(ok, comp, torch.zeros_like(comp)))


def covars_borderline(means, covars6, viewmat, K, width, height, args, rel=U.REL_GAUSS):
    """bool [N], float64: the rows whose near / far, det1, radius-ceil, radius_clip or off-screen decision lies within
    `rel` (relative to the sizes of the quantities compared) of its threshold."""
    from oracle import ref_torch as O
    with torch.no_grad():
        q = _internals(means.double(), covars6.double(), viewmat, K, width, height, args["near_plane"], args["far_plane"],
                       args["eps2d"])
        z = q["z"].numpy()
        planes = (np.abs(z - args["near_plane"]) <= rel * args["near_plane"]) | (np.abs(z - args["far_plane"]) <= rel * args["far_plane"])
        b00, b11, det1 = q["b00"].numpy(), q["b11"].numpy(), q["det1"].numpy()
        bad = np.abs(det1) <= rel * np.abs(b00 * b11)
        bh = 0.5 * (b00 + b11)
        raw = O.RADIUS_SIGMAS * np.sqrt(bh + np.sqrt(np.maximum(bh * bh - det1, O.RADIUS_DET_FLOOR)))
        bad |= np.abs(raw - np.rint(raw)) <= rel * np.maximum(raw, 1.0)
        radius = np.ceil(raw)
        bad |= np.abs(radius - args["radius_clip"]) <= rel * max(args["radius_clip"], 1.0)
        u, v = q["mean2d"][:, 0].numpy(), q["mean2d"][:, 1].numpy()
        for val, lim in ((u + radius, 0.0), (u - radius, float(width)), (v + radius, 0.0), (v - radius, float(height))):
            bad |= np.abs(val - lim) <= rel * np.maximum(np.abs(u) + np.abs(v) + radius, 1.0)
    # (a row the planes cull outright has no other decision to make)
    return planes | (bad & q["in_z"].numpy())


def ref_covars_vjps(means, covars6, viewmats, Ks, args, cots, dtype=torch.float64):
    """ref_project_covars + autograd for the cameras of one call, one output's cotangent at a time (tests.util's
    ref_project_vjps for this form).  Returns (outs, grads: {output name: {"means" | "covars": [N, k]}})."""
    p = [t.detach().to(dtype).clone().requires_grad_(True) for t in (means, covars6)]
    per_cam = [ref_project_covars(p[0], p[1], viewmats[c], Ks[c], W, H, args["near_plane"], args["far_plane"],
                                  args["eps2d"], args["radius_clip"]) for c in range(viewmats.shape[0])]
    outs = {"radii": torch.stack([o[0] for o in per_cam])}
    for i, name in enumerate(U.PROJ_OUTPUTS):
        outs[name] = torch.stack([o[1 + i] for o in per_cam])
    grads = {}
    for name, cot in cots.items():
        y = outs[name]
        g = torch.autograd.grad(y, p, cot.to(dtype).reshape(y.shape), retain_graph=True, allow_unused=True)
        grads[name] = {k: (gi if gi is not None else torch.zeros_like(pi)).detach() for k, gi, pi in zip(COVAR_GRADS, g, p)}
    return {k: v.detach() for k, v in outs.items()}, grads


_cache = {}


def covars_inputs(case):
    """(spec, means fp32 [N,3], covars fp32 [N,6] = fp32(triu(float64 covariance)), quats, scales, viewmats, Ks, group)"""
    from oracle import ref_torch as O
    spec = U.PROJ_CASES[case]
    vms_all, Ks_all = U.projection_cameras()
    cams = list(spec["cams"])
    means, quats, scales, group = U.projection_scene(spec["kind"], spec["scene_cam"])
    covars = triu6(O.quat_scale_to_covar(quats.double(), scales.double())).float().contiguous()
    return spec, means, covars, quats, scales, vms_all[cams].contiguous(), Ks_all[cams].contiguous(), group


def covars_reference(case):
    """tests.util.projection_reference for the covariance form: fp32 inputs, N(0,1) cotangents [C, N, k] of the case's
    outputs, float64 outputs and per-cotangent gradients (summed over the cameras), kappa per (cotangent, gradient)
    from four one-ulp perturbations of means and covars, the per-camera borderline sets, the compensation rows."""
    key = ("ref", case)
    if key in _cache:
        return _cache[key]
    spec, means, covars, quats, scales, vms, Ks, group = covars_inputs(case)
    N, C = means.shape[0], vms.shape[0]
    gen = torch.Generator().manual_seed(11)
    widths = dict(means2d=2, depths=1, conics=3, compensations=1)
    cots = {name: torch.randn(C, N, widths[name], generator=gen) for name in U.PROJ_OUTPUTS}
    cots = {name: cots[name] for name in spec["cots"]}
    outs, grads = ref_covars_vjps(means, covars, vms, Ks, spec["args"], cots)
    pert = [ref_covars_vjps(*U.ulp_perturbed((means, covars), gen), vms, Ks, spec["args"], cots)[1] for _ in range(4)]
    kappa = {c: {g: U.row_kappa(grads[c][g], [p[c][g] for p in pert]) for g in COVAR_GRADS} for c in cots}
    border = np.stack([covars_borderline(means, covars, vms[c], Ks[c], W, H, spec["args"]) for c in range(C)])
    vis = outs["radii"].numpy() > 0
    comp = outs["compensations"].numpy()
    comp_ok = 1.0 - comp * comp >= U.COMP_MIN_ONE_MINUS_SQ
    comp_rows = vis.any(axis=0) & (comp_ok | ~vis).all(axis=0)
    ref = dict(case=case, spec=spec, means=means, covars=covars, quats=quats, scales=scales, group=group, viewmats=vms, Ks=Ks,
               cots=cots, outs=outs, grads=grads, kappa=kappa, border=border, vis=vis,
               comp_rows=comp_rows)
    _cache[key] = ref
    return ref


# ---------------------------------------------------------------------------------------------------
QS_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
QS_BASES = (0.003, 0.12)
QS_FORMS = ((True, True), (True, False), (False, True))   # (compute_covar, compute_preci) that compute something


def qs_inputs(n, base):
    """un-normalised quaternions randn * U(0.5, 1.5), scales U(0.7, 1.4) * base * a permutation of (1, 2.2, 4.5)"""
    gen = torch.Generator().manual_seed(1000 + n + int(base * 1e4))
    quats = torch.randn(n, 4, generator=gen, dtype=torch.float64) * (0.5 + torch.rand(n, 1, generator=gen, dtype=torch.float64))
    size = base * (0.7 + 0.7 * torch.rand(n, 1, generator=gen, dtype=torch.float64))
    perm = torch.argsort(torch.rand(n, 3, generator=gen), dim=1)
    scales = size * torch.tensor(U.SCALE_RATIOS, dtype=torch.float64)[perm]
    return quats.float().contiguous(), scales.float().contiguous(), gen


def ref_quat_scale_to_covar_preci(quats, scales, triu, dtype=torch.float64):
    """(covars, precis) from oracle.ref_torch.quat_to_rotmat: R diag(s^2) R^T and R diag(1 / s^2) R^T; with `triu` the
    upper triangle selected from the full matrix (so autograd gives the convention the kernels follow)."""
    from oracle import ref_torch as O
    R = O.quat_to_rotmat(quats.to(dtype))
    s = scales.to(dtype)
    M = R * s[..., None, :]
    L = R * (1.0 / s)[..., None, :]
    covars, precis = M @ M.transpose(-1, -2), L @ L.transpose(-1, -2)
    return (triu6(covars), triu6(precis)) if triu else (covars, precis)


def qs_reference(n, base, triu):
    """float64 outputs, the gradients of one output's N(0,1) cotangent at a time, kappa per (output, gradient) and per
    forward row from four one-ulp perturbations of quats and scales."""
    key = ("qs", n, base, triu)
    if key in _cache:
        return _cache[key]
    quats, scales, gen = qs_inputs(n, base)
    shape = (n, 6) if triu else (n, 3, 3)
    cots = {"covars": torch.randn(shape, generator=gen), "precis": torch.randn(shape, generator=gen)}

    def run(q, s):
        p = [q.double().clone().requires_grad_(True), s.double().clone().requires_grad_(True)]
        outs = dict(zip(("covars", "precis"), ref_quat_scale_to_covar_preci(p[0], p[1], triu)))
        grads = {k: dict(zip(("quats", "scales"), (g.detach() for g in torch.autograd.grad(outs[k], p, cots[k].double(), retain_graph=True))))
                 for k in outs}
        return {k: v.detach() for k, v in outs.items()}, grads

    outs, grads = run(quats, scales)
    pert = [run(*U.ulp_perturbed((quats, scales), gen)) for _ in range(4)]
    kappa = {k: {g: U.row_kappa(grads[k][g], [p[1][k][g] for p in pert]) for g in ("quats", "scales")} for k in outs}
    kappa_fwd = {k: U.row_kappa(outs[k].reshape(n, -1), [p[0][k].reshape(n, -1) for p in pert]) for k in outs}
    ref = dict(quats=quats, scales=scales, cots=cots, outs=outs, grads=grads, kappa=kappa, kappa_fwd=kappa_fwd)
    _cache[key] = ref
    return ref
