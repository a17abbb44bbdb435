"""References and scene discipline of the orthographic-camera tests (tests/test_ortho_host.py on the CPU,
tests/test_gpu_ortho.py on the device).

`ref_project_ortho` is oracle.ref_torch.project restated with the orthographic mean and Jacobian (mean2d = (fx x + cx,
fy y + cy), J = [[fx, 0, 0], [0, fy, 0]], no fov clamp), in the quats + scales form and in the six-number covariance
form; it reuses the oracle's quat_scale_to_covar, _Compensation and RADIUS_* constants and keeps its cull order.
Autograd supplies every VJP, in float64.  A `viewmat` may be given per Gaussian ([N, 4, 4]): the gradient with respect
to it is then the contribution of every pair to the pose gradient, in one call.

The scenes are built in camera space on tests.util.PROJ_SIZE with the cameras of tests.util.projection_cameras() and
orthographic intrinsics fx / d, fy / d (d = the camera-space depth of the scene centre), so that footprints have the
size they have under the pinhole.  One scene of N_FULL rows serves every size: the groups are interleaved, the first
n rows are the scene of size n.  Every reference is computed once per process and never modified."""
import numpy as np
import torch

from tests import functional_util as F
from tests import util as U

W, H = U.PROJ_SIZE
SIZES = (1, 65, 257, 1000)
N_FULL = max(SIZES)
CAMS = {1: (0,), 3: (0, 1, 2)}
ARGS = {"defaults": U.PROJ_DEFAULTS, "eps0.05": U.off_default_args(0.05), "eps1": U.off_default_args(1.0)}
CASES = tuple((a, c) for a in ARGS for c in CAMS)
FORMS = {"quats": ("means", "quats", "scales"), "covars": ("means", "covars")}
CENTRE_DEPTH = 3.75
Z_RANGE = (3.35, 4.15)        # inside both plane settings (near 3.3 / far 4.2 off the defaults)
BASE_SCALE, TINY_SCALE, MEDIUM_SCALE = 0.03, 0.003, 0.012
SEED = 234                    # (a seed whose scene meets the conditions tests/test_ortho_host.py asserts)
# groups: ((ax_lo, ax_hi), (ay_lo, ay_hi)) in half-screens from the principal point, (z_lo, z_hi) or None, base scale,
# scale ratios.  With fx / d = 74 pixels per world unit the inside Gaussians have sigmas of 1.5 .. 14 pixels (radii up to
# 42), the tiny ones 0.15 .. 1.4 (radii 2 .. 6: visible at the defaults, removed to the last by radius_clip 6.5), the
# medium ones 0.6 .. 5.6: rows on which the compensation is far from 1 at eps2d = 1 and which the clip mostly keeps.
# (At eps2d = 0.05 the clip removes every Gaussian of the size of eps2d -- tests/test_gpu_projection.py,
# test_arguments_off_defaults -- so the compensation cotangent has few rows to be checked on there.)
GROUP_NAMES = ("inside", "left", "right", "top", "bottom", "outside", "near", "near_finite", "far_finite", "tiny", "medium")
_IN = (-0.9, 0.9)
_R = U.SCALE_RATIOS
GROUPS = (
    ((_IN, _IN), None, BASE_SCALE, _R),
    (((-1.04, -0.96), _IN), None, BASE_SCALE, _R), (((0.96, 1.04), _IN), None, BASE_SCALE, _R),   # straddling x = 0, x = W
    ((_IN, (-1.04, -0.96)), None, BASE_SCALE, _R), ((_IN, (0.96, 1.04)), None, BASE_SCALE, _R),   # straddling y = 0, y = H
    (((1.7, 2.0), (-1.9, 1.9)), None, BASE_SCALE, _R),                                            # fully outside
    ((_IN, _IN), (-0.5, 0.005), BASE_SCALE, _R),                                                  # behind near_plane = 0.01
    ((_IN, _IN), (3.0, 3.28), BASE_SCALE, _R),                                                    # in front of near_plane = 3.3
    ((_IN, _IN), (4.22, 4.5), BASE_SCALE, _R),                                                    # beyond far_plane = 4.2
    ((_IN, _IN), None, TINY_SCALE, _R),                                                           # radius_clip 6.5 removes them
    ((_IN, _IN), None, MEDIUM_SCALE, _R),
)
GROUP_PATTERN = (0, 10, 0, 9, 1, 2, 0, 10, 3, 4, 5, 0, 6, 7, 8, 9, 10)   # group of row i: GROUP_PATTERN[i % 17]


# ---------------------------------------------------------------------------------------------------
def _internals(means, covar_w, viewmat, K, near_plane, far_plane, eps2d):
    """oracle.ref_torch.project up to the determinant with the orthographic mean and J; covar_w [N, 3, 3]"""
    dt = means.dtype
    N = means.shape[0]
    vm = viewmat.to(dt)
    vm = vm if vm.dim() == 3 else vm.expand(N, 4, 4)
    Rv, tv = vm[:, :3, :3], vm[:, :3, 3]
    fx, fy, cx, cy = K[0, 0].to(dt), K[1, 1].to(dt), K[0, 2].to(dt), K[1, 2].to(dt)
    mean_c = (Rv @ means[..., None])[..., 0] + tv
    x, y, z = mean_c.unbind(-1)
    in_z = (z >= near_plane) & (z <= far_plane)
    covar_c = Rv @ covar_w @ Rv.transpose(-1, -2)
    zero = torch.zeros((), dtype=dt)
    J = torch.stack([fx, zero, zero, zero, fy, zero]).reshape(2, 3)
    cov2d = J @ covar_c @ J.T
    mean2d = torch.stack([fx * x + cx, fy * y + cy], dim=-1)
    c00, c01, c10, c11 = cov2d[:, 0, 0], cov2d[:, 0, 1], cov2d[:, 1, 0], cov2d[:, 1, 1]
    det0 = c00 * c11 - c01 * c10
    b00, b11 = c00 + eps2d, c11 + eps2d
    det1 = b00 * b11 - c01 * c10
    return dict(z=z, in_z=in_z, mean2d=mean2d, cov2d=cov2d, c01=c01, det0=det0, b00=b00, b11=b11, det1=det1)


def ref_project_ortho(means, quats, scales, viewmat, K, width, height, near_plane=0.01, far_plane=1e10, eps2d=0.3,
                      radius_clip=0.0, covars=None):
    """(radii i32 [N], means2d [N, 2], depths [N], conics [N, 3], compensations [N]) under camera_model="ortho", from
    `quats` [N, 4] + `scales` [N, 3] or, with `covars` [N, 6] (upper triangle; quats and scales None), from
    covariances.  `viewmat` [4, 4] or [N, 4, 4].  Culled rows: radius 0, zeros in every float output."""
    from oracle import ref_torch as O
    covar_w = F.sym_from6(covars) if covars is not None else O.quat_scale_to_covar(quats, scales)
    q = _internals(means, covar_w, viewmat, K, near_plane, far_plane, eps2d)
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


def ortho_borderline(means, covars6, viewmat, K, width, height, args, rel=U.REL_GAUSS):
    """bool [N], float64: the rows whose near / far, det1, radius-ceil, radius_clip or off-screen decision lies within
    `rel` (relative to the sizes of the quantities compared) of its threshold (tests.functional_util.covars_borderline
    for this model; there is no clamp decision).  The quats form passes the six numbers of its float64 covariance."""
    from oracle import ref_torch as O
    with torch.no_grad():
        q = _internals(means.double(), F.sym_from6(covars6.double()), viewmat.double(), K.double(), args["near_plane"],
                       args["far_plane"], args["eps2d"])
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
    return planes | (bad & q["in_z"].numpy())


def ref_vjps(form, inputs, viewmats, Ks, args, cots, dtype=torch.float64):
    """ref_project_ortho + autograd for the cameras of one call, one output's cotangent at a time.  `inputs`: (means,
    quats, scales) or (means, covars6).  Returns (outs: {name: [C, N, ...], "radii"}, grads: {cotangent: {input name:
    [N, k] summed over the cameras}})."""
    names = FORMS[form]
    p = [t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    a = (args["near_plane"], args["far_plane"], args["eps2d"], args["radius_clip"])
    per_cam = []
    for c in range(viewmats.shape[0]):
        vm, K = viewmats[c].to(dtype), Ks[c].to(dtype)
        per_cam.append(ref_project_ortho(p[0], p[1], p[2], vm, K, W, H, *a) if form == "quats"
                       else ref_project_ortho(p[0], None, None, vm, K, W, H, *a, covars=p[1]))
    outs = {"radii": torch.stack([o[0] for o in per_cam])}
    for i, name in enumerate(U.PROJ_OUTPUTS):
        outs[name] = torch.stack([o[1 + i] for o in per_cam])
    grads = {}
    for name, cot in cots.items():
        y = outs[name]
        g = torch.autograd.grad(y, p, cot.to(dtype).reshape(y.shape), retain_graph=True, allow_unused=True)
        grads[name] = {k: (gi if gi is not None else torch.zeros_like(pi)).detach() for k, gi, pi in zip(names, g, p)}
    return {k: v.detach() for k, v in outs.items()}, grads


# ---------------------------------------------------------------------------------------------------
_cache = {}


def ortho_intrinsics(Ks, depth):
    """fx / d, fy / d; the principal point stays"""
    K = Ks.clone()
    K[..., 0, 0] = Ks[..., 0, 0] / depth
    K[..., 1, 1] = Ks[..., 1, 1] / depth
    return K


def scene():
    """fp32 (means [N,3], quats [N,4], scales [N,3], covars [N,6] = fp32(triu(float64 covariance)), group [N]) built in
    the space of camera 0; its centre (0, 0, CENTRE_DEPTH) there."""
    if "scene" in _cache:
        return _cache["scene"]
    from oracle import ref_torch as O
    vms, Ks = U.projection_cameras()
    vm, Kd = vms[0].double(), Ks[0].double()
    R, t = vm[:3, :3], vm[:3, 3]
    fx_o, fy_o = float(Kd[0, 0]) / CENTRE_DEPTH, float(Kd[1, 1]) / CENTRE_DEPTH
    gen = torch.Generator().manual_seed(SEED)
    N = N_FULL
    group = torch.tensor([GROUP_PATTERN[i % len(GROUP_PATTERN)] for i in range(N)])
    u = torch.rand(N, 3, generator=gen, dtype=torch.float64)
    pick = lambda f: torch.tensor([f(GROUPS[g]) for g in group.tolist()], dtype=torch.float64)
    ax = pick(lambda g: g[0][0][0]) + (pick(lambda g: g[0][0][1]) - pick(lambda g: g[0][0][0])) * u[:, 0]
    ay = pick(lambda g: g[0][1][0]) + (pick(lambda g: g[0][1][1]) - pick(lambda g: g[0][1][0])) * u[:, 1]
    z_lo, z_hi = pick(lambda g: (g[1] or Z_RANGE)[0]), pick(lambda g: (g[1] or Z_RANGE)[1])
    z = z_lo + (z_hi - z_lo) * u[:, 2]
    p_c = torch.stack([ax * (W / 2) / fx_o, ay * (H / 2) / fy_o, z], dim=-1)
    means = (p_c - t) @ R
    quats = torch.randn(N, 4, generator=gen, dtype=torch.float64) * (0.5 + torch.rand(N, 1, generator=gen, dtype=torch.float64))
    size = pick(lambda g: g[2])[:, None] * (0.7 + 0.7 * torch.rand(N, 1, generator=gen, dtype=torch.float64))
    perm = torch.argsort(torch.rand(N, 3, generator=gen), dim=1)
    ratios = torch.tensor([GROUPS[g][3] for g in group.tolist()], dtype=torch.float64)
    scales = size * torch.gather(ratios, 1, perm)
    means, quats, scales = means.float().contiguous(), quats.float().contiguous(), scales.float().contiguous()
    covars = F.triu6(O.quat_scale_to_covar(quats.double(), scales.double())).float().contiguous()
    _cache["scene"] = (means, quats, scales, covars, group)
    return _cache["scene"]


def cameras(n_cams):
    """(viewmats [C,4,4], orthographic Ks [C,3,3], extent): camera c's intrinsics divided by the depth of the scene
    centre in camera c; extent = the largest |camera-space coordinate| of the scene over these cameras."""
    vms_all, Ks_all = U.projection_cameras()
    cams = list(CAMS[n_cams])
    vms, Ks = vms_all[cams].contiguous(), Ks_all[cams].clone()
    centre_w = (torch.tensor([0.0, 0.0, CENTRE_DEPTH], dtype=torch.float64) - vms_all[0].double()[:3, 3]) @ vms_all[0].double()[:3, :3]
    means = scene()[0].double()
    extent = 0.0
    for c in range(len(cams)):
        R, t = vms[c].double()[:3, :3], vms[c].double()[:3, 3]
        Ks[c] = ortho_intrinsics(Ks[c], float((R @ centre_w + t)[2]))
        extent = max(extent, float((means @ R.T + t).abs().max()))
    return vms, Ks.contiguous(), extent


def reference(form, args_name, n_cams):
    """Everything the comparisons of one (form, arguments, cameras) case need, on the N_FULL rows (the first n rows of
    every per-row entry are the reference of size n): fp32 inputs, N(0,1) cotangents [C, N, k] of the four outputs,
    float64 outputs and per-cotangent gradients summed over the cameras, kappa per (cotangent, gradient) from four
    one-ulp perturbations, the per-camera borderline sets, the rows the compensation cotangent is checked on."""
    from oracle import ref_torch as O
    key = ("ref", form, args_name, n_cams)
    if key in _cache:
        return _cache[key]
    means, quats, scales, covars, group = scene()
    inputs = (means, quats, scales) if form == "quats" else (means, covars)
    vms, Ks, extent = cameras(n_cams)
    args = ARGS[args_name]
    N, C = means.shape[0], vms.shape[0]
    gen = torch.Generator().manual_seed(13)
    widths = dict(means2d=2, depths=1, conics=3, compensations=1)
    cots = {name: torch.randn(C, N, widths[name], generator=gen) for name in U.PROJ_OUTPUTS}
    outs, grads = ref_vjps(form, inputs, vms, Ks, args, cots)
    pert = [ref_vjps(form, U.ulp_perturbed(inputs, gen), vms, Ks, args, cots)[1] for _ in range(4)]
    kappa = {c: {g: U.row_kappa(grads[c][g], [p[c][g] for p in pert]) for g in FORMS[form]} for c in cots}
    cov6 = covars if form == "covars" else F.triu6(O.quat_scale_to_covar(quats.double(), scales.double()))
    border = np.stack([ortho_borderline(means, cov6, vms[c], Ks[c], W, H, args) for c in range(C)])
    vis = outs["radii"].numpy() > 0
    comp = outs["compensations"].numpy()
    comp_ok = 1.0 - comp * comp >= U.COMP_MIN_ONE_MINUS_SQ
    comp_rows = vis.any(axis=0) & (comp_ok | ~vis).all(axis=0)
    ref = dict(form=form, args=args, inputs=inputs, names=FORMS[form], means=means, quats=quats, scales=scales, covars=covars,
               group=group, viewmats=vms, Ks=Ks, extent=extent, cots=cots, outs=outs, grads=grads, kappa=kappa, border=border,
               vis=vis, comp_rows=comp_rows)
    _cache[key] = ref
    return ref


def pose_reference(args_name, n_cams):
    """{cotangent: float64 G [C, N, 3, 4]}: the contribution of every pair to the gradient of sum(out * cotangent) with
    respect to viewmats[c] (quats form, the cotangents of `reference`), from ONE ref_project_ortho call per camera with a
    viewmat per Gaussian; and the largest |bottom-row entry| autograd returned.  The reference of a call on the first n
    rows is G[:, :n].sum(1), its scale |G|[:, :n].sum(1) (tests/viewmat_util.py)."""
    key = ("pose", args_name, n_cams)
    if key in _cache:
        return _cache[key]
    ref = reference("quats", args_name, n_cams)
    a = ref["args"]
    C, N = ref["vis"].shape
    p = [t.double() for t in ref["inputs"]]
    G = {k: torch.zeros(C, N, 3, 4, dtype=torch.float64) for k in ref["cots"]}
    bottom = 0.0
    for c in range(C):
        vm = ref["viewmats"][c].double().expand(N, 4, 4).clone().requires_grad_(True)
        out = ref_project_ortho(p[0], p[1], p[2], vm, ref["Ks"][c].double(), W, H, a["near_plane"], a["far_plane"], a["eps2d"],
                                a["radius_clip"])
        for k, cot in ref["cots"].items():
            y = out[1 + U.PROJ_OUTPUTS.index(k)]
            g = torch.autograd.grad(y, vm, cot[c].double().reshape(y.shape), retain_graph=True)[0]
            G[k][c] = g[:, :3]
            bottom = max(bottom, float(g[:, 3].abs().max()))
    _cache[key] = (G, bottom)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------
# The whole call (tests/test_gpu_ortho.py): a synth scene under orthographic intrinsics, its float-borderline sets, and
# the oracle's binning and compositing on the orthographic reference projection.
WHOLE_ARGS = dict(n_gauss=500, n_views=4, width=70, height=52, seed=3, spread_opacity=True, scale=0.02, anisotropy=5.0)
WHOLE_CAMS = (0, 1)
TILE_SIZES = (8, 16, 32)


def whole_scene():
    """dict(means, quats, scales, opacities: fp32 leaves' values; viewmats, Ks (pinhole), Ks_o (ortho: K / depth of the
    scene's centroid in each camera), W, H, removed, n0) for the cameras WHOLE_CAMS, without the Gaussians whose integer
    decisions (culls, radius ceil, the tile box at 8, 16 or 32 pixels) hinge on rounding in any of them."""
    if "whole" in _cache:
        return _cache["whole"]
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    from tests import tile_util as TU
    a = WHOLE_ARGS
    sc = synth.make_scene(a["n_gauss"], a["n_views"], a["width"], a["height"], seed=a["seed"], spread_opacity=a["spread_opacity"],
                          scale=a["scale"], anisotropy=a["anisotropy"])
    cams = list(WHOLE_CAMS)
    vms, Ks = sc.viewmats[cams].contiguous(), sc.Ks[cams].contiguous()
    centre = sc.means.double().mean(0)
    Ks_o = Ks.clone()
    for c in range(len(cams)):
        Ks_o[c] = ortho_intrinsics(Ks[c], float((vms[c].double()[:3, :3] @ centre + vms[c].double()[:3, 3])[2]))
    means, quats, scales = sc.means, sc.quats, torch.exp(sc.log_scales)
    cov6 = F.triu6(O.quat_scale_to_covar(quats.double(), scales.double()))
    bad = np.zeros(means.shape[0], bool)
    for c in range(len(cams)):
        bad |= ortho_borderline(means, cov6, vms[c], Ks_o[c], sc.width, sc.height, U.PROJ_DEFAULTS)
        with torch.no_grad():
            radii, m2d = ref_project_ortho(means, quats, scales, vms[c], Ks_o[c], sc.width, sc.height)[:2]
        for ts in TILE_SIZES:
            bad |= TU.tile_box_borderline(m2d.numpy(), radii.numpy(), ts)
    keep = torch.from_numpy(~bad)
    out = dict(means=means[keep].contiguous(), quats=quats[keep].contiguous(), scales=scales[keep].contiguous(),
               opacities=torch.sigmoid(sc.logit_opacities).squeeze(-1)[keep].contiguous(), viewmats=vms, Ks=Ks, Ks_o=Ks_o.contiguous(),
               W=sc.width, H=sc.height, removed=int(bad.sum()), n0=int(means.shape[0]))
    _cache["whole"] = out
    return out


def whole_projection(ws, c, p=None):
    """ref_project_ortho in fp32 for camera c of the whole-call scene (on the leaves `p` = (means, quats, scales) if given)"""
    m, q, s = p if p is not None else (ws["means"], ws["quats"], ws["scales"])
    return ref_project_ortho(m, q, s, ws["viewmats"][c], ws["Ks_o"][c], ws["W"], ws["H"])


def whole_keep(ts, antialiased):
    """bool [C, H, W]: the pixels whose walk over the oracle's `ts`-pixel tile lists stays clear of the float thresholds
    (tests.tile_util.borderline_pixels_ts for this projection: alpha within REL_ALPHA of 1/255 or 0.999, running T within
    REL_T of 1e-4, on an entry the walk looks at), in float64 from the fp32 reference projection."""
    key = ("keep", ts, antialiased)
    if key in _cache:
        return _cache[key]
    import math
    from oracle import ref_torch as O
    ws = whole_scene()
    W_, H_ = ws["W"], ws["H"]
    tw, th = math.ceil(W_ / ts), math.ceil(H_ / ts)
    amin, amax, tstop = 1.0 / 255.0, 0.999, 1e-4
    masks = []
    for c in range(len(WHOLE_CAMS)):
        with torch.no_grad():
            radii, m2d, depths, conics, comp = whole_projection(ws, c)
        op = (ws["opacities"] * comp if antialiased else ws["opacities"]).numpy().astype(np.float64)
        _tpg, ids, flat = O.isect_tiles(m2d.numpy(), radii.numpy(), depths.numpy(), ts, tw, th)
        offs = np.concatenate([O.isect_offset_encode(ids, tw, th).reshape(-1).astype(np.int64), [flat.shape[0]]])
        m, con = m2d.numpy().astype(np.float64), conics.numpy().astype(np.float64)
        mask = np.zeros((H_, W_), bool)
        for t in range(tw * th):
            g = flat[offs[t]:offs[t + 1]]
            if g.size == 0:
                continue
            ty, tx = divmod(t, tw)
            ii, jj = np.meshgrid(np.arange(ty * ts, min(ty * ts + ts, H_)), np.arange(tx * ts, min(tx * ts + ts, W_)), indexing="ij")
            dx = m[g, 0][None, :] - (jj.reshape(-1, 1) + 0.5)
            dy = m[g, 1][None, :] - (ii.reshape(-1, 1) + 0.5)
            sigma = 0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
            araw = op[g][None, :] * np.exp(-sigma)
            alpha = np.minimum(amax, araw)
            incl = (sigma >= 0.0) & (alpha >= amin)
            T_after = np.cumprod(np.where(incl, 1.0 - alpha, 1.0), axis=1)
            stops = incl & (T_after <= tstop)
            first = np.where(stops.any(axis=1), stops.argmax(axis=1), g.size)
            looked = np.arange(g.size)[None, :] <= first[:, None]
            near_a = (np.abs(araw - amin) <= U.REL_ALPHA * amin) | (np.abs(araw - amax) <= U.REL_ALPHA * amax)
            near_T = incl & (np.abs(T_after - tstop) <= U.REL_T * tstop)
            mask[ii.reshape(-1), jj.reshape(-1)] = (looked & (near_a | near_T)).any(axis=1)
        masks.append(torch.from_numpy(~mask))
    _cache[key] = torch.stack(masks)
    return _cache[key]


def oracle_whole(p, colors_of, ts, antialiased):
    """The reference image of the whole call on the CPU leaves p = (means, quats, scales, opacities): ref_project_ortho
    -> oracle isect_tiles -> isect_offset_encode -> composite, per camera.  `colors_of(c, projection)` gives camera c's
    colours [N, D] (on the graph).  Returns (render [C, H, W, D], alphas [C, H, W, 1], projections)."""
    import math
    from oracle import ref_torch as O
    ws = whole_scene()
    W_, H_ = ws["W"], ws["H"]
    tw, th = math.ceil(W_ / ts), math.ceil(H_ / ts)
    renders, alphas, projs = [], [], []
    for c in range(len(WHOLE_CAMS)):
        pr = whole_projection(ws, c, p[:3])
        radii, m2d, depths, conics, comp = pr
        op = p[3] * comp if antialiased else p[3]
        _tpg, ids, flat = O.isect_tiles(m2d.detach().numpy(), radii.numpy(), depths.detach().numpy(), ts, tw, th)
        offs = O.isect_offset_encode(ids, tw, th)
        r, a, _last = O.composite(m2d, conics, colors_of(c, pr), op, W_, H_, ts, offs, flat)
        renders.append(r)
        alphas.append(a)
        projs.append(pr)
    return torch.stack(renders), torch.stack(alphas), projs
