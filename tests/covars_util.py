"""References and scene discipline of the tests of `rasterization(covars=[N, 3, 3])` (tests/test_covars_host.py on the
CPU, tests/test_gpu_covars.py on the device).

The projection references are tests.functional_util.ref_project_covars (pinhole) and tests.ortho_util.ref_project_ortho
(covars=..., orthographic), float64 with autograd.  `ref_project_covars_pg` restates the first with a viewmat per
Gaussian ([N, 4, 4]), as tests/ortho_util.py's reference takes one: the gradient with respect to it is the contribution
of every pair to the pose gradient, in one call.  The [N, 3, 3] gradient convention is autograd's through
``sym_from6(covars[:, IU, JU])``.  The whole-call scene is tests/ortho_util.py's under the scene's own (pinhole)
intrinsics, with the covariances as leaves.  Every reference is computed once per process and never modified."""
import math

import numpy as np
import torch

from tests import functional_util as F
from tests import ortho_util as OU
from tests import util as U

W, H = U.PROJ_SIZE
IU, JU = [i for i, _ in F.TRIU], [j for _, j in F.TRIU]
LOWER = [(1, 0), (2, 0), (2, 1)]
SIZES = OU.SIZES
POSE_CASES = {"pinhole": "three_cams_eps1", "ortho": ("eps1", 3)}
POSE_MIN_PAIRS = 200


def full33(c6, lower=None):
    """[N, 6] -> [N, 3, 3] with the six numbers in the upper triangle; below the diagonal the symmetric entries, or with
    `lower` that constant (the call must not read it)."""
    out = F.sym_from6(c6).clone()
    if lower is not None:
        for i, j in LOWER:
            out[:, i, j] = lower
    return out.contiguous()


def upper6(g33):
    """[N, 3, 3] -> [N, 6]: the entries i <= j"""
    return g33[:, IU, JU]


def lower3(g33):
    """[N, 3, 3] -> [N, 3]: the entries below the diagonal"""
    return torch.stack([g33[:, i, j] for i, j in LOWER], dim=-1)


# ---------------------------------------------------------------------------------------------------
def ref_project_covars_pg(means, covars6, viewmat, K, width, height, near_plane=0.01, far_plane=1e10, eps2d=0.3,
                          radius_clip=0.0, covar_w=None):
    """tests.functional_util.ref_project_covars with `viewmat` [4, 4] or [N, 4, 4] (one per Gaussian): the same
    arithmetic, culls and cull order; (radii i32 [N], means2d [N, 2], depths [N], conics [N, 3], compensations [N]).
    With `covar_w` [N, 3, 3] (covars6 None) the world covariance is that full matrix, every entry a variable of its own."""
    from oracle import ref_torch as O
    dt = means.dtype
    N = means.shape[0]
    vm = viewmat.to(dt)
    vm = vm if vm.dim() == 3 else vm.expand(N, 4, 4)
    Rv, tv = vm[:, :3, :3], vm[:, :3, 3]
    fx, fy, cx, cy = K[0, 0].to(dt), K[1, 1].to(dt), K[0, 2].to(dt), K[1, 2].to(dt)
    mean_c = (Rv @ means[..., None])[..., 0] + tv
    x, y, z = mean_c.unbind(-1)
    in_z = (z >= near_plane) & (z <= far_plane)
    zs = torch.where(in_z, z, torch.ones_like(z))
    covar_c = Rv @ (covar_w if covar_w is not None else F.sym_from6(covars6)) @ Rv.transpose(-1, -2)
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
    det_ok = det1 > 0
    det1s = torch.where(det_ok, det1, torch.ones_like(det1))
    comp = O._Compensation.apply(det0 / det1s)
    inv = 1.0 / det1s
    conic = torch.stack([b11 * inv, -c01 * inv, b00 * inv], dim=-1)
    with torch.no_grad():
        bh = 0.5 * (b00 + b11)
        v1 = bh + torch.sqrt(torch.clamp(bh * bh - det1, min=O.RADIUS_DET_FLOOR))
        radius = torch.ceil(O.RADIUS_SIGMAS * torch.sqrt(v1))
        ok = in_z & det_ok & (radius > radius_clip)
        ok &= ~((mean2d[:, 0] + radius <= 0) | (mean2d[:, 0] - radius >= width)
                | (mean2d[:, 1] + radius <= 0) | (mean2d[:, 1] - radius >= height))
        radii = torch.where(ok, radius, torch.zeros_like(radius)).to(torch.int32)
    return (radii, torch.where(ok[:, None], mean2d, torch.zeros_like(mean2d)), torch.where(ok, z, torch.zeros_like(z)),
            torch.where(ok[:, None], conic, torch.zeros_like(conic)), torch.where(ok, comp, torch.zeros_like(comp)))


def ref_grad33(means, covars33, viewmats, Ks, args, cots, dtype=torch.float64):
    """The gradient of the [N, 3, 3] input as the call defines it: autograd through sym_from6(covars[:, IU, JU]) and
    ref_project_covars, one output's cotangent at a time.  Returns {cotangent: [N, 3, 3]}."""
    c = covars33.detach().to(dtype).clone().requires_grad_(True)
    m = means.detach().to(dtype).clone().requires_grad_(True)  # (every output is on the graph, whatever it depends on)
    c6 = c[:, IU, JU]
    per_cam = [F.ref_project_covars(m, c6, viewmats[k], Ks[k], W, H, args["near_plane"], args["far_plane"], args["eps2d"],
                                    args["radius_clip"]) for k in range(viewmats.shape[0])]
    grads = {}
    for name, cot in cots.items():
        y = torch.stack([o[1 + U.PROJ_OUTPUTS.index(name)] for o in per_cam])
        g = torch.autograd.grad(y, c, cot.to(dtype).reshape(y.shape), retain_graph=True, allow_unused=True)[0]
        grads[name] = (g if g is not None else torch.zeros_like(c)).detach()
    return grads


# ---------------------------------------------------------------------------------------------------
_cache = {}


def pose_inputs(model):
    """The reference dict of the pose-gradient case of `model` ("pinhole": tests.functional_util.covars_reference, "ortho":
    tests.ortho_util.reference in the covars form) and its arguments: both carry means, covars [N, 6], viewmats, Ks,
    cots (the four outputs), vis and border."""
    if model == "pinhole":
        ref = F.covars_reference(POSE_CASES[model])
        return ref, ref["spec"]["args"]
    ref = OU.reference("covars", *POSE_CASES[model])
    return ref, ref["args"]


def pose_reference(model):
    """({cotangent: float64 G [C, N, 3, 4]}, largest |bottom-row entry| autograd returned): the contribution of every
    pair to the gradient of sum(out * cotangent) with respect to viewmats[c], from ONE reference call per camera with a
    viewmat per Gaussian.  The reference of the call is G.sum(1), its scale |G|.sum(1) (tests/viewmat_util.py)."""
    key = ("pose", model)
    if key in _cache:
        return _cache[key]
    ref, a = pose_inputs(model)
    C, N = ref["vis"].shape
    m, c6 = ref["means"].double(), ref["covars"].double()
    G = {k: torch.zeros(C, N, 3, 4, dtype=torch.float64) for k in ref["cots"]}
    bottom = 0.0
    for c in range(C):
        vm = ref["viewmats"][c].double().expand(N, 4, 4).clone().requires_grad_(True)
        lims = (a["near_plane"], a["far_plane"], a["eps2d"], a["radius_clip"])
        if model == "pinhole":
            out = ref_project_covars_pg(m, c6, vm, ref["Ks"][c].double(), W, H, *lims)
        else:
            out = OU.ref_project_ortho(m, None, None, vm, ref["Ks"][c].double(), W, H, *lims, covars=c6)
        assert torch.equal(out[0], ref["outs"]["radii"][c])
        for k, cot in ref["cots"].items():
            y = out[1 + U.PROJ_OUTPUTS.index(k)]
            g = torch.autograd.grad(y, vm, cot[c].double().reshape(y.shape), retain_graph=True)[0]
            G[k][c] = g[:, :3]
            bottom = max(bottom, float(g[:, 3].abs().max()))
    _cache[key] = (G, bottom)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------
# Packed against dense (tests/test_gpu_ortho.py's scene with covariances as leaves): near_plane 3.7 and radius_clip 3.5
# keep about 70 % of the pairs under either camera model.
PACKED_ARGS = dict(near_plane=3.7, radius_clip=3.5)
PACKED_SHARE = (0.1, 0.95)


def packed_scene(ortho=False):
    """dict(means, covars [N, 6] = fp32(triu(float64 covariance of the scene's quats and scales)), quats, scales, opacities,
    viewmats [3, 4, 4], Ks [3, 3, 3] (orthographic: K / depth of the centroid), W, H) of synth.make_scene(500, 3, 70, 52)"""
    key = ("packed", ortho)
    if key in _cache:
        return _cache[key]
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    sc = synth.make_scene(500, 3, 70, 52, seed=3, spread_opacity=True, scale=0.02, anisotropy=5.0)
    centre = sc.means.double().mean(0)
    Ks = sc.Ks.clone()
    for c in range(3 if ortho else 0):
        Ks[c] = OU.ortho_intrinsics(sc.Ks[c], float((sc.viewmats[c].double()[:3, :3] @ centre + sc.viewmats[c].double()[:3, 3])[2]))
    scales = torch.exp(sc.log_scales)
    covars = F.triu6(O.quat_scale_to_covar(sc.quats.double(), scales.double())).float().contiguous()
    _cache[key] = dict(means=sc.means, covars=covars, quats=sc.quats, scales=scales,
                       opacities=torch.sigmoid(sc.logit_opacities).squeeze(-1).contiguous(),
                       viewmats=sc.viewmats.contiguous(), Ks=Ks.contiguous(), W=70, H=52)
    return _cache[key]


def packed_visible_share(ortho=False):
    """share of the Gaussians each camera keeps, from the float64 reference projection under PACKED_ARGS"""
    ps = packed_scene(ortho)
    m, c6 = ps["means"].double(), ps["covars"].double()
    shares = []
    with torch.no_grad():
        for c in range(3):
            vm, K = ps["viewmats"][c].double(), ps["Ks"][c].double()
            if ortho:
                radii = OU.ref_project_ortho(m, None, None, vm, K, ps["W"], ps["H"], covars=c6, **PACKED_ARGS)[0]
            else:
                radii = F.ref_project_covars(m, c6, vm, K, ps["W"], ps["H"], **PACKED_ARGS)[0]
            shares.append(float((radii > 0).float().mean()))
    return shares


# ---------------------------------------------------------------------------------------------------
# The whole call: tests/ortho_util.py's synth scene (WHOLE_ARGS, WHOLE_CAMS) under its own pinhole intrinsics, the
# covariances as leaves; float-borderline pixels and integer-borderline Gaussians as there.
TILE_SIZES = OU.TILE_SIZES
WHOLE_CAMS = OU.WHOLE_CAMS


def whole_scene():
    """dict(means, covars [N, 6], quats, scales, opacities: fp32 values; viewmats, Ks, W, H, removed, n0) for the cameras
    WHOLE_CAMS, without the Gaussians whose integer decisions (culls, radius ceil, the tile box at 8, 16 or 32 pixels)
    hinge on rounding in any of them."""
    if "whole" in _cache:
        return _cache["whole"]
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    from tests import tile_util as TU
    a = OU.WHOLE_ARGS
    sc = synth.make_scene(a["n_gauss"], a["n_views"], a["width"], a["height"], seed=a["seed"], spread_opacity=a["spread_opacity"],
                          scale=a["scale"], anisotropy=a["anisotropy"])
    cams = list(WHOLE_CAMS)
    vms, Ks = sc.viewmats[cams].contiguous(), sc.Ks[cams].contiguous()
    means, quats, scales = sc.means, sc.quats, torch.exp(sc.log_scales)
    cov6 = F.triu6(O.quat_scale_to_covar(quats.double(), scales.double())).float().contiguous()
    bad = np.zeros(means.shape[0], bool)
    for c in range(len(cams)):
        bad |= F.covars_borderline(means, cov6, vms[c], Ks[c], sc.width, sc.height, U.PROJ_DEFAULTS)
        with torch.no_grad():
            radii, m2d = F.ref_project_covars(means, cov6, vms[c], Ks[c], sc.width, sc.height)[:2]
        for ts in TILE_SIZES:
            bad |= TU.tile_box_borderline(m2d.numpy(), radii.numpy(), ts)
    keep = torch.from_numpy(~bad)
    out = dict(means=means[keep].contiguous(), covars=cov6[keep].contiguous(), quats=quats[keep].contiguous(),
               scales=scales[keep].contiguous(), opacities=torch.sigmoid(sc.logit_opacities).squeeze(-1)[keep].contiguous(),
               viewmats=vms, Ks=Ks, W=sc.width, H=sc.height, removed=int(bad.sum()), n0=int(means.shape[0]))
    _cache["whole"] = out
    return out


def whole_projection(ws, c, p=None):
    """ref_project_covars in fp32 for camera c of the whole-call scene (on the leaves `p` = (means, covars6) if given)"""
    m, c6 = p if p is not None else (ws["means"], ws["covars"])
    return F.ref_project_covars(m, c6, ws["viewmats"][c], ws["Ks"][c], ws["W"], ws["H"])


def whole_keep(ts, antialiased):
    """bool [C, H, W]: the pixels whose walk over the oracle's `ts`-pixel tile lists stays clear of the float thresholds
    (tests.ortho_util.whole_keep for this projection: alpha within REL_ALPHA of 1/255 or 0.999, running T within REL_T of
    1e-4, on an entry the walk looks at), in float64 from the fp32 reference projection."""
    key = ("keep", ts, antialiased)
    if key in _cache:
        return _cache[key]
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
    """The reference image of the whole call on the CPU leaves p = (means, covars33 [N, 3, 3], opacities):
    ref_project_covars on covars33[:, IU, JU] -> oracle isect_tiles -> isect_offset_encode -> composite, per camera.
    `colors_of(c, projection)` gives camera c's colours [N, D] (on the graph).  Returns (render [C, H, W, D], alphas
    [C, H, W, 1], projections)."""
    from oracle import ref_torch as O
    ws = whole_scene()
    W_, H_ = ws["W"], ws["H"]
    tw, th = math.ceil(W_ / ts), math.ceil(H_ / ts)
    renders, alphas, projs = [], [], []
    c6 = p[1][:, IU, JU]
    for c in range(len(WHOLE_CAMS)):
        pr = whole_projection(ws, c, (p[0], c6))
        radii, m2d, depths, conics, comp = pr
        op = p[2] * comp if antialiased else p[2]
        _tpg, ids, flat = O.isect_tiles(m2d.detach().numpy(), radii.numpy(), depths.detach().numpy(), ts, tw, th)
        offs = O.isect_offset_encode(ids, tw, th)
        r, a, _last = O.composite(m2d, conics, colors_of(c, pr), op, W_, H_, ts, offs, flat)
        renders.append(r)
        alphas.append(a)
        projs.append(pr)
    return torch.stack(renders), torch.stack(alphas), projs


def whole_inputs():
    """(whole scene, colours [N, 3], render weights [C, H, W, 3], alpha weights [C, H, W, 1])"""
    ws = whole_scene()
    g = torch.Generator().manual_seed(29)
    N = ws["means"].shape[0]
    C = len(WHOLE_CAMS)
    colors = 0.2 + 0.8 * torch.rand(N, 3, generator=g)
    wr = torch.rand(C, ws["H"], ws["W"], 3, generator=g)
    wa = torch.rand(C, ws["H"], ws["W"], 1, generator=g)
    return ws, colors, wr, wa
