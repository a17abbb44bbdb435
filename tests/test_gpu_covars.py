"""`rasterization(covars=[N, 3, 3])` on the device, against the float64 references of tests/covars_util.py (whose
conditions tests/test_covars_host.py asserts with the references alone):

1. the dense call is the stage call `fully_fused_projection(covars=[N, 6])`, bit for bit, outputs and gradients;
2. packed=True against packed=False under both camera models, sparse_grad included; 3. the packed backward per row
against float64; 4. the pose gradient in both layouts under both camera models; 5. the whole call against the oracle's
binning and compositing on the reference projection, tile sizes 8 / 16 / 32, both modes; 6. the covariance form against
the quats + scales form; 7. one case each of RGB+ED with backgrounds, five channels, spherical harmonics, the dense
orthographic call, an empty visible set; 8. a call without the argument is the call it was.

Every test that passes `covars=` fails without the feature (TypeError: an unexpected keyword argument).

The compositing backward accumulates with float atomics (its bits vary from run to run), so wherever two device runs are
compared bit for bit through a backward, the loss is formed on the projection's outputs (info["means2d"], ["depths"],
["conics"], ["opacities"]), whose backward adds in a fixed order."""
import pytest
import torch

from tests import covars_util as CU
from tests import functional_util as F
from tests import ortho_util as OU
from tests import util as U
from tests import viewmat_util as V
from tests.tile_util import BORDER_CAP
from tests.util import assert_close, record, rel_err

pytestmark = pytest.mark.gpu

W, H = U.PROJ_SIZE
MODES = ("classic", "antialiased")
INFO_OF = dict(means2d="means2d", depths="depths", conics="conics", compensations="opacities")


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import rasterizer
    return rasterizer


def _args_kw(a):
    return dict(eps2d=a["eps2d"], near_plane=a["near_plane"], far_plane=a["far_plane"], radius_clip=a["radius_clip"])


def _tensor_items(info):
    return {k: v for k, v in info.items() if isinstance(v, torch.Tensor)}


def _same_layout(info, info_q, packed):
    """`info` of a covars call against the quats + scales call's: the same keys, dtypes and trailing shapes; the whole
    shape wherever it does not depend on which pairs are visible."""
    assert set(info.keys()) == set(info_q.keys())
    for k, v in info_q.items():
        if not isinstance(v, torch.Tensor):
            assert type(info[k]) is type(v) and (v is None or info[k] == v), k
            continue
        t = info[k]
        assert isinstance(t, torch.Tensor) and t.dtype == v.dtype and t.dim() == v.dim() and t.shape[1:] == v.shape[1:], k
        if k in ("isect_offsets", "last_ids") or (not packed and k not in ("isect_ids", "flatten_ids")):
            assert t.shape == v.shape, k


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CU.SIZES)
@pytest.mark.parametrize("case", F.COVAR_CASES)
def test_dense_call_is_the_stage_call(env, case, n):
    """rasterization(packed=False, covars=S) on the first n rows of a projection case: info["radii" | "means2d" |
    "depths" | "conics"] and the compensation folded into info["opacities"] are fully_fused_projection(means, S[:, iu, ju],
    None, None, ...), torch.equal; for a loss on those outputs means.grad and the upper triangle of covars.grad are the
    stage call's gradients bit for bit and the lower triangle -- filled with junk in the input -- gets exactly zero."""
    import gsplat
    spec, means, c6, _q, _s, vms, Ks, _g = F.covars_inputs(case)
    kw = _args_kw(spec["args"])
    C = vms.shape[0]
    g = torch.Generator().manual_seed(17 + n)
    opac = (0.1 + 0.8 * torch.rand(n, generator=g)).cuda()
    colors = torch.rand(n, 3, generator=g).cuda()
    w = dict(means2d=torch.randn(C, n, 2, generator=g).cuda(), depths=torch.randn(C, n, generator=g).cuda(),
             conics=torch.randn(C, n, 3, generator=g).cuda(), opacities=torch.randn(C, n, generator=g).cuda())
    vms, Ks = vms.cuda(), Ks.cuda()
    for mode in MODES:
        aa = mode == "antialiased"
        m1 = means[:n].cuda().requires_grad_(True)
        s1 = CU.full33(c6[:n], lower=123.0).cuda().requires_grad_(True)
        _r, _a, info = gsplat.rasterization(m1, None, None, opac, colors, vms, Ks, W, H, packed=False, rasterize_mode=mode,
                                            covars=s1, **kw)
        m2 = means[:n].cuda().requires_grad_(True)
        s2 = c6[:n].cuda().requires_grad_(True)
        radii, means2d, depths, conics, comps = gsplat.fully_fused_projection(m2, s2, None, None, vms, Ks, W, H,
                                                                              calc_compensations=aa, **kw)
        assert (comps is not None) == aa
        op2 = opac[None].expand(C, n) * comps if aa else opac[None].expand(C, n)
        stage = dict(radii=radii, means2d=means2d, depths=depths, conics=conics, opacities=op2)
        for k, t in stage.items():
            assert info[k].dtype == t.dtype and torch.equal(info[k].detach(), t.detach()), (mode, k)
        sum((info[k] * w[k]).sum() for k in w).backward()
        sum((stage[k] * w[k]).sum() for k in w).backward()
        assert torch.equal(m1.grad, m2.grad), mode
        assert s1.grad.shape == (n, 3, 3)
        assert torch.equal(CU.upper6(s1.grad), s2.grad), mode
        assert not CU.lower3(s1.grad).any(), mode
        assert n == 1 or ((radii > 0).any() and s2.grad.abs().max() > 0 and m2.grad.abs().max() > 0)


# ---------------------------------------------------------------------------------------------------
def _packed_scene(ortho):
    ps = CU.packed_scene(ortho)
    g = torch.Generator().manual_seed(41)
    N = ps["means"].shape[0]
    leaves = [ps["means"], CU.full33(ps["covars"]), ps["opacities"], 0.2 + 0.8 * torch.rand(N, 3, generator=g)]
    fixed = dict(viewmats=ps["viewmats"].cuda(), Ks=ps["Ks"].cuda(), width=70, height=52,
                 backgrounds=torch.rand(3, 3, generator=g).cuda(), camera_model="ortho" if ortho else "pinhole", **CU.PACKED_ARGS)
    w = dict(render=torch.rand(3, 52, 70, 3, generator=g).cuda(), alpha=torch.rand(3, 52, 70, 1, generator=g).cuda(),
             means2d=torch.randn(3, N, 2, generator=g).cuda(), depths=torch.randn(3, N, generator=g).cuda(),
             conics=torch.randn(3, N, 3, generator=g).cuda(), opacities=torch.randn(3, N, generator=g).cuda())
    return leaves, fixed, w, N


def _packed_run(leaves, fixed, w, mode, loss_kind, **kw):
    from edgegaussians_amd import rasterization
    p = [t.clone().cuda().requires_grad_(True) for t in leaves]
    render, alpha, info = rasterization(p[0], None, None, p[2], p[3], rasterize_mode=mode, covars=p[1], **fixed, **kw)
    cam, gid = info["camera_ids"], info["gaussian_ids"]
    pick = (lambda t: t[cam, gid]) if cam is not None else (lambda t: t)
    if loss_kind == "image":
        loss = (render * w["render"]).sum() + (alpha * w["alpha"]).sum()
    else:   # the projection's outputs only: a backward without atomics
        loss = sum((info[k] * pick(w[k])).sum() for k in ("means2d", "depths", "conics", "opacities"))
    loss.backward()
    torch.cuda.synchronize()
    return render.detach(), alpha.detach(), info, [t.grad for t in p]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ortho", [False, True], ids=["pinhole", "ortho"])
def test_packed_equals_the_dense_call(env, ortho, mode):
    """packed=True with covars: the id lists are the set radii > 0 of the packed=False call in ascending order, every
    per-pair info tensor is the dense one at [camera_ids, gaussian_ids] bit for bit, render and alphas are torch.equal;
    dense gradients of an image loss agree to 1e-4 (the compositing backward adds with atomics); with sparse_grad the
    gradients of means and covars for a loss on the projection's outputs are sparse with indices gaussian_ids (covars:
    values [nnz, 3, 3]) and equal the dense ones after to_dense() (to 1e-6: a three-camera sum in another order); they
    are marked coalesced exactly when there is one camera.  near_plane 3.7 and radius_clip 3.5 cull a part of the pairs."""
    leaves, fixed, w, N = _packed_scene(ortho)
    rd, ad, di, gd = _packed_run(leaves, fixed, w, mode, "image", packed=False)
    rp, ap, pi, gp = _packed_run(leaves, fixed, w, mode, "image", packed=True)
    cam, gid = pi["camera_ids"], pi["gaussian_ids"]
    vis = di["radii"] > 0
    share = vis.float().mean(dim=1).tolist()
    print("visible share per camera:", share)
    assert CU.PACKED_SHARE[0] <= min(share) and max(share) <= CU.PACKED_SHARE[1], share
    assert torch.equal(cam * N + gid, torch.nonzero(vis.reshape(-1))[:, 0])
    for k in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss"):
        assert torch.equal(pi[k].detach(), di[k].detach()[cam, gid]), k
    assert torch.equal(rp, rd) and torch.equal(ap, ad)
    assert float(ad.mean()) > 0.05
    names = ("means", "covars", "opacities", "colors")
    for name, a, b in zip(names, gp, gd):
        assert b.abs().max() > 0
        assert_close(a.cpu(), b.cpu(), name=f"packed grad {name}")
    for g33 in (gp[1], gd[1]):
        assert g33.shape == (N, 3, 3) and not CU.lower3(g33).any()
    _r, _a, _i, g_dense = _packed_run(leaves, fixed, w, mode, "projection", packed=True)
    _r, _a, si, g_sparse = _packed_run(leaves, fixed, w, mode, "projection", packed=True, sparse_grad=True)
    nnz = si["gaussian_ids"].shape[0]
    for name, a, b, tail in zip(names[:2], g_sparse, g_dense, ((3,), (3, 3))):
        assert a.is_sparse and torch.equal(a._indices()[0], si["gaussian_ids"]), name
        assert tuple(a.shape) == (N,) + tail and tuple(a._values().shape) == (nnz,) + tail, name
        assert not a.is_coalesced(), name   # (three cameras: a Gaussian may appear three times)
        assert b.abs().max() > 0
        assert_close(a.to_dense().cpu(), b.cpu(), rtol=1e-6, name=f"sparse grad {name}")
    assert not CU.lower3(g_sparse[1].to_dense()).any()
    assert_close(g_sparse[2].cpu(), g_dense[2].cpu(), rtol=1e-6, name="opacities")   # (a gather's backward: atomics over the cameras)
    # one camera: the ids are unique and ascending, and the gradients say so
    one = {k: (v[:1].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in fixed.items()}
    w1 = {k: v[:1].contiguous() for k, v in w.items()}
    _r, _a, _i, g1 = _packed_run(leaves, one, w1, mode, "projection", packed=True, sparse_grad=True)
    assert g1[0].is_sparse and g1[0].is_coalesced() and g1[1].is_sparse and g1[1].is_coalesced()


# ---------------------------------------------------------------------------------------------------
def _projection_call(ref, args, packed, camera_model="pinhole", with_pose=False):
    """rasterization(covars=..., rasterize_mode="antialiased") on a projection case with opacities of one, so that
    info["opacities"] IS the compensation; returns the leaves, the four outputs (per pair when packed) and the ids."""
    from edgegaussians_amd import rasterization
    N = ref["means"].shape[0]
    means = ref["means"].cuda().requires_grad_(True)
    covars = CU.full33(ref["covars"]).cuda().requires_grad_(True)
    vm = ref["viewmats"].clone().cuda().requires_grad_(with_pose)
    g = torch.Generator().manual_seed(3)
    colors = torch.rand(N, 3, generator=g).cuda()
    _r, _a, info = rasterization(means, None, None, torch.ones(N, device="cuda"), colors, vm, ref["Ks"].cuda(), W, H,
                                 packed=packed, rasterize_mode="antialiased", camera_model=camera_model, covars=covars,
                                 **_args_kw(args))
    C = vm.shape[0]
    vis = torch.zeros(C, N, dtype=torch.bool, device="cuda")
    cam, gid = info["camera_ids"], info["gaussian_ids"]
    if packed:
        vis[cam, gid] = True
    else:
        vis = info["radii"] > 0
    return dict(means=means, covars=covars, vm=vm, outs={k: info[INFO_OF[k]] for k in U.PROJ_OUTPUTS}, vis=vis.cpu(), cam=cam,
                gid=gid)


def _cotangent(run, name, cot, keep=None):
    y = run["outs"][name]
    ct = cot.cuda().reshape(cot.shape[0], cot.shape[1], -1)
    if keep is not None:
        ct = ct * keep.cuda()[..., None]
    if run["cam"] is not None:
        ct = ct[run["cam"], run["gid"]]
    return y, ct.reshape(y.shape).contiguous()


@pytest.mark.parametrize("case", F.COVAR_CASES)
def test_packed_backward_per_row_against_float64(env, case):
    """eg_packed_bwd_covars through rasterization(packed=True, covars=...): the gradients of means and covars (upper
    triangle; the lower exactly zero) for one N(0,1) cotangent per output, row by row under U.row_bound_check with the
    float64 reference's kappa, on every row but the reference's borderline ones (no cull decision differs outside that
    set); the compensation cotangent on comp_rows, as the projection tests take it."""
    ref = F.covars_reference(case)
    run = _projection_call(ref, ref["spec"]["args"], packed=True)
    vis, vis64 = run["vis"].numpy(), ref["vis"]
    differ = vis != vis64
    assert ref["border"].mean(axis=1).max() <= 0.02
    assert not (differ & ~ref["border"]).any(), f"{int((differ & ~ref['border']).sum())} cull decisions differ outside the borderline set"
    rows_ok = ~differ.any(axis=0)
    assert vis.sum() >= 100
    cells = {}
    got = {}
    for cot_name, cot in ref["cots"].items():
        y, ct = _cotangent(run, cot_name, cot)
        gm, gc = torch.autograd.grad(y, [run["means"], run["covars"]], ct, retain_graph=True)
        assert gc.shape == (ref["means"].shape[0], 3, 3) and not CU.lower3(gc).any()
        got[cot_name] = {"means": gm.cpu(), "covars": CU.upper6(gc).cpu()}
        rows = rows_ok & ref["comp_rows"] if cot_name == "compensations" else rows_ok
        for g in F.COVAR_GRADS:
            ratio, _loose, nonzero, over = U.row_bound_ratio(got[cot_name][g], ref["grads"][cot_name][g], ref["kappa"][cot_name][g], rows)
            cells[f"{cot_name}->{g}"] = ratio
            print(f"packed covars {case} {cot_name}->{g}: {ratio:.3f} of the bound, {over} rows over, {nonzero} rows not exactly zero")
    record("covars_packed_vjp_per_row", case=case, ratio_to_bound=cells, decision_mismatches_inside=int(differ.sum()))
    for cot_name in ref["cots"]:
        rows = rows_ok & ref["comp_rows"] if cot_name == "compensations" else rows_ok
        for g in F.COVAR_GRADS:
            U.row_bound_check(got[cot_name][g], ref["grads"][cot_name][g], ref["kappa"][cot_name][g],
                              f"packed covars {case} {cot_name}->v_{g}", rows)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("model", list(CU.POSE_CASES))
def test_pose_gradient(env, model, packed):
    """viewmats.grad of the covariance form (eg_project_covars_bwd_viewmats, both layouts, both camera models) against the
    float64 reference with a viewmat per Gaussian, entry by entry: |got - ref64| <= TAU_SMALL * S with S the sum of the
    pairs' absolute contributions (tests/viewmat_util.py), an exactly zero bottom row; asking for it leaves the
    gradients of means and covars bit for bit what they are without it."""
    ref, args = CU.pose_inputs(model)
    G, bottom = CU.pose_reference(model)
    assert bottom == 0.0
    assert ref["vis"].sum(axis=1).min() >= CU.POSE_MIN_PAIRS
    run = _projection_call(ref, args, packed, camera_model=model, with_pose=True)
    keep = run["vis"] == torch.from_numpy(ref["vis"])
    drop = ~keep
    assert not (drop.numpy() & ~ref["border"]).any(), "a cull decision differs outside the borderline set"
    pairs = [_cotangent(run, name, cot, keep) for name, cot in ref["cots"].items()]
    ratios, grads = {}, {}
    for name, (y, ct) in zip(ref["cots"], pairs):
        grads[name] = torch.autograd.grad(y, run["vm"], ct, retain_graph=True)[0].cpu()
        gk = G[name] * keep[:, :, None, None]
        ratios[name] = V.bound_ratio(grads[name], gk.sum(1), gk.abs().sum(1))[0]
        print(f"covars pose {model} {'packed' if packed else 'dense'} {name}: |got - ref64| / S = {ratios[name]:.3e} "
              f"({ratios[name] / V.TAU_SMALL:.3f} of the bound)")
    record("covars_viewmat_grad_per_entry", model=model, packed=packed, ratio_to_S=ratios, tau=V.TAU_SMALL,
           dropped_pairs=int(drop.sum()))
    for name in ref["cots"]:
        gk = G[name] * keep[:, :, None, None]
        assert gk.abs().sum() > 0
        V.check(grads[name], gk.sum(1), gk.abs().sum(1), f"covars pose {model} {name}", V.TAU_SMALL)
    ys, cts = [p[0] for p in pairs], [p[1] for p in pairs]
    with_pose = torch.autograd.grad(ys, [run["means"], run["covars"], run["vm"]], cts)
    plain = _projection_call(ref, args, packed, camera_model=model, with_pose=False)
    pairs0 = [_cotangent(plain, name, cot, keep) for name, cot in ref["cots"].items()]
    without = torch.autograd.grad([p[0] for p in pairs0], [plain["means"], plain["covars"]], [p[1] for p in pairs0])
    for name, a, b in zip(("means", "covars"), with_pose, without):
        assert b.abs().max() > 0 and torch.equal(a, b), name
    assert not with_pose[2][:, 3].any()


# ---------------------------------------------------------------------------------------------------
def _whole_device(ws, leaves, covars=True, **kw):
    """leaves: (means, covars33, opacities, colors) or, with covars=False, (means, quats, scales, opacities, colors)"""
    from edgegaussians_amd import rasterization
    p = [t.clone().cuda().requires_grad_(True) for t in leaves]
    vms, Ks = ws["viewmats"].cuda(), ws["Ks"].cuda()
    kw.setdefault("packed", False)
    if covars:
        render, alpha, info = rasterization(p[0], None, None, p[2], p[3], vms, Ks, ws["W"], ws["H"], covars=p[1], **kw)
    else:
        render, alpha, info = rasterization(p[0], p[1], p[2], p[3], p[4], vms, Ks, ws["W"], ws["H"], **kw)
    return p, render, alpha, info


def _whole_leaves(ws, colors):
    return [ws["means"], CU.full33(ws["covars"]), ws["opacities"], colors]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ts", CU.TILE_SIZES)
def test_whole_call_against_the_oracle(env, ts, mode):
    """rasterization(covars=..., packed=False, tile_size=ts) on two cameras with [N, 3] colours against ref_project_covars
    -> oracle isect_tiles -> isect_offset_encode -> composite in fp32 on the CPU and its autograd gradients of a
    random-cotangent loss (covars: the upper triangle, the lower exactly zero), to 1e-4 outside the float-borderline
    pixels (at most BORDER_CAP of them); no Gaussian of the synth scene had to be removed for an integer-borderline
    decision beyond the cap of the tile tests.  The covariances scaled by 4 give another image."""
    ws, colors, wr, wa = CU.whole_inputs()
    aa = mode == "antialiased"
    keep = CU.whole_keep(ts, aa)
    assert (~keep).float().mean() <= BORDER_CAP
    assert ws["removed"] <= max(3, 0.016 * ws["n0"])
    leaves = _whole_leaves(ws, colors)
    pc = [t.clone().requires_grad_(True) for t in leaves]
    r_c, a_c, projs = CU.oracle_whole(pc[:3], lambda c, pr: pc[3], ts, aa)
    ((r_c * wr * keep[..., None]).sum() + (a_c * wa * keep[..., None]).sum()).backward()
    pg, r_g, a_g, info = _whole_device(ws, leaves, tile_size=ts, rasterize_mode=mode)
    kg = keep.cuda()[..., None]
    ((r_g * wr.cuda() * kg).sum() + (a_g * wa.cuda() * kg).sum()).backward()
    assert torch.equal(info["radii"].cpu(), torch.stack([pr[0] for pr in projs]))
    assert info["tile_size"] == ts
    assert float(a_g.detach().mean()) > 0.05
    e = {"render": rel_err(r_g.detach().cpu()[keep], r_c.detach()[keep]), "alpha": rel_err(a_g.detach().cpu()[keep], a_c.detach()[keep])}
    names = ("means", "covars", "opacities", "colors")
    for name, a, b in zip(names, pg, pc):
        e[name] = rel_err(a.grad.cpu(), b.grad)
    record("covars_whole_call", tile_size=ts, mode=mode, gaussians=int(leaves[0].shape[0]), borderline_pixels=int((~keep).sum()),
           max_rel_err=e)
    print(f"covars whole call ts={ts} {mode}: {e}")
    assert_close(r_g.detach().cpu()[keep], r_c.detach()[keep], name="render")
    assert_close(a_g.detach().cpu()[keep], a_c.detach()[keep], name="alpha")
    assert not CU.lower3(pg[1].grad).any() and not CU.lower3(pc[1].grad).any()
    for name, a, b in zip(names, pg, pc):
        assert b.grad.abs().max() > 0
        assert_close(a.grad.cpu(), b.grad, name=f"grad {name}")
    # the argument reaches the kernels: four times the covariance is another image
    with torch.no_grad():
        r4 = _whole_device(ws, [leaves[0], 4.0 * leaves[1], leaves[2], leaves[3]], tile_size=ts, rasterize_mode=mode)[1]
    assert rel_err(r4.cpu(), r_g.detach().cpu()) > 0.1


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_both_forms_agree(env, packed):
    """rasterization(covars=quat_scale_to_covar_preci(q, s)[0]) against rasterization(q, s) on the whole-call scene: the
    images within 1e-4 on the keep mask of the whole-call test, and the gradients of q and s through the covariance
    (eg_quat_scale_to_covar_preci_bwd behind covars.grad) within 1e-4 of the direct ones, as are those of means,
    opacities and colours."""
    import gsplat
    ws, colors, wr, wa = CU.whole_inputs()
    keep = CU.whole_keep(16, False).cuda()[..., None]
    leaves = [ws["means"], ws["quats"], ws["scales"], ws["opacities"], colors]
    vms, Ks = ws["viewmats"].cuda(), ws["Ks"].cuda()
    runs = []
    for form in ("covars", "quats"):
        p = [t.clone().cuda().requires_grad_(True) for t in leaves]
        if form == "covars":
            cov = gsplat.quat_scale_to_covar_preci(p[1], p[2], compute_preci=False)[0]
            assert cov.shape == (p[0].shape[0], 3, 3)
            render, alpha, info = gsplat.rasterization(p[0], None, None, p[3], p[4], vms, Ks, ws["W"], ws["H"], packed=packed,
                                                       covars=cov)
        else:
            render, alpha, info = gsplat.rasterization(*p, vms, Ks, ws["W"], ws["H"], packed=packed)
        ((render * wr.cuda() * keep).sum() + (alpha * wa.cuda() * keep).sum()).backward()
        runs.append((render.detach(), alpha.detach(), info, [t.grad for t in p]))
    (rc, ac, ic, gc), (rq, aq, iq, gq) = runs
    _same_layout(ic, iq, packed)
    k3 = keep.expand_as(rc)
    assert_close(rc[k3].cpu(), rq[k3].cpu(), name="render")
    assert_close(ac[keep].cpu(), aq[keep].cpu(), name="alpha")
    for name, a, b in zip(("means", "quats", "scales", "opacities", "colors"), gc, gq):
        assert b.abs().max() > 0
        assert_close(a.cpu(), b.cpu(), name=f"grad {name}")


# ---------------------------------------------------------------------------------------------------
def _quats_info(ws, colors, **kw):
    with torch.no_grad():
        return _whole_device(ws, [ws["means"], ws["quats"], ws["scales"], ws["opacities"], colors], covars=False, **kw)[3]


def test_rider_depth_mode_with_backgrounds(env):
    """render_mode="RGB+ED" with backgrounds: the oracle composite of the reference projection with the depth as a fourth
    colour; colours + (1 - alpha) background, depth / alpha."""
    ws, colors, wr, wa = CU.whole_inputs()
    keep = CU.whole_keep(16, False)
    g = torch.Generator().manual_seed(43)
    C = len(CU.WHOLE_CAMS)
    bg = torch.rand(C, 3, generator=g)
    wd = torch.rand(C, ws["H"], ws["W"], 1, generator=g)
    leaves = _whole_leaves(ws, colors)
    pc = [t.clone().requires_grad_(True) for t in leaves]
    r4, a_c, _ = CU.oracle_whole(pc[:3], lambda c, pr: torch.cat([pc[3], pr[2][:, None]], dim=-1), 16, False)
    r_c = torch.cat([r4[..., :3] + (1.0 - a_c) * bg[:, None, None, :], r4[..., 3:] / a_c.clamp(min=1e-10)], dim=-1)
    seen = keep & (a_c.detach()[..., 0] > 0.05)   # (the expected depth divides by alpha)
    wfull = torch.cat([wr, wd], dim=-1) * seen[..., None]
    (r_c * wfull).sum().backward()
    pg, r_g, a_g, info = _whole_device(ws, leaves, render_mode="RGB+ED", backgrounds=bg.cuda())
    (r_g * wfull.cuda()).sum().backward()
    assert r_g.shape[-1] == 4
    _same_layout(info, _quats_info(ws, colors, render_mode="RGB+ED", backgrounds=bg.cuda()), False)
    assert_close(r_g.detach().cpu()[seen], r_c.detach()[seen], name="RGB+ED render")
    assert_close(a_g.detach().cpu()[keep], a_c.detach()[keep], name="alpha")
    for name, a, b in zip(("means", "covars", "opacities", "colors"), pg, pc):
        assert_close(a.grad.cpu(), b.grad, name=f"RGB+ED grad {name}")


def test_rider_five_channels(env):
    """D = 5 (the wide entries of csrc/tiles.hip behind the projection from covariances) against the oracle composite."""
    ws, _colors, _wr, _wa = CU.whole_inputs()
    keep = CU.whole_keep(16, True)
    g = torch.Generator().manual_seed(47)
    N = ws["means"].shape[0]
    colors = torch.rand(N, 5, generator=g)
    w5 = torch.rand(len(CU.WHOLE_CAMS), ws["H"], ws["W"], 5, generator=g) * keep[..., None]
    leaves = _whole_leaves(ws, colors)
    pc = [t.clone().requires_grad_(True) for t in leaves]
    r_c, a_c, _ = CU.oracle_whole(pc[:3], lambda c, pr: pc[3], 16, True)
    (r_c * w5).sum().backward()
    pg, r_g, a_g, info = _whole_device(ws, leaves, rasterize_mode="antialiased")
    (r_g * w5.cuda()).sum().backward()
    assert r_g.shape[-1] == 5
    _same_layout(info, _quats_info(ws, colors, rasterize_mode="antialiased"), False)
    assert_close(r_g.detach().cpu()[keep], r_c.detach()[keep], name="D=5 render")
    assert_close(a_g.detach().cpu()[keep], a_c.detach()[keep], name="D=5 alpha")
    for name, a, b in zip(("means", "covars", "opacities", "colors"), pg, pc):
        assert_close(a.grad.cpu(), b.grad, name=f"D=5 grad {name}")


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_rider_spherical_harmonics(env, packed):
    """sh_degree = 2 with covars: the colours are spherical_harmonics on means - campos, clamp_min(. + 0.5, 0) -- the
    unpacked covars call with those colours [C, N, 3] gives the same alphas bit for bit and the same image to 1e-6; the
    packed call goes through another compositing kernel: fp32 sums of at most a few dozen terms agree to 1e-5."""
    import gsplat
    ws, _colors, _wr, _wa = CU.whole_inputs()
    g = torch.Generator().manual_seed(53)
    N = ws["means"].shape[0]
    coeffs = (torch.randn(N, 9, 3, generator=g) * 0.3).cuda()
    means, opac, cov = ws["means"].cuda(), ws["opacities"].cuda(), CU.full33(ws["covars"]).cuda()
    vms, Ks = ws["viewmats"].cuda(), ws["Ks"].cuda()
    with torch.no_grad():
        r_sh, a_sh, info = gsplat.rasterization(means, None, None, opac, coeffs, vms, Ks, ws["W"], ws["H"], sh_degree=2,
                                                packed=packed, covars=cov)
        campos = torch.linalg.inv(vms)[:, :3, 3]
        dirs = means[None] - campos[:, None]
        cols = torch.clamp_min(gsplat.spherical_harmonics(2, dirs, coeffs[None].expand(vms.shape[0], N, 9, 3)) + 0.5, 0.0)
        r_dense, a_dense, _i = gsplat.rasterization(means, None, None, opac, cols.contiguous(), vms, Ks, ws["W"], ws["H"],
                                                    packed=False, covars=cov)
        info_q = gsplat.rasterization(means, ws["quats"].cuda(), ws["scales"].cuda(), opac, coeffs, vms, Ks, ws["W"], ws["H"],
                                      sh_degree=2, packed=packed)[2]
    _same_layout(info, info_q, packed)
    if packed:
        assert rel_err(a_sh.cpu(), a_dense.cpu()) <= 1e-5 and rel_err(r_sh.cpu(), r_dense.cpu()) <= 1e-5
    else:
        assert torch.equal(a_sh, a_dense)
        assert rel_err(r_sh.cpu(), r_dense.cpu()) <= 1e-6
    assert float(a_sh.mean()) > 0.05 and r_sh.shape[-1] == 3


def test_rider_dense_orthographic_call(env):
    """camera_model="ortho", packed=False with covars against ref_project_ortho(covars=...) -> the oracle's binning and
    compositing, on the whole-call scene under orthographic intrinsics (tests/ortho_util.py), to 1e-4 outside the
    float-borderline pixels of that scene's quats + scales form."""
    from oracle import ref_torch as O
    import math
    wo = OU.whole_scene()
    keep = OU.whole_keep(16, False)
    g = torch.Generator().manual_seed(29)
    N = wo["means"].shape[0]
    C = len(OU.WHOLE_CAMS)
    colors = 0.2 + 0.8 * torch.rand(N, 3, generator=g)
    wr = torch.rand(C, wo["H"], wo["W"], 3, generator=g) * keep[..., None]
    cov6 = F.triu6(O.quat_scale_to_covar(wo["quats"].double(), wo["scales"].double())).float()
    leaves = [wo["means"], CU.full33(cov6), wo["opacities"], colors]
    pc = [t.clone().requires_grad_(True) for t in leaves]
    tw, th = math.ceil(wo["W"] / 16), math.ceil(wo["H"] / 16)
    renders = []
    for c in range(C):
        radii, m2d, depths, conics, _comp = OU.ref_project_ortho(pc[0], None, None, wo["viewmats"][c], wo["Ks_o"][c], wo["W"], wo["H"],
                                                                 covars=pc[1][:, CU.IU, CU.JU])
        _tpg, ids, flat = O.isect_tiles(m2d.detach().numpy(), radii.numpy(), depths.detach().numpy(), 16, tw, th)
        renders.append(O.composite(m2d, conics, pc[3], pc[2], wo["W"], wo["H"], 16, O.isect_offset_encode(ids, tw, th), flat)[0])
    r_c = torch.stack(renders)
    (r_c * wr).sum().backward()
    from edgegaussians_amd import rasterization
    p = [t.clone().cuda().requires_grad_(True) for t in leaves]
    vms, Ks = wo["viewmats"].cuda(), wo["Ks_o"].cuda()
    r_g, a_g, info = rasterization(p[0], None, None, p[2], p[3], vms, Ks, wo["W"], wo["H"], packed=False, camera_model="ortho",
                                   covars=p[1])
    (r_g * wr.cuda()).sum().backward()
    with torch.no_grad():
        info_q = rasterization(p[0], wo["quats"].cuda(), wo["scales"].cuda(), p[2], p[3], vms, Ks, wo["W"], wo["H"], packed=False,
                               camera_model="ortho")[2]
    _same_layout(info, info_q, False)
    assert float(a_g.detach().mean()) > 0.05
    assert_close(r_g.detach().cpu()[keep], r_c.detach()[keep], name="ortho render")
    for name, a, b in zip(("means", "covars", "opacities", "colors"), p, pc):
        assert_close(a.grad.cpu(), b.grad, name=f"ortho grad {name}")


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_rider_empty_visible_set(env, packed):
    """far_plane in front of every Gaussian: the call returns the backgrounds, zero alphas, the per-pair tensors of the
    quats + scales call (empty when packed) and zero gradients."""
    ws, colors, _wr, _wa = CU.whole_inputs()
    C = len(CU.WHOLE_CAMS)
    bg = torch.rand(C, 3, generator=torch.Generator().manual_seed(59)).cuda()
    kw = dict(packed=packed, backgrounds=bg, far_plane=0.02)
    pg, r_g, a_g, info = _whole_device(ws, _whole_leaves(ws, colors), **kw)
    _same_layout(info, _quats_info(ws, colors, **kw), packed)
    assert not a_g.any()
    assert torch.equal(r_g.detach(), bg[:, None, None, :].expand_as(r_g))
    assert not (info["radii"] > 0).any()
    if packed:
        assert info["gaussian_ids"].numel() == 0 and info["means2d"].shape == (0, 2)
    (r_g.sum() + a_g.sum() + info["means2d"].sum() + info["conics"].sum() + info["depths"].sum()).backward()
    for name, t in zip(("means", "covars", "opacities", "colors"), pg):
        assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any(), name


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_a_call_without_covars_is_the_call_it_was(env, packed, monkeypatch):
    """covars=None passed explicitly against the call without the argument: render, alphas, every info tensor and every
    gradient torch.equal (loss on the projection's outputs; one camera packed: the gather of the opacities per pair sums
    over the cameras with atomics).  And a covars call on the reference's own call pattern -- torch.ones(N, 3), one
    camera, default arguments -- never enters the unit-colour fast path."""
    from edgegaussians_amd import rasterization
    R = env
    ps = CU.packed_scene(False)
    g = torch.Generator().manual_seed(61)
    N = ps["means"].shape[0]
    nc = 1 if packed else 3
    leaves = [ps["means"], ps["quats"], ps["scales"], ps["opacities"], 0.2 + 0.8 * torch.rand(N, 3, generator=g)]
    fixed = dict(viewmats=ps["viewmats"][:nc].cuda(), Ks=ps["Ks"][:nc].cuda(), width=70, height=52,
                 backgrounds=torch.rand(nc, 3, generator=g).cuda(), **CU.PACKED_ARGS)
    w = dict(means2d=torch.randn(nc, N, 2, generator=g).cuda(), depths=torch.randn(nc, N, generator=g).cuda(),
             conics=torch.randn(nc, N, 3, generator=g).cuda(), opacities=torch.randn(nc, N, generator=g).cuda())
    runs = []
    for extra in ({}, {"covars": None}):
        p = [t.clone().cuda().requires_grad_(True) for t in leaves]
        render, alpha, info = rasterization(*p, rasterize_mode="antialiased", packed=packed, **fixed, **extra)
        cam, gid = info["camera_ids"], info["gaussian_ids"]
        pick = (lambda t: t[cam, gid]) if cam is not None else (lambda t: t)
        sum((info[k] * pick(w[k])).sum() for k in w).backward()
        runs.append((render.detach(), alpha.detach(), _tensor_items(info), [t.grad for t in p[:4]]))
    (r0, a0, i0, g0), (r1, a1, i1, g1) = runs
    assert torch.equal(r0, r1) and torch.equal(a0, a1)
    assert set(i0) == set(i1) and len(i0) >= 9
    for k in i0:
        assert torch.equal(i0[k].detach(), i1[k].detach()), k
    for a, b in zip(g0, g1):
        assert a.abs().max() > 0 and torch.equal(a, b)
    # the fast path: taken by the reference's call pattern, never with covars
    entered = []
    real_fast = R._fast_rasterization
    monkeypatch.setattr(R, "_fast_rasterization", lambda *a, **k: (entered.append(1), real_fast(*a, **k))[1])
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    dev = [t.cuda() for t in leaves[:4]]
    ones = torch.ones(N, 3, device="cuda")
    vm1, K1 = ps["viewmats"][:1].cuda(), ps["Ks"][:1].cuda()
    cov = CU.full33(ps["covars"]).cuda()
    with torch.no_grad():
        if not packed:
            _r, _a, i_fast = rasterization(*dev, ones, vm1, K1, 70, 52, packed=False)
            assert entered == [1] and isinstance(i_fast, R._LazyInfo)
        del seen[:]
        r_c, a_c, i_c = rasterization(dev[0], None, None, dev[3], ones, vm1, K1, 70, 52, packed=packed, covars=cov)
    assert len(entered) == (0 if packed else 1), entered
    assert not isinstance(i_c, R._LazyInfo)
    assert "eg_operator_fwd" not in seen and "eg_project_fwd_cams" not in seen and "eg_packed_count" not in seen, seen
    assert ("eg_packed_count_covars" if packed else "eg_project_covars_fwd_cams_flags") in seen, seen
    assert r_c.shape == (1, 52, 70, 3) and float(a_c.mean()) > 0.05
    assert rel_err(r_c.cpu(), a_c.expand(1, 52, 70, 3).cpu()) <= 1e-5   # (unit colours: the image is the alpha)


# ---------------------------------------------------------------------------------------------------
def _single_cotangent_scene():
    """200 Gaussians in a unit box, 70 x 52, two cameras looking down +z from 3 and from 5 units: far_plane = 5 culls
    about half of the rows of the second camera and none of the first."""
    g = torch.Generator().manual_seed(67)
    N = 200
    means = torch.rand(N, 3, generator=g) - 0.5
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=-1)
    scales = 0.03 + 0.05 * torch.rand(N, 3, generator=g)
    w, x, y, z = quats.unbind(-1)
    rot = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                       2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(N, 3, 3)
    covars = rot @ torch.diag_embed(scales ** 2) @ rot.transpose(1, 2)
    covars = 0.5 * (covars + covars.transpose(1, 2))
    vms = torch.eye(4).repeat(2, 1, 1)
    vms[0, 2, 3], vms[1, 2, 3] = 3.0, 5.0
    Ks = torch.tensor([[60.0, 0.0, 35.0], [0.0, 60.0, 26.0], [0.0, 0.0, 1.0]]).repeat(2, 1, 1)
    opac = 0.1 + 0.8 * torch.rand(N, generator=g)
    w8 = dict(means2d=torch.randn(2, N, 2, generator=g), depths=torch.randn(2, N, generator=g),
              conics=torch.randn(2, N, 3, generator=g), comps=torch.randn(2, N, generator=g))
    return dict(means=means, quats=quats, scales=scales, covars=covars, vms=vms, Ks=Ks, opac=opac, w=w8)


SINGLE_NODES = ("_Projection", "_CovarProjection", "_PackedProjection", "_PackedCovarProjection")


@pytest.mark.parametrize("aa", [False, True], ids=list(MODES))
@pytest.mark.parametrize("node", SINGLE_NODES)
def test_single_cotangent_backwards(env, node, aa):
    """Each of the four projection nodes, applied directly: the backward of a loss that touches ONE of means2d, conics,
    depths (and, antialiased, the compensation) against the backward of the same loss plus ``(other * 0).sum()`` for
    every output it does not touch, i.e. a missing cotangent against an explicit zero one: the gradients of means, of
    the shape tensors and of viewmats are torch.equal.  (These kernels use no float atomics -- packed.hip,
    viewmat_grad.hip and functional.hip say so -- and the same call gives the same bits twice.)  Every zero-fill branch of
    the shared cotangent code, dense and packed, with the pose gradient on."""
    R = env
    s = _single_cotangent_scene()
    packed, covar = "Packed" in node, "Covar" in node
    touched = ("means2d", "conics", "depths") + (("comps",) if aa else ())

    def run(name, explicit):
        m = s["means"].cuda().requires_grad_(True)
        shape = [s["covars"].cuda().requires_grad_(True)] if covar else [s["quats"].cuda().requires_grad_(True),
                                                                         s["scales"].cuda().requires_grad_(True)]
        vm = s["vms"].cuda().requires_grad_(True)
        tail = (False, {}) if packed else ()
        out = getattr(R, node).apply(m, *shape, s["opac"].cuda(), vm, s["Ks"].cuda(), 70, 52, 0.3, 0.01, 5.0, 0.0, aa, *tail)
        outs = dict(radii=out[0], means2d=out[1], depths=out[2], conics=out[3], comps=out[4])
        if packed:
            cam, gid = out[8], out[9]
            vis = torch.zeros(2, 200, dtype=torch.bool, device="cuda")
            vis[cam, gid] = True
            pick = lambda t: t.cuda()[cam, gid]
        else:
            vis = outs["radii"] > 0
            pick = lambda t: t.cuda()
        loss = (outs[name] * pick(s["w"][name])).sum()
        if explicit:
            loss = loss + sum((outs[k] * 0).sum() for k in touched if k != name)
        loss.backward()
        return vis, [m.grad, *[t.grad for t in shape], vm.grad]

    for name in touched:
        vis, missing = run(name, False)
        _vis, explicit = run(name, True)
        n_vis = vis.sum(dim=1).tolist()
        assert n_vis[0] == 200 and 40 <= n_vis[1] <= 160, n_vis   # (far_plane culls rows of the second camera alone)
        assert len(missing) == (3 if covar else 4)
        for a, b in zip(missing, explicit):
            assert a is not None and a.shape == b.shape and torch.equal(a, b), (node, name)
        assert missing[0].abs().max() > 0 and missing[-1].abs().max() > 0, (node, name)
        assert not missing[-1][:, 3].any()
