"""The orthographic camera (camera_model="ortho") on the device, against the float64 references of tests/ortho_util.py
(whose conditions tests/test_ortho_host.py asserts with the references alone):

1. / 2. the projection and its VJP per Gaussian, from quats + scales and from covariances (the new entry pair), every
   size, one and three cameras, the defaults and the off-default arguments; 3. row independence of N; 4. packed=True
   against packed=False; 5. the pose gradient; 6. the whole call against the oracle's binning and compositing on the
   reference projection, tile sizes 8 / 16 / 32, both modes; 7. the stages against the whole call, and the fast path
   stepping aside; 8. one case each of RGB+ED with backgrounds, five channels, spherical harmonics; 9. "pinhole" is the
   call without the argument, bit for bit.

The compositing backward accumulates with float atomics (its bits vary from run to run), so wherever two device runs are
compared bit for bit through a backward, the loss is formed on the projection's outputs (info["means2d"], ["depths"],
["conics"], ["opacities"]), whose backward adds in a fixed order -- or on the unit-colour fast path, which has no atomics."""
import pytest
import torch

from tests import ortho_util as OU
from tests import util as U
from tests import viewmat_util as V
from tests.tile_util import BORDER_CAP
from tests.util import assert_close, record, rel_err

pytestmark = pytest.mark.gpu

W, H = U.PROJ_SIZE
MODES = ("classic", "antialiased")


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import rasterizer
    return rasterizer


# ---------------------------------------------------------------------------------------------------
def _device_projection(form, ref, n, cots=None):
    """fully_fused_projection(camera_model="ortho", calc_compensations=True) on the first n rows; one autograd.grad per
    cotangent.  Returns (outs: name -> cpu [C, n, ...], grads: cotangent -> {input name: cpu [n, k]})."""
    import gsplat
    a = ref["args"]
    p = [t[:n].cuda().requires_grad_(True) for t in ref["inputs"]]
    kw = dict(eps2d=a["eps2d"], near_plane=a["near_plane"], far_plane=a["far_plane"], radius_clip=a["radius_clip"],
              calc_compensations=True, camera_model="ortho")
    vms, Ks = ref["viewmats"].cuda(), ref["Ks"].cuda()
    if form == "quats":
        out = gsplat.fully_fused_projection(p[0], None, p[1], p[2], vms, Ks, W, H, **kw)
    else:
        out = gsplat.fully_fused_projection(p[0], p[1], None, None, vms, Ks, W, H, **kw)
    outs = dict(zip(("radii",) + U.PROJ_OUTPUTS, out))
    grads = {}
    for name, cot in (ref["cots"] if cots is None else cots).items():
        y = outs[name]
        g = torch.autograd.grad(y, p, cot[:, :n].cuda().reshape(y.shape).contiguous(), retain_graph=True)
        grads[name] = {k: gi.cpu() for k, gi in zip(ref["names"], g)}
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in outs.items()}, grads


def _check_projection(form, args_name, n_cams, n):
    ref = OU.reference(form, args_name, n_cams)
    outs, grads = _device_projection(form, ref, n)
    C = n_cams
    label = f"ortho {form} {args_name} C={C} n={n}"
    r, r64, border = outs["radii"].numpy(), ref["outs"]["radii"].numpy()[:, :n], ref["border"][:, :n]
    assert outs["radii"].dtype == torch.int32 and r.shape == (C, n)
    if n == OU.N_FULL:
        assert border.mean(axis=1).max() <= 0.02, border.mean(axis=1)
    differ = r != r64
    assert not (differ & ~border).any(), f"{label}: {int((differ & ~border).sum())} radii / culls differ outside the borderline set"
    culled = r == 0
    for name in U.PROJ_OUTPUTS:
        assert (outs[name].numpy()[culled] == 0).all(), f"{label}: {name} is not zero on a culled row"
    rows_ok = ((r > 0) == (r64 > 0)).all(axis=0)
    vis = ref["vis"][:, :n]
    fwd = {}
    for name in U.PROJ_OUTPUTS:
        fwd[name] = max(U.fwd_row_err(outs[name][c], ref["outs"][name][c, :n], vis[c] & rows_ok) for c in range(C))
        print(f"{label} fwd {name}: {fwd[name]:.3e}")
    cells = {}
    never = torch.from_numpy(~(r > 0).any(axis=0))
    for cot in ref["cots"]:
        rows = rows_ok & ref["comp_rows"][:n] if cot == "compensations" else rows_ok
        for g in ref["names"]:
            ratio, _loose, nonzero, over = U.row_bound_ratio(grads[cot][g], ref["grads"][cot][g][:n], ref["kappa"][cot][g][:n], rows)
            cells[f"{cot}->{g}"] = ratio
            print(f"{label} {cot}->{g}: {ratio:.3f} of the bound, {over} rows over, {nonzero} rows not exactly zero")
            assert not grads[cot][g][never].any(), f"{label}: v_{g} is not zero on a row no camera keeps"
    record("ortho_projection_vjp_per_row", form=form, args=args_name, cameras=C, gaussians=n, ratio_to_bound=cells,
           fwd_row_err=fwd, decision_mismatches_inside=int(differ.sum()))
    for name in U.PROJ_OUTPUTS:
        assert fwd[name] <= U.FWD_ROW_TOL, (label, name, fwd[name])
    for cot in ref["cots"]:
        rows = rows_ok & ref["comp_rows"][:n] if cot == "compensations" else rows_ok
        for g in ref["names"]:
            U.row_bound_check(grads[cot][g], ref["grads"][cot][g][:n], ref["kappa"][cot][g][:n], f"{label} {cot}->v_{g}", rows)
    return outs, grads


@pytest.mark.parametrize("n", OU.SIZES)
@pytest.mark.parametrize("args_name,n_cams", OU.CASES)
def test_projection_from_quats_and_scales(env, args_name, n_cams, n):
    """eg_project_fwd_cams / eg_project_bwd_cams with EG_FLAG_ORTHO: forward outputs per row to U.FWD_ROW_TOL, the VJP of
    one N(0,1) cotangent per output to means, quats and scales per row to U.row_bound_check, radii equal outside the
    borderline set, exact zeros on culled rows; three cameras: camera 0 writes, the others add."""
    _check_projection("quats", args_name, n_cams, n)


@pytest.mark.parametrize("n", OU.SIZES)
@pytest.mark.parametrize("args_name,n_cams", OU.CASES)
def test_projection_from_covariances(env, args_name, n_cams, n):
    """The same through eg_project_covars_{fwd,bwd}_cams_flags, for the gradients of means and covars."""
    _check_projection("covars", args_name, n_cams, n)


def test_classic_mode_has_no_compensation_gradient(env):
    """Without calc_compensations the projection node runs without EG_FLAG_ANTIALIASED: the outputs are the same bits
    and the compensation plays no part."""
    import gsplat
    ref = OU.reference("quats", "eps1", 3)
    a = ref["args"]
    p = [t.cuda() for t in ref["inputs"]]
    kw = dict(eps2d=a["eps2d"], near_plane=a["near_plane"], far_plane=a["far_plane"], radius_clip=a["radius_clip"], camera_model="ortho")
    vms, Ks = ref["viewmats"].cuda(), ref["Ks"].cuda()
    plain = gsplat.fully_fused_projection(p[0], None, p[1], p[2], vms, Ks, W, H, **kw)
    comp = gsplat.fully_fused_projection(p[0], None, p[1], p[2], vms, Ks, W, H, calc_compensations=True, **kw)
    assert plain[4] is None and comp[4] is not None
    for x, y in zip(plain[:4], comp[:4]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("form", list(OU.FORMS))
def test_rows_do_not_depend_on_n(env, form):
    """One Gaussian per lane, contraction off: the first rows of the N = 1000 call equal the N = 1, 65, 257 calls bit
    for bit, in every output and gradient, for every camera of a three-camera call."""
    ref = OU.reference(form, "eps1", 3)
    full_outs, full_grads = _device_projection(form, ref, OU.N_FULL)
    assert (full_outs["radii"] > 0).sum() >= 500
    for n in OU.SIZES[:-1]:
        outs, grads = _device_projection(form, ref, n)
        for name, t in outs.items():
            assert torch.equal(t, full_outs[name][:, :n]), (n, name)
        for cot in grads:
            for g in ref["names"]:
                assert torch.equal(grads[cot][g], full_grads[cot][g][:n]), (n, cot, g)


# ---------------------------------------------------------------------------------------------------
def _packed_scene(ortho=True):
    """500 Gaussians, 3 cameras, 70 x 52, orthographic intrinsics (or the scene's own, for the pinhole); near_plane 3.7 and
    radius_clip 3.5 keep about 70 % of the pairs under either model"""
    from edgegaussians_amd import synth
    sc = synth.make_scene(500, 3, 70, 52, seed=3, spread_opacity=True, scale=0.02, anisotropy=5.0)
    centre = sc.means.double().mean(0)
    Ks = sc.Ks.clone()
    for c in range(3 if ortho else 0):
        Ks[c] = OU.ortho_intrinsics(sc.Ks[c], float((sc.viewmats[c].double()[:3, :3] @ centre + sc.viewmats[c].double()[:3, 3])[2]))
    g = torch.Generator().manual_seed(41)
    N = sc.means.shape[0]
    leaves = [sc.means, sc.quats, torch.exp(sc.log_scales), torch.sigmoid(sc.logit_opacities).squeeze(-1),
              0.2 + 0.8 * torch.rand(N, 3, generator=g)]
    fixed = dict(viewmats=sc.viewmats.contiguous().cuda(), Ks=Ks.contiguous().cuda(), width=70, height=52,
                 backgrounds=torch.rand(3, 3, generator=g).cuda(), near_plane=3.7, radius_clip=3.5)
    w = dict(render=torch.rand(3, 52, 70, 3, generator=g).cuda(), alpha=torch.rand(3, 52, 70, 1, generator=g).cuda(),
             means2d=torch.randn(3, N, 2, generator=g).cuda(), depths=torch.randn(3, N, generator=g).cuda(),
             conics=torch.randn(3, N, 3, generator=g).cuda(), opacities=torch.randn(3, N, generator=g).cuda())
    return leaves, fixed, w, N


def _packed_run(leaves, fixed, w, mode, loss_kind, **kw):
    from edgegaussians_amd import rasterization
    p = [t.clone().cuda().requires_grad_(True) for t in leaves]
    render, alpha, info = rasterization(p[0], p[1], p[2], p[3], p[4], rasterize_mode=mode, camera_model="ortho", **fixed, **kw)
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
def test_packed_equals_the_dense_call(env, mode):
    """packed=True under ortho: the id lists are the set radii > 0 of the packed=False call in ascending order, every
    per-pair info tensor is the dense one at [camera_ids, gaussian_ids] bit for bit, render and alphas are torch.equal;
    dense gradients of an image loss agree to 1e-4 (the compositing backward adds with atomics); with sparse_grad the
    gradients of a loss on the projection's outputs equal the dense ones after to_dense() (to 1e-6: a three-camera sum
    in another order) and their indices are gaussian_ids.  near_plane 3.7 and radius_clip 3.5 cull a part of the pairs."""
    leaves, fixed, w, N = _packed_scene()
    rd, ad, di, gd = _packed_run(leaves, fixed, w, mode, "image", packed=False)
    rp, ap, pi, gp = _packed_run(leaves, fixed, w, mode, "image", packed=True)
    cam, gid = pi["camera_ids"], pi["gaussian_ids"]
    vis = di["radii"] > 0
    share = vis.float().mean(dim=1).tolist()
    print("visible share per camera:", share)
    assert 0.1 <= min(share) and max(share) <= 0.95, share
    assert torch.equal(cam * N + gid, torch.nonzero(vis.reshape(-1))[:, 0])
    for k in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss"):
        assert torch.equal(pi[k].detach(), di[k].detach()[cam, gid]), k
    assert torch.equal(rp, rd) and torch.equal(ap, ad)
    assert float(ad.mean()) > 0.05
    for name, a, b in zip(("means", "quats", "scales", "opacities", "colors"), gp, gd):
        assert_close(a.cpu(), b.cpu(), name=f"packed grad {name}")
    _r, _a, _i, g_dense = _packed_run(leaves, fixed, w, mode, "projection", packed=True)
    _r, _a, si, g_sparse = _packed_run(leaves, fixed, w, mode, "projection", packed=True, sparse_grad=True)
    for name, a, b in zip(("means", "quats", "scales"), g_sparse, g_dense):
        assert a.is_sparse and torch.equal(a._indices()[0], si["gaussian_ids"]), name
        assert b.abs().max() > 0
        assert_close(a.to_dense().cpu(), b.cpu(), rtol=1e-6, name=f"sparse grad {name}")
    assert_close(g_sparse[3].cpu(), g_dense[3].cpu(), rtol=1e-6, name="opacities")   # (a gather's backward: atomics over the cameras)


# ---------------------------------------------------------------------------------------------------
def _pose_run(R, ref, packed, with_pose, cots):
    a = ref["args"]
    n = OU.N_FULL
    C = ref["vis"].shape[0]
    p = [t.cuda().requires_grad_(True) for t in ref["inputs"]]
    vm = ref["viewmats"].clone().cuda().requires_grad_(with_pose)
    common = (p[0], p[1], p[2], torch.full((n,), 0.5, device="cuda"), vm, ref["Ks"].cuda(), W, H, float(a["eps2d"]),
              float(a["near_plane"]), float(a["far_plane"]), float(a["radius_clip"]), True)
    vis = torch.zeros(C, n, dtype=torch.bool, device="cuda")
    if packed:
        out = R._PackedProjection.apply(*common, False, {}, R.TILE, True)
        cam, gid = out[8], out[9]
        vis[cam, gid] = True
    else:
        out = R._Projection.apply(*common, R.TILE, True)
        cam = gid = None
        vis = out[0] > 0
    return dict(p=p, vm=vm, outs=dict(zip(U.PROJ_OUTPUTS, out[1:5])), vis=vis.cpu(), cam=cam, gid=gid)


def _pose_cots(run, cots, keep):
    ys, cts = [], []
    for name, cot in cots.items():
        y = run["outs"][name]
        ct = cot.cuda() * keep.cuda()[..., None]
        if run["cam"] is not None:
            ct = ct[run["cam"], run["gid"]]
        ys.append(y)
        cts.append(ct.reshape(y.shape).contiguous())
    return ys, cts


@pytest.mark.parametrize("packed", [False, True])
def test_pose_gradient(env, packed):
    """viewmats.grad under ortho (eg_project_bwd_viewmats with EG_FLAG_ORTHO, both layouts) against the float64 autograd
    of the reference, entry by entry: |got - ref64| <= TAU_SMALL * S with S the sum of the pairs' absolute contributions
    (tests/viewmat_util.py: the bound for any number of pairs), an exactly zero bottom row; asking for it leaves the
    gradients of means, quats and scales bit for bit what they are without it."""
    R = env
    ref = OU.reference("quats", "eps1", 3)
    G, bottom = OU.pose_reference("eps1", 3)
    assert bottom == 0.0
    run = _pose_run(R, ref, packed, True, ref["cots"])
    keep = run["vis"] == torch.from_numpy(ref["vis"])
    drop = ~keep
    assert not (drop.numpy() & ~ref["border"]).any(), "a cull decision differs outside the borderline set"
    assert run["vis"].sum(dim=1).min() >= 200
    ys, cts = _pose_cots(run, ref["cots"], keep)
    ratios = {}
    for name, y, ct in zip(ref["cots"], ys, cts):
        g = torch.autograd.grad(y, run["vm"], ct, retain_graph=True)[0].cpu()
        gk = G[name] * keep[:, :, None, None]
        ratios[name] = V.bound_ratio(g, gk.sum(1), gk.abs().sum(1))[0]
        print(f"ortho pose {'packed' if packed else 'dense'} {name}: |got - ref64| / S = {ratios[name]:.3e} "
              f"({ratios[name] / V.TAU_SMALL:.3f} of the bound)")
    record("ortho_viewmat_grad_per_entry", packed=packed, ratio_to_S=ratios, tau=V.TAU_SMALL, dropped_pairs=int(drop.sum()))
    for name, y, ct in zip(ref["cots"], ys, cts):
        g = torch.autograd.grad(y, run["vm"], ct, retain_graph=True)[0].cpu()
        gk = G[name] * keep[:, :, None, None]
        V.check(g, gk.sum(1), gk.abs().sum(1), f"ortho pose {name}", V.TAU_SMALL)
    with_pose = torch.autograd.grad(ys, run["p"] + [run["vm"]], cts)
    plain = _pose_run(R, ref, packed, False, ref["cots"])
    ys0, cts0 = _pose_cots(plain, ref["cots"], keep)
    without = torch.autograd.grad(ys0, plain["p"], cts0)
    for name, a, b in zip(ref["names"], with_pose, without):
        assert torch.equal(a, b), name
    assert not with_pose[3][:, 3].any()


# ---------------------------------------------------------------------------------------------------
def _whole_inputs():
    ws = OU.whole_scene()
    g = torch.Generator().manual_seed(29)
    N = ws["means"].shape[0]
    C = len(OU.WHOLE_CAMS)
    colors = 0.2 + 0.8 * torch.rand(N, 3, generator=g)
    wr = torch.rand(C, ws["H"], ws["W"], 3, generator=g)
    wa = torch.rand(C, ws["H"], ws["W"], 1, generator=g)
    return ws, colors, wr, wa


def _whole_device(ws, leaves, Ks, **kw):
    from edgegaussians_amd import rasterization
    p = [t.clone().cuda().requires_grad_(True) for t in leaves]
    render, alpha, info = rasterization(p[0], p[1], p[2], p[3], p[4], ws["viewmats"].cuda(), Ks.cuda(), ws["W"], ws["H"],
                                        packed=False, **kw)
    return p, render, alpha, info


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ts", OU.TILE_SIZES)
def test_whole_call_against_the_oracle(env, ts, mode):
    """rasterization(camera_model="ortho", packed=False, tile_size=ts) on two cameras with [N, 3] colours against
    ref_project_ortho -> oracle isect_tiles -> isect_offset_encode -> composite in fp32 on the CPU and its autograd
    gradients of a random-cotangent loss, to 1e-4 outside the float-borderline pixels (at most BORDER_CAP of them); no
    Gaussian of the synth scene had to be removed for an integer-borderline decision beyond the cap of the tile tests."""
    ws, colors, wr, wa = _whole_inputs()
    aa = mode == "antialiased"
    keep = OU.whole_keep(ts, aa)
    assert (~keep).float().mean() <= BORDER_CAP
    assert ws["removed"] <= max(3, 0.016 * ws["n0"])
    leaves = [ws["means"], ws["quats"], ws["scales"], ws["opacities"], colors]
    pc = [t.clone().requires_grad_(True) for t in leaves]
    r_c, a_c, projs = OU.oracle_whole(pc, lambda c, pr: pc[4], ts, aa)
    ((r_c * wr * keep[..., None]).sum() + (a_c * wa * keep[..., None]).sum()).backward()
    pg, r_g, a_g, info = _whole_device(ws, leaves, ws["Ks_o"], tile_size=ts, rasterize_mode=mode, camera_model="ortho")
    kg = keep.cuda()[..., None]
    ((r_g * wr.cuda() * kg).sum() + (a_g * wa.cuda() * kg).sum()).backward()
    assert torch.equal(info["radii"].cpu(), torch.stack([pr[0] for pr in projs]))
    assert info["tile_size"] == ts
    assert float(a_g.detach().mean()) > 0.05
    e = {"render": rel_err(r_g.detach().cpu()[keep], r_c.detach()[keep]), "alpha": rel_err(a_g.detach().cpu()[keep], a_c.detach()[keep])}
    names = ("means", "quats", "scales", "opacities", "colors")
    for name, a, b in zip(names, pg, pc):
        e[name] = rel_err(a.grad.cpu(), b.grad)
    record("ortho_whole_call", tile_size=ts, mode=mode, gaussians=int(leaves[0].shape[0]), borderline_pixels=int((~keep).sum()),
           max_rel_err=e)
    print(f"ortho whole call ts={ts} {mode}: {e}")
    assert_close(r_g.detach().cpu()[keep], r_c.detach()[keep], name="render")
    assert_close(a_g.detach().cpu()[keep], a_c.detach()[keep], name="alpha")
    for name, a, b in zip(names, pg, pc):
        assert_close(a.grad.cpu(), b.grad, name=f"grad {name}")
    # the switch reaches the kernels: the pinhole image of the same scene (its own intrinsics) is another image
    with torch.no_grad():
        r_p = _whole_device(ws, leaves, ws["Ks"], tile_size=ts, rasterize_mode=mode)[1]
        r_same = _whole_device(ws, leaves, ws["Ks_o"], tile_size=ts, rasterize_mode=mode)[1]
    assert rel_err(r_g.detach().cpu(), r_p.cpu()) > 0.1
    assert rel_err(r_g.detach().cpu(), r_same.cpu()) > 0.1   # ... and so is the pinhole image under the ortho intrinsics


# ---------------------------------------------------------------------------------------------------
def test_stages_reproduce_the_whole_call_and_the_fast_path_steps_aside(env, monkeypatch):
    """fully_fused_projection(camera_model="ortho") -> isect_tiles -> isect_offset_encode -> rasterize_to_pixels is
    rasterization(packed=False, camera_model="ortho"), torch.equal in classic mode.  Then the reference's own call
    pattern -- torch.ones(N, 3), one camera, default arguments -- under ortho: it runs the general path's entries (never
    eg_operator_fwd) and gives the general path's result and info keys."""
    import gsplat
    R = env
    ws, colors, _wr, _wa = _whole_inputs()
    dev = [t.cuda() for t in (ws["means"], ws["quats"], ws["scales"], ws["opacities"], colors)]
    vms, Ks = ws["viewmats"].cuda(), ws["Ks_o"].cuda()
    Wd, Hd = ws["W"], ws["H"]
    C, N = vms.shape[0], dev[0].shape[0]
    with torch.no_grad():
        render, alpha, info = gsplat.rasterization(*dev, vms, Ks, Wd, Hd, packed=False, camera_model="ortho")
        radii, means2d, depths, conics, comps = gsplat.fully_fused_projection(dev[0], None, dev[1], dev[2], vms, Ks, Wd, Hd,
                                                                              camera_model="ortho")
        assert comps is None
        for k, t in (("radii", radii), ("means2d", means2d), ("depths", depths), ("conics", conics)):
            assert torch.equal(t, info[k]), k
        tw, th = info["tile_width"], info["tile_height"]
        tpg, isect_ids, flatten_ids = gsplat.isect_tiles(means2d, radii, depths, 16, tw, th)
        offsets = gsplat.isect_offset_encode(isect_ids, C, tw, th)
        assert torch.equal(tpg, info["tiles_per_gauss"]) and torch.equal(isect_ids, info["isect_ids"])
        assert torch.equal(flatten_ids, info["flatten_ids"]) and torch.equal(offsets, info["isect_offsets"])
        r2, a2 = gsplat.rasterize_to_pixels(means2d, conics, dev[4][None].expand(C, N, 3).contiguous(),
                                            dev[3][None].expand(C, N).contiguous(), Wd, Hd, 16, offsets, flatten_ids)
        assert torch.equal(r2, render) and torch.equal(a2, alpha)
        assert float(alpha.mean()) > 0.05
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    ones = torch.ones(N, 3, device="cuda")
    with torch.no_grad():
        r1, a1, i1 = gsplat.rasterization(dev[0], dev[1], dev[2], dev[3], ones, vms[:1], Ks[:1], Wd, Hd, packed=False,
                                          camera_model="ortho")
    assert "eg_operator_fwd" not in seen and seen.count("eg_project_fwd_cams") == 1, seen
    assert not isinstance(i1, R._LazyInfo)
    assert set(i1.keys()) == set(info.keys())
    assert torch.equal(i1["radii"], info["radii"][:1]) and torch.equal(i1["means2d"], info["means2d"][:1])
    # (unit colours take the general path's order-independent kernels: another fp32 summation of the same terms, a few
    # dozen per pixel, each good to ~1e-7)
    assert rel_err(a1.cpu(), alpha[:1].cpu()) <= 1e-5
    assert r1.shape == (1, Hd, Wd, 3) and rel_err(r1.cpu(), a1.expand(1, Hd, Wd, 3).cpu()) <= 1e-5   # the image is the alpha


# ---------------------------------------------------------------------------------------------------
def test_rider_depth_mode_with_backgrounds(env):
    """render_mode="RGB+ED" with backgrounds under ortho: the oracle composite of the reference projection with the
    depth as a fourth colour; colours + (1 - alpha) background, depth / alpha."""
    ws, colors, wr, wa = _whole_inputs()
    keep = OU.whole_keep(16, False)
    g = torch.Generator().manual_seed(43)
    bg = torch.rand(len(OU.WHOLE_CAMS), 3, generator=g)
    wd = torch.rand(len(OU.WHOLE_CAMS), ws["H"], ws["W"], 1, generator=g)
    leaves = [ws["means"], ws["quats"], ws["scales"], ws["opacities"], colors]
    pc = [t.clone().requires_grad_(True) for t in leaves]
    r4, a_c, _ = OU.oracle_whole(pc, lambda c, pr: torch.cat([pc[4], pr[2][:, None]], dim=-1), 16, False)
    r_c = torch.cat([r4[..., :3] + (1.0 - a_c) * bg[:, None, None, :], r4[..., 3:] / a_c.clamp(min=1e-10)], dim=-1)
    seen = keep & (a_c.detach()[..., 0] > 0.05)   # (the expected depth divides by alpha)
    wfull = torch.cat([wr, wd], dim=-1) * seen[..., None]
    (r_c * wfull).sum().backward()
    pg, r_g, a_g, _info = _whole_device(ws, leaves, ws["Ks_o"], render_mode="RGB+ED", backgrounds=bg.cuda(), camera_model="ortho")
    (r_g * wfull.cuda()).sum().backward()
    assert r_g.shape[-1] == 4
    assert_close(r_g.detach().cpu()[seen], r_c.detach()[seen], name="RGB+ED render")
    assert_close(a_g.detach().cpu()[keep], a_c.detach()[keep], name="alpha")
    for name, a, b in zip(("means", "quats", "scales", "opacities", "colors"), pg, pc):
        assert_close(a.grad.cpu(), b.grad, name=f"RGB+ED grad {name}")


def test_rider_five_channels(env):
    """D = 5 under ortho (the wide entries of csrc/tiles.hip behind the orthographic projection) against the oracle composite."""
    ws, _colors, _wr, wa = _whole_inputs()
    keep = OU.whole_keep(16, True)
    g = torch.Generator().manual_seed(47)
    N = ws["means"].shape[0]
    colors = torch.rand(N, 5, generator=g)
    w5 = torch.rand(len(OU.WHOLE_CAMS), ws["H"], ws["W"], 5, generator=g) * keep[..., None]
    leaves = [ws["means"], ws["quats"], ws["scales"], ws["opacities"], colors]
    pc = [t.clone().requires_grad_(True) for t in leaves]
    r_c, a_c, _ = OU.oracle_whole(pc, lambda c, pr: pc[4], 16, True)
    (r_c * w5).sum().backward()
    pg, r_g, a_g, _info = _whole_device(ws, leaves, ws["Ks_o"], rasterize_mode="antialiased", camera_model="ortho")
    (r_g * w5.cuda()).sum().backward()
    assert r_g.shape[-1] == 5
    assert_close(r_g.detach().cpu()[keep], r_c.detach()[keep], name="D=5 render")
    assert_close(a_g.detach().cpu()[keep], a_c.detach()[keep], name="D=5 alpha")
    for name, a, b in zip(("means", "quats", "scales", "opacities", "colors"), pg, pc):
        assert_close(a.grad.cpu(), b.grad, name=f"D=5 grad {name}")


@pytest.mark.parametrize("packed", [False, True])
def test_rider_spherical_harmonics(env, packed):
    """sh_degree = 2 under ortho: the colours are spherical_harmonics on means - campos (the directions of every camera
    model), clamp_min(. + 0.5, 0) -- the unpacked call with those colours [C, N, 3] gives the same alphas bit for bit and
    the same image to 1e-6 (the same compositing kernel on colours evaluated by the same arithmetic); the packed call goes
    through another compositing kernel: fp32 sums of at most a few dozen terms, each good to ~1e-7, agree to 1e-5."""
    import gsplat
    ws, _colors, _wr, _wa = _whole_inputs()
    g = torch.Generator().manual_seed(53)
    N = ws["means"].shape[0]
    coeffs = (torch.randn(N, 9, 3, generator=g) * 0.3).cuda()
    dev = [t.cuda() for t in (ws["means"], ws["quats"], ws["scales"], ws["opacities"])]
    vms, Ks = ws["viewmats"].cuda(), ws["Ks_o"].cuda()
    with torch.no_grad():
        r_sh, a_sh, info = gsplat.rasterization(*dev, coeffs, vms, Ks, ws["W"], ws["H"], sh_degree=2, packed=packed,
                                                camera_model="ortho")
        campos = torch.linalg.inv(vms)[:, :3, 3]
        dirs = dev[0][None] - campos[:, None]
        cols = torch.clamp_min(gsplat.spherical_harmonics(2, dirs, coeffs[None].expand(vms.shape[0], N, 9, 3)) + 0.5, 0.0)
        r_dense, a_dense, dinfo = gsplat.rasterization(*dev, cols.contiguous(), vms, Ks, ws["W"], ws["H"], packed=False,
                                                       camera_model="ortho")
    if packed:
        assert rel_err(a_sh.cpu(), a_dense.cpu()) <= 1e-5 and rel_err(r_sh.cpu(), r_dense.cpu()) <= 1e-5
    else:
        assert torch.equal(a_sh, a_dense)
        assert rel_err(r_sh.cpu(), r_dense.cpu()) <= 1e-6
    assert float(a_sh.mean()) > 0.05 and r_sh.shape[-1] == 3


# ---------------------------------------------------------------------------------------------------
def _tensor_items(info):
    return {k: v for k, v in info.items() if isinstance(v, torch.Tensor)}


@pytest.mark.parametrize("packed", [False, True])
def test_pinhole_is_the_call_without_the_argument(env, packed):
    """camera_model="pinhole" against the call without the argument: render, alphas, every info tensor and every
    gradient torch.equal, with backgrounds and culls (loss on the projection's outputs: see the module docstring; three
    cameras unpacked, one camera packed -- the gather of the opacities per pair sums over the cameras with atomics in its
    backward) and, unpacked, on the reference's own call pattern (unit colours, one camera: the fast path, whose backward has no
    atomics) with a loss on the image."""
    from edgegaussians_amd import rasterization
    leaves, fixed, w, N = _packed_scene(ortho=False)
    if packed:
        fixed = {k: (v[:1].contiguous() if isinstance(v, torch.Tensor) else v) for k, v in fixed.items()}
        w = {k: v[:1].contiguous() for k, v in w.items()}
    runs = []
    for extra in ({}, {"camera_model": "pinhole"}):
        p = [t.clone().cuda().requires_grad_(True) for t in leaves]
        render, alpha, info = rasterization(p[0], p[1], p[2], p[3], p[4], rasterize_mode="antialiased", packed=packed, **fixed, **extra)
        cam, gid = info["camera_ids"], info["gaussian_ids"]
        pick = (lambda t: t[cam, gid]) if cam is not None else (lambda t: t)
        sum((info[k] * pick(w[k])).sum() for k in ("means2d", "depths", "conics", "opacities")).backward()
        runs.append((render.detach(), alpha.detach(), _tensor_items(info), [t.grad for t in p[:4]]))
    (r0, a0, i0, g0), (r1, a1, i1, g1) = runs
    assert torch.equal(r0, r1) and torch.equal(a0, a1)
    assert set(i0) == set(i1) and len(i0) >= 9
    for k in i0:
        assert torch.equal(i0[k].detach(), i1[k].detach()), k
    for a, b in zip(g0, g1):
        assert a.abs().max() > 0 and torch.equal(a, b)
    if packed:
        return
    runs = []
    ones = torch.ones(N, 3, device="cuda")
    for extra in ({}, {"camera_model": "pinhole"}):
        p = [t.clone().cuda().requires_grad_(True) for t in leaves[:4]]
        render, alpha, info = rasterization(p[0], p[1], p[2], p[3], ones, fixed["viewmats"][:1], fixed["Ks"][:1], 70, 52,
                                            packed=False, absgrad=True, **extra)
        assert isinstance(info, env._LazyInfo)   # the fast path, with and without the argument
        info["means2d"].retain_grad()
        (render * w["render"][:1]).sum().backward()
        runs.append((render.detach(), alpha.detach(), info["radii"], info["means2d"].detach(), info["means2d"].absgrad,
                     [t.grad for t in p]))
    for x, y in zip(runs[0][:5], runs[1][:5]):
        assert torch.equal(x, y)
    for a, b in zip(runs[0][5], runs[1][5]):
        assert a.abs().max() > 0 and torch.equal(a, b)
