"""Camera-pose gradients of `rasterization` (csrc/viewmat_grad.hip, eg_project_bwd_viewmats; the pose branches of
edgegaussians_amd/rasterizer.py and sh.py):

1. the dense projection's v_viewmats, one output's cotangent at a time, entry by entry against float64
   (tests.viewmat_util: |got - ref64| <= TAU * S with S the sum of the pairs' absolute contributions -- TAU_SMALL on
   a part of a scene -- exact zeros where no pair contributes, bottom row exactly zero); 2. ragged sizes; 3. the
   packed projection, sparse_grad off and on;
4. no visible pair; 5. run-to-run determinism; 6. the whole call against the CPU oracle's autograd, the other gradients
   bit for bit those of the call without a pose gradient; 7. the whole call's projection share isolated from the
   compositing; 8. the unit-colour fast path steps aside; 9. the view directions of sh_degree.

A pair whose cull decision differs between the device and float64 (inside the quantified borderline set of
tests.util.projection_reference) has no reference: its cotangent rows are zeroed on the device and it is left out of
the float64 sum."""
import numpy as np
import pytest
import torch

from tests import sh_oracle
from tests import util as U
from tests import viewmat_util as V
from tests.util import assert_close, borderline_pixel_mask, clean_scene, record, rel_err

pytestmark = pytest.mark.gpu

W, H = U.PROJ_SIZE
MODES = ("classic", "antialiased")
FAR_IN_FRONT = dict(near_plane=0.01, far_plane=0.5, radius_clip=0.0, eps2d=0.3)   # the scenes start at depth 3


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import rasterizer
    return rasterizer


def _away(viewmat):
    """The same camera turned half a turn about its own y axis: everything it saw is now behind it."""
    return torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0])) @ viewmat


def _cotangents(ref, mode):
    """The case's own cotangents; in classic mode a compensation cotangent on top (it must reach nothing)."""
    cots = dict(ref["cots"])
    if mode == "classic" and "compensations" not in cots:
        C, N = ref["vis"].shape
        cots["compensations"] = torch.randn(C, N, 1, generator=torch.Generator().manual_seed(19))
    return cots


def _project(R, ref, mode, n, packed=False, sparse=False, viewmats=None, args=None):
    """_Projection.apply / _PackedProjection.apply on the first n rows with viewmats that require grad."""
    a = ref["spec"]["args"] if args is None else args
    C = ref["vis"].shape[0]
    p = [ref[k][:n].cuda().requires_grad_(True) for k in ("means", "quats", "scales")]
    vm = (ref["viewmats"] if viewmats is None else viewmats).clone().cuda().requires_grad_(True)
    common = (p[0], p[1], p[2], torch.full((n,), 0.5, device="cuda"), vm, ref["Ks"].cuda(), W, H, float(a["eps2d"]),
              float(a["near_plane"]), float(a["far_plane"]), float(a["radius_clip"]), mode == "antialiased")
    vis = torch.zeros(C, n, dtype=torch.bool, device="cuda")
    if packed:
        out = R._PackedProjection.apply(*common, sparse, {})
        cam, gid = out[8], out[9]
        vis[cam, gid] = True
    else:
        out = R._Projection.apply(*common)
        cam = gid = None
        vis = out[0] > 0
    return dict(vm=vm, outs=dict(zip(U.PROJ_OUTPUTS, out[1:5])), vis=vis.cpu(), cam=cam, gid=gid, n=n)


def _viewmat_grads(run, cots, keep=None, at_once=False):
    """viewmats.grad per cotangent (or of their sum): cpu [C, 4, 4].  The cotangent rows of the pairs outside `keep`
    (bool [C, n]) are zeroed; on packed outputs the cotangents are gathered at the visible pairs."""
    n, cam, gid = run["n"], run["cam"], run["gid"]
    ys, cts = [], []
    for name, cot in cots.items():
        y = run["outs"][name]
        ct = cot[:, :n].cuda()
        if keep is not None:
            ct = ct * keep.cuda()[..., None]
        if cam is not None:
            ct = ct[cam, gid]
        ys.append(y)
        cts.append(ct.reshape(y.shape).contiguous())
    if at_once:
        return torch.autograd.grad(ys, run["vm"], cts, retain_graph=True)[0].cpu()
    return {name: torch.autograd.grad(y, run["vm"], ct, retain_graph=True)[0].cpu() for name, y, ct in zip(cots, ys, cts)}


def _check_case(R, case, mode, n=None, packed=False, sparse=False):
    ref = U.projection_reference(case)
    n = ref["means"].shape[0] if n is None else n
    run = _project(R, ref, mode, n, packed, sparse)
    keep = run["vis"] == torch.from_numpy(ref["vis"][:, :n])
    drop = ~keep
    assert not (drop.numpy() & ~ref["border"][:, :n]).any(), "a cull decision differs outside the borderline set"
    cots = _cotangents(ref, mode)
    grads = _viewmat_grads(run, cots, keep)
    label = f"{'packed' if packed else 'dense'}{' sparse' if sparse else ''} {case} {mode} n={n}"
    refs, ratios, tau = {}, {}, V.tau_for(case, n)
    for cot, g in grads.items():
        refs[cot] = V.reference(case, cot, n, drop=drop, mode=mode)
        ratios[cot] = V.bound_ratio(g, *refs[cot])[0]
        print(f"{label} {cot}: |got - ref64| / S = {ratios[cot]:.3e} ({ratios[cot] / tau:.3f} of the bound)")
    record("viewmat_grad_per_entry", case=case, mode=mode, n=n, packed=packed, sparse_grad=sparse, ratio_to_S=ratios,
           tau=tau, dropped_pairs=int(drop.sum()), visible_pairs=int(run["vis"].sum()))
    for cot, g in grads.items():
        if cot == "compensations" and mode == "classic":
            assert tuple(g.shape) == (ref["vis"].shape[0], 4, 4) and not g.any(), f"{label}: the compensation cotangent reached v_viewmats"
        V.check(g, *refs[cot], f"{label} {cot}", tau)
    return grads


# ---- 1. dense, projection level ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", V.CASES)
def test_dense_projection(env, case, mode):
    grads = _check_case(env, case, mode)
    live = [c for c in grads if not (c == "compensations" and mode == "classic")]
    assert all(float(grads[c].abs().max()) > 0 for c in live)


# ---- 2. ragged sizes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", V.RAGGED_N + (None,))
def test_ragged_sizes(env, n):
    """1 lane, less than a wave, one workgroup + one lane, a ragged fourth workgroup, twelve workgroups: the fold sees
    1, 1, 2, 4 and 12 partials per camera."""
    _check_case(env, V.RAGGED_CASE, "antialiased", n)


# ---- 3. packed --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_packed_projection(env, mode, sparse):
    grads = _check_case(env, V.RAGGED_CASE, mode, packed=True, sparse=sparse)
    assert float(grads["conics"].abs().max()) > 0


@pytest.mark.parametrize("n", [1, 257])
def test_packed_ragged(env, n):
    _check_case(env, V.RAGGED_CASE, "antialiased", n, packed=True)


# ---- 4. no visible pair -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_no_visible_pair(env, packed):
    ref = U.projection_reference(V.RAGGED_CASE)
    run = _project(env, ref, "antialiased", 300, packed, args=FAR_IN_FRONT)
    assert not run["vis"].any()
    if packed:
        assert run["gid"].numel() == 0   # nnz == 0: no partial kernel, the fold alone
    g = _viewmat_grads(run, ref["cots"], at_once=True)
    assert tuple(g.shape) == (3, 4, 4) and g.dtype == torch.float32 and not g.any()


@pytest.mark.parametrize("packed", [False, True])
def test_a_camera_that_sees_nothing_gets_exact_zeros(env, packed):
    ref = U.projection_reference(V.RAGGED_CASE)
    n = ref["means"].shape[0]
    vms = ref["viewmats"].clone()
    vms[1] = _away(vms[1])
    blind = _project(env, ref, "antialiased", n, packed, viewmats=vms)
    full = _project(env, ref, "antialiased", n, packed)
    assert not blind["vis"][1].any() and blind["vis"][0].any() and blind["vis"][2].any()
    gb = _viewmat_grads(blind, ref["cots"], at_once=True)
    gf = _viewmat_grads(full, ref["cots"], at_once=True)
    assert not gb[1].any()
    assert float(gf[1].abs().max()) > 0
    for c in (0, 2):   # the other cameras' sums do not notice (the packed list moved: the partials are formed per camera)
        assert float(gb[c].abs().max()) > 0 and torch.equal(gb[c], gf[c]), c


# ---- 5. determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_backward_is_deterministic(env, packed):
    ref = U.projection_reference(V.RAGGED_CASE)
    n = ref["means"].shape[0]
    a = _viewmat_grads(_project(env, ref, "antialiased", n, packed), ref["cots"], at_once=True)
    b = _viewmat_grads(_project(env, ref, "antialiased", n, packed), ref["cots"], at_once=True)
    assert float(a.abs().max()) > 0 and torch.equal(a, b)


# ---- 6. / 7. the whole call -------------------------------------------------------------------------------------------
EW, EH = 64, 48
_E2E = {}


def _e2e_scene(mode):
    """(clean scene of ~500 Gaussians for cameras 0 and 1 at 64 x 48, kept-pixel mask [2, H, W]) per rasterize mode."""
    if mode not in _E2E:
        from edgegaussians_amd import synth
        from oracle import c_oracle as CO
        sc0 = synth.make_scene(500, 2, EW, EH, seed=0, spread_opacity=True, scale=0.02, anisotropy=5.0)
        sc, _removed = clean_scene(sc0, [0, 1])
        N = sc.means.shape[0]
        keep = []
        for v in (0, 1):
            fw = CO.rasterize(sc.means.numpy(), sc.quats.numpy(), torch.exp(sc.log_scales).numpy(),
                              torch.sigmoid(sc.logit_opacities).squeeze(-1).numpy(), np.ones((N, 1), np.float32),
                              sc.viewmats[v].numpy(), sc.Ks[v].numpy(), EW, EH, antialiased=(mode == "antialiased"))
            keep.append(~borderline_pixel_mask(fw))
        _E2E[mode] = (sc, torch.stack(keep))
    return _E2E[mode]


def _e2e_leaves(sc):
    g = torch.Generator().manual_seed(17)
    N = sc.means.shape[0]
    return [sc.means, sc.quats, torch.exp(sc.log_scales), torch.sigmoid(sc.logit_opacities).squeeze(-1),
            0.2 + 0.8 * torch.rand(N, 3, generator=g)]


def _e2e_loss(render, alpha, wr, keep, dev):
    return (render * wr.to(dev)).sum() * 1e-3 + ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_whole_call_rgb(env, mode, packed):
    from edgegaussians_amd import rasterization
    from oracle import ref_torch as O
    sc, keep = _e2e_scene(mode)
    wr = torch.rand(2, EH, EW, 3, generator=torch.Generator().manual_seed(13)) * keep[..., None]
    key = ("cpu", mode)
    if key not in _E2E:   # the oracle's viewmats.grad, once per mode
        p = [t.clone().requires_grad_(True) for t in _e2e_leaves(sc)]
        vm = sc.viewmats[:2].clone().requires_grad_(True)
        render, alpha, _ = O.rasterization(*p, vm, sc.Ks[:2], EW, EH, packed=False, rasterize_mode=mode)
        _e2e_loss(render, alpha, wr, keep, "cpu").backward()
        _E2E[key] = vm.grad.clone()
    want = _E2E[key]
    assert not want[:, 3].any() and float(want.abs().max()) > 0
    aa = mode == "antialiased"
    res = {}
    for pose in (False, True):
        p = [t.clone().cuda().requires_grad_(True) for t in _e2e_leaves(sc)]
        vm = sc.viewmats[:2].clone().cuda().requires_grad_(pose)
        render, alpha, info = rasterization(*p, vm, sc.Ks[:2].cuda(), EW, EH, packed=packed, rasterize_mode=mode)
        reach = [info["means2d"], info["conics"]] + ([info["opacities"]] if aa else [])   # what reaches the projection
        for t in reach:
            t.retain_grad()
        _e2e_loss(render, alpha, wr, keep, "cuda").backward(retain_graph=pose)
        res[pose] = (p, vm, reach)
    assert res[False][1].grad is None
    got = res[True][1].grad.cpu()
    assert tuple(got.shape) == (2, 4, 4) and not got[:, 3].any()
    e = [rel_err(got[c, :3], want[c, :3]) for c in range(2)]
    print(f"whole call {mode} packed={packed}: viewmats.grad norm-rel error per camera {e}")
    record("viewmat_grad_whole_call", mode=mode, packed=packed, max_rel_err=e)
    for c in range(2):
        assert_close(got[c, :3], want[c, :3], rtol=1e-4, name=f"viewmats.grad camera {c}")
    # The other gradients must not notice the pose gradient.  The colour compositing backward accumulates with float
    # atomics, so two runs of one and the same call already differ in the last bits and the two calls can only be held to
    # the project's 1e-4 ...
    for name, a, b in zip(("means", "quats", "scales", "opacities", "colors"), res[True][0], res[False][0]):
        assert float(b.grad.abs().max()) > 0
        assert_close(a.grad, b.grad, rtol=1e-4, name=f"grad {name} with / without the pose gradient")
    # ... but means, quats and scales come from the projection backward alone: replayed on the very cotangents of the
    # pose call, without the pose gradient, it must give their bits.  (test_fast_path_... holds all four to torch.equal
    # between two whole calls on the unit-colour kernels, which are deterministic.)
    p, _vm, reach = res[True]
    replay = torch.autograd.grad(reach, p[:3], [t.grad for t in reach])
    for name, a, b in zip(("means", "quats", "scales"), p[:3], replay):
        assert torch.equal(a.grad, b), name


def test_whole_call_depth_isolates_the_projection(env):
    """render_mode="RGB+ED", classic: the cotangents that reach the projection (the .grad of info's means2d, conics and
    depths) go through the float64 projection VJP; viewmats.grad is held to TAU_SMALL * S of that (the bound for any
    number of pairs: this scene has hundreds, not thousands), whatever the compositing did."""
    from edgegaussians_amd import rasterization
    sc, keep = _e2e_scene("classic")
    wr = torch.rand(2, EH, EW, 4, generator=torch.Generator().manual_seed(14)) * keep[..., None]
    p = [t.clone().cuda().requires_grad_(True) for t in _e2e_leaves(sc)]
    vm = sc.viewmats[:2].clone().cuda().requires_grad_(True)
    render, alpha, info = rasterization(*p, vm, sc.Ks[:2].cuda(), EW, EH, packed=False, render_mode="RGB+ED",
                                        rasterize_mode="classic")
    for k in ("means2d", "conics", "depths"):
        info[k].retain_grad()
    _e2e_loss(render, alpha, wr, keep, "cuda").backward()
    cots = {k: info[k].grad.cpu() for k in ("means2d", "conics", "depths")}
    assert all(float(v.abs().max()) > 0 for v in cots.values())
    vis = (info["radii"] > 0).cpu()
    G, vis64, bottom = V.contributions(p[0].cpu(), p[1].cpu(), p[2].cpu(), sc.viewmats[:2], sc.Ks[:2], EW, EH, U.PROJ_DEFAULTS,
                                       cots, vis.numpy())
    assert bottom == 0.0 and torch.equal(vis64, vis)   # (the scene holds no integer-borderline Gaussian)
    Gs = sum(G.values())                               # the pair's contribution under the three cotangents together
    ratio = V.check(vm.grad, Gs.sum(1), Gs.abs().sum(1), "RGB+ED classic, projection share", V.TAU_SMALL)
    record("viewmat_grad_projection_share", ratio_to_S=ratio, tau=V.TAU_SMALL, visible_pairs=int(vis.sum()))


# ---- 8. the fast path -------------------------------------------------------------------------------------------------
def test_fast_path_steps_aside_for_a_pose_gradient(env, monkeypatch):
    from edgegaussians_amd import rasterization
    R = env
    sc, keep = _e2e_scene("classic")
    N = sc.means.shape[0]
    wr = torch.rand(1, EH, EW, 3, generator=torch.Generator().manual_seed(15)) * keep[:1, ..., None]
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda n, *a: (seen.append(n), real_call(n, *a))[1])

    def run(pose, colors_grad=False):
        seen.clear()
        p = [t.clone().cuda().requires_grad_(True) for t in _e2e_leaves(sc)[:4]]
        vm = sc.viewmats[:1].clone().cuda().requires_grad_(pose)
        col = torch.ones(N, 3, device="cuda", requires_grad=colors_grad)
        render, alpha, _ = rasterization(p[0], p[1], p[2], p[3], col, vm, sc.Ks[:1].cuda(), EW, EH, packed=False)
        _e2e_loss(render, alpha, wr, keep[:1], "cuda").backward()
        run.grads = [t.grad for t in p]
        return vm.grad, list(seen)

    g_none, log = run(False)      # the reference's own call: the log is what it was
    assert g_none is None
    assert "eg_operator_fwd" in log and "eg_operator_bwd" in log, log
    assert set(log) <= {"eg_project_fwd", "eg_tile_offsets", "eg_operator_fwd", "eg_operator_bwd"}, log
    g_pose, log = run(True)
    assert g_pose is not None and tuple(g_pose.shape) == (1, 4, 4) and float(g_pose.abs().max()) > 0
    assert "eg_operator_fwd" not in log and "eg_operator_bwd" not in log, log
    assert log.count("eg_project_fwd_cams") == 1 and log.count("eg_project_bwd_viewmats") == 1, log
    pose_grads = run.grads
    # the same general path without the pose gradient (the fast path switched off): its unit-colour kernels have no
    # atomics, so means, quats, scales and opacities must come out bit for bit
    monkeypatch.setattr(R, "_FAST_ENABLED", False)
    g_off, log = run(False)
    assert g_off is None and "eg_operator_fwd" not in log and "eg_project_bwd_viewmats" not in log, log
    for name, a, b in zip(("means", "quats", "scales", "opacities"), pose_grads, run.grads):
        assert float(b.abs().max()) > 0 and torch.equal(a, b), name
    g_general, log = run(True, colors_grad=True)   # the general path's colour kernels, no unit-colour shortcut anywhere
    assert "eg_composite_bwd_colors" in log, log
    assert_close(g_pose.cpu()[0, :3], g_general.cpu()[0, :3], rtol=1e-4, name="viewmats.grad, unit colours")
    assert not g_pose[:, 3].any()


# ---- 9. spherical harmonics -------------------------------------------------------------------------------------------
SH_MARGIN = 1e-5


@pytest.mark.parametrize("packed", [False, True])
def test_sh_directions_reach_the_poses(env, packed):
    """sh_degree=2 against the same call given [C, N, 3] colours evaluated in torch on means - inverse(viewmats)[:, :3, 3]:
    both share the projection's gradient (tests 1-3), so the agreement checks the direction chain."""
    from edgegaussians_amd import rasterization
    sc, keep = _e2e_scene("antialiased")
    L, K = 2, 9
    leaves = _e2e_leaves(sc)[:4]
    N = sc.means.shape[0]
    g = torch.Generator().manual_seed(21)
    coeffs = torch.randn(N, K, 3, generator=g) * (0.5 * (4 * torch.pi / (L + 1) ** 2) ** 0.5)
    # Gaussians whose unclamped colour lies within SH_MARGIN of the clamp in a camera may take the other branch: left out
    campos = torch.linalg.inv(sc.viewmats[:2].double())[:, :3, 3]
    raw = sh_oracle.sh_eval(L, sc.means.double()[None] - campos[:, None], coeffs.double()[None].expand(2, N, K, 3)) + 0.5
    ok = ~(raw.abs() < SH_MARGIN).any(-1).any(0)
    assert float(ok.float().mean()) >= 0.99
    leaves, coeffs = [t[ok].contiguous() for t in leaves], coeffs[ok].contiguous()
    N = leaves[0].shape[0]
    wr = torch.rand(2, EH, EW, 3, generator=torch.Generator().manual_seed(16)).cuda()
    Ks = sc.Ks[:2].cuda()

    def run(torch_colors):
        p = [t.clone().cuda().requires_grad_(True) for t in leaves]
        co = coeffs.clone().cuda().requires_grad_(True)
        vm = sc.viewmats[:2].clone().cuda().requires_grad_(True)
        if torch_colors:
            with torch.no_grad():
                info = rasterization(p[0], p[1], p[2], p[3], torch.ones(N, 3, device="cuda"), vm, Ks, EW, EH, packed=False)[2]
                mask = info["radii"] > 0
            dirs = p[0].double()[None] - torch.linalg.inv(vm.double())[:, :3, 3][:, None]
            col = (sh_oracle.sh_eval(L, dirs, co.double()[None].expand(2, N, K, 3)) + 0.5).clamp_min(0.0)
            colors, sh = torch.where(mask[..., None], col, torch.zeros_like(col)).float(), None
        else:
            colors, sh = co, L
        render, alpha, _ = rasterization(p[0], p[1], p[2], p[3], colors, vm, Ks, EW, EH, sh_degree=sh, packed=packed,
                                         rasterize_mode="antialiased")
        ((render * wr).sum() * 1e-3 + (alpha ** 2).sum() * 1e-3).backward()
        return vm.grad.cpu(), p[0].grad.cpu()

    got, got_means = run(False)
    want, want_means = run(True)
    # (torch.inverse's backward fills the bottom row as well, on both sides alike: the whole [4, 4] is compared)
    assert float(want[:, :3].abs().max()) > 0 and float(want[:, 3].abs().max()) > 0
    e = [rel_err(got[c], want[c]) for c in range(2)]
    print(f"sh_degree=2 packed={packed}: viewmats.grad norm-rel error per camera {e}")
    record("viewmat_grad_sh", packed=packed, max_rel_err=e)
    for c in range(2):
        assert_close(got[c, :3], want[c, :3], rtol=1e-4, name=f"viewmats.grad camera {c}")
        assert_close(got[c, 3], want[c, 3], rtol=1e-4, name=f"viewmats.grad camera {c}, bottom row")
    assert_close(got_means, want_means, rtol=1e-4, name="grad means")
