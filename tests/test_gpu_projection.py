"""Projection and its VJP (csrc/project_dev.h: forward_geom, radius_of, backward_geom; project.hip; cams.hip) through
the entry pair eg_project_fwd_cams / eg_project_bwd_cams, one Gaussian at a time, against oracle.ref_torch.project in
float64 with autograd:

* one output's N(0,1) cotangent at a time (means2d, depths, conics, compensations), each of v_means, v_quats, v_scales
  held row by row to tests.util.row_bound_check -- under a tensor-wide tolerance the means2d path (fx / z) carries
  v_means and every Jacobian term that reaches it through the conic, the FOV clamp included, is invisible;
* near_plane, far_plane, radius_clip and eps2d off their defaults and pairwise distinct; the FOV-clamp branches on
  scenes built in camera space for them; three cameras in one call (write, then accumulate); row independence of N;
  the same arguments through `rasterization`;
* integer decisions identical to the float64 reference's outside the quantified borderline set.

tests/test_projection_host.py asserts, with the references alone, that every scene used here reaches its branch and
that a correct fp32 evaluation stays within half of every bound."""
import numpy as np
import pytest
import torch

from tests import util as U
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


def _device_run(R, ref, mode, cots, n=None):
    """_Projection.apply on the first n rows of the case's scene; one autograd.grad per cotangent.
    Returns (outs: name -> cpu tensor [C, n, ...], grads: cotangent -> {"means" | "quats" | "scales": cpu [n, k]})."""
    a = ref["spec"]["args"]
    n = ref["means"].shape[0] if n is None else n
    p = [ref[k][:n].cuda().requires_grad_(True) for k in ("means", "quats", "scales")]
    opac = torch.full((n,), 0.5, device="cuda")
    out = R._Projection.apply(p[0], p[1], p[2], opac, ref["viewmats"].cuda(), ref["Ks"].cuda(), W, H, float(a["eps2d"]),
                              float(a["near_plane"]), float(a["far_plane"]), float(a["radius_clip"]), mode == "antialiased")
    outs = dict(zip(("radii",) + U.PROJ_OUTPUTS + ("tiles_per_gauss",), out[:6]))
    grads = {}
    for name, cot in cots.items():
        y = outs[name]
        g = torch.autograd.grad(y, p, cot[:, :n].cuda().reshape(y.shape).contiguous(), retain_graph=True)
        grads[name] = {k: gi.cpu() for k, gi in zip(U.PROJ_GRADS, g)}
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in outs.items()}, grads


def _comp_cot(ref):
    C, N = ref["vis"].shape
    return torch.randn(C, N, 1, generator=torch.Generator().manual_seed(19))


def _check_case(R, case, mode):
    ref = U.projection_reference(case)
    spec = ref["spec"]
    cots = dict(ref["cots"])
    if mode == "classic":   # no compensation in this mode: its cotangent reaches nothing (the `if (aa)` gate)
        cots["compensations"] = _comp_cot(ref)
    outs, grads = _device_run(R, ref, mode, cots)
    C, N = ref["vis"].shape
    # ---- integer decisions: identical to the float64 reference's outside the borderline set
    r, r64, border = outs["radii"].numpy(), ref["outs"]["radii"].numpy(), ref["border"]
    assert border.mean(axis=1).max() <= 0.02, border.mean(axis=1)
    differ = r != r64
    assert not (differ & ~border).any(), f"{int((differ & ~border).sum())} radii / culls differ outside the borderline set"
    culled = r == 0
    assert (outs["tiles_per_gauss"].numpy()[culled] == 0).all()
    for name in U.PROJ_OUTPUTS:
        assert (outs[name].numpy()[culled] == 0).all(), f"{name} is not zero on a culled row"
    rows_ok = ((r > 0) == (r64 > 0)).all(axis=0)    # (a cull decision that differs inside the set: nothing to compare)
    # ---- forward outputs, row by row against float64
    fwd = {}
    for name in U.PROJ_OUTPUTS:
        fwd[name] = max(U.fwd_row_err(outs[name][c], ref["outs"][name][c], ref["vis"][c] & rows_ok) for c in range(C))
        print(f"{case} {mode} fwd {name}: {fwd[name]:.3e}")
    for name in U.PROJ_OUTPUTS:
        assert fwd[name] <= U.FWD_ROW_TOL, (name, fwd[name])
    if spec["args"]["eps2d"] == 0.0:
        comp = outs["compensations"].numpy()[ref["vis"] & rows_ok[None]]
        assert np.abs(comp - 1.0).max() <= 1e-6
    # ---- the VJP, one cotangent at a time, row by row
    cells, loose_max, failures = {}, 0.0, []
    for cot in cots:
        if cot == "compensations" and mode == "classic":
            for g in U.PROJ_GRADS:
                assert not grads[cot][g].any(), f"classic mode: the compensation cotangent reached v_{g}"
            continue
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in U.PROJ_GRADS:
            ratio, loose, nonzero, over = U.row_bound_ratio(grads[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g], rows)
            cells[f"{cot}->{g}"] = ratio
            loose_max = max(loose_max, loose)
            print(f"{case} {mode} {cot}->{g}: {ratio:.3f} of the bound, {over} rows over, {nonzero} rows not exactly zero")
    record("projection_vjp_per_row", case=case, mode=mode, cameras=C, gaussians=N, args=spec["args"],
           ratio_to_bound=cells, loose_share=loose_max, fwd_row_err=fwd, borderline=int(border.sum()),
           decision_mismatches_inside=int(differ.sum()))
    for cot in cots:
        if cot == "compensations" and mode == "classic":
            continue
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in U.PROJ_GRADS:
            U.row_bound_check(grads[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g], f"{case} {mode} {cot}->v_{g}", rows)
    return ref, outs, grads


@pytest.mark.parametrize("mode", MODES)
def test_defaults(env, mode):
    """Inside-screen scene at the default arguments; in antialiased mode the compensation cotangent on its own scene of
    small Gaussians (rows with 1 - comp^2 >= 0.2: the cancellation inside the formula is not an input-conditioning
    matter), in classic mode it must reach nothing."""
    _check_case(env, "defaults", mode)
    if mode == "antialiased":
        _check_case(env, "defaults_comp", mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["fov_cam1", "fov_cam3"])
def test_fov_clamp(env, case, mode):
    """The in_x / in_y branches of backward_geom: five groups of Gaussians whose centres lie 1.35-1.8 half-screens off
    axis and whose radii still reach the screen, next to an inside and an off-screen-unclamped group; conic cotangent."""
    ref, outs, _ = _check_case(env, case, mode)
    group = ref["group"].numpy()
    per_group = [int((outs["radii"].numpy()[0] > 0)[group == k].sum()) for k in range(len(U.FOV_GROUPS))]
    assert min(per_group) >= 300, per_group


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["args_eps0.05", "args_eps1", "args_eps0"])
def test_arguments_off_defaults(env, case, mode):
    """near_plane 3.3, far_plane 4.2, radius_clip 6.5, eps2d 0.05 / 1.0 / 0.0: each cull removes >= 100 rows (host test),
    the backward runs on Gaussians a non-default plane culled (it trusts the stored radius).  The compensation
    cotangent at eps2d 0.05 needs Gaussians of the size of eps2d, which radius_clip 6.5 removes to the last: it runs on
    its own scene with radius_clip 2.5, the other three arguments unchanged."""
    _check_case(env, case, mode)
    if case == "args_eps0.05" and mode == "antialiased":
        _check_case(env, "args_eps0.05_comp", mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["three_cams_eps0.05", "three_cams_eps1"])
def test_three_cameras_in_one_call(env, case, mode):
    """Camera 0 writes, cameras 1 and 2 accumulate: the reference is the sum of the float64 per-camera gradients.
    >= 100 rows are culled in camera 0 and visible later, >= 100 are culled everywhere (host test) -- those rows are
    exactly zero (row_bound_check demands it wherever the reference row is zero)."""
    ref, outs, grads = _check_case(env, case, mode)
    never = ~(outs["radii"].numpy() > 0).any(axis=0)
    assert never.sum() >= 100
    for cot in grads:
        for g in U.PROJ_GRADS:
            assert not grads[cot][g][torch.from_numpy(never)].any()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_rows_do_not_depend_on_n(env, n):
    """One Gaussian per thread, contraction off: the first n rows alone give bit for bit the rows of the full run, in
    every output and every gradient, for every camera of a three-camera call (whose [C, N, ...] blocks move with N)."""
    ref = U.projection_reference("three_cams_eps1")
    key = ("device_full", "three_cams_eps1")
    if key not in U._proj_cache:
        U._proj_cache[key] = _device_run(env, ref, "antialiased", ref["cots"])
    full_outs, full_grads = U._proj_cache[key]
    outs, grads = _device_run(env, ref, "antialiased", ref["cots"], n=n)
    for name, t in outs.items():
        assert torch.equal(t, full_outs[name][:, :n]), name
    for cot in grads:
        for g in U.PROJ_GRADS:
            assert torch.equal(grads[cot][g], full_grads[cot][g][:n]), (cot, g)
    assert (outs["radii"] > 0).any() or n == 1


@pytest.mark.parametrize("eps2d", [0.05, 1.0])
@pytest.mark.parametrize("mode", MODES)
def test_arguments_through_rasterization(env, mode, eps2d, monkeypatch):
    """The general path of `rasterization` (two cameras, [N, 3] colours with grad) forwards near_plane, far_plane,
    radius_clip and eps2d to the projection pair; against oracle.ref_torch.rasterization with the same arguments."""
    from edgegaussians_amd import rasterization
    from oracle import c_oracle as CO
    from oracle import ref_torch as O
    R = env
    args = U.off_default_args(eps2d)
    vms_all, Ks_all = U.projection_cameras()
    cams = [0, 1]
    vms, Ks = vms_all[cams].contiguous(), Ks_all[cams].contiguous()
    means, quats, scales, _ = U.projection_scene("args", 0)
    bad = np.zeros(means.shape[0], bool)
    for c in range(2):
        bad |= U.projection_borderline(means, quats, scales, vms[c], Ks[c], W, H, args)
    keep_g = torch.from_numpy(~bad)
    means, quats, scales = means[keep_g].contiguous(), quats[keep_g].contiguous(), scales[keep_g].contiguous()
    N = means.shape[0]
    assert bad.sum() <= 0.02 * bad.size
    gen = torch.Generator().manual_seed(23)
    opac = 0.05 + 0.85 * torch.rand(N, generator=gen)
    colors0 = 0.2 + 0.8 * torch.rand(N, 3, generator=gen)
    keep = []
    for c in range(2):
        fw = CO.rasterize(means.numpy(), quats.numpy(), scales.numpy(), opac.numpy(), np.ones((N, 1), np.float32),
                          vms[c].numpy(), Ks[c].numpy(), W, H, args["near_plane"], args["far_plane"], args["eps2d"],
                          args["radius_clip"], mode == "antialiased")
        keep.append(~U.borderline_pixel_mask(fw))
    keep = torch.stack(keep)
    wr = torch.rand(2, H, W, 3, generator=gen) * keep[..., None]
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    res = {}
    for dev in ("cpu", "cuda"):
        p = [t.clone().to(dev).requires_grad_(True) for t in (means, quats, scales, opac, colors0)]
        fn = O.rasterization if dev == "cpu" else rasterization
        render, alpha, info = fn(means=p[0], quats=p[1], scales=p[2], opacities=p[3], colors=p[4], viewmats=vms.to(dev),
                                 Ks=Ks.to(dev), width=W, height=H, packed=False, rasterize_mode=mode, **args)
        loss = (render * wr.to(dev)).sum() * 1e-3 + ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3
        loss.backward()
        res[dev] = dict(render=render.detach().cpu(), alpha=alpha.detach().cpu(), radii=info["radii"].cpu(),
                        grads=[t.grad.cpu() for t in p])
    assert "eg_operator_fwd" not in seen, seen
    assert seen.count("eg_project_fwd_cams") == 1 and seen.count("eg_project_bwd_cams") == 1, seen
    cpu, gpu = res["cpu"], res["cuda"]
    assert torch.equal(gpu["radii"], cpu["radii"])
    assert (cpu["radii"] > 0).sum(dim=1).min() >= 500 and (cpu["radii"] == 0).sum(dim=1).min() >= 500
    e = {"render": rel_err(gpu["render"][keep], cpu["render"][keep]), "alpha": rel_err(gpu["alpha"][keep], cpu["alpha"][keep])}
    for name, a, b in zip(("means", "quats", "scales", "opacities", "colors"), gpu["grads"], cpu["grads"]):
        e[name] = rel_err(a, b)
    record("projection_args_through_rasterization", mode=mode, args=args, gaussians=N, removed_borderline_gaussians=int(bad.sum()),
           borderline_pixels=int((~keep).sum()), max_rel_err=e)
    assert_close(gpu["render"][keep], cpu["render"][keep], name="render")
    assert_close(gpu["alpha"][keep], cpu["alpha"][keep], name="alpha")
    for name, a, b in zip(("means", "quats", "scales", "opacities", "colors"), gpu["grads"], cpu["grads"]):
        assert_close(a, b, name=f"grad {name}")


# ---------------------------------------------------------------------------------------------------
def cat_calls_in_backward(rasterization, unit, monkeypatch):
    """torch.cat calls during the backward of render.sum() + alphas.sum() of a dense three-camera call (300 Gaussians,
    70 x 52, absgrad=False): D = 3 colours that require grad, or with `unit` torch.ones(N, 3) without grad."""
    from edgegaussians_amd import synth
    sc = synth.make_scene(300, 3, 70, 52, seed=5, spread_opacity=True, scale=0.05)
    p = [t.clone().cuda().requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    N = p[0].shape[0]
    if unit:
        colors = torch.ones(N, 3, device="cuda")
    else:
        colors = (0.2 + 0.8 * torch.rand(N, 3, generator=torch.Generator().manual_seed(5))).cuda().requires_grad_(True)
    render, alphas, _info = rasterization(p[0], p[1], torch.exp(p[2]), torch.sigmoid(p[3]).squeeze(-1), colors,
                                          sc.viewmats.cuda(), sc.Ks.cuda(), 70, 52, packed=False, absgrad=False)
    assert float(alphas.detach().mean()) > 0.05
    calls = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, "cat", lambda *a, **k: (calls.append(1), real_cat(*a, **k))[1])
    (render.sum() + alphas.sum()).backward()
    monkeypatch.setattr(torch, "cat", real_cat)
    assert all(t.grad is not None and t.grad.abs().max() > 0 for t in p[:3])
    return len(calls)


# What the commit before the projection nodes were merged gives, measured on it with this very function: one torch.cat
# behind colours that require grad, none behind unit colours.  The colour backward (eg_composite_bwd_colors) returns
# contiguous COPIES of its record's words, so `_Projection.backward` re-packs them once (`_g2d_record`); the shortcut
# -- both cotangents views of one [C, N, 8] record, passed on as it is -- is the unit-colour footprint backward's.
CAT_CALLS_OF_THE_PARENT = {False: 1, True: 0}


@pytest.mark.parametrize("unit", [False, True], ids=["colours", "unit"])
def test_backward_repacks_the_cotangent_record_as_often_as_before(env, unit, monkeypatch):
    """The number of torch.cat calls in the backward of a dense `rasterization` call is the parent commit's
    (CAT_CALLS_OF_THE_PARENT, measured on the parent): the no-re-pack shortcut of `_Projection.backward` is taken where
    it was taken, and no other assembly of the cotangent record has appeared."""
    from edgegaussians_amd import rasterization
    assert cat_calls_in_backward(rasterization, unit, monkeypatch) == CAT_CALLS_OF_THE_PARENT[unit]
