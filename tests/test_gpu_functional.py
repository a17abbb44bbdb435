"""gsplat's functional API on the device (edgegaussians_amd/functional.py; csrc/functional.hip for the stages that have
kernels of their own):

* quat_scale_to_covar_preci and the projection from covariances, forward and VJP, one Gaussian at a time against
  float64 references with the per-row bounds of tests/util.py (tests/test_functional_host.py asserts, with the
  references alone, that a correct fp32 evaluation stays within half of each);
* the stages that run `rasterization`'s kernels -- projection from quats + scales, isect_tiles, rasterize_to_pixels --
  and isect_offset_encode against `rasterization(packed=False)` itself, bit for bit where no atomics are involved;
* what only this API can do: centres shifted between projection and binning (against the torch oracle on its own
  binning of the shifted centres), Gaussians given as covariances;
* every unsupported corner raises what functional.py states."""
import math

import numpy as np
import pytest
import torch

from tests import functional_util as F
from tests import tile_util as TU
from tests import util as U
from tests.util import assert_close, record, rel_err

pytestmark = pytest.mark.gpu

W, H = U.PROJ_SIZE
SW, SH = 70, 52          # the small image of the stage tests: no tile size divides it
TS = (8, 16, 32)


@pytest.fixture(scope="module")
def G():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    import gsplat
    return gsplat


# ---------------------------------------------------------------------------------------------------
def _qs_device(G, ref, covar, preci, triu):
    """forward + one autograd.grad per computed output; returns (outs, grads) on the CPU"""
    p = [ref["quats"].cuda().requires_grad_(True), ref["scales"].cuda().requires_grad_(True)]
    c, q = G.quat_scale_to_covar_preci(p[0], p[1], compute_covar=covar, compute_preci=preci, triu=triu)
    assert (c is None) == (not covar) and (q is None) == (not preci)
    outs, grads = {}, {}
    for name, t in (("covars", c), ("precis", q)):
        if t is None:
            continue
        outs[name] = t.detach().cpu()
        g = torch.autograd.grad(t, p, ref["cots"][name].cuda(), retain_graph=True)
        grads[name] = {"quats": g[0].cpu(), "scales": g[1].cpu()}
    return outs, grads


@pytest.mark.parametrize("base", F.QS_BASES)
@pytest.mark.parametrize("n", F.QS_SIZES)
def test_quat_scale_to_covar_preci(G, n, base):
    """Every (compute_covar, compute_preci) x triu form that computes something: forward rows and the VJP of one output's
    N(0,1) cotangent at a time against float64, row by row under (ROW_FLOOR + 32 kappa_r) sigma_r; an absent output is
    None; full matrices are symmetric; the triu result is the upper triangle of the full one bit for bit."""
    worst = {}
    full_outs = None
    for triu in (False, True):
        ref = F.qs_reference(n, base, triu)
        for covar, preci in F.QS_FORMS:
            outs, grads = _qs_device(G, ref, covar, preci, triu)
            for name, t in outs.items():
                assert t.shape == ((n, 6) if triu else (n, 3, 3))
                if not triu:
                    assert torch.equal(t, t.transpose(-1, -2)), f"{name} is not symmetric"
                r, _ = U.row_bound_check(t.reshape(n, -1), ref["outs"][name].reshape(n, -1), ref["kappa_fwd"][name],
                                         f"n={n} base={base} triu={triu} {name}")
                worst[f"fwd {name}"] = max(worst.get(f"fwd {name}", 0.0), r)
                for g in ("quats", "scales"):
                    r, _ = U.row_bound_check(grads[name][g], ref["grads"][name][g], ref["kappa"][name][g],
                                             f"n={n} base={base} triu={triu} ({covar},{preci}) {name}->v_{g}")
                    worst[f"{name}->{g}"] = max(worst.get(f"{name}->{g}", 0.0), r)
            if covar and preci:
                if not triu:
                    full_outs = outs
                else:
                    for name in outs:
                        assert torch.equal(outs[name], F.triu6(full_outs[name])), name
    assert G.quat_scale_to_covar_preci(ref["quats"].cuda(), ref["scales"].cuda(), False, False) == (None, None)
    print(f"n={n} base={base}: ratio to the per-row bound {worst}")
    record("functional_quat_scale_to_covar_preci", gaussians=n, base_scale=base, ratio_to_bound=worst)


# ---------------------------------------------------------------------------------------------------
def _covars_device(G, ref, comp, cots, n=None):
    a = ref["spec"]["args"]
    n = ref["means"].shape[0] if n is None else n
    p = [ref[k][:n].cuda().requires_grad_(True) for k in ("means", "covars")]
    out = G.fully_fused_projection(p[0], p[1], None, None, ref["viewmats"].cuda(), ref["Ks"].cuda(), W, H, eps2d=a["eps2d"],
                                   near_plane=a["near_plane"], far_plane=a["far_plane"], radius_clip=a["radius_clip"],
                                   calc_compensations=comp)
    assert (out[4] is None) == (not comp)
    outs = {k: v for k, v in zip(("radii",) + U.PROJ_OUTPUTS, out) if v is not None}
    grads = {}
    for name, cot in cots.items():
        if name not in outs:
            continue
        y = outs[name]
        g = torch.autograd.grad(y, p, cot[:, :n].cuda().reshape(y.shape).contiguous(), retain_graph=True)
        grads[name] = {k: gi.cpu() for k, gi in zip(F.COVAR_GRADS, g)}
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in outs.items()}, grads


@pytest.mark.parametrize("comp", [False, True], ids=["classic", "calc_compensations"])
@pytest.mark.parametrize("case", F.COVAR_CASES)
def test_projection_from_covars(G, case, comp):
    """tests/test_gpu_projection.py's _check_case for fully_fused_projection(means, covars, None, None, ...): integer
    decisions equal to the float64 reference's outside the borderline set, culled rows exactly zero, forward rows within
    FWD_ROW_TOL, v_means and v_covars row by row for one cotangent at a time (the compensation cotangent on comp_rows);
    the backward run twice gives the same bits."""
    ref = F.covars_reference(case)
    cots = ref["cots"]
    outs, grads = _covars_device(G, ref, comp, cots)
    C, N = ref["vis"].shape
    r, r64, border = outs["radii"].numpy(), ref["outs"]["radii"].numpy(), ref["border"]
    assert outs["radii"].dtype == torch.int32 and outs["radii"].shape == (C, N)
    assert border.mean(axis=1).max() <= 0.02, border.mean(axis=1)
    differ = r != r64
    assert not (differ & ~border).any(), f"{int((differ & ~border).sum())} radii / culls differ outside the borderline set"
    culled = r == 0
    names = [k for k in U.PROJ_OUTPUTS if k in outs]
    assert ("compensations" in names) == comp
    for name in names:
        assert (outs[name].numpy()[culled] == 0).all(), f"{name} is not zero on a culled row"
    rows_ok = ((r > 0) == (r64 > 0)).all(axis=0)
    fwd = {}
    for name in names:
        got = outs[name].reshape(C, N, -1)
        fwd[name] = max(U.fwd_row_err(got[c], ref["outs"][name][c], ref["vis"][c] & rows_ok) for c in range(C))
        print(f"{case} comp={comp} fwd {name}: {fwd[name]:.3e}")
    cells, loose_max = {}, 0.0
    for cot in grads:
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in F.COVAR_GRADS:
            ratio, loose, nonzero, over = U.row_bound_ratio(grads[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g], rows)
            cells[f"{cot}->{g}"] = ratio
            loose_max = max(loose_max, loose)
            print(f"{case} comp={comp} {cot}->{g}: {ratio:.3f} of the bound, {over} rows over, {nonzero} rows not exactly zero")
    record("functional_covars_projection_per_row", case=case, calc_compensations=comp, cameras=C, gaussians=N,
           args=ref["spec"]["args"], ratio_to_bound=cells, loose_share=loose_max, fwd_row_err=fwd, borderline=int(border.sum()),
           decision_mismatches_inside=int(differ.sum()))
    for name in names:
        assert fwd[name] <= U.FWD_ROW_TOL, (name, fwd[name])
    for cot in grads:
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in F.COVAR_GRADS:
            U.row_bound_check(grads[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g], f"{case} comp={comp} {cot}->v_{g}", rows)
    if comp or "compensations" not in cots:
        assert set(grads) == set(cots)
    # no atomics: a second run gives the same bits
    outs2, grads2 = _covars_device(G, ref, comp, cots)
    for name in outs:
        assert torch.equal(outs[name], outs2[name]), name
    for cot in grads:
        for g in F.COVAR_GRADS:
            assert torch.equal(grads[cot][g], grads2[cot][g]), (cot, g)
    if C > 1:   # camera 0 writes, the later cameras accumulate; rows nobody sees are exactly zero
        vis = r > 0
        assert int((~vis[0] & vis[1:].any(axis=0)).sum()) >= 100
        never = torch.from_numpy(~vis.any(axis=0))
        assert int(never.sum()) >= 100
        for cot in grads:
            for g in F.COVAR_GRADS:
                assert not grads[cot][g][never].any()
    U._proj_cache[("functional_device_full", case, comp)] = (outs, grads)


@pytest.mark.parametrize("n", [1, 65, 257])
def test_covars_rows_do_not_depend_on_n(G, n):
    """One Gaussian per lane, contraction off: the first n rows alone give bit for bit the rows [:n] of the full call, in
    every output and every gradient, for every camera of a three-camera call."""
    ref = F.covars_reference("three_cams_eps1")
    key = ("functional_device_full", "three_cams_eps1", True)
    if key not in U._proj_cache:
        U._proj_cache[key] = _covars_device(G, ref, True, ref["cots"])
    full_outs, full_grads = U._proj_cache[key]
    outs, grads = _covars_device(G, ref, True, ref["cots"], n=n)
    for name, t in outs.items():
        assert torch.equal(t, full_outs[name][:, :n]), name
    for cot in grads:
        for g in F.COVAR_GRADS:
            assert torch.equal(grads[cot][g], full_grads[cot][g][:n]), (cot, g)


def test_projection_from_quats_is_rasterizations(G):
    """fully_fused_projection(means, None, quats, scales, ...) runs the projection node of `rasterization`: radii,
    means2d, depths and conics are those of info[...] bit for bit (three cameras, every argument off its default);
    the compensations are within FWD_ROW_TOL of the float64 oracle's."""
    ref = U.projection_reference("three_cams_eps1")
    a = ref["spec"]["args"]
    means, quats, scales = (ref[k].cuda() for k in ("means", "quats", "scales"))
    vms, Ks = ref["viewmats"].cuda(), ref["Ks"].cuda()
    N, C = means.shape[0], vms.shape[0]
    with torch.no_grad():
        _r, _a, info = G.rasterization(means, quats, scales, torch.full((N,), 0.5, device="cuda"), torch.rand(N, 3, device="cuda"),
                                       vms, Ks, W, H, packed=False, rasterize_mode="antialiased", **a)
        out = G.fully_fused_projection(means, None, quats, scales, vms, Ks, W, H, eps2d=a["eps2d"], near_plane=a["near_plane"],
                                       far_plane=a["far_plane"], radius_clip=a["radius_clip"], calc_compensations=True)
        plain = G.fully_fused_projection(means, None, quats, scales, vms, Ks, W, H, eps2d=a["eps2d"], near_plane=a["near_plane"],
                                         far_plane=a["far_plane"], radius_clip=a["radius_clip"])
    assert plain[4] is None
    for k, name in enumerate(("radii", "means2d", "depths", "conics")):
        assert torch.equal(out[k], info[name]), name
        assert torch.equal(plain[k], info[name]), name
    r = out[0].cpu().numpy()
    assert (r > 0).sum(axis=1).min() >= 1000
    rows_ok = ((r > 0) == ref["vis"]).all(axis=0)
    err = max(U.fwd_row_err(out[4][c].cpu(), ref["outs"]["compensations"][c], ref["vis"][c] & rows_ok) for c in range(C))
    record("functional_quats_projection", compensations_fwd_row_err=err)
    assert err <= U.FWD_ROW_TOL, err
    # the pose gradient stays available on this form
    vm_g = vms.clone().requires_grad_(True)
    m2d = G.fully_fused_projection(means, None, quats, scales, vm_g, Ks, W, H)[1]
    m2d.sum().backward()
    assert vm_g.grad is not None and vm_g.grad.abs().max() > 0


# ---------------------------------------------------------------------------------------------------
GRIDS = {1: (1, 1), 4: (2, 2), 35: (7, 5), 64: (8, 8)}   # T: (tile_width, tile_height), around the steps of tile_bits


def _ids(cells, T, gen):
    """sorted isect ids of the (camera * T + tile) cells, with random positive-float depth bits"""
    tile_bits = int(math.floor(math.log2(T))) + 1
    cells = np.sort(np.asarray(cells, np.int64))
    depth = torch.rand(cells.shape[0], generator=gen).add(0.5).numpy().view(np.int32).astype(np.int64)
    ids = ((cells // T) << (32 + tile_bits)) | ((cells % T) << 32) | depth
    return np.sort(ids), cells


@pytest.mark.parametrize("T", list(GRIDS))
@pytest.mark.parametrize("M", [0, 1, 255, 256, 257])
def test_isect_offset_encode_on_hand_made_ids(G, M, T):
    """Against np.searchsorted on the decoded (camera * T + tile): three cameras of which the middle one is empty, all
    entries in the first tile, all in the last."""
    tw, th = GRIDS[T]
    C = 3
    gen = torch.Generator().manual_seed(31 * M + T)
    np_rng = np.random.default_rng(17 * M + T)
    layouts = {
        "empty_camera_between": np.concatenate([np_rng.integers(0, T, M // 2), 2 * T + np_rng.integers(0, T, M - M // 2)]),
        "all_in_first_tile": np.zeros(M, np.int64),
        "all_in_last_tile": np.full(M, C * T - 1, np.int64),
    }
    for name, cells in layouts.items():
        ids, cells = _ids(cells, T, gen)
        got = G.isect_offset_encode(torch.from_numpy(ids).cuda(), C, tw, th)
        assert got.dtype == torch.int32 and got.shape == (C, th, tw)
        want = np.searchsorted(cells, np.arange(C * T), side="left").astype(np.int32).reshape(C, th, tw)
        assert np.array_equal(got.cpu().numpy(), want), (name, M, T)


def _stage_scene(n=500, views=4, seed=3):
    key = ("functional_stage_scene", n, views, seed)
    if key not in U._proj_cache:
        from edgegaussians_amd import synth
        U._proj_cache[key] = synth.make_scene(n, views, SW, SH, seed=seed, spread_opacity=True, scale=0.02, anisotropy=5.0)
    return U._proj_cache[key]


def _scene_params(sc, dev="cuda"):
    return [t.clone().to(dev) for t in (sc.means, sc.quats, torch.exp(sc.log_scales), torch.sigmoid(sc.logit_opacities).squeeze(-1))]


@pytest.mark.parametrize("ts", TS)
@pytest.mark.parametrize("cams", [[1], [0, 2, 3]], ids=["C1", "C3"])
def test_binning_stages_equal_rasterizations(G, ts, cams):
    """isect_tiles + isect_offset_encode on the projection's outputs give info["tiles_per_gauss" | "isect_ids" |
    "flatten_ids" | "isect_offsets"] of rasterization(packed=False, tile_size=ts) bit for bit (70 x 52: partial tiles on
    both axes at every size); one camera: also oracle.ref_torch's binning of the same floats."""
    from oracle import ref_torch as O
    sc = _stage_scene()
    means, quats, scales, opac = _scene_params(sc)
    vms, Ks = sc.viewmats[cams].cuda(), sc.Ks[cams].cuda()
    C, N = len(cams), means.shape[0]
    tw, th = math.ceil(SW / ts), math.ceil(SH / ts)
    with torch.no_grad():
        _r, _a, info = G.rasterization(means, quats, scales, opac, torch.rand(N, 3, device="cuda"), vms, Ks, SW, SH, packed=False,
                                       tile_size=ts)
        radii, m2d, depths, _conics, _ = G.fully_fused_projection(means, None, quats, scales, vms, Ks, SW, SH)
        tpg, ids, flat = G.isect_tiles(m2d, radii, depths, ts, tw, th, n_cameras=C)
        offs = G.isect_offset_encode(ids, C, tw, th)
    assert ids.shape[0] >= 500 * C
    assert tpg.dtype == torch.int32 and ids.dtype == torch.int64 and flat.dtype == torch.int32 and offs.dtype == torch.int32
    for name, t in (("tiles_per_gauss", tpg), ("isect_ids", ids), ("flatten_ids", flat), ("isect_offsets", offs)):
        assert t.shape == info[name].shape and torch.equal(t, info[name]), name
    if C == 1:
        t0, i0, f0 = O.isect_tiles(m2d[0].cpu().numpy(), radii[0].cpu().numpy(), depths[0].cpu().numpy(), ts, tw, th)
        assert np.array_equal(tpg[0].cpu().numpy(), t0) and np.array_equal(ids.cpu().numpy(), i0)
        assert np.array_equal(flat.cpu().numpy(), f0)
        assert np.array_equal(offs[0].cpu().numpy(), O.isect_offset_encode(i0, tw, th))


# ---------------------------------------------------------------------------------------------------
def _chain(G, p, colors, bg, vms, Ks, ts, mode, covars=False, shift=None, absgrad=True):
    """projection -> isect_tiles -> isect_offset_encode -> rasterize_to_pixels; returns (render, alphas, means2d)"""
    means, quats, scales, opac = p
    C, N = vms.shape[0], means.shape[0]
    aa = mode == "antialiased"
    if covars:
        cv = G.quat_scale_to_covar_preci(quats, scales, compute_covar=True, compute_preci=False, triu=True)[0]
        radii, m2d, depths, conics, comps = G.fully_fused_projection(means, cv, None, None, vms, Ks, SW, SH, calc_compensations=aa)
    else:
        radii, m2d, depths, conics, comps = G.fully_fused_projection(means, None, quats, scales, vms, Ks, SW, SH,
                                                                     calc_compensations=aa)
    if shift is not None:
        m2d = m2d + shift
    o = opac[None, :].expand(C, N)
    if aa:
        o = o * comps
    tw, th = math.ceil(SW / ts), math.ceil(SH / ts)
    _tpg, ids, flat = G.isect_tiles(m2d, radii, depths, ts, tw, th)
    offs = G.isect_offset_encode(ids, C, tw, th)
    col = colors[None].expand(C, N, colors.shape[-1])
    if m2d.requires_grad:
        m2d.retain_grad()
    render, alphas = G.rasterize_to_pixels(m2d, conics, col, o, SW, SH, ts, offs, flat, backgrounds=bg, absgrad=absgrad)
    return render, alphas, m2d


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
@pytest.mark.parametrize("with_bg", [False, True], ids=["nobg", "bg"])
@pytest.mark.parametrize("D", [1, 3, 5])
@pytest.mark.parametrize("ts", TS)
def test_chain_equals_rasterization(G, ts, D, with_bg, mode):
    """Two cameras.  render / alphas: torch.equal in classic mode (the same kernels on the same floats), assert_close in
    antialiased mode (opacity * compensation is a torch product here, a product inside the projection kernel there); the
    gradients of a random-cotangent loss and means2d.absgrad under assert_close (the compositing backward accumulates
    with atomics)."""
    sc = _stage_scene()
    cams = [0, 2]
    vms, Ks = sc.viewmats[cams].cuda(), sc.Ks[cams].cuda()
    N, C = sc.means.shape[0], 2
    gen = torch.Generator().manual_seed(41)
    colors0 = 0.2 + 0.8 * torch.rand(N, D, generator=gen)
    bg0 = torch.rand(C, D, generator=gen) if with_bg else None
    wr, wa = torch.rand(C, SH, SW, D, generator=gen).cuda(), torch.rand(C, SH, SW, 1, generator=gen).cuda()
    res = []
    for which in ("rasterization", "chain"):
        p = [t.requires_grad_(True) for t in _scene_params(sc)]
        col = colors0.clone().cuda().requires_grad_(True)
        bg = bg0.clone().cuda().requires_grad_(True) if with_bg else None
        if which == "rasterization":
            render, alphas, info = G.rasterization(p[0], p[1], p[2], p[3], col, vms, Ks, SW, SH, packed=False, tile_size=ts,
                                                   backgrounds=bg, absgrad=True, rasterize_mode=mode)
            m2d = info["means2d"]
            m2d.retain_grad()
        else:
            render, alphas, m2d = _chain(G, p, col, bg, vms, Ks, ts, mode)
        ((render * wr).sum() * 1e-3 + (alphas * wa).sum() * 1e-3).backward()
        grads = {k: t.grad for k, t in zip(("means", "quats", "scales", "opacities"), p)}
        grads["colors"] = col.grad
        if with_bg:
            grads["backgrounds"] = bg.grad
        grads["v_means2d"], grads["absgrad"] = m2d.grad, m2d.absgrad
        res.append(dict(render=render.detach(), alphas=alphas.detach(), grads=grads))
    want, got = res
    assert got["render"].shape == (C, SH, SW, D) and got["alphas"].shape == (C, SH, SW, 1)
    assert float(want["alphas"].mean()) > 0.05
    e = {"render": rel_err(got["render"], want["render"]), "alphas": rel_err(got["alphas"], want["alphas"])}
    e.update({k: rel_err(got["grads"][k], want["grads"][k]) for k in want["grads"]})
    record("functional_chain_vs_rasterization", tile_size=ts, channels=D, backgrounds=with_bg, mode=mode, max_rel_err=e)
    if mode == "classic":
        assert torch.equal(got["render"], want["render"]) and torch.equal(got["alphas"], want["alphas"])
    else:
        assert_close(got["render"], want["render"], name="render")
        assert_close(got["alphas"], want["alphas"], name="alphas")
    for k in want["grads"]:
        assert got["grads"][k] is not None and got["grads"][k].shape == want["grads"][k].shape, k
        assert_close(got["grads"][k], want["grads"][k], name=f"grad {k}")


@pytest.mark.parametrize("ts", TS)
def test_shifted_centres_against_the_oracle(G, ts):
    """What `rasterization` cannot do: means2d moved by (+3.25, -1.5) px between projection and binning, one camera.
    Against oracle.ref_torch.composite on the oracle's own projection and its own binning of the shifted centres;
    max_bad is the borderline-pixel share the tile-size tests allow for this comparison (tests/tile_util.BORDER_CAP)."""
    from oracle import ref_torch as O
    sc = _stage_scene()
    cam = 1
    shift = torch.tensor([3.25, -1.5])
    N = sc.means.shape[0]
    colors = 0.2 + 0.8 * torch.rand(N, 3, generator=torch.Generator().manual_seed(43))
    tw, th = math.ceil(SW / ts), math.ceil(SH / ts)
    with torch.no_grad():
        means, quats, scales, opac = _scene_params(sc, "cpu")
        radii, m2d, depths, conics, _ = O.project(means, quats, scales, sc.viewmats[cam], sc.Ks[cam], SW, SH)
        m2d = m2d + shift
        _t, ids, flat = O.isect_tiles(m2d.numpy(), radii.numpy(), depths.numpy(), ts, tw, th)
        want_r, want_a, _ = O.composite(m2d, conics, colors, opac, SW, SH, ts, O.isect_offset_encode(ids, tw, th), flat)
        plain_r = O.composite(m2d - shift, conics, colors, opac, SW, SH, ts, *_oracle_bins(O, m2d - shift, radii, depths, ts, tw, th))[0]
        render, alphas, _m = _chain(G, _scene_params(sc), colors.cuda(), None, sc.viewmats[[cam]].cuda(), sc.Ks[[cam]].cuda(), ts,
                                    "classic", shift=shift.cuda(), absgrad=False)
    assert rel_err(plain_r, want_r) > 0.1     # the shift is visible: the unshifted image is another image
    e = {"render": rel_err(render[0].cpu(), want_r), "alphas": rel_err(alphas[0].cpu(), want_a),
         "render_bad": U.frac_bad(render[0].cpu(), want_r), "alphas_bad": U.frac_bad(alphas[0].cpu(), want_a)}
    record("functional_shifted_centres_vs_oracle", tile_size=ts, **e)
    assert_close(render[0].cpu(), want_r, max_bad=TU.BORDER_CAP, name="render")
    assert_close(alphas[0].cpu(), want_a, max_bad=TU.BORDER_CAP, name="alphas")


def _oracle_bins(O, m2d, radii, depths, ts, tw, th):
    _t, ids, flat = O.isect_tiles(m2d.numpy(), radii.numpy(), depths.numpy(), ts, tw, th)
    return O.isect_offset_encode(ids, tw, th), flat


@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_covars_chain_matches_quats_chain(G, mode):
    """Gaussians that exist only as covariances: quat_scale_to_covar_preci(triu=True) -> projection from covars -> the
    same later stages, against the chain from quats + scales; images and the gradients that reach means, quats, scales
    (through the covariances), colours and opacities."""
    sc = _stage_scene()
    cams = [0, 2]
    vms, Ks = sc.viewmats[cams].cuda(), sc.Ks[cams].cuda()
    N = sc.means.shape[0]
    gen = torch.Generator().manual_seed(47)
    colors0 = 0.2 + 0.8 * torch.rand(N, 3, generator=gen)
    wr, wa = torch.rand(2, SH, SW, 3, generator=gen).cuda(), torch.rand(2, SH, SW, 1, generator=gen).cuda()
    res = []
    for covars in (False, True):
        p = [t.requires_grad_(True) for t in _scene_params(sc)]
        col = colors0.clone().cuda().requires_grad_(True)
        render, alphas, _m = _chain(G, p, col, None, vms, Ks, 16, mode, covars=covars)
        ((render * wr).sum() * 1e-3 + (alphas * wa).sum() * 1e-3).backward()
        res.append(dict(render=render.detach(), alphas=alphas.detach(),
                        grads={k: t.grad for k, t in zip(("means", "quats", "scales", "opacities", "colors"), p + [col])}))
    want, got = res
    e = {"render": rel_err(got["render"], want["render"]), "alphas": rel_err(got["alphas"], want["alphas"])}
    e.update({k: rel_err(got["grads"][k], want["grads"][k]) for k in want["grads"]})
    record("functional_covars_chain_vs_quats_chain", mode=mode, max_rel_err=e)
    assert_close(got["render"], want["render"], name="render")
    assert_close(got["alphas"], want["alphas"], name="alphas")
    for k in want["grads"]:
        assert_close(got["grads"][k], want["grads"][k], name=f"grad {k}")


# ---------------------------------------------------------------------------------------------------
def test_unsupported_corners_raise(G):
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)  # noqa: E731
    i32 = dict(dtype=torch.int32)
    vm, K = torch.eye(4, device="cuda")[None], torch.eye(3, device="cuda")[None]
    proj = (vm, K, 32, 32)
    with pytest.raises(NotImplementedError, match=r"rasterization\(packed=True\)"):
        G.fully_fused_projection(z(4, 3), z(4, 6), None, None, *proj, packed=True)
    with pytest.raises(NotImplementedError, match="sparse_grad"):
        G.fully_fused_projection(z(4, 3), None, z(4, 4), z(4, 3), *proj, sparse_grad=True)
    with pytest.raises(NotImplementedError, match="viewmats"):
        G.fully_fused_projection(z(4, 3), z(4, 6), None, None, vm.clone().requires_grad_(True), K, 32, 32)
    with pytest.raises(ValueError, match="exactly one"):
        G.fully_fused_projection(z(4, 3), None, None, None, *proj)
    with pytest.raises(ValueError, match="exactly one"):
        G.fully_fused_projection(z(4, 3), z(4, 6), z(4, 4), z(4, 3), *proj)
    with pytest.raises(ValueError, match="covars"):
        G.fully_fused_projection(z(4, 3), z(4, 3, 3), None, None, *proj)
    with pytest.raises(TypeError, match="covars"):
        G.fully_fused_projection(z(4, 3), z(4, 6, dtype=torch.float64), None, None, *proj)
    with pytest.raises(TypeError, match="quats"):
        G.quat_scale_to_covar_preci(z(4, 4, dtype=torch.float16), z(4, 3))
    with pytest.raises(ValueError, match="scales"):
        G.quat_scale_to_covar_preci(z(4, 4), z(5, 3))
    tiles = (z(1, 4, 2), z(1, 4, **i32), z(1, 4))
    with pytest.raises(NotImplementedError, match=r"rasterization\(packed=True\)"):
        G.isect_tiles(*tiles, 16, 2, 2, packed=True)
    with pytest.raises(NotImplementedError, match="sort=False"):
        G.isect_tiles(*tiles, 16, 2, 2, sort=False)
    for bad in (4, 12, 64, True):
        with pytest.raises(NotImplementedError, match="tile_size"):
            G.isect_tiles(*tiles, bad, 2, 2)
    with pytest.raises(TypeError, match="radii"):
        G.isect_tiles(z(1, 4, 2), z(1, 4), z(1, 4), 16, 2, 2)
    with pytest.raises(ValueError, match="depths"):
        G.isect_tiles(z(1, 4, 2), z(1, 4, **i32), z(1, 5), 16, 2, 2)
    with pytest.raises(TypeError, match="isect_ids"):
        G.isect_offset_encode(z(4, **i32), 1, 2, 2)
    ras = (z(1, 4, 2), z(1, 4, 3), z(1, 4, 3), z(1, 4), 32, 32)
    offs, flat = z(1, 2, 2, **i32), z(0, **i32)
    with pytest.raises(NotImplementedError, match=r"rasterization\(packed=True\)"):
        G.rasterize_to_pixels(*ras, 16, offs, flat, packed=True)
    with pytest.raises(NotImplementedError, match="masks"):
        G.rasterize_to_pixels(*ras, 16, offs, flat, masks=z(1, 2, 2, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="tile_size"):
        G.rasterize_to_pixels(*ras, 24, offs, flat)
    with pytest.raises(ValueError, match="isect_offsets"):
        G.rasterize_to_pixels(*ras, 16, z(1, 3, 2, **i32), flat)
    with pytest.raises(ValueError, match="backgrounds"):
        G.rasterize_to_pixels(*ras, 16, offs, flat, backgrounds=z(1, 4))
    with pytest.raises(ValueError, match="colors"):
        G.rasterize_to_pixels(z(1, 4, 2), z(1, 4, 3), z(4, 3), z(1, 4), 32, 32, 16, offs, flat)
    # ... and the empty intersection list renders the background under a transmittance of one
    bg = torch.rand(1, 3, device="cuda")
    render, alphas = G.rasterize_to_pixels(*ras, 16, offs, flat, backgrounds=bg)
    assert not alphas.any() and torch.equal(render, bg[:, None, None, :].expand(1, 32, 32, 3))
