"""`rasterization(packed=True)` (csrc/packed.hip, the packed branch of edgegaussians_amd/rasterizer.py):

1. projection and binning against the dense path of the same commit, bit for bit (the same device functions decide the
   culls, the same records reach the same compositing kernel in the same order);
2. the projection VJP, one output's cotangent at a time, row by row against float64 (tests.util.projection_reference,
   the bounds of tests/test_gpu_projection.py);
3. the whole call against the dense CPU oracle (oracle.ref_torch, wrapped by the render-mode and channel tests);
4. the native calls it makes; 5. sparse_grad; 6. run-to-run determinism; 7. no visible pair at all; 8. the default
   call; 9. peak memory against the dense path.

Visible shares of the scenes of test 1 (float64 oracle, per camera): three_cams_eps0.05 0.43 / 0.31 / 0.36,
three_cams_eps1 0.50 / 0.37 / 0.43, args_eps1 0.50, and 0.41-0.49 on their first 37 rows: inside the 20 %-80 % band the
test asserts.  fov_cam1 runs at the DEFAULT arguments and keeps 0.987 of its pairs (only part of its off-screen group
is culled), and a single Gaussian is kept or not: for those the test asserts what can hold -- fov_cam1 has both kept
and culled pairs -- and prints the share."""
import math

import pytest
import torch

from tests import util as U
from tests.util import assert_close, record, rel_err

pytestmark = pytest.mark.gpu

W, H = U.PROJ_SIZE
MODES = ("classic", "antialiased")
PER_PAIR = ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss")


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    from oracle import c_oracle as CO
    return synth, O, CO


def _away(viewmat):
    """The same camera turned half a turn about its own y axis: everything it saw is now behind it."""
    return torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0])) @ viewmat


def _proj_inputs(case, n=None, empty_middle=False):
    spec = U.PROJ_CASES[case]
    vms_all, Ks_all = U.projection_cameras()
    cams = list(spec["cams"])
    vms, Ks = vms_all[cams].clone(), Ks_all[cams].clone()
    if empty_middle:
        vms[1] = _away(vms[1])
    means, quats, scales, _ = U.projection_scene(spec["kind"], spec["scene_cam"])
    n = means.shape[0] if n is None else n
    g = torch.Generator().manual_seed(31)
    kw = dict(means=means[:n].contiguous().cuda(), quats=quats[:n].contiguous().cuda(), scales=scales[:n].contiguous().cuda(),
              opacities=(0.05 + 0.9 * torch.rand(n, generator=g)).cuda(), colors=(0.2 + 0.8 * torch.rand(n, 3, generator=g)).cuda(),
              viewmats=vms.contiguous().cuda(), Ks=Ks.contiguous().cuda(), width=W, height=H,
              backgrounds=torch.rand(len(cams), 3, generator=g).cuda(), **spec["args"])
    return kw, len(cams), n


def _check_against_dense(kw, C, N, mode, shares=None, empty=()):
    from edgegaussians_amd import rasterization
    with torch.no_grad():
        rd, ad, di = rasterization(packed=False, rasterize_mode=mode, **kw)
        rp, ap, pi = rasterization(packed=True, rasterize_mode=mode, **kw)
    cam, gid = pi["camera_ids"], pi["gaussian_ids"]
    assert cam.dtype == torch.int64 and gid.dtype == torch.int64
    assert di["camera_ids"] is None and di["gaussian_ids"] is None
    lin = cam * N + gid
    assert bool((lin[1:] > lin[:-1]).all())
    vis = di["radii"] > 0
    assert torch.equal(lin, torch.nonzero(vis.reshape(-1))[:, 0])
    share = vis.float().mean(dim=1).tolist()
    print("visible share per camera:", share)
    for c in range(C):
        if c in empty:
            assert share[c] == 0.0
        elif shares is not None:
            assert shares[0] <= share[c] <= shares[1], share
    for k in PER_PAIR:
        assert pi[k].dtype == di[k].dtype, k
        assert torch.equal(pi[k], di[k][cam, gid]), k
    assert pi["radii"].dtype == torch.int32 and pi["tiles_per_gauss"].dtype == torch.int32
    assert bool((pi["radii"] > 0).all()) or lin.numel() == 0
    assert torch.equal(pi["isect_offsets"], di["isect_offsets"])
    assert torch.equal(pi["isect_ids"], di["isect_ids"]) and pi["isect_ids"].dtype == torch.int64
    f = pi["flatten_ids"].long()
    assert pi["flatten_ids"].dtype == torch.int32
    assert torch.equal(cam[f] * N + gid[f], di["flatten_ids"].long())
    assert torch.equal(rp, rd) and torch.equal(ap, ad) and torch.equal(pi["last_ids"], di["last_ids"])
    for k in ("tile_width", "tile_height", "width", "height", "tile_size", "n_cameras"):
        assert pi[k] == di[k], k
    return share


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [None, 37, 1])
@pytest.mark.parametrize("case", ["three_cams_eps0.05", "three_cams_eps1", "args_eps1", "fov_cam1"])
def test_projection_and_binning_equal_the_dense_path(env, case, n, mode):
    kw, C, N = _proj_inputs(case, n)
    banded = case != "fov_cam1" and n != 1   # (see the module docstring)
    share = _check_against_dense(kw, C, N, mode, shares=(0.2, 0.8) if banded else None)
    if case == "fov_cam1" and n is None:
        assert 0.0 < share[0] < 1.0


@pytest.mark.parametrize("mode", MODES)
def test_a_camera_that_sees_nothing_owns_an_empty_range(env, mode):
    kw, C, N = _proj_inputs("three_cams_eps1", empty_middle=True)
    _check_against_dense(kw, C, N, mode, shares=(0.2, 0.8), empty=(1,))


# ---- 2. the projection VJP per cotangent -----------------------------------------------------------------------------
INFO_OF = {"means2d": "means2d", "depths": "depths", "conics": "conics", "compensations": "opacities"}


def _packed_projection_grads(ref, mode, cots, all_at_once=False):
    """rasterization(packed=True) on the case's scene; opacities == 1, so that in antialiased mode info["opacities"] IS
    the compensation.  One autograd.grad per cotangent (or one for their sum)."""
    from edgegaussians_amd import rasterization
    a = ref["spec"]["args"]
    N = ref["means"].shape[0]
    p = [ref[k].cuda().requires_grad_(True) for k in ("means", "quats", "scales")]
    _r, _a, info = rasterization(p[0], p[1], p[2], torch.ones(N, device="cuda"), torch.ones(N, 1, device="cuda"),
                                 ref["viewmats"].cuda(), ref["Ks"].cuda(), W, H, packed=True, rasterize_mode=mode, **a)
    cam, gid = info["camera_ids"], info["gaussian_ids"]
    losses = {}
    for name, cot in cots.items():
        y = info[INFO_OF[name]]
        losses[name] = (y * cot.cuda()[cam, gid].reshape(y.shape)).sum()
    if all_at_once:
        g = torch.autograd.grad(sum(losses.values()), p)
        grads = dict(zip(U.PROJ_GRADS, g))
    else:
        grads = {name: dict(zip(U.PROJ_GRADS, (t.cpu() for t in torch.autograd.grad(l, p, retain_graph=True))))
                 for name, l in losses.items()}
    radii = torch.zeros(ref["vis"].shape, dtype=torch.int32, device="cuda")
    radii[cam, gid] = info["radii"]
    return grads, radii.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ["three_cams_eps0.05", "three_cams_eps1", "args_eps1"])
def test_projection_vjp_per_cotangent(env, case, mode):
    ref = U.projection_reference(case)
    cots = {k: v for k, v in ref["cots"].items() if not (k == "compensations" and mode == "classic")}
    grads, r = _packed_projection_grads(ref, mode, cots)
    r64, border = ref["outs"]["radii"].numpy(), ref["border"]
    assert not ((r != r64) & ~border).any()
    rows_ok = ((r > 0) == (r64 > 0)).all(axis=0)
    never = torch.from_numpy(~(r > 0).any(axis=0))
    cells = {}
    for cot in cots:
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in U.PROJ_GRADS:
            assert grads[cot][g].shape == ref["grads"][cot][g].shape
            ratio, _ = U.row_bound_check(grads[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g],
                                         f"packed {case} {mode} {cot}->v_{g}", rows)
            cells[f"{cot}->{g}"] = ratio
            print(f"packed {case} {mode} {cot}->{g}: {ratio:.3f} of the bound")
            assert not grads[cot][g][never].any()  # rows no camera sees: exact zeros
    record("packed_projection_vjp_per_row", case=case, mode=mode, ratio_to_bound=cells)


def test_backward_is_deterministic(env):
    ref = U.projection_reference("three_cams_eps1")
    a, _ = _packed_projection_grads(ref, "antialiased", ref["cots"], all_at_once=True)
    b, _ = _packed_projection_grads(ref, "antialiased", ref["cots"], all_at_once=True)
    for g in U.PROJ_GRADS:
        assert float(a[g].abs().max()) > 0
        assert torch.equal(a[g], b[g]), g


# ---- 3. the whole call against the CPU oracle ------------------------------------------------------------------------
from tests.test_gpu_channels import _setup, oracle_rasterization as oracle_wide  # noqa: E402
from tests.test_gpu_render_modes import oracle_rasterization as oracle_modes  # noqa: E402
from tests.test_gpu_sh import CLAMP_MARGIN, _coefficients, _oracle_colors  # noqa: E402

WHOLE = {  # name: render_mode, rasterize_mode, cameras, colours, backgrounds, channel_chunk, sh_degree
    "rgb_classic_bg": ("RGB", "classic", [0, 2, 3], ("N", 3), True, 32, None),
    "rgb_ed_percam": ("RGB+ED", "antialiased", [0, 2, 3], ("CN", 3), False, 32, None),
    "depth_one_cam": ("D", "antialiased", [1], ("N", 3), False, 32, None),
    "five_channels_chunk4": ("RGB", "antialiased", [0, 2, 3], ("N", 5), True, 4, None),
    "sh_degree2": ("RGB", "antialiased", [0, 2, 3], ("NK", 9), False, 32, 2),
    "unit_one_cam": ("RGB", "antialiased", [1], ("unit", 1), False, 32, None),
}
_CPU = {}


def _whole_inputs(env, name):
    render_mode, mode, cams, (ckind, D), with_bg, chunk, L = WHOLE[name]
    sc, keep, removed = _setup(env, cams, mode)
    C, N = len(cams), sc.means.shape[0]
    g = torch.Generator().manual_seed(11)
    if ckind == "unit":
        col = torch.ones(N, 1)
    elif ckind == "NK":
        col = _coefficients(L, D, (N,))
    else:
        col = 0.2 + 0.8 * torch.rand(*((C, N, D) if ckind == "CN" else (N, D)), generator=g)
    Dc = 3 if L is not None else D
    bg = torch.rand(C, Dc, generator=torch.Generator().manual_seed(12)) if with_bg else None
    Dout = (0 if render_mode in ("D", "ED") else Dc) + int(render_mode != "RGB")
    wr = torch.rand(C, H, W, Dout, generator=torch.Generator().manual_seed(13)) * keep[..., None]
    leaves = [sc.means, sc.quats, torch.exp(sc.log_scales), torch.sigmoid(sc.logit_opacities).squeeze(-1)]
    return sc, keep, removed, cams, leaves, col, bg, wr


def _loss(render, alpha, wr, keep, dev):
    return (render * wr.to(dev)).sum() * 1e-3 + ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3


def _cpu_run(env, name):
    """The oracle's forward and backward of one case, computed once and shared (never modified)."""
    if name in _CPU:
        return _CPU[name]
    O = env[1]
    render_mode, mode, _cams, (ckind, D), _with_bg, chunk, L = WHOLE[name]
    sc, keep, removed, cams, leaves, col0, bg0, wr = _whole_inputs(env, name)
    p = [t.clone().requires_grad_(True) for t in leaves]
    col = col0.clone().requires_grad_(ckind != "unit")
    bg = bg0.clone().requires_grad_(True) if bg0 is not None else None
    kw = dict(means=p[0], quats=p[1], scales=p[2], opacities=p[3], viewmats=sc.viewmats[cams], Ks=sc.Ks[cams], width=W,
              height=H, backgrounds=bg, render_mode=render_mode, rasterize_mode=mode)
    near = torch.zeros(p[0].shape[0], dtype=torch.bool)
    if L is not None:
        colors, raw, vis = _oracle_colors(O, L, p[0], col, kw["viewmats"], kw["Ks"], p[1].detach(), p[2].detach())
        near = ((raw.abs() < CLAMP_MARGIN) & vis[..., None]).any(-1).any(0)
        assert float(near.float().mean()) <= 0.01
    else:
        colors = col
    if render_mode in ("D", "ED"):
        render, alpha, info = oracle_modes(O, colors=colors, **kw)
    else:
        render, alpha, info = oracle_wide(O, colors=colors, channel_chunk=chunk, **kw)
    info["means2d"].retain_grad()
    loss = _loss(render, alpha, wr, keep, "cpu")
    loss.backward()
    _CPU[name] = dict(render=render.detach(), alpha=alpha.detach(), loss=float(loss.detach()), p=[t.grad for t in p],
                      col=col.grad, bg=bg.grad if bg is not None else None, v_means2d=info["means2d"].grad,
                      absgrad=info["means2d"].absgrad, near=near)
    return _CPU[name]


def _gpu_run(env, name, seen=None, **extra):
    from edgegaussians_amd import rasterization
    render_mode, mode, _cams, (ckind, D), _with_bg, chunk, L = WHOLE[name]
    sc, keep, removed, cams, leaves, col0, bg0, wr = _whole_inputs(env, name)
    p = [t.clone().cuda().requires_grad_(True) for t in leaves]
    col = col0.clone().cuda().requires_grad_(ckind != "unit")
    bg = bg0.clone().cuda().requires_grad_(True) if bg0 is not None else None
    if seen is not None:
        seen.clear()
    render, alpha, info = rasterization(p[0], p[1], p[2], p[3], col, sc.viewmats[cams].cuda(), sc.Ks[cams].cuda(), W, H,
                                        backgrounds=bg, render_mode=render_mode, rasterize_mode=mode, absgrad=True,
                                        channel_chunk=chunk, sh_degree=L, packed=True, **extra)
    info["means2d"].retain_grad()
    loss = _loss(render, alpha, wr, keep, "cuda")
    loss.backward()
    return dict(render=render.detach().cpu(), alpha=alpha.detach().cpu(), loss=float(loss.detach()), p=p, col=col, bg=bg, info=info,
                keep=keep, removed=removed)


@pytest.mark.parametrize("name", list(WHOLE))
def test_whole_call_matches_the_oracle(env, name, monkeypatch):
    from edgegaussians_amd import rasterizer as R
    render_mode, mode, cams, (ckind, D), with_bg, chunk, L = WHOLE[name]
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda n, *a: (seen.append(n), real_call(n, *a))[1])
    cpu = _cpu_run(env, name)
    gpu = _gpu_run(env, name, seen=seen)
    keep, info = gpu["keep"], gpu["info"]
    cam, gid = info["camera_ids"].cpu(), info["gaussian_ids"].cpu()
    assert info["means2d"].shape == (cam.shape[0], 2) and info["means2d"].requires_grad and not info["means2d"].is_leaf
    e = {}
    assert gpu["render"].shape == cpu["render"].shape
    for k in ("render", "alpha"):
        e[k] = rel_err(gpu[k][keep], cpu[k][keep])
        assert_close(gpu[k][keep], cpu[k][keep], name=k)
    assert abs(gpu["loss"] - cpu["loss"]) <= 1e-4 * abs(cpu["loss"])
    ok = ~cpu["near"]
    for k, a, b in zip(("means", "quats", "scales", "opacities"), gpu["p"], cpu["p"]):
        ga, gb = (a.grad.cpu()[ok], b[ok]) if k == "means" else (a.grad.cpu(), b)
        assert not a.grad.is_sparse
        e[k] = rel_err(ga, gb)
        assert_close(ga, gb, name=f"grad {k}")
    if render_mode in ("D", "ED") or ckind == "unit":
        assert gpu["col"].grad is None
    else:
        ga, gb = gpu["col"].grad.cpu(), cpu["col"]
        assert ga.shape == gb.shape
        if L is not None:
            ga, gb = ga[ok], gb[ok]
        assert float(gb.abs().max()) > 0
        e["colors"] = rel_err(ga, gb)
        assert_close(ga, gb, name="grad colors")
    if with_bg:
        e["backgrounds"] = rel_err(gpu["bg"].grad, cpu["bg"])
        assert_close(gpu["bg"].grad.cpu(), cpu["bg"], name="grad backgrounds")
    v2, ab = info["means2d"].grad.cpu(), info["means2d"].absgrad.cpu()
    assert v2.shape == ab.shape == (cam.shape[0], 2)
    e["v_means2d"] = rel_err(v2, cpu["v_means2d"][cam, gid])
    e["absgrad"] = rel_err(ab, cpu["absgrad"][cam, gid])
    assert_close(v2, cpu["v_means2d"][cam, gid], name="v_means2d")
    assert_close(ab, cpu["absgrad"][cam, gid], name="absgrad")
    # 4. the native calls: the packed entries once each, nothing of the dense projection or the fast path underneath
    for entry in ("eg_packed_count", "eg_packed_write", "eg_packed_bin", "eg_packed_bwd"):
        assert seen.count(entry) == 1, (entry, seen)
    assert not [n for n in seen if n in ("eg_project_fwd_cams", "eg_project_bwd_cams", "eg_operator_fwd", "eg_project_fwd",
                                         "eg_packed_bwd_sparse")], seen
    record("packed_vs_torch_oracle", case=name, pairs=int(cam.shape[0]), removed_borderline_gaussians=gpu["removed"],
           borderline_pixels=int((~keep).sum()), max_rel_err=e)


# ---- 5. sparse_grad ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rgb_classic_bg", "depth_one_cam"])
def test_sparse_grad(env, name, monkeypatch):
    from edgegaussians_amd import rasterizer as R
    C = len(WHOLE[name][2])
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda n, *a: (seen.append(n), real_call(n, *a))[1])
    cpu = _cpu_run(env, name)
    gpu = _gpu_run(env, name, sparse_grad=True)
    assert seen.count("eg_packed_bwd_sparse") == 1 and "eg_packed_bwd" not in seen
    gid = gpu["info"]["gaussian_ids"]
    N = gpu["p"][0].shape[0]
    for k, a, b, width in zip(("means", "quats", "scales"), gpu["p"], cpu["p"], (3, 4, 3)):
        g = a.grad
        assert g.is_sparse and tuple(g.shape) == (N, width), k
        assert g.is_coalesced() == (C == 1), k
        assert torch.equal(g._indices()[0], gid), k
        assert tuple(g._values().shape) == (gid.shape[0], width), k
        assert_close(g.to_dense().cpu(), b, name=f"sparse grad {k}")
    assert not gpu["p"][3].grad.is_sparse
    assert_close(gpu["p"][3].grad.cpu(), cpu["p"][3], name="grad opacities")
    if gpu["col"].grad is not None:
        assert not gpu["col"].grad.is_sparse
        assert_close(gpu["col"].grad.cpu(), cpu["col"], name="grad colors")


def test_sparse_grad_needs_packed(env):
    from edgegaussians_amd import rasterization
    kw, _, _ = _proj_inputs("args_eps1", 37)
    with pytest.raises(ValueError, match="sparse_grad"):
        rasterization(packed=False, sparse_grad=True, **kw)


# ---- 7. no visible pair -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("sparse", [False, True])
def test_no_visible_pair(env, with_bg, sparse):
    from edgegaussians_amd import rasterization
    kw, C, N = _proj_inputs("three_cams_eps1", 300)
    kw["viewmats"] = torch.stack([_away(v) for v in kw["viewmats"].cpu()]).cuda()
    bg = kw.pop("backgrounds").requires_grad_(True) if with_bg else (kw.pop("backgrounds"), None)[1]
    p = {k: kw[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "colors")}
    kw.update(p)
    render, alphas, info = rasterization(packed=True, sparse_grad=sparse, backgrounds=bg, render_mode="RGB+D", absgrad=True,
                                         **kw)
    assert render.shape == (C, H, W, 4) and alphas.shape == (C, H, W, 1)
    assert not alphas.any()
    if with_bg:
        want = torch.cat([bg.detach(), torch.zeros(C, 1, device="cuda")], dim=-1)[:, None, None, :].expand(C, H, W, 4)
        assert torch.equal(render.detach(), want)
    else:
        assert not render.any()
    shapes = {"camera_ids": ((0,), torch.int64), "gaussian_ids": ((0,), torch.int64), "radii": ((0,), torch.int32),
              "means2d": ((0, 2), torch.float32), "depths": ((0,), torch.float32), "conics": ((0, 3), torch.float32),
              "opacities": ((0,), torch.float32), "tiles_per_gauss": ((0,), torch.int32), "isect_ids": ((0,), torch.int64),
              "flatten_ids": ((0,), torch.int32)}
    for k, (shape, dtype) in shapes.items():
        assert tuple(info[k].shape) == shape and info[k].dtype == dtype, k
    assert tuple(info["isect_offsets"].shape) == (C, math.ceil(H / 16), math.ceil(W / 16)) and not info["isect_offsets"].any()
    assert not info["last_ids"].any()
    info["means2d"].retain_grad()
    (render.sum() + (alphas ** 2).sum()).backward()
    for k in ("means", "quats", "scales"):
        g = p[k].grad
        assert g is not None and tuple(g.shape) == tuple(p[k].shape), k
        if sparse:
            assert g.is_sparse and g._values().shape[0] == 0, k
        else:
            assert not g.is_sparse and not g.any(), k
    for k in ("opacities", "colors"):
        assert p[k].grad is not None and not p[k].grad.is_sparse and not p[k].grad.any(), k
    assert tuple(info["means2d"].absgrad.shape) == (0, 2)
    if with_bg:  # every pixel shows the whole background
        assert_close(bg.grad.cpu(), torch.full((C, 3), float(H * W)), name="grad backgrounds")


# ---- 8. the default call ----------------------------------------------------------------------------------------------
def test_the_default_call_is_packed(env):
    from edgegaussians_amd import rasterization
    kw, C, N = _proj_inputs("args_eps1", 37)
    kw.pop("backgrounds")
    with torch.no_grad():
        render, alphas, info = rasterization(**kw)  # raised NotImplementedError before packed existed
    assert info["camera_ids"] is not None and info["gaussian_ids"] is not None
    assert info["means2d"].shape == (info["camera_ids"].shape[0], 2)
    assert render.shape == (C, H, W, 3) and float(alphas.max()) > 0


# ---- 9. memory --------------------------------------------------------------------------------------------------------
def test_peak_memory_is_under_half_of_the_dense_projection_outputs(env):
    """C = 4, N = 131072, 64 x 64: every Gaussian projects inside every image, the near / far planes keep the slab
    4.00 <= z <= 4.16 of depths uniform in [2, 6]: a share of 0.04 of the pairs."""
    from edgegaussians_amd import rasterization
    C, N, S = 4, 131072, 64
    g = torch.Generator().manual_seed(5)
    means = torch.cat([torch.rand(N, 2, generator=g) - 0.5, 2.0 + 4.0 * torch.rand(N, 1, generator=g)], dim=-1)
    quats = torch.randn(N, 4, generator=g)
    scales = 0.002 * (0.7 + 0.6 * torch.rand(N, 3, generator=g))
    vms = torch.eye(4).repeat(C, 1, 1)
    vms[:, 0, 3] = torch.tensor([-0.06, -0.02, 0.02, 0.06])
    Ks = torch.tensor([[100.0, 0.0, S / 2], [0.0, 100.0, S / 2], [0.0, 0.0, 1.0]]).repeat(C, 1, 1)
    kw = dict(means=means.cuda(), quats=quats.cuda(), scales=scales.cuda(), opacities=torch.rand(N, generator=g).cuda(),
              colors=torch.rand(N, 3, generator=g).cuda(), viewmats=vms.cuda(), Ks=Ks.cuda(), width=S, height=S,
              near_plane=4.0, far_plane=4.16)
    dense_outputs = 68 * C * N  # the 17 words per pair of _Projection.forward

    def peak(packed):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = rasterization(packed=packed, **kw)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    dense, (_r, _a, di) = peak(False)
    del _r, _a
    packed, (_r, _a, pi) = peak(True)
    nnz = pi["camera_ids"].shape[0]
    share = nnz / (C * N)
    print(f"peak bytes: dense {dense}, packed {packed}; 68 C N = {dense_outputs}; visible share {share:.4f}")
    assert nnz == int((di["radii"] > 0).sum())
    assert 1.0 / 64.0 < share <= 1.0 / 16.0, share
    assert dense >= dense_outputs, "the measurement does not see the dense projection's outputs"
    assert packed <= dense_outputs // 2, (packed, dense_outputs)
    record("packed_peak_memory", cameras=C, gaussians=N, pairs=nnz, dense_bytes=int(dense), packed_bytes=int(packed))
