"""The orthographic camera (camera_model="ortho") as far as it can be checked without a device: the float64 reference
of tests/ortho_util.py against the pinhole oracle seen from far away and against the model's closed-form VJP, the
conditions the device tests (tests/test_gpu_ortho.py) rest on -- with the references alone --, `proj`, the argument
checks of `rasterization` and `fully_fused_projection` on CPU tensors, and the argument checks of the new native entry
pair."""
import numpy as np
import pytest
import torch

from tests import functional_util as F
from tests import ortho_util as OU
from tests import util as U
from tests.util import record_cpu

W, H = U.PROJ_SIZE
HALF = 0.5            # the fp32 reference stays within half of every bound the device is held to
MAX_LOOSE = 0.03      # share of rows whose per-row bound exceeds the project's 1e-4 (U.ROW_LOOSE)
MAX_BORDER = 0.02     # share of integer-borderline rows per camera
Z0 = 1e6


@pytest.mark.parametrize("args_name", list(OU.ARGS))
def test_a_pinhole_camera_far_away_gives_the_ortho_reference(args_name):
    """oracle.ref_torch.project with the camera moved back to z0 = 1e6 from the scene centre along its own axis and
    fx = fx_o z0 differs from the orthographic reference by (z - d) / z0 to first order: means2d, conics and
    compensations agree to 4 extent / z0 (relative to the tensor's largest entry) on the rows both keep, the integer
    radii are equal outside the borderline set.  The planes are the defaults for both (a depth of 1e6 is beyond 4.2)."""
    from oracle import ref_torch as O
    ref = OU.reference("quats", args_name, 1)
    a = dict(ref["args"], near_plane=0.01, far_plane=1e10)
    means, quats, scales = (t.double() for t in ref["inputs"])
    vm, K = ref["viewmats"][0].double(), ref["Ks"][0].double()
    vm_far = vm.clone()
    vm_far[2, 3] += Z0 - OU.CENTRE_DEPTH
    K_far = K.clone()
    K_far[0, 0], K_far[1, 1] = K[0, 0] * Z0, K[1, 1] * Z0
    cull = (a["near_plane"], a["far_plane"], a["eps2d"], a["radius_clip"])
    got = OU.ref_project_ortho(means, quats, scales, vm, K, W, H, *cull)
    want = O.project(means, quats, scales, vm_far, K_far, W, H, *cull)
    both = (got[0] > 0) & (want[0] > 0)
    assert both.sum() >= 500
    tol = 4.0 * ref["extent"] / Z0
    errs = {}
    for name, g, w in zip(U.PROJ_OUTPUTS, got[1:], want[1:]):
        if name == "depths":
            continue   # (z against z + z0 - d: the models' depths differ by construction)
        errs[name] = U.rel_err(g[both], w[both])
        assert errs[name] <= tol, (name, errs[name], tol)
    cov6 = F.triu6(O.quat_scale_to_covar(quats, scales))
    border = OU.ortho_borderline(means, cov6, vm, K, W, H, a)
    differ = (got[0] != want[0]).numpy() & both.numpy()
    assert not (differ & ~border).any(), int((differ & ~border).sum())
    record_cpu("ortho_reference_vs_far_pinhole", args=args_name, rows=int(both.sum()), rel_err=errs, tol=tol,
               radii_differ_inside_borderline=int(differ.sum()))


def test_the_closed_form_vjp_is_autograd_of_the_plain_expression():
    """mean2d = (fx x + cx, fy y + cy), cov2d = J cc J^T with J = [[fx, 0, 0], [0, fy, 0]]: v_mean_c = (fx v_u, fy v_v,
    v_depth), v_cc = J^T v_cov2d J (only the 00, 01, 10, 11 entries are non-zero), c00 = fx^2 cc00, c01 = fx fy cc01,
    c11 = fy^2 cc11."""
    gen = torch.Generator().manual_seed(3)
    n = 50
    fx, fy, cx, cy = 74.1, 61.3, 99.5, 67.5
    mean_c = torch.randn(n, 3, generator=gen, dtype=torch.float64).requires_grad_(True)
    A = torch.randn(n, 3, 3, generator=gen, dtype=torch.float64)
    cc = (A @ A.transpose(-1, -2)).requires_grad_(True)
    J = torch.tensor([[fx, 0.0, 0.0], [0.0, fy, 0.0]], dtype=torch.float64)
    cov2d = J @ cc @ J.T
    mean2d = torch.stack([fx * mean_c[:, 0] + cx, fy * mean_c[:, 1] + cy], -1)
    depth = mean_c[:, 2]
    want = torch.stack([fx * fx * cc[:, 0, 0], fx * fy * cc[:, 0, 1], fx * fy * cc[:, 1, 0], fy * fy * cc[:, 1, 1]], -1)
    assert U.rel_err(cov2d.reshape(n, 4), want) <= 1e-14
    v_uv = torch.randn(n, 2, generator=gen, dtype=torch.float64)
    v_d = torch.randn(n, generator=gen, dtype=torch.float64)
    v_cov = torch.randn(n, 2, 2, generator=gen, dtype=torch.float64)
    g_mean, g_cc = torch.autograd.grad([mean2d, depth, cov2d], [mean_c, cc], [v_uv, v_d, v_cov])
    assert U.rel_err(g_mean, torch.stack([fx * v_uv[:, 0], fy * v_uv[:, 1], v_d], -1)) <= 1e-14
    v_cc = J.T @ v_cov @ J
    assert U.rel_err(g_cc, v_cc) <= 1e-14
    assert not v_cc[:, 2, :].any() and not v_cc[:, :, 2].any()


def test_the_per_gaussian_viewmat_gives_the_whole_call_pose_gradient():
    """ortho_util.pose_reference's device (one viewmat per Gaussian) sums to autograd's gradient with respect to the one
    viewmat, with a bottom row of zeros."""
    G, bottom = OU.pose_reference("eps1", 3)
    ref = OU.reference("quats", "eps1", 3)
    a = ref["args"]
    p = [t.double() for t in ref["inputs"]]
    assert bottom == 0.0
    for c in range(3):
        vm = ref["viewmats"][c].double().clone().requires_grad_(True)
        out = OU.ref_project_ortho(p[0], p[1], p[2], vm, ref["Ks"][c].double(), W, H, a["near_plane"], a["far_plane"],
                                   a["eps2d"], a["radius_clip"])
        for k, cot in ref["cots"].items():
            y = out[1 + U.PROJ_OUTPUTS.index(k)]
            g = torch.autograd.grad(y, vm, cot[c].double().reshape(y.shape), retain_graph=True)[0]
            S = G[k][c].abs().sum(0)
            assert float(((g[:3] - G[k][c].sum(0)).abs() / S.clamp(min=1e-300)).max()) <= 1e-12, (c, k)
            assert not g[3].any()
    # culled pairs contribute exactly nothing
    vis = torch.from_numpy(ref["vis"])
    for k in G:
        assert not G[k][~vis].any()


@pytest.mark.parametrize("form", list(OU.FORMS))
@pytest.mark.parametrize("args_name,n_cams", OU.CASES)
def test_fp32_reference_meets_half_of_every_bound(form, args_name, n_cams):
    """The bounds of the device tests are the project's own (U.FWD_ROW_TOL per forward row, the kappa bound of
    U.row_bound_check per gradient row), unchanged: an fp32 torch evaluation of the reference stays within half of each,
    at most 3 % of the rows have a bound above U.ROW_LOOSE, at most 2 % per camera are integer-borderline, and the fp32
    evaluation takes the float64 one's integer decisions outside that set.  Every group of the scene does what it is
    there for."""
    ref = OU.reference(form, args_name, n_cams)
    outs32, grads32 = OU.ref_vjps(form, ref["inputs"], ref["viewmats"], ref["Ks"], ref["args"], ref["cots"], dtype=torch.float32)
    r64, r32 = ref["outs"]["radii"].numpy(), outs32["radii"].numpy()
    C, N = r64.shape
    assert N == OU.N_FULL and C == n_cams
    assert ref["border"].mean(axis=1).max() <= MAX_BORDER, ref["border"].mean(axis=1)
    assert not ((r32 != r64) & ~ref["border"]).any()
    rows_ok = ((r32 > 0) == (r64 > 0)).all(axis=0)
    cells, loose_max = {}, 0.0
    for cot in ref["cots"]:
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in ref["names"]:
            ratio, loose, nonzero, _ = U.row_bound_ratio(grads32[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g], rows)
            cells[f"{cot}->{g}"] = ratio
            loose_max = max(loose_max, loose)
            assert nonzero == 0 and ratio <= HALF, (cot, g, ratio, nonzero)
            assert loose <= MAX_LOOSE, (cot, g, loose)
    fwd = {name: max(U.fwd_row_err(outs32[name][c], ref["outs"][name][c], ref["vis"][c] & rows_ok) for c in range(C))
           for name in U.PROJ_OUTPUTS}
    assert max(fwd.values()) <= HALF * U.FWD_ROW_TOL, fwd
    # the groups, in the camera the scene is built for
    group, vis0, r0 = ref["group"].numpy(), ref["vis"][0], r64[0]
    per = {name: (int(vis0[group == k].sum()), int((group == k).sum())) for k, name in enumerate(OU.GROUP_NAMES)}
    off = args_name != "defaults"
    assert per["inside"][0] == per["inside"][1] >= 200
    means2d = ref["outs"]["means2d"][0].numpy()
    for name, axis, lim in (("left", 0, 0.0), ("right", 0, float(W)), ("top", 1, 0.0), ("bottom", 1, float(H))):
        sel = (group == OU.GROUP_NAMES.index(name)) & vis0
        assert per[name][0] == per[name][1] >= 50
        m = means2d[sel][:, axis]
        assert (m < lim).any() and (m > lim).any(), name          # centres on both sides of the edge
        assert (np.abs(m - lim) < r0[sel]).all(), name            # every footprint crosses it
    assert per["outside"][0] == 0 and per["near"][0] == 0 and per["outside"][1] >= 50 and per["near"][1] >= 50
    for name in ("near_finite", "far_finite", "tiny"):   # culled by the finite planes / radius_clip, visible at the defaults
        assert per[name][1] >= 50 and per[name][0] == (0 if off else per[name][1]), (name, per[name])
    for cot in ("means2d", "depths"):   # neither depends on the covariance
        if form == "covars":
            assert not ref["grads"][cot]["covars"].any()
    if args_name != "eps0.05":   # (radius_clip 6.5 removes every Gaussian of the size of eps2d = 0.05)
        assert ref["comp_rows"].sum() >= 100
    record_cpu("ortho_reference_conditions", form=form, args=args_name, cameras=C, visible=[int(v) for v in ref["vis"].sum(axis=1)],
               borderline=int(ref["border"].sum()), fp32_ratio_to_bound=cells, loose_share=loose_max, fwd_row_err=fwd,
               comp_rows=int(ref["comp_rows"].sum()))


def test_proj():
    """`proj`: the ortho branch against an einsum restatement in float64 (1e-12), the pinhole branch torch.equal to
    persp_proj; exported by the package, the shim and its __all__; FLAG_ORTHO is the header's bit."""
    import gsplat
    from edgegaussians_amd import _lib, functional
    assert "proj" in gsplat.__all__ and "proj" in functional.__all__ and gsplat.proj is functional.proj
    assert _lib.FLAG_ORTHO == 128
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "edgegs.h")).read()
    assert re.search(r"#define EG_FLAG_ORTHO 128u", hdr)
    gen = torch.Generator().manual_seed(5)
    C, N = 3, 40
    means_c = torch.randn(C, N, 3, generator=gen, dtype=torch.float64) + torch.tensor([0.0, 0.0, 4.0], dtype=torch.float64)
    A = torch.randn(C, N, 3, 3, generator=gen, dtype=torch.float64)
    covars_c = A @ A.transpose(-1, -2)
    Ks = torch.eye(3, dtype=torch.float64).repeat(C, 1, 1)
    Ks[:, 0, 0] = torch.tensor([74.1, 50.0, 120.5], dtype=torch.float64)
    Ks[:, 1, 1] = torch.tensor([61.3, 55.0, 110.5], dtype=torch.float64)
    Ks[:, 0, 2], Ks[:, 1, 2] = 99.5, 67.5
    p = [means_c.clone().requires_grad_(True), covars_c.clone().requires_grad_(True)]
    m2d, c2d = gsplat.proj(p[0], p[1], Ks, W, H, camera_model="ortho")
    assert m2d.shape == (C, N, 2) and c2d.shape == (C, N, 2, 2)
    J = torch.zeros(C, 2, 3, dtype=torch.float64)
    J[:, 0, 0], J[:, 1, 1] = Ks[:, 0, 0], Ks[:, 1, 1]
    want_c = torch.einsum("cij,cnjk,clk->cnil", J, covars_c, J)
    want_m = torch.einsum("cij,cnj->cni", J, means_c) + Ks[:, None, :2, 2]
    assert U.rel_err(c2d, want_c) <= 1e-12 and U.rel_err(m2d, want_m) <= 1e-12
    g = torch.autograd.grad(m2d.sum() + (c2d ** 2).sum(), p)
    assert all(gi.abs().max() > 0 for gi in g)
    assert not g[0][..., 2].any()   # nothing depends on z
    # width and height play no part
    m2, c2 = gsplat.proj(means_c, covars_c, Ks, 7, 3, camera_model="ortho")
    assert torch.equal(m2, m2d.detach()) and torch.equal(c2, c2d.detach())
    for a, b in zip(gsplat.proj(means_c, covars_c, Ks, W, H), gsplat.persp_proj(means_c, covars_c, Ks, W, H)):
        assert torch.equal(a, b)
    for a, b in zip(gsplat.proj(means_c, covars_c, Ks, W, H, "pinhole"), gsplat.persp_proj(means_c, covars_c, Ks, W, H)):
        assert torch.equal(a, b)
    with pytest.raises(NotImplementedError, match="fisheye"):
        gsplat.proj(means_c, covars_c, Ks, W, H, camera_model="fisheye")
    with pytest.raises(ValueError, match="Unknown camera_model: bogus"):
        gsplat.proj(means_c, covars_c, Ks, W, H, camera_model="bogus")


def test_proj_is_the_reference_cov2d():
    """proj(world_to_cam(...), "ortho") + eps2d on the diagonal is the cov2d inside ref_project_ortho, recovered from
    its conic, and its means2d are the reference's."""
    import gsplat
    from oracle import ref_torch as O
    ref = OU.reference("quats", "defaults", 1)
    means, quats, scales = (t.double() for t in ref["inputs"])
    vms, Ks = ref["viewmats"].double(), ref["Ks"].double()
    radii, m2d_ref, _d, conics, _c = OU.ref_project_ortho(means, quats, scales, vms[0], Ks[0], W, H)
    vis = radii > 0
    means_c, covars_c = gsplat.world_to_cam(means, O.quat_scale_to_covar(quats, scales), vms)
    m2d, cov2d = gsplat.proj(means_c, covars_c, Ks, W, H, camera_model="ortho")
    B = cov2d[0] + 0.3 * torch.eye(2, dtype=torch.float64)
    a, b, c = conics[vis].unbind(-1)
    det = a * c - b * b
    want = torch.stack([c / det, -b / det, -b / det, a / det], -1).reshape(-1, 2, 2)
    assert U.rel_err(B[vis], want) <= 1e-12
    assert U.rel_err(m2d[0][vis], m2d_ref[vis]) <= 1e-12


def test_camera_model_is_checked_before_any_tensor():
    """CPU tensors: "fisheye" and an unknown model are refused before the device check that would refuse the tensors;
    "pinhole" and "ortho" get as far as that check."""
    import gsplat
    z = torch.zeros
    vm, K = torch.eye(4)[None], torch.eye(3)[None]
    ras = (z(4, 3), z(4, 4), z(4, 3), z(4), torch.ones(4, 3), vm, K, 32, 32)
    ffp_q = (z(4, 3), None, z(4, 4), z(4, 3), vm, K, 32, 32)
    ffp_c = (z(4, 3), z(4, 6), None, None, vm, K, 32, 32)
    for fn, args in ((gsplat.rasterization, ras), (gsplat.fully_fused_projection, ffp_q), (gsplat.fully_fused_projection, ffp_c)):
        with pytest.raises(NotImplementedError, match="fisheye"):
            fn(*args, camera_model="fisheye")
        with pytest.raises(ValueError, match="Unknown camera_model: bogus"):
            fn(*args, camera_model="bogus")
        for model in ("pinhole", "ortho"):
            with pytest.raises(ValueError, match="device tensor"):
                fn(*args, camera_model=model)
    # the model is looked at first: before the tile size, and before the functional stages' refusals
    with pytest.raises(NotImplementedError, match="fisheye"):
        gsplat.rasterization(*ras, tile_size=12, camera_model="fisheye")
    with pytest.raises(ValueError, match="Unknown camera_model"):
        gsplat.fully_fused_projection(*ffp_c, packed=True, camera_model="bogus")
    # ... which stay exactly as they are
    with pytest.raises(NotImplementedError, match="packed=True"):
        gsplat.fully_fused_projection(*ffp_c, packed=True, camera_model="ortho")
    with pytest.raises(NotImplementedError, match="sparse_grad"):
        gsplat.fully_fused_projection(*ffp_q, sparse_grad=True, camera_model="ortho")
    # appended last: the positional call written for gsplat 1.0.0 keeps its meaning
    import inspect
    assert list(inspect.signature(gsplat.rasterization).parameters)[-2:] == ["channel_chunk", "camera_model"]
    assert list(inspect.signature(gsplat.fully_fused_projection).parameters)[-1] == "camera_model"
    assert inspect.signature(gsplat.rasterization).parameters["camera_model"].default == "pinhole"


def test_new_entry_pair_checks_its_arguments():
    """eg_project_covars_{fwd,bwd}_cams_flags: null pointers by name, C = 0 refused, N = 0 nothing to do, unknown flag
    bits refused; the entries of the training path refuse EG_FLAG_ORTHO instead of ignoring it."""
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    h = _lib.load(require_device=False)
    ORTHO = _lib.FLAG_ORTHO
    fwd = lambda n, c, flags: h.eg_project_covars_fwd_cams_flags(None, None, None, None, n, c, 32, 32, 0.01, 1e10, 0.3, 0.0,
                                                                 None, None, None, None, None, flags, None)
    bwd = lambda n, c, flags: h.eg_project_covars_bwd_cams_flags(None, None, None, None, n, c, 32, 32, 0.3, None, None, None,
                                                                 None, None, None, None, flags, None)
    for name, fn in (("eg_project_covars_fwd_cams_flags", fwd), ("eg_project_covars_bwd_cams_flags", bwd)):
        for flags in (0, ORTHO):
            assert fn(4, 1, flags) == -1
            assert name.encode() in h.eg_last_error_string() and b"null pointer" in h.eg_last_error_string()
            assert fn(4, 0, flags) == -1 and b"bad sizes" in h.eg_last_error_string()
            assert fn(0, 1, flags) == 0
        assert fn(0, 1, ORTHO | _lib.FLAG_ANTIALIASED) == -1 and b"flags" in h.eg_last_error_string()
    # entries that take caller flags and do not implement the bit
    assert h.eg_project_bin(*([None] * 6), 4, 32, 32, ORTHO | _lib.FLAG_TIGHT_TILES, None, None, None, 0, None, None, None, None, None) == -1
    assert b"eg_project_bin" in h.eg_last_error_string() and b"EG_FLAG_ORTHO" in h.eg_last_error_string()
    assert h.eg_project_emit(*([None] * 6), 4, 32, 32, ORTHO | _lib.FLAG_TIGHT_TILES, None, None, 128, None, None, 16, None, None, None) == -1
    assert b"eg_project_emit" in h.eg_last_error_string() and b"EG_FLAG_ORTHO" in h.eg_last_error_string()
    hy = _lib.AdamHyper()
    hy.step = 1
    assert h.eg_project_bwd_adam(*([None] * 6), 4, 32, 32, 0.3, ORTHO, None, None, None, None, None, hy, None) == -1
    assert b"eg_project_bwd_adam" in h.eg_last_error_string() and b"EG_FLAG_ORTHO" in h.eg_last_error_string()
    assert h.eg_backward_fused(*([None] * 6), 4, 32, 32, 0.3, ORTHO, *([None] * 10), None, None) == -1
    assert b"eg_backward_fused" in h.eg_last_error_string() and b"EG_FLAG_ORTHO" in h.eg_last_error_string()
    a = _lib.OperatorArgs()
    a.N, a.width, a.height, a.seg_cap, a.max_items, a.flags = 4, 32, 32, 128, 16, ORTHO
    import ctypes
    assert h.eg_operator_fwd(ctypes.byref(a), None) == -1
    assert b"eg_operator_fwd" in h.eg_last_error_string() and b"EG_FLAG_ORTHO" in h.eg_last_error_string()
