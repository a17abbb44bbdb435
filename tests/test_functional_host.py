"""The functional API (edgegaussians_amd/functional.py, re-exported by the gsplat shim) as far as it can be checked
without a device: the exported names, the argument checks of the new native entries, the two plain-torch stages against
an independent restatement, and -- with the references alone -- the conditions the device tests of the projection from
covariances (tests/test_gpu_functional.py) rest on: the restated float64 reference equals oracle.ref_torch.project, a
correct fp32 evaluation stays within half of every bound, the borderline and loose sets are small."""
import numpy as np
import pytest
import torch

from tests import functional_util as F
from tests import util as U
from tests.util import record_cpu

W, H = U.PROJ_SIZE
HALF = 0.5            # the fp32 reference stays within half of every bound the device is held to
MAX_LOOSE = 0.03      # share of rows whose per-row bound exceeds the project's 1e-4
MAX_BORDER = 0.02     # share of integer-borderline rows per camera (the cap tests/test_gpu_projection.py applies)
NAMES = ("fully_fused_projection", "quat_scale_to_covar_preci", "isect_tiles", "isect_offset_encode", "rasterize_to_pixels",
         "world_to_cam", "persp_proj")


def test_the_shim_exports_the_functional_api():
    import gsplat
    for name in NAMES + ("rasterization", "spherical_harmonics"):
        assert callable(getattr(gsplat, name)), name
        assert name in gsplat.__all__, name


def test_new_entries_reject_null_pointers_by_name():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    h = _lib.load(require_device=False)
    calls = {
        "eg_quat_scale_to_covar_preci_fwd": (None, None, 4, 0, None, None, None),
        "eg_quat_scale_to_covar_preci_bwd": (None, None, 4, 1, None, None, None, None, None),
        "eg_project_covars_fwd_cams": (None, None, None, None, 4, 1, 32, 32, 0.01, 1e10, 0.3, 0.0, None, None, None, None, None, None),
        "eg_project_covars_bwd_cams": (None, None, None, None, 4, 1, 32, 32, 0.3, None, None, None, None, None, None, None, None),
        "eg_isect_offset_encode": (None, 4, 1, 2, 2, None, None),
    }
    for name, args in calls.items():
        assert getattr(h, name)(*args) == -1, name
        assert name.encode() in h.eg_last_error_string(), (name, h.eg_last_error_string())
    # bad sizes are refused before the pointers are looked at; nothing to do is a success
    assert h.eg_project_covars_fwd_cams(None, None, None, None, 4, 0, 32, 32, 0.01, 1e10, 0.3, 0.0, None, None, None, None, None, None) == -1
    assert h.eg_isect_offset_encode(None, -1, 1, 2, 2, None, None) == -1
    assert h.eg_isect_offset_encode(None, 0, 1, 2, 2, None, None) == -1    # (M == 0 still fills `offsets`)
    assert h.eg_quat_scale_to_covar_preci_fwd(None, None, 0, 0, None, None, None) == 0
    assert h.eg_quat_scale_to_covar_preci_bwd(None, None, 0, 0, None, None, None, None, None) == 0
    assert h.eg_project_covars_fwd_cams(None, None, None, None, 0, 1, 32, 32, 0.01, 1e10, 0.3, 0.0, None, None, None, None, None, None) == 0
    assert h.eg_project_covars_bwd_cams(None, None, None, None, 0, 1, 32, 32, 0.3, None, None, None, None, None, None, None, None) == 0


def test_kernel_backed_functions_refuse_cpu_tensors_and_bad_arguments():
    import gsplat
    z = torch.zeros
    vm, K = torch.eye(4)[None], torch.eye(3)[None]
    with pytest.raises(ValueError, match="device tensor"):
        gsplat.quat_scale_to_covar_preci(z(4, 4), z(4, 3))
    with pytest.raises(ValueError, match="device tensor"):
        gsplat.fully_fused_projection(z(4, 3), z(4, 6), None, None, vm, K, 32, 32)
    with pytest.raises(ValueError, match="device tensor"):
        gsplat.isect_tiles(z(1, 4, 2), z(1, 4, dtype=torch.int32), z(1, 4), 16, 2, 2)
    with pytest.raises(ValueError, match="device tensor"):
        gsplat.isect_offset_encode(z(4, dtype=torch.int64), 1, 2, 2)
    with pytest.raises(ValueError, match="device tensor"):
        gsplat.rasterize_to_pixels(z(1, 4, 2), z(1, 4, 3), z(1, 4, 3), z(1, 4), 32, 32, 16, z(1, 2, 2, dtype=torch.int32),
                                   z(0, dtype=torch.int32))
    for covars, quats, scales in ((None, None, None), (z(4, 6), z(4, 4), z(4, 3)), (None, z(4, 4), None), (z(4, 6), None, z(4, 3))):
        with pytest.raises(ValueError, match="exactly one"):
            gsplat.fully_fused_projection(z(4, 3), covars, quats, scales, vm, K, 32, 32)
    # the corners that are out of scope say so before anything else is looked at
    with pytest.raises(NotImplementedError, match="packed=True"):
        gsplat.fully_fused_projection(z(4, 3), z(4, 6), None, None, vm, K, 32, 32, packed=True)
    with pytest.raises(NotImplementedError, match="sparse_grad"):
        gsplat.fully_fused_projection(z(4, 3), z(4, 6), None, None, vm, K, 32, 32, sparse_grad=True)
    with pytest.raises(NotImplementedError, match="packed=True"):
        gsplat.isect_tiles(z(1, 4, 2), z(1, 4, dtype=torch.int32), z(1, 4), 16, 2, 2, packed=True)
    with pytest.raises(NotImplementedError, match="sort=False"):
        gsplat.isect_tiles(z(1, 4, 2), z(1, 4, dtype=torch.int32), z(1, 4), 16, 2, 2, sort=False)
    with pytest.raises(NotImplementedError, match="tile_size"):
        gsplat.isect_tiles(z(1, 4, 2), z(1, 4, dtype=torch.int32), z(1, 4), 12, 2, 2)
    ras = (z(1, 4, 2), z(1, 4, 3), z(1, 4, 3), z(1, 4), 32, 32)
    with pytest.raises(NotImplementedError, match="packed=True"):
        gsplat.rasterize_to_pixels(*ras, 16, z(1, 2, 2, dtype=torch.int32), z(0, dtype=torch.int32), packed=True)
    with pytest.raises(NotImplementedError, match="masks"):
        gsplat.rasterize_to_pixels(*ras, 16, z(1, 2, 2, dtype=torch.int32), z(0, dtype=torch.int32), masks=z(1, 2, 2, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="tile_size"):
        gsplat.rasterize_to_pixels(*ras, 64, z(1, 1, 1, dtype=torch.int32), z(0, dtype=torch.int32))


def _scene64(n=400, cams=(0, 1, 3), seed=5):
    from oracle import ref_torch as O
    vms, Ks = U.projection_cameras()
    gen = torch.Generator().manual_seed(seed)
    means, quats, scales, _ = U.camera_space_scene(vms[0], Ks[0], W, H, (U.INSIDE_GROUP,), n, 0.02, gen)
    covars = O.quat_scale_to_covar(quats.double(), scales.double())
    return means.double(), quats.double(), scales.double(), covars, vms[list(cams)].double(), Ks[list(cams)].double()


def test_world_to_cam_and_persp_proj_against_an_einsum_restatement():
    """CPU float64, three cameras (two of which see the scene built for camera 0 partly outside the 1.3 tan-fov limit:
    the clamp is live), to 1e-12 relative; gradients flow to every input."""
    import gsplat
    means, _q, _s, covars, vms, Ks = _scene64()
    p = [t.clone().requires_grad_(True) for t in (means, covars, vms)]
    means_c, covars_c = gsplat.world_to_cam(*p)
    C, N = vms.shape[0], means.shape[0]
    assert means_c.shape == (C, N, 3) and covars_c.shape == (C, N, 3, 3)
    R, t = vms[:, :3, :3], vms[:, :3, 3]
    want_m = (R[:, None] @ means[None, :, :, None])[..., 0] + t[:, None]
    want_c = R[:, None] @ covars[None] @ R[:, None].transpose(-1, -2)
    assert U.rel_err(means_c, want_m) <= 1e-12 and U.rel_err(covars_c, want_c) <= 1e-12
    g = torch.autograd.grad(means_c.sum() + (covars_c ** 2).sum(), p)
    assert all(gi.abs().max() > 0 for gi in g)

    means2d, covars2d = gsplat.persp_proj(means_c.detach(), covars_c.detach(), Ks, W, H)
    assert means2d.shape == (C, N, 2) and covars2d.shape == (C, N, 2, 2)
    fx, fy, cx, cy = Ks[:, 0, 0, None], Ks[:, 1, 1, None], Ks[:, 0, 2, None], Ks[:, 1, 2, None]
    x, y, z = want_m.unbind(-1)
    lx, ly = 1.3 * 0.5 * W / fx, 1.3 * 0.5 * H / fy
    xc, yc = z * (x / z).clamp(-lx, lx), z * (y / z).clamp(-ly, ly)
    assert ((x / z).abs() > lx).any() or ((y / z).abs() > ly).any()      # the clamp is exercised
    J = torch.zeros(C, N, 2, 3, dtype=torch.float64)
    J[..., 0, 0], J[..., 1, 1] = fx / z, fy / z
    J[..., 0, 2], J[..., 1, 2] = -fx * xc / z ** 2, -fy * yc / z ** 2
    want2 = torch.einsum("cnij,cnjk,cnlk->cnil", J, want_c, J)
    assert U.rel_err(covars2d, want2) <= 1e-12
    assert U.rel_err(means2d, torch.stack([fx * x / z + cx, fy * y / z + cy], -1)) <= 1e-12
    assert torch.equal(covars2d, covars2d.transpose(-1, -2)) or U.rel_err(covars2d, covars2d.transpose(-1, -2)) <= 1e-14


def test_persp_proj_gives_the_oracles_cov2d():
    """persp_proj(world_to_cam(...)) + eps2d on the diagonal is the cov2d inside oracle.ref_torch.project: the oracle
    does not return it, so it is recovered from the oracle's conic (conic = inverse(cov2d + eps2d I)), on an
    inside-screen scene seen by its own camera."""
    import gsplat
    from oracle import ref_torch as O
    means, quats, scales, covars, vms, Ks = _scene64(cams=(0,))
    eps2d = 0.3
    radii, _m2d, _d, conics, _comp = O.project(means, quats, scales, vms[0], Ks[0], W, H, eps2d=eps2d)
    assert (radii > 0).all()
    means_c, covars_c = gsplat.world_to_cam(means, covars, vms)
    m2d, cov2d = gsplat.persp_proj(means_c, covars_c, Ks, W, H)
    B = cov2d[0] + eps2d * torch.eye(2, dtype=torch.float64)
    a, b, c = conics.unbind(-1)
    det = a * c - b * b
    want = torch.stack([c / det, -b / det, -b / det, a / det], -1).reshape(-1, 2, 2)
    assert U.rel_err(B, want) <= 1e-12
    assert U.rel_err(m2d[0], _m2d) <= 1e-12


@pytest.mark.parametrize("case", F.COVAR_CASES)
def test_the_restated_reference_is_the_oracle(case):
    """ref_project_covars fed triu(quat_scale_to_covar(q, s)) in float64 equals oracle.ref_torch.project(q, s): the
    restatement is proven before it judges a kernel."""
    from oracle import ref_torch as O
    spec, means, _cv, quats, scales, vms, Ks, _ = F.covars_inputs(case)
    a = spec["args"]
    c64 = F.triu6(O.quat_scale_to_covar(quats.double(), scales.double()))
    for c in range(vms.shape[0]):
        want = O.project(means.double(), quats.double(), scales.double(), vms[c], Ks[c], W, H, a["near_plane"], a["far_plane"],
                         a["eps2d"], a["radius_clip"])
        got = F.ref_project_covars(means.double(), c64, vms[c], Ks[c], W, H, a["near_plane"], a["far_plane"], a["eps2d"],
                                   a["radius_clip"])
        # (an integer decision may differ only where the two float64 evaluations straddle a threshold: nowhere here)
        assert torch.equal(got[0], want[0])
        assert (want[0] > 0).sum() >= 1000
        for name, g, w in zip(U.PROJ_OUTPUTS, got[1:], want[1:]):
            assert U.fwd_row_err(g, w, (want[0] > 0).numpy()) <= 1e-12, (case, c, name)


@pytest.mark.parametrize("case", F.COVAR_CASES)
def test_fp32_reference_meets_half_of_every_bound(case):
    """The bounds of the device test are the project's own (FWD_ROW_TOL per forward row, the kappa bound per gradient
    row), unchanged: the fp32 evaluation of the reference stays within half of each on every case (measured: forward
    <= 1.5e-6 of the 2e-5, gradients <= 0.13 of the bound), so no forward output needs the kappa form and no case is
    dropped.  Borderline rows <= 2 % per camera, loose rows <= 3 %."""
    ref = F.covars_reference(case)
    spec = ref["spec"]
    outs32, grads32 = F.ref_covars_vjps(ref["means"], ref["covars"], ref["viewmats"], ref["Ks"], spec["args"], ref["cots"],
                                        dtype=torch.float32)
    r64, r32 = ref["outs"]["radii"].numpy(), outs32["radii"].numpy()
    C, N = r64.shape
    assert ref["border"].mean(axis=1).max() <= MAX_BORDER, ref["border"].mean(axis=1)
    assert not ((r32 != r64) & ~ref["border"]).any()
    assert ref["vis"].sum(axis=1).min() >= 1000
    rows_ok = ((r32 > 0) == (r64 > 0)).all(axis=0)
    cells, loose_max = {}, 0.0
    for cot in spec["cots"]:
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in F.COVAR_GRADS:
            ratio, loose, nonzero, _ = U.row_bound_ratio(grads32[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g], rows)
            cells[f"{cot}->{g}"] = ratio
            loose_max = max(loose_max, loose)
            assert nonzero == 0 and ratio <= HALF, (case, cot, g, ratio, nonzero)
            assert loose <= MAX_LOOSE, (case, cot, g, loose)
    fwd = {name: max(U.fwd_row_err(outs32[name][c], ref["outs"][name][c], ref["vis"][c] & rows_ok) for c in range(C))
           for name in U.PROJ_OUTPUTS}
    assert max(fwd.values()) <= HALF * U.FWD_ROW_TOL, fwd
    if "compensations" in spec["cots"]:
        assert ref["comp_rows"].sum() / max(int(ref["vis"].any(axis=0).sum()), 1) >= U.COMP_MIN_SHARE
    # the covariance cotangents that must vanish do: means2d and depths do not depend on the covariance
    for cot in ("means2d", "depths"):
        if cot in spec["cots"]:
            assert not ref["grads"][cot]["covars"].any()
    record_cpu("functional_covars_conditions", case=case, gaussians=N, visible=[int(v) for v in ref["vis"].sum(axis=1)],
               borderline=int(ref["border"].sum()), fp32_radius_mismatches=int((r32 != r64).sum()), fp32_ratio_to_bound=cells,
               loose_share=loose_max, fwd_row_err=fwd)


def test_quat_scale_reference_conditions():
    """The float64 reference of quat_scale_to_covar_preci in fp32 stays within half of the per-row kappa bound on the
    largest size and both scale bases, full and upper-triangle forms (forward rows: (ROW_FLOOR + 32 kappa) of the row
    maximum as well -- the entries of R diag(s^2) R^T cancel against each other, which FWD_ROW_TOL does not allow for)."""
    for base in F.QS_BASES:
        for triu in (False, True):
            ref = F.qs_reference(1000, base, triu)
            q, s = ref["quats"], ref["scales"]
            p = [q.clone().requires_grad_(True), s.clone().requires_grad_(True)]
            outs = dict(zip(("covars", "precis"), F.ref_quat_scale_to_covar_preci(p[0], p[1], triu, dtype=torch.float32)))
            for k in outs:
                ratio, loose, _, _ = U.row_bound_ratio(outs[k].detach().reshape(1000, -1), ref["outs"][k].reshape(1000, -1), ref["kappa_fwd"][k])
                assert ratio <= HALF and loose <= MAX_LOOSE, (base, triu, k, ratio, loose)
                g = torch.autograd.grad(outs[k], p, ref["cots"][k], retain_graph=True)
                for name, gi in zip(("quats", "scales"), g):
                    ratio, loose, nonzero, _ = U.row_bound_ratio(gi, ref["grads"][k][name], ref["kappa"][k][name])
                    assert nonzero == 0 and ratio <= HALF and loose <= MAX_LOOSE, (base, triu, k, name, ratio, loose)
            if triu:   # the convention: an off-diagonal cotangent stands for both symmetric entries
                full = F.qs_reference(1000, base, False)
                assert torch.equal(ref["outs"]["covars"], F.triu6(full["outs"]["covars"]))
