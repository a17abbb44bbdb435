"""The conditions the device tests of the projection (tests/test_gpu_projection.py) rest on, checked on the CPU with
the references alone: oracle.ref_torch.project in fp32 against itself in float64 on every scene and argument set the
device tests use.  If the fp32 oracle -- a correct fp32 evaluation -- could not meet a bound, or a scene did not reach
the branch it was built for, the device assertion would say nothing about the kernels; here that is ruled out before a
GPU is involved.  The scenes, cases and bounds themselves live in tests/util.py (shared with the device tests)."""
import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import record_cpu

W, H = U.PROJ_SIZE
HALF = 0.5            # the fp32 oracle stays within half of every bound the device is held to
MAX_LOOSE = 0.03      # share of rows whose per-row bound exceeds the project's 1e-4
MAX_BORDER = 0.02     # share of integer-borderline rows (the cap test_projection_forward uses)


def _fp32(ref):
    return U.ref_project_vjps(ref["means"], ref["quats"], ref["scales"], ref["viewmats"], ref["Ks"], W, H,
                              ref["spec"]["args"], ref["cots"], dtype=torch.float32)


def _depths(ref, c):
    vm = ref["viewmats"][c].double()
    return (ref["means"].double() @ vm[:3, :3].T + vm[:3, 3])[:, 2].numpy()


def _cull_counts(ref, c):
    """rows removed by the near plane, the far plane and the radius clip in camera c (float64)"""
    from oracle import ref_torch as O
    a = ref["spec"]["args"]
    z = _depths(ref, c)
    r0 = O.project(ref["means"].double(), ref["quats"].double(), ref["scales"].double(), ref["viewmats"][c], ref["Ks"][c],
                   W, H, a["near_plane"], a["far_plane"], a["eps2d"], 0.0)[0].numpy()
    return int((z < a["near_plane"]).sum()), int((z > a["far_plane"]).sum()), int(((r0 > 0) & ~ref["vis"][c]).sum())


@pytest.mark.parametrize("case", list(U.PROJ_CASES))
def test_fp32_oracle_meets_half_of_every_bound(case):
    ref = U.projection_reference(case)
    spec = ref["spec"]
    outs32, grads32 = _fp32(ref)
    r64, r32 = ref["outs"]["radii"].numpy(), outs32["radii"].numpy()
    C, N = r64.shape
    # integer decisions: identical outside the borderline set, which is small
    assert ref["border"].mean(axis=1).max() <= MAX_BORDER, ref["border"].mean(axis=1)
    assert not ((r32 != r64) & ~ref["border"]).any()
    rows_ok = ((r32 > 0) == (r64 > 0)).all(axis=0)
    cells, loose_max = {}, 0.0
    for cot in spec["cots"]:
        rows = rows_ok & ref["comp_rows"] if cot == "compensations" else rows_ok
        for g in U.PROJ_GRADS:
            ratio, loose, nonzero, _ = U.row_bound_ratio(grads32[cot][g], ref["grads"][cot][g], ref["kappa"][cot][g], rows)
            cells[f"{cot}->{g}"] = ratio
            loose_max = max(loose_max, loose)
            assert nonzero == 0 and ratio <= HALF, (case, cot, g, ratio, nonzero)
            assert loose <= MAX_LOOSE, (case, cot, g, loose)
    fwd = {name: max(U.fwd_row_err(outs32[name][c], ref["outs"][name][c], ref["vis"][c] & rows_ok) for c in range(C))
           for name in U.PROJ_OUTPUTS}
    assert max(fwd.values()) <= HALF * U.FWD_ROW_TOL, fwd
    rec = dict(case=case, gaussians=N, visible=[int(v) for v in ref["vis"].sum(axis=1)], borderline=int(ref["border"].sum()),
               fp32_radius_mismatches=int((r32 != r64).sum()), fp32_ratio_to_bound=cells, loose_share=loose_max, fwd_row_err=fwd)
    if "compensations" in spec["cots"]:
        share = float(ref["comp_rows"].sum() / max(int(ref["vis"].any(axis=0).sum()), 1))
        assert share >= U.COMP_MIN_SHARE, share
        rec["compensation_rows_share"] = share
    if spec["kind"] == "fov":   # every group reaches the screen with most of its rows
        per_group = [int(ref["vis"][0][ref["group"].numpy() == k].sum()) for k in range(len(U.FOV_GROUPS))]
        assert min(per_group) >= 300, per_group
        rec["visible_per_group"] = per_group
    if spec["args"] is not U.PROJ_DEFAULTS:
        a = spec["args"]
        vals = [a["near_plane"], a["far_plane"], a["radius_clip"], a["eps2d"]]
        assert len(set(vals)) == 4 and all(a[k] != U.PROJ_DEFAULTS[k] for k in a), vals
        near, far, clip = _cull_counts(ref, 0)
        assert min(near, far, clip) >= 100 and ref["vis"][0].sum() >= 1000, (near, far, clip, ref["vis"][0].sum())
        rec.update(culled_near=near, culled_far=far, culled_clip=clip)
    if C > 1:
        vis = ref["vis"]
        late = int((~vis[0] & vis[1:].any(axis=0)).sum())     # camera 0 writes zeros, a later camera adds
        never = int((~vis.any(axis=0)).sum())
        assert late >= 100 and never >= 100, (late, never)
        rec.update(culled_in_cam0_visible_later=late, culled_everywhere=never)
    record_cpu("projection_conditions", **rec)


@pytest.mark.parametrize("case", ["fov_cam1", "fov_cam3"])
def test_the_bound_sees_the_fov_clamp(case, monkeypatch):
    """Without the clamp (FOV_CLAMP out of reach) the float64 v_means rows of the clamped groups move by more than the
    per-row bound -- so a backward that ignored the clamp cannot pass -- and the other groups' rows do not move."""
    from oracle import ref_torch as O
    ref = U.projection_reference(case)
    args = (ref["means"], ref["quats"], ref["scales"], ref["viewmats"], ref["Ks"], W, H, ref["spec"]["args"], ref["cots"])
    monkeypatch.setattr(O, "FOV_CLAMP", 1e6)
    outs_nc, grads_nc = U.ref_project_vjps(*args)
    monkeypatch.undo()
    assert O.FOV_CLAMP == 1.3
    want, free = ref["grads"]["conics"]["means"].numpy(), grads_nc["conics"]["means"].numpy()
    both = ref["vis"][0] & (outs_nc["radii"][0].numpy() > 0)
    group = ref["group"].numpy()
    clamped = np.isin(group, U.FOV_CLAMPED_GROUPS) & both
    sigma = np.abs(want).max(axis=1)
    move = np.abs(free - want).max(axis=1) / np.where(sigma > 0, sigma, 1.0)
    bound = U.ROW_FLOOR + U.ROW_KAPPA_FACTOR * ref["kappa"]["conics"]["means"]
    seen = float((move[clamped] > bound[clamped]).mean())
    assert clamped.sum() >= 5 * 300 and seen >= 0.99, (int(clamped.sum()), seen)
    assert (move[~np.isin(group, U.FOV_CLAMPED_GROUPS) & both] == 0).all()
    record_cpu("projection_fov_clamp_sensitivity", case=case, clamped_rows=int(clamped.sum()), share_moved_beyond_bound=seen,
               median_move=float(np.median(move[clamped])))
