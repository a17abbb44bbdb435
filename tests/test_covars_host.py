"""`rasterization(covars=[N, 3, 3])` on the CPU: the argument checks (they run before any device call), the [N, 3, 3]
gradient convention on the float64 reference alone, and the conditions that tests/test_gpu_covars.py relies on, asserted
from the references alone (tests/covars_util.py)."""
import numpy as np
import pytest
import torch

from tests import covars_util as CU
from tests import functional_util as F
from tests import util as U
from tests.tile_util import BORDER_CAP


def _cpu_call(covars, quats="given", scales="given", n=5, **kw):
    from edgegaussians_amd import rasterization
    g = torch.Generator().manual_seed(1)
    q = torch.randn(n, 4, generator=g) if isinstance(quats, str) else quats
    s = torch.rand(n, 3, generator=g) if isinstance(scales, str) else scales
    vm = torch.eye(4)[None]
    K = torch.tensor([[[50.0, 0.0, 16.0], [0.0, 50.0, 16.0], [0.0, 0.0, 1.0]]])
    return rasterization(torch.randn(n, 3, generator=g), q, s, torch.rand(n, generator=g), torch.rand(n, 3, generator=g), vm, K,
                         32, 32, covars=covars, **kw)


def test_covars_is_a_keyword_that_defaults_to_none_and_moves_no_earlier_parameter():
    """camera_model stays the last parameter (tests/test_ortho_host.py pins it), so covars stands in front of
    channel_chunk: the 21 parameters of gsplat 1.0.0 before channel_chunk keep their positions, and a call that still
    passes channel_chunk (or camera_model) in covars's position is refused by name, never misread."""
    import inspect
    import gsplat
    from edgegaussians_amd import rasterization
    first21 = ["means", "quats", "scales", "opacities", "colors", "viewmats", "Ks", "width", "height", "near_plane", "far_plane",
               "radius_clip", "eps2d", "sh_degree", "packed", "tile_size", "backgrounds", "render_mode", "sparse_grad", "absgrad",
               "rasterize_mode"]
    for fn in (rasterization, gsplat.rasterization):
        names = list(inspect.signature(fn).parameters)
        assert names == first21 + ["covars", "channel_chunk", "camera_model"]
        assert inspect.signature(fn).parameters["covars"].default is None
    for stray in (32, "ortho"):
        with pytest.raises(TypeError, match="covars must be a tensor or None.*by keyword"):
            _cpu_call(stray)


@pytest.mark.parametrize("shape", [(5, 6), (5, 3), (4, 3, 3), (5, 3, 3, 1), (5, 9)])
def test_a_wrong_covars_shape_is_refused(shape):
    with pytest.raises(ValueError, match="covars must have shape"):
        _cpu_call(torch.zeros(shape))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.int32])
def test_a_wrong_covars_dtype_is_refused(dtype):
    with pytest.raises(TypeError, match="covars must be torch.float32"):
        _cpu_call(torch.zeros(5, 3, 3, dtype=dtype))
    with pytest.raises(TypeError, match="covars must be a tensor"):
        _cpu_call([[1.0]])


def test_a_cpu_covars_is_refused_for_its_device_with_and_without_quats_and_scales():
    """A well-formed covars on the CPU gets past the shape and dtype checks and is refused for its device -- the same
    error whether quats and scales are given or None: with covars they are not looked at."""
    cov = torch.eye(3).expand(5, 3, 3).contiguous()
    for q, s in (("given", "given"), (None, None)):
        with pytest.raises(ValueError, match="covars must be a device tensor"):
            _cpu_call(cov, quats=q, scales=s)


def test_an_unknown_camera_model_is_refused_before_any_tensor_is_looked_at():
    with pytest.raises(ValueError, match="Unknown camera_model"):
        _cpu_call(torch.zeros(7, 2), camera_model="equirect")      # (a covars that would be refused next)
    with pytest.raises(NotImplementedError, match="fisheye"):
        _cpu_call("not a tensor", camera_model="fisheye")


# ---------------------------------------------------------------------------------------------------
def test_gradient_convention_of_the_full_matrix_input():
    """Autograd through sym_from6(covars[:, IU, JU]) on the float64 reference: the lower triangle gets exactly zero, an
    off-diagonal entry of the upper triangle the sum of both symmetric cotangents of the symmetric matrix, and the whole
    is the [N, 6] gradient of ref_covars_vjps scattered to the upper triangle.  What is below the diagonal is not read."""
    spec, means, covars, _q, _s, vms, Ks, _g = F.covars_inputs("three_cams_eps1")
    n = 257
    means, covars = means[:n], covars[:n]
    gen = torch.Generator().manual_seed(5)
    widths = dict(means2d=2, depths=1, conics=3, compensations=1)
    cots = {k: torch.randn(vms.shape[0], n, widths[k], generator=gen) for k in U.PROJ_OUTPUTS}
    outs, g6 = F.ref_covars_vjps(means, covars, vms, Ks, spec["args"], cots)
    assert (outs["radii"] > 0).sum() >= 100
    g33 = CU.ref_grad33(means, CU.full33(covars), vms, Ks, spec["args"], cots)
    g33_junk = CU.ref_grad33(means, CU.full33(covars, lower=123.0), vms, Ks, spec["args"], cots)
    for k in cots:
        # (the mean and the depth do not depend on the covariance: their cotangents give exact zeros)
        assert (g6[k]["covars"].abs().max() > 0) == (k in ("conics", "compensations")), k
        assert not CU.lower3(g33[k]).any(), k
        assert torch.equal(CU.upper6(g33[k]), g6[k]["covars"]), k
        assert torch.equal(g33[k], g33_junk[k]), k
    # both symmetric cotangents: differentiate with respect to the full matrix, every entry a variable of its own
    S = F.sym_from6(covars.double()).clone().requires_grad_(True)
    a = spec["args"]
    for k in ("conics", "compensations"):
        y = torch.stack([CU.ref_project_covars_pg(means.double(), None, vms[c], Ks[c], CU.W, CU.H, a["near_plane"], a["far_plane"],
                                                  a["eps2d"], a["radius_clip"], covar_w=S)[1 + U.PROJ_OUTPUTS.index(k)]
                         for c in range(vms.shape[0])])
        gS = torch.autograd.grad(y, S, cots[k].double().reshape(y.shape))[0]
        expect = torch.stack([gS[:, i, j] if i == j else gS[:, i, j] + gS[:, j, i] for i, j in F.TRIU], dim=-1)
        assert (CU.upper6(g33[k]) - expect).abs().max() <= 1e-12 * expect.abs().max(), k


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ortho", [False, True], ids=["pinhole", "ortho"])
def test_packed_scene_keeps_a_part_of_the_pairs(ortho):
    shares = CU.packed_visible_share(ortho)
    U.record_cpu("covars_packed_scene_visible_share", ortho=ortho, shares=shares)
    print("visible share per camera:", shares)
    assert CU.PACKED_SHARE[0] <= min(shares) and max(shares) <= CU.PACKED_SHARE[1], shares


@pytest.mark.parametrize("model", list(CU.POSE_CASES))
def test_pose_reference_conditions(model):
    """At least POSE_MIN_PAIRS visible pairs per camera, few borderline rows, an exactly zero bottom row from autograd,
    and the per-Gaussian-viewmat reference sums to the gradient of the ordinary call with one viewmat per camera."""
    ref, a = CU.pose_inputs(model)
    G, bottom = CU.pose_reference(model)
    assert bottom == 0.0
    vis = ref["vis"]
    assert vis.sum(axis=1).min() >= CU.POSE_MIN_PAIRS, vis.sum(axis=1)
    assert ref["border"].mean(axis=1).max() <= 0.02
    assert set(G) == set(U.PROJ_OUTPUTS)
    m, c6 = ref["means"].double(), ref["covars"].double()
    from tests import ortho_util as OU
    for c in range(vis.shape[0]):
        vm = ref["viewmats"][c].double().clone().requires_grad_(True)
        lims = (a["near_plane"], a["far_plane"], a["eps2d"], a["radius_clip"])
        if model == "pinhole":
            out = F.ref_project_covars(m, c6, vm, ref["Ks"][c], CU.W, CU.H, *lims)
        else:
            out = OU.ref_project_ortho(m, None, None, vm, ref["Ks"][c].double(), CU.W, CU.H, *lims, covars=c6)
        for k, cot in ref["cots"].items():
            y = out[1 + U.PROJ_OUTPUTS.index(k)]
            g = torch.autograd.grad(y, vm, cot[c].double().reshape(y.shape), retain_graph=True)[0]
            S = G[k][c].abs().sum(0)
            assert not g[3].any()
            assert ((g[:3] - G[k][c].sum(0)).abs() <= 1e-12 * S + 1e-300).all(), (model, c, k)
            assert (S > 0).any()


@pytest.mark.parametrize("antialiased", [False, True], ids=["classic", "antialiased"])
@pytest.mark.parametrize("ts", CU.TILE_SIZES)
def test_whole_scene_conditions(ts, antialiased):
    ws = CU.whole_scene()
    keep = CU.whole_keep(ts, antialiased)
    share = float((~keep).float().mean())
    U.record_cpu("covars_whole_scene_conditions", tile_size=ts, antialiased=antialiased, borderline_share=share,
                 removed=ws["removed"], n0=ws["n0"])
    print(f"ts={ts} antialiased={antialiased}: borderline pixels {share:.4%}, removed {ws['removed']} of {ws['n0']}")
    assert share <= BORDER_CAP
    assert ws["removed"] <= max(3, 0.016 * ws["n0"])
    with torch.no_grad():
        for c in range(len(CU.WHOLE_CAMS)):
            assert (CU.whole_projection(ws, c)[0] > 0).sum() >= 100


def test_new_entries_check_their_arguments():
    """The five entries of the covariance form refuse null pointers and bad sizes by name before any device call, and
    have nothing to do without pairs (eg_packed_write_covars / _bwd_sparse_covars) or without Gaussians (_bwd_covars)."""
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    h = _lib.load(require_device=False)
    nul = [None] * 4
    count = lambda n, c: h.eg_packed_count_covars(*nul, n, c, 32, 32, 0.01, 1e10, 0.3, 0.0, 0, None, None, None)
    write = lambda n, c, nnz: h.eg_packed_write_covars(*nul, None, n, c, 32, 32, 0.01, 1e10, 0.3, 0.0, 0, None, nnz,
                                                       *([None] * 10), None)
    bwd = lambda n, c, nnz: h.eg_packed_bwd_covars(*nul, n, c, 32, 32, 0.3, 0, None, nnz, *([None] * 6), None)
    sparse = lambda n, c, nnz: h.eg_packed_bwd_sparse_covars(*nul, n, c, 32, 32, 0.3, 0, nnz, *([None] * 7), None)
    pose = lambda n, c, nnz: h.eg_project_covars_bwd_viewmats(*nul, n, c, 32, 32, 0.3, 0, None, None, nnz, *([None] * 5), 0,
                                                              None, None)
    err = h.eg_last_error_string
    assert count(4, 1) == -1 and b"eg_packed_count_covars" in err() and b"null pointer" in err()
    assert count(4, 0) == -1 and b"bad sizes" in err()
    assert write(4, 1, 2) == -1 and b"eg_packed_write_covars" in err() and b"null pointer" in err()
    assert write(4, 1, 5) == -1 and b"bad nnz" in err()
    assert write(4, 0, 0) == -1 and b"bad sizes" in err()
    assert write(4, 1, 0) == 0
    assert bwd(4, 1, 2) == -1 and b"eg_packed_bwd_covars" in err() and b"null pointer" in err()
    assert bwd(4, 1, -1) == -1 and b"bad nnz" in err()
    assert bwd(0, 1, 0) == 0
    assert sparse(4, 1, 2) == -1 and b"eg_packed_bwd_sparse_covars" in err() and b"null pointer" in err()
    assert sparse(4, 1, 5) == -1 and b"bad nnz" in err()
    assert sparse(4, 1, 0) == 0
    assert pose(4, 1, 2) == -1 and b"eg_project_covars_bwd_viewmats" in err() and b"null pointer" in err()
    assert pose(4, 0, 0) == -1 and b"bad sizes" in err()
    assert pose(4, 1, 5) == -1 and b"bad nnz" in err()
