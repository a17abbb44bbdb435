"""The bilateral grid without a device: the grid_sample statement of tests/bilagrid_util.py against the closed form in
float64 (values and all three gradients), the borderline share of every case the device tests use, the TV closed form
against autograd, the C ABI (declared, exported, bound with the header's signatures, argument checks), the build list,
the refusals in their stated order on CPU tensors, the shim, the module and the import hygiene of the product."""
import ctypes
import os
import re

import pytest
import torch

from tests import bilagrid_util as BU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("eg_bilagrid_slice_fwd", "eg_bilagrid_slice_bwd", "eg_bilagrid_tv_fwd", "eg_bilagrid_tv_bwd")


@pytest.mark.parametrize("scene", BU.SCENES)
def test_grid_sample_form_is_the_closed_form(scene):
    for grid_size, image, idx in BU.cases():
        ref = BU.reference(scene, grid_size, image, idx)
        out, v_rgb, v_grids = BU.closed_form(ref["grids"].double(), ref["rgb"].double(), ref["xy"].double(), ref["idx"],
                                             ref["v"].double())
        tag = (scene, grid_size, image, idx)
        assert float((out - ref["out"]).abs().max()) <= 1e-13 * max(1.0, float(ref["out"].abs().max())), tag
        assert float((v_grids - ref["v_grids"]).abs().max()) <= 1e-12 * max(1.0, float(ref["v_grids"].abs().max())), tag
        keep = ~ref["borderline"]
        scale = max(1.0, float(ref["v_rgb"].abs().max()))
        assert float((v_rgb - ref["v_rgb"])[keep].abs().max()) <= 1e-12 * scale, tag
        # black pixels are compared, and their guidance term is exactly absent: v_rgb is the direct part alone
        black = (ref["rgb"] == 0).all(-1)
        assert not bool((black & ref["borderline"]).any())
        if bool(black.any()):
            L = grid_size[0]
            raws = BU.raw_coords(ref["rgb"].double(), ref["xy"].double(), grid_size)
            (cu, cv, cw), cells = BU._cells(raws, grid_size)
            A = BU.Blend(ref["grids"].double(), ref["idx"], cu, cv, cw, cells).A().reshape(*black.shape, 3, 4)
            direct = (ref["v"].double()[..., :, None] * A[..., :, :3]).sum(-2)
            assert torch.equal(ref["v_rgb"][black], direct[black]) or \
                float((ref["v_rgb"] - direct)[black].abs().max()) <= 1e-13 * scale, tag
        # unused grids: exactly zero; a shared grid: the sum over both images
        for g in set(range(BU.N_GRIDS)) - set(idx):
            assert not bool(ref["v_grids"][g].any()) and not bool(ref["bound_v_grids"][g].any()), tag


def test_coordinates_outside_the_unit_square_match_grid_sample():
    g = torch.Generator().manual_seed(3)
    grids = torch.randn(2, 12, 3, 4, 5, generator=g, dtype=torch.float64)
    rgb = torch.rand(2, 6, 7, 3, generator=g, dtype=torch.float64) * 1.6 - 0.3      # gray below 0 and above 1
    xy = torch.rand(2, 6, 7, 2, generator=g, dtype=torch.float64) * 1.6 - 0.3
    v = torch.randn(2, 6, 7, 3, generator=g, dtype=torch.float64)
    want = BU.grads_grid_sample(grids, rgb, xy, [1, 0], v)
    got = BU.closed_form(grids, rgb, xy, [1, 0], v)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) == 0.0 or float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())


def test_borderline_share_of_every_device_case():
    worst = 0.0
    for scene in BU.SCENES:
        for grid_size, image, idx in BU.cases():
            share = float(BU.reference(scene, grid_size, image, idx)["borderline"].double().mean())
            worst = max(worst, share)
            assert share <= BU.BORDERLINE_SHARE_MAX, (scene, grid_size, image, idx, share)
    # white pixels are borderline, black ones are not
    assert bool(BU.borderline(torch.ones(1, 1, 1, 3, dtype=torch.float64), 8).all())
    assert not bool(BU.borderline(torch.zeros(1, 1, 1, 3, dtype=torch.float64), 8).any())
    assert not bool(BU.borderline(torch.full((1, 1, 1, 3), 0.3, dtype=torch.float64), 1).any())


def test_fp32_model_of_the_kernels_lies_inside_the_bounds():
    """the kernels' arithmetic in fp32 on the CPU: inside every bound, exact on identity grids; a mutant that drops the
    guidance term, and one that swaps x and y, leave them"""
    from tests.util import record_cpu
    worst = [0.0, 0.0, 0.0]
    for scene in BU.SCENES:
        for grid_size, image, idx in BU.cases():
            ref = BU.reference(scene, grid_size, image, idx)
            out, v_rgb, v_grids = BU.model_f32(ref["grids"], ref["rgb"], ref["xy"], ref["idx"], ref["v"])
            pairs = (BU.ratio(out, ref["out"], ref["bound_out"]),
                     BU.ratio(v_rgb, ref["v_rgb"], ref["bound_v_rgb"], ~ref["borderline"]),
                     BU.ratio(v_grids, ref["v_grids"], ref["bound_v_grids"]))
            for k, (r, over) in enumerate(pairs):
                assert over == 0, (scene, grid_size, image, idx, k, r)
                worst[k] = max(worst[k], r)
            if scene == "identity":
                assert torch.equal(out, ref["rgb"])
    record_cpu("bilagrid_fp32_model_over_bound", out=worst[0], v_rgb=worst[1], v_grids=worst[2])
    ref = BU.reference("rand", (8, 16, 16), (2, 37, 53), (0, 1))
    keep = ~ref["borderline"]
    raws = BU.raw_coords(ref["rgb"].double(), ref["xy"].double(), (8, 16, 16))
    (cu, cv, cw), cells = BU._cells(raws, (8, 16, 16))
    A = BU.Blend(ref["grids"].double(), ref["idx"], cu, cv, cw, cells).A().reshape(2, 37, 53, 3, 4)
    direct = (ref["v"].double()[..., :, None] * A[..., :, :3]).sum(-2)                    # no guidance term
    assert BU.ratio(direct, ref["v_rgb"], ref["bound_v_rgb"], keep)[1] > 0
    shifted = BU.closed_form(ref["grids"].double(), ref["rgb"].double(), ref["xy"].double().flip(-1), ref["idx"], ref["v"].double())
    assert BU.ratio(shifted[0], ref["out"], ref["bound_out"])[1] > 0                      # x and y swapped
    assert BU.ratio(shifted[2], ref["v_grids"], ref["bound_v_grids"])[1] > 0


def test_persistent_and_wave_cases_reach_what_they_are_for():
    """the conditions on the inputs of the two device cases that exist for a code path: with the lowered workgroup
    count a workgroup of the forward / v_rgb kernel makes several trips, the last one partly filled, and a lane of the
    scatter owns run >= 2 samples with the image ending INSIDE some lane's run; the wave scene has whole waves in one
    cell, waves that are not, and a partial last wave in one cell -- and the fp32 model holds its bounds on it"""
    plans = []
    for wgs, (B, H, W), idx in BU.PERSISTENT_CASES:
        n = H * W
        blocks, trips, sblocks, run = BU.persistent_plan(B, n, wgs)
        plans.append((blocks, trips, sblocks, run))
        assert trips >= 2 and n % (blocks * 1024) != 0          # several trips, a ragged last one
        assert run >= 2 and n % run != 0                          # the image ends inside a lane's run
        assert BU.persistent_plan(B, n, 256)[1::2] == (1, 1)      # ... none of which the default count reaches here
    assert plans == [(1, 5, 1, 5), (1, 2, 1, 2), (3, 2, 3, 2)]
    assert BU.persistent_plan(1, 1200 * 1600, 256) == (256, 8, 235, 8)
    ref = BU.wave_reference()
    L, Hg, Wg = BU.GRID_ABOVE_BUDGET
    from edgegaussians_amd import bilagrid
    assert bilagrid.scatter_path(L, Hg, Wg) == "global"
    raws = BU.raw_coords(ref["rgb"].double(), ref["xy"].double(), (L, Hg, Wg))
    _, cells = BU._cells(raws, (L, Hg, Wg))
    key = ((cells[4] * Hg + cells[2]) * Wg + cells[0]).view(-1)
    uniform = [bool((key[w:w + 64] == key[w]).all()) for w in range(0, key.numel(), 64)]
    assert uniform == [True, True, True, False, False, True] and key.numel() % 64 != 0 and key.numel() > 256
    # the one-cell samples sit well inside their cell: no fp32 rounding moves a lane of those waves out of it
    for raw, n in zip(raws, (Wg, Hg, L)):
        frac = (raw.view(-1)[ref["shared"]] % 1.0)
        assert float(frac.min()) > 1e-3 and float(frac.max()) < 1 - 1e-3
    assert not bool(ref["borderline"].any())
    out, v_rgb, v_grids = BU.model_f32(ref["grids"], ref["rgb"], ref["xy"], ref["idx"], ref["v"])
    assert BU.ratio(out, ref["out"], ref["bound_out"])[1] == 0 and BU.ratio(v_rgb, ref["v_rgb"], ref["bound_v_rgb"])[1] == 0
    assert BU.ratio(v_grids, ref["v_grids"], ref["bound_v_grids"])[1] == 0
    # a wave-combined sum that lost a lane (lane 0 of the first wave) leaves the bound
    lost = ref["v"].clone()
    lost.view(-1, 3)[0] = 0.0
    assert BU.ratio(BU.model_f32(ref["grids"], ref["rgb"], ref["xy"], ref["idx"], lost)[2], ref["v_grids"], ref["bound_v_grids"])[1] > 0


def test_tv_closed_form_is_autograd_and_a_size_one_axis_contributes_nothing():
    for shape in BU.TV_SHAPES:
        case = BU.tv_case(shape)
        got = BU.tv_grad_closed(case["x"].double())
        assert float((got - case["grad"]).abs().max()) <= 1e-15 * max(1.0, float(case["grad"].abs().max())), shape
    assert BU.tv_case((2, 12, 1, 1, 1))["value"] == 0.0 and not bool(BU.tv_case((2, 12, 1, 1, 1))["grad"].any())
    x = BU.tv_case((1, 12, 1, 7, 1))["x"].double()
    assert abs(BU.tv_case((1, 12, 1, 7, 1))["value"] - float(((x[:, :, :, 1:] - x[:, :, :, :-1]) ** 2).mean())) <= 1e-15
    assert BU.tv_depth(1) == 11 + 6 + 3 + 0 + 6 and BU.tv_depth(65 * 1024) == 11 + 6 + 3 + 1 + 6


def test_entries_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib, bilagrid, build
    assert "bilagrid.hip" in build.SOURCES
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "edgegs.h")).read(), flags=re.S)
    h = ctypes.CDLL(_lib.LIB_PATH)
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "eg_stream_t": ctypes.c_void_p}
    for name in ENTRIES:
        assert hasattr(h, name) and name in _lib._SIGS and name in _lib.EXPORTS, name
        decl = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl, name
        want = []
        for arg in decl.group(1).split(","):
            arg = arg.strip()
            if "int64_t *" in arg:
                want.append(ctypes.POINTER(ctypes.c_int64))
            elif "*" in arg:
                want.append(ctypes.c_void_p)
            else:
                want.append(ctype_of[arg.split()[0]])
        assert _lib._SIGS[name] == want, (name, _lib._SIGS[name], want)
    m = re.search(r"#define\s+EG_BILAGRID_LDS_BUDGET\s+\((\d+)\s*\*\s*(\d+)\)", header)
    assert m and int(m.group(1)) * int(m.group(2)) == bilagrid.LDS_BUDGET_BYTES
    src = open(os.path.join(ROOT, "edgegaussians_amd", "csrc", "bilagrid.hip")).read()
    assert "constexpr int kMapThreads = 1024;" in src and "constexpr int kScatterThreads = 1024;" in src
    assert "constexpr int kThreads = 256;" in src and "constexpr int kTvQuad = 4;" in src and "constexpr int kFinLanes = 64;" in src
    assert (bilagrid.MAP_THREADS, bilagrid.SCATTER_THREADS, bilagrid.TV_WG_ELEMS, bilagrid.FIN_LANES) == (1024, 1024, 1024, 64)
    assert bilagrid.scatter_path(8, 16, 16) == "lds" and bilagrid.scatter_path(*BU.GRID_ABOVE_BUDGET) == "global"
    assert all(bilagrid.scatter_path(*s) == "lds" for s in BU.GRID_SIZES)


def test_c_abi_argument_validation_without_launching():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    h = _lib.load(require_device=False)
    st = (ctypes.c_int64 * 4)(36, 12, 3, 1)
    neg = (ctypes.c_int64 * 4)(36, -12, 3, 1)
    p = 4096  # never dereferenced: every call below is refused before any HIP call

    def swap(args, i, value):
        return args[:i] + (value,) + args[i + 1:]

    def refused(name, args):
        assert getattr(h, name)(*args) == -1, (name, args)
        assert name.encode() in h.eg_last_error_string()

    # (grids, N, L, Hg, Wg, rgb, xy, grid_idx, idx_is_int64, B, H, W, strides_rgb, strides_xy, ...)
    ok_f = (p, 2, 8, 16, 16, p, p, p, 1, 3, 4, 5, st, st, 0, p, None)
    ok_b = (p, 2, 8, 16, 16, p, p, p, 1, 3, 4, 5, st, st, 0, p, p, p, None)
    for name, ok in (("eg_bilagrid_slice_fwd", ok_f), ("eg_bilagrid_slice_bwd", ok_b)):
        for args in (swap(ok, 0, None), swap(ok, 1, 0), swap(ok, 2, 0), swap(ok, 3, -1), swap(ok, 4, 0), swap(ok, 5, None),
                     swap(ok, 6, None), swap(ok, 7, None),              # no grid_idx with B != N
                     swap(ok, 8, 2), swap(ok, 9, 0), swap(ok, 10, 0), swap(ok, 11, 0),
                     swap(swap(swap(ok, 9, 1 << 11), 10, 1 << 10), 11, 1 << 10),   # 2^31 samples
                     swap(swap(ok, 1, 1 << 12), 2, 1 << 12),           # 2^31 grid elements
                     swap(ok, 12, None), swap(ok, 13, None), swap(ok, 12, neg), swap(ok, 13, neg), swap(ok, 14, -1)):
            refused(name, args)
    refused("eg_bilagrid_slice_fwd", swap(ok_f, 15, None))
    refused("eg_bilagrid_slice_bwd", swap(ok_b, 15, None))
    refused("eg_bilagrid_slice_bwd", swap(swap(ok_b, 16, None), 17, None))
    ok_tf = (p, 2, 8, 16, 16, p, 48, p, None)      # 2 * 12 * 2048 / 1024 = 48 partials
    ok_tb = (p, 2, 8, 16, 16, p, p, None)
    for args in (swap(ok_tf, 0, None), swap(ok_tf, 1, 0), swap(ok_tf, 4, 0), swap(ok_tf, 5, None), swap(ok_tf, 6, 47),
                 swap(ok_tf, 7, None), swap(swap(ok_tf, 1, 1 << 12), 2, 1 << 12)):
        refused("eg_bilagrid_tv_fwd", args)
    for args in (swap(ok_tb, 0, None), swap(ok_tb, 2, 0), swap(ok_tb, 5, None), swap(ok_tb, 6, None)):
        refused("eg_bilagrid_tv_bwd", args)


def test_refusals_on_cpu_tensors_in_the_stated_order():
    from edgegaussians_amd import bilagrid as BG
    grids = torch.rand(2, 12, 3, 4, 5)
    rgb, xy = torch.rand(2, 6, 7, 3), torch.rand(2, 6, 7, 2)
    idx = torch.tensor([1, 0])
    # every later fault is present too: the earlier one is the one reported
    with pytest.raises(ValueError, match=r"grids must be \[N, 12"):
        BG.slice(grids[:, :11].double(), xy[..., :1], rgb[..., :2])
    with pytest.raises(ValueError, match=r"grids must be \[N, 12"):
        BG.slice(grids[0], xy, rgb)
    with pytest.raises(ValueError, match="contiguous"):
        BG.slice(grids.transpose(3, 4).double(), xy, rgb[..., :2])
    with pytest.raises(ValueError, match=r"rgb must be \[B, ..., 3\]"):
        BG.slice(grids.double(), xy[..., :1], rgb[..., :2])
    with pytest.raises(ValueError, match=r"xy must be \[B, ..., 2\]"):
        BG.slice(grids.double(), xy[..., :1], rgb)
    with pytest.raises(ValueError, match="leading shape"):
        BG.slice(grids.double(), xy[:, :5], rgb)
    with pytest.raises(ValueError, match="None only when B == N"):
        BG.slice(grids.double(), xy[:1], rgb[:1])
    with pytest.raises(ValueError, match=r"grid_idx must be \[B\] or \[B, 1\]"):
        BG.slice(grids.double(), xy, rgb, torch.tensor([0, 1, 0]).float())
    with pytest.raises(ValueError, match="empty"):
        BG.slice(grids.double(), xy[:, :0], rgb[:, :0])
    with pytest.raises(ValueError, match="empty"):
        BG.slice(grids[:0].double(), xy[:0], rgb[:0])
    huge = torch.zeros(1, 1, 1, 3).expand(2, 1 << 15, 1 << 15, 3)          # 2^31 samples, no memory
    with pytest.raises(ValueError, match="2\\^31 samples"):
        BG.slice(grids.double(), torch.zeros(1, 1, 1, 2).expand(2, 1 << 15, 1 << 15, 2), huge)
    with pytest.raises(TypeError, match="grids must be torch.float32"):
        BG.slice(grids.double(), xy.clone().requires_grad_(True), rgb)
    with pytest.raises(TypeError, match="rgb must be torch.float32"):
        BG.slice(grids, xy, rgb.half())
    with pytest.raises(TypeError, match="xy must be torch.float32"):
        BG.slice(grids, xy.double(), rgb)
    with pytest.raises(TypeError, match="grid_idx must be torch.int32 or torch.int64"):
        BG.slice(grids, xy.clone().requires_grad_(True), rgb, idx.float())
    with pytest.raises(ValueError, match="xy must not require grad"):
        BG.slice(grids, xy.clone().requires_grad_(True), rgb, idx)
    for args in ((grids, xy, rgb), (grids, xy, rgb, idx), (grids, xy, rgb, idx.int().view(2, 1)), (BG.BilateralGrid(2, 5, 4, 3), xy, rgb)):
        with pytest.raises(ValueError, match="no CPU path"):
            BG.slice(*args)
    with pytest.raises(ValueError, match="no CPU path"):
        BG.slice(grids, xy, rgb, idx, check_idx=False)
    with pytest.raises(ValueError, match=r"grids must be \[N, 12"):
        BG.total_variation_loss(grids[:, :3].double())
    with pytest.raises(ValueError, match="empty"):
        BG.total_variation_loss(grids[:0].double())
    with pytest.raises(TypeError, match="float32"):
        BG.total_variation_loss(grids.double())
    with pytest.raises(ValueError, match="no CPU path"):
        BG.total_variation_loss(grids)
    with pytest.raises(ValueError, match="no CPU path"):
        BG.BilateralGrid(2).tv_loss()


def test_shim_and_module():
    import edgegaussians_amd
    import fused_bilagrid
    from edgegaussians_amd import bilagrid
    assert "bilagrid" in edgegaussians_amd.__all__ and edgegaussians_amd.bilagrid is bilagrid
    assert fused_bilagrid.__all__ == ["BilateralGrid", "slice", "total_variation_loss"]
    for name in fused_bilagrid.__all__:
        assert getattr(fused_bilagrid, name) is getattr(bilagrid, name), name
    assert not hasattr(fused_bilagrid, "color_correct") and "color_correct" in fused_bilagrid.__doc__
    assert "rgb_affine_mats" in bilagrid.__doc__ and "host sync" in bilagrid.__doc__.lower()
    assert "from memory" in bilagrid.__doc__
    m = bilagrid.BilateralGrid(5)
    assert isinstance(m, torch.nn.Module) and isinstance(m.grids, torch.nn.Parameter)
    assert m.grids.shape == (5, 12, 8, 16, 16) and m.grids.dtype == torch.float32 and m.grids.is_contiguous()
    m = bilagrid.BilateralGrid(2, grid_X=5, grid_Y=4, grid_W=3)
    assert m.grids.shape == (2, 12, 3, 4, 5) and [p is m.grids for p in m.parameters()] == [True]
    eye = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0])
    assert torch.equal(m.grids.detach(), eye.view(1, 12, 1, 1, 1).expand(2, 12, 3, 4, 5))
    with pytest.raises(NotImplementedError, match="slice"):
        m(torch.rand(2, 4, 4, 2), torch.rand(2, 4, 4, 3))


def test_product_never_imports_the_oracle_or_the_tests():
    bad = []
    for path in (os.path.join(ROOT, "edgegaussians_amd", "bilagrid.py"), os.path.join(ROOT, "fused_bilagrid", "__init__.py")):
        if re.search(r"^\s*(from|import)\s+(oracle|tests)\b", open(path).read(), re.M):
            bad.append(path)
    assert not bad, bad
