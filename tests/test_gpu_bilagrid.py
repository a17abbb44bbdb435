"""The bilateral grid on the device (csrc/bilagrid.hip through edgegaussians_amd/bilagrid.py) against the float64
statements of tests/bilagrid_util.py: every element of out, of v_rgb outside the borderline set and of v_grids inside
its bound, exact zeros for unused grids, identity grids, run-to-run and batch independence, layouts, the chain
rasterization -> slice -> l1_loss against the float32 torch composition, evaluation mode, and the refusals that need
device tensors.

Shapes (bilagrid_util.GRID_SIZES, GRID_ABOVE_BUDGET, IMAGES): the default grid, odd sizes, axes of size 1, one grid one
column above the LDS budget (the global-atomics scatter); two images of 37 x 53 sharing grid 2 or on grids 0 and 1, and
one image of 69 x 69: two 32 x 32 blocks plus 5 in each direction, 4 761 samples -- five workgroups of 1024 lanes of the
LDS kernels, the last one partly filled, nineteen of 256 of the kernels for grids above the budget.

v_grids is summed with float atomics: it is not bit-reproducible, so two runs are held to twice the bound against
each other and the largest difference is recorded."""
import pytest
import torch
import torch.nn.functional as F

from tests import bilagrid_util as BU
from tests.util import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bg():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import bilagrid as mod
    assert (mod.TV_WG_ELEMS, mod.FIN_LANES) == (BU.TV_WG_ELEMS, BU.FIN_LANES)
    return mod


def _run(bg, ref, grids_grad=True, rgb_grad=True, **kw):
    grids = ref["grids"].cuda().requires_grad_(grids_grad)
    rgb = ref["rgb"].cuda().requires_grad_(rgb_grad)
    idx = torch.tensor(ref["idx"], device="cuda")
    out = bg.slice(grids, ref["xy"].cuda(), rgb, idx, **kw)["rgb"]
    if grids_grad or rgb_grad:
        out.backward(ref["v"].cuda())
    return out.detach(), rgb.grad, grids.grad


@pytest.mark.parametrize("scene", BU.SCENES)
@pytest.mark.parametrize("grid_size", BU.GRID_SIZES + (BU.GRID_ABOVE_BUDGET,), ids=lambda s: "x".join(map(str, s)))
def test_out_and_gradients_within_their_bounds(bg, scene, grid_size):
    worst = {"out": 0.0, "v_rgb": 0.0, "v_grids": 0.0, "v_grids_run_to_run": 0.0}
    for image, idx in BU.IMAGES:
        ref = BU.reference(scene, grid_size, image, idx)
        tag = (scene, grid_size, image, idx, bg.scatter_path(*grid_size))
        out, v_rgb, v_grids = _run(bg, ref)
        assert out.shape == ref["rgb"].shape and out.is_contiguous() and out.dtype == torch.float32
        keep = ~ref["borderline"]
        r_out, over_out = BU.ratio(out.cpu(), ref["out"], ref["bound_out"])
        r_rgb, over_rgb = BU.ratio(v_rgb.cpu(), ref["v_rgb"], ref["bound_v_rgb"], keep)
        r_g, over_g = BU.ratio(v_grids.cpu(), ref["v_grids"], ref["bound_v_grids"])
        print(f"{tag}: out {r_out:.3f}, v_rgb {r_rgb:.3f}, v_grids {r_g:.3f} of the bound; borderline "
              f"{float(ref['borderline'].double().mean()):.2e}")
        assert over_out == 0, f"{tag}: {over_out} elements of out over the bound, the worst by {r_out:.2f} x"
        assert over_rgb == 0, f"{tag}: {over_rgb} elements of v_rgb over the bound, the worst by {r_rgb:.2f} x"
        assert over_g == 0, f"{tag}: {over_g} elements of v_grids over the bound, the worst by {r_g:.2f} x"
        for g in set(range(BU.N_GRIDS)) - set(idx):                       # unused grids: exactly zero
            assert not bool(v_grids[g].any()), tag
        # two runs: out and v_rgb bit-equal, v_grids within twice the bound of each other
        out2, v_rgb2, v_grids2 = _run(bg, ref)
        assert torch.equal(out, out2) and torch.equal(v_rgb, v_rgb2), tag
        diff = (v_grids - v_grids2).abs().cpu().double()
        assert bool((diff <= 2 * ref["bound_v_grids"]).all()), tag
        pos = ref["bound_v_grids"] > 0
        run_to_run = float((diff[pos] / ref["bound_v_grids"][pos]).max()) if bool(pos.any()) else 0.0
        for k, r in zip(worst, (r_out, r_rgb, r_g, run_to_run)):
            worst[k] = max(worst[k], r)
        if scene == "identity":
            assert torch.equal(out.cpu(), ref["rgb"]), tag                   # lerps of equal corners are exact
    record("bilagrid_over_bound", scene=scene, grid=list(grid_size), **worst)


@pytest.mark.parametrize("scene", ("rand", "render_like"))
def test_persistent_workgroups_that_walk_several_blocks(bg, scene, monkeypatch):
    """The loops of the persistent LDS kernels (bilagrid_util.PERSISTENT_CASES; the host test states what each case
    reaches): MAX_WORKGROUPS lowered so that a workgroup of the forward / v_rgb kernel makes several trips with a ragged
    last one, and a lane of the scatter owns run >= 2 consecutive samples with the image ending inside a run.  out and
    v_rgb: the bits of the default launch; v_grids: inside its bound, unused grids exactly zero."""
    for grid_size in ((8, 16, 16), (3, 4, 5)):
        for wgs, image, idx in BU.PERSISTENT_CASES:
            ref = BU.reference(scene, grid_size, image, idx)
            want = _run(bg, ref)
            monkeypatch.setattr(bg, "MAX_WORKGROUPS", wgs)
            out, v_rgb, v_grids = _run(bg, ref)
            monkeypatch.undo()
            tag = (scene, grid_size, wgs, image, idx)
            assert torch.equal(out, want[0]) and torch.equal(v_rgb, want[1]), tag
            r_out, over_out = BU.ratio(out.cpu(), ref["out"], ref["bound_out"])
            r_rgb, over_rgb = BU.ratio(v_rgb.cpu(), ref["v_rgb"], ref["bound_v_rgb"], ~ref["borderline"])
            r_g, over_g = BU.ratio(v_grids.cpu(), ref["v_grids"], ref["bound_v_grids"])
            print(f"{tag}: out {r_out:.3f}, v_rgb {r_rgb:.3f}, v_grids {r_g:.3f} of the bound")
            assert over_out == 0 and over_rgb == 0, tag
            assert over_g == 0, f"{tag}: {over_g} elements of v_grids over the bound, the worst by {r_g:.2f} x"
            for g in set(range(BU.N_GRIDS)) - set(idx):
                assert not bool(v_grids[g].any()), tag


def test_wave_combined_scatter_of_grids_above_the_budget(bg):
    """slice_vgrid_global_kernel on bilagrid_util.make_wave_scene: three waves whose 64 samples share one cell (the DPP
    sum, one atomic per word from lane 63), two waves that do not (one atomic per lane), and a partial last wave in one
    cell whose dead lanes carry zeros.  Every element of v_grids inside its bound, against float64."""
    ref = BU.wave_reference()
    assert bg.scatter_path(*BU.GRID_ABOVE_BUDGET) == "global"
    out, v_rgb, v_grids = _run(bg, ref)
    r_out, over_out = BU.ratio(out.cpu(), ref["out"], ref["bound_out"])
    r_rgb, over_rgb = BU.ratio(v_rgb.cpu(), ref["v_rgb"], ref["bound_v_rgb"], ~ref["borderline"])
    r_g, over_g = BU.ratio(v_grids.cpu(), ref["v_grids"], ref["bound_v_grids"])
    print(f"wave scene: out {r_out:.3f}, v_rgb {r_rgb:.3f}, v_grids {r_g:.3f} of the bound")
    assert over_out == 0 and over_rgb == 0
    assert over_g == 0, f"{over_g} elements of v_grids over the bound, the worst by {r_g:.2f} x"
    assert not bool(v_grids[0].any()) and not bool(v_grids[2].any())
    # the one-cell samples alone: the cells of a shared wave receive the sum of ALL its lanes
    only = dict(ref, v=torch.where(ref["shared"].view(1, 5, 70, 1), ref["v"], torch.zeros_like(ref["v"])))
    got = _run(bg, only)[2].cpu().double()
    want = BU.closed_form(ref["grids"].double(), ref["rgb"].double(), ref["xy"].double(), ref["idx"], only["v"].double())[2]
    assert int((want != 0).sum()) == 2 * 8 * 12                      # two cells' corners, all 12 channels
    assert bool(((got - want).abs() <= ref["bound_v_grids"]).all()) and torch.equal(got != 0, want != 0)
    record("bilagrid_wave_combined_over_bound", v_grids=r_g)


def test_a_shared_grid_is_the_sum_over_both_images(bg):
    ref = BU.reference("rand", (3, 4, 5), (2, 37, 53), (2, 2))
    parts = []
    for b in (0, 1):
        grids = ref["grids"].cuda().requires_grad_(True)
        out = bg.slice(grids, ref["xy"][b:b + 1].cuda(), ref["rgb"][b:b + 1].cuda(), torch.tensor([2], device="cuda"))["rgb"]
        out.backward(ref["v"][b:b + 1].cuda())
        parts.append(grids.grad)
    _, _, both = _run(bg, ref)
    # each side is inside its own bound of the float64 sum: the two differ by at most twice the bound
    assert bool(((both - (parts[0] + parts[1])).abs().cpu().double() <= 2 * ref["bound_v_grids"] + 2 * BU.U * both.abs().cpu().double()).all())
    assert not bool(both[:2].any())


def test_an_image_does_not_depend_on_its_batch(bg):
    for grid_size in ((8, 16, 16), (3, 4, 5)):
        ref = BU.reference("render_like", grid_size, (2, 37, 53), (0, 1))
        out, v_rgb, _ = _run(bg, ref)
        for b in (0, 1):
            rgb = ref["rgb"][b:b + 1].cuda().requires_grad_(True)
            one = bg.slice(ref["grids"].cuda(), ref["xy"][b:b + 1].cuda(), rgb, torch.tensor([b], device="cuda", dtype=torch.int32))["rgb"]
            one.backward(ref["v"][b:b + 1].cuda())
            assert torch.equal(one.detach(), out[b:b + 1]) and torch.equal(rgb.grad, v_rgb[b:b + 1]), (grid_size, b)


@pytest.mark.parametrize("shape", BU.TV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tv_value_and_gradient_within_their_bounds(bg, shape):
    case = BU.tv_case(shape)
    runs = []
    for _ in range(2):
        x = case["x"].cuda().requires_grad_(True)
        value = bg.total_variation_loss(x)
        assert value.dim() == 0 and value.dtype == torch.float32 and value.grad_fn is not None
        value.backward()
        runs.append((value.detach().clone(), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    err = abs(float(runs[0][0]) - case["value"])
    r, over = BU.ratio(runs[0][1].cpu(), case["grad"], case["bound_grad"])
    print(f"{shape}: value {float(runs[0][0]):.9g} (float64 {case['value']:.9g}), error {err:.3e} of {case['bound_value']:.3e}; "
          f"gradient {r:.3f} of the bound")
    assert err <= case["bound_value"], (shape, float(runs[0][0]), case["value"], case["bound_value"])
    assert over == 0, f"{shape}: {over} gradient elements over the bound, the worst by {r:.2f} x"
    record("bilagrid_tv_over_bound", shape=list(shape), value_ratio=err / case["bound_value"] if case["bound_value"] else 0.0,
           gradient_ratio=r)
    # a cotangent other than 1, and evaluation mode: the same value bits, nothing kept
    x = case["x"].cuda().requires_grad_(True)
    (0.25 * bg.total_variation_loss(x)).backward()
    _, b_grad = BU.tv_bounds(case["x"], 0.25)
    assert BU.ratio(x.grad.cpu(), 0.25 * case["grad"], b_grad)[1] == 0
    with torch.no_grad():
        plain = bg.total_variation_loss(x)
    assert plain.grad_fn is None and torch.equal(plain, runs[0][0])
    assert torch.equal(bg.total_variation_loss(case["x"].cuda()), runs[0][0])
    if shape[2:] == (8, 16, 16):
        m = bg.BilateralGrid(shape[0]).cuda()
        assert float(m.tv_loss().detach()) == 0.0                                   # identity grids: no variation
        with torch.no_grad():
            m.grids.copy_(case["x"].cuda())
        assert torch.equal(m.tv_loss().detach(), runs[0][0])


def _small_render(render_mode="RGB"):
    """200 Gaussians at 48 x 40: (render, means)"""
    from edgegaussians_amd import rasterization, synth
    W, H = 48, 40
    sc = synth.make_scene(200, 1, W, H, seed=5)
    g = torch.Generator().manual_seed(11)
    N = sc.means.shape[0]
    means = sc.means.cuda().requires_grad_(True)
    colors = (0.1 + 0.8 * torch.rand(N, 3, generator=g)).cuda()
    render, _, _ = rasterization(means, sc.quats.cuda(), torch.exp(sc.log_scales).cuda(),
                                 torch.sigmoid(sc.logit_opacities).squeeze(-1).cuda(), colors, sc.viewmats[:1].cuda(),
                                 sc.Ks[:1].cuda(), W, H, packed=False, render_mode=render_mode)
    return render, means


def _mesh(H, W, B):
    ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    return torch.stack([xs, ys], dim=-1).cuda()[None].expand(B, H, W, 2)


def test_layouts_give_the_bits_of_their_contiguous_copies(bg, monkeypatch):
    gen = torch.Generator().manual_seed(2)
    grids = torch.randn(1, 12, 8, 16, 16, generator=gen).cuda()
    copies = []
    real = torch.Tensor.contiguous

    def counting(self, *args, **kw):
        if self.dim() >= 3 and not self.is_contiguous():
            copies.append(tuple(self.shape))
        return real(self, *args, **kw)

    xy = _mesh(40, 48, 1)
    for mode in ("RGB", "RGB+D"):
        render = _small_render(mode)[0].detach()
        assert render.shape == (1, 40, 48, 3 if mode == "RGB" else 4)
        outs = []
        for in_place in (True, False):
            src = render.clone().requires_grad_(True)
            view = src if mode == "RGB" else src[..., :3]
            assert (mode == "RGB") == view.is_contiguous()
            arg, coords = (view, xy) if in_place else (real(view), real(xy))
            monkeypatch.setattr(torch.Tensor, "contiguous", counting)
            out = bg.slice(grids, coords, arg)["rgb"]
            monkeypatch.undo()
            out.backward(torch.ones_like(out))
            outs.append((out.detach(), src.grad.clone()))
            assert not bool(src.grad[..., 3:].any())
        assert not copies, f"a layout that is read in place went through .contiguous(): {copies}"
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), mode
    # xy expanded over the batch with stride 0
    ref = BU.reference("rand", (3, 4, 5), (2, 37, 53), (0, 1))
    xy0 = ref["xy"][0].cuda()[None].expand(2, 37, 53, 2)
    assert xy0.stride(0) == 0
    monkeypatch.setattr(torch.Tensor, "contiguous", counting)
    a = bg.slice(ref["grids"].cuda(), xy0, ref["rgb"].cuda(), torch.tensor([0, 1], device="cuda"))["rgb"]
    monkeypatch.undo()
    assert not copies
    assert torch.equal(a, _run(bg, ref, False, False)[0])
    # anything else takes one .contiguous(): the same bits; leading shapes other than [B, H, W]
    rgbT = ref["rgb"].cuda().permute(0, 2, 1, 3)                           # [B, W, H, 3]: dense, read in place
    xyT = ref["xy"].cuda().permute(0, 2, 1, 3)
    b = bg.slice(ref["grids"].cuda(), xyT, rgbT, torch.tensor([0, 1], device="cuda"))["rgb"]
    assert b.is_contiguous() and torch.equal(b, a.permute(0, 2, 1, 3))
    flat = bg.slice(ref["grids"].cuda(), ref["xy"].cuda().view(2, -1, 2), ref["rgb"].cuda().view(2, -1, 3),
                    torch.tensor([[0], [1]], device="cuda"))["rgb"]
    assert flat.shape == (2, 37 * 53, 3) and torch.equal(flat.view_as(a), a)
    five = bg.slice(ref["grids"].cuda(), ref["xy"].cuda().view(2, 37, 1, 53, 2), ref["rgb"].cuda().view(2, 37, 1, 53, 3),
                    torch.tensor([0, 1], device="cuda"))["rgb"]
    assert five.shape == (2, 37, 1, 53, 3) and torch.equal(five.view_as(a), a)
    strided = torch.zeros(2, 37, 53, 6, device="cuda")
    strided[..., ::2] = ref["rgb"].cuda()
    c = bg.slice(ref["grids"].cuda(), ref["xy"].cuda(), strided[..., ::2], torch.tensor([0, 1], device="cuda"))["rgb"]
    assert torch.equal(c, a)


def test_rasterization_slice_l1_against_the_torch_composition(bg):
    """means.grad and grids.grad of rasterization -> slice -> l1_loss against the same chain with the float32 torch
    composition (grid_sample + permute + affine product, F.l1_loss) at the project's parity figure for operator chains"""
    from edgegaussians_amd import losses
    from tests.util import assert_close
    gen = torch.Generator().manual_seed(4)
    eye = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0]).view(1, 12, 1, 1, 1)
    base = (eye + 0.2 * torch.randn(1, 12, 8, 16, 16, generator=gen)).cuda()
    target = torch.rand(1, 40, 48, 3, generator=gen).cuda()
    xy = _mesh(40, 48, 1)
    got = {}
    for kind in ("fused", "torch"):
        render, means = _small_render()
        grids = base.clone().requires_grad_(True)
        if kind == "fused":
            loss = losses.l1_loss(bg.slice(grids, xy, render)["rgb"], target)
        else:
            loss = F.l1_loss(BU.slice_grid_sample(grids, render, xy.contiguous(), [0]), target)
        loss.backward()
        got[kind] = (float(loss.detach()), means.grad.clone(), grids.grad.clone())
    assert abs(got["fused"][0] - got["torch"][0]) <= 1e-4 * abs(got["torch"][0])
    assert float(got["torch"][1].abs().max()) > 0 and float(got["torch"][2].abs().max()) > 0
    assert_close(got["fused"][1], got["torch"][1], rtol=1e-4, name="means.grad")
    assert_close(got["fused"][2], got["torch"][2], rtol=1e-4, name="grids.grad")


def test_evaluation_mode_saves_nothing_and_launches_no_backward(bg, monkeypatch):
    ref = BU.reference("rand", (3, 4, 5), (2, 37, 53), (0, 1))
    train = _run(bg, ref)[0]
    calls = []
    real = bg.call
    monkeypatch.setattr(bg, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    grids, rgb = ref["grids"].cuda().requires_grad_(True), ref["rgb"].cuda().requires_grad_(True)
    idx, xy = torch.tensor([0, 1], device="cuda"), ref["xy"].cuda()
    with torch.no_grad():
        out = bg.slice(grids, xy, rgb, idx)["rgb"]
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, train)
    out = bg.slice(grids.detach(), xy, rgb.detach(), idx)["rgb"]
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, train)
    assert calls == ["eg_bilagrid_slice_fwd"] * 2
    # only what requires a gradient gets one: without grids.requires_grad the scatter does not run
    seen = []
    monkeypatch.setattr(bg, "call", lambda name, *a: (seen.append((name, a[-3] is not None, a[-2] is not None)), real(name, *a))[1])
    out = bg.slice(grids.detach(), xy, rgb, idx)["rgb"]
    out.backward(ref["v"].cuda())
    assert grids.grad is None and seen[-1] == ("eg_bilagrid_slice_bwd", True, False)
    rgb_only = rgb.grad.clone()
    out = bg.slice(grids, xy, rgb.detach(), idx)["rgb"]
    out.backward(ref["v"].cuda())
    assert seen[-1] == ("eg_bilagrid_slice_bwd", False, True)
    both = _run(bg, ref)
    assert torch.equal(rgb_only, both[1])
    # a BilateralGrid in place of the tensor, grid_idx None with B == N
    m = bg.BilateralGrid(2, 5, 4, 3).cuda()
    with torch.no_grad():
        m.grids.copy_(ref["grids"][:2].cuda())
    out = bg.slice(m, xy, ref["rgb"].cuda())["rgb"]
    assert out.grad_fn is not None and torch.equal(out.detach(), train)
    assert "rgb_affine_mats" not in bg.slice(m, xy, ref["rgb"].cuda())


def test_refusals_on_device_tensors(bg):
    grids = torch.rand(2, 12, 3, 4, 5, device="cuda")
    rgb, xy = torch.rand(2, 6, 7, 3, device="cuda"), torch.rand(2, 6, 7, 2, device="cuda")
    with pytest.raises(ValueError, match="no CPU path"):
        bg.slice(grids, xy, rgb.cpu())
    with pytest.raises(ValueError, match="no CPU path"):
        bg.slice(grids, xy, rgb, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match=r"grid_idx must lie in \[0, 2\)"):
        bg.slice(grids, xy, rgb, torch.tensor([0, 2], device="cuda"))
    with pytest.raises(ValueError, match=r"grid_idx must lie in \[0, 2\)"):
        bg.slice(grids, xy, rgb, torch.tensor([-1, 1], device="cuda", dtype=torch.int32))
    # check_idx=False skips the read-back; an index outside the range is clamped into it by the kernels
    a = bg.slice(grids, xy, rgb, torch.tensor([0, 7], device="cuda"), check_idx=False)["rgb"]
    assert torch.equal(a, bg.slice(grids, xy, rgb, torch.tensor([0, 1], device="cuda"))["rgb"])
    with pytest.raises(TypeError, match="float32"):
        bg.slice(grids.half(), xy, rgb)
    with pytest.raises(ValueError, match="xy must not require grad"):
        bg.slice(grids, xy.clone().requires_grad_(True), rgb)
    with pytest.raises(ValueError, match="None only when B == N"):
        bg.slice(grids, xy[:1], rgb[:1])
    with pytest.raises(ValueError, match="contiguous"):
        bg.slice(grids.transpose(3, 4), xy, rgb)
    with pytest.raises(TypeError, match="float32"):
        bg.total_variation_loss(grids.double())
