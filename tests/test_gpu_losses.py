"""The scalar image losses on the device (csrc/losses.hip and the photometric kernels of csrc/ssim.hip through
edgegaussians_amd/losses.py) against the float64 statements of tests/losses_util.py: values inside the sum bound,
every gradient element inside its bound with exact zeros, the same bits across layouts and runs, evaluation mode, the
losses on a render of `rasterization`, and the refusals on device tensors.

The pointwise shapes (losses_util.SHAPES) are stated in the kernels' constants: (1, 1, 1, WG_ELEMS + 1) is one element
more than a workgroup covers, (1, 1, FIN_LANES + 1, WG_ELEMS) one workgroup more than the finalize wave has lanes --
with WG_ELEMS = 1024 and FIN_LANES = 64 that one, 66 560 elements, is larger than (1, 3, 64, 65)."""
import pytest
import torch

from tests import losses_util as LU
from tests import ssim_util as SU
from tests.util import record

pytestmark = pytest.mark.gpu

LAYOUTS = ("contiguous", "channels_last", "render_view")


@pytest.fixture(scope="module")
def losses():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import losses as mod
    assert (mod.WG_ELEMS, mod.FIN_LANES) == (LU.WG_ELEMS, LU.FIN_LANES)
    return mod


def _laid_out(t, shape, layout):
    """(the leaf that receives the gradient, the operand) of the CPU tensor t [shape] on the device: contiguous in its
    own shape; the permute(0, 3, 1, 2) view of a contiguous [B, H, W, C]; element 0 of a trailing dimension of 3 (what
    render[0, ..., 0] is: dense up to one skipped stride)"""
    if layout == "contiguous":
        leaf = t.cuda().requires_grad_(True)
        return leaf, leaf
    t4 = t.reshape(LU.shape4(shape)).cuda()
    if layout == "channels_last":
        leaf = t4.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        return leaf, leaf.permute(0, 3, 1, 2)
    leaf = torch.rand(*t4.shape, 3, device="cuda")
    leaf[..., 0] = t4
    leaf.requires_grad_(True)
    return leaf, leaf[..., 0]


def _grad_of(leaf, shape, layout):
    """the gradient of the operand, in the logical 4-D shape"""
    if layout == "contiguous":
        return leaf.grad.reshape(LU.shape4(shape))
    if layout == "channels_last":
        return leaf.grad.permute(0, 3, 1, 2)
    assert not bool(leaf.grad[..., 1:].any())
    return leaf.grad[..., 0]


@pytest.mark.parametrize("shape", LU.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradient_within_the_bounds_and_bit_equal_across_layouts(losses, shape):
    x, y, _, _ = LU.inputs(shape)
    s4 = LU.shape4(shape)
    worst_v = worst_g = 0.0
    for weighting, kind, clamp, reduction in LU.pointwise_cases():
        ref = LU.pointwise_case(shape, weighting, kind, clamp, reduction)
        w = LU.weights_of(shape, weighting)
        values, grads = [], []
        for layout in LAYOUTS:
            leaf, xd = _laid_out(x, shape, layout)
            four_d = layout != "contiguous"
            yd = y.reshape(s4).cuda() if four_d else y.cuda()
            if w is None:
                wd = None
            elif w.dtype == torch.bool:
                wd = w.reshape(s4).cuda() if four_d else w.cuda()
            else:  # [H, W, 1] on the device, expanded: strides 0 on the batch and the channels
                B, C, H, W = s4
                wd = LU.inputs(shape)[2].cuda().expand(H, W, C).permute(2, 0, 1)
                assert C == 1 or wd.stride(0) == 0
                if not four_d and wd.dim() > len(shape):
                    wd = wd[(0,) * (wd.dim() - len(shape))]
            for run in range(3 if layout == "contiguous" else 1):
                leaf.grad = None
                got = losses.image_loss(xd, yd, wd, kind=kind, clamp=clamp, reduction=reduction)
                assert got.dim() == 0 and got.dtype == torch.float32 and got.grad_fn is not None
                got.backward()
                values.append(got.detach().clone())
                grads.append(_grad_of(leaf, shape, layout).detach().clone())
        tag = (shape, weighting, kind, clamp, reduction)
        got = float(values[0])
        err = abs(got - ref["value"])
        print(f"{tag}: value {got:.9g} (float64 {ref['value']:.9g}), error {err:.3e} of {ref['bound_value']:.3e}")
        assert LU.check_value(got, ref["value"], ref["bound_value"]), (tag, got, ref["value"], ref["bound_value"])
        if ref["bound_value"] > 0:
            worst_v = max(worst_v, err / ref["bound_value"])
        g0 = grads[0].cpu().reshape(shape)
        r, over = SU.ratio(g0, ref["grad"], ref["bound_grad"])   # (a bound of zero demands an exact zero)
        assert over == 0, f"{tag}: {over} gradient elements over the bound, the worst by {r:.2f} x"
        worst_g = max(worst_g, r)
        for v in values[1:]:      # three runs, then the other layouts
            assert torch.equal(v.view(torch.int32), values[0].view(torch.int32)) or (torch.isnan(v) and torch.isnan(values[0])), tag
        for g in grads[1:]:
            assert torch.equal(g, grads[0]), tag
    record("losses_pointwise_over_bound", shape=list(shape), worst_value_ratio=worst_v, worst_gradient_ratio=worst_g)


@pytest.mark.parametrize("shape", [(2, 3, 7, 5), (1, 3, 64, 64), (1, 3, 64, 65)], ids=lambda s: "x".join(map(str, s)))
def test_stride_zero_target_and_an_all_false_mask(losses, shape):
    x, y, _, _ = LU.inputs(shape)
    row = y[:1, :1, :1].cuda()                         # [1, 1, 1, W]: broadcast over B, C and H
    expanded, material = row.expand(shape), row.expand(shape).contiguous()
    assert all(st == 0 for n, st in zip(shape[:3], expanded.stride()[:3]) if n > 1)   # (an expand to size 1 keeps its stride)
    out = []
    for target in (expanded, material, row):
        a = x.cuda().requires_grad_(True)
        loss = losses.image_loss(a, target, kind="l2", clamp=True)
        loss.backward()
        out.append((loss.detach(), a.grad))
    for loss, grad in out[1:]:
        assert torch.equal(loss, out[0][0]) and torch.equal(grad, out[0][1])
    x64, y64 = x.double(), row.cpu().double().expand(shape)
    t = LU.terms(x64, y64, None, "l2", True)
    assert abs(float(out[0][0]) - float(t.mean())) <= LU.sum_bound(t, t.numel())
    g64 = LU.image_grad_ref(x64, y64, None, "l2", True)
    r, over = SU.ratio(out[0][1].cpu(), g64, LU.grad_bound(g64))
    assert over == 0, r
    # nothing selected: nan with a gradient of exact zeros, as F.l1_loss(input[mask], target[mask])
    a = x.cuda().requires_grad_(True)
    loss = losses.masked_l1_loss(a, y.cuda(), torch.zeros(shape, dtype=torch.bool, device="cuda"))
    loss.backward()
    assert bool(torch.isnan(loss)) and not bool(a.grad.any())


def test_named_losses_are_the_general_form(losses):
    shape = (2, 3, 7, 5)
    x, y, wbase, mask = LU.inputs(shape)
    a, b, m = x.cuda(), y.cuda(), mask.cuda()
    w = wbase.cuda().expand(7, 5, 3).permute(2, 0, 1)
    assert torch.equal(losses.l1_loss(a, b), losses.image_loss(a, b))
    assert torch.equal(losses.mse_loss(a, b), losses.image_loss(a, b, kind="l2"))
    assert torch.equal(losses.weighted_l1_loss(a, b, w), losses.image_loss(a, b, w))
    assert torch.equal(losses.masked_l1_loss(a, b, m), losses.image_loss(a, b, m))
    assert torch.equal(losses.projection_loss(a, b, w), losses.image_loss(a, b, w, clamp=True, reduction="sum"))
    got = losses.l1_loss(a, b)
    assert got.grad_fn is None and not got.requires_grad
    train = losses.l1_loss(a.clone().requires_grad_(True), b)
    assert train.grad_fn is not None and torch.equal(train.detach(), got)      # evaluation mode: the same bits
    with torch.no_grad():
        assert torch.equal(losses.l1_loss(a.clone().requires_grad_(True), b), got)
    # any other stride pattern takes one .contiguous() and gives the same bits
    wide = torch.zeros(2, 3, 7, 9, device="cuda")
    wide[..., :5] = a
    sliced = wide[..., :5].requires_grad_(True)
    a2 = a.clone().requires_grad_(True)
    losses.mse_loss(sliced, b).backward()
    losses.mse_loss(a2, b).backward()
    assert torch.equal(sliced.grad, a2.grad)


def _photo_inputs(ref, layout, grad=True):
    a = SU.as_layout(ref["img1"].cuda(), layout)
    b = SU.as_layout(ref["img2"].cuda(), layout)
    return (a.requires_grad_(True) if grad else a), b


@pytest.mark.parametrize("scene", SU.SCENES)
def test_photometric_value_and_gradient_within_the_bounds(losses, scene):
    from edgegaussians_amd.ssim import fused_ssim
    worst = [0.0, 0.0]
    for shape in SU.SHAPES:
        for padding in SU.paddings_of(shape):
            ref = SU.reference(scene, shape, padding)
            for layout in SU.LAYOUTS:
                for lam in LU.LAMBDAS:
                    case = LU.photometric_case(scene, shape, padding, lam)
                    a, b = _photo_inputs(ref, layout)
                    loss, l1, s = losses.photometric_loss(a, b, lam, padding, return_terms=True)
                    assert loss.dim() == 0 and loss.grad_fn is not None and not l1.requires_grad and not s.requires_grad
                    loss.backward()
                    tag = (scene, shape, padding, layout, lam)
                    err = abs(float(loss.detach()) - case["loss"])
                    r, over = SU.ratio(a.grad.cpu(), case["grad"], case["bound_grad"])
                    print(f"{tag}: loss error {err:.3e} of {case['bound_loss']:.3e}, gradient {r:.3f} of the bound")
                    assert err <= case["bound_loss"], (tag, float(loss.detach()), case["loss"], case["bound_loss"])
                    assert over == 0, f"{tag}: {over} gradient elements over the bound, the worst by {r:.2f} x"
                    assert all(p == q for n, p, q in zip(a.shape, a.grad.stride(), a.stride()) if n > 1)
                    worst[0], worst[1] = max(worst[0], err / case["bound_loss"]), max(worst[1], r)
                    # the terms: the pointwise L1 mean and fused_ssim, each inside the two bounds
                    b_l1, b_s = LU.photometric_term_bounds(ref, case["l1"])
                    assert abs(float(l1) - case["l1"]) <= b_l1 and abs(float(s) - case["s"]) <= b_s, tag
                    if lam == 0.2:
                        n = a.numel()
                        t = (ref["img1"].double() - ref["img2"].double()).abs()
                        assert abs(float(l1) - float(losses.l1_loss(a.detach(), b))) <= b_l1 + LU.sum_bound(t, n), tag
                        tol = b_s + float(ref["bound_S"].mean()) + (n.bit_length() + 2) * LU.U * float(ref["S"].abs().mean())
                        assert abs(float(s) - float(fused_ssim(a.detach(), b, padding))) <= tol, tag
                    if lam == 0.0:      # the pointwise L1's gradient, bit for bit
                        a1, b1 = _photo_inputs(ref, layout)
                        losses.l1_loss(a1, b1).backward()
                        assert torch.equal(a.grad, a1.grad), tag
                    # evaluation mode: the same bits
                    with torch.no_grad():
                        assert torch.equal(losses.photometric_loss(a, b, lam, padding), loss.detach()), tag
    record("losses_photometric_over_bound", scene=scene, worst_loss_ratio=worst[0], worst_gradient_ratio=worst[1],
           loose_share=max(SU.loose_share(LU.photometric_case(scene, sh, p, 0.2)["bound_grad"],
                                          LU.photometric_case(scene, sh, p, 0.2)["grad"])
                           for sh in SU.SHAPES for p in SU.paddings_of(sh)))


def test_photometric_runs_and_layouts_are_bit_equal(losses):
    shape = (2, 3, 2 * SU.TILE_H + 5, 2 * SU.TILE_W + 5)
    img1, img2 = SU.make_scene("render_like", shape)
    runs = []
    for layout in ("nchw", "nchw", "nchw", "channels_last"):
        a = SU.as_layout(img1.cuda(), layout).requires_grad_(True)
        loss = losses.photometric_loss(a, SU.as_layout(img2.cuda(), layout), 0.2, "valid")
        loss.backward()
        runs.append((loss.detach().clone(), a.grad.clone()))
    for loss, grad in runs[1:]:
        assert torch.equal(loss, runs[0][0]) and torch.equal(grad, runs[0][1])


def test_evaluation_mode_allocates_no_derivative_maps(losses):
    shape = (1, 3, 4 * SU.TILE_H, 4 * SU.TILE_W)
    img1, img2 = SU.make_scene("render_like", shape)
    a, b = img1.cuda().requires_grad_(True), img2.cuda()
    map_bytes = 4 * a.numel()
    train = losses.photometric_loss(a, b).detach().clone()
    torch.cuda.synchronize()
    a_plain = a.detach()

    def peak_growth(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        return out, torch.cuda.max_memory_allocated() - base

    def under_no_grad():
        with torch.no_grad():
            return losses.photometric_loss(a, b)

    for kind, fn in (("no_grad", under_no_grad), ("no requires_grad", lambda: losses.photometric_loss(a_plain, b))):
        out, grown = peak_growth(fn)
        assert out.grad_fn is None and not out.requires_grad, kind
        assert grown < map_bytes, (kind, grown, map_bytes)       # the slab and the scalars: no map at all
        assert torch.equal(out, train), kind
        del out
    out, grown = peak_growth(lambda: losses.photometric_loss(a, b))
    assert 3 * map_bytes <= grown < 4 * map_bytes, (grown, map_bytes)   # the three derivative maps, no S, no cotangent map
    del out
    out, grown = peak_growth(lambda: losses.l1_loss(a_plain, b))
    assert grown < map_bytes and out.grad_fn is None


def _render(channels_gt):
    """the small scene of test_gpu_ssim.py's trainer-loss case: (render [1, H, W, 3] with retain_grad, means, gt)"""
    from edgegaussians_amd import rasterization, synth
    from tests import ortho_util as OU
    from tests import util as U
    a = OU.WHOLE_ARGS
    W, H = U.PROJ_SIZE
    sc = synth.make_scene(a["n_gauss"], a["n_views"], W, H, seed=a["seed"], spread_opacity=a["spread_opacity"],
                          scale=a["scale"], anisotropy=a["anisotropy"])
    g = torch.Generator().manual_seed(11)
    N = sc.means.shape[0]
    means = sc.means.cuda().requires_grad_(True)
    colors = (0.2 + 0.8 * torch.rand(N, 3, generator=g)).cuda()
    gt = torch.rand((1, 3, H, W) if channels_gt else (H, W), generator=g)
    render, _, _ = rasterization(means, sc.quats.cuda(), torch.exp(sc.log_scales).cuda(),
                                 torch.sigmoid(sc.logit_opacities).squeeze(-1).cuda(), colors, sc.viewmats[:1].cuda(),
                                 sc.Ks[:1].cuda(), W, H, packed=False)
    assert render.shape == (1, H, W, 3)
    render.retain_grad()
    return render, means, gt


def test_projection_loss_on_a_render_of_rasterization(losses, monkeypatch):
    """projection_loss on render[0, ..., 0], read in place, against the reference's torch chain: the loss inside the sum
    bound, render.grad inside the element bound on the float64 statement of the same device render (not through the
    compositing backward: its atomics vary run to run), exact zeros in the other channels"""
    from edgegaussians_amd import synth
    render, means, gt = _render(False)
    gt = (gt > 0.8).float() * gt          # an edge map: mostly background
    wmap = synth.weight_map("weighted", gt)
    pred = render[0, ..., 0]
    copies = []
    real = torch.Tensor.contiguous

    def counting(self, *args, **kw):
        if self.shape[-2:] == pred.shape and not self.is_contiguous():
            copies.append(tuple(self.stride()))
        return real(self, *args, **kw)

    monkeypatch.setattr(torch.Tensor, "contiguous", counting)
    loss = losses.projection_loss(pred, gt.cuda(), wmap.cuda())
    monkeypatch.undo()
    assert not copies, "the channel view of the render went through .contiguous()"
    chain = (wmap.cuda() * torch.abs(torch.clamp(pred.detach(), 0.0, 1.0) - gt.cuda())).sum()   # the reference's chain
    loss.backward()
    assert means.grad is not None and bool(torch.isfinite(means.grad).all()) and float(means.grad.abs().max()) > 0
    x64 = pred.detach().cpu().double()
    t = LU.terms(x64, gt.double(), wmap.double(), "l1", True)
    want = float(t.sum())
    bound = LU.sum_bound(t, 1.0)
    print(f"projection loss {float(loss):.9g}, float64 {want:.9g}, torch chain {float(chain):.9g}, bound {bound:.3e}")
    assert abs(float(loss.detach()) - want) <= bound
    # torch's chain: the same term roundings and a tree sum of depth <= log2(n) + 1
    assert abs(float(chain) - want) <= (t.numel().bit_length() + 1 + LU.TERM_ROUNDINGS) * LU.U * want
    g64 = LU.image_grad_ref(x64, gt.double(), wmap.double(), "l1", True, "sum")
    r, over = SU.ratio(render.grad[0, ..., 0].cpu(), g64, LU.grad_bound(g64))
    record("losses_projection_render_grad", worst_ratio=r)
    assert over == 0, f"{over} elements of render.grad over the bound, the worst by {r:.2f} x"
    assert not bool(render.grad[..., 1:].any())


def test_photometric_loss_on_a_render_of_rasterization(losses):
    """photometric_loss on the permuted view of the render against 0.8 l1 + 0.2 (1 - fused_ssim): the tolerances of
    test_gpu_ssim.py's trainer-loss case"""
    from fused_ssim import fused_ssim
    render, means, gt = _render(True)
    gt = gt.cuda()
    pred = render.permute(0, 3, 1, 2)
    loss = losses.photometric_loss(pred, gt, 0.2)
    loss.backward()
    assert means.grad is not None and bool(torch.isfinite(means.grad).all()) and float(means.grad.abs().max()) > 0
    composed = 0.8 * (pred.detach() - gt).abs().mean() + 0.2 * (1.0 - fused_ssim(pred.detach(), gt))
    x1, x2 = pred.detach().cpu().contiguous(), gt.cpu()
    n = x1.numel()
    v_mean = torch.full(x1.shape, 1.0 / n, dtype=torch.float32)
    g_ssim = SU.ssim_grad_autograd(x1.double(), x2.double(), v_mean.double())
    l1 = 0.8 * torch.sign(x1.double() - x2.double()) / n
    want = l1 - 0.2 * g_ssim
    bound_S, bound_g = SU.bounds(x1, x2, v_mean)
    bound = 0.2 * bound_g + 4 * SU.U_ROUND * (l1.abs() + 0.2 * g_ssim.abs())
    worst, over = SU.ratio(render.grad.permute(0, 3, 1, 2).cpu(), want, bound)
    record("losses_photometric_render_grad", worst_ratio=worst)
    assert over == 0, f"{over} elements of render.grad over the bound, the worst by {worst:.2f} x"
    l1_64, ssim_64 = float((x1.double() - x2.double()).abs().mean()), float(SU.ssim_map_ref(x1.double(), x2.double()).mean())
    want_loss = 0.8 * l1_64 + 0.2 * (1.0 - ssim_64)
    tol = 0.2 * float(bound_S.mean()) + (n.bit_length() + 8) * SU.U_ROUND * (0.8 * l1_64 + 0.2 + 0.2 * abs(ssim_64))
    print(f"photometric loss {float(loss):.9g}, composed {float(composed):.9g}, float64 {want_loss:.9g}, tolerance {tol:.3e}")
    assert abs(float(loss.detach()) - want_loss) <= tol and abs(float(composed) - want_loss) <= tol


def test_refusals_on_device_tensors(losses):
    a, b = torch.rand(1, 3, 12, 12, device="cuda"), torch.rand(1, 3, 12, 12, device="cuda")
    with pytest.raises(ValueError, match="no CPU path"):
        losses.l1_loss(a, b.cpu())
    with pytest.raises(ValueError, match="no CPU path"):
        losses.weighted_l1_loss(a, b, torch.rand(12, 12))
    with pytest.raises(ValueError, match="not broadcastable"):
        losses.l1_loss(a, b[..., :11])
    with pytest.raises(TypeError, match="float32"):
        losses.mse_loss(a.half(), b.half())
    with pytest.raises(TypeError, match="torch.bool"):
        losses.masked_l1_loss(a, b, torch.ones(12, 12, device="cuda"))
    with pytest.raises(ValueError, match="target must not require grad"):
        losses.l1_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="reduction"):
        losses.image_loss(a, b, reduction="none")
    with pytest.raises(ValueError, match="H, W >= 11"):
        losses.photometric_loss(a[:, :, :10], b[:, :, :10], padding="valid")
    with pytest.raises(ValueError, match="symmetric.*first"):
        losses.photometric_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="no CPU path"):
        losses.photometric_loss(a, b.cpu())
    assert losses.photometric_loss(a[:, :, :11, :11], b[:, :, :11, :11], padding="valid").dim() == 0
