"""Fused SSIM on the device (csrc/ssim.hip through edgegaussians_amd/ssim.py) against the float64 reference of
tests/ssim_util.py, every pixel inside its first-order bound; determinism, plane independence, layouts, evaluation mode,
the loss of a 3DGS trainer on a render of `rasterization`, and the refusals on device tensors."""
import pytest
import torch

from tests import ssim_util as SU
from tests.util import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ssim():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import ssim as mod
    assert (mod.TILE_H, mod.TILE_W) == (SU.TILE_H, SU.TILE_W)
    return mod


def _inputs(ref, layout, grad=True):
    a = SU.as_layout(ref["img1"].cuda(), layout)
    b = SU.as_layout(ref["img2"].cuda(), layout)
    return (a.requires_grad_(True) if grad else a), b


def _cases(scene):
    for shape in SU.SHAPES:
        for padding in SU.paddings_of(shape):
            for layout in SU.LAYOUTS:
                yield shape, padding, layout


@pytest.mark.parametrize("scene", SU.SCENES)
def test_map_every_pixel_within_the_bound(ssim, scene):
    for shape, padding, layout in _cases(scene):
        ref = SU.reference(scene, shape, padding)
        a, b = _inputs(ref, layout, grad=False)
        S = ssim.ssim_map(a, b, padding)
        assert S.shape == ref["S"].shape and S.dtype == torch.float32
        worst, over = SU.ratio(S.cpu(), ref["S"], ref["bound_S"])
        print(f"map {scene} {shape} {padding} {layout}: {worst:.3f} of the bound")
        record("ssim_map_over_bound", scene=scene, shape=list(shape), padding=padding, layout=layout, worst_ratio=worst,
               loose_share=SU.loose_share(ref["bound_S"], ref["S"]))
        assert over == 0, f"map {scene} {shape} {padding} {layout}: {over} pixels over the bound, the worst by {worst:.2f} x"


@pytest.mark.parametrize("scene", SU.SCENES)
def test_gradient_every_element_within_the_bound(ssim, scene):
    for shape, padding, layout in _cases(scene):
        ref = SU.reference(scene, shape, padding)
        # a random cotangent through ssim_map
        a, b = _inputs(ref, layout)
        ssim.ssim_map(a, b, padding).backward(ref["v"].cuda())
        w1, over1 = SU.ratio(a.grad.cpu(), ref["grad"], ref["bound_g"])
        # 1 / numel through fused_ssim
        a2, b2 = _inputs(ref, layout)
        ssim.fused_ssim(a2, b2, padding).backward()
        w2, over2 = SU.ratio(a2.grad.cpu(), ref["grad_mean"], ref["bound_g_mean"])
        print(f"gradient {scene} {shape} {padding} {layout}: {w1:.3f} (random v), {w2:.3f} (mean) of the bound")
        record("ssim_gradient_over_bound", scene=scene, shape=list(shape), padding=padding, layout=layout,
               worst_ratio_random_v=w1, worst_ratio_mean=w2, loose_share=SU.loose_share(ref["bound_g"], ref["grad"]))
        assert a.grad.shape == a.shape
        assert all(s == t for n, s, t in zip(a.shape, a.grad.stride(), a.stride()) if n > 1)  # (a dimension of 1 has no stride to keep)
        assert over1 == 0, f"gradient {scene} {shape} {padding} {layout}: {over1} elements over the bound, worst {w1:.2f} x"
        assert over2 == 0, f"mean gradient {scene} {shape} {padding} {layout}: {over2} elements over the bound, worst {w2:.2f} x"


@pytest.mark.parametrize("scene", SU.SCENES)
def test_scalar_within_the_mean_of_the_bound(ssim, scene):
    for shape, padding, layout in _cases(scene):
        ref = SU.reference(scene, shape, padding)
        a, b = _inputs(ref, layout)
        got = ssim.fused_ssim(a, b, padding)
        assert got.dim() == 0 and got.grad_fn is not None
        want, tol = float(ref["S"].mean()), float(ref["bound_S"].mean())
        err = abs(float(got.detach()) - want)
        print(f"scalar {scene} {shape} {padding} {layout}: {err:.3e} of {tol:.3e}")
        assert err <= tol, (scene, shape, padding, layout, float(got), want, tol)


def test_two_runs_are_bit_equal(ssim):
    shape = (2, 3, 2 * SU.TILE_H + 5, 2 * SU.TILE_W + 5)
    img1, img2 = SU.make_scene("render_like", shape)
    v = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    runs = []
    for _ in range(2):
        a = img1.cuda().requires_grad_(True)
        S = ssim.ssim_map(a, img2.cuda())
        S.backward(v)
        runs.append((S.detach().clone(), a.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_a_plane_does_not_depend_on_its_batch(ssim):
    shape = (2, 3, SU.TILE_H + 1, 2 * SU.TILE_W + 5)
    img1, img2 = SU.make_scene("rand", shape)
    v = torch.randn(shape, generator=torch.Generator().manual_seed(2)).cuda()
    a = img1.cuda().requires_grad_(True)
    S = ssim.ssim_map(a, img2.cuda())
    S.backward(v)
    for bi in range(shape[0]):
        for ci in range(shape[1]):
            a1 = img1[bi:bi + 1, ci:ci + 1].cuda().contiguous().requires_grad_(True)
            S1 = ssim.ssim_map(a1, img2[bi:bi + 1, ci:ci + 1].cuda().contiguous())
            S1.backward(v[bi:bi + 1, ci:ci + 1].contiguous())
            assert torch.equal(S1.detach(), S.detach()[bi:bi + 1, ci:ci + 1]), (bi, ci)
            assert torch.equal(a1.grad, a.grad[bi:bi + 1, ci:ci + 1]), (bi, ci)


def test_channels_last_view_is_read_in_place(ssim, monkeypatch):
    shape = (2, 3, SU.TILE_H + 1, SU.TILE_W + 7)
    img1, img2 = SU.make_scene("render_like", shape)
    v = torch.randn(shape, generator=torch.Generator().manual_seed(3)).cuda()
    a_cl = SU.as_layout(img1.cuda(), "channels_last").requires_grad_(True)
    b_cl = SU.as_layout(img2.cuda(), "channels_last")
    assert not a_cl.is_contiguous() and a_cl.stride() == (shape[1] * shape[2] * shape[3], 1, shape[3] * shape[1], shape[1])
    a_nc = a_cl.detach().contiguous().requires_grad_(True)
    b_nc = b_cl.contiguous()
    S_nc = ssim.ssim_map(a_nc, b_nc)
    S_nc.backward(v)
    copied = []
    real = torch.Tensor.contiguous

    def counting(self, *args, **kw):
        if self.shape == a_cl.shape and self.stride() == a_cl.stride():
            copied.append(self.data_ptr())
        return real(self, *args, **kw)

    monkeypatch.setattr(torch.Tensor, "contiguous", counting)
    S_cl = ssim.ssim_map(a_cl, b_cl)
    S_cl.backward(v)
    loss = ssim.fused_ssim(a_cl, b_nc)   # mixed layouts: each input through its own strides
    monkeypatch.undo()
    assert not copied, "a dense channels-last input went through .contiguous()"
    assert S_cl.is_contiguous() and torch.equal(S_cl.detach(), S_nc.detach())
    assert a_cl.grad.stride() == a_cl.stride() and torch.equal(a_cl.grad, a_nc.grad)
    assert torch.equal(loss.detach(), ssim.fused_ssim(a_nc, b_nc).detach())
    # any other stride pattern takes one .contiguous() and gives the same bits
    wide = torch.zeros(shape[0], shape[1], shape[2], shape[3] + 3, device="cuda")
    wide[..., :shape[3]] = a_nc.detach()
    a_sl = wide[..., :shape[3]].requires_grad_(True)
    S_sl = ssim.ssim_map(a_sl, b_nc)
    S_sl.backward(v)
    assert torch.equal(S_sl.detach(), S_nc.detach()) and torch.equal(a_sl.grad, a_nc.grad)


def test_evaluation_mode_allocates_one_map(ssim):
    shape = (1, 3, 4 * SU.TILE_H, 4 * SU.TILE_W)
    img1, img2 = SU.make_scene("render_like", shape)
    a, b = img1.cuda().requires_grad_(True), img2.cuda()
    want = ssim.fused_ssim(a, b)
    assert want.grad_fn is not None
    map_bytes = 4 * a.numel()
    del want
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
            return ssim.fused_ssim(a, b)

    for kind, fn in (("train=False", lambda: ssim.fused_ssim(a, b, train=False)), ("no_grad", under_no_grad),
                     ("no requires_grad", lambda: ssim.fused_ssim(a_plain, b))):
        out, grown = peak_growth(fn)
        assert out.grad_fn is None and not out.requires_grad, kind
        assert map_bytes <= grown < 2 * map_bytes, (kind, grown, map_bytes)  # one map (and the scalar), not four
        del out
    S, grown = peak_growth(lambda: ssim.ssim_map(a, b))
    assert grown >= 4 * map_bytes  # the map and the three derivative maps
    del S
    train = ssim.fused_ssim(a, b)
    evalv = ssim.fused_ssim(a, b, train=False)
    assert evalv.grad_fn is None and train.grad_fn is not None
    assert torch.equal(evalv, train.detach())
    with torch.no_grad():
        assert torch.equal(ssim.fused_ssim(a, b), train.detach())
    assert torch.equal(ssim.fused_ssim(a.detach(), b), train.detach())
    assert torch.equal(ssim.fused_ssim(a, b, "valid", train=False), ssim.fused_ssim(a, b, "valid").detach())


def test_trainer_loss_on_a_render_of_rasterization(ssim):
    """0.8 L1 + 0.2 (1 - SSIM) of a 3DGS trainer on `rasterization`'s render, read in place through its permuted view:
    render.grad against the float64 reference's gradient on the same device render (not through the compositing
    backward: its atomics vary run to run)."""
    from edgegaussians_amd import rasterization, synth
    from fused_ssim import fused_ssim
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
    gt = torch.rand(1, 3, H, W, generator=g).cuda()
    render, _, _ = rasterization(means, sc.quats.cuda(), torch.exp(sc.log_scales).cuda(),
                                 torch.sigmoid(sc.logit_opacities).squeeze(-1).cuda(), colors, sc.viewmats[:1].cuda(),
                                 sc.Ks[:1].cuda(), W, H, packed=False)
    assert render.shape == (1, H, W, 3)
    render.retain_grad()
    pred = render.permute(0, 3, 1, 2)
    loss = 0.8 * (pred - gt).abs().mean() + 0.2 * (1.0 - fused_ssim(pred, gt))
    loss.backward()
    assert render.grad is not None and means.grad is not None
    assert bool(torch.isfinite(means.grad).all()) and float(means.grad.abs().max()) > 0
    x1, x2 = pred.detach().cpu().contiguous(), gt.cpu()
    n = x1.numel()
    v_mean = torch.full(x1.shape, 1.0 / n, dtype=torch.float32)
    g_ssim = SU.ssim_grad_autograd(x1.double(), x2.double(), v_mean.double())
    l1 = 0.8 * torch.sign(x1.double() - x2.double()) / n
    want = l1 - 0.2 * g_ssim
    bound_S, bound_g = SU.bounds(x1, x2, v_mean)
    # the L1 term's share is exact up to the roundings of 0.8 / n, of -0.2 / n and of the sum of the two gradients
    bound = 0.2 * bound_g + 4 * SU.U_ROUND * (l1.abs() + 0.2 * g_ssim.abs())
    worst, over = SU.ratio(render.grad.permute(0, 3, 1, 2).cpu(), want, bound)
    print(f"trainer loss: render.grad at {worst:.3f} of the bound")
    record("ssim_trainer_loss_render_grad", worst_ratio=worst, gaussians=N, width=W, height=H)
    assert over == 0, f"{over} elements of render.grad over the bound, the worst by {worst:.2f} x"
    # the loss itself: the SSIM term within 0.2 x the mean of its bound; the fp32 L1 mean (a subtraction, a tree sum of
    # depth <= log2(n) + 1 and a division) and the operations that combine the terms: log2(n) + 8 roundings of the
    # terms' sizes
    l1_64, ssim_64 = float((x1.double() - x2.double()).abs().mean()), float(SU.ssim_map_ref(x1.double(), x2.double()).mean())
    want_loss = 0.8 * l1_64 + 0.2 * (1.0 - ssim_64)
    tol = 0.2 * float(bound_S.mean()) + (n.bit_length() + 8) * SU.U_ROUND * (0.8 * l1_64 + 0.2 + 0.2 * abs(ssim_64))
    assert abs(float(loss.detach()) - want_loss) <= tol, (float(loss.detach()), want_loss, tol)


def test_refusals_on_device_tensors(ssim):
    a, b = torch.rand(1, 3, 12, 12, device="cuda"), torch.rand(1, 3, 12, 12, device="cuda")
    with pytest.raises(ValueError, match="H, W >= 11"):
        ssim.fused_ssim(a[:, :, :10], b[:, :, :10], padding="valid")
    with pytest.raises(ValueError, match="symmetric.*first"):
        ssim.ssim_map(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="one shape"):
        ssim.fused_ssim(a, b[..., :11])
    with pytest.raises(ValueError, match="no CPU path"):
        ssim.fused_ssim(a, b.cpu())
    with pytest.raises(TypeError, match="float32"):
        ssim.ssim_map(a.half(), b.half())
    assert ssim.ssim_map(a[:, :, :11, :11], b[:, :, :11, :11], "valid").shape == (1, 3, 1, 1)
