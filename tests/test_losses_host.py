"""The scalar image losses without a device: the float64 statements of tests/losses_util.py against torch's own losses,
literal restatements of the reference's loss classes and its recorded values; the closed-form gradients against
autograd; the rounding bounds on the fp32 model of the kernels and on mutants of it; the loose share of the combined
photometric bound; the exports, the refusals in their order and the C ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import losses_util as LU
from tests import ssim_util as SU
from tests.util import record_cpu


def _rand64(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 1.5 - 0.25,
            torch.rand(shape, generator=g, dtype=torch.float64))


# ---- the reference's two loss classes, restated literally (models/losses.py)
def _reference_masked_l1(input, target, mask):
    return F.l1_loss(input[mask], target[mask])


def _reference_weighted_l1(input, target, weights):
    return torch.mean(weights * torch.abs(input - target))


@pytest.mark.parametrize("shape", [(1,), (7, 5), (2, 3, 7, 5)])
def test_statements_are_torchs_losses_and_the_references_classes(shape):
    x, y = _rand64(shape, 1)
    g = torch.Generator().manual_seed(2)
    w = torch.rand(shape, generator=g, dtype=torch.float64)
    mask = torch.rand(shape, generator=g) > 0.5
    mask.view(-1)[0] = True
    assert abs(float(LU.l1_loss_ref(x, y) - F.l1_loss(x, y))) <= 1e-15
    assert abs(float(LU.mse_loss_ref(x, y) - F.mse_loss(x, y))) <= 1e-15
    assert abs(float(LU.weighted_l1_loss_ref(x, y, w) - _reference_weighted_l1(x, y, w))) <= 1e-15
    assert abs(float(LU.masked_l1_loss_ref(x, y, mask) - _reference_masked_l1(x, y, mask))) <= 1e-15
    assert abs(float(LU.projection_loss_ref(x, y, w) - (w * (x.clamp(0, 1) - y).abs()).sum())) <= 1e-13
    assert abs(float(LU.image_loss_ref(x, y, w, "l2", True, "sum") - (w * (x.clamp(0, 1) - y) ** 2).sum())) <= 1e-13


def test_statements_give_the_recorded_reference_values(golden_dir):
    from edgegaussians_amd import synth
    from tests.test_golden import _crop_gt
    d = np.load(os.path.join(golden_dir, "losses.npz"))
    gt32 = _crop_gt(golden_dir, d)
    gt, pred = gt32.double(), torch.from_numpy(d["pred"]).double()
    edge = gt32 >= 0.5
    hw = edge.numel()
    weight_mask = (synth.weight_map("weighted", gt32) * hw).double()
    H, W = edge.shape
    sel = torch.zeros(H * W, dtype=torch.bool)
    sel[torch.from_numpy(d["randperm_head"]).long() % (H * W)] = True   # the recorded draw, as test_golden.py replays it
    sel = sel.view(H, W)

    def close(got, name, rel=2e-6):
        assert abs(float(got) - float(d[name])) <= rel * abs(float(d[name])) + 1e-9, (name, float(got), float(d[name]))

    close(LU.l1_loss_ref(pred, gt), "loss_whole")
    close(LU.weighted_l1_loss_ref(pred, gt, weight_mask), "loss_weighted")
    close(LU.weighted_l1_loss_ref(pred, gt, weight_mask), "weighted_l1")
    close(LU.masked_l1_loss_ref(pred, gt, edge), "masked_l1")
    close(LU.masked_l1_loss_ref(pred, gt, edge) + LU.masked_l1_loss_ref(pred, gt, sel), "loss_bg_edge_ratio")
    # ... and the weight-map form the trainer and projection_loss use
    close(LU.projection_loss_ref(pred, gt, synth.weight_map("whole", gt32).double()), "loss_whole")
    close(LU.projection_loss_ref(pred, gt, synth.weight_map("weighted", gt32).double()), "loss_weighted")


def _special(shape, seed):
    """x with exact ties: x == y, x exactly 0 and exactly 1"""
    x, y = _rand64(shape, seed)
    fx, fy = x.view(-1), y.view(-1)
    fx[0::7] = fy[0::7]
    fx[1::7] = 0.0
    fx[2::7] = 1.0
    fy[2::14] = 1.0
    return x, y


@pytest.mark.parametrize("weighting", LU.WEIGHTINGS + ("all_false_mask",))
@pytest.mark.parametrize("kind", LU.KINDS)
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("reduction", LU.REDUCTIONS)
def test_closed_form_gradient_is_autograd(weighting, kind, clamp, reduction):
    shape = (2, 3, 7, 5)
    x, y = _special(shape, 3)
    g = torch.Generator().manual_seed(4)
    w = {"none": None, "weights": torch.rand(shape, generator=g, dtype=torch.float64) * (torch.rand(shape, generator=g) > 0.2),
         "mask": torch.rand(shape, generator=g) > 0.5, "all_false_mask": torch.zeros(shape, dtype=torch.bool)}[weighting]
    xa = x.clone().requires_grad_(True)
    # torch's own formulation: index with the mask, clamp, abs / square, mean or sum
    d = (xa.clamp(0.0, 1.0) if clamp else xa) - y
    t = d.abs() if kind == "l1" else d * d
    if w is not None and w.dtype == torch.bool:
        sel = t[w]
        loss = sel.mean() if reduction == "mean" else sel.sum()
    else:
        t = t if w is None else w * t
        loss = t.mean() if reduction == "mean" else t.sum()
    v = 0.7
    want = torch.autograd.grad(loss, xa, torch.tensor(v, dtype=torch.float64))[0]
    got = LU.image_grad_ref(x, y, w, kind, clamp, reduction, v)
    assert float((got - want).abs().max()) <= 1e-15 * max(1.0, float(want.abs().max()))
    assert torch.equal(got == 0, want == 0)       # sign(0) = 0, the closed clamp gate, masked-out elements
    value = LU.image_loss_ref(x, y, w, kind, clamp, reduction)
    assert torch.allclose(value, loss.detach(), rtol=1e-14, atol=0, equal_nan=True)
    if weighting == "all_false_mask" and reduction == "mean":
        assert bool(torch.isnan(value)) and not bool(got.any())   # nan with a zero gradient, as torch


def test_photometric_gradient_is_autograd():
    shape = (1, 2, 12, 23)
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)
    for padding in ("same", "valid"):
        ms = SU.map_shape(shape, padding)
        v_mean = torch.full(ms, 1.0 / torch.Size(ms).numel(), dtype=torch.float64)
        grad_mean = SU.ssim_grad_closed(x1, x2, v_mean, padding)
        for lam in LU.LAMBDAS:
            xa = x1.clone().requires_grad_(True)
            loss, _, _ = LU.photometric_ref(xa, x2, lam, padding)
            want = torch.autograd.grad(loss, xa)[0]
            got = LU.photometric_grad_ref(x1, x2, lam, grad_mean)
            assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


def test_fp32_model_lies_inside_the_bounds():
    worst_v = worst_g = 0.0
    for shape in LU.SHAPES:
        x, y, _, _ = LU.inputs(shape)
        s4 = LU.shape4(shape)
        for weighting, kind, clamp, reduction in LU.pointwise_cases():
            ref = LU.pointwise_case(shape, weighting, kind, clamp, reduction)
            w = LU.weights_of(shape, weighting)
            w4 = None if w is None else w.reshape(s4) if w.dtype == torch.bool else w
            got = float(LU.model_value(x.reshape(s4), y.reshape(s4), w4, kind, clamp, reduction))
            assert LU.check_value(got, ref["value"], ref["bound_value"]), (shape, weighting, kind, clamp, reduction)
            if ref["bound_value"] > 0:
                worst_v = max(worst_v, abs(got - ref["value"]) / ref["bound_value"])
            grad = LU.model_grad(x.reshape(s4), y.reshape(s4), w4, kind, clamp, reduction).reshape(shape)
            r, over = SU.ratio(grad, ref["grad"], ref["bound_grad"])
            assert over == 0, (shape, weighting, kind, clamp, reduction, r)
            worst_g = max(worst_g, r)
    record_cpu("losses_fp32_model_over_bound", worst_value_ratio=worst_v, worst_gradient_ratio=worst_g)


def test_model_sum_is_a_sum_in_another_order():
    g = torch.Generator().manual_seed(6)
    for n in (1, 3, LU.WG_ELEMS, LU.WG_ELEMS + 1, LU.FIN_LANES * LU.WG_ELEMS + 5):
        t = torch.rand(n, generator=g)
        assert abs(float(LU.model_sum(t)) - float(t.double().sum())) <= LU.depth(n) * LU.U * float(t.double().sum())
    ints = torch.randint(0, 4, (3 * LU.WG_ELEMS + 7,), generator=g).float()   # small integers: every order is exact
    assert float(LU.model_sum(ints)) == float(ints.sum())
    assert LU.depth(1) == 18 and LU.depth((LU.FIN_LANES + 1) * LU.WG_ELEMS) == 19


def test_fp32_photometric_model_lies_inside_the_bounds():
    for scene in SU.SCENES:
        for shape in SU.SHAPES:
            for padding in SU.paddings_of(shape):
                ref = SU.reference(scene, shape, padding)
                for lam in LU.LAMBDAS:
                    case = LU.photometric_case(scene, shape, padding, lam)
                    loss, grad = LU.model_photometric(ref["img1"], ref["img2"], lam, padding)
                    assert abs(float(loss) - case["loss"]) <= case["bound_loss"], (scene, shape, padding, lam)
                    r, over = SU.ratio(grad, case["grad"], case["bound_grad"])
                    assert over == 0, (scene, shape, padding, lam, r)


def test_mutants_exceed_the_bounds():
    shape = (2, 3, 7, 5)
    x, y, _, mask = LU.inputs(shape)
    # 1. the clamp gate dropped: elements outside [0, 1] get a gradient
    ref = LU.pointwise_case(shape, "none", "l1", True, "mean")
    _, over = SU.ratio(LU.model_grad(x, y, None, "l1", True, "mean", gate=False), ref["grad"], ref["bound_grad"])
    assert over > 0
    # 2. sign(0) = +1 or -1
    ref = LU.pointwise_case(shape, "none", "l1", False, "mean")
    for s0 in (1.0, -1.0):
        _, over = SU.ratio(LU.model_grad(x, y, None, "l1", False, "mean", sign_at_zero=s0), ref["grad"], ref["bound_grad"])
        assert over > 0
    # 3. the mask form divided by numel
    ref = LU.pointwise_case(shape, "mask", "l1", False, "mean")
    got = float(LU.model_value(x, y, mask, "l1", False, "mean", mask_divisor_is_numel=True))
    assert abs(got - ref["value"]) > 10 * ref["bound_value"]
    _, over = SU.ratio(LU.model_grad(x, y, mask, "l1", False, "mean", mask_divisor_is_numel=True), ref["grad"], ref["bound_grad"])
    assert over > 0
    # 4. padding="valid" averaged over n instead of the cropped count
    pshape = (1, 3, SU.TILE_H + 1, 2 * SU.TILE_W + 5)
    pref = SU.reference("rand", pshape, "valid")
    case = LU.photometric_case("rand", pshape, "valid", 0.2)
    loss, grad = LU.model_photometric(pref["img1"], pref["img2"], 0.2, "valid", n_s_is_n=True)
    assert abs(float(loss) - case["loss"]) > 10 * case["bound_loss"]
    worst, over = SU.ratio(grad, case["grad"], case["bound_grad"])
    assert over > 0 and worst > 10.0
    # 5. a term dropped from the sum
    t = LU.terms(x, y)
    ref = LU.pointwise_case(shape, "none", "l1", False, "sum")
    assert abs(float(LU.model_sum(t.reshape(-1)[1:])) - ref["value"]) > 10 * ref["bound_value"]


def test_loose_share_of_the_combined_photometric_bound():
    """the condition test_ssim_host.py establishes for `sparse` and `render_like`, for the photometric gradient's bound
    against the photometric gradient, on the float64 reference alone"""
    shares = {}
    for scene in SU.SCENES:
        for shape in SU.SHAPES:
            for padding in SU.paddings_of(shape):
                for lam in LU.LAMBDAS:
                    case = LU.photometric_case(scene, shape, padding, lam)
                    share = SU.loose_share(case["bound_grad"], case["grad"])
                    shares[scene] = max(shares.get(scene, 0.0), share)
                    if scene in SU.CAPPED_SCENES:
                        assert share <= SU.LOOSE_SHARE_MAX, (scene, shape, padding, lam, share)
    record_cpu("losses_photometric_loose_share", largest_share_per_scene=shares)


def test_exports():
    import edgegaussians_amd
    from edgegaussians_amd import losses
    assert "losses" in edgegaussians_amd.__all__ and edgegaussians_amd.losses is losses
    for name in ("image_loss", "l1_loss", "mse_loss", "weighted_l1_loss", "masked_l1_loss", "projection_loss",
                 "photometric_loss"):
        assert callable(getattr(losses, name)), name
    assert (losses.WG_ELEMS, losses.FIN_LANES) == (1024, 64)
    src = open(os.path.join(os.path.dirname(losses.__file__), "csrc", "losses.hip")).read()
    assert "constexpr int kThreads = 256;" in src and "constexpr int kQuad = 4;" in src and "constexpr int kFinLanes = 64;" in src


def test_refusals_on_cpu_tensors_in_the_stated_order():
    from edgegaussians_amd import losses as L
    a, b = torch.rand(2, 3, 4, 5), torch.rand(2, 3, 4, 5)
    w, m = torch.rand(4, 5), torch.rand(2, 3, 4, 5) > 0.5
    five = torch.rand(1, 2, 3, 4, 5)
    # every later fault is present too: the earlier one is the one reported
    with pytest.raises(ValueError, match="reduction"):
        L.image_loss(five, b.double(), reduction="max", kind="l3")
    with pytest.raises(ValueError, match="kind"):
        L.image_loss(five, b.double(), kind="l3")
    with pytest.raises(ValueError, match="1 to 4 dimensions"):
        L.image_loss(five, torch.rand(7).double())
    with pytest.raises(ValueError, match="1 to 4 dimensions"):
        L.l1_loss(torch.tensor(1.0), torch.tensor(1.0))
    with pytest.raises(ValueError, match="not broadcastable"):
        L.image_loss(a[:, :, :0], torch.rand(7).double())
    with pytest.raises(ValueError, match="not broadcastable"):
        L.l1_loss(a[:, :1], b)                      # target larger than input
    with pytest.raises(ValueError, match="not broadcastable"):
        L.weighted_l1_loss(a, b, torch.rand(3, 5))
    with pytest.raises(ValueError, match="empty"):
        L.l1_loss(a[:, :, :0].double(), b[:, :, :0])
    with pytest.raises(TypeError, match="float32"):
        L.l1_loss(a.double(), b.clone().requires_grad_(True))
    with pytest.raises(TypeError, match="float32"):
        L.mse_loss(a, b.half())
    with pytest.raises(TypeError, match="weights must be torch.float32"):
        L.weighted_l1_loss(a, b, m)
    with pytest.raises(TypeError, match="weights must be torch.bool"):
        L.masked_l1_loss(a, b, w)
    with pytest.raises(TypeError, match="weights must be torch.float32"):
        L.projection_loss(a, b, m)
    with pytest.raises(TypeError, match="torch.float32 or torch.bool"):
        L.image_loss(a, b, w.double())
    with pytest.raises(ValueError, match="target must not require grad"):
        L.l1_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="weights must not require grad"):
        L.weighted_l1_loss(a, b, w.clone().requires_grad_(True))
    for fn, args in ((L.l1_loss, (a, b)), (L.mse_loss, (a, b)), (L.weighted_l1_loss, (a, b, w)),
                     (L.masked_l1_loss, (a, b, m)), (L.projection_loss, (a[0, 0], b[0, 0], w)), (L.image_loss, (a, b, m))):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(*args)
    # photometric_loss: the checks of fused_ssim
    p, q = torch.rand(1, 3, 12, 12), torch.rand(1, 3, 12, 12)
    with pytest.raises(ValueError, match="padding"):
        L.photometric_loss(p[0], q.double(), padding="reflect")
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        L.photometric_loss(p[0], q[0])
    with pytest.raises(ValueError, match="one shape"):
        L.photometric_loss(p, q[:, :2])
    with pytest.raises(ValueError, match="empty"):
        L.photometric_loss(p[:, :0], q[:, :0])
    with pytest.raises(ValueError, match="H, W >= 11"):
        L.photometric_loss(p[..., :10], q[..., :10], padding="valid")
    with pytest.raises(TypeError, match="float32"):
        L.photometric_loss(p.double(), q.double())
    with pytest.raises(ValueError, match="symmetric.*first"):
        L.photometric_loss(p, q.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="no CPU path"):
        L.photometric_loss(p, q, 0.2, "valid", True)


def test_c_abi_argument_validation_without_launching():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    h = _lib.load(require_device=False)
    st = (ctypes.c_int64 * 4)(36, 12, 4, 1)
    neg = (ctypes.c_int64 * 4)(36, 12, -4, 1)
    zero = (ctypes.c_int64 * 4)(36, 12, 0, 1)
    p = 4096  # never dereferenced: every call below is refused before any HIP call

    def swap(args, i, value):
        return args[:i] + (value,) + args[i + 1:]

    def refused(name, args):
        assert getattr(h, name)(*args) == -1, (name, args)
        assert name.encode() in h.eg_last_error_string()

    # eg_loss_fwd(x, y, w, w_kind, B, C, H, W, sx, sy, sw, q, clamp, reduction, slab, slab_words, out, stream)
    ok_f = (p, p, p, 1, 1, 3, 3, 4, st, st, st, 1, 0, 1, p, 1, p, None)
    # eg_loss_bwd(x, y, w, w_kind, B, C, H, W, sx, sy, sw, q, clamp, v, fwd_out, g, sg, stream)
    ok_b = (p, p, p, 1, 1, 3, 3, 4, st, st, st, 1, 0, p, p, p, st, None)
    for name, ok in (("eg_loss_fwd", ok_f), ("eg_loss_bwd", ok_b)):
        bad = [swap(ok, 0, None), swap(ok, 1, None), swap(ok, 2, None), swap(ok, 3, 3), swap(ok, 3, 0),  # w with w_kind 0
               swap(swap(ok, 2, None), 3, 2), swap(ok, 4, 0), swap(ok, 5, 0), swap(ok, 6, 0), swap(ok, 7, -1),
               swap(swap(swap(ok, 4, 1 << 11), 5, 1 << 10), 6, 1 << 10),   # 2^31 elements
               swap(ok, 8, None), swap(ok, 9, None), swap(ok, 10, None), swap(ok, 8, neg), swap(ok, 9, neg),
               swap(ok, 10, neg), swap(ok, 11, 0), swap(ok, 11, 3)]
        for args in bad:
            refused(name, args)
    for args in (swap(ok_f, 13, 3), swap(ok_f, 13, 2),      # the mask mean needs a mask
                 swap(ok_f, 14, None), swap(ok_f, 16, None), swap(ok_f, 15, 0),
                 swap(swap(ok_f, 3, 2), 15, 1)):              # a mask needs two words per workgroup
        refused("eg_loss_fwd", args)
    for args in (swap(ok_b, 13, None), swap(ok_b, 14, None), swap(ok_b, 15, None), swap(ok_b, 16, None),
                 swap(ok_b, 16, neg), swap(ok_b, 16, zero)):
        refused("eg_loss_bwd", args)
    # eg_photometric_fwd(img1, img2, B, C, H, W, s1, s2, valid, lambda, d_m1, d_s1, d_s12, slab, slab_len, out, stream)
    ok_pf = (p, p, 1, 3, 12, 40, st, st, 0, 0.2, p, p, p, p, 12, p, None)
    # eg_photometric_bwd(img1, img2, B, C, H, W, s1, s2, valid, lambda, v, d_m1, d_s1, d_s12, v_img1, stream)
    ok_pb = (p, p, 1, 3, 12, 40, st, st, 0, 0.2, p, p, p, p, p, None)
    for name, ok in (("eg_photometric_fwd", ok_pf), ("eg_photometric_bwd", ok_pb)):
        bad = [swap(ok, 0, None), swap(ok, 1, None), swap(ok, 6, None), swap(ok, 7, None), swap(ok, 2, 0), swap(ok, 3, 0),
               swap(ok, 4, 0), swap(ok, 5, -1), swap(ok, 6, neg), swap(ok, 7, neg), swap(swap(ok, 2, 256), 3, 256),
               swap(ok, 4, 65535 * 32 + 1), swap(ok, 5, (1 << 24) + 1),
               swap(swap(ok, 8, 1), 4, 10)]                  # valid below 11
        for args in bad:
            refused(name, args)
    for args in (swap(ok_pf, 10, None), swap(swap(ok_pf, 10, None), 11, None), swap(ok_pf, 13, None),
                 swap(ok_pf, 15, None), swap(ok_pf, 14, 11)):   # 1 x 2 tiles x 3 planes x 2 floats = 12
        refused("eg_photometric_fwd", args)
    for i in (10, 11, 12, 13, 14):
        refused("eg_photometric_bwd", swap(ok_pb, i, None))
