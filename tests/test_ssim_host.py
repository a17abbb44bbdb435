"""Fused SSIM without a device: the float64 reference against independent formulations, the closed-form backward
against autograd, the error bound (tests/ssim_util.py) on the fp32 CPU model and on mutants, the window constants of
csrc/ssim.hip, the exports, the refusals and the C ABI's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ssim_util as SU
from tests.util import record_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand64(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("shape", [(2, 3, 7, 5), (1, 2, 12, 23)])
def test_separable_blur_is_the_2d_window_on_the_padded_image(shape):
    x, _ = _rand64(shape, 1)
    g = SU.window()
    B, C, H, W = shape
    padded = F.pad(x.reshape(B * C, 1, H, W), (SU.RADIUS,) * 4)
    want = F.conv2d(padded, torch.outer(g, g).view(1, 1, 11, 11)).reshape(shape)
    assert float((SU.blur(x) - want).abs().max()) <= 1e-15
    assert abs(float(g.sum()) - 1.0) <= 1e-15 and torch.equal(g, g.flip(0))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 7, 5), (1, 1, 11, 11), (1, 2, 12, 23), (1, 3, 33, 70)])
def test_closed_form_backward_is_autograd_of_the_forward(shape):
    x1, x2 = _rand64(shape, 2)
    v = torch.randn(shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    want = SU.ssim_grad_autograd(x1, x2, v)
    got = SU.ssim_grad_closed(x1, x2, v)
    assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max()))


def test_valid_is_the_cropped_map_and_the_unpadded_convolution():
    shape = (1, 2, 12, 23)
    x1, x2 = _rand64(shape, 4)
    same, valid = SU.ssim_map_ref(x1, x2, "same"), SU.ssim_map_ref(x1, x2, "valid")
    assert valid.shape == (1, 2, 2, 13) and torch.equal(valid, same[:, :, 5:-5, 5:-5])
    g2 = torch.outer(SU.window(), SU.window()).view(1, 1, 11, 11)

    def unpadded(x):
        return F.conv2d(x.reshape(2, 1, 12, 23), g2).reshape(1, 2, 2, 13)

    want = SU.pointwise(*SU.moments(x1, x2, unpadded))
    assert float((valid - want).abs().max()) <= 1e-14
    # ... and its backward is the backward of the full map on v zero-padded back
    v = torch.randn(valid.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    assert float((SU.ssim_grad_autograd(x1, x2, v, "valid") - SU.ssim_grad_closed(x1, x2, v, "valid")).abs().max()) <= 1e-13


def test_window_constants_of_the_kernel_source():
    src = open(os.path.join(ROOT, "edgegaussians_amd", "csrc", "ssim.hip")).read()
    m = re.search(r"#define\s+EG_SSIM_WINDOW\s+(.*)", src)
    assert m, "EG_SSIM_WINDOW not found"
    vals = [np.float32(float(t.strip().rstrip("f"))) for t in m.group(1).split(",")]
    want = SU.window().numpy().astype(np.float32)
    assert len(vals) == 11 and all(a == b for a, b in zip(vals, want)), (vals, want)
    tiles = re.search(r"constexpr int kTW = (\d+), kTH = (\d+);", src)
    assert (int(tiles.group(2)), int(tiles.group(1))) == (SU.TILE_H, SU.TILE_W)
    consts = re.search(r"kC1 = ([0-9.e-]+)f, kC2 = ([0-9.e-]+)f;", src)
    assert np.float32(float(consts.group(1))) == np.float32(SU.C1) and np.float32(float(consts.group(2))) == np.float32(SU.C2)


CASES = [(sc, sh, p) for sc in SU.SCENES for sh in SU.SHAPES for p in SU.paddings_of(sh)]


def test_fp32_model_lies_inside_the_bound():
    assert SU.K_ROUNDINGS <= 32
    worst = {}
    for scene, shape, padding in CASES:
        ref = SU.reference(scene, shape, padding)
        S, g = SU.model_f32(ref["img1"], ref["img2"], ref["v"], padding)
        rs, over_s = SU.ratio(S, ref["S"], ref["bound_S"])
        rg, over_g = SU.ratio(g, ref["grad"], ref["bound_g"])
        assert over_s == 0 and over_g == 0, (scene, shape, padding, rs, rg)
        w = worst.setdefault(scene, [0.0, 0.0])
        w[0], w[1] = max(w[0], rs), max(w[1], rg)
    record_cpu("ssim_fp32_model_over_bound", K=SU.K_ROUNDINGS, worst_map_and_grad_ratio_per_scene=worst)


def test_loose_share_of_the_bound():
    """on `sparse` and `render_like` at most 3 % of the pixels have a bound above 1e-4 max|reference|; `flat` and `rand`
    carry no cap, their shares are recorded"""
    shares = {}
    for scene, shape, padding in CASES:
        ref = SU.reference(scene, shape, padding)
        ls, lg = SU.loose_share(ref["bound_S"], ref["S"]), SU.loose_share(ref["bound_g"], ref["grad"])
        w = shares.setdefault(scene, [0.0, 0.0])
        w[0], w[1] = max(w[0], ls), max(w[1], lg)
        if scene in SU.CAPPED_SCENES:
            assert ls <= SU.LOOSE_SHARE_MAX and lg <= SU.LOOSE_SHARE_MAX, (scene, shape, padding, ls, lg)
    record_cpu("ssim_loose_share", K=SU.K_ROUNDINGS, largest_map_and_grad_share_per_scene=shares)


def _shifted_window():
    g = SU.window()
    return torch.cat([torch.zeros(1, dtype=g.dtype), g[:-1]])


MUTANTS = {
    "sigma_1.4": dict(blur_fn=lambda x: SU.blur(x, SU.window(1.4))),
    "c2_times_1.01": dict(c2=SU.C2 * 1.01),
    "window_shifted_by_one_tap": dict(blur_fn=lambda x: SU.blur(x, _shifted_window())),
    "replicate_padding": dict(blur_fn=lambda x: SU.blur(x, pad_mode="replicate")),
}


@pytest.mark.parametrize("scene", ["rand", "sparse", "render_like"])
@pytest.mark.parametrize("mutant", list(MUTANTS) + ["dropped_chain_term"])
def test_mutants_exceed_the_bound(mutant, scene):
    shape = (1, 3, SU.TILE_H + 1, 2 * SU.TILE_W + 5)
    ref = SU.reference(scene, shape, "same")
    x1, x2 = ref["img1"].double(), ref["img2"].double()
    if mutant == "dropped_chain_term":
        got, want, bound = SU.ssim_grad_closed(x1, x2, ref["v"].double(), drop_chain_term=True), ref["grad"], ref["bound_g"]
    else:
        got, want, bound = SU.ssim_map_ref(x1, x2, **MUTANTS[mutant]), ref["S"], ref["bound_S"]
    worst, over = SU.ratio(got, want, bound)
    assert over > 0 and worst > 10.0, (mutant, scene, worst)


def test_exports():
    import edgegaussians_amd
    import fused_ssim
    from edgegaussians_amd import ssim
    assert "ssim" in edgegaussians_amd.__all__ and edgegaussians_amd.ssim is ssim
    assert fused_ssim.fused_ssim is ssim.fused_ssim and fused_ssim.__all__ == ["fused_ssim"]
    assert callable(ssim.ssim_map) and (ssim.TILE_H, ssim.TILE_W) == (SU.TILE_H, SU.TILE_W)


def test_refusals_on_cpu_tensors():
    from edgegaussians_amd.ssim import fused_ssim, ssim_map
    a, b = torch.rand(1, 3, 12, 12), torch.rand(1, 3, 12, 12)
    for fn in (ssim_map, fused_ssim):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(a, b)
        with pytest.raises(TypeError, match="float32"):
            fn(a.double(), b.double())
        with pytest.raises(TypeError, match="float32"):
            fn(a, b.half())
        with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
            fn(a[0], b[0])
        with pytest.raises(ValueError, match="one shape"):
            fn(a, b[:, :2])
        with pytest.raises(ValueError, match="empty"):
            fn(a[:, :0], b[:, :0])
        with pytest.raises(ValueError, match="padding"):
            fn(a, b, padding="reflect")
        with pytest.raises(ValueError, match="H, W >= 11"):
            fn(a[..., :10], b[..., :10], padding="valid")
        with pytest.raises(ValueError, match="H, W >= 11"):
            fn(a[:, :, :10], b[:, :, :10], padding="valid")
        with pytest.raises(ValueError, match="symmetric.*first"):
            fn(a, b.clone().requires_grad_(True))


def test_c_abi_argument_validation_without_launching():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    h = _lib.load(require_device=False)
    st = (ctypes.c_int64 * 4)(36, 12, 4, 1)
    neg = (ctypes.c_int64 * 4)(36, 12, -4, 1)
    p = 4096  # never dereferenced: every call below is refused before any HIP call
    ok_f = (p, p, 1, 3, 3, 4, st, st, p, p, p, p, None)
    ok_b = (p, p, 1, 3, 3, 4, st, st, p, p, p, p, p, None)

    def swap(args, i, value):
        return args[:i] + (value,) + args[i + 1:]

    for name, ok in (("eg_ssim_fwd", ok_f), ("eg_ssim_bwd", ok_b)):
        fn = getattr(h, name)
        bad = [swap(ok, 0, None), swap(ok, 1, None), swap(ok, 6, None), swap(ok, 7, None), swap(ok, 8, None),
               swap(ok, 2, 0), swap(ok, 3, 0), swap(ok, 4, 0), swap(ok, 5, -1), swap(ok, 6, neg), swap(ok, 7, neg),
               swap(swap(ok, 2, 256), 3, 256),          # 65536 planes
               swap(ok, 4, 65535 * 32 + 1), swap(ok, 5, (1 << 24) + 1)]
        if name == "eg_ssim_fwd":
            bad += [swap(ok, 9, None), swap(swap(ok, 9, None), 10, None)]   # derivative maps: all three or none
        else:
            bad += [swap(ok, i, None) for i in (9, 10, 11, 12)]
        for args in bad:
            assert fn(*args) == -1, (name, args)
            assert name.encode() in h.eg_last_error_string()
