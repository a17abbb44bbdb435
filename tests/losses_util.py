"""What the loss tests share (tests/test_losses_host.py, tests/test_gpu_losses.py): the float64 statements of
edgegaussians_amd/losses.py's functions, an fp32 CPU model of the kernels' arithmetic and summation order, the cases,
and the first-order rounding bounds that are the tolerance everywhere.  Scenes, shapes, layouts and the SSIM references
come from tests/ssim_util.py.

The sum bound.  csrc/losses.hip adds the terms t_p = w_p |c(x_p) - y_p|^q in a fixed tree: a lane adds its QUAD = 4
terms in index order (3 additions; the first onto 0 is exact), the wave's DPP tree has 6 levels, the THREADS / 64 = 4
waves of a workgroup are added in order (3), the finalize wave's lane l adds the partials l, l + 64, .. of the G =
ceil(n / WG_ELEMS) workgroups in order (ceil(G / 64) - 1) and one more DPP tree follows (6):
    depth(n) = 3 + 6 + 3 + (ceil(G / 64) - 1) + 6.
Every addition rounds a partial sum whose size is at most the sum of the |t_p| under it, so a term passes through at
most depth(n) roundings of relative size u = 2^-24.  A term itself carries c = 3 roundings (the difference, the square
with q = 2, the weight), the division by D one more, and the conversion of D (numel or the count) to fp32 one:
    |value - ref| <= (depth(n) + c + 2) u sum_p |t_p| / D.
The count of the mask form is an integer sum: exact.

A gradient element is a product of rounded factors -- v / D (the conversion of D and the division: 2), the weight (1),
2 d (the difference: 1) and the final product (1): |g_p - ref_p| <= GRAD_ROUNDINGS u |ref_p| with GRAD_ROUNDINGS = 5,
and exactly 0 where the statement has a zero (mask false, weight 0, x = y, shut clamp gate).  The sign of d is exact:
fp32 subtraction of distinct numbers never gives 0.

The photometric loss (csrc/ssim.hip).  A workgroup adds the S of its pixels (a lane's kRows = 8 in row order: 7; DPP: 6;
waves: 3) and the |x1 - x2| of its TILE_H x TILE_W tile (a lane's 4: 3; 6; 3); the finalize wave adds the G partials
(ceil(G / 64) - 1, then 6).  S itself is inside ssim_util's bound_S.  With the two divisions, the conversions of n and
n_S and the five operations of (1 - lambda) l1 + lambda (1 - s):
    |value - ref| <= (1 - lambda) (depth_l1 + 3) u mean|x1 - x2|
                     + lambda (mean(bound_S) + (depth_s + 2) u mean|S|) + 5 u ((1 - lambda) l1 + lambda (1 + |s|)).
Its gradient is (1 - lambda) / n sign(x1 - x2) - lambda grad(mean S): the second part inside lambda times ssim_util's
bound for the cotangent 1 / n_S (`bound_g_mean`: ssim_util.bounds scaled by 1 / n_S), the scales (1 - lambda) (v / n),
lambda (v / n_S) and the final difference 4 roundings of the parts' sizes:
    |g - ref| <= lambda bound_g_mean + 4 u ((1 - lambda) / n |sign| + lambda |grad_mean|)."""
import functools
import math

import torch

from edgegaussians_amd.losses import FIN_LANES, WG_ELEMS
from tests import ssim_util as SU

U = SU.U_ROUND
QUAD, WAVE = 4, 64
THREADS = WG_ELEMS // QUAD
TERM_ROUNDINGS = 3
GRAD_ROUNDINGS = 5

KINDS = ("l1", "l2")
REDUCTIONS = ("mean", "sum")
WEIGHTINGS = ("none", "weights", "mask")
# the smallest shapes at which the kernels take another path: one lane, odd sizes (the element-wise path, quads that
# cross rows and planes), one element more than a workgroup covers, one workgroup more than the finalize wave has
# lanes (its lane 0 adds two partials), and W % 4 == 0 / W % 4 != 0 at the size of a small image
SHAPES = ((1,), (7, 5), (2, 3, 7, 5), (1, 1, 1, WG_ELEMS + 1), (1, 1, FIN_LANES + 1, WG_ELEMS), (1, 3, 64, 65))
LAMBDAS = (0.0, 0.2, 1.0)


def shape4(shape):
    return (1,) * (4 - len(shape)) + tuple(shape)


# ---------------------------------------------------------------- float64 statements

def residual(x, y, clamp):
    return (x.clamp(0.0, 1.0) if clamp else x) - y


def terms(x, y, w=None, kind="l1", clamp=False):
    """t_p, in the dtype of x (float64: the statement)"""
    t = residual(x, y, clamp).abs()
    t = t * t if kind == "l2" else t
    if w is None:
        return t
    return torch.where(w, t, torch.zeros_like(t)) if w.dtype == torch.bool else w * t


def divisor(x, w, reduction, mask_divisor_is_numel=False):
    if reduction == "sum":
        return 1.0
    if w is not None and w.dtype == torch.bool and not mask_divisor_is_numel:
        return float(w.expand(x.shape).sum())
    return float(x.numel())


def image_loss_ref(x, y, w=None, kind="l1", clamp=False, reduction="mean"):
    D = divisor(x, w, reduction)
    s = terms(x, y, w, kind, clamp).sum()
    return s / D if D != 0 else s * float("nan")


def image_grad_ref(x, y, w=None, kind="l1", clamp=False, reduction="mean", v=1.0, *, gate=True, sign_at_zero=0.0,
                   mask_divisor_is_numel=False):
    """the closed form of the module docstring of losses.py (the keyword switches are the mutants)"""
    d = residual(x, y, clamp)
    sgn = torch.where(d == 0, torch.full_like(d, sign_at_zero), torch.sign(d))
    coef = 2 * d.abs() * sgn if kind == "l2" else sgn
    if kind == "l2" and sign_at_zero != 0.0:
        coef = torch.where(d == 0, torch.full_like(d, sign_at_zero), coef)
    D = divisor(x, w, reduction, mask_divisor_is_numel)
    g = coef * (v / D if D != 0 else float("inf"))
    if w is not None:
        g = torch.where(w, g, torch.zeros_like(g)) if w.dtype == torch.bool else torch.where(w == 0, torch.zeros_like(g), w * g)
    if clamp and gate:
        g = torch.where((x >= 0) & (x <= 1), g, torch.zeros_like(g))
    return torch.where(coef == 0, torch.zeros_like(g), g)


def l1_loss_ref(x, y):
    return image_loss_ref(x, y)


def mse_loss_ref(x, y):
    return image_loss_ref(x, y, kind="l2")


def weighted_l1_loss_ref(x, y, w):
    return image_loss_ref(x, y, w)


def masked_l1_loss_ref(x, y, mask):
    return image_loss_ref(x, y, mask)


def projection_loss_ref(render, gt, wmap, clamp=True):
    return image_loss_ref(render, gt, wmap, clamp=clamp, reduction="sum")


def photometric_ref(x1, x2, lam, padding="same"):
    """(loss, l1 mean, ssim mean) in the dtype of the inputs"""
    l1, s = (x1 - x2).abs().mean(), SU.ssim_map_ref(x1, x2, padding).mean()
    return (1.0 - lam) * l1 + lam * (1.0 - s), l1, s


def photometric_grad_ref(x1, x2, lam, grad_mean_ssim):
    return (1.0 - lam) / x1.numel() * torch.sign(x1 - x2) - lam * grad_mean_ssim


# ---------------------------------------------------------------- the fp32 model of the kernels

def _wave_tree(v):
    """v [..., 64] fp32 -> [...]: the DPP tree of common.h's wave_sum_dpp_f (row_shr 1, 2, 4, 8 inside the rows of 16,
    row_bcast 15 into rows 1 and 3, row_bcast 31 into rows 2 and 3; lane 63)"""
    r = v.reshape(*v.shape[:-1], 4, 16).clone()
    for sh in (1, 2, 4, 8):
        shifted = torch.zeros_like(r)
        shifted[..., sh:] = r[..., :-sh]
        r = r + shifted
    rows = r[..., 15]
    return (rows[..., 3] + rows[..., 2]) + (rows[..., 1] + rows[..., 0])


def _slab_sum(slab):
    """slab [G] fp32 -> the finalize wave's sum"""
    G = slab.numel()
    padded = torch.zeros(-(-G // FIN_LANES) * FIN_LANES, dtype=torch.float32)
    padded[:G] = slab
    acc = torch.zeros(FIN_LANES, dtype=torch.float32)
    for row in padded.reshape(-1, FIN_LANES):
        acc = acc + row
    return _wave_tree(acc)


def model_sum(t):
    """the fp32 sum of the terms t (any shape, logical order) in the order of csrc/losses.hip"""
    t = t.reshape(-1).float()
    G = -(-t.numel() // WG_ELEMS)
    padded = torch.zeros(G * WG_ELEMS, dtype=torch.float32)
    padded[:t.numel()] = t
    q = padded.reshape(G, THREADS // WAVE, WAVE, QUAD)
    lane = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    waves = _wave_tree(lane)
    wg = waves[:, 0]
    for k in range(1, THREADS // WAVE):
        wg = wg + waves[:, k]
    return _slab_sum(wg)


def model_value(x, y, w=None, kind="l1", clamp=False, reduction="mean", **mutant):
    """the kernels' value in fp32 (x, y, w fp32 / bool)"""
    s = model_sum(terms(x, y, w, kind, clamp))
    return s / torch.tensor(divisor(x, w, reduction, **mutant), dtype=torch.float32)


def model_grad(x, y, w=None, kind="l1", clamp=False, reduction="mean", v=1.0, **mutant):
    """the kernels' gradient in fp32: the closed form on fp32 tensors"""
    return image_grad_ref(x, y, w, kind, clamp, reduction, torch.tensor(v, dtype=torch.float32), **mutant)


def model_photometric(x1, x2, lam, padding="same", n_s_is_n=False):
    """fp32 torch: (loss, gradient by fp32 autograd); n_s_is_n: the mutant that divides the cropped sum by n"""
    x = x1.detach().clone().requires_grad_(True)
    S = SU.ssim_map_ref(x, x2, padding)
    s = S.sum() / (x.numel() if n_s_is_n else S.numel())
    loss = (1.0 - lam) * (x - x2).abs().mean() + lam * (1.0 - s)
    return loss.detach(), torch.autograd.grad(loss, x)[0]


# ---------------------------------------------------------------- bounds

def depth(n):
    G = -(-n // WG_ELEMS)
    return (QUAD - 1) + 6 + (THREADS // WAVE - 1) + (-(-G // FIN_LANES) - 1) + 6


def sum_bound(t64, D):
    """bound of the value for the float64 terms t64 and the divisor D"""
    return (depth(t64.numel()) + TERM_ROUNDINGS + 2) * U * float(t64.abs().sum()) / D


def grad_bound(g64):
    return GRAD_ROUNDINGS * U * g64.abs()


def photometric_workgroups(shape):
    B, C, H, W = shape
    return -(-W // SU.TILE_W) * -(-H // SU.TILE_H) * B * C


def photometric_term_bounds(ref, l1):
    """(bound of the L1 mean, bound of the SSIM mean) for ref = ssim_util.reference(scene, shape, padding)"""
    tail = (-(-photometric_workgroups(tuple(ref["img1"].shape)) // FIN_LANES) - 1) + 6
    depth_l1 = (SU.TILE_H * SU.TILE_W // 256 - 1) + 6 + 3 + tail
    depth_s = (SU.TILE_H // (256 // SU.TILE_W) - 1) + 6 + 3 + tail  # (a lane's kRows = 8 values: 7)
    return ((depth_l1 + 3) * U * abs(l1),
            float(ref["bound_S"].mean()) + (depth_s + 2) * U * float(ref["S"].abs().mean()))


def photometric_value_bound(ref, lam, l1, s):
    """ref: ssim_util.reference(scene, shape, padding); l1, s: the float64 means"""
    b_l1, b_s = photometric_term_bounds(ref, l1)
    return (1.0 - lam) * b_l1 + lam * b_s + 5 * U * ((1.0 - lam) * abs(l1) + lam * (1.0 + abs(s)))


def photometric_grad_bound(ref, lam):
    x1, x2 = ref["img1"].double(), ref["img2"].double()
    return lam * ref["bound_g_mean"] + 4 * U * ((1.0 - lam) / x1.numel() * torch.sign(x1 - x2).abs()
                                                + lam * ref["grad_mean"].abs())


@functools.lru_cache(maxsize=None)
def photometric_case(scene, shape, padding, lam):
    """float64 reference of one photometric case, computed once and never modified"""
    ref = SU.reference(scene, shape, padding)
    x1, x2 = ref["img1"].double(), ref["img2"].double()
    loss, l1, s = (float(t) for t in photometric_ref(x1, x2, lam, padding))
    return dict(loss=loss, l1=l1, s=s, grad=photometric_grad_ref(x1, x2, lam, ref["grad_mean"]),
                bound_loss=photometric_value_bound(ref, lam, l1, s), bound_grad=photometric_grad_bound(ref, lam))


# ---------------------------------------------------------------- pointwise cases

@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(x, y, weights base [H, W, 1], mask) fp32 / bool CPU for a pointwise shape: x spills over [0, 1] and hits 0, 1
    and y exactly at a few elements each"""
    B, C, H, W = shape4(shape)
    g = torch.Generator().manual_seed(31 + 7 * sum(shape) + len(shape))
    x = (torch.rand((B, C, H, W), generator=g) * 1.5 - 0.25).float()
    y = torch.rand((B, C, H, W), generator=g).float()
    flat_x, flat_y = x.view(-1), y.view(-1)
    n = flat_x.numel()
    if n >= 8:
        flat_x[1::11] = flat_y[1::11]   # x == y
        flat_x[2::13] = 0.0
        flat_x[3::17] = 1.0
        flat_y[3::34] = 1.0              # x == y == 1 under the clamp
    wbase = torch.rand((H, W, 1), generator=g).float()
    wbase.view(-1)[::5] = 0.0            # zero weights
    mask = torch.rand((B, C, H, W), generator=g) > 0.6
    return x.reshape(shape), y.reshape(shape), wbase, mask.reshape(shape)


def weights_of(shape, weighting):
    """None, the fp32 weights [H, W, 1] expanded over the channels and the batch (logical [B, C, H, W], strides 0 on
    B and C), or the bool mask"""
    x, _, wbase, mask = inputs(shape)
    if weighting == "none":
        return None
    if weighting == "mask":
        return mask
    B, C, H, W = shape4(shape)
    return wbase.expand(H, W, C).permute(2, 0, 1).expand(B, C, H, W)


@functools.lru_cache(maxsize=None)
def pointwise_case(shape, weighting, kind, clamp, reduction):
    """float64 reference of one pointwise case (v = 1), computed once and never modified"""
    x, y, _, _ = inputs(shape)
    w = weights_of(shape, weighting)
    s4 = shape4(shape)
    x64, y64 = x.double().reshape(s4), y.double().reshape(s4)
    w64 = None if w is None else (w.reshape(s4) if w.dtype == torch.bool else w.double())
    t = terms(x64, y64, w64, kind, clamp)
    D = divisor(x64, w64, reduction)
    grad = image_grad_ref(x64, y64, w64, kind, clamp, reduction)
    return dict(value=float(image_loss_ref(x64, y64, w64, kind, clamp, reduction)), bound_value=sum_bound(t, D) if D else 0.0,
                grad=grad.reshape(shape), bound_grad=grad_bound(grad).reshape(shape), D=D)


def pointwise_cases():
    for weighting in WEIGHTINGS:
        for kind in KINDS:
            for clamp in (False, True):
                for reduction in REDUCTIONS:
                    yield weighting, kind, clamp, reduction


def check_value(got, want, bound):
    """|got - want| <= bound, nan matching nan"""
    if math.isnan(want):
        return math.isnan(got)
    return abs(got - want) <= bound
