"""What the SSIM tests share (tests/test_ssim_host.py, tests/test_gpu_ssim.py): the float64 reference of
edgegaussians_amd/ssim.py's semantics, an fp32 CPU model of the same formulas (the torch conv formulation), the scenes,
and the per-pixel first-order error bound that is the tolerance everywhere.

The bound.  A fixed rtol cannot serve: in fp32, e11 - m1^2 cancels against C2 = 9e-4, so the honest error of a flat
image is 1e-3 of the map while that of a random one is 1e-6.  Each moment q of {m1, m2, e11, e22, e12} may be off by
e_q = K u G*|.| (u = 2^-24, G*|.| the blur of the absolute values of what q blurs); to first order the map is then off by
bound_S = sum_q |dS/dq| e_q + K u |S|, each derivative map d_x of {d_m1, d_s1, d_s12} by delta_x built the same way, and
the gradient by
    bound_g = G*(|v| delta_m1) + 2 |img1| G*(|v| delta_s1) + |img2| G*(|v| delta_s12)
              + K u (G*|v d_m1| + 2 |img1| G*|v d_s1| + |img2| G*|v d_s12|).
The partials come from autograd on the pointwise function of the five moments, in float64.

K = 25: the roundings behind one moment in csrc/ssim.hip -- 11 in the fmaf chain of the horizontal pass (the first fmaf
onto 0 rounds once, like a product), 11 in the vertical one, one per pass for the fp32 window constant, one for the
product under the blur (img1^2, img2^2, img1 img2).  Every one of them is relative to a partial sum of non-negative
weights times |.|, hence bounded by u G*|.|."""
import functools

import torch
import torch.nn.functional as F

from edgegaussians_amd.ssim import RADIUS, TILE_H, TILE_W

K_ROUNDINGS = 25
U_ROUND = 2.0 ** -24
C1, C2 = 0.01 ** 2, 0.03 ** 2
LOOSE = 1e-4            # a pixel whose bound exceeds LOOSE * max|reference| counts as loose
LOOSE_SHARE_MAX = 0.03  # ... and on `sparse` and `render_like` at most this share of the pixels may be

SCENES = ("rand", "sparse", "render_like", "flat", "zeros_vs_rand")
CAPPED_SCENES = ("sparse", "render_like")
SHAPES = ((1, 1, 1, 1), (2, 3, 7, 5), (1, 2, 11, 11), (1, 4, 6, TILE_W + 1), (2, 3, TILE_H - 1, TILE_W),
          (1, 3, TILE_H + 1, 2 * TILE_W + 5), (2, 1, 2 * TILE_H + 5, TILE_W - 1))
LAYOUTS = ("nchw", "channels_last")


def window(sigma=1.5, dtype=torch.float64):
    k = torch.arange(2 * RADIUS + 1, dtype=torch.float64)
    g = torch.exp(-(k - RADIUS) ** 2 / (2.0 * sigma ** 2))
    return (g / g.sum()).to(dtype)


def blur(x, g=None, pad_mode="zeros"):
    """G*x: g along W, then g along H, per plane of x [B, C, H, W]; zero padding of RADIUS (or replicate: a mutant)"""
    g = window(dtype=x.dtype) if g is None else g.to(x.dtype)
    B, C, H, W = x.shape
    y = x.reshape(B * C, 1, H, W)
    if pad_mode == "replicate":
        y = F.pad(y, (RADIUS,) * 4, mode="replicate")
        y = F.conv2d(F.conv2d(y, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1))
    else:
        y = F.conv2d(y, g.view(1, 1, 1, -1), padding=(0, RADIUS))
        y = F.conv2d(y, g.view(1, 1, -1, 1), padding=(RADIUS, 0))
    return y.reshape(B, C, H, W)


def moments(x1, x2, blur_fn=blur):
    return blur_fn(x1), blur_fn(x2), blur_fn(x1 * x1), blur_fn(x2 * x2), blur_fn(x1 * x2)


def pointwise(m1, m2, e11, e22, e12, c2=C2):
    """S of the five moments"""
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    A1, A2 = 2 * m1 * m2 + C1, 2 * s12 + c2
    B1, B2 = m1 * m1 + m2 * m2 + C1, s1 + s2 + c2
    return A1 * A2 / (B1 * B2)


def derivative_maps(m1, m2, e11, e22, e12, drop_chain_term=False):
    """the closed form: (d_m1, d_s1, d_s12) of the five moments"""
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    A1, A2 = 2 * m1 * m2 + C1, 2 * s12 + C2
    B1, B2 = m1 * m1 + m2 * m2 + C1, s1 + s2 + C2
    d_s1 = -A1 * A2 / (B1 * B2 * B2)
    d_s12 = 2 * A1 / (B1 * B2)
    d_m1 = 2 * m2 * A2 / (B1 * B2) - 2 * m1 * A1 * A2 / (B1 * B1 * B2) - m2 * d_s12
    if not drop_chain_term:
        d_m1 = d_m1 - 2 * m1 * d_s1
    return d_m1, d_s1, d_s12


def crop(x):
    return x[:, :, RADIUS:-RADIUS, RADIUS:-RADIUS]


def pad_back(v):
    return F.pad(v, (RADIUS,) * 4)


def ssim_map_ref(img1, img2, padding="same", blur_fn=blur, c2=C2):
    """the map, in the dtype of the inputs (float64: the reference; float32: the CPU model)"""
    S = pointwise(*moments(img1, img2, blur_fn), c2=c2)
    return S if padding == "same" else crop(S)


def ssim_grad_autograd(img1, img2, v, padding="same"):
    """v_img1 by autograd of the forward, in the dtype of the inputs; v has the map's shape"""
    x = img1.detach().clone().requires_grad_(True)
    return torch.autograd.grad(ssim_map_ref(x, img2, padding), x, v)[0]


def ssim_grad_closed(img1, img2, v, padding="same", drop_chain_term=False, blur_fn=blur):
    """v_img1 by the closed form of the module docstring"""
    if padding == "valid":
        v = pad_back(v)
    d_m1, d_s1, d_s12 = derivative_maps(*moments(img1, img2, blur_fn), drop_chain_term=drop_chain_term)
    return blur_fn(v * d_m1) + 2 * img1 * blur_fn(v * d_s1) + img2 * blur_fn(v * d_s12)


def bounds(img1, img2, v, padding="same", K=K_ROUNDINGS):
    """(bound_S in the map's shape, bound_g [B, C, H, W]) in float64; v has the map's shape"""
    x1, x2 = img1.double(), img2.double()
    v = v.double()
    if padding == "valid":
        v = pad_back(v)
    ku = K * U_ROUND
    e = [ku * blur(t) for t in (x1.abs(), x2.abs(), x1 * x1, x2 * x2, (x1 * x2).abs())]
    mom = [m.detach().clone().requires_grad_(True) for m in moments(x1, x2)]
    outs = (pointwise(*mom),) + derivative_maps(*mom)
    deltas = []
    for out in outs:
        parts = torch.autograd.grad(out.sum(), mom, retain_graph=True, allow_unused=True)
        d = ku * out.detach().abs()
        for p, eq in zip(parts, e):
            if p is not None:
                d = d + p.abs() * eq
        deltas.append(d)
    bound_S, dm1, ds1, ds12 = deltas
    d_m1, d_s1, d_s12 = (o.detach() for o in outs[1:])
    av = v.abs()
    bound_g = (blur(av * dm1) + 2 * x1.abs() * blur(av * ds1) + x2.abs() * blur(av * ds12)
               + ku * (blur((v * d_m1).abs()) + 2 * x1.abs() * blur((v * d_s1).abs()) + x2.abs() * blur((v * d_s12).abs())))
    return (bound_S if padding == "same" else crop(bound_S)), bound_g


def make_scene(scene, shape, seed=0):
    """(img1, img2) fp32 CPU, contiguous NCHW"""
    g = torch.Generator().manual_seed(1000 * SCENES.index(scene) + 17 * sum(shape) + seed)
    u1, u2 = torch.rand(shape, generator=g, dtype=torch.float64), torch.rand(shape, generator=g, dtype=torch.float64)
    if scene == "rand":
        a, b = u1, u2
    elif scene == "sparse":
        a, b = (u1 > 0.9).double(), (u2 > 0.9).double()
    elif scene == "render_like":
        a, b = u1 ** 6, u2 ** 6
    elif scene == "flat":
        a = 0.9 + 1e-3 * torch.randn(shape, generator=g, dtype=torch.float64)
        b = 0.9 + 1e-3 * torch.randn(shape, generator=g, dtype=torch.float64)
    elif scene == "zeros_vs_rand":
        a, b = torch.zeros(shape, dtype=torch.float64), u2
    else:
        raise KeyError(scene)
    return a.float().contiguous(), b.float().contiguous()


def map_shape(shape, padding):
    B, C, H, W = shape
    return shape if padding == "same" else (B, C, H - 2 * RADIUS, W - 2 * RADIUS)


def paddings_of(shape):
    return ("same", "valid") if min(shape[2], shape[3]) >= 2 * RADIUS + 1 else ("same",)


@functools.lru_cache(maxsize=None)
def reference(scene, shape, padding="same"):
    """Everything the comparisons of one case need, computed once and never modified: the fp32 inputs, the random
    cotangent v and the cotangent of the mean (1 / numel), the float64 map, the float64 gradients by autograd for both,
    and the bounds."""
    img1, img2 = make_scene(scene, shape)
    ms = map_shape(shape, padding)
    g = torch.Generator().manual_seed(7 + sum(shape))
    v = torch.randn(ms, generator=g).float()
    v_mean = torch.full(ms, 1.0 / torch.Size(ms).numel(), dtype=torch.float32)
    x1, x2 = img1.double(), img2.double()
    S = ssim_map_ref(x1, x2, padding)
    bound_S, bound_g = bounds(img1, img2, v, padding)
    _, bound_g_mean = bounds(img1, img2, v_mean, padding)
    return dict(img1=img1, img2=img2, v=v, v_mean=v_mean, S=S, grad=ssim_grad_autograd(x1, x2, v.double(), padding),
                grad_mean=ssim_grad_autograd(x1, x2, v_mean.double(), padding), bound_S=bound_S, bound_g=bound_g,
                bound_g_mean=bound_g_mean)


def ratio(got, ref, bound):
    """(largest |got - ref| / bound over the elements with a positive bound, number of elements over their bound --
    an element whose bound is zero must be exact)"""
    err = (got.double() - ref).abs()
    over = int((err > bound).sum())
    pos = bound > 0
    return (float((err[pos] / bound[pos]).max()) if pos.any() else 0.0), over


def loose_share(bound, ref):
    mx = float(ref.abs().max())
    return float((bound > LOOSE * mx).double().mean())


def model_f32(img1, img2, v, padding="same"):
    """the fp32 CPU model: (map, gradient by fp32 autograd)"""
    x = img1.detach().clone().requires_grad_(True)
    S = ssim_map_ref(x, img2, padding)
    return S.detach(), torch.autograd.grad(S, x, v)[0]


def as_layout(t, layout):
    """t [B, C, H, W] contiguous -> the same values as NCHW-contiguous or as the permute(0, 3, 1, 2) view of a
    contiguous [B, H, W, C] (what rasterization's render gives)"""
    if layout == "nchw":
        return t.contiguous()
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
