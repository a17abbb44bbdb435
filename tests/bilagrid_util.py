"""What the bilateral-grid tests share (tests/test_bilagrid_host.py, tests/test_gpu_bilagrid.py): the float64
statements of edgegaussians_amd/bilagrid.py -- once on ``F.grid_sample`` + autograd, once in closed form --, an fp32 CPU
model of the kernels' arithmetic, the scenes, the borderline set, and the per-element first-order bounds that are the
tolerance everywhere.

Statement.  gray = (gw0 r + gw1 g) + gw2 b with gw the fp32 constants 0.299, 0.587, 0.114; u = clamp(x (Wg - 1), 0,
Wg - 1), v = clamp(y (Hg - 1), 0, Hg - 1), w = clamp(gray (L - 1), 0, L - 1); per axis i0 = min(floor(u), n - 2) (0 for
n == 1), t = u - i0, weights (1 - t, t); A = sum of the 8 corners w_corner grids[g, :, l, j, i]; out_c = sum_k A[c,k]
(r, g, b, 1)_k.  The gradients are those of the module docstring.

Bounds (u = 2^-24; every count is a count of roundings in csrc/bilagrid.hip, contraction off).
* A lerp a + t (b - a) rounds three times (difference, product, sum).  With M(x) the sum of the |terms| of the lerp
  form -- M(lerp) = (1 + t) M(a) + t M(b), M(leaf) = |leaf| -- induction over the levels gives |error| <= 3 u depth M:
  9 u M(A) for the three levels x, y, z, and 6 u for the xy blends.  (The weights (1 - t, t) do not bound it: at t = 1 the
  lerp is a + (b - a), off by u |b - a| from b.)
* out_c = ((A0 r + A1 g) + A2 b) + A3: one product and three sums more: OUT_ROUNDINGS = 9 + 4 = 13 on
  sum_k M(A[c,k]) |p_k|.
* v_rgb_k: the direct part sum_c v_c A[c,k]: 9 + product + two sums + the final sum with the guidance part = 13 on
  sum_c |v_c| M(A[c,k]).  The guidance part: dA = blend(l1) - blend(l0): 6 + 1 on M_d = M_xy(l0) + M_xy(l1); q_c = dA . p:
  + 4; D = sum_c v_c q_c: + 3; the coefficient gw_k (L - 1): 1; its product with D: 1; the final sum: 1: 17 on
  |gw_k| (L - 1) sum_c |v_c| sum_k' M_d[c,k'] |p_k'|.
* A contribution to v_grids is ((wz wy) wx) (v_c p_k): three weights 1 - t, two products, v_c p_k, the last product:
  7.  A cell's n contributions are added in an order nobody fixes (LDS and global float atomics); any order is within
  (n - 1) u sum |contributions|: (7 + n - 1) u sum |contributions|.  A grid nobody uses has bound 0: exact zeros.
* Coordinates.  u = fl(x (Wg - 1)) is one rounding of an exact product: off by at most u |x (Wg - 1)|, and -- rounding
  is monotone, integers are fp32 numbers -- never across a cell border, at most ONTO it, where t = 0 and the closed cell's
  own linear piece still holds.  gray carries 3 roundings on its longest chain and w one more: off by at most
  4 u (L - 1) sum_k |gw_k rgb_k|; w may cross a border, where out and the contributions are continuous but the slope
  changes: the slope is taken as the largest of the cells at w - e_w, w, w + e_w, and the far corners of those cells
  get the contribution bound too.  Each coordinate adds |slope| times its error, the slopes by autograd of the closed
  form in float64.
* v_rgb's guidance part is NOT continuous across the cells of w, nor across the gate at gray (L - 1) = 0 and L - 1: the
  borderline set (below) is left out of the v_rgb comparison, and of that one only.
* TV value: a term ((d d) / count) carries 5 roundings (d, d d, the conversion of the count, its reciprocal, the
  product); a lane adds its 4 cells x 3 axes in order (11), then the tree of losses.hip: 6 + 3 + (ceil(G / 64) - 1) + 6,
  G = ceil(numel / TV_WG_ELEMS) workgroups.  All terms are >= 0, so sum |terms| is the value.
* TV gradient: ((x - prev) - (next - x)) (2 / count) summed over the axes, times v: inner difference 1, outer 1, the
  count's reciprocal 2 (the doubling is exact), product 1, two sums, the product with v: 8 on
  |v| sum_a (2 / count_a) (|x - prev| + |next - x|)."""
import functools

import torch
import torch.nn.functional as F

from edgegaussians_amd.bilagrid import FIN_LANES, TV_WG_ELEMS

U = 2.0 ** -24
GW = tuple(float(torch.tensor(c, dtype=torch.float32)) for c in (0.299, 0.587, 0.114))
OUT_ROUNDINGS = 13
VRGB_DIRECT_ROUNDINGS = 13
VRGB_GUIDE_ROUNDINGS = 17
CONTRIB_ROUNDINGS = 7
GRAY_ROUNDINGS = 4
TV_TERM_ROUNDINGS = 5
TV_GRAD_ROUNDINGS = 8
TV_QUAD, WAVE, TV_THREADS = 4, 64, 256
BORDERLINE_SHARE_MAX = 0.01

SCENES = ("rand", "render_like", "identity")
N_GRIDS = 3
GRID_SIZES = ((8, 16, 16), (3, 4, 5), (2, 1, 3), (1, 1, 1))      # (L, Hg, Wg)
GRID_ABOVE_BUDGET = (8, 16, 17)                                  # 48 * 2176 bytes: one column more than the LDS budget
IMAGES = (((2, 37, 53), (2, 2)), ((2, 37, 53), (0, 1)), ((1, 2 * 32 + 5, 2 * 32 + 5), (1,)))   # ((B, H, W), grid_idx)


# ---------------------------------------------------------------- scenes

def make_scene(scene, grid_size, image, seed=0):
    """(grids [N, 12, L, Hg, Wg], rgb [B, H, W, 3], xy [B, H, W, 2], v [B, H, W, 3]) fp32 CPU"""
    L, Hg, Wg = grid_size
    B, H, W = image
    g = torch.Generator().manual_seed(100 * SCENES.index(scene) + 7 * (L + Hg + Wg) + B * H * W + seed)
    eye = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0]).view(1, 12, 1, 1, 1)
    if scene == "identity":
        grids = eye.repeat(N_GRIDS, 1, L, Hg, Wg)
    else:
        grids = torch.randn(N_GRIDS, 12, L, Hg, Wg, generator=g) + (eye if scene == "render_like" else 0.0)
    if scene == "render_like":
        lo, hi = -0.02, 1.03          # reaches 0 and 1 and lies slightly outside
        hh = torch.arange(H, dtype=torch.float64).view(1, H, 1, 1) / max(H - 1, 1)
        ww = torch.arange(W, dtype=torch.float64).view(1, 1, W, 1) / max(W - 1, 1)
        ph = torch.tensor([0.0, 1.3, 2.1], dtype=torch.float64).view(1, 1, 1, 3) + torch.arange(B, dtype=torch.float64).view(B, 1, 1, 1)
        rgb = 0.5 + 0.45 * torch.sin(5.0 * hh + 3.0 * ww + ph) * torch.cos(2.0 * ww - hh)
        rgb[:, 2:2 + H // 6, 3:3 + W // 6] = 0.0          # exactly black
        rgb[:, H // 2:H // 2 + H // 16 + 1, W // 2:W // 2 + W // 16 + 1] = 1.0   # exactly white (borderline: well under 1 %)
    else:
        lo, hi = 0.0, 1.0
        rgb = torch.rand(B, H, W, 3, generator=g, dtype=torch.float64)
    xs = torch.linspace(lo, hi, W, dtype=torch.float64)
    ys = torch.linspace(lo, hi, H, dtype=torch.float64)
    if scene == "render_like" and W >= 4 and H >= 4:
        xs[1], xs[-2], ys[1], ys[-2] = 0.0, 1.0, 0.0, 1.0
    xy = torch.stack([xs.view(1, W).expand(H, W), ys.view(H, 1).expand(H, W)], dim=-1)
    v = torch.randn(B, H, W, 3, generator=g)
    return grids.float().contiguous(), rgb.float().contiguous(), xy.float().expand(B, H, W, 2).contiguous(), v.float()


# ---------------------------------------------------------------- the grid_sample statement

def gray_of(rgb):
    return (GW[0] * rgb[..., 0] + GW[1] * rgb[..., 1]) + GW[2] * rgb[..., 2]


def slice_grid_sample(grids, rgb, xy, idx):
    """out [B, H, W, 3] in the dtype of the inputs: F.grid_sample + permute + the affine product"""
    B, H, W, _ = rgb.shape
    coords = torch.cat([2.0 * xy - 1.0, 2.0 * gray_of(rgb)[..., None] - 1.0], dim=-1).view(B, 1, H, W, 3)
    A = F.grid_sample(grids[idx], coords, mode="bilinear", align_corners=True, padding_mode="border")   # [B, 12, 1, H, W]
    A = A.view(B, 12, H, W).permute(0, 2, 3, 1).reshape(B, H, W, 3, 4)
    return (A[..., :3] @ rgb[..., None]).squeeze(-1) + A[..., 3]


def grads_grid_sample(grids, rgb, xy, idx, v):
    """(out, v_rgb, v_grids) by autograd of the grid_sample statement"""
    G, p = grids.detach().clone().requires_grad_(True), rgb.detach().clone().requires_grad_(True)
    out = slice_grid_sample(G, p, xy, idx)
    v_rgb, v_grids = torch.autograd.grad(out, (p, G), v)
    return out.detach(), v_rgb, v_grids


# ---------------------------------------------------------------- the closed form

def raw_coords(rgb, xy, sizes):
    L, Hg, Wg = sizes
    return xy[..., 0] * (Wg - 1), xy[..., 1] * (Hg - 1), gray_of(rgb) * (L - 1)


def cell_of(raw, n):
    """(clamped coordinate, i0, i1) on an axis of n cells"""
    c = raw.clamp(0.0, float(n - 1))
    i0 = torch.floor(c).long().clamp(max=n - 2).clamp(min=0)
    return c, i0, (i0 + 1).clamp(max=n - 1)


class Blend:
    """the trilinear blend of one call, at clamped coordinates (cu, cv, cw) inside the given cells"""

    def __init__(self, grids, idx, cu, cv, cw, cells):
        self.i0, self.i1, self.j0, self.j1, self.l0, self.l1 = cells
        B = cu.shape[0]
        self.Gc = grids[idx].permute(0, 2, 3, 4, 1)                      # [B, L, Hg, Wg, 12]
        self.bi = torch.arange(B).view(B, *([1] * (cu.dim() - 1))).expand(cu.shape)
        self.tx, self.ty, self.tz = cu - self.i0, cv - self.j0, cw - self.l0

    def corner(self, z, y, x):
        return self.Gc[self.bi, (self.l0, self.l1)[z], (self.j0, self.j1)[y], (self.i0, self.i1)[x]]   # [..., 12]

    def weight(self, z, y, x):
        w = lambda t, s: t if s else 1.0 - t
        return w(self.tz, z) * w(self.ty, y) * w(self.tx, x)

    def xy_blend(self, z, absolute=False, lerp_weights=False):
        """sum over (y, x) of the weights times the corners of level z; `absolute`: of |corner|; `lerp_weights`:
        (1 + t, t) in place of (1 - t, t): M of the lerp form"""
        w = (lambda t, s: t if s else 1.0 + t) if lerp_weights else (lambda t, s: t if s else 1.0 - t)
        acc = 0.0
        for y in (0, 1):
            for x in (0, 1):
                c = self.corner(z, y, x)
                acc = acc + (w(self.ty, y) * w(self.tx, x))[..., None] * (c.abs() if absolute else c)
        return acc

    def A(self):
        return (1.0 - self.tz)[..., None] * self.xy_blend(0) + self.tz[..., None] * self.xy_blend(1)

    def dA(self):
        return self.xy_blend(1) - self.xy_blend(0)

    def M_A(self):
        return (1.0 + self.tz)[..., None] * self.xy_blend(0, True, True) + self.tz[..., None] * self.xy_blend(1, True, True)

    def M_d(self):
        return self.xy_blend(0, True, True) + self.xy_blend(1, True, True)


def _p4(rgb):
    return torch.cat([rgb, torch.ones_like(rgb[..., :1])], dim=-1)


def _out_of(bl, rgb):
    return (bl.A().reshape(*rgb.shape[:-1], 3, 4) * _p4(rgb)[..., None, :]).sum(-1)


def _vrgb_of(bl, rgb, v, gate, L):
    A, dA = bl.A().reshape(*rgb.shape[:-1], 3, 4), bl.dA().reshape(*rgb.shape[:-1], 3, 4)
    direct = (v[..., :, None] * A[..., :, :3]).sum(-2)
    D = (v[..., :, None] * dA * _p4(rgb)[..., None, :]).sum((-1, -2))
    gw = torch.tensor(GW, dtype=rgb.dtype)
    return direct + gw * (L - 1) * (gate.to(rgb.dtype) * D)[..., None]


def _cells(raws, sizes):
    L, Hg, Wg = sizes
    cu, i0, i1 = cell_of(raws[0], Wg)
    cv, j0, j1 = cell_of(raws[1], Hg)
    cw, l0, l1 = cell_of(raws[2], L)
    return (cu, cv, cw), (i0, i1, j0, j1, l0, l1)


def closed_form(grids, rgb, xy, idx, v):
    """(out, v_rgb, v_grids) in closed form, in the dtype of the inputs"""
    N, _, L, Hg, Wg = grids.shape
    raws = raw_coords(rgb, xy, (L, Hg, Wg))
    (cu, cv, cw), cells = _cells(raws, (L, Hg, Wg))
    bl = Blend(grids, idx, cu, cv, cw, cells)
    gate = (raws[2] > 0) & (raws[2] < L - 1)
    out = _out_of(bl, rgb)
    v_rgb = _vrgb_of(bl, rgb, v, gate, L)
    vA = (v[..., :, None] * _p4(rgb)[..., None, :]).reshape(*rgb.shape[:-1], 12)
    v_grids = _scatter(grids, idx, bl, lambda z, y, x: bl.weight(z, y, x)[..., None] * vA)
    return out, v_rgb, v_grids


def _scatter(grids, idx, bl, value_of, cells=None):
    """sum over samples and corners of value_of(z, y, x) [..., 12] into the shape of grids"""
    N, _, L, Hg, Wg = grids.shape
    n_cells = L * Hg * Wg
    acc = torch.zeros(N * n_cells, 12, dtype=torch.float64)
    g = torch.as_tensor(idx).view(-1, *([1] * (bl.tx.dim() - 1))).expand(bl.tx.shape)
    for z in (0, 1):
        for y in (0, 1):
            for x in (0, 1):
                cell = ((bl.l0, bl.l1)[z] * Hg + (bl.j0, bl.j1)[y]) * Wg + (bl.i0, bl.i1)[x]
                acc.index_add_(0, (g * n_cells + cell).reshape(-1), value_of(z, y, x).reshape(-1, 12).double())
    return acc.view(N, L, Hg, Wg, 12).permute(0, 4, 1, 2, 3).contiguous()


# ---------------------------------------------------------------- borderline set and bounds

def borderline(rgb64, L):
    """bool [B, H, W]: the samples left out of the v_rgb comparison (module docstring).  gray == 0 -- black pixels, and
    every pixel's w when L == 1 -- is computed exactly on both sides: never borderline."""
    gray = gray_of(rgb64)
    w = gray * (L - 1)
    near_int = ((w - torch.round(w)).abs() < 1e-5 * max(1, L - 1)) if L > 1 else torch.zeros_like(gray, dtype=torch.bool)
    near_end = (gray.abs() < 1e-6) | ((gray - 1.0).abs() < 1e-6)
    return (near_int | near_end) & (gray != 0)


def _slopes(fn, coords):
    """|d fn_k / d coordinate| per sample for the three outputs k: [3 coords][..., 3]"""
    leaves = [c.detach().clone().requires_grad_(True) for c in coords]
    y = fn(*leaves)
    per_k = [torch.autograd.grad(y[..., k].sum(), leaves, retain_graph=True, allow_unused=True) for k in range(3)]
    return [torch.stack([(per_k[k][a] if per_k[k][a] is not None else torch.zeros_like(leaves[a])).abs() for k in range(3)], dim=-1)
            for a in range(3)]


def bounds(grids, rgb, xy, idx, v):
    """(bound_out, bound_v_rgb, bound_v_grids) in float64 for fp32 inputs (module docstring)"""
    grids, rgb, xy, v = grids.double(), rgb.double(), xy.double(), v.double()
    N, _, L, Hg, Wg = grids.shape
    sizes = (L, Hg, Wg)
    raws = raw_coords(rgb, xy, sizes)
    e_u, e_v = U * raws[0].abs(), U * raws[1].abs()
    e_w = GRAY_ROUNDINGS * U * (L - 1) * sum(abs(GW[k]) * rgb[..., k].abs() for k in range(3))
    gate = (raws[2] > 0) & (raws[2] < L - 1)
    p4, gw = _p4(rgb).abs(), torch.tensor(GW, dtype=torch.float64).abs()
    (cu, cv, cw), cells = _cells(raws, sizes)
    bl = Blend(grids, idx, cu, cv, cw, cells)
    M_A, M_d = bl.M_A().reshape(*rgb.shape[:-1], 3, 4), bl.M_d().reshape(*rgb.shape[:-1], 3, 4)
    b_out = OUT_ROUNDINGS * U * (M_A * p4[..., None, :]).sum(-1)
    b_rgb = (VRGB_DIRECT_ROUNDINGS * U * (v.abs()[..., :, None] * M_A[..., :, :3]).sum(-2)
             + VRGB_GUIDE_ROUNDINGS * U * gw * (L - 1)
             * (gate.double() * (v.abs()[..., :, None] * M_d * p4[..., None, :]).sum((-1, -2)))[..., None])
    # coordinate terms: the slopes in the cells at w - e_w, w, w + e_w (u and v never leave their closed cell)
    s_out, s_rgb = [None] * 3, [None] * 3
    vA = (v[..., :, None] * _p4(rgb)[..., None, :]).reshape(*rgb.shape[:-1], 12).abs()
    b_grids = torch.zeros_like(grids)
    count = torch.zeros_like(grids)
    for shift in (0.0, -1.0, 1.0):
        _, cells_s = _cells((raws[0], raws[1], raws[2] + shift * e_w), sizes)
        make = lambda a, b, c, cells_s=cells_s: Blend(grids, idx, a, b, c, cells_s)
        so = _slopes(lambda a, b, c: _out_of(make(a, b, c), rgb), (cu, cv, cw))
        sr = _slopes(lambda a, b, c: _vrgb_of(make(a, b, c), rgb, v, gate, L), (cu, cv, cw))
        s_out = [x if y is None else torch.maximum(x, y) for x, y in zip(so, s_out)]
        s_rgb = [x if y is None else torch.maximum(x, y) for x, y in zip(sr, s_rgb)]
        bs = make(cu, cv, cw)
        moved = torch.ones_like(gate) if shift == 0.0 else (cells_s[4] != cells[4])
        wa = lambda t, s: (t if s else 1.0 - t).abs()

        def coord_part(z, y, x, bs=bs, moved=moved, own=(shift == 0.0)):
            wz, wy, wx = wa(bs.tz, z), wa(bs.ty, y), wa(bs.tx, x)
            part = wy * wx * e_w
            if own:
                part = part + wz * wy * e_u + wz * wx * e_v
            return (moved.double() * part)[..., None] * vA

        b_grids = b_grids + _scatter(grids, idx, bs, coord_part)
        if shift == 0.0:
            terms = _scatter(grids, idx, bs, lambda z, y, x: bs.weight(z, y, x).abs()[..., None] * vA)
        count = count + _scatter(grids, idx, bs, lambda z, y, x: moved.double()[..., None] * torch.ones_like(vA))
    errs = (e_u, e_v, e_w)
    b_out = b_out + sum(s_out[a] * errs[a][..., None] for a in range(3))
    b_rgb = b_rgb + sum(s_rgb[a] * errs[a][..., None] for a in range(3))
    b_grids = b_grids + (CONTRIB_ROUNDINGS + (count - 1.0).clamp(min=0.0)) * U * terms
    return b_out, b_rgb, b_grids


def ratio(got, ref, bound, keep=None):
    """(largest |got - ref| / bound over the kept elements with a positive bound, number of kept elements over their
    bound -- an element whose bound is zero must be exact)"""
    err = (got.double() - ref).abs()
    if keep is not None:
        err, bound = err[keep], bound[keep]
    pos = bound > 0
    return (float((err[pos] / bound[pos]).max()) if pos.any() else 0.0), int((err > bound).sum())


# (max_workgroups, image, grid_idx): the persistent LDS kernels with fewer workgroups than the default 256, so that
# at test sizes one workgroup walks several blocks of samples (persistent_plan: what the host then launches)
PERSISTENT_CASES = ((1, (1, 2 * 32 + 5, 2 * 32 + 5), (1,)), (2, (2, 37, 53), (2, 2)), (3, (1, 2 * 32 + 5, 2 * 32 + 5), (1,)))


def persistent_plan(B, per_image, max_workgroups, threads=1024):
    """the launch arithmetic of csrc/bilagrid.hip restated: (workgroups per image of the forward / v_rgb kernel, its
    trips through the sample loop in workgroup 0, workgroups per image of the scatter, its `run` = consecutive samples
    per lane)"""
    most = -(-per_image // threads)
    blocks = min(max(-(-max_workgroups // B), 1), most)
    trips = -(-per_image // (blocks * threads))
    run = -(-per_image // (blocks * threads))
    return blocks, trips, -(-per_image // (run * threads)), run


WAVE_IMAGE = (1, 5, 70)      # 350 samples in flat order: two workgroups of 256 of the kernel for grids above the budget
WAVE_SHARED = ((0, 192), (320, 350))   # flat ranges whose samples all lie in ONE cell: waves 0-2 and the last, partial wave


def make_wave_scene(grid_size=GRID_ABOVE_BUDGET):
    """The scene for the wave-combined scatter of grids above the LDS budget (csrc/bilagrid.hip:
    slice_vgrid_global_kernel): random grids; the samples [0, 192) -- three whole waves -- share one xy and colours whose
    luminance stays inside one cell of the guidance axis, so each of those waves adds its 64 samples with the DPP tree;
    [192, 320) are a mesh with random colours (two waves that do not share a cell: one atomic per lane); [320, 350) share
    another cell and are the live lanes of the last wave, whose lanes from 350 on carry zeros."""
    L, Hg, Wg = grid_size
    B, H, W = WAVE_IMAGE
    g = torch.Generator().manual_seed(77)
    grids = torch.randn(N_GRIDS, 12, L, Hg, Wg, generator=g)
    n = H * W
    rgb = torch.rand(n, 3, generator=g, dtype=torch.float64)
    xy = torch.rand(n, 2, generator=g, dtype=torch.float64)
    for (lo, hi), (x, y, level) in zip(WAVE_SHARED, ((0.30, 0.62, 2.2), (0.81, 0.13, 4.3))):
        xy[lo:hi] = torch.tensor([x, y], dtype=torch.float64)
        # luminance in (level, level + 0.5) / (L - 1): every channel equal, so gray = the channel (gw sums to 1)
        rgb[lo:hi] = ((level + 0.5 * torch.rand(hi - lo, 1, generator=g, dtype=torch.float64)) / max(L - 1, 1)).expand(-1, 3)
    v = torch.randn(B, H, W, 3, generator=g)
    return grids.float().contiguous(), rgb.float().view(B, H, W, 3).contiguous(), xy.float().view(B, H, W, 2).contiguous(), v.float()


@functools.lru_cache(maxsize=None)
def wave_reference():
    """reference() for make_wave_scene on grid 1, with `shared`: bool [n], the samples of the one-cell ranges"""
    grids, rgb, xy, v = make_wave_scene()
    ref = _reference_of(grids, rgb, xy, v, [1], GRID_ABOVE_BUDGET[0])
    shared = torch.zeros(rgb.shape[1] * rgb.shape[2], dtype=torch.bool)
    for lo, hi in WAVE_SHARED:
        shared[lo:hi] = True
    return dict(ref, shared=shared)


@functools.lru_cache(maxsize=None)
def reference(scene, grid_size, image, idx):
    """Everything the comparisons of one case need, computed once and never modified: fp32 inputs, the float64
    grid_sample statement with its gradients, the bounds and the borderline set."""
    grids, rgb, xy, v = make_scene(scene, grid_size, image)
    return _reference_of(grids, rgb, xy, v, list(idx), grid_size[0])


def _reference_of(grids, rgb, xy, v, index, L):
    out, v_rgb, v_grids = grads_grid_sample(grids.double(), rgb.double(), xy.double(), index, v.double())
    b_out, b_rgb, b_grids = bounds(grids, rgb, xy, index, v)
    return dict(grids=grids, rgb=rgb, xy=xy, v=v, idx=index, out=out, v_rgb=v_rgb, v_grids=v_grids, bound_out=b_out,
                bound_v_rgb=b_rgb, bound_v_grids=b_grids, borderline=borderline(rgb.double(), L))


def cases():
    """(grid size, image, grid_idx) of the device tests"""
    for grid_size in GRID_SIZES + (GRID_ABOVE_BUDGET,):
        for image, idx in IMAGES:
            yield grid_size, image, idx


# ---------------------------------------------------------------- the fp32 model of the kernels

def _axis_f32(raw, n):
    top = torch.tensor(float(n - 1), dtype=torch.float32)
    u = torch.minimum(torch.maximum(raw, torch.zeros((), dtype=torch.float32)), top)
    i0 = torch.floor(u).long().clamp(max=n - 2).clamp(min=0)
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, u - i0.to(torch.float32)


def _lerp(a, b, t):
    return a + t * (b - a)


def model_f32(grids, rgb, xy, idx, v):
    """(out, v_rgb, v_grids) of fp32 CPU tensors in the arithmetic of csrc/bilagrid.hip: nested lerps, the sums in the
    kernels' order, the select on the gate; v_grids added in index_add's order (one of the orders the bound covers)"""
    N, _, L, Hg, Wg = grids.shape
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    gw = [torch.tensor(c, dtype=torch.float32) for c in (0.299, 0.587, 0.114)]
    gray = (gw[0] * r + gw[1] * g) + gw[2] * b
    top = torch.tensor(float(L - 1), dtype=torch.float32)
    wraw = gray * top
    gate = (wraw > 0) & (wraw < top)
    i0, i1, tx = _axis_f32(xy[..., 0] * float(Wg - 1), Wg)
    j0, j1, ty = _axis_f32(xy[..., 1] * float(Hg - 1), Hg)
    l0, l1, tz = _axis_f32(wraw, L)
    B = rgb.shape[0]
    Gc = grids[idx].permute(0, 2, 3, 4, 1)
    bi = torch.arange(B).view(B, 1, 1).expand(tx.shape)
    c = lambda l, j, i: Gc[bi, l, j, i]
    t3 = lambda t: t[..., None]
    a0 = _lerp(_lerp(c(l0, j0, i0), c(l0, j0, i1), t3(tx)), _lerp(c(l0, j1, i0), c(l0, j1, i1), t3(tx)), t3(ty))
    a1 = _lerp(_lerp(c(l1, j0, i0), c(l1, j0, i1), t3(tx)), _lerp(c(l1, j1, i0), c(l1, j1, i1), t3(tx)), t3(ty))
    A = _lerp(a0, a1, t3(tz)).reshape(*tx.shape, 3, 4)
    dA = (a1 - a0).reshape(*tx.shape, 3, 4)
    out = ((A[..., 0] * t3(r) + A[..., 1] * t3(g)) + A[..., 2] * t3(b)) + A[..., 3]
    q = ((dA[..., 0] * t3(r) + dA[..., 1] * t3(g)) + dA[..., 2] * t3(b)) + dA[..., 3]
    D = (v[..., 0] * q[..., 0] + v[..., 1] * q[..., 1]) + v[..., 2] * q[..., 2]
    direct = (v[..., 0:1] * A[..., 0, :3] + v[..., 1:2] * A[..., 1, :3]) + v[..., 2:3] * A[..., 2, :3]
    coef = torch.stack([gw[k] * top for k in range(3)])
    v_rgb = torch.where(t3(gate), direct + coef * t3(D), direct)
    # scatter, fp32, index_add order
    cells = L * Hg * Wg
    acc = torch.zeros(N * cells, 12, dtype=torch.float32)
    gi = torch.as_tensor(idx).view(-1, 1, 1).expand(tx.shape)
    p4 = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1)
    vA = (v[..., :, None] * p4[..., None, :]).reshape(*tx.shape, 12)
    for z in (0, 1):
        for y in (0, 1):
            for x in (0, 1):
                wz = tz if z else 1 - tz
                wy = ty if y else 1 - ty
                wx = tx if x else 1 - tx
                w = (wz * wy) * wx
                cell = ((l1 if z else l0) * Hg + (j1 if y else j0)) * Wg + (i1 if x else i0)
                acc.index_add_(0, (gi * cells + cell).reshape(-1), (t3(w) * vA).reshape(-1, 12))
    v_grids = acc.view(N, L, Hg, Wg, 12).permute(0, 4, 1, 2, 3)
    return out, v_rgb, v_grids


# ---------------------------------------------------------------- total variation

def tv_counts(shape):
    N, _, L, Hg, Wg = shape
    return [N * 12 * (n - 1) * (L * Hg * Wg // n) for n in (L, Hg, Wg)]


def tv_ref(x):
    total = x.new_zeros(())
    for axis in (2, 3, 4):
        n = x.shape[axis]
        if n > 1:
            total = total + ((x.narrow(axis, 1, n - 1) - x.narrow(axis, 0, n - 1)) ** 2).mean()
    return total


def _tv_diffs(x, axis):
    """(x - prev where prev exists else 0, next - x where next exists else 0) along axis"""
    n = x.shape[axis]
    dp, dn = torch.zeros_like(x), torch.zeros_like(x)
    if n > 1:
        d = x.narrow(axis, 1, n - 1) - x.narrow(axis, 0, n - 1)
        dp.narrow(axis, 1, n - 1).copy_(d)
        dn.narrow(axis, 0, n - 1).copy_(d)
    return dp, dn


def tv_grad_closed(x, v=1.0):
    g = torch.zeros_like(x)
    for axis, count in zip((2, 3, 4), tv_counts(x.shape)):
        if x.shape[axis] > 1:
            dp, dn = _tv_diffs(x, axis)
            g = g + (2.0 / count) * (dp - dn)
    return v * g


def tv_depth(numel):
    G = -(-numel // TV_WG_ELEMS)
    return (3 * TV_QUAD - 1) + 6 + (TV_THREADS // WAVE - 1) + (-(-G // FIN_LANES) - 1) + 6


def tv_bounds(x, v=1.0):
    """(bound of the value, bound of the gradient) for the fp32 grids x"""
    x = x.double()
    b_value = (TV_TERM_ROUNDINGS + tv_depth(x.numel())) * U * float(tv_ref(x))
    mag = torch.zeros_like(x)
    for axis, count in zip((2, 3, 4), tv_counts(x.shape)):
        if x.shape[axis] > 1:
            dp, dn = _tv_diffs(x, axis)
            mag = mag + (2.0 / count) * (dp.abs() + dn.abs())
    return b_value, TV_GRAD_ROUNDINGS * U * abs(v) * mag


TV_SHAPES = ((3, 12, 8, 16, 16), (3, 12, 3, 4, 5), (3, 12, 2, 1, 3), (2, 12, 1, 1, 1), (1, 12, 1, 7, 1),
             (6, 12, 8, 16, 16 * 3 + 1))    # the last: more workgroups than the finalize wave has lanes


@functools.lru_cache(maxsize=None)
def tv_case(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).float()
    x64 = x.double().requires_grad_(True)
    value = tv_ref(x64)
    grad, = torch.autograd.grad(value, x64) if value.requires_grad and value.grad_fn is not None else (torch.zeros_like(x64),)
    b_value, b_grad = tv_bounds(x)
    return dict(x=x, value=float(value.detach()), grad=grad, bound_value=b_value, bound_grad=b_grad)
