"""Host helpers of the per-pixel / per-Gaussian tests of the TRAINING STEP's unit-colour compositing
(tests/test_step_composite_host.py, tests/test_gpu_step_composite.py).  Nothing here needs a GPU.

  ref_forward    float64 front-to-back walk of every pixel over the sorted list of its 16-pixel tile: T_final, last
                 contributor, stop, alphas, render, v, the {gT, stop_id, stop_depth} record of finalize_pixel
                 (csrc/composite.h) and the loss sum
  ref_backward   float64 footprint backward FROM A GIVEN RECORD IMAGE: per Gaussian the eight g2d columns, summed over
                 the pixels of gsplat's tile box (intersected with the image) -- no tile lists, like the kernel
  ref_autograd   the same gradient through CU.ref_composite (colours all ones, one channel) and autograd
  record_kappa   kappa_r of every row from N_DRAWS one-ulp perturbations of the records AND of the gT words
  model32_T      the fp32 model of the forward's transmittance in the kernels' two orders (one running product; a
                 product of 128-Gaussian slice products) -- what d32, the gT tolerance, is measured from

Records are CU.pack_records' [N, 8] fp32 rows (x y a b c o depth radius-bits); lists are CU.Lists (classic offsets).
A record no projection produces -- radius <= 0, a <= 0 or det <= 0 -- is invisible by the kernels' contract
(walk_of in csrc/footprint_dev.h) and by this reference.
"""
import collections
import functools
import math

import numpy as np
import torch

from tests import composite_util as CU
from tests.util import REL_ALPHA, row_kappa, ulp_perturbed

TS = 16
AMIN, AMAX, TSTOP = CU.AMIN, CU.AMAX, CU.TSTOP
NO_STOP_DEPTH = 0xFFFFFFFF
BORDER_SHARE_CAP = 0.03           # the cap of tests/test_gpu_oracle_floats.py
SIGN_MARGIN = 1e-6                # |clamp(pix) - gt| below this (and != 0): the sign of v hinges on rounding (tests/util.py)
GT_TOL_FACTOR, GT_TOL_FLOOR = 4.0, 1e-6   # gT: max(4 d32, 1e-6) relative, the rule and margin of tests/test_gpu_sh.py
# Share of a case's live rows whose relative bound ROW_FLOOR + ROW_KAPPA_FACTOR kappa_r may exceed ROW_LOOSE, per column
# group at most.  The 3 % of the projection tests cannot hold here (tests/test_step_composite_host.py says why); these
# are properties of the float64 reference alone: half of the rows of a random scene, nearly all rows of the cases made
# of sub-pixel and 30:1 Gaussians, every row on the 2304-px image (one ulp of x = 1000 is 6e-5 px).
LOOSE_CAP = {"n": 0.6, "mix": 0.9, "shear": 0.9, "stops": 0.3, "large": 1.0}
FP_W, FP_H = 72, 40               # image of the footprint cases: 4.5 x 2.5 tiles
BIG_W, BIG_H = 2304, 1824         # rows x ceil(pw / 2) = 1824 x 1152 = 2.10 M pairs > 2^21

Fwd = collections.namedtuple("Fwd", "T last_idx last_id stopped alphas v gT stop_id stop_depth loss abs_terms n_terms")
RecImg = collections.namedtuple("RecImg", "gT stop_id stop_depth")     # float [H, W], int64 [H, W], int64 [H, W]


def tiles_of(W, H):
    return math.ceil(W / TS), math.ceil(H / TS)


def lists_of(rec, W, H):
    """CU.Lists of 16-pixel tiles from oracle.ref_torch's integer binning on the records' floats"""
    from oracle import ref_torch as O
    tw, th = tiles_of(W, H)
    _tpg, ids, flat = O.isect_tiles(rec[:, 0:2], rec[:, 7].view(np.int32), rec[:, 6], TS, tw, th)
    offs = np.concatenate([O.isect_offset_encode(ids, tw, th).reshape(-1), [flat.shape[0]]]).astype(np.int32)
    return CU.Lists(offs, np.ascontiguousarray(flat, np.int32))


def depth_bits(rec):
    return np.ascontiguousarray(rec[:, 6]).view(np.uint32).astype(np.int64)


def lists_sorted(rec, lst):
    """every tile's list ascending by (depth bits, id)"""
    key = (depth_bits(rec)[lst.flat] << 32) | lst.flat.astype(np.int64)
    return all(np.all(np.diff(key[lst.offsets[t]:lst.offsets[t + 1]]) > 0) for t in range(len(lst.offsets) - 1))


# ---------------------------------------------------------------------------------------------------
# forward
def ref_forward(rec, lst, W, H, gt=None, wmap=None, loss_scale=1.0, vals=None):
    """Float64 walk.  vals: float64 [N, 6] replacing the records' x y a b c o (perturbed draws).  Without wmap the
    record carries T_final itself (v = 1) and the loss is 0.  abs_terms / n_terms: sum of |w |c0 - gt|| and the number of
    non-zero terms (the loss check's cancellation slack)."""
    tw, th = tiles_of(W, H)
    p = np.asarray(rec[:, 0:6], np.float64) if vals is None else vals
    T_img = np.ones((H, W))
    last_idx = np.full((H, W), -1, np.int64)
    stopped = np.zeros((H, W), bool)
    offs = np.asarray(lst.offsets, np.int64)
    for t in range(tw * th):
        g = lst.flat[offs[t]:offs[t + 1]]
        if g.size == 0:
            continue
        ty, tx = divmod(t, tw)
        ii, jj = np.meshgrid(np.arange(ty * TS, min(ty * TS + TS, H)), np.arange(tx * TS, min(tx * TS + TS, W)), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        dx = p[g, 0][None, :] - (jj[:, None] + 0.5)
        dy = p[g, 1][None, :] - (ii[:, None] + 0.5)
        sigma = 0.5 * (p[g, 2] * dx * dx + p[g, 4] * dy * dy) + p[g, 3] * dx * dy
        alpha = np.minimum(AMAX, p[g, 5][None, :] * np.exp(-sigma))
        incl = (sigma >= 0.0) & (alpha >= AMIN)
        T_after = np.cumprod(np.where(incl, 1.0 - alpha, 1.0), axis=1)
        stops = incl & (T_after <= TSTOP)
        has_stop = stops.any(axis=1)
        first = np.where(has_stop, stops.argmax(axis=1), g.size)
        idx = np.arange(g.size)[None, :]
        contrib = incl & (idx < first[:, None])
        T_img[ii, jj] = np.prod(np.where(contrib, 1.0 - alpha, 1.0), axis=1)
        last = np.where(contrib, idx, -1).max(axis=1)
        last_idx[ii, jj] = np.where(last >= 0, last + offs[t], -1)
        stopped[ii, jj] = has_stop
    touched = last_idx >= 0
    last_id = np.where(touched, lst.flat[np.maximum(last_idx, 0)] if lst.flat.size else 0, -1).astype(np.int64)
    alphas = np.where(touched, 1.0 - T_img, 0.0)
    if wmap is not None:
        d = np.clip(alphas, 0.0, 1.0) - np.asarray(gt, np.float64)
        w = np.asarray(wmap, np.float64)
        v = float(loss_scale) * w * np.sign(d)
        terms = w * np.abs(d)
        loss, abs_terms, n_terms = float(terms.sum()), float(np.abs(terms).sum()), int((terms != 0).sum())
    else:
        v, loss, abs_terms, n_terms = np.ones((H, W)), 0.0, 0.0, 0
    gT = np.where(touched, v * T_img, 0.0)
    stop_id = np.where(stopped, last_id, -1)
    stop_depth = np.where(stopped, depth_bits(rec)[np.maximum(last_id, 0)], NO_STOP_DEPTH)
    return Fwd(T_img, last_idx, last_id, stopped, alphas, v, gT, stop_id, stop_depth, loss, abs_terms, n_terms)


def fwd_ref_dict(f):
    """the [1, H, W (, 1)] dict CU.fwd_check takes (a pixel nothing contributes to reports index 0, as the kernels do)"""
    return {"alphas": torch.from_numpy(f.alphas)[None], "render": torch.from_numpy(f.alphas)[None, ..., None],
            "last_ids": torch.from_numpy(np.maximum(f.last_idx, 0))[None]}


def forward_borderline(rec, lst, W, H, f=None, gt=None):
    """bool [H, W]: CU.borderline_walk's mask, plus (with gt) the pixels whose sign of clamp(pix) - gt hinges on rounding"""
    m = CU.borderline_walk(rec[:, 0:2], rec[:, 2:5], rec[:, 5], lst.flat, lst.offsets, TS, W, H, CU.STAGE[TS]).mask.numpy().copy()
    if gt is not None:
        d = np.clip(f.alphas, 0.0, 1.0) - np.asarray(gt, np.float64)
        m |= (np.abs(d) < SIGN_MARGIN) & (d != 0)
    return m


def loss_slack(f, rel):
    """|device loss - float64 loss| allowed: `rel` of the sum, plus the rounding of an fp32 sum of n terms in any order,
    n 2^-23 sum|terms| (each of the n - 1 additions rounds a partial sum that is at most sum|terms|)"""
    return rel * abs(f.loss) + f.n_terms * 2.0 ** -23 * f.abs_terms


# ---------------------------------------------------------------------------------------------------
# backward from a record image
def _visible(rec):
    r = rec[:, 7].view(np.int32)
    a, b, c = (rec[:, k].astype(np.float64) for k in (2, 3, 4))
    return (r > 0) & (a > 0) & (a * c - b * b > 0) & (rec[:, 5] > 0)


def pixel_boxes(rec, W, H):
    """gsplat's tile box of every Gaussian in pixels, cut to the image: j0, i0, j1, i1 (exclusive ends)"""
    from oracle import ref_torch as O
    tw, th = tiles_of(W, H)
    x0, y0, x1, y1 = O.tile_bounds(rec[:, 0:2], rec[:, 7].view(np.int32), TS, tw, th)
    return x0 * TS, y0 * TS, np.minimum(x1 * TS, W), np.minimum(y1 * TS, H)


def _footprints(rec, W, H, vals=None, only=None):
    """yields (g, row slice, column slice, dx, dy, sigma, vis, araw) over the visible Gaussians' boxes, float64; the box
    is also cut to a generous bound of the ellipse o exp(-sigma) >= 1/255 (1 % + 2 px wider), outside which nothing counts"""
    p = np.asarray(rec[:, 0:6], np.float64) if vals is None else vals
    j0, i0, j1, i1 = pixel_boxes(rec, W, H)
    sel = _visible(rec) & (j1 > j0) & (i1 > i0)
    for g in (np.nonzero(sel)[0] if only is None else [k for k in only if sel[k]]):
        x, y, a, b, c, o = p[g]
        k = 2.0 * max(math.log(255.0 * o), 0.0) / (a * c - b * b)
        ex, ey = math.sqrt(k * c) * 1.01 + 2.0, math.sqrt(k * a) * 1.01 + 2.0
        ja, jb = max(int(j0[g]), math.floor(x - ex)), min(int(j1[g]), math.ceil(x + ex))
        ia, ib = max(int(i0[g]), math.floor(y - ey)), min(int(i1[g]), math.ceil(y + ey))
        if jb <= ja or ib <= ia:
            continue
        dx = x - (np.arange(ja, jb) + 0.5)[None, :]
        dy = y - (np.arange(ia, ib) + 0.5)[:, None]
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        vis = np.exp(-sigma)
        yield g, slice(ia, ib), slice(ja, jb), dx, dy, sigma, vis, o * vis


def ref_backward(rec, img, W, H, vals=None, tie_lt=False, only=None):
    """[N, 8] float64: vx vy |vx| |vy| va vb vc vo of every Gaussian from the record image `img` (RecImg).  A pixel
    counts for Gaussian g where sigma >= 0, 1/255 <= o exp(-sigma), and -- where the record has a stop --
    (depth bits, g) <= (stop_depth, stop_id); no gradient through a contribution capped at 0.999.
    tie_lt: the PLANTED defect of the host test, (depth bits, g) < (stop_depth, stop_id).  only: the rows to compute."""
    out = np.zeros((rec.shape[0], 8))
    dbits = depth_bits(rec)
    p = np.asarray(rec[:, 0:6], np.float64) if vals is None else vals
    for g, si, sj, dx, dy, sigma, vis, araw in _footprints(rec, W, H, vals, only):
        sid, sd = img.stop_id[si, sj], img.stop_depth[si, sj]
        tie = (g < sid) if tie_lt else (g <= sid)
        counts = (sid < 0) | (dbits[g] < sd) | ((dbits[g] == sd) & tie)
        ok = (sigma >= 0.0) & (araw >= AMIN) & (araw <= AMAX) & counts
        v_alpha = np.where(ok, img.gT[si, sj] / np.where(ok, 1.0 - araw, 1.0), 0.0)
        w = -araw * v_alpha
        a, b, c = p[g, 2:5]
        gx, gy = w * (a * dx + b * dy), w * (b * dx + c * dy)
        out[g] = (gx.sum(), gy.sum(), np.abs(gx).sum(), np.abs(gy).sum(), 0.5 * (w * dx * dx).sum(), (w * dx * dy).sum(),
                  0.5 * (w * dy * dy).sum(), (vis * v_alpha).sum())
    return out


def record_borderline(rec, W, H):
    """bool [H, W]: pixels at which ANY Gaussian's o exp(-sigma) lies within REL_ALPHA of 1/255 or of 0.999"""
    m = np.zeros((H, W), bool)
    for _g, si, sj, _dx, _dy, sigma, _vis, araw in _footprints(rec, W, H):
        m[si, sj] |= (np.abs(araw - AMIN) <= REL_ALPHA * AMIN) | (np.abs(araw - AMAX) <= REL_ALPHA * AMAX)
    return m


def masked(img, mask):
    """the record image with gT = 0 on `mask` (both sides get it)"""
    return RecImg(np.where(mask, 0.0, img.gT), img.stop_id, img.stop_depth)


def record_of(f, mask=None):
    """RecImg of a reference forward, gT rounded to fp32 (what a device image can hold), zero on `mask`"""
    gT = f.gT.astype(np.float32).astype(np.float64)
    return RecImg(gT if mask is None else np.where(mask, 0.0, gT), f.stop_id.astype(np.int64), f.stop_depth.astype(np.int64))


def record_kappa(rec, img, W, H, ref=None, seed=77):
    """(float64 reference [N, 8], {column group: kappa_r [N]}) under N_DRAWS one-ulp draws on x y a b c o and the gT words"""
    ref = ref_backward(rec, img, W, H) if ref is None else ref
    gen = torch.Generator().manual_seed(seed)
    draws = []
    for _ in range(CU.N_DRAWS):
        vals, gT = ulp_perturbed([torch.from_numpy(np.ascontiguousarray(rec[:, 0:6])), torch.from_numpy(img.gT)], gen)
        draws.append(ref_backward(rec, RecImg(gT.numpy(), img.stop_id, img.stop_depth), W, H, vals=vals.numpy()))
    kappa = {k: row_kappa(torch.from_numpy(ref[:, a:b]), [d[:, a:b] for d in draws]) for k, (a, b) in CU.G2D_COLS.items()}
    return ref, kappa


def device_image(img):
    """[H, W, 3] int32 words of a RecImg: fp32 gT bits, stop id, stop depth bits"""
    out = np.empty(img.gT.shape + (3,), np.int32)
    out[..., 0] = img.gT.astype(np.float32).view(np.int32)
    out[..., 1] = img.stop_id.astype(np.int32)
    out[..., 2] = img.stop_depth.astype(np.uint32).view(np.int32)
    return out


def image_of_words(words):
    """RecImg of a device's [H, W, 3] int32 words"""
    w = np.ascontiguousarray(words)
    return RecImg(w[..., 0].view(np.float32).astype(np.float64), w[..., 1].astype(np.int64),
                  w[..., 2].view(np.uint32).astype(np.int64))


def ref_autograd(rec, lst, v):
    """[N, 8] float64 through CU.ref_composite (CU.W x CU.H, colours all ones, one channel, v_render = v) and autograd"""
    ones = torch.ones(rec.shape[0], 1)
    r = CU.ref_composite((rec,), ones, None, False, (lst,), TS, torch.from_numpy(v)[None, ..., None], None)
    return np.concatenate([r[k][0].numpy() for k in ("v_means2d", "absgrad", "v_conics", "v_opacities")], axis=1)


# ---------------------------------------------------------------------------------------------------
# walk_of's integers (csrc/footprint_dev.h) in numpy fp32: what the host test shows the shear cases to contain
def walk_ints(rec, W, H):
    """per Gaussian: fw, fh (axis-aligned box inside the clips), pw (sheared width before the pw < fw switch); 0 where
    invisible.  fp32 arithmetic with numpy's log / sqrt (the integers may differ from the device's on a rounding edge;
    the host test only asks that every class occurs)."""
    f = np.float32
    j0b, i0b, j1b, i1b = pixel_boxes(rec, W, H)
    x, y, a, b, c, o = (rec[:, k].astype(f) for k in range(6))
    with np.errstate(all="ignore"):
        thr = np.log(f(255.0) * o).astype(f) + f(1e-3)
        det = a * c - b * b
        k = f(2.0) * thr / det
        ex = np.sqrt(k * c) * f(1.001) + f(0.01)
        ey = np.sqrt(k * a) * f(1.001) + f(0.01)
        hw = np.sqrt(f(2.0) * thr / a) * f(1.001) + f(0.01)
        ok = _visible(rec) & (thr > 0)
        ex, ey, hw = (np.where(ok, t, 0) for t in (ex, ey, hw))
        j0 = np.maximum(j0b, np.ceil(x - ex - f(0.5)).astype(np.int64))
        j1 = np.minimum(j1b - 1, np.floor(x + ex - f(0.5)).astype(np.int64))
        i0 = np.maximum(i0b, np.ceil(y - ey - f(0.5)).astype(np.int64))
        i1 = np.minimum(i1b - 1, np.floor(y + ey - f(0.5)).astype(np.int64))
    fw, fh = j1 - j0 + 1, i1 - i0 + 1
    live = ok & (fw > 0) & (fh > 0)
    pw = (f(2.0) * hw).astype(np.int64) + 1
    return np.where(live, fw, 0), np.where(live, fh, 0), np.where(live, pw, 0)


# ---------------------------------------------------------------------------------------------------
# records of the footprint cases
def ellipse_records(xy, s_major, ratio, theta, op, depths, radii=None):
    """records from centres, major sigma, axis ratio, angle: conic = inverse covariance, radius = ceil(3 sigma_major)"""
    xy, s_major, ratio, theta = (np.asarray(t, np.float64) for t in (xy, s_major, ratio, theta))
    s_minor = s_major / ratio
    c, s = np.cos(theta), np.sin(theta)
    cxx = c * c * s_major ** 2 + s * s * s_minor ** 2
    cyy = s * s * s_major ** 2 + c * c * s_minor ** 2
    cxy = c * s * (s_major ** 2 - s_minor ** 2)
    det = cxx * cyy - cxy * cxy
    conics = np.stack([cyy / det, -cxy / det, cxx / det], axis=1)
    radii = np.ceil(3.0 * s_major).astype(np.int32) if radii is None else np.asarray(radii, np.int32)
    return CU.pack_records(xy, conics, op, depths, radii)


def random_records(n, seed, W, H, sigma=(0.8, 5.0), opacity_lo=0.01, capped_share=0.05, tie_every=7):
    """CU.make_records' recipe on a W x H image: centres U over the image + 6 px, axis ratio 1 .. 4, opacity log-uniform
    in opacity_lo .. 0.95 with `capped_share` beyond the 0.999 cap, every tie_every-th depth bit-equal to the first"""
    g = np.random.default_rng(seed)
    xy = np.stack([g.uniform(-6.0, W + 6.0, n), g.uniform(-6.0, H + 6.0, n)], axis=1)
    op = np.exp(g.uniform(math.log(opacity_lo), math.log(0.95), n))
    op = np.where(g.uniform(0.0, 1.0, n) < capped_share, g.uniform(0.9992, 1.0, n), op)
    depths = g.uniform(0.5, 5.0, n)
    depths[::tie_every] = depths[0]
    return ellipse_records(xy, g.uniform(sigma[0], sigma[1], n), g.uniform(1.0, 4.0, n), g.uniform(0.0, math.pi, n), op, depths)


DEAD_KINDS = ("radius0", "faint", "det", "off_image", "box_on_ellipse_off")


def dead_records(n, seed, W, H):
    """n rows no pixel counts for, cycling through DEAD_KINDS: radius 0; o < 1/255; det <= 0; entirely off-image; tile
    box on-image but the ellipse off-image (a small Gaussian 14 px left of the image with a radius of 16)"""
    rec = random_records(n, seed, W, H, sigma=(1.0, 3.0), capped_share=0.0)
    rec[:, 0] = np.clip(rec[:, 0], 8.0, W - 8.0)
    rec[:, 1] = np.clip(rec[:, 1], 8.0, H - 8.0)
    for k in range(n):
        kind = DEAD_KINDS[k % len(DEAD_KINDS)]
        if kind == "radius0":
            rec[k, 7] = np.int32(0).view(np.float32)
        elif kind == "faint":
            rec[k, 5] = 0.0035
        elif kind == "det":
            rec[k, 3] = 1.5 * math.sqrt(rec[k, 2] * rec[k, 4])
        elif kind == "off_image":
            rec[k, 0] = W + 200.0
        else:
            rec[k, 0:2] = (-14.0, 20.0)
            rec[k, 2:5] = (4.0, 0.0, 4.0)
            rec[k, 7] = np.int32(16).view(np.float32)
    return rec


def mix_wave(pos, seed, W, H):
    """eight rows: one footprint covering the whole image at position `pos`, seven of about one pixel"""
    g = np.random.default_rng(seed)
    xy = np.stack([g.uniform(2.0, W - 2.0, 8), g.uniform(2.0, H - 2.0, 8)], axis=1)
    s = np.full(8, 0.35)
    op = g.uniform(0.3, 0.9, 8)
    xy[pos], s[pos], op[pos] = (W / 2 + 0.3, H / 2 - 0.2), 60.0, 0.7
    return ellipse_records(xy, s, np.ones(8), np.zeros(8), op, g.uniform(0.5, 5.0, 8))


def shear_records(W, H):
    """thin Gaussians (axis ratio about 30) at 0, +-10, +-45, +-80, 90 degrees and a sweep of small tilts (where the
    sheared width passes the axis-aligned one: pw == fw - 1, fw, fw + 1); centres on pixel centres, on pixel corners
    and +-1e-3 off both; minor sigmas 0.12 .. 0.5 (pw odd and even); plus rows cut by each image edge and rows whose
    radius (2) ends the tile box inside a wide ellipse"""
    angles = [0.0, 10.0, -10.0, 45.0, -45.0, 80.0, -80.0, 90.0] + [0.25 * k for k in range(1, 13)] + [90.0 - 0.5 * k for k in range(1, 7)]
    fracs = [0.5, 0.0, 0.5 + 1e-3, 0.5 - 1e-3, 1e-3, -1e-3]
    rows = []
    k = 0
    for ang in angles:
        for fr in fracs:
            for s_minor in (0.12, 0.2, 0.31, 0.5):
                cx, cy = 20.0 + 5.0 * (k % 7) + fr, 12.0 + 3.0 * (k % 5) + fr
                rows.append((cx, cy, 30.0 * s_minor, 30.0, math.radians(ang), 0.35 + 0.08 * (k % 7), 0.5 + 0.01 * k, None))
                k += 1
    for cx, cy in ((0.7, 20.2), (W - 0.4, 11.5), (30.3, 0.2), (41.5, H - 0.6), (-2.5, -1.5), (W + 3.0, H + 2.0)):
        for ang in (20.0, -70.0):
            rows.append((cx, cy, 7.0, 12.0, math.radians(ang), 0.6, 0.5 + 0.01 * k, None))
            k += 1
    for cx, cy in ((24.0, 24.0), (33.7, 9.2), (47.9, 16.1), (16.0, 31.9)):
        rows.append((cx, cy, 9.0, 3.0, math.radians(35.0), 0.8, 0.5 + 0.01 * k, 2))
        k += 1
    xy = np.array([(r[0], r[1]) for r in rows])
    s_major, ratio, th, op, dep = (np.array([r[i] for r in rows]) for i in range(2, 7))
    rec = ellipse_records(xy, s_major, ratio, th, op, dep)
    for i, r in enumerate(rows):
        if r[7] is not None:
            rec[i, 7] = np.int32(r[7]).view(np.float32)
    return rec


GRAZE_QUADRANTS = (   # (quadrant origin, which of its corners, k, side): eight thin diagonals with disjoint supports on CU.W x CU.H
    ((8, 8), (0, 0), 2, -1), ((24, 8), (0, 0), 2, 1), ((32, 8), (1, 0), 3, -1), ((8, 16), (0, 1), 3, 1),
    ((16, 16), (1, 1), 4, -1), ((32, 16), (1, 1), 4, 1), ((16, 8), (0, 1), 5, -1), ((32, 8), (0, 1), 5, 1))


def grazing_quadrant_records():
    """The quadrant cull's grazing case (quad_hit / quad_hit_staged / hitq[] of the compositing kernels): thin diagonal
    ellipses (sigmas 2 and 0.5 px) whose flank touches an 8 x 8 quadrant only at a corner pixel centre, the float64 alpha
    there (1/255)(1 - side 10^-k) ... i.e. side -1: just visible, side +1: just invisible.  o is solved at the record
    level, from the fp32 record's own sigma at that pixel.  The supports are disjoint (asserted by
    tests/test_cull_host.py), so the alpha image is the single Gaussian's alpha."""
    rows = []
    for (qx, qy), (cx, cy), _k, _side in GRAZE_QUADRANTS:
        px, py = qx + 0.5 + 7.0 * cx, qy + 0.5 + 7.0 * cy
        nx, ny = (1.0 if cx else -1.0) * math.sqrt(0.5), (1.0 if cy else -1.0) * math.sqrt(0.5)
        rows.append((px + 1.12 * nx, py + 1.12 * ny, math.atan2(nx, -ny)))   # the major axis is perpendicular to the approach
    n = len(rows)
    rec = ellipse_records(np.array([(r[0], r[1]) for r in rows]), np.full(n, 2.0), np.full(n, 4.0), np.array([r[2] for r in rows]),
                          np.full(n, 0.5), 1.0 + 0.1 * np.arange(n))
    for i, ((qx, qy), (cx, cy), k, side) in enumerate(GRAZE_QUADRANTS):
        x, y, a, b, c = (float(v) for v in rec[i, 0:5])
        dx, dy = x - (qx + 0.5 + 7.0 * cx), y - (qy + 0.5 + 7.0 * cy)
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        rec[i, 5] = np.float32(math.exp(sigma) * (1.0 - side * 10.0 ** -k) / 255.0)
    return rec


def single_alphas(rec, W, H):
    """float64 [N, H, W]: o exp(-sigma) of every Gaussian on its own, uncapped"""
    p = np.asarray(rec[:, 0:6], np.float64)
    dx = p[:, 0, None, None] - (np.arange(W) + 0.5)[None, None, :]
    dy = p[:, 1, None, None] - (np.arange(H) + 0.5)[None, :, None]
    sigma = 0.5 * (p[:, 2, None, None] * dx * dx + p[:, 4, None, None] * dy * dy) + p[:, 3, None, None] * dx * dy
    return p[:, 5, None, None] * np.exp(-sigma)


def stop_records(W, H):
    """48 rows.  Wave 0-1: ordinary Gaussians with twins at bit-equal depth (rows 0 / 5 / 11 share one depth, 2 / 9
    another) and rows one ulp either side of row 5's depth (rows 6, 7).  Wave 2: depths no record ever names (the
    wave-uniform tie branch is not taken there).  Wave 3: o > 0.999 mixed with ordinary rows.  Wave 4: o > 0.999 alone.
    Wave 5: ordinary rows again."""
    rec = random_records(48, 5, W, H, sigma=(4.0, 14.0), opacity_lo=0.05, capped_share=0.0, tie_every=1000)
    rec[:, 0] = np.clip(rec[:, 0], 4.0, W - 4.0)
    rec[:, 1] = np.clip(rec[:, 1], 4.0, H - 4.0)
    d = rec[:, 6].copy()
    d[[5, 11]] = d[0]
    d[9] = d[2]
    d[6] = np.nextafter(d[5], np.float32(10.0))
    d[7] = np.nextafter(d[5], np.float32(0.0))
    d[16:24] = np.float32(7.0) + np.arange(8, dtype=np.float32) * np.float32(0.125)   # never a stop: see stop_image
    rec[:, 6] = d
    g = np.random.default_rng(9)
    rec[[24, 27, 29], 5] = g.uniform(0.9992, 1.0, 3).astype(np.float32)
    rec[32:40, 5] = g.uniform(0.9992, 1.0, 8).astype(np.float32)
    return rec


def random_image(rec, W, H, seed, stop_ids=None, zero_share=0.2, stop_share=0.1, special=False, one_sign=False):
    """RecImg: gT a smooth field of both signs in (-1, 1) (periods 29 .. 71 px; per-pixel random signs would make every
    row a cancelling sum, loose by construction) rounded to fp32, exact zeros on `zero_share` of the 4 x 4 blocks, stops on `stop_share` of the pixels
    (stop id drawn from stop_ids, default all rows; stop_depth = the depth bits of splat[stop_id]).  special: -0.0 and
    fp32 denormals of both signs on some pixels, in 4 x 4 blocks (so that some small footprint sees nothing else).
    one_sign: per-pixel random positive gT instead of the field (a mix-up of neighbouring pixels shows in every row)."""
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    ph = g.uniform(0.0, 2.0 * math.pi, 4)
    field = (np.sin(2.0 * math.pi * xx / 37.0 + ph[0]) * np.cos(2.0 * math.pi * yy / 29.0 + ph[1])
             + 0.5 * np.sin(2.0 * math.pi * (xx + yy) / 53.0 + ph[2]) + 0.3 * np.cos(2.0 * math.pi * (xx - 2.0 * yy) / 71.0 + ph[3]))
    gT = (field / 1.8).astype(np.float32)
    if one_sign:   # per-pixel random magnitudes U(0.2, 1) of ONE sign: no cancellation, and no two neighbours alike
        gT = g.uniform(0.2, 1.0, (H, W)).astype(np.float32)
    zb = g.uniform(0, 1, ((H + 3) // 4, (W + 3) // 4)) < zero_share
    gT[np.kron(zb, np.ones((4, 4), bool))[:H, :W]] = 0.0
    if special:
        blocks = g.integers(0, 4, ((H + 3) // 4, (W + 3) // 4))
        kind = np.kron(blocks, np.ones((4, 4), np.int64))[:H, :W]
        sign = np.where(g.uniform(0, 1, (H, W)) < 0.5, -1.0, 1.0).astype(np.float32)
        gT = np.where(kind == 1, np.float32(-0.0), gT)
        gT = np.where(kind == 2, sign * np.float32(3e-40), gT).astype(np.float32)
    ids = np.arange(rec.shape[0]) if stop_ids is None else np.asarray(stop_ids)
    sid = np.where(g.uniform(0, 1, (H, W)) < stop_share, ids[g.integers(0, ids.size, (H, W))], -1).astype(np.int64)
    sd = np.where(sid >= 0, depth_bits(rec)[np.maximum(sid, 0)], NO_STOP_DEPTH)
    return RecImg(gT.astype(np.float64), sid, sd)


FOOTPRINT_SIZES = (1, 7, 8, 9, 31, 32, 33, 255, 257)
FOOTPRINT_CASES = tuple(f"n{n}" for n in FOOTPRINT_SIZES) + ("n257_onesign", "mix", "shear", "stops", "large")
FpCase = collections.namedtuple("FpCase", "name rec W H img mask ref kappa")


@functools.lru_cache(maxsize=None)
def footprint_case(name):
    """records + record image (gT zero on the borderline pixels) + float64 reference + kappa of one case of the
    footprint backward -- computed once, shared, never modified"""
    W, H = FP_W, FP_H
    if name.startswith("n"):
        n = int(name[1:].split("_")[0])
        rec = random_records(n, 100 + n, W, H)
        if n == 1:
            rec[0, 0:2] = (30.3, 17.8)
        img = random_image(rec, W, H, 200 + n, one_sign=name.endswith("_onesign"))
    elif name == "mix":
        waves = []
        for pos in range(8):
            waves += [mix_wave(pos, 300 + pos, W, H), dead_records(8, 320 + pos, W, H), mix_wave(7 - pos, 340 + pos, W, H)]
        rec = np.concatenate(waves)
        img = random_image(rec, W, H, 360, stop_share=0.05)
    elif name == "shear":
        rec = shear_records(W, H)
        img = random_image(rec, W, H, 400, zero_share=0.1, stop_share=0.05)
    elif name == "stops":
        rec = stop_records(W, H)
        ids = np.concatenate([np.arange(0, 16), np.arange(24, 48)])         # wave 2's depths are never named
        img = random_image(rec, W, H, 500, stop_ids=ids, stop_share=0.6, special=True)
    elif name == "large":
        W, H = BIG_W, BIG_H
        small = random_records(8, 600, W, H, sigma=(0.8, 3.0), capped_share=0.0)
        small[:, 0] = np.clip(small[:, 0], 8.0, W - 8.0)
        small[:, 1] = np.clip(small[:, 1], 8.0, H - 8.0)
        # (off the image's centre: about it the first moments cancel to 4e-4 of their terms, and an fp32 sum of 74 k terms
        # per lane in the kernel's lane order -- lane_order_model32 below -- is then 1.4e-3 off, as the device measured)
        big = ellipse_records([(0.3 * W + 0.25, 0.36 * H - 0.25)], [1500.0], [1.0], [0.0], [0.9], [2.0])
        rec = np.concatenate([small[:3], big, small[3:]])
        img = RecImg(np.full((H, W), float(np.float32(0.37))), np.full((H, W), -1, np.int64),
                     np.full((H, W), NO_STOP_DEPTH, np.int64))
    else:
        raise ValueError(name)
    mask = record_borderline(rec, W, H)
    img = masked(img, mask)
    ref, kappa = record_kappa(rec, img, W, H)
    return FpCase(name, rec, W, H, img, mask, ref, kappa)


# ---------------------------------------------------------------------------------------------------
# scenes of the forward: every Gaussian inside ONE tile, so that the lists' lengths are what the case names
FWD_LENGTHS = {"short": (127, 128, 1, 129, 255, 0), "long": (256, 257, 1100, 2300, 3100, 0)}
STOP_DEPTH = 7.0                  # mean optical depth of the stopping regimes (the stop is at ln 1e4 = 9.2)
FWD_REGIMES = ("nostop", "third", "quadrant")
FwdCase = collections.namedtuple("FwdCase", "name rec lst gt wmap loss_scale f mask")


def tile_records(lengths, regime, seed):
    """CU.W x CU.H (3 x 2 tiles, the right column and the bottom row partial).  Tile t gets lengths[t] Gaussians whose
    tile box is tile t alone (radius 3, centre at least 3 px inside the tile's left / top edge, the right / bottom
    neighbour reached only across the image's edge).  nostop: opacity about 0.08 and sub-pixel sigmas, no pixel stops.
    third: the opacity grows with the list so that about a third of the pixels stop.  quadrant: `third`, and in the
    longest tile 14 near-opaque wide Gaussians at the front saturate the top-left quadrant inside the first slice."""
    g = np.random.default_rng(seed)
    tw, th = tiles_of(CU.W, CU.H)
    parts = []
    longest = int(np.argmax(lengths))
    for t, n in enumerate(lengths):
        if n == 0:
            continue
        ty, tx = divmod(t, tw)
        x_hi = 13.0 if tx < tw - 1 else CU.W - 16.0 * tx
        y_hi = 13.0 if ty < th - 1 else CU.H - 16.0 * ty
        xy = np.stack([16.0 * tx + g.uniform(3.0, x_hi, n), 16.0 * ty + g.uniform(3.0, y_hi, n)], axis=1)
        ratio = g.uniform(1.0, 3.0, n)
        if regime == "nostop":
            s, op = g.uniform(0.35, 0.8, n), g.uniform(0.06, 0.1, n)
        else:  # mean optical depth STOP_DEPTH per pixel: the integral of o exp(-sigma) is 2 pi o s_major s_minor
            s = g.uniform(0.7, 1.3, n) * min(4.0, max(0.6, 8.0 / math.sqrt(n / 8.0)))
            op = np.minimum(0.95, STOP_DEPTH * g.uniform(0.5, 1.5, n) * 256.0 / (n * 2.0 * math.pi * s * s / ratio))
        depths = g.uniform(1.0, 5.0, n)
        depths[::7] = depths[0]
        r = ellipse_records(xy, s, ratio, g.uniform(0.0, math.pi, n), op, depths, radii=np.full(n, 3))
        if regime == "quadrant" and t == longest:
            k = 14
            r[:k] = ellipse_records(np.stack([16.0 * tx + g.uniform(3.5, 4.5, k), 16.0 * ty + g.uniform(3.5, 4.5, k)], axis=1),
                                    np.full(k, 6.0), np.ones(k), np.zeros(k), np.full(k, 0.9), g.uniform(0.1, 0.2, k),
                                    radii=np.full(k, 3))
        parts.append(r)
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def forward_case(lengths_name, regime, with_loss=True):
    """records, lists, gt in {0, 1} and random values, a weight map, the float64 forward and the borderline mask (the
    weight map is zero on it) -- computed once, shared, never modified"""
    name = f"{lengths_name}-{regime}"
    if lengths_name == "grazing":   # (regime "nostop": eight Gaussians, no pixel stops)
        rec = grazing_quadrant_records()
    else:
        rec = tile_records(FWD_LENGTHS[lengths_name], regime, 700 + 10 * FWD_REGIMES.index(regime) + len(lengths_name))
    lst = lists_of(rec, CU.W, CU.H)
    if not with_loss:
        f = ref_forward(rec, lst, CU.W, CU.H)
        return FwdCase(name, rec, lst, None, None, 1.0, f, forward_borderline(rec, lst, CU.W, CU.H))
    g = np.random.default_rng(800 + len(name))
    pick = g.integers(0, 3, (CU.H, CU.W))
    gt = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, g.uniform(0.0, 1.0, (CU.H, CU.W)))).astype(np.float32)
    wmap = g.uniform(0.2, 2.0, (CU.H, CU.W)).astype(np.float32)
    loss_scale = 0.75
    f0 = ref_forward(rec, lst, CU.W, CU.H, gt, wmap, loss_scale)
    mask = forward_borderline(rec, lst, CU.W, CU.H, f0, gt)
    wmap = np.where(mask, np.float32(0.0), wmap)
    return FwdCase(name, rec, lst, gt, wmap, loss_scale, ref_forward(rec, lst, CU.W, CU.H, gt, wmap, loss_scale), mask)


def segment_tables(lst, seg_cap, seed=0):
    """Hand-built segmented tables of the classic lists `lst`: tile t's ids sit at a gap of 1 .. 5 unused slots (-1)
    into its own segment of seg_cap slots, the tiles' segments in a SHUFFLED order, so that no two lists are adjacent;
    empty tiles own an empty segment and one empty item.  Returns dict(tile_start, tile_end, item_first, item_end,
    item_tile, flat, n_items, pos: classic list index -> slot)."""
    g = np.random.default_rng(seed)
    T = len(lst.offsets) - 1
    lens = np.diff(lst.offsets)
    assert int(lens.max()) + 5 <= seg_cap
    order = g.permutation(T)
    flat = np.full(T * seg_cap, -1, np.int32)
    start, end = np.zeros(T, np.int32), np.zeros(T, np.int32)
    pos = np.zeros(max(int(lst.offsets[-1]), 1), np.int64)
    for slot, t in enumerate(order):
        s = slot * seg_cap + int(g.integers(1, 6))
        start[t], end[t] = s, s + lens[t]
        flat[s:s + lens[t]] = lst.flat[lst.offsets[t]:lst.offsets[t + 1]]
        pos[lst.offsets[t]:lst.offsets[t + 1]] = np.arange(s, s + lens[t])
    items = np.maximum(1, (lens + 127) // 128)
    item_end = np.cumsum(items).astype(np.int32)
    item_first = (item_end - items).astype(np.int32)
    item_tile = np.repeat(np.arange(T, dtype=np.int32), items)
    return dict(tile_start=start, tile_end=end, item_first=item_first, item_end=item_end, item_tile=item_tile, flat=flat,
                n_items=int(item_end[-1]), pos=pos)


# ---------------------------------------------------------------------------------------------------
# the fp32 model of the forward's transmittance
def model32_T(rec, lst, f, W, H, slice_len=128):
    """(T of one running fp32 product front to back [H, W], T as the fp32 product of the fp32 products of the
    `slice_len`-Gaussian slices [H, W]) with numpy's fp32 exponential, over the contributions the float64 walk `f`
    found (the borderline pixels, where fp32 may decide otherwise, are outside every comparison)"""
    fl = np.float32
    tw, th = tiles_of(W, H)
    seq, sl = np.ones((H, W), fl), np.ones((H, W), fl)
    offs = np.asarray(lst.offsets, np.int64)
    for t in range(tw * th):
        g = lst.flat[offs[t]:offs[t + 1]]
        if g.size == 0:
            continue
        ty, tx = divmod(t, tw)
        ii, jj = np.meshgrid(np.arange(ty * TS, min(ty * TS + TS, H)), np.arange(tx * TS, min(tx * TS + TS, W)), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        dx = rec[g, 0][None, :] - (jj[:, None].astype(fl) + fl(0.5))
        dy = rec[g, 1][None, :] - (ii[:, None].astype(fl) + fl(0.5))
        sigma = fl(0.5) * (rec[g, 2] * dx * dx + rec[g, 4] * dy * dy) + rec[g, 3] * dx * dy
        alpha = np.minimum(fl(AMAX), rec[g, 5][None, :] * np.exp(-sigma))
        last = f.last_idx[ii, jj] - offs[t]                                  # -1 - offs: nothing contributes
        contrib = (sigma >= 0) & (alpha >= fl(AMIN)) & (np.arange(g.size)[None, :] <= last[:, None])
        one_m = np.where(contrib, fl(1) - alpha, fl(1)).astype(fl)
        seq[ii, jj] = np.cumprod(one_m, axis=1, dtype=fl)[:, -1]
        acc = np.ones(ii.size, fl)
        for s in range(0, g.size, slice_len):
            acc = acc * np.cumprod(one_m[:, s:s + slice_len], axis=1, dtype=fl)[:, -1]
        sl[ii, jj] = acc
    return seq, sl


def d32_of(rec, lst, f, mask, W, H):
    """worst relative deviation of the fp32 model's T (either order) from the float64 T over the kept, touched pixels"""
    seq, sl = model32_T(rec, lst, f, W, H)
    keep = ~mask & (f.last_idx >= 0)
    if not keep.any():
        return 0.0
    dev = np.maximum(np.abs(seq.astype(np.float64) - f.T), np.abs(sl.astype(np.float64) - f.T)) / f.T
    return float(dev[keep].max())


# ---------------------------------------------------------------------------------------------------
# the per-pixel check of a device record image
def record_check(words, rec, f, mask, tol, name, empty=None):
    """words: a device's [H, W, 3] int32 record image; f: the float64 forward; mask: the borderline pixels; empty: bool
    [H, W] of pixels the call does not write (tiles it leaves out), excluded.  Asserts: stop_depth BIT-EQUAL to
    splat[stop_id]'s depth (0xffffffff without a stop) on every pixel; stop_id exact and gT within `tol` (relative, per
    pixel; exactly 0 where the reference is 0) outside the mask.  Returns the largest relative gT deviation."""
    img = image_of_words(words)
    look = np.ones(mask.shape, bool) if empty is None else ~empty
    want_depth = np.where(img.stop_id >= 0, depth_bits(rec)[np.clip(img.stop_id, 0, rec.shape[0] - 1)], NO_STOP_DEPTH)
    bad = look & (img.stop_depth != want_depth)
    assert not bad.any(), f"{name}: stop_depth is not the depth bits of splat[stop_id] on {int(bad.sum())} pixels, first {np.argwhere(bad)[0].tolist()}"
    keep = look & ~mask
    bad = keep & (img.stop_id != f.stop_id)
    assert not bad.any(), f"{name}: stop_id differs on {int(bad.sum())} kept pixels, first {np.argwhere(bad)[0].tolist()}"
    zero = keep & (f.gT == 0)
    assert not (img.gT[zero] != 0).any(), f"{name}: gT is not exactly 0 on {int((img.gT[zero] != 0).sum())} pixels where the reference is"
    live = keep & (f.gT != 0)
    dev = np.abs(img.gT - f.gT)[live] / np.abs(f.gT[live])
    worst = float(dev.max(initial=0.0))
    assert worst <= tol, f"{name}: gT off by {worst:.2e} relative on a kept pixel (allowed {tol:.2e})"
    return worst


def swapped_slice_record(rec, lst, W, H, y, x, f, k, slice_len=128):
    """The PLANTED defect 'two slice products folded in swapped order': pixel (y, x)'s float64 walk with the slices k and
    k + 1 of its tile's list visited in swapped order (k + 1 first), the stop rule applied along the way.  Returns
    (gT, stop_id) as a forward with that defect would record them (v is the reference's)."""
    tw, _th = tiles_of(W, H)
    t = (y // TS) * tw + x // TS
    g = lst.flat[lst.offsets[t]:lst.offsets[t + 1]]
    order = np.arange(g.size)
    a, b, c = k * slice_len, (k + 1) * slice_len, min((k + 2) * slice_len, g.size)
    order = np.concatenate([order[:a], order[b:c], order[a:b], order[c:]])
    p = np.asarray(rec[g[order], 0:6], np.float64)
    dx, dy = p[:, 0] - (x + 0.5), p[:, 1] - (y + 0.5)
    sigma = 0.5 * (p[:, 2] * dx * dx + p[:, 4] * dy * dy) + p[:, 3] * dx * dy
    alpha = np.minimum(AMAX, p[:, 5] * np.exp(-sigma))
    T, last, stopped = 1.0, -1, False
    for i in np.nonzero((sigma >= 0) & (alpha >= AMIN))[0]:
        nT = T * (1.0 - alpha[i])
        if nT <= TSTOP:
            stopped = True
            break
        T, last = nT, i
    return f.v[y, x] * T, (int(g[order[last]]) if stopped else -1)


def lane_order_model32(rec, g, img, W, H, lanes):
    """fp32 model of the footprint kernel's accumulation for ONE Gaussian whose walk is the axis-aligned box of the whole
    image (W even): the float64 terms of the four first / second moments rounded to fp32, dealt to `lanes` lanes pair by
    pair (lane r takes the pairs r, r + lanes, ... of the row-major cells), every lane a running fp32 sum, the lanes'
    sums added in lane order.  Returns (model [vx, vy], float64 [vx, vy])."""
    x, y, a, b, c, o = np.asarray(rec[g, 0:6], np.float64)
    dx = x - (np.arange(W) + 0.5)[None, :]
    dy = y - (np.arange(H) + 0.5)[:, None]
    araw = o * np.exp(-(0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy))
    assert (araw >= AMIN).all() and (araw <= AMAX).all() and (img.stop_id < 0).all() and W % 2 == 0
    w = -araw * img.gT / (1.0 - araw)
    sums32, sums64 = [], []
    for term in (w * dx, w * dy):
        pairs = term.astype(np.float32).reshape(-1, 2)
        tot = np.float32(0.0)
        for r in range(lanes):
            tot = np.float32(tot + np.cumsum(pairs[r::lanes].reshape(-1), dtype=np.float32)[-1])
        sums32.append(float(tot))
        sums64.append(float(term.sum()))
    mix = lambda m: np.array([a * m[0] + b * m[1], b * m[0] + c * m[1]])   # noqa: E731
    return mix(sums32), mix(sums64)
