"""Host helpers of the per-(Gaussian, tile) tests of the training path's tile cull (tests/test_cull_host.py,
tests/test_gpu_tile_cull.py): tile_box_tight, ellipse_hits_rect and splat_hits_tile of csrc/common.h and their copies.
Nothing here needs a GPU.

Everything is evaluated FROM the fp32 records splat[N, 8] = x y a b c o depth radius-bits (projection is tested
elsewhere).  A pair is a (Gaussian, tile) couple, stored as the int64 key g * T + ty * tw + tx.

  references    three pair sets in float64
      box         gsplat's tile box from (x, y, radius): tile_box restated in numpy float32, decision-identical
      must_keep   box pairs where one of the tile's 256 pixel centres has o exp(-sigma64) >= 1/255 (the centres past the
                  image's edge in a partial tile included: that only enlarges the set).  Rows no projection produces
                  (radius <= 0, a <= 0, det <= 0, o <= 0) are invisible by the kernels' contract and own no pair.
      may_keep    box pairs with thr64 = ln(255 o) + 1e-3 > 0, det > 0, the tile inside the extent box (the kernel's 1.001
                  and 0.01, plus a few ulps of the coordinates) and the float64 minimum of sigma over the tile's
                  pixel-centre rectangle <= 1.001 thr64 + 1e-3 + band
  model32       tile_box_tight + splat_hits_tile in numpy float32 (every operation rounded on its own, IEEE division for
                the hardware reciprocal): the kept pairs and the mask word; takes the MUTANTS of the host test
  check_*       the assertions both test files apply

band.  The fp32 allowance of one pair is BAND_FACTOR 2^-24 (0.5 |a| dx^2 + 0.5 |c| dy^2 + |b dx dy|) with (dx, dy) the
rectangle corner farthest from the centre.  Counting the roundings of one sigma_at evaluation behind its largest term
(two subtractions forming dx / dy, the clamp's product and reciprocal, three products, two sums and the final sum: at
most 11 half-ulp roundings of a term no larger than the sum above, i.e. 5.5 units of 2^-24) plus one ulp each for the
hardware rcp, sqrt and log gives 8.5 if every rounding pulls the same way.  That first value (with a factor two in hand,
16) proved needlessly large: model32 keeps every pair of `thin` (4000 Gaussians, 200 x 136) and of `grazing` inside
may_keep with a factor of 0.089 -- the terms are bounded at the FARTHEST corner, the minimum is evaluated at the nearest
edge, and eleven roundings of either sign add up to about one unit, not 5.5.  BAND_FACTOR = 4 keeps a factor 45 over what
the model needs (tests/test_cull_host.py::test_band_is_what_the_model_needs states the need and asserts it is at most half
the factor).  The model decides this, never a kernel; what the device needed is recorded next to its figures.
"""
import collections
import functools
import math

import numpy as np

TS = 16
F = np.float32
AMIN = 1.0 / 255.0
BAND_FACTOR = 4.0
SHARE_CAP = 0.03
FOCAL = 1024.0
EPS2D = 0.3
FOV_CLAMP = 1.3
ALL_ONES = 0xFFFFFFFF
MUTANTS = ("noslack", "x1_no_plus1", "rect16", "mask_bh", "small31", "edge_sign")


def tiles_of(W, H):
    return (W + TS - 1) // TS, (H + TS - 1) // TS


def radius_of(rec):
    return np.ascontiguousarray(rec[:, 7]).view(np.int32).astype(np.int64)


def _to_int(v, lo, hi):
    return np.clip(np.nan_to_num(v, nan=0.0, posinf=1e9, neginf=-1e9), lo, hi).astype(np.int64)


def tile_box32(rec, tw, th):
    """x0, y0, x1, y1 (exclusive ends) of every row: csrc/common.h tile_box in float32 -- (c / 16) -+ (r / 16), floor /
    ceil, clamp to the grid; an empty box on rows with radius <= 0"""
    x, y = rec[:, 0].astype(F), rec[:, 1].astype(F)
    r = radius_of(rec)
    ts = F(TS)
    with np.errstate(all="ignore"):
        tr = r.astype(F) / ts
        tx, ty = x / ts, y / ts
        x0, y0 = _to_int(np.floor(tx - tr), 0, tw), _to_int(np.floor(ty - tr), 0, th)
        x1, y1 = _to_int(np.ceil(tx + tr), 0, tw), _to_int(np.ceil(ty + tr), 0, th)
    live = r > 0
    return tuple(np.where(live, v, 0) for v in (x0, y0, x1, y1))


def expand(x0, y0, x1, y1):
    """(g, tx, ty) of every tile of every box, row-major inside a box, rows ascending"""
    w, h = np.maximum(x1 - x0, 0), np.maximum(y1 - y0, 0)
    n = np.where((w > 0) & (h > 0), w * h, 0)
    g = np.repeat(np.arange(n.size), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    return g, x0[g] + k % np.maximum(w[g], 1), y0[g] + k // np.maximum(w[g], 1)


def keys_of(g, tx, ty, tw, th):
    return g.astype(np.int64) * (tw * th) + ty * tw + tx


def split_keys(keys, tw, th):
    keys = np.asarray(keys, np.int64)
    g, t = keys // (tw * th), keys % (tw * th)
    return g, t % tw, t // tw


# ---------------------------------------------------------------------------------------------------
# float64 references
Refs = collections.namedtuple("Refs", "W H tw th N g tx ty key must may rmin thr band box_xyxy")


def rect_min64(p, g, tx, ty):
    """float64 minimum of sigma over the pixel-centre rectangle of tile (tx, ty) for rows g of p = [x y a b c o]: 0 with the
    centre inside, else the least of the four clamped edge minimisers.  Also the farthest-corner offsets (dx, dy)."""
    x, y, a, b, c = (p[g, k] for k in range(5))
    u0, u1 = TS * tx + 0.5 - x, TS * tx + 15.5 - x
    v0, v1 = TS * ty + 0.5 - y, TS * ty + 15.5 - y
    sig = lambda dx, dy: 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy   # noqa: E731
    with np.errstate(all="ignore"):
        us0, us1 = np.clip(-b * v0 / a, u0, u1), np.clip(-b * v1 / a, u0, u1)
        vs0, vs1 = np.clip(-b * u0 / c, v0, v1), np.clip(-b * u1 / c, v0, v1)
        m = np.minimum(np.minimum(sig(us0, v0), sig(us1, v1)), np.minimum(sig(u0, vs0), sig(u1, vs1)))
    inside = (u0 <= 0) & (u1 >= 0) & (v0 <= 0) & (v1 >= 0)
    return np.where(inside, 0.0, m), np.maximum(np.abs(u0), np.abs(u1)), np.maximum(np.abs(v0), np.abs(v1))


def references(rec, W, H, band_factor=BAND_FACTOR):
    rec = np.ascontiguousarray(rec, np.float32)
    tw, th = tiles_of(W, H)
    N = rec.shape[0]
    box = tile_box32(rec, tw, th)
    g, tx, ty = expand(*box)
    p = rec[:, 0:6].astype(np.float64)
    x, y, a, b, c, o = p.T
    r = radius_of(rec)
    det = a * c - b * b
    visible = (r > 0) & (a > 0) & (det > 0) & (o > 0)
    # must_keep: all 256 centres of every box pair
    must = np.zeros(g.size, bool)
    off = np.arange(TS) + 0.5
    for s in range(0, g.size, 16384):
        gg = g[s:s + 16384]
        dx = (TS * tx[s:s + 16384, None] + off[None, :] - x[gg, None])[:, None, :]
        dy = (TS * ty[s:s + 16384, None] + off[None, :] - y[gg, None])[:, :, None]
        sigma = 0.5 * (a[gg, None, None] * dx * dx + c[gg, None, None] * dy * dy) + b[gg, None, None] * dx * dy
        with np.errstate(all="ignore"):
            alpha = o[gg, None, None] * np.exp(-sigma)
        must[s:s + 16384] = visible[gg] & ((alpha >= AMIN) & (sigma >= 0)).any(axis=(1, 2))
    # may_keep
    with np.errstate(all="ignore"):
        thr = np.where(o > 0, np.log(255.0 * np.where(o > 0, o, 1.0)), -np.inf) + 1e-3
        ok = (r > 0) & (thr > 0) & (det > 0) & (a > 0)
        k2 = np.where(ok, 2.0 * thr / np.where(ok, det, 1.0), 0.0)
        ex = np.sqrt(k2 * np.where(ok, c, 0.0)) * 1.001 + 0.01
        ey = np.sqrt(k2 * np.where(ok, a, 0.0)) * 1.001 + 0.01
    ulps = 8.0 * 2.0 ** -24
    ax, ay = ulps * (np.abs(x) + ex + TS), ulps * (np.abs(y) + ey + TS)
    in_x = (x[g] - ex[g] - 15.5 <= TS * tx + ax[g]) & (TS * tx <= x[g] + ex[g] - 0.5 + ax[g])
    in_y = (y[g] - ey[g] - 15.5 <= TS * ty + ay[g]) & (TS * ty <= y[g] + ey[g] - 0.5 + ay[g])
    rmin, fx, fy = rect_min64(p, g, tx, ty)
    band = band_factor * 2.0 ** -24 * (0.5 * np.abs(a[g]) * fx * fx + 0.5 * np.abs(c[g]) * fy * fy + np.abs(b[g]) * fx * fy)
    with np.errstate(all="ignore"):
        may = ok[g] & in_x & in_y & (rmin <= 1.001 * thr[g] + 1e-3 + band)
    return Refs(W, H, tw, th, N, g, tx, ty, keys_of(g, tx, ty, tw, th), must, may, rmin, thr, band, box)


def needed_band_factor(refs, emitted):
    """the smallest BAND_FACTOR under which the emitted pairs (all inside gsplat's box) pass the rectangle test of may_keep"""
    e = np.asarray(emitted, np.int64)
    i = np.searchsorted(refs.key, e)
    over = refs.rmin[i] - (1.001 * refs.thr[refs.g[i]] + 1e-3)
    unit = refs.band[i] / BAND_FACTOR
    sel = over > 0
    with np.errstate(all="ignore"):
        return float((over[sel] / unit[sel]).max(initial=0.0))


def figures(refs, emitted=None):
    out = dict(box=int(refs.key.size), must_keep=int(refs.must.sum()), may_keep=int(refs.may.sum()),
               band_max=float(refs.band[refs.may].max(initial=0.0)))
    if emitted is not None:
        out["emitted"] = int(np.asarray(emitted).size)
    return out


def _describe(refs, rec, key):
    g, tx, ty = (int(v[0]) for v in split_keys([key], refs.tw, refs.th))
    i = np.searchsorted(refs.key, key)
    num = ""
    if i < refs.key.size and refs.key[i] == key:
        num = f", rect min {refs.rmin[i]:.9g}, thr64 {refs.thr[g]:.9g}, band {refs.band[i]:.3g}"
    return f"Gaussian {g} tile ({tx}, {ty}) record {rec[g, 0:6].tolist()}{num}"


def check_sets(refs, rec, emitted, name):
    """(1) must_keep <= emitted, no allowance; (2) emitted <= may_keep <= box, no pair twice.  Returns the figures."""
    e = np.asarray(emitted, np.int64)
    u = np.unique(e)
    assert u.size == e.size, f"{name}: {e.size - u.size} pairs were emitted twice"
    missing = np.setdiff1d(refs.key[refs.must], u)
    assert missing.size == 0, (f"{name}: {missing.size} must_keep pairs (a pixel centre with alpha >= 1/255) were dropped, first: "
                               + _describe(refs, rec, missing[0]))
    assert not (refs.must & ~refs.may).any(), f"{name}: the references disagree, must_keep is no subset of may_keep"
    extra = np.setdiff1d(u, refs.key[refs.may])
    assert extra.size == 0, (f"{name}: {extra.size} emitted pairs lie outside may_keep"
                             f" ({np.setdiff1d(u, refs.key).size} of them outside gsplat's box), first: " + _describe(refs, rec, extra[0]))
    return dict(figures(refs, u), needed_band_factor=needed_band_factor(refs, u))


def check_share(refs, name):
    """(3) the references alone: |may_keep \\ must_keep| <= 3 % of |must_keep|"""
    n_must, n_gap = int(refs.must.sum()), int((refs.may & ~refs.must).sum())
    assert n_must > 0 and n_gap <= SHARE_CAP * n_must, f"{name}: may_keep exceeds must_keep by {n_gap} pairs of {n_must}"
    return n_gap / n_must


def counts_of(emitted, N, tw, th):
    """tiles_per_gauss [N], tile populations [T] of a pair set"""
    g, tx, ty = split_keys(emitted, tw, th)
    return np.bincount(g, minlength=N).astype(np.int64), np.bincount(ty * tw + tx, minlength=tw * th).astype(np.int64)


def tight_box64(rec, tw, th, shift=(0, 0, 0, 0)):
    """The tight box of every row in float64 (x0, y0, x1, y1; empty as (x0, y0, x0, y0)), and `amb` [N, 4]: whether the
    bound's floor / ceil argument lies within a few fp32 ulps of an integer.  shift: -1 / 0 / +1 per bound moves an
    ambiguous argument across that integer (the candidates of check_mask)."""
    x0, y0, x1, y1 = tile_box32(rec, tw, th)
    p = rec[:, 0:6].astype(np.float64)
    x, y, a, b, c, o = p.T
    r = radius_of(rec)
    det = a * c - b * b
    with np.errstate(all="ignore"):
        thr = np.where(o > 0, np.log(255.0 * np.where(o > 0, o, 1.0)), -np.inf) + 1e-3
        ok = (r > 0) & (thr > 0) & (det > 0) & (a > 0)
        k2 = np.where(ok, 2.0 * thr / np.where(ok, det, 1.0), 0.0)
        ex = np.sqrt(k2 * np.where(ok, c, 0.0)) * 1.001 + 0.01
        ey = np.sqrt(k2 * np.where(ok, a, 0.0)) * 1.001 + 0.01
    args = [(x - ex - 15.5) / TS, (y - ey - 15.5) / TS, (x + ex - 0.5) / TS, (y + ey - 0.5) / TS]
    ext = [ex, ey, ex, ey]
    pos = [x, y, x, y]
    amb = np.zeros((rec.shape[0], 4), bool)
    vals = []
    for k in range(4):
        delta = 8.0 * 2.0 ** -24 * (np.abs(pos[k]) + ext[k] + TS) / TS + 1e-7
        amb[:, k] = np.abs(args[k] - np.round(args[k])) <= delta
        vals.append(np.where(amb[:, k], np.round(args[k]) + 0.5 * shift[k], args[k]))
    nx0 = np.maximum(x0, _to_int(np.ceil(vals[0]), -1e9, 1e9))
    ny0 = np.maximum(y0, _to_int(np.ceil(vals[1]), -1e9, 1e9))
    nx1 = np.minimum(x1, _to_int(np.floor(vals[2]), -1e9, 1e9) + 1)
    ny1 = np.minimum(y1, _to_int(np.floor(vals[3]), -1e9, 1e9) + 1)
    empty = ~ok | (nx1 <= nx0) | (ny1 <= ny0)
    nx0, ny0 = np.where(ok, nx0, x0), np.where(ok, ny0, y0)
    return (nx0, ny0, np.where(empty, nx0, nx1), np.where(empty, ny0, ny1)), amb & ok[:, None]


def mask_of(emitted, box, N, tw, th):
    """(the row-major bit mask of the emitted pairs inside `box` per row -- all ones on a box above 32 tiles, 0 on an empty
    one --, rows with an emitted pair outside their box)"""
    x0, y0, x1, y1 = box
    bw, area = x1 - x0, (x1 - x0) * (y1 - y0)
    g, tx, ty = split_keys(emitted, tw, th)
    inside = (tx >= x0[g]) & (tx < x1[g]) & (ty >= y0[g]) & (ty < y1[g])
    small = area[g] <= 32
    bit = np.where(inside & small, (ty - y0[g]) * bw[g] + tx - x0[g], 0)
    m = np.zeros(N, np.uint64)
    sel = inside & small
    np.add.at(m, g[sel], np.uint64(1) << bit[sel].astype(np.uint64))
    m = np.where(area > 32, np.uint64(ALL_ONES), m)
    bad = np.zeros(N, bool)
    bad[g[~inside]] = True
    return m, bad


def check_mask(rec, emitted, mask, W, H, name):
    """(4) tile_mask[g] == the row-major mask of the emitted pairs inside the tight box (<= 32 tiles), 0xffffffff above,
    0 on dead rows.  The tight box is the float64 one; a row one of whose four bounds sits within a few fp32 ulps of a
    tile border may match under either reading of that bound.  Returns the number of rows that needed the second reading."""
    import itertools
    tw, th = tiles_of(W, H)
    N = rec.shape[0]
    mask = np.asarray(mask).astype(np.int64) & ALL_ONES
    box, amb = tight_box64(rec, tw, th)
    want, bad = mask_of(emitted, box, N, tw, th)
    wrong = bad | (want.astype(np.int64) != mask)
    hard = wrong & ~amb.any(axis=1)
    assert not hard.any(), (f"{name}: tile_mask differs on {int(hard.sum())} rows, first row {int(np.argmax(hard))}: "
                            f"{int(mask[np.argmax(hard)]):#x} against {int(want[np.argmax(hard)]):#x}, tight box "
                            f"{[int(v[np.argmax(hard)]) for v in box]}")
    rows = np.nonzero(wrong)[0]
    if rows.size:
        sub = rec[rows]
        g_e, _tx, _ty = split_keys(emitted, tw, th)
        pos = np.searchsorted(rows, g_e)
        mine = (pos < rows.size) & (rows[np.minimum(pos, rows.size - 1)] == g_e)
        sub_e = keys_of(pos[mine], _tx[mine], _ty[mine], tw, th)
        solved = np.zeros(rows.size, bool)
        for shift in itertools.product((-1, 1), repeat=4):
            b2, _ = tight_box64(sub, tw, th, shift)
            w2, bad2 = mask_of(sub_e, b2, rows.size, tw, th)
            solved |= ~bad2 & (w2.astype(np.int64) == mask[rows])
        assert solved.all(), f"{name}: tile_mask of row {int(rows[np.argmin(solved)])} matches no reading of its tight box"
    return int(rows.size)


# ---------------------------------------------------------------------------------------------------
# the fp32 model
def model32(rec, W, H, mutant=None):
    """(kept pair keys ascending, mask word [N] uint64, tight box) of tile_box_tight + splat_hits_tile + the mask of
    project_fwd_kernel / emit_body in numpy float32.  mutant: one of MUTANTS, the planted defects of the host test."""
    assert mutant is None or mutant in MUTANTS
    rec = np.ascontiguousarray(rec, np.float32)
    tw, th = tiles_of(W, H)
    N = rec.shape[0]
    x, y, a, b, c, o = (np.ascontiguousarray(rec[:, k]) for k in range(6))
    r = radius_of(rec)
    x0, y0, x1, y1 = tile_box32(rec, tw, th)
    ts = F(TS)
    hi = F(16.0) if mutant == "rect16" else F(15.5)
    with np.errstate(all="ignore"):
        if mutant == "noslack":
            thr = np.log(F(255.0) * o) * F(0.99)
        else:
            thr = np.log(F(255.0) * o) + F(1e-3)
        det = a * c - b * b
        ok = (r > 0) & (thr > 0) & (det > 0)
        k2 = F(2.0) * thr * (F(1.0) / det)
        ex = np.sqrt(k2 * c) * F(1.001) + F(0.01)
        ey = np.sqrt(k2 * a) * F(1.001) + F(0.01)
        if mutant == "noslack":
            ex, ey = np.sqrt(k2 * c), np.sqrt(k2 * a)
        nx0 = np.maximum(x0, _to_int(np.ceil((x - ex - hi) / ts), -1e9, 1e9))
        ny0 = np.maximum(y0, _to_int(np.ceil((y - ey - hi) / ts), -1e9, 1e9))
        nx1 = np.minimum(x1, _to_int(np.floor((x + ex - F(0.5)) / ts), -1e9, 1e9) + (0 if mutant == "x1_no_plus1" else 1))
        ny1 = np.minimum(y1, _to_int(np.floor((y + ey - F(0.5)) / ts), -1e9, 1e9) + 1)
    empty = ~ok | (nx1 <= nx0) | (ny1 <= ny0)
    nx0, ny0 = np.where(ok, nx0, x0), np.where(ok, ny0, y0)
    nx1, ny1 = np.where(empty, nx0, nx1), np.where(empty, ny0, ny1)
    g, tx, ty = expand(nx0, ny0, nx1, ny1)
    X0, Y0 = (tx * TS).astype(F), (ty * TS).astype(F)
    xg, yg, ag, bg, cg, tg = x[g], y[g], a[g], b[g], c[g], thr[g]
    u0, u1 = (X0 + F(0.5)) - xg, (X0 + hi) - xg
    v0, v1 = (Y0 + F(0.5)) - yg, (Y0 + hi) - yg
    inside = (u0 <= 0) & (u1 >= 0) & (v0 <= 0) & (v1 >= 0)
    sig = lambda dx, dy, s=F(1.0): F(0.5) * (ag * dx * dx + cg * dy * dy) + s * bg * dx * dy   # noqa: E731
    with np.errstate(all="ignore"):
        nba, nbc = -bg * (F(1.0) / ag), -bg * (F(1.0) / cg)
        us0, us1 = np.minimum(np.maximum(nba * v0, u0), u1), np.minimum(np.maximum(nba * v1, u0), u1)
        vs0, vs1 = np.minimum(np.maximum(nbc * u0, v0), v1), np.minimum(np.maximum(nbc * u1, v0), v1)
        e4 = sig(u1, vs1, F(-1.0) if mutant == "edge_sign" else F(1.0))
        best = np.minimum(np.minimum(sig(us0, v0), sig(us1, v1)), np.minimum(sig(u0, vs0), e4))
        limit = tg if mutant == "noslack" else tg * F(1.001) + F(1e-3)
        hit = inside | (best <= limit)
    assert best.dtype == np.float32 and limit.dtype == np.float32
    # the mask word, as the kernels form it
    bw, bh = nx1 - nx0, ny1 - ny0
    area = bw * bh
    small = area <= (31 if mutant == "small31" else 32)
    stride = bh if mutant == "mask_bh" else bw
    bit = (ty - ny0[g]) * stride[g] + (tx - nx0[g])
    sel = hit & small[g]
    mask = np.zeros(N, np.uint64)
    np.bitwise_or.at(mask, g[sel], np.uint64(1) << (bit[sel] & 31).astype(np.uint64))
    mask = np.where((r > 0) & ~small, np.uint64(ALL_ONES), mask)
    return keys_of(g[hit], tx[hit], ty[hit], tw, th), mask, (nx0, ny0, nx1, ny1)


# ---------------------------------------------------------------------------------------------------
# cases, built in camera space: identity rotation, a Gaussian at depth z turned about the view axis, (long, thin, thin)
Params = collections.namedtuple("Params", "means quats log_scales logit_opacities viewmats Ks W H")
Case = collections.namedtuple("Case", "name params info")


def cameras(W, H, n_views=1):
    """identity rotation; view v is shifted by (0.011 v, -0.007 v, 0) in camera space"""
    vm = np.tile(np.eye(4, dtype=np.float32), (n_views, 1, 1))
    for v in range(n_views):
        vm[v, 0, 3], vm[v, 1, 3] = 0.011 * v, -0.007 * v
    K = np.tile(np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]], np.float32), (n_views, 1, 1))
    return vm, K


def params_of(xy, s_major, s_minor, theta, sig_op, depth, W, H, n_views=1):
    """screen centre (px), major / minor sigma (px, before eps2d), angle of the major axis, sigmoid(logit), depth"""
    xy, s_major, s_minor, theta, sig_op, z = (np.asarray(t, np.float64) for t in (xy, s_major, s_minor, theta, sig_op, depth))
    means = np.stack([(xy[:, 0] - W / 2) * z / FOCAL, (xy[:, 1] - H / 2) * z / FOCAL, z], axis=1)
    quats = np.stack([np.cos(theta / 2), np.zeros_like(theta), np.zeros_like(theta), np.sin(theta / 2)], axis=1)
    ls = np.log(np.stack([s_major, s_minor, s_minor], axis=1) * z[:, None] / FOCAL)
    sig_op = np.clip(sig_op, 1e-4, 0.999)
    logit = np.log(sig_op / (1.0 - sig_op))
    vm, K = cameras(W, H, n_views)
    f = lambda t: np.ascontiguousarray(t, np.float32)   # noqa: E731
    return Params(f(means), f(quats), f(ls), f(logit), vm, K, W, H)


def project64(p, view=0):
    """float64 restatement of forward_geom + radius_of (csrc/project_dev.h: pinhole, log-scales, logits, antialiased,
    eps2d 0.3, near 0.01) for the identity rotation of `cameras`: records [N, 8] float64 (radius as a number) and the
    compensation factor.  What the host test takes its records from; the GPU tests read the device's."""
    m = p.means.astype(np.float64) + p.viewmats[view, :3, 3].astype(np.float64)[None, :]
    q = p.quats.astype(np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    Rq = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                   2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    Wm = Rq * np.exp(p.log_scales.astype(np.float64))[:, None, :]
    fx, fy, cx, cy = (float(p.Ks[view][i]) for i in ((0, 0), (1, 1), (0, 2), (1, 2)))
    zc = m[:, 2]
    front = zc >= 0.01
    zs = np.where(front, zc, 1.0)
    lim_x, lim_y = FOV_CLAMP * 0.5 * p.W / fx, FOV_CLAMP * 0.5 * p.H / fy
    tx, ty = zs * np.clip(m[:, 0] / zs, -lim_x, lim_x), zs * np.clip(m[:, 1] / zs, -lim_y, lim_y)
    p0 = (fx / zs)[:, None] * Wm[:, 0, :] + (-fx * tx / zs ** 2)[:, None] * Wm[:, 2, :]
    p1 = (fy / zs)[:, None] * Wm[:, 1, :] + (-fy * ty / zs ** 2)[:, None] * Wm[:, 2, :]
    c00, c01, c11 = (p0 * p0).sum(1), (p0 * p1).sum(1), (p1 * p1).sum(1)
    det0 = c00 * c11 - c01 * c01
    b00, b11 = c00 + EPS2D, c11 + EPS2D
    det1 = b00 * b11 - c01 * c01
    comp = np.sqrt(np.maximum(0.0, det0 / det1))
    u, v = fx * m[:, 0] / zs + cx, fy * m[:, 1] / zs + cy
    bh = 0.5 * (b00 + b11)
    radius = np.ceil(3.0 * np.sqrt(bh + np.sqrt(np.maximum(0.01, bh * bh - det1))))
    seen = front & (det1 > 0) & ~((u + radius <= 0) | (u - radius >= p.W) | (v + radius <= 0) | (v - radius >= p.H))
    o = comp / (1.0 + np.exp(-p.logit_opacities.astype(np.float64)))
    rec = np.stack([u, v, b11 / det1, -c01 / det1, b00 / det1, o, zc, radius], axis=1)
    return np.where(seen[:, None], rec, 0.0), comp


def pack32(rec64):
    """float64 records (radius as a number) -> the device's fp32 layout (radius as int32 bits)"""
    rec = rec64.astype(np.float32)
    rec[:, 7] = rec64[:, 7].astype(np.int32).view(np.float32)
    return rec


def records_host(p, view=0):
    return pack32(project64(p, view)[0])


def _thin_draw(n, seed, W, H):
    g = np.random.default_rng(seed)
    xy = np.stack([g.uniform(-20.0, W + 20.0, n), g.uniform(-20.0, H + 20.0, n)], axis=1)
    s_major = np.exp(g.uniform(math.log(1.0), math.log(100.0), n))
    s_minor = np.minimum(np.exp(g.uniform(math.log(0.01), math.log(3.0), n)), s_major)
    theta = g.uniform(0.0, math.pi, n)
    diag = g.uniform(0, 1, n) < 1.0 / 3.0
    theta = np.where(diag, np.where(g.uniform(0, 1, n) < 0.5, 0.25, -0.25) * math.pi + g.uniform(-0.02, 0.02, n), theta)
    op = 10.0 ** g.uniform(-2.3, 0.0, n)
    depth = g.uniform(3.0, 5.0, n)
    return xy, s_major, s_minor, theta, op, depth


def thin_params(n, seed, W, H, n_views=1):
    """the `thin` recipe: major sigma 1 .. 100 px log-uniform, minor 0.01 .. 3 px before eps2d, a third of the angles within
    0.02 rad of +-45 degrees, opacity 10^U(-2.3, 0), centres from 20 px outside the image to 20 px outside"""
    return params_of(*_thin_draw(n, seed, W, H), W, H, n_views)


def behind_camera(p, n_total, live_rows):
    """p's rows scattered to `live_rows` of n_total rows; every other row sits behind the camera"""
    live_rows = np.asarray(live_rows)
    assert live_rows.size == p.means.shape[0]
    means = np.zeros((n_total, 3), np.float32)
    means[:, 2] = -1.0
    quats = np.tile(np.array([1, 0, 0, 0], np.float32), (n_total, 1))
    ls = np.full((n_total, 3), math.log(0.01), np.float32)
    lo = np.zeros(n_total, np.float32)
    means[live_rows], quats[live_rows], ls[live_rows], lo[live_rows] = p.means, p.quats, p.log_scales, p.logit_opacities
    return p._replace(means=means, quats=quats, log_scales=ls, logit_opacities=lo)


def _solve_shape(Sx, Sy, s_floor=0.15):
    """major / minor raw sigma and angle of a thin ellipse whose screen covariance (after eps2d) has diagonal Sx^2, Sy^2 and
    the smallest minor axis allowed"""
    sm2 = s_floor ** 2 + EPS2D
    sM2 = Sx * Sx + Sy * Sy - sm2
    cos2 = np.clip((Sx * Sx - Sy * Sy) / (sM2 - sm2), -1.0, 1.0)
    return math.sqrt(sM2 - EPS2D), s_floor, 0.5 * math.acos(cos2)


BOX_OP = 0.3   # o * comp of the mask cases: sqrt(2 thr) = 2.95 < 3, so gsplat's 3-sigma box never cuts the extent


def box_rows(tx0, ty0, w, h, kind, margin=7.0):
    """one Gaussian whose TIGHT box is exactly tiles [tx0, tx0 + w) x [ty0, ty0 + h): its extent reaches from `margin` px
    left of the first tile's centre to `margin` px right of the last one's (likewise in y).  kind "blob": axis-aligned;
    "diag": thin, along the box's diagonal."""
    ex, ey = 8.0 * (w - 1) + margin, 8.0 * (h - 1) + margin
    xc, yc = TS * tx0 + 8.0 * w, TS * ty0 + 8.0 * h
    thr = math.log(255.0 * BOX_OP) + 1e-3
    Sx, Sy = (ex - 0.01) / 1.001 / math.sqrt(2 * thr), (ey - 0.01) / 1.001 / math.sqrt(2 * thr)
    if kind == "blob":
        sM, sm, th = math.sqrt(Sx * Sx - EPS2D), math.sqrt(Sy * Sy - EPS2D), 0.0
        if sm > sM:
            sM, sm, th = sm, sM, math.pi / 2
    else:
        sM, sm, th = _solve_shape(Sx, Sy)
    comp = sM * sm / math.sqrt((sM * sM + EPS2D) * (sm * sm + EPS2D))
    return (xc, yc), sM, sm, th, BOX_OP / comp


MASK_IMAGES = {"mask_a": (200, 136), "mask_b": (544, 48), "mask_c": (48, 544)}
MASK_BOXES = {   # (tx0, ty0, w, h) of the exact boxes per image; every one as a blob and as a diagonal
    "mask_a": [(2, 0, 4, 8), (3, 1, 8, 4)],
    "mask_b": [(1, 1, 32, 1)],
    "mask_c": [(1, 1, 1, 32), (0, 1, 2, 16), (0, 20, 3, 11), (2, 0, 1, 33)],
}


def mask_params(name):
    W, H = MASK_IMAGES[name]
    rows, want = [], []
    for tx0, ty0, w, h in MASK_BOXES[name]:
        for kind in ("blob", "diag"):
            rows.append(box_rows(tx0, ty0, w, h, kind))
            want.append((tx0, ty0, w, h, kind))
    if name == "mask_a":
        tw, th = tiles_of(W, H)
        # >= 100 tiles: a blob and a diagonal that cover the whole 13 x 9 grid (clipped by all four borders)
        rows.append(((W / 2, H / 2), 400.0, 300.0, 0.0, 0.5))
        want.append((0, 0, tw, th, "blob"))
        rows.append(((W / 2 + 0.3, H / 2 - 0.2), 150.0, 0.15, math.atan2(H, W), 0.999))
        want.append((0, 0, tw, th, "diag"))
        # boxes clipped by each border and corner
        for cx, cy in ((2.0, 60.0), (W - 2.0, 70.0), (90.0, 1.0), (100.0, H - 1.5), (3.0, 3.0), (W - 3.0, H - 2.0), (-8.0, 40.0), (60.0, H + 9.0)):
            rows.append(((cx, cy), 12.0, 9.0, 0.3, 0.5))
            want.append(None)
            rows.append(((cx, cy), 25.0, 0.15, 0.8, 0.9))
            want.append(None)
    xy = np.array([r[0] for r in rows])
    sM, sm, th, op = (np.array([r[k] for r in rows]) for k in range(1, 5))
    depth = 3.0 + 0.01 * np.arange(len(rows))
    return Case(name, params_of(xy, sM, sm, th, op, depth, W, H), want)


DEAD_KINDS = ("behind", "faint", "off_image", "far_off", "tiny_comp")


def dead_params(n, seed, W, H):
    """rows the projection leaves without a pair: behind the camera (radius 0), o * comp < 1/255 (a faint logit; a minor
    axis so thin that the compensation does it), centres off the image by more than the radius, centres far off"""
    xy, sM, sm, th, op, depth = _thin_draw(n, seed, W, H)
    sM = np.minimum(sM, 20.0)
    op = np.maximum(op, 0.2)
    for k in range(n):
        kind = DEAD_KINDS[k % len(DEAD_KINDS)]
        if kind == "faint":
            op[k] = 0.0035
        elif kind == "off_image":
            xy[k, 0] = W + 3.0 * math.sqrt(sM[k] ** 2 + EPS2D) + 6.0
        elif kind == "far_off":
            xy[k] = (-40.0 * W, 55.0 * H)
        elif kind == "tiny_comp":
            sm[k], op[k] = 0.0015, 0.5
    p = params_of(xy, sM, sm, th, op, depth, W, H)
    behind = np.arange(n) % len(DEAD_KINDS) == 0
    p.means[behind, 2] = -2.0
    return p


def dead_records(n, seed, W, H):
    """the records of dead_params plus, at the record level, rows no projection writes: det <= 0 and radius == 0 with a
    live-looking ellipse"""
    rec = records_host(thin_params(n, seed, W, H))
    rec[:, 5] = np.maximum(rec[:, 5], 0.3)
    for k in range(n):
        if k % 3 == 0:
            rec[k, 7] = np.int32(0).view(np.float32)
        elif k % 3 == 1:
            rec[k, 3] = np.float32(1.5 * math.sqrt(abs(float(rec[k, 2]) * float(rec[k, 4]))))
        else:
            rec[k, 5] = np.float32(0.0039)
    return rec


# ---- grazing
GRAZE_KS = (2, 3, 4, 5)
GRAZE_FAMILIES = ("alpha", "slack")      # the threshold grazed: ln(255 o); the kernel's own 1.001 (ln(255 o) + 1e-3) + 1e-3
GRAZE_GEOMS = ("corner", "edge", "between", "long_diag")
GRAZE_M = 3.0


def _graze_geometry(geom):
    """canonical frame, the tile's rectangle at [0.5, 15.5]^2: (anchor, unit direction of approach, major, minor (before
    eps2d), angle, offset along the major axis)"""
    r2 = math.sqrt(0.5)
    if geom == "corner":       # a diagonal ellipse whose flank meets the corner pixel centre
        return (0.5, 0.5), (r2, r2), 6.0, 1.0, -0.25 * math.pi, 0.0
    if geom == "edge":         # a wide, tilted ellipse meets the left edge between its ends
        return (0.5, 8.3), (1.0, 0.0), 9.0, 3.0, math.radians(80.0), 0.0
    if geom == "between":      # the tip of a thin ellipse enters across the left edge between two rows of pixel centres
        return (0.5, 8.0), (1.0, 0.0), 12.0, 0.15, 0.01, 0.0
    if geom == "long_diag":    # the flank of a long thin diagonal meets the corner 50 px from its centre
        return (0.5, 0.5), (r2, r2), 40.0, 0.15, -0.25 * math.pi, 50.0
    raise ValueError(geom)


def _graze_target_logo(m, k, side, family):
    """ln(255 o) for which the rectangle minimum m is (1 + side 10^-k) times the family's threshold"""
    t = m / (1.0 + side * 10.0 ** -k)
    return t if family == "alpha" else (t - 1e-3) / 1.001 - 1e-3


def graze_threshold(o, family):
    lo = np.log(255.0 * np.asarray(o, np.float64))
    return lo if family == "alpha" else 1.001 * (lo + 1e-3) + 1e-3


def graze_rows(W=200, H=136):
    """the design list: (geom, quarter turns, k, side, family, tile)"""
    rows = []
    tiles = [(tx, ty) for ty in (2, 4, 6) for tx in (3, 5, 7, 9)]
    for geom in GRAZE_GEOMS:
        for rot in range(4):
            for k in GRAZE_KS:
                for side in (-1, 1):
                    for fam in GRAZE_FAMILIES:
                        rows.append((geom, rot, k, side, fam, tiles[len(rows) % len(tiles)]))
    return rows


def _turn(pt, rot):
    """`rot` quarter turns about the rectangle's centre (8, 8)"""
    x, y = pt[0] - 8.0, pt[1] - 8.0
    for _ in range(rot):
        x, y = -y, x
    return x + 8.0, y + 8.0


def _graze_one(geom, rot, tile, d, W, H, sig_op=0.5):
    anchor, n, sM, sm, th, along = _graze_geometry(geom)
    cx = anchor[0] - d * n[0] + along * math.cos(th)
    cy = anchor[1] - d * n[1] + along * math.sin(th)
    cx, cy = _turn((cx, cy), rot)
    return (TS * tile[0] + cx, TS * tile[1] + cy), sM, sm, th + 0.5 * math.pi * rot


def grazing_case(W=200, H=136):
    """Case whose info lists, per row, (geom, rot, k, side, family, tile).  Every ellipse is placed (bisection on the
    distance of approach, float64 projection of the fp32 parameters) so that the rectangle minimum of its tile is about
    GRAZE_M, then the logit is set so that this minimum is (1 + side 10^-k) times the family's threshold."""
    design = graze_rows(W, H)
    n = len(design)
    depth = 3.0 + 0.005 * np.arange(n)
    lo, hi = np.zeros(n), np.full(n, 120.0)
    tiles = np.array([r[5] for r in design])

    def build(d, sig_op):
        rows = [_graze_one(r[0], r[1], r[5], d[i], W, H) for i, r in enumerate(design)]
        return params_of(np.array([q[0] for q in rows]), [q[1] for q in rows], [q[2] for q in rows], [q[3] for q in rows],
                         sig_op, depth, W, H)

    for _ in range(60):
        mid = 0.5 * (lo + hi)
        rec, _comp = project64(build(mid, np.full(n, 0.5)))
        m, _, _ = rect_min64(rec[:, 0:6], np.arange(n), tiles[:, 0], tiles[:, 1])
        lo, hi = np.where(m < GRAZE_M, mid, lo), np.where(m < GRAZE_M, hi, mid)
    d = 0.5 * (lo + hi)
    p = build(d, np.full(n, 0.5))
    rec, comp = project64(p)
    m, _, _ = rect_min64(rec[:, 0:6], np.arange(n), tiles[:, 0], tiles[:, 1])
    logo = np.array([_graze_target_logo(m[i], r[2], r[3], r[4]) for i, r in enumerate(design)])
    sig_op = np.exp(logo) / 255.0 / comp
    assert (sig_op > 0.01).all() and (sig_op < 0.99).all(), (sig_op.min(), sig_op.max())
    return Case("grazing", build(d, sig_op), design)


def grazing_records(case):
    """the host's records of the grazing case with o re-solved AT THE RECORD LEVEL (o has 2^-24 relative steps, the
    position only 8e-6 px ones): every row's ratio is the designed one to 1e-7"""
    rec = records_host(case.params)
    n = rec.shape[0]
    tiles = np.array([r[5] for r in case.info])
    m, _, _ = rect_min64(rec[:, 0:6].astype(np.float64), np.arange(n), tiles[:, 0], tiles[:, 1])
    logo = np.array([_graze_target_logo(m[i], r[2], r[3], r[4]) for i, r in enumerate(case.info)])
    rec[:, 5] = (np.exp(logo) / 255.0).astype(np.float32)
    return rec


def grazing_ratios(rec, case):
    """per row: rectangle minimum of the chosen tile / the family's threshold - 1, in float64 from the records"""
    n = rec.shape[0]
    tiles = np.array([r[5] for r in case.info])
    m, _, _ = rect_min64(rec[:, 0:6].astype(np.float64), np.arange(n), tiles[:, 0], tiles[:, 1])
    fam = np.array([r[4] == "alpha" for r in case.info])
    with np.errstate(all="ignore"):
        t = np.where(fam, graze_threshold(rec[:, 5], "alpha"), graze_threshold(rec[:, 5], "slack"))
    return m / t - 1.0


# ---- the named cases
SIZES = (1, 255, 256, 257, 511, 513)
BIG_N, BIG_LIVE = 65537, 2000
GRIDS = {"grid_1456": (1456, 1456), "grid_2064": (2064, 2064)}
CASE_NAMES = (("thin", "grazing", "mask_a", "mask_b", "mask_c", "dead") + tuple(f"n{n}" for n in SIZES) + ("n65537",) + tuple(GRIDS)
              + ("grid_1456_n65537",))


@functools.lru_cache(maxsize=None)
def case(name):
    """Case (parameters in camera space, one view) -- built once, shared, never modified"""
    W, H = 200, 136
    if name == "thin":
        return Case(name, thin_params(4000, 11, W, H), None)
    if name == "grazing":
        return grazing_case(W, H)
    if name in MASK_IMAGES:
        return mask_params(name)
    if name == "dead":
        return Case(name, dead_params(200, 13, W, H), None)
    if name == "grid_1456_n65537":   # the sparse grid's rows scattered over 65 537: no-LDS emit_body with 512 threads
        W, H = GRIDS["grid_1456"]
        g = np.random.default_rng(29)
        rows = np.unique(np.concatenate([[0, BIG_N - 1], g.choice(BIG_N, 298, replace=False)]))
        return Case(name, behind_camera(thin_params(rows.size, 23 + W, W, H), BIG_N, rows), rows)
    if name == "n65537":
        g = np.random.default_rng(17)
        rows = np.unique(np.concatenate([[0, BIG_N - 1], g.choice(BIG_N, BIG_LIVE - 2, replace=False)]))
        return Case(name, behind_camera(thin_params(rows.size, 19, W, H), BIG_N, rows), rows)
    if name.startswith("n"):
        n = int(name[1:])
        return Case(name, thin_params(n, 100 + n, W, H), None)
    if name in GRIDS:
        W, H = GRIDS[name]
        return Case(name, thin_params(300, 23 + W, W, H), None)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def tail_scene(n_total):
    """the `thin` scene with two views, its 4000 rows scattered over n_total rows (row 0 and the last one live), the
    others behind the camera: what the fused tails of a step project"""
    p = thin_params(4000, 11, 200, 136, n_views=2)
    if n_total == 4000:
        return p
    g = np.random.default_rng(31)
    rows = np.unique(np.concatenate([[0, n_total - 1], g.choice(np.arange(1, n_total - 1), 3998, replace=False)]))
    return behind_camera(p, n_total, rows)


@functools.lru_cache(maxsize=None)
def host_case(name):
    """(Case, host records, Refs) -- computed once, shared, never modified"""
    c = case(name)
    rec = grazing_records(c) if name == "grazing" else records_host(c.params)
    rec.setflags(write=False)
    return c, rec, references(rec, c.params.W, c.params.H)
