"""Float64 references and the screen-space scenes of the per-pixel intersection lists (functional.
rasterize_to_indices_in_range / accumulate; tests/test_indices_host.py, tests/test_gpu_indices.py).

(a) `walk_call`: the per-call walk -- the batches [range_start, range_end) of every tile's list, from a given T per
    pixel -- in float64 numpy; the three id lists in (camera, pixel) order;
(b) `ref_accumulate`: `accumulate` as gsplat defines it (no 1/255 skip, no stop), torch, float64 by default, autograd
    for the gradients;
(c) the borderline pixel set of a call (the `mask` of `walk_call`): tests.composite_util.borderline_walk's notion --
    on an entry the walk looks at, opacity * exp(-sigma) within REL_ALPHA of 1/255 or 0.999, or the running T within
    REL_T of 1e-4 -- extended by the start batch and the start T, which borderline_walk does not take.

Scenes are hand-made in screen space (the stages take screen-space tensors), 40 x 36 pixels, two cameras; everything
is computed once per process, shared between the tests and never modified."""
import collections
import functools
import math

import numpy as np
import torch

from tests.util import REL_ALPHA, REL_T

W, H, C = 40, 36, 2
HW = W * H
AMIN, AMAX, TSTOP = 1.0 / 255.0, 0.999, 1e-4
FULL = (0, 10 ** 10)
SLICES = ((0, 1), (1, 2), (1, 10 ** 10), (5, 9))
SCENE_OF = {8: "S8_16", 16: "S8_16", 32: "S32"}
REGIMES = ("thin", "thick")
# name: (N, seed); the seeds are fixed so that the conditions tests/test_indices_host.py asserts hold
SCENES = {"S8_16": (700, 11), "S32": (1300, 17)}
OPACITY = {"thin": (0.002, 0.03), "thick": (0.05, 0.95)}
MARGIN = 6.0          # px around the image in which centres may lie (S8_16)
SIGMA_RANGE = (1.5, 12.0)
N_TIES = 6
# S32 puts 1300 centres into one tile.  A Gaussian's 1/255 ring (relative width 2 REL_ALPHA) covers about 2 pi sigma_1
# sigma_2 * 2e-4 pixels, so with log-uniform sigmas (skew 1) the 2 x 1100 visible ones make ~50 of the 2880 pixels
# borderline in the thin regime, three times BORDER_CAP; mostly small footprints bring that below the cap
SIGMA_SKEW = {"S8_16": 1.0, "S32": 5.0}

Scene = collections.namedtuple("Scene", "name N means2d conics radii depths")   # [C,N,2] [C,N,3] [C,N] [C,N]
Lists = collections.namedtuple("Lists", "flat offsets")   # per camera: flat [M_c] (Gaussian indices), offsets [T + 1]
Call = collections.namedtuple("Call", "gaussian_ids pixel_ids camera_ids counts mask stopped stop_batch T_out looked")


@functools.lru_cache(maxsize=None)
def scene(name):
    N, seed = SCENES[name]
    rng = np.random.default_rng(seed)
    if name == "S32":   # every centre inside the first 32 x 32 tile
        xy = rng.uniform(0.5, 31.5, size=(C, N, 2))
    else:
        xy = np.stack([rng.uniform(-MARGIN, W + MARGIN, size=(C, N)), rng.uniform(-MARGIN, H + MARGIN, size=(C, N))], -1)
    lo, hi = math.log(SIGMA_RANGE[0]), math.log(SIGMA_RANGE[1])
    # sigmas in [1.5, 12], log-uniform in u ** SIGMA_SKEW[name]
    k = SIGMA_SKEW[name]
    s1, s2 = (np.exp(lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(C, N)) ** k) for _ in range(2))
    th = rng.uniform(0.0, math.pi, size=(C, N))
    cs, sn = np.cos(th), np.sin(th)
    # covariance R diag(s1^2, s2^2) R^T and its inverse (a, b, c)
    cxx = cs * cs * s1 ** 2 + sn * sn * s2 ** 2
    cxy = cs * sn * (s1 ** 2 - s2 ** 2)
    cyy = sn * sn * s1 ** 2 + cs * cs * s2 ** 2
    det = cxx * cyy - cxy * cxy
    conics = np.stack([cyy / det, -cxy / det, cxx / det], -1)
    radii = np.ceil(3.0 * np.maximum(s1, s2)).astype(np.int32)
    depths = rng.uniform(0.5, 9.5, size=(C, N))
    for c in range(C):   # a handful of exact depth ties
        a, b = rng.choice(N, size=(2, N_TIES), replace=False)
        depths[c, a] = depths[c, b]
    # the cameras see different subsets
    idx = np.arange(N)
    radii[0, idx % 8 == 3] = 0
    radii[1, idx % 7 == 5] = 0
    if name == "S8_16":  # one corner clear: the 8-pixel tile at the image's bottom right stays empty
        reach = (xy[..., 0] + radii >= 32.0) & (xy[..., 1] + radii >= 32.0)
        radii[reach] = 0
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return Scene(name, N, f32(xy), f32(conics), np.ascontiguousarray(radii), f32(depths))


@functools.lru_cache(maxsize=None)
def opacities(name, regime):
    N, seed = SCENES[name]
    lo, hi = OPACITY[regime]
    rng = np.random.default_rng(seed * 100 + REGIMES.index(regime))
    return np.ascontiguousarray(rng.uniform(lo, hi, size=(C, N)), dtype=np.float32)


def grid(ts):
    return math.ceil(W / ts), math.ceil(H / ts)


@functools.lru_cache(maxsize=None)
def lists(name, ts):
    """The oracle's binning per camera: (flat [M_c] Gaussian indices in depth order per tile, offsets [T + 1])."""
    from oracle import ref_torch as O
    sc = scene(name)
    tw, th = grid(ts)
    out = []
    for c in range(C):
        _tpg, ids, flat = O.isect_tiles(sc.means2d[c], sc.radii[c], sc.depths[c], ts, tw, th)
        offs = np.concatenate([O.isect_offset_encode(ids, tw, th).reshape(-1).astype(np.int64), [flat.shape[0]]])
        out.append(Lists(flat.astype(np.int64), offs))
    return tuple(out)


def device_lists(name, ts):
    """(isect_offsets [C, th, tw] int32, flatten_ids [M] int32 = c * N + n): what isect_tiles / isect_offset_encode return."""
    sc, ls = scene(name), lists(name, ts)
    tw, th = grid(ts)
    base, offs, flat = 0, [], []
    for c, l in enumerate(ls):
        offs.append(l.offsets[:-1] + base)
        flat.append(l.flat + c * sc.N)
        base += l.flat.shape[0]
    return (torch.from_numpy(np.stack(offs).reshape(C, th, tw).astype(np.int32)),
            torch.from_numpy(np.concatenate(flat).astype(np.int32)))


def local_lists(isect_offsets, flatten_ids, N):
    """Lists per camera from the global (isect_offsets [C, th, tw], flatten_ids [M]) the way rasterize_to_pixels reads
    them: every row local to its camera's list, the camera's end the next camera's first offset (the last one: M), all
    clamped into [0, M]; the cameras' lists one after the other."""
    offs = np.asarray(isect_offsets, np.int64)
    flat = np.asarray(flatten_ids, np.int64)
    Cn, M = offs.shape[0], flat.shape[0]
    first = offs.reshape(Cn, -1)
    ends = np.concatenate([first[1:, 0], [M]])
    local = np.clip(np.concatenate([first - first[:, :1], (ends - first[:, 0])[:, None]], axis=1), 0, M)
    out, base = [], 0
    for c in range(Cn):   # (a tile's range is [o[t], max(o[t], o[t + 1])): see walk_call)
        out.append(Lists(np.mod(flat, N), np.clip(base + local[c], 0, M)))
        base += int(local[c, -1])
    return out


def walk_call(means2d, conics, opac, ls, ts, range_start, range_end, T0=None, width=W, height=H,
              rel_alpha=REL_ALPHA, rel_T=REL_T):
    """Reference (a) and (c).  means2d [C,N,2], conics [C,N,3], opac [C,N]; ls: per camera Lists whose offsets index
    `flat` directly (a tile's entries are flat[offsets[t] : max(offsets[t], offsets[t + 1])]); T0 [C,H,W] (None: ones).
    Returns Call(the three id lists int64 in (camera, pixel) order and list order inside a pixel; counts [C,H,W];
    mask bool [C,H,W] = borderline; stopped bool [C,H,W]; stop_batch int [C,H,W] = batch of the tile's list that holds
    the entry the walk stopped before (-1: no stop); T_out float64 [C,H,W]; looked int [C,H,W] = entries looked at)."""
    Cn = len(ls)
    tw, th = math.ceil(width / ts), math.ceil(height / ts)
    B = ts * ts
    m, con, op = (np.asarray(a, np.float64) for a in (means2d, conics, opac))
    T0 = np.ones((Cn, height, width)) if T0 is None else np.asarray(T0, np.float64)
    counts = np.zeros((Cn, height, width), np.int64)
    mask = np.zeros((Cn, height, width), bool)
    stopped = np.zeros((Cn, height, width), bool)
    stop_batch = np.full((Cn, height, width), -1, np.int64)
    looked_n = np.zeros((Cn, height, width), np.int64)
    T_out = T0.copy()
    keys, gids = [], []
    for c in range(Cn):
        flat, offs = ls[c].flat, ls[c].offsets
        for t in range(tw * th):
            lo, hi = int(offs[t]), max(int(offs[t]), int(offs[t + 1]))
            a, b = min(lo + range_start * B, hi), min(lo + range_end * B, hi)
            if b <= a:
                continue
            g = flat[a:b]
            ty, tx = divmod(t, tw)
            ii, jj = np.meshgrid(np.arange(ty * ts, min(ty * ts + ts, height)), np.arange(tx * ts, min(tx * ts + ts, width)),
                                 indexing="ij")
            ii, jj = ii.reshape(-1), jj.reshape(-1)
            dx = m[c, g, 0][None, :] - (jj[:, None] + 0.5)
            dy = m[c, g, 1][None, :] - (ii[:, None] + 0.5)
            sigma = 0.5 * (con[c, g, 0] * dx * dx + con[c, g, 2] * dy * dy) + con[c, g, 1] * dx * dy
            araw = op[c, g][None, :] * np.exp(-sigma)
            alpha = np.minimum(AMAX, araw)
            incl = (sigma >= 0.0) & (alpha >= AMIN)
            t0 = T0[c, ii, jj][:, None]
            T_after = t0 * np.cumprod(np.where(incl, 1.0 - alpha, 1.0), axis=1)
            stops = incl & (T_after <= TSTOP)
            has_stop = stops.any(axis=1)
            first = np.where(has_stop, stops.argmax(axis=1), g.size)
            idx = np.arange(g.size)[None, :]
            looked = idx <= first[:, None]
            near_a = (np.abs(araw - AMIN) <= rel_alpha * AMIN) | (np.abs(araw - AMAX) <= rel_alpha * AMAX)
            near_T = incl & (np.abs(T_after - TSTOP) <= rel_T * TSTOP)
            contrib = incl & (idx < first[:, None])
            mask[c, ii, jj] = (looked & (near_a | near_T)).any(axis=1)
            stopped[c, ii, jj] = has_stop
            stop_batch[c, ii, jj] = np.where(has_stop, (a - lo + first) // B, -1)
            looked_n[c, ii, jj] = np.minimum(first + 1, g.size)
            counts[c, ii, jj] = contrib.sum(axis=1)
            T_out[c, ii, jj] = t0[:, 0] * np.prod(np.where(contrib, 1.0 - alpha, 1.0), axis=1)
            rows, cols = np.nonzero(contrib)   # (row-major: list order inside a pixel)
            keys.append(c * width * height + ii[rows] * width + jj[rows])
            gids.append(g[cols])
    if keys:
        key, gid = np.concatenate(keys), np.concatenate(gids)
        order = np.argsort(key, kind="stable")
        key, gid = key[order], gid[order]
    else:
        key = gid = np.zeros(0, np.int64)
    return Call(gid.astype(np.int64), (key % (width * height)).astype(np.int64), (key // (width * height)).astype(np.int64),
                counts, mask, stopped, stop_batch, T_out, looked_n)


@functools.lru_cache(maxsize=None)
def start_T(ts, regime, range_start):
    """float32 [C,H,W]: the transmittance reference (a) carries to batch `range_start` -- the float64 product over the
    entries the call (0, range_start) records from T = 1, rounded to fp32 (given to both sides)."""
    if range_start == 0:
        return np.ones((C, H, W), np.float32)
    return call(ts, regime, 0, range_start).T_out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def call(ts, regime, range_start, range_end):
    """Reference (a) of the case (tile size, regime, range) on its scene, from start_T."""
    name = SCENE_OF[ts]
    sc = scene(name)
    return walk_call(sc.means2d, sc.conics, opacities(name, regime), lists(name, ts), ts, range_start, range_end,
                     start_T(ts, regime, range_start))


def segments(call_or_ids, n_pixels=C * HW):
    """(starts, counts) [n_pixels] of the id lists' (camera, pixel) segments"""
    _g, pid, cid = call_or_ids[:3]
    key = np.asarray(cid, np.int64) * HW + np.asarray(pid, np.int64)
    counts = np.bincount(key, minlength=n_pixels)
    return np.cumsum(counts) - counts, counts


def same_segments(got, want, keep):
    """Number of pixels of `keep` (bool [C,H,W]) whose segment of Gaussian ids differs between two id-list triples, and
    whether both lists are ordered by (camera, pixel)."""
    keep = np.asarray(keep).reshape(-1)
    out = []
    for g, p, c in (got, want):
        g, p, c = (np.asarray(a, np.int64) for a in (g, p, c))
        key = c * HW + p
        assert key.size == 0 or (key.min() >= 0 and key.max() < keep.size)
        assert np.all(np.diff(key) >= 0), "rows are not in (camera, pixel) order"
        out.append((g, key, np.bincount(key, minlength=keep.size)))
    (g0, k0, n0), (g1, k1, n1) = out
    bad = (n0 != n1)
    # pixels with equal counts: compare element by element through each side's own starts
    s0, s1 = np.cumsum(n0) - n0, np.cumsum(n1) - n1
    eq = ~bad
    pos0 = np.arange(g0.size) - s0[k0]
    sel = eq[k0]
    diff = g0[sel] != g1[s1[k0[sel]] + pos0[sel]]
    bad_pix = np.zeros(keep.size, bool)
    bad_pix[k0[sel][diff]] = True
    bad |= bad_pix
    return int((bad & keep).sum())


def ref_accumulate(means2d, conics, opac, colors, gaussian_ids, pixel_ids, camera_ids, width=W, height=H,
                   dtype=torch.float64):
    """Reference (b): gsplat `accumulate` in torch (`dtype`), differentiable in the four float tensors ([C,N,...]).
    Inside each (camera, pixel), in the order given: w_k = alpha_k prod_{earlier} (1 - alpha), no skip, no stop."""
    Cn, N = means2d.shape[0], means2d.shape[1]
    D = colors.shape[-1]
    P = Cn * width * height
    g, p, c = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (gaussian_ids, pixel_ids, camera_ids))
    row = c * N + g
    px = (p % width).to(dtype) + 0.5
    py = torch.div(p, width, rounding_mode="floor").to(dtype) + 0.5
    xy, con = means2d.reshape(-1, 2)[row], conics.reshape(-1, 3)[row]
    dx, dy = xy[:, 0] - px, xy[:, 1] - py
    sigma = 0.5 * (con[:, 0] * dx * dx + con[:, 2] * dy * dy) + con[:, 1] * dx * dy
    alpha = torch.clamp(opac.reshape(-1)[row] * torch.exp(-sigma), max=AMAX)
    key = c * (width * height) + p
    counts = torch.bincount(key, minlength=P)
    starts = torch.cumsum(counts, 0) - counts
    pos = torch.arange(key.shape[0]) - starts[key]
    L = int(counts.max()) if key.numel() else 0
    dense = torch.zeros(P, max(L, 1), dtype=dtype).index_put((key, pos), alpha)
    cp = torch.cumprod(1.0 - dense, dim=1)
    T_excl = torch.cat([torch.ones_like(cp[:, :1]), cp[:, :-1]], dim=1)
    w = (dense * T_excl)[key, pos]
    renders = torch.zeros(P, D, dtype=dtype).index_add(0, key, w[:, None] * colors.reshape(-1, D)[row])
    alphas = torch.zeros(P, dtype=dtype).index_add(0, key, w)
    return renders.reshape(Cn, height, width, D), alphas.reshape(Cn, height, width, 1)


def colors(name, D, seed=5):
    N = SCENES[name][0]
    return 0.2 + 0.8 * torch.rand(C, N, D, generator=torch.Generator().manual_seed(seed + D))


def tensors(name, regime, dtype=torch.float32):
    """(means2d, conics, opacities) of the scene as torch tensors"""
    sc = scene(name)
    return tuple(torch.from_numpy(a).to(dtype) for a in (sc.means2d, sc.conics, opacities(name, regime)))
