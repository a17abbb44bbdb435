"""Host helpers of the per-pixel / per-Gaussian compositing tests (tests/test_composite_host.py,
tests/test_gpu_composite_rows.py): synthetic splat records with no projection behind them, their tile lists from
oracle.ref_torch's integer binning, the float64 walk that classifies every pixel, the float64 reference of the chunked
compositing entries (oracle.ref_torch.composite + autograd) and the per-row bounds.  Nothing here needs a GPU.

The chunked entries and the kernels behind them (DISPATCH below is checked against the case table by the host test):

  eg_composite_{fwd,bwd}_ts_cams    csrc/tiles.hip      ts_composite_{fwd,bwd}_kernel<TS, CH, DEPTH, BG>
      TS in {8, 32}; CH = 0 with (DEPTH, BG) = (1, 0) only; CH in {2, 4, 8, 16, 32} with all four (DEPTH, BG)
  eg_composite_{fwd,bwd}_wide_cams  csrc/tiles.hip      ts_composite_{fwd,bwd}_kernel<16, CH, DEPTH, BG>
      CH in {2, 4, 8, 16, 32}, all four (DEPTH, BG)
  eg_composite_{fwd,bwd}_modes_cams csrc/composite.hip  composite_fwd_kernel<CH, false, DEPTH, BG> /
      composite_bwd_colors_kernel<CH, DEPTH, BG>: CH = 0 with (1, 0); CH in {1, 3} with (1, 0), (0, 1), (1, 1)
  eg_composite_fwd / eg_composite_bwd_colors csrc/composite.hip  the same kernels with CH in {1, 3} and (0, 0)
"""
import collections
import functools
import math

import numpy as np
import torch

from tests.util import (FWD_ROW_TOL, REL_ALPHA, REL_T, ROW_FLOOR, ROW_KAPPA_FACTOR, ROW_LOOSE, row_kappa, to_np,
                        ulp_perturbed)

W, H = 44, 27                     # partial tiles on both axes at 8, 16 and 32 pixels
STAGE = {8: 128, 16: 256, 32: 256}  # Gaussians per staging batch (kStage8, kStage32, kStage32); == _lib.TS_STAGE_BATCH at 8 / 32
AMIN, AMAX, TSTOP = 1.0 / 255.0, 0.999, 1e-4
N_DRAWS = 4                       # one-ulp perturbation draws behind kappa_r
BORDER_ALPHA_SLACK = 1.0 / 255.0 + 2e-4   # what one flipped threshold contribution moves a borderline pixel's alpha by
GRAD_NAMES = ("v_means2d", "absgrad", "v_conics", "v_opacities", "v_colors", "v_depths")
G2D_COLS = {"v_means2d": (0, 2), "absgrad": (2, 4), "v_conics": (4, 7), "v_opacities": (7, 8)}

Scene = collections.namedtuple("Scene", "name records")            # records: tuple over cameras of fp32 [N, 8]
Lists = collections.namedtuple("Lists", "offsets flat")            # per camera: int32 [T + 1] (local, last = M), int32 [M]
Walk = collections.namedtuple("Walk", "mask stopped lens last_batch capped looked")


# ---------------------------------------------------------------------------------------------------
# scenes: records built directly
def pack_records(means2d, conics, opacities, depths, radii):
    """[N, 8] fp32: x y a b c opacity depth radius-bits (the record of the compositing kernels)."""
    n = means2d.shape[0]
    sp = np.zeros((n, 8), np.float32)
    sp[:, 0:2] = means2d
    sp[:, 2:5] = conics
    sp[:, 5] = opacities
    sp[:, 6] = depths
    sp[:, 7] = np.asarray(radii, np.int32).view(np.float32)
    return sp


def make_records(n, seed, sigma=(1.5, 6.0), opacity_lo=0.003, capped_share=0.03, free_corner=0.0):
    """Centres uniform in [-6, W + 6] x [-6, H + 6]; major sigma uniform in `sigma` px, axis ratio 1 .. 4, random angle,
    conic = inverse covariance, radius = ceil(3 sigma_major); opacity log-uniform in opacity_lo .. 0.95 with
    `capped_share` of them reset to U(0.9992, 1) (beyond the 0.999 cap); depths U(0.5, 5), every 7th equal to the first.
    free_corner > 0: centres are pushed out of the top-left corner so that no tile box reaches [0, free_corner)^2."""
    g = np.random.default_rng(seed)
    xy = np.stack([g.uniform(-6.0, W + 6.0, n), g.uniform(-6.0, H + 6.0, n)], axis=1)
    s_major = g.uniform(sigma[0], sigma[1], n)
    s_minor = s_major / g.uniform(1.0, 4.0, n)
    th = g.uniform(0.0, math.pi, n)
    c, s = np.cos(th), np.sin(th)
    cxx = c * c * s_major ** 2 + s * s * s_minor ** 2
    cyy = s * s * s_major ** 2 + c * c * s_minor ** 2
    cxy = c * s * (s_major ** 2 - s_minor ** 2)
    det = cxx * cyy - cxy * cxy
    conics = np.stack([cyy / det, -cxy / det, cxx / det], axis=1)
    radii = np.ceil(3.0 * s_major).astype(np.int32)
    op = np.exp(g.uniform(math.log(opacity_lo), math.log(0.95), n))
    capped = g.uniform(0.0, 1.0, n) < capped_share
    op = np.where(capped, g.uniform(0.9992, 1.0, n), op)
    depths = g.uniform(0.5, 5.0, n)
    depths[::7] = depths[0]
    if free_corner > 0:
        near = (xy[:, 0] - radii < free_corner) & (xy[:, 1] - radii < free_corner)
        xy[near, 0] = free_corner + radii[near] + 0.5 + np.mod(xy[near, 0], 8.0)
    return pack_records(xy, conics, op, depths, radii)


@functools.lru_cache(maxsize=None)
def scene(name):
    """dense: every tile's list spans at least three staging batches.  sparse: lists under one batch, most pixels
    untouched, tile 0 (at every tile size) empty.  twocam: two record sets of one N whose lists differ in length."""
    if name == "dense":
        return Scene(name, (make_records(1400, 57),))
    if name == "sparse":
        return Scene(name, (make_records(40, 12, sigma=(0.6, 1.6), opacity_lo=0.05, capped_share=0.0, free_corner=32.0),))
    if name == "twocam":
        return Scene(name, (make_records(420, 13), make_records(420, 14, sigma=(1.0, 3.0), opacity_lo=0.02)))
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def lists(name, ts):
    """Per camera, the sorted lists of `ts`-pixel tiles from oracle.ref_torch's integer binning on the records' floats."""
    from oracle import ref_torch as O
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    out = []
    for rec in scene(name).records:
        _tpg, ids, flat = O.isect_tiles(rec[:, 0:2], rec[:, 7].view(np.int32), rec[:, 6], ts, tw, th)
        offs = np.concatenate([O.isect_offset_encode(ids, tw, th).reshape(-1), [flat.shape[0]]]).astype(np.int32)
        out.append(Lists(offs, np.ascontiguousarray(flat, np.int32)))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------
# the float64 walk: which pixels hinge on a float threshold, where every pixel's walk ends
def borderline_walk(means2d, conics, opacities, flat, offs, ts, width, height, stage=None, rel_alpha=REL_ALPHA,
                    rel_T=REL_T):
    """Float64 dense walk of every pixel over the list of its `ts`-pixel tile (offs [T + 1], flat [M]).  Returns
    Walk(mask bool [H, W]: an entry the walk looks at, up to and including the first stopping one, has
    opac * exp(-sigma) within `rel_alpha` (relative) of 1/255 or of 0.999, or takes the running T within `rel_T` of
    1e-4; number of pixels that reach the transmittance stop; the tiles' list lengths [T]; int [H, W]: index of the
    staging batch (of `stage` entries, counted from the list's start) that holds the pixel's last contributor, -1 on a
    pixel nothing contributes to; number of contributions at the 0.999 cap; int [H, W]: how many entries of its list
    the pixel's walk looks at)."""
    tw, th = math.ceil(width / ts), math.ceil(height / ts)
    m = np.asarray(means2d, np.float64)
    con = np.asarray(conics, np.float64)
    op = np.asarray(opacities, np.float64)
    offs = np.asarray(offs, np.int64)
    stage = int(stage) if stage else 1 << 30
    mask = np.zeros((height, width), bool)
    last_batch = np.full((height, width), -1, np.int64)
    n_looked = np.zeros((height, width), np.int64)
    stopped = capped = 0
    for t in range(tw * th):
        g = flat[offs[t]:offs[t + 1]]
        if g.size == 0:
            continue
        ty, tx = divmod(t, tw)
        ii, jj = np.meshgrid(np.arange(ty * ts, min(ty * ts + ts, height)), np.arange(tx * ts, min(tx * ts + ts, width)),
                             indexing="ij")
        dx = m[g, 0][None, :] - (jj.reshape(-1, 1) + 0.5)
        dy = m[g, 1][None, :] - (ii.reshape(-1, 1) + 0.5)
        sigma = 0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
        araw = op[g][None, :] * np.exp(-sigma)
        alpha = np.minimum(AMAX, araw)
        incl = (sigma >= 0.0) & (alpha >= AMIN)
        T_after = np.cumprod(np.where(incl, 1.0 - alpha, 1.0), axis=1)
        stops = incl & (T_after <= TSTOP)
        has_stop = stops.any(axis=1)
        first = np.where(has_stop, stops.argmax(axis=1), g.size)
        idx = np.arange(g.size)[None, :]
        looked = idx <= first[:, None]
        near_a = (np.abs(araw - AMIN) <= rel_alpha * AMIN) | (np.abs(araw - AMAX) <= rel_alpha * AMAX)
        near_T = incl & (np.abs(T_after - TSTOP) <= rel_T * TSTOP)
        mask[ii.reshape(-1), jj.reshape(-1)] = (looked & (near_a | near_T)).any(axis=1)
        contrib = incl & (idx < first[:, None])
        last = np.where(contrib, idx, -1).max(axis=1)
        last_batch[ii.reshape(-1), jj.reshape(-1)] = np.where(last >= 0, last // stage, -1)
        n_looked[ii.reshape(-1), jj.reshape(-1)] = np.minimum(first + 1, g.size)
        stopped += int(has_stop.sum())
        capped += int((contrib & (araw > AMAX)).sum())
    return Walk(torch.from_numpy(mask), stopped, np.diff(offs), last_batch, capped, n_looked)


@functools.lru_cache(maxsize=None)
def walks(name, ts):
    """Per camera, the Walk of scene `name` at tile size `ts` -- computed once, shared, never modified."""
    return tuple(borderline_walk(rec[:, 0:2], rec[:, 2:5], rec[:, 5], l.flat, l.offsets, ts, W, H, STAGE[ts])
                 for rec, l in zip(scene(name).records, lists(name, ts)))


def keep_mask(name, ts):
    """bool [C, H, W]: pixels outside the borderline set"""
    return torch.stack([~w.mask for w in walks(name, ts)])


# ---------------------------------------------------------------------------------------------------
# inputs of one case
Case = collections.namedtuple("Case", "family ts channels n_real depth bg scene per_camera va")


def case(family, ts, channels, depth, bg, scene="dense", n_real=None, per_camera=False, va=True):
    return Case(family, ts, channels, channels if n_real is None else n_real, bool(depth), bool(bg), scene, per_camera, va)


ALL_DB = ((0, 0), (1, 0), (0, 1), (1, 1))
MODE_DB = ((1, 0), (0, 1), (1, 1))
WIDTHS = (2, 4, 8, 16, 32)
DENSE_CASES = tuple(
    [case("ts", ts, 0, 1, 0) for ts in (8, 32)]
    + [case("ts", ts, ch, d, b) for ts in (8, 32) for ch in WIDTHS for d, b in ALL_DB]
    + [case("wide", 16, ch, d, b) for ch in WIDTHS for d, b in ALL_DB]
    + [case("modes", 16, 0, 1, 0)]
    + [case("modes", 16, ch, d, b) for ch in (1, 3) for d, b in MODE_DB])
# the reduced cross-section on the other scenes: per family one narrow and one 32-wide (modes: 3-wide) case
CROSS_CASES = tuple(
    case(f, ts, ch, d, b, scene=s, per_camera=(s == "twocam" and ch > 4))
    for s in ("sparse", "twocam")
    for f, ts, ch, d, b in (("ts", 8, 2, 1, 1), ("ts", 8, 32, 0, 1), ("ts", 32, 2, 0, 0), ("ts", 32, 32, 1, 1),
                            ("wide", 16, 2, 1, 0), ("wide", 16, 32, 1, 1), ("modes", 16, 1, 1, 0), ("modes", 16, 3, 1, 1)))


def kernel_of(c):
    """the instantiation a case runs in: (family, TS, CH, DEPTH, BG), by the dispatch of the three entry pairs"""
    if c.family == "modes":
        return (c.family, 16, c.channels, c.depth, c.bg and c.channels > 0)
    ch = 0 if c.channels == 0 else next(w for w in WIDTHS if c.channels <= w)
    return (c.family, c.ts, ch, c.depth, c.bg and c.channels > 0)


# eg_composite_bwd_colors (the operator's backward for general colours, tests/test_gpu_step_composite.py): the mode
# kernels without a depth channel and without a background, composite_bwd_colors_kernel<1 | 3, false, false>
COLORS_CASES = tuple(case("modes", 16, ch, 0, 0, scene=s, va=va)
                     for s, ch, va in (("dense", 1, True), ("dense", 1, False), ("dense", 3, True), ("dense", 3, False),
                                       ("sparse", 1, True), ("sparse", 3, False)))

DISPATCH = frozenset(
    [("ts", ts, 0, True, False) for ts in (8, 32)]
    + [("ts", ts, ch, bool(d), bool(b)) for ts in (8, 32) for ch in WIDTHS for d, b in ALL_DB]
    + [("wide", 16, ch, bool(d), bool(b)) for ch in WIDTHS for d, b in ALL_DB]
    + [("modes", 16, 0, True, False)]
    + [("modes", 16, ch, bool(d), bool(b)) for ch in (1, 3) for d, b in MODE_DB]
    + [("modes", 16, ch, False, False) for ch in (1, 3)])


@functools.lru_cache(maxsize=None)
def inputs(name, ts):
    """Colours [C, N, 32] in U(0, 1) (a case takes the first n_real channels; camera 0's when they are shared),
    backgrounds [C, 32] in U(0, 1), cotangents v_render [C, H, W, 33] and v_alphas [C, H, W] in U(-1, 1), zero on the
    borderline pixels of tile size `ts` (a case's depth cotangent is the LAST column).  fp32, shared, never modified."""
    C, N = len(scene(name).records), scene(name).records[0].shape[0]
    gen = torch.Generator().manual_seed(1000 + len(name))
    colors = torch.rand(C, N, 32, generator=gen)
    bgs = torch.rand(C, 32, generator=gen)
    v_render = 2.0 * torch.rand(C, H, W, 33, generator=gen) - 1.0
    v_alphas = 2.0 * torch.rand(C, H, W, generator=gen) - 1.0
    keep = keep_mask(name, ts)
    return colors, bgs, v_render * keep[..., None], v_alphas * keep


def grad_names(c):
    """the cotangents a case produces: no v_colors without colour channels, no v_depths without the depth channel"""
    return tuple(n for n in GRAD_NAMES if not (n == "v_colors" and c.n_real == 0) and not (n == "v_depths" and not c.depth))


def case_inputs(c):
    """(colors [C, N, n_real] or [N, n_real], backgrounds [C, n_real] or None, v_render [C, H, W, n_real + depth],
    v_alphas [C, H, W] or None) of a case, fp32 contiguous"""
    colors, bgs, v_render, v_alphas = inputs(c.scene, c.ts)
    n = c.n_real
    col = colors[:, :, :n] if c.per_camera else colors[0, :, :n]
    vr = torch.cat([v_render[..., :n], v_render[..., 32:]], dim=-1) if c.depth else v_render[..., :n]
    return (col.contiguous(), bgs[:, :n].contiguous() if c.bg else None, vr.contiguous(),
            v_alphas.contiguous() if c.va else None)


# ---------------------------------------------------------------------------------------------------
# the reference
def ref_composite(records, colors, backgrounds, depth, lsts, ts, v_render, v_alphas, dtype=torch.float64, gen=None):
    """oracle.ref_torch.composite on the records' floats in `dtype`, per camera, with the projection depth appended as
    the last colour channel (depth; its background 0) and pix += (1 - alpha) * background, then autograd (and the
    abs-gradient hook) with the cotangents v_render / v_alphas.  colors [N, D] (shared) or [C, N, D]; D may be 0 with
    depth.  gen: every float input of the operation (records, colours, backgrounds) gets one-ulp noise first.
    Returns a dict of [C, ...] tensors: render, alphas, last_ids and the cotangents GRAD_NAMES (v_colors [C, N, D],
    per camera even where the colours are shared; v_depths zeros without depth)."""
    from oracle import ref_torch as O
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    out = collections.defaultdict(list)
    for c, rec in enumerate(records):
        rec = torch.from_numpy(np.ascontiguousarray(rec))
        col = colors if colors.dim() == 2 else colors[c]
        parts = [rec[:, 0:2], rec[:, 2:5], rec[:, 5], col, rec[:, 6]]
        bg = backgrounds[c] if backgrounds is not None else None
        if gen is not None:
            *parts, bg = ulp_perturbed(parts + [bg if bg is not None else torch.zeros(0)], gen)
            bg = bg if backgrounds is not None else None
        m, con, op, col, dep = [p.to(dtype).clone().requires_grad_(True) for p in parts]
        D = col.shape[1]
        cc = torch.cat([col, dep[:, None]], dim=-1) if depth else col
        buf = torch.zeros(rec.shape[0], 2, dtype=dtype)
        l = lsts[c]
        render, alphas, last = O.composite(m, con, cc, op, W, H, ts, l.offsets[:-1].reshape(th, tw), l.flat, buf)
        alphas = alphas[..., 0]
        if bg is not None:
            pad = torch.cat([bg.to(dtype), torch.zeros(int(depth), dtype=dtype)])
            render = render + (1.0 - alphas)[..., None] * pad
        loss = (render * v_render[c].to(dtype)).sum()
        if v_alphas is not None:
            loss = loss + (alphas * v_alphas[c].to(dtype)).sum()
        grads = [torch.zeros_like(p) for p in (m, con, op, col, dep)]
        if loss.requires_grad:  # (an empty list of every tile leaves nothing to differentiate)
            got = torch.autograd.grad(loss, (m, con, op, col, dep), allow_unused=True)
            grads = [z if gi is None else gi for z, gi in zip(grads, got)]
        for k, v in zip(("render", "alphas", "last_ids", "v_means2d", "absgrad", "v_conics", "v_opacities", "v_colors",
                         "v_depths"), (render, alphas, last, grads[0], buf, grads[1], grads[2][:, None], grads[3],
                                       grads[4][:, None])):
            out[k].append(v.detach())
    return {k: torch.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(c):
    """(float64 reference of case `c`, {gradient name: kappa_r [C * N]}) -- cached per (scene, tile size, channels,
    depth, background, colour sharing, v_alphas): the family and the riders that only change addressing share it."""
    c = c._replace(family="", channels=c.n_real)
    return _reference(c)


@functools.lru_cache(maxsize=None)
def _reference(c):
    col, bg, vr, va = case_inputs(c)
    recs, lsts = scene(c.scene).records, lists(c.scene, c.ts)
    ref = ref_composite(recs, col, bg, c.depth, lsts, c.ts, vr, va)
    gen = torch.Generator().manual_seed(77)
    pert = [ref_composite(recs, col, bg, c.depth, lsts, c.ts, vr, va, gen=gen) for _ in range(N_DRAWS)]
    kappa = {k: row_kappa(_rows(ref[k]), [_rows(p[k]) for p in pert]) for k in grad_names(c)}
    return ref, kappa


def model_ratio(c):
    """{gradient name: largest ratio to the row bound of walk32 (the fp32 model of the kernels' order, from the stored
    alpha) against the float64 reference} for case `c` -- cached like the reference."""
    return _model_ratio(c._replace(family="", channels=c.n_real))


@functools.lru_cache(maxsize=None)
def _model_ratio(c):
    ref, kappa = _reference(c)
    m = walk32(c)
    return {k: grad_row_ratio(_rows(m[k]), ref[k], kappa[k])[0] for k in grad_names(c)}


def allowed_scale(c):
    """What a device backward may use of the row bound, per gradient: 1 where the fp32 model of its order holds the bound,
    else twice the model's own ratio (measured figures: tests/test_gpu_composite_rows.py)."""
    return {k: max(1.0, 2.0 * r) for k, r in model_ratio(c).items()}


def _rows(t):
    """[C, N, k] -> [C * N, k]"""
    return t.reshape(t.shape[0] * t.shape[1], -1)


# ---------------------------------------------------------------------------------------------------
# the checks
def grad_row_ratio(got, ref64, kappa, scale=1.0):
    """Per Gaussian row: |got - ref64|_rowmax against min((ROW_FLOOR + ROW_KAPPA_FACTOR kappa_r) sigma_r,
    1e-4 max|ref64| + 1e-4 sigma_r) -- tests.util's row bound, clipped to what assert_close grants the row, so that no
    row is held to less than the max-norm check.  Returns (largest ratio to the bound over the rows with sigma_r > 0,
    share of those rows whose UNCLIPPED relative bound exceeds ROW_LOOSE, the share exceeding 1e-3, rows over `scale`
    times the bound [indices], rows with sigma_r == 0 on which `got` is not exactly zero [indices])."""
    ref = to_np(_rows(ref64)).astype(np.float64)
    g = to_np(got).astype(np.float64).reshape(ref.shape)
    sigma = np.abs(ref).max(axis=1)
    live = sigma > 0
    rel = ROW_FLOOR + ROW_KAPPA_FACTOR * np.asarray(kappa, np.float64)
    bound = np.minimum(rel * sigma, 1e-4 * sigma.max(initial=0.0) + 1e-4 * sigma)
    ratio = np.where(live, np.abs(g - ref).max(axis=1) / np.where(live, bound, 1.0), 0.0)
    nonzero = np.nonzero(~live & (np.abs(g) != 0).any(axis=1))[0]
    n_live = max(int(live.sum()), 1)
    return (float(ratio.max(initial=0.0)), float((rel[live] > ROW_LOOSE).sum() / n_live),
            float((rel[live] > 1e-3).sum() / n_live), np.nonzero(ratio > scale)[0], nonzero)


def grad_row_check(got, ref64, kappa, name, scale=1.0):
    """Asserts grad_row_ratio's statement (the bound times `scale`); returns (largest ratio, share of loose rows)."""
    ratio, loose, _, over, nonzero = grad_row_ratio(got, ref64, kappa, scale)
    assert nonzero.size == 0, f"{name}: rows {nonzero[:8].tolist()} ({nonzero.size}) are not exactly zero where the float64 reference is"
    assert ratio <= scale, f"{name}: rows {over[:8].tolist()} ({over.size}) over {scale:.2f} x the per-row bound, the worst by {ratio:.2f} x"
    return ratio, loose


def fwd_ratios(render, alphas, last_ids, ref, keep):
    """Forward statement against the float64 reference `ref` on the kept pixels (bool [C, H, W]); every argument [C, H, W
    (, D)].  Returns dict(last_id_mismatches, untouched_nonzero: kept pixels with reference alpha == 0 whose alpha is
    not exactly 0, alpha_rel / alpha_abs: largest |d alpha| / alpha and |d alpha|, render_row: largest per-pixel
    |d render|_max / row maximum, border_alpha: largest |d alpha| inside the borderline set)."""
    keep = to_np(keep).astype(bool)
    a, a64 = to_np(alphas).astype(np.float64), to_np(ref["alphas"]).astype(np.float64)
    out = {}
    if last_ids is not None:
        out["last_id_mismatches"] = int((to_np(last_ids)[keep] != to_np(ref["last_ids"])[keep]).sum())
    out["untouched_nonzero"] = int((a[keep & (a64 == 0)] != 0).sum())
    live = keep & (a64 > 0)
    d = np.abs(a - a64)
    out["alpha_rel"] = float((d[live] / a64[live]).max(initial=0.0))
    out["alpha_abs"] = float(d[keep].max(initial=0.0))
    out["border_alpha"] = float(d[~keep].max(initial=0.0))
    r, r64 = to_np(render).astype(np.float64), to_np(ref["render"]).astype(np.float64)
    rowmax = np.abs(r64).max(axis=-1)
    dr = np.abs(r - r64).max(axis=-1)
    rl = keep & (rowmax > 0)
    out["render_row"] = float((dr[rl] / rowmax[rl]).max(initial=0.0))
    out["render_zero_rows_nonzero"] = int((dr[keep & (rowmax == 0)] != 0).sum())
    return out


def fwd_check(render, alphas, last_ids, ref, keep, name, tol=FWD_ROW_TOL):
    f = fwd_ratios(render, alphas, last_ids, ref, keep)
    assert f.get("last_id_mismatches", 0) == 0, f"{name}: {f['last_id_mismatches']} kept pixels disagree on the last contributor"
    assert f["untouched_nonzero"] == 0, f"{name}: alpha is not exactly zero on {f['untouched_nonzero']} untouched pixels"
    assert f["render_zero_rows_nonzero"] == 0, f"{name}: render is not exactly zero where the reference row is"
    assert f["alpha_rel"] <= tol and f["alpha_abs"] <= tol, f"{name}: alphas off by {f['alpha_rel']:.2e} relative, {f['alpha_abs']:.2e} absolute"
    assert f["render_row"] <= tol, f"{name}: a render row is off by {f['render_row']:.2e} of its maximum"
    assert f["border_alpha"] <= BORDER_ALPHA_SLACK, f"{name}: a borderline pixel's alpha moved by {f['border_alpha']:.2e}"
    return f


# ---------------------------------------------------------------------------------------------------
# the order of the device backward, in fp32 on the CPU
def walk32(c, stored_alpha=True):
    """Plain numpy float32 model of how the kernels (and gsplat's) walk a pixel, camera 0 of case `c`.  Forward: front to
    back, T a running fp32 product, alphas = 1 - T.  Backward: from the STORED alpha, T_final = 1 - alphas, then back to
    front T *= 1 / (1 - alpha) from the last contributor, the colours behind a Gaussian a running fp32 sum; a
    Gaussian's row is the fp32 sum of its pixels' terms.  Every step is rounded to fp32 where the kernels round; the
    exponential is numpy's, the order of the sums over pixels is numpy's.  stored_alpha False: the backward starts from
    the forward's T itself instead of 1 - (1 - T).  Returns the GRAD_NAMES tensors [C, N, k]."""
    cams = [_walk32_cam(c, cam, stored_alpha) for cam in range(len(scene(c.scene).records))]
    return {k: torch.cat([o[k] for o in cams]) for k in cams[0]}


def _walk32_cam(c, cam, stored_alpha):
    f = np.float32
    rec, l = scene(c.scene).records[cam], lists(c.scene, c.ts)[cam]
    col, bg, vr, va = [None if t is None else t.numpy() for t in case_inputs(c)]
    col = col[cam] if col.ndim == 3 else col
    N, n_ch, ts = rec.shape[0], c.n_real, c.ts
    K = n_ch + int(c.depth)
    full = np.concatenate([col, rec[:, 6:7]], axis=1) if c.depth else col          # [N, K]: the depth rides as a colour
    bgk = np.concatenate([bg[cam], np.zeros(int(c.depth), f)]) if bg is not None else None
    g2d, v_full = np.zeros((N, 8), f), np.zeros((N, K), f)
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    for t in range(tw * th):
        g = l.flat[l.offsets[t]:l.offsets[t + 1]]
        if g.size == 0:
            continue
        ty, tx = divmod(t, tw)
        ii, jj = np.meshgrid(np.arange(ty * ts, min(ty * ts + ts, H)), np.arange(tx * ts, min(tx * ts + ts, W)), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        dx = rec[g, 0][None, :] - (jj[:, None].astype(f) + f(0.5))
        dy = rec[g, 1][None, :] - (ii[:, None].astype(f) + f(0.5))
        A, B, Cc, o = rec[g, 2][None, :], rec[g, 3][None, :], rec[g, 4][None, :], rec[g, 5][None, :]
        sigma = f(0.5) * (A * dx * dx + Cc * dy * dy) + B * dx * dy
        vis = np.exp(-sigma)
        alpha = np.minimum(f(AMAX), o * vis)
        incl = (sigma >= 0) & (alpha >= f(AMIN))
        one_m = np.where(incl, f(1) - alpha, f(1))
        stops = incl & (np.cumprod(one_m, axis=1, dtype=f) <= f(TSTOP))
        first = np.where(stops.any(axis=1), stops.argmax(axis=1), g.size)
        contrib = incl & (np.arange(g.size)[None, :] < first[:, None])
        T_fwd = np.cumprod(np.where(contrib, one_m, f(1)), axis=1, dtype=f)[:, -1]
        alphas = f(1) - T_fwd                                                       # what the forward stores
        T_final = f(1) - alphas if stored_alpha else T_fwd
        # back to front: column r of the reversed arrays is the r-th entry from the list's end
        rev = slice(None, None, -1)
        cb, al, vs = contrib[:, rev], alpha[:, rev], vis[:, rev]
        ra = np.where(cb, f(1) / (f(1) - al), f(1)).astype(f)
        T = np.cumprod(np.concatenate([T_final[:, None], ra], axis=1), axis=1, dtype=f)[:, 1:]
        fac = np.where(cb, al * T, f(0))
        gr = g[rev]
        vrp = vr[cam, ii, jj]                                                         # [P, K]
        v_alpha = np.zeros_like(T)
        for k in range(K):
            ck = full[gr, k][None, :]
            term = ck * fac
            behind = np.cumsum(np.concatenate([np.zeros_like(term[:, :1]), term[:, :-1]], axis=1), axis=1, dtype=f)
            v_alpha = v_alpha + (ck * T - behind * ra) * vrp[:, k:k + 1]
            v_full[:, k] += np.bincount(gr, weights=(fac * vrp[:, k:k + 1]).sum(axis=0, dtype=f), minlength=N).astype(f)
        if va is not None:
            v_alpha = v_alpha + T_final[:, None] * ra * va[cam, ii, jj][:, None]
        if bgk is not None:
            bg_vr = f(0)
            for k in range(n_ch):
                bg_vr = bg_vr + bgk[k] * vrp[:, k]
            v_alpha = v_alpha + (-T_final[:, None]) * ra * bg_vr[:, None]
        v_alpha = np.where(cb, v_alpha, f(0)).astype(f)
        oo, dxr, dyr = o[:, rev], dx[:, rev], dy[:, rev]
        live = cb & (oo * vs <= f(AMAX))
        v_sigma = np.where(live, -oo * vs * v_alpha, f(0)).astype(f)
        gx = v_sigma * (A[:, rev] * dxr + B[:, rev] * dyr)
        gy = v_sigma * (B[:, rev] * dxr + Cc[:, rev] * dyr)
        comps = (gx, gy, np.abs(gx), np.abs(gy), f(0.5) * v_sigma * dxr * dxr, v_sigma * dxr * dyr,
                 f(0.5) * v_sigma * dyr * dyr, np.where(live, vs * v_alpha, f(0)))
        for k, comp in enumerate(comps):
            g2d[:, k] += np.bincount(gr, weights=comp.sum(axis=0, dtype=f), minlength=N).astype(f)
    out = {k: torch.from_numpy(g2d[None, :, a:b].copy()) for k, (a, b) in G2D_COLS.items()}
    out["v_colors"] = torch.from_numpy(v_full[None, :, :n_ch].copy())
    out["v_depths"] = torch.from_numpy(v_full[None, :, n_ch:].copy()) if c.depth else torch.zeros(1, N, 1)
    return out
