"""Scene discipline of the parity tests for tile sizes other than 16.  tests.util.clean_scene and borderline_pixel_mask
go through the C oracle, whose tile is fixed at 16 pixels; here the same two sets -- Gaussians whose integer decisions
hinge on rounding, pixels whose walk passes within a margin of a float threshold -- are formed for a tile size `ts` from
oracle.ref_torch's fp32 projection and its `isect_tiles` lists, in float64."""
import dataclasses
import functools
import math

import numpy as np
import torch

from tests.util import REL_ALPHA, REL_GAUSS, REL_T, clean_scene

SCENE_ARGS = dict(n_gauss=2500, n_views=5, width=204, height=140, seed=0, spread_opacity=True, scale=0.02, anisotropy=5.0)


def scene():
    """204 x 140 leaves partial tiles on both axes at 8, 16 and 32 pixels."""
    from edgegaussians_amd import synth
    a = SCENE_ARGS
    return synth.make_scene(a["n_gauss"], a["n_views"], a["width"], a["height"], seed=a["seed"],
                            spread_opacity=a["spread_opacity"], scale=a["scale"], anisotropy=a["anisotropy"])


def removed_cap(n0):
    return max(3, 0.016 * n0)


BORDER_CAP = 0.006  # share of the pixels (tests/util.py, check_fused_step_vs_c_oracle)


def _project(sc, v):
    from oracle import ref_torch as O
    with torch.no_grad():
        return O.project(sc.means, sc.quats, torch.exp(sc.log_scales), sc.viewmats[v], sc.Ks[v], sc.width, sc.height)


def tile_box_borderline(means2d, radii, ts, rel=REL_GAUSS):
    """bool [N]: visible Gaussians for which one of (x -+ r) / ts, (y -+ r) / ts -- float64, from the oracle's fp32
    means2d and radii -- lies within `rel` (relative, sized to max(1, |q|)) of an integer: floor / ceil may go either way."""
    m = np.asarray(means2d, np.float64)
    r = np.asarray(radii, np.float64)
    bad = np.zeros(m.shape[0], bool)
    for q in (m[:, 0] - r, m[:, 0] + r, m[:, 1] - r, m[:, 1] + r):
        q = q / float(ts)
        bad |= np.abs(q - np.rint(q)) <= rel * np.maximum(1.0, np.abs(q))
    return bad & (np.asarray(radii) > 0)


def clean_scene_ts(sc, views, ts):
    """tests.util.clean_scene (radius ceil, culls, the 16-pixel tile box), then the Gaussians whose tile box at `ts` hinges
    on rounding in any of `views`.  Returns (scene, number of Gaussians removed in all)."""
    sc1, removed = clean_scene(sc, views)
    bad = np.zeros(sc1.means.shape[0], bool)
    for v in views:
        radii, m2d = _project(sc1, v)[:2]
        bad |= tile_box_borderline(m2d.numpy(), radii.numpy(), ts)
    keep = torch.from_numpy(~bad)
    out = dataclasses.replace(sc1, means=sc1.means[keep].contiguous(), log_scales=sc1.log_scales[keep].contiguous(),
                              quats=sc1.quats[keep].contiguous(), logit_opacities=sc1.logit_opacities[keep].contiguous())
    return out, removed + int(bad.sum())


def borderline_pixels_ts(sc, view, ts, antialiased, rel_alpha=REL_ALPHA, rel_T=REL_T):
    """Float64 dense walk of every pixel over the `isect_tiles` list of its `ts`-pixel tile.  Returns (bool [H, W]: an
    entry the walk looks at, up to and including the first stopping one, has opac * exp(-sigma) within `rel_alpha`
    (relative) of 1/255 or of 0.999, or takes the running T within `rel_T` of 1e-4; number of pixels that reach the
    transmittance stop; the tiles' list lengths [T])."""
    from oracle import ref_torch as O
    from tests.composite_util import borderline_walk
    W, H = sc.width, sc.height
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    radii, m2d, depths, conics, comp = _project(sc, view)
    op = torch.sigmoid(sc.logit_opacities).squeeze(-1)
    op = (op * comp if antialiased else op).numpy()
    _tpg, ids, flat = O.isect_tiles(m2d.numpy(), radii.numpy(), depths.numpy(), ts, tw, th)
    offs = np.concatenate([O.isect_offset_encode(ids, tw, th).reshape(-1).astype(np.int64), [flat.shape[0]]])
    walk = borderline_walk(m2d.numpy(), conics.numpy(), op, flat, offs, ts, W, H, None, rel_alpha, rel_T)
    return walk.mask, walk.stopped, walk.lens


@functools.lru_cache(maxsize=None)
def setup(ts, cams, mode):
    """(clean scene, keep [C, H, W] = not borderline, Gaussians removed, N before, longest tile list over the cameras,
    pixels that reach the transmittance stop) for the cameras `cams` (a tuple) -- computed once per process; the
    tensors are shared between the tests and never modified."""
    sc0 = scene()
    sc, removed = clean_scene_ts(sc0, list(cams), ts)
    keep, longest, stopped = [], 0, 0
    for v in cams:
        border, st, lens = borderline_pixels_ts(sc, v, ts, mode == "antialiased")
        keep.append(~border)
        longest = max(longest, int(lens.max()))
        stopped += st
    return sc, torch.stack(keep), removed, sc0.means.shape[0], longest, stopped
