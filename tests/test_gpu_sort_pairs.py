"""The tile sort's 512-thread variant takes TWO tiles per workgroup on the "prefix here" path (binning.hip,
tile_sort_kernel<.., PAIR>: middle-out rank b and rank T - 1 - b, both tiles' loads in one round trip).  Every output of
the sort is a function of the cursors and keys alone, so the paired variant must leave what the one-tile-per-workgroup
variants leave, bit for bit: here against the 256-thread variant (which the launcher picks while the population hint is
<= 1536) on the same scene, and against the plain-C oracle's stable (tile, depth) sort of the keys the step emitted.

All scenes are 512 x 512 (1024 tiles), 496 x 528 (31 x 33 = 1023 tiles: the middle rank has no partner) or, for the
three-batch prefix (which stays unpaired), 800 x 800 (2500 tiles), with 3000 .. 8000 Gaussians; each carries a clump that puts ~2000 hits into
one tile, so that the hint the trainer holds after `ensure_capacity` selects the 512-thread variant."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HINT_ONE_TILE = 1000  # <= 1536: the launcher takes the 256-thread variant, one tile per workgroup
VIEW = 1


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import synth
    return _lib, synth


def _world_at(sc, px, py, depth=3.9):
    """World point that view VIEW projects to pixel (px, py) at the given depth."""
    vm, K = sc.viewmats[VIEW], sc.Ks[VIEW]
    R, t = vm[:3, :3], vm[:3, 3]
    cam = torch.tensor([(px - float(K[0, 2])) / float(K[0, 0]) * depth, (py - float(K[1, 2])) / float(K[1, 1]) * depth, depth])
    return R.T @ (cam - t)


def _pixels(sc, means):
    vm, K = sc.viewmats[VIEW], sc.Ks[VIEW]
    p = means @ vm[:3, :3].T + vm[:3, 3]
    return K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]


def _clump(sc, gen, n, px, py, sigma=0.003):
    """n small round Gaussians around the world point behind pixel (px, py): about n hits in that pixel's tile."""
    means = _world_at(sc, px, py) + sigma * torch.randn(n, 3, generator=gen)
    return means, torch.full((n, 3), math.log(0.004))


def _scene(synth, kind):
    W, H = {"odd_grid": (496, 528), "prefix3": (800, 800)}.get(kind, (512, 512))
    n = 5900 if kind == "prefix3" else 5000
    sc = synth.make_scene(n, 2, W, H, seed=11, anisotropy=5.0, spread_opacity=True, scale=0.01)
    gen = torch.Generator().manual_seed(17)
    means, ls = sc.means, sc.log_scales
    tw, th = (W + 15) // 16, (H + 15) // 16
    if kind == "centred":
        means = 0.5 + 0.6 * (means - 0.5)  # everything well inside the middle rows: every partner tile B is empty
    else:
        means = 0.5 + 2.4 * (means - 0.5)   # out to (and beyond) all four borders
        px, py = _pixels(sc, means)
        # nothing of the spread cloud near tile 0, tile T - 1 and the first tile of row th / 2 (a footprint reaches < 60
        # pixels): the scenes decide
        far = torch.ones_like(px, dtype=torch.bool)
        for cx, cy in ((0.0, 0.0), (float(W), float(H)), (8.0, 16.0 * (th // 2) + 8.0)):
            far &= (px - cx).square() + (py - cy).square() > 90 ** 2
        means, ls = means[far], ls[far]
    extra = [_clump(sc, gen, 2000, 16 * (tw // 2) + 8.0, 16 * (th // 2) + 8.0)]  # ~2000 hits in one tile near the middle
    last_px, last_py = 16 * (tw - 1) + min(8.0, (W - 16 * (tw - 1)) / 2), 16 * (th - 1) + min(8.0, (H - 16 * (th - 1)) / 2)
    if kind in ("spread", "odd_grid", "prefix3", "overflow"):
        extra += [_clump(sc, gen, 40, last_px, last_py), _clump(sc, gen, 40, 8.0, 8.0)]  # tile T - 1 and tile 0 populated
    if kind == "heavy_partner":
        # tile 0 is middle-out rank T - 1, the partner B of rank 0's tile T / 2 (row th / 2, column 0): 800 keys in B, and
        # some in its A
        extra += [_clump(sc, gen, 800, 8.0, 8.0), _clump(sc, gen, 60, 8.0, 16 * (th // 2) + 8.0)]
    means = torch.cat([means] + [e[0] for e in extra])
    ls = torch.cat([ls] + [e[1] for e in extra])
    n = means.shape[0]
    g2 = torch.Generator().manual_seed(23)
    quats = synth.random_quats(n, g2)
    logit = torch.logit(0.05 + 0.85 * torch.rand(n, 1, generator=g2))
    assert 3000 <= n <= 8000, n
    return dataclasses.replace(sc, means=means.contiguous(), log_scales=ls.contiguous(), quats=quats, logit_opacities=logit)


def _trainer(sc, hint=None, seg_cap=None):
    from edgegaussians_amd import EdgeTrainer, LRSchedule
    tr = EdgeTrainer(sc.means, sc.log_scales, sc.quats, sc.logit_opacities, sc.viewmats, sc.Ks, sc.gt, sc.width, sc.height,
                     schedule=LRSchedule(scales_start=0, quats_start=0, opacities_start=0))
    tr.ensure_capacity()
    from edgegaussians_amd import _lib
    assert tr.seg_cap > 0 and tr.T <= _lib.PREFIX_HERE_MAX_TILES
    # the hint the trainer holds selects the 512-thread variant (launch_tile_sort: > 1536), and with it the pairs
    assert 1536 < tr.max_tile_seen <= 4096, tr.max_tile_seen  # (<= 4096: the small variant sorts every tile)
    tr.true_tile_max = tr.max_tile_seen
    if seg_cap is not None:
        tr._alloc_isect(tr.capacity, seg_cap)
    if hint is not None:
        tr.max_tile_seen = hint
        tr._args_cache = {}
    # what the launcher itself asks before it sizes the grid: pairs with the trainer's own hint on grids of 513 .. 2048
    # tiles, one tile per workgroup with the small hint and on the three-batch grid
    paired = int(_lib.load().eg_sort_two_tiles_per_workgroup(tr.T, tr.max_tile_seen))
    assert paired == (1 if hint is None and 512 < tr.T <= 2048 else 0), (tr.T, tr.max_tile_seen, paired)
    return tr


def _tables(tr):
    """Everything the sort leaves behind for one grad step of view VIEW (numpy), plus the keys it sorted."""
    torch.cuda.synchronize()
    T, sc_ = tr.T, tr.seg_cap
    total = tr.total.cpu().numpy().copy()
    table = tr.item_rec.cpu().numpy()
    valid = table[:, 2] == tr._ws_tag
    rec_at = np.nonzero(valid)[0]
    rec = table[valid]
    has_rec = np.zeros(T, bool)
    has_rec[rec[:, 0]] = True
    start, end = tr.offsets.cpu().numpy()[:T], tr.tile_end.cpu().numpy()[:T]
    pop = np.where(has_rec, end - start, 0)  # (an empty tile other than the last has no record and no table entry)
    first, iend = tr.item_offsets.cpu().numpy()[:T], tr.item_end.cpu().numpy()[:T]
    n_items = int(total[2])
    flat = tr.flatten_ids.cpu().numpy().reshape(-1)[:T * sc_].reshape(T, sc_)
    keys = tr.keys.cpu().numpy().reshape(-1)[:T * sc_].reshape(T, sc_)
    return dict(T=T, seg_cap=sc_, total=total, rec_at=rec_at, rec=rec, has_rec=has_rec, pop=pop,
                start=np.where(has_rec, start, -1), end=np.where(has_rec, end, -1), first=np.where(has_rec, first, -1),
                iend=np.where(has_rec, iend, -1), item_tile=tr.item_tile.cpu().numpy()[:n_items].copy(), flat=flat, keys=keys)


def _assert_same_tables(a, b, skip_ids_of=()):
    """Paired (a) against one tile per workgroup (b): bit for bit."""
    assert np.array_equal(a["total"], b["total"]), (a["total"], b["total"])
    assert np.array_equal(a["has_rec"], b["has_rec"]) and np.array_equal(a["pop"], b["pop"])
    for k in ("start", "end", "first", "iend", "item_tile"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["rec_at"], b["rec_at"]), "the records sit at other dispatch indices"
    assert np.array_equal(a["rec"][:, [0, 1, 3]], b["rec"][:, [0, 1, 3]])  # (word 2 is each call's own tag)
    for i in range(a["T"]):
        if i not in skip_ids_of:
            assert np.array_equal(a["flat"][i, :a["pop"][i]], b["flat"][i, :b["pop"][i]]), f"sorted ids of tile {i}"


def _assert_c_oracle_order(t, W, H):
    """The plain-C oracle's stable (tile, depth bits) sort of the keys the step emitted -- one single-tile pseudo-Gaussian per
    (Gaussian, tile) pair, in Gaussian order inside a tile, so that the oracle's tie-break is the Gaussian id -- gives the
    sorted ids per tile and the tile ranges."""
    from oracle import c_oracle as CO
    T, pop, tw = t["T"], t["pop"], (W + 15) // 16
    tile_of = np.repeat(np.arange(T), pop)
    keys = np.concatenate([t["keys"][i, :pop[i]] for i in range(T)]).astype(np.uint64)
    gid, dbits = (keys & np.uint64(0xffffffff)).astype(np.int64), (keys >> np.uint64(32)).astype(np.uint32)
    order = np.lexsort((gid, tile_of))  # emission order of the pseudo-Gaussians: by tile, then by Gaussian id
    tile_of, gid, dbits = tile_of[order], gid[order], dbits[order]
    for i in np.nonzero(pop)[0][:: max(1, T // 50)]:
        g = gid[tile_of == i]
        assert len(np.unique(g)) == len(g), "a Gaussian was emitted twice into a tile"
    M = len(gid)
    m2d = np.stack([16.0 * (tile_of % tw) + 8.0, 16.0 * (tile_of // tw) + 8.0], axis=1).astype(np.float32)
    radii, depths = np.ones(M, np.int32), np.ascontiguousarray(dbits).view(np.float32)
    tpg = np.zeros(M, np.int32)
    lib = CO.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert int(lib.ego_isect_count(p(m2d), p(radii), M, W, H, p(tpg))) == M and (tpg == 1).all()
    ids, flat, offs = np.zeros(M, np.int64), np.zeros(M, np.int32), np.zeros(T, np.int32)
    lib.ego_isect_emit_sort(p(m2d), p(radii), p(depths), M, W, H, C.c_int64(M), p(ids), p(flat), p(offs))
    want = gid[flat]
    ends = np.concatenate([offs[1:], [M]])
    assert np.array_equal(ends - offs, pop), "tile ranges"
    for i in range(T):
        assert np.array_equal(t["flat"][i, :pop[i]], want[offs[i]:ends[i]]), f"tile {i}: order differs from the C oracle's sort"
    # the tables against the populations: key ranges, the contiguous item numbering, the totals
    items = np.maximum(1, (pop + 127) // 128)
    starts = np.concatenate([[0], np.cumsum(items)[:-1]])
    hr = t["has_rec"]
    assert hr[T - 1] and np.array_equal(hr[:T - 1], pop[:T - 1] > 0)
    assert np.array_equal(t["start"][hr], (np.arange(T) * t["seg_cap"])[hr]) and np.array_equal((t["end"] - t["start"])[hr], pop[hr])
    assert np.array_equal(t["first"][hr], starts[hr]) and np.array_equal(t["iend"][hr], (starts + items)[hr])
    assert int(t["total"][2]) == int(items.sum()) and np.array_equal(t["item_tile"][starts[hr]], np.nonzero(hr)[0])
    return pop


def _run_pair(synth, kind):
    sc = _scene(synth, kind)
    w = synth.weight_map("whole", sc.gt[VIEW]).cuda()
    out = []
    for hint in (None, HINT_ONE_TILE):  # None: the trainer's own hint -> the paired 512-thread variant
        tr = _trainer(sc, hint)
        tr.grad_step(VIEW, w)
        t = _tables(tr)
        assert t["total"][1] == 0
        out.append((t, tr.pop_loss()))
    (tp, lp), (t1, l1) = out
    _assert_same_tables(tp, t1)
    assert abs(lp - l1) <= 1e-6 * abs(l1), (lp, l1)  # (only the order of the float atomics into the 64 partial sums differs)
    pop = _assert_c_oracle_order(tp, sc.width, sc.height)
    assert int(tp["total"][0]) == int(pop.sum()) and int(tp["total"][3]) == int(pop.max()) > 1536
    return sc, pop


def _partner(T):
    """tile -> (is it the first tile A of its workgroup, the other tile of the pair or -1)."""
    tile_of_rank = [(T // 2 - (r + 1) // 2) if (r & 1) else (T // 2 + r // 2) for r in range(T)]
    first, other = np.zeros(T, bool), np.full(T, -1)
    for b in range((T + 1) // 2):
        a, bb = tile_of_rank[b], tile_of_rank[T - 1 - b]
        first[a] = True
        if bb != a:
            other[a], other[bb] = bb, a
    return first, other


def test_every_partner_empty(env):
    """(a) a centred object: the second tile of every pair is empty (it only adds its background loss term)."""
    _lib, synth = env
    sc, pop = _run_pair(synth, "centred")
    first, other = _partner(1024)
    assert sorted(np.nonzero(~first)[0]) == sorted(other[first]) and (pop[~first][:-1] == 0).all()
    assert (pop[first] > 0).sum() > 100


def test_both_tiles_of_most_pairs_populated(env):
    """(b) Gaussians out to all four borders, tile T - 1 and tile 0 populated."""
    _lib, synth = env
    sc, pop = _run_pair(synth, "spread")
    first, other = _partner(1024)
    a = np.nonzero(first)[0]
    assert ((pop[a] > 0) & (pop[other[a]] > 0)).mean() > 0.5 and pop[1023] > 0 and pop[0] > 0
    assert pop[512] == 0 and other[512] == 0, "the pair (512, 0): only its SECOND tile is populated"


def test_first_and_last_tile_empty(env):
    """(c) as (b) with tile T - 1 (which keeps its full path: it leaves the view's totals) and tile 0 empty."""
    _lib, synth = env
    sc, pop = _run_pair(synth, "spread_empty_corners")
    assert pop[1023] == 0 and pop[0] == 0 and (pop > 0).mean() > 0.5


def test_partner_with_more_keys_than_threads(env):
    """(d) a second tile with more than 512 keys: further key batches after the one requested in the prologue."""
    _lib, synth = env
    sc, pop = _run_pair(synth, "heavy_partner")
    first, other = _partner(1024)
    assert not first[0] and other[0] == 512 and pop[0] > 512 and pop[512] > 0


def test_odd_grid(env):
    """(e) 31 x 33 = 1023 tiles: the middle rank's workgroup has one tile."""
    _lib, synth = env
    sc, pop = _run_pair(synth, "odd_grid")
    first, other = _partner(1023)
    assert (other == -1).sum() == 1 and pop[np.nonzero(other == -1)[0][0]] > 0 and pop[1022] > 0


def test_three_prefix_batches_keep_one_tile_per_workgroup(env):
    """(g) 800 x 800 = 2500 tiles: the PREFIX3 instantiations are not paired (not measured there); the 512-thread one against
    the 256-thread one and the oracle all the same."""
    _lib, synth = env
    sc, pop = _run_pair(synth, "prefix3")
    assert len(pop) == 2500 and pop[2499] > 0 and pop[0] > 0


def test_segment_overflow(env):
    """(f) a tile that outgrows seg_cap: the sticky flag goes up, the tile keeps seg_cap keys, the totals count the kept keys
    and the TRUE largest population.  (Which of the tile's keys got a slot depends on the order of the emit atomics: the ids
    of the truncated tiles are checked against the oracle's sort of each run's own keys, the rest bit for bit.)"""
    _lib, synth = env
    sc = _scene(synth, "overflow")
    w = synth.weight_map("whole", sc.gt[VIEW]).cuda()
    out = []
    for hint in (None, HINT_ONE_TILE):
        tr = _trainer(sc, hint, seg_cap=1024)
        true_max = tr.true_tile_max
        tr.grad_step(VIEW, w)
        t = _tables(tr)
        assert t["total"][1] == 1 and int(tr.tile_counts.abs().sum()) == 0
        _assert_c_oracle_order(t, sc.width, sc.height)
        out.append(t)
    tp, t1 = out
    full = set(np.nonzero(tp["pop"] == 1024)[0].tolist())
    # (the hint is the maximum over both views' counts; total[3] is this view's)
    assert full and tp["pop"].max() == 1024 and 1536 < int(tp["total"][3]) <= true_max
    assert int(tp["total"][0]) == int(tp["pop"].sum())
    _assert_same_tables(tp, t1, skip_ids_of=full)


def test_native_run_of_steps(env):
    """Ten chained steps of a native run (EdgeTrainer.train_steps: the one-kernel backward projects and bins the next view, the
    sort follows, the forward reads its records) on scene (b): parameters, moments and absgrads bit-identical between the
    paired variant and one tile per workgroup -- the forward finds every record and its look-back's dispatch-order
    assumption holds."""
    _lib, synth = env
    sc = _scene(synth, "spread")
    w = synth.weight_map("whole", sc.gt[0]).cuda()
    runs = []
    for hint in (None, HINT_ONE_TILE):
        tr = _trainer(sc, hint)
        tr.train_steps([s % 2 for s in range(10)], [w] * 10)
        torch.cuda.synchronize()
        assert not tr.overflowed() and int(tr.tile_counts.abs().sum()) == 0
        loss = tr.pop_loss()
        assert tr.overflow_events == 0
        st = dict(tr.state_dict(), m=tr.adam_m.clone(), v=tr.adam_v.clone(), absgrads=tr.absgrads.clone())
        runs.append((st, loss))
    for k, v in runs[0][0].items():
        assert torch.equal(runs[1][0][k], v), f"{k} differs between the paired sort and one tile per workgroup"
    assert math.isfinite(runs[0][1]) and abs(runs[0][1] - runs[1][1]) <= 1e-6 * abs(runs[1][1])


def test_where_the_launcher_pairs(env):
    """Pairs only where one 512-thread workgroup per tile is more than the chip holds (512) and the prefix takes at most two
    batches; never with a hint that selects the 256-thread variant."""
    _lib, synth = env
    q = _lib.load().eg_sort_two_tiles_per_workgroup
    assert [int(q(t, 2000)) for t in (1, 273, 512, 513, 1023, 1024, 2048, 2049, 2500, 2560)] == [0, 0, 0, 1, 1, 1, 1, 0, 0, 0]
    assert int(q(1024, 1536)) == 0 and int(q(1024, 1537)) == 1 and int(q(1024, 0)) == 0
