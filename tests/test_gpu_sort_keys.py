"""The tile sort per key (csrc/binning.hip, tile_sort_kernel): eg_sort_pairs and eg_sort_segments on keys written by hand
(tests/sort_util.py), against np.sort of every segment's uint64 keys.  The sort's outputs are functions of its integer
inputs, so every assertion is bit-exact and nothing is excluded: flatten_ids and isect_ids are pre-filled with a sentinel,
equal the reference inside every segment and keep the sentinel outside and in the guards; key slots outside every segment,
beyond `capacity` and in the guards keep their bits (inside a segment the keys are not asserted: bucket + rank leaves
them, the networks rewrite them); with isect_ids = NULL flatten_ids is the same; eg_sort_segments leaves tile_start /
tile_end / item_end / item_tile as the formulas of include/edgegs.h give them, the cursors at zero, and no id of a stale
slot anywhere.  That every case sits on its boundary and takes the path named here is asserted on the CPU by
tests/test_sort_host.py from the fp32 bucket model, with `scale` moved by 1 +- 2^-20.

Which test reaches which instantiation (hint -> launch: 0: 256 threads + large, 1000: 256 only, 2000: 512 only, 4000:
512 + large):

  tile_sort_kernel<256, 4096, false>   bucket + rank   test_sort_pairs[small_sizes | small_kinds | handover | t1_4096 | t37 |
                                                       list_* | stride_* | cut_*, hints 0 / 1000], test_sort_segments[hints 0 / 1000]
                                       in-LDS network  test_sort_pairs[small_sizes (all_equal above 96 keys) | small_kinds (fill97,
                                                       outlier, two_values) | handover-0], test_sort_segments[seg_40_128 | seg_9_4096]
                                       hybrid network  test_sort_pairs[small_hybrid-1000 | t1_4097-1000 | cut_small-1000 | cut_big-1000],
                                                       test_sort_segments[seg_7_5000-1000 | seg_3_20000-1000]
  tile_sort_kernel<512, 4096, false>   the same three  the same cases at hints 2000 / 4000
  tile_sort_kernel<1024, 16384, true>  bucket + rank   test_sort_pairs[large_bucket | handover | t1_4097 | t37 | list_* | stride_* |
                                                       cut_small-0 | cut_big-0], test_sort_segments[seg_7_5000 | seg_3_20000,
                                                       hints 0 / 4000]
                                       in-LDS network  test_sort_pairs[large_network | handover | t37], test_sort_segments[seg_7_5000-0 /
                                                       4000], test_trainer_tile_above_4096_keys
                                       hybrid network  test_sort_pairs[large_hybrid | list_3_of_40], test_sort_segments[seg_3_20000-0 / 4000]
                                       list form       every case above with at most 512 oversized tiles; more entries than
                                                       workgroups: list_300_of_300 | list_300_of_340 (two rounds), list_512_of_520
                                                       (the list exactly full)
                                       stride form     test_sort_pairs[stride_513_of_520-0]
  tile_sort_kernel<512, 4096, false, false, PAIR> writing the "prefix here" tables the large variant then reads:
                                                       test_trainer_tile_above_4096_keys

Not reached here: PAIR and PREFIX3 on tiles the small variant sorts (tests/test_gpu_sort_pairs.py: every test pairs, and
test_three_prefix_batches_keep_one_tile_per_workgroup runs PREFIX3, both against the 256-thread variant and the plain-C
oracle's sort); batched launches with C > 1 (test_batched_projection of tests/test_gpu_tile_cull.py compares their pair
sets, not the order); item_front (grids above 2560 tiles inside a trainer).

Measured on the MI355X (recorded per case through tests.util.record as `sort_keys`: keys, tiles per variant and path, the
model's largest fill per path, seconds): 58 tests -- 36 eg_sort_pairs runs of 18 cases, each with and without isect_ids,
capacity 0, 20 eg_sort_segments runs of 5 cases, one trainer -- in 3.8 s for the whole file, the slowest the trainer case
(0.7 s) and stride_513_of_520 (0.1 s; 2 132 643 keys).  The model's largest fill and the path it implies, per case:
  small_sizes     spread <= 19: bucket + rank; all_equal n: bucket + rank up to 65 keys, the network from 255 keys on
  small_kinds     fill96 96 bucket + rank | fill97 97 network | outlier 4095 network | two_values ~n / 2 network (2 keys: 1,
                  bucket + rank) | full_range, descending, ascending <= 18: bucket + rank
  small_hybrid    21 tiles of 4097 .. 20 000 keys, all the small variant's hybrid network
  large_bucket    spread <= 32, full_range 29, fill96 96: all bucket + rank      large_network  all_equal n, fill97 97, outlier n - 1
  large_hybrid    8 tiles of 16 385 .. 40 000 keys          handover / t37  4096 keys small, 4097 large; fill96 / fill97 on either side
  list_* / stride_*  oversized tiles 4097 .. 4200 keys, fill <= 18 (1024 buckets): bucket + rank; small tiles fill <= 7
  cut_*           the cut tile: 350 of 700 keys (small), 4500 of 6000 (large at hint 0, small hybrid at 1000), 3000 of 6000 (small)
  seg_40_128      32 tiles bucket + rank (96 the fullest), 5 network (97 .. 128)       seg_9_4096(_clip)  fill <= 19; 1023 and 97 network
  seg_7_5000      hints 0 / 4000: large bucket + rank (<= 15) and network (4998, 5000); 1000 / 2000: four hybrid tiles
  seg_3_20000     hints 0 / 4000: 16 384 keys large bucket + rank (30), 20 000 twice large hybrid; 1000 / 2000: three small hybrid
  trainer         1024 tiles, 32 648 keys, one tile of 5628 keys (seg_cap 8704): fill 1210, the large variant's network
Every assertion held on the first run: the sort needed no change.  (A planted defect -- the large variant's rank pass
comparing depth bits alone -- fails exactly the 20 runs listed above under its bucket + rank path, and no other.)
"""
import time

import numpy as np
import pytest
import torch

from tests import sort_util as U
from tests.util import record

pytestmark = pytest.mark.gpu

FLAGS = 1 | 2 | 4 | 8   # log-scales, logit opacities, antialiased, tight tiles
VIEW = 1


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    t0 = time.perf_counter()
    yield _lib
    record("sort_keys", case="whole file", seconds=round(time.perf_counter() - t0, 2))


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda().contiguous()


def _back(dev, like):
    return {k: (v.cpu().numpy().view(np.uint64) if like[k].dtype == np.uint64 else v.cpu().numpy()) for k, v in dev.items()}


def _sort_pairs(L, with_isect):
    from edgegaussians_amd._lib import call, ptr, stream
    before = U.outputs_before(L, with_isect)
    d = {k: _dev(v) for k, v in before.items()}
    call("eg_sort_pairs", ptr(d["keys"]), ptr(d["offsets"]), L.T, L.capacity, ptr(d["flat"]),
         ptr(d["isect"]) if with_isect else None, L.hint, stream())
    torch.cuda.synchronize()
    return _back(d, before)


def _sort_segments(L):
    from edgegaussians_amd._lib import call, ptr, stream
    before = U.outputs_before(L)
    d = {k: _dev(v) for k, v in before.items()}
    call("eg_sort_segments", ptr(d["keys"]), ptr(d["cursor"]), L.T, L.seg_cap, ptr(d["flat"]), ptr(d["tile_start"]),
         ptr(d["tile_end"]), ptr(d["item_first"]), ptr(d["item_end"]), ptr(d["item_tile"]), L.max_items, L.hint, stream())
    torch.cuda.synchronize()
    return _back(d, before)


@pytest.mark.parametrize("name,hint", U.CLASSIC_RUNS)
def test_sort_pairs(lib, name, hint):
    t0 = time.perf_counter()
    L = U.classic_case(name, hint)
    e = U.expected(L)
    out = _sort_pairs(L, True)
    U.check_sorted(L, out, e)
    out = _sort_pairs(L, False)   # isect_ids = NULL: the same flatten_ids
    U.check_sorted(L, out, e)
    record("sort_keys", **U.figures(L), seconds=round(time.perf_counter() - t0, 2))


def test_capacity_zero_touches_nothing(lib):
    """capacity == 0 returns EG_OK before anything is launched"""
    from edgegaussians_amd._lib import call, ptr, stream
    L = U.build_classic("capacity0", [(5, "spread"), (0, "spread"), (300, "all_equal")], 0, seed=9)
    before = U.outputs_before(L, True)
    d = {k: _dev(v) for k, v in before.items()}
    call("eg_sort_pairs", ptr(d["keys"]), ptr(d["offsets"]), L.T, 0, ptr(d["flat"]), ptr(d["isect"]), 0, stream())
    call("eg_sort_pairs", None, ptr(d["offsets"]), L.T, 0, None, None, 1000, stream())
    torch.cuda.synchronize()
    after = _back(d, before)
    for k, v in before.items():
        assert np.array_equal(after[k], v), f"capacity 0: {k} was written"


@pytest.mark.parametrize("name,hint", U.SEGMENTED_RUNS)
def test_sort_segments(lib, name, hint):
    t0 = time.perf_counter()
    L = U.segmented_case(name, hint)
    out = _sort_segments(L)
    U.check_sorted(L, out)
    record("sort_keys", **U.figures(L), seg_cap=L.seg_cap, max_items=L.max_items, seconds=round(time.perf_counter() - t0, 2))


# ---------------------------------------------------------------------------------------------------
# inside a training step: the large variant behind the small one that writes the "prefix here" tables
def _heavy_scene(synth):
    """512 x 512 (1024 tiles), Gaussians out to all four borders, one clump of ~5000 hits in one tile near the middle,
    tile 0 and tile T - 1 populated"""
    import dataclasses
    import math
    from tests.test_gpu_sort_pairs import _clump, _pixels
    W = H = 512
    sc = synth.make_scene(5000, 2, W, H, seed=11, anisotropy=5.0, spread_opacity=True, scale=0.01)
    gen = torch.Generator().manual_seed(17)
    means, ls = 0.5 + 2.4 * (sc.means - 0.5), sc.log_scales
    px, py = _pixels(sc, means)
    far = torch.ones_like(px, dtype=torch.bool)
    for cx, cy in ((0.0, 0.0), (float(W), float(H))):
        far &= (px - cx).square() + (py - cy).square() > 90 ** 2
    means, ls = means[far], ls[far]
    extra = [_clump(sc, gen, 5600, 16 * 16 + 8.0, 16 * 16 + 8.0), _clump(sc, gen, 40, W - 8.0, H - 8.0), _clump(sc, gen, 40, 8.0, 8.0)]
    means = torch.cat([means] + [x[0] for x in extra])
    ls = torch.cat([ls] + [x[1] for x in extra])
    n = means.shape[0]
    g2 = torch.Generator().manual_seed(23)
    quats = synth.random_quats(n, g2)
    logit = torch.logit(0.05 + 0.85 * torch.rand(n, 1, generator=g2))
    assert math.isfinite(float(means.sum())) and 8000 <= n <= 11000, n
    return dataclasses.replace(sc, means=means.contiguous(), log_scales=ls.contiguous(), quats=quats, logit_opacities=logit)


def _heavy_trainer(sc):
    from edgegaussians_amd import EdgeTrainer, LRSchedule, _lib
    tr = EdgeTrainer(sc.means, sc.log_scales, sc.quats, sc.logit_opacities, sc.viewmats, sc.Ks, sc.gt, sc.width, sc.height,
                     schedule=LRSchedule(scales_start=0, quats_start=0, opacities_start=0))
    tr.ensure_capacity()
    assert tr.T == 1024 <= _lib.PREFIX_HERE_MAX_TILES
    assert tr.max_tile_seen > U.SMALL_CAP and tr.seg_cap > U.SMALL_CAP, (tr.max_tile_seen, tr.seg_cap)
    return tr


def test_trainer_tile_above_4096_keys(lib):
    """grad_step on a view with one tile above 4096 keys: the (paired, 512-thread) small variant writes every tile's
    tables and leaves that tile to the large variant, which reads its range from them.  Every tile's flatten_ids against
    np.sort of the keys a second, identical trainer's parameters give through eg_project_emit; the tables against the
    populations."""
    from edgegaussians_amd import synth
    from edgegaussians_amd._lib import call, ptr, stream
    from tests.test_gpu_sort_pairs import _tables
    t0 = time.perf_counter()
    sc = _heavy_scene(synth)
    tr = _heavy_trainer(sc)
    assert int(lib.load().eg_sort_two_tiles_per_workgroup(tr.T, tr.max_tile_seen)) == 1
    w = synth.weight_map("whole", sc.gt[VIEW]).cuda()
    tr.grad_step(VIEW, w)
    t = _tables(tr)
    assert t["total"][1] == 0 and int(tr.tile_counts.abs().sum()) == 0
    T, seg_cap = tr.T, tr.seg_cap
    # the same view's keys from a second trainer's parameters
    two = _heavy_trainer(sc)
    splat = torch.full((two.N, 8), float("nan"), device="cuda")
    cursor, item_first, total, ticket = (torch.zeros(k, dtype=torch.int32, device="cuda") for k in (T, T, 4, T + 2))
    keys = torch.full((T * seg_cap,), -1, dtype=torch.int64, device="cuda")
    call("eg_project_emit", ptr(two.means), ptr(two.quats), ptr(two.log_scales), ptr(two.logit_opacities),
         ptr(two.viewmats[VIEW].contiguous()), ptr(two.Ks[VIEW].contiguous()), two.N, sc.width, sc.height, FLAGS, ptr(splat),
         ptr(cursor), seg_cap, ptr(keys), ptr(item_first), tr.max_items, ptr(total), ptr(ticket), stream())
    torch.cuda.synchronize()
    pop = cursor.cpu().numpy().astype(np.int64)
    k = keys.cpu().numpy().view(np.uint64).reshape(T, seg_cap)
    heavy = int(np.argmax(pop))
    assert U.SMALL_CAP < pop[heavy] <= min(seg_cap, U.LARGE_CAP) and (pop > U.SMALL_CAP).sum() >= 1 and pop[0] > 0 and pop[T - 1] > 0
    assert int(total.cpu()[1]) == 0
    for i in range(T):
        seg = k[i, :pop[i]]
        U.assert_precondition(seg)
    # (the large variant's path on the heavy tile, from the model)
    variant, path, fill = U.path_of(k[heavy, :pop[heavy]], U.Form(512, True))
    assert variant == "large"
    # the tables: an empty tile other than the last has no record and no entry
    hr = t["has_rec"]
    assert hr[T - 1] and np.array_equal(hr[:T - 1], pop[:T - 1] > 0) and np.array_equal(t["pop"], pop)
    items = np.maximum(1, (pop + 127) // 128)
    first = np.cumsum(items) - items
    assert items.sum() <= tr.max_items
    assert np.array_equal(t["start"][hr], (np.arange(T) * seg_cap)[hr]) and np.array_equal(t["end"][hr], (np.arange(T) * seg_cap + pop)[hr])
    assert np.array_equal(t["first"][hr], first[hr]) and np.array_equal(t["iend"][hr], (first + items)[hr])
    want_tile = np.repeat(np.arange(T), items)
    rec_items = np.repeat(hr, items)
    assert np.array_equal(t["item_tile"][rec_items], want_tile[rec_items])
    assert t["total"].tolist() == [int(pop.sum()), 0, int(items.sum()), int(pop.max())]
    # the order, every tile
    _ks, ids, _isect = U.ref_sort(k.reshape(-1), np.arange(T) * seg_cap, np.arange(T) * seg_cap + pop, range(T))
    for i in range(T):
        assert np.array_equal(t["flat"][i, :pop[i]], ids[i]), f"tile {i} ({pop[i]} keys): order differs from np.sort of its keys"
    record("sort_keys", case="trainer", tiles=T, keys=int(pop.sum()), largest_tile=int(pop[heavy]), seg_cap=seg_cap,
           **{f"{variant}_{path}": 1, f"{variant}_{path}_max_fill": fill}, tiles_above_4096=int((pop > U.SMALL_CAP).sum()),
           seconds=round(time.perf_counter() - t0, 2))
