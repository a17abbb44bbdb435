"""CPU-only statements behind tests/test_gpu_sort_keys.py: every case of tests/sort_util.py is built and sits on the boundary
it is named for, the path each tile is meant to take (bucket + rank, the in-LDS network, the hybrid network) follows
from the fp32 bucket model with `scale` moved by 1 +- 2^-20, launch_form equals a literal reading of launch_tile_sort's
conditions, and check_sorted -- the comparer of the GPU file -- rejects every planted defect.

Measured here: 36 classic runs (18 cases x their hints) and 20 segmented ones; the largest, stride_513_of_520, holds
2 132 643 keys in 520 tiles (43 MB of keys, ids and isect ids).  Largest fill of the model on the `spread` tiles that take
bucket + rank: 19 at 4096 keys and 512 buckets (256 threads), 15 at 1024 buckets (512 threads), 32 on the large variant's
16 383 keys at 1024 buckets; exactly 96 / 97 on fill96 / fill97, n - 1 on `outlier`, n on `all_equal`.
"""
import numpy as np
import pytest

from tests import sort_util as U
from tests.util import record_cpu

BUCKET_KINDS = ("spread", "full_range", "descending", "ascending")


def _want_path(kind, keys, form):
    """(variant, path, exact fill or None) from the case's NAME alone"""
    n = len(keys)
    if n == 0:
        return "none", "empty", 0
    large = form.large and n > U.SMALL_CAP
    variant = "large" if large else f"small{form.threads}"
    if n > (U.LARGE_CAP if large else U.SMALL_CAP):
        return variant, "hybrid", 0
    depth = keys >> U.U64(32)
    fill = {"all_equal": n, "outlier": n - 1, "fill96": 96, "fill97": 97,
            "two_values": int(np.unique(depth, return_counts=True)[1].max())}.get(kind)
    if fill is None:
        assert kind in BUCKET_KINDS
        return variant, "bucket", None
    return variant, ("bucket" if fill <= U.MAX_FILL else "network"), fill


def _check_paths(L):
    """the model's verdict (asserted inside path_of to hold with the margin) is the one the case is built for"""
    got = L.paths()
    for t, (n, kind) in enumerate(L.specs):
        variant, path, fill = _want_path(kind, L.segment_keys(t), L.form)
        assert got[t][:2] == (variant, path), (L.name, L.hint, t, n, kind, got[t])
        if fill is not None and path != "hybrid":
            assert got[t][2] == fill, (L.name, t, kind, got[t], fill)
        elif path == "bucket":
            assert got[t][2] <= U.MAX_FILL
        U.assert_precondition(L.segment_keys(t))
    return got


def _literal_form(T, hint):
    """launch_tile_sort read condition by condition (C == 1, seg.total == nullptr)"""
    wide = hint > 1536 and T <= 4096
    small_only = hint > 0 and hint * 5 // 4 <= 4096
    return U.Form(512 if wide else 256, not small_only)


def test_launch_form_is_the_launchers_conditions():
    pairs = {(len(c["tiles"]), h) for c in U.CLASSIC.values() for h in c["hints"]}
    pairs |= {(c["T"], h) for c in U.SEGMENTED.values() for h in U.HINTS}
    pairs |= {(T, h) for T in (1, 4096, 4097, 7500) for h in U.HINTS}
    for T, h in sorted(pairs):
        for seg in (False, True):
            f = U.launch_form(T, h, seg)
            assert f == _literal_form(T, h), (T, h)
            assert f.nb == 2 * f.threads and f.small_cap == (4096 if f.large else 0x7fffffff)
    assert [(U.launch_form(40, h).threads, U.launch_form(40, h).large) for h in U.HINTS] == \
        [(256, True), (256, False), (512, False), (512, True)]
    assert U.launch_form(4097, 2000).threads == 256 and U.launch_form(4097, 4000) == U.Form(256, True)


def test_reference_on_keys_written_by_hand():
    keys = np.array([U.make_key(5, 9), U.make_key(5, 3), U.make_key(1, 0x7fffffff), U.make_key(0xffffffff, 0),
                     U.make_key(7, 1), U.make_key(2, 2)], dtype=U.U64)
    ks, ids, isect = U.ref_sort(keys, [0, 4, 4], [4, 4, 6], [0, 1, 2])
    assert [a.tolist() for a in ids] == [[0x7fffffff, 3, 9, 0], [], [2, 1]]
    assert isect[0].tolist() == [1, 5, 5, 0xffffffff] and isect[2].tolist() == [(2 << 32) | 2, (2 << 32) | 7]
    assert ks[0].tolist() == [(1 << 32) | 0x7fffffff, (5 << 32) | 3, (5 << 32) | 9, 0xffffffff << 32]
    assert ids[0].dtype == np.int32 and isect[0].dtype == np.int64 and ks[0].dtype == np.uint64


def test_bucket_model_on_known_maps():
    d = np.uint32(0x40000000) + np.arange(1024, dtype=np.uint32) * np.uint32(256)
    assert U.bucket_model(d, 1024) == 1          # range 1023 * 256: scale a little above 2^-8, one key per bucket
    assert U.bucket_model(d, 512) == 2
    assert U.bucket_model(np.full(97, 7, np.uint32), 512) == 97
    assert U.bucket_model(np.array([0, 0xffffffff, 0x80000000], np.uint32), 512) == 1
    assert U.bucket_model(np.zeros(0, np.uint32), 512) == 0
    # a key on a bucket's edge: the verdict would hang on the rounding, and path_of says so
    edge = np.concatenate([np.zeros(96), [256.0], [512 * 256 - 1]]).astype(np.uint32)
    assert U.bucket_model(edge, 512) == 96 and U.bucket_model(edge, 512, 1.0 - 2.0 ** -20) == 97
    with pytest.raises(AssertionError):
        U.path_of(U.make_key(edge, np.arange(98)), U.Form(256, False))


@pytest.mark.parametrize("kind", U.KINDS)
def test_generators(kind):
    rng = np.random.default_rng(3)
    for nb in (512, 1024):
        k = U.gen_keys(kind, 4096, rng, nb)
        d, ids = (k >> U.U64(32)).astype(np.int64), (k & U.U64(0xffffffff)).astype(np.int64)
        assert not (np.diff(ids) > 0).all(), "ids in ascending slot order"
        if kind == "full_range":
            assert d.min() == 0 and d.max() == 0xffffffff
        if kind == "all_equal":
            assert len(np.unique(d)) == 1
        if kind == "two_values":
            assert len(np.unique(d)) == 2
        if kind == "outlier":
            assert U.bucket_model(d, nb) == 4095
        if kind in ("fill96", "fill97"):
            m = 96 if kind == "fill96" else 97
            b = (d - d.min()) >> 8
            assert (d == d.min()).sum() == m and (b == 0).sum() == m and np.bincount(b)[1:].max() <= 9 and b.max() == nb - 1
            assert [U.bucket_model(d, nb, f) for f in U.MARGINS] == [m] * 3
        if kind == "descending":
            assert (np.diff(k.astype(object)) < 0).all()
        if kind == "ascending":
            assert (np.diff(k.astype(object)) > 0).all()


def _boundaries_classic(L, got):
    pops, kept = np.array([n for n, _k in L.specs]), L.kept
    variant = np.array([g[0] for g in got])
    path = np.array([g[1] for g in got])
    name, f = L.name, L.form
    n_big = int((kept > L.form.small_cap).sum())
    if not name.startswith("cut"):
        assert np.array_equal(pops, kept) and int(L.offsets[L.T]) <= L.capacity
    if name == "small_sizes":
        for th in (64, 256, 512):   # a wave, and the workgroup of either small variant
            assert {th - 1, th, th + 1} <= set(pops.tolist())
        assert {1023, 1025} <= set(pops.tolist())
        assert {0, 1, 2, f.threads, U.SMALL_CAP - 1, U.SMALL_CAP} <= set(pops.tolist()) and n_big == 0
        assert set(path[pops > 96]) == {"bucket", "network"}
    elif name == "small_kinds":
        assert set(path) == {"bucket", "network"} and not f.large
        assert [tuple(g[1:]) for g in got[:2]] == [("bucket", 96), ("network", 97)] and pops[0] == U.SMALL_CAP
        assert [tuple(g[1:]) for g in got[7:9]] == [("bucket", 96), ("network", 97)] and pops[7] == 300
    elif name == "small_hybrid":
        assert not f.large and set(path) == {"hybrid"} and pops.min() == U.SMALL_CAP + 1
        assert {2 * U.SMALL_CAP - 1, 2 * U.SMALL_CAP, 2 * U.SMALL_CAP + 1} <= set(pops.tolist())
    elif name == "large_bucket":
        assert f.large and set(variant) == {"large"} and set(path) == {"bucket"}
        assert {U.SMALL_CAP + 1, U.LARGE_CAP - 1, U.LARGE_CAP} <= set(pops.tolist())
    elif name == "large_network":
        assert f.large and set(variant) == {"large"} and set(path) == {"network"} and pops.max() == U.LARGE_CAP
    elif name == "large_hybrid":
        assert f.large and set(variant) == {"large"} and set(path) == {"hybrid"} and pops.min() == U.LARGE_CAP + 1
    elif name in ("handover", "t37"):
        assert f.large and {"large", f"small{f.threads}", "none"} == set(variant)
        assert set(variant[pops == 4096]) == {f"small{f.threads}"} and set(variant[pops == 4097]) == {"large"}
        assert name != "t37" or L.T == 37
    elif name.startswith("t1_"):
        assert L.T == 1 and variant[0] == ("large" if (f.large and pops[0] == 4097) else f"small{f.threads}")
        assert path[0] == ("bucket" if variant[0] == "large" or pops[0] == 4096 else "hybrid")
    elif name.startswith("list") or name.startswith("stride"):
        want_big, want_T = {"list_3_of_40": (3, 40), "list_300_of_300": (300, 300), "list_300_of_340": (300, 340),
                            "list_512_of_520": (512, 520), "stride_513_of_520": (513, 520)}[name]
        assert f.large and (n_big, L.T) == (want_big, want_T)
        assert (n_big <= U.BIG_LIST) == (not name.startswith("stride"))           # by_list, or the stride over all tiles
        if name.startswith("list_300"):
            assert n_big > min(L.T, U.LARGE_GRID)                                  # the list is walked in two rounds
        if name != "list_300_of_300":                                              # small tiles in between, some populated
            small = kept <= U.SMALL_CAP
            assert small.sum() == L.T - n_big and (kept[small] > 0).sum() >= 5
            assert name == "list_3_of_40" or (small[1:-1] & ~small[:-2] & ~small[2:]).sum() >= 7   # oversized on both sides
        if name != "list_3_of_40":
            assert kept[kept > U.SMALL_CAP].min() == 4097 and kept.max() == 4200 and set(path[kept > U.SMALL_CAP]) == {"bucket"}
    elif name.startswith("cut"):
        total = int(L.offsets[L.T])
        assert total > L.capacity and np.array_equal(L.offsets[:L.T + 1], np.concatenate([[0], np.cumsum(pops)]))
        cut = int(np.nonzero((L.offsets[:L.T] < L.capacity) & (L.offsets[1:L.T + 1] > L.capacity))[0][0])
        assert 0 < kept[cut] < pops[cut] and (L.offsets[cut + 1:L.T] > L.capacity).all() and not kept[cut + 1:].any()
        assert (pops[cut + 1:] > 0).any() and L.ends[cut] == L.capacity
        if name == "cut_small":
            assert pops[cut] <= U.SMALL_CAP
        if name == "cut_big":
            assert kept[cut] > U.SMALL_CAP and variant[cut] == ("large" if f.large else "small256")
        if name == "cut_big_to_small":
            assert pops[cut] > U.SMALL_CAP >= kept[cut] and variant[cut] == "small256" and path[cut] == "bucket"
    else:
        raise AssertionError(f"no boundary statement for {name}")


@pytest.mark.parametrize("name,hint", U.CLASSIC_RUNS)
def test_classic_case(name, hint):
    L = U.classic_case(name, hint)
    assert L.keys.size == L.capacity + U.GUARD and (L.keys[L.capacity:] == U.GUARD_KEY).all()
    assert (np.diff(L.offsets[:L.T + 1]) >= 0).all() and L.offsets[0] == 0
    got = _check_paths(L)
    _boundaries_classic(L, got)
    # the reference passes its own comparer, with and without isect_ids
    e = U.expected(L)
    for with_isect in (True, False):
        out = U.outputs_before(L, with_isect)
        out["flat"] = e["flat"].copy()
        if with_isect:
            out["isect"] = e["isect"].copy()
        U.check_sorted(L, out, e)
    record_cpu("sort_keys_cases", **U.figures(L))


@pytest.mark.parametrize("name,hint", U.SEGMENTED_RUNS)
def test_segmented_case(name, hint):
    L = U.segmented_case(name, hint)
    c = U.SEGMENTED[name]
    got = _check_paths(L)
    pops, kept, T, cap = np.array([n for n, _k in L.specs]), L.kept, L.T, L.seg_cap
    assert (T, cap) in {(40, 128), (9, 4096), (7, 5000), (3, 20000)}
    assert 0 in pops or T == 3
    assert cap in pops and (pops > cap).any() and np.array_equal(kept, np.minimum(pops, cap))
    if T in (40, 9):
        assert {127, 128, 129} <= set(pops.tolist())
    items = np.maximum(1, -(-kept // 128))
    first = np.minimum(np.cumsum(items) - items, L.max_items)
    assert np.array_equal(L.item_first[:T], first) and np.array_equal(L.cursor[:T], pops)
    assert np.array_equal(L.item_end, first + np.minimum(items, np.maximum(0, L.max_items - first)))
    if "max_items" in c:
        assert L.max_items < items.sum()
        t = int(np.nonzero(first + items > L.max_items)[0][0])
        assert 0 < L.item_end[t] - first[t] < items[t] and (L.item_end[t + 1:] == first[t + 1:]).all() and t + 1 < T
    else:
        assert L.max_items > items.sum()
    # stale slots: smaller than every real key of their tile, ids of their own
    n_stale = 0
    for t in range(T):
        stale = L.keys[int(L.ends[t]):(t + 1) * cap]
        n_stale += stale.size
        if kept[t] and stale.size:
            assert stale.max() < L.segment_keys(t).min()
        assert np.isin(stale & U.U64(0xffffffff), L.stale_ids).all()
        assert not np.isin(L.segment_keys(t) & U.U64(0xffffffff), L.stale_ids).any()
    assert n_stale == L.stale_ids.size == T * cap - kept.sum()
    variants = {g[0] for g in got}
    if cap > U.SMALL_CAP:
        assert ("large" in variants) == L.form.large
    e = U.expected(L)
    out = U.outputs_before(L)
    out.update({k: e[k].copy() for k in ("flat", "tile_start", "tile_end", "item_end", "item_tile", "cursor")})
    U.check_sorted(L, out, e)
    record_cpu("sort_keys_cases", **U.figures(L))


# ---------------------------------------------------------------------------------------------------
# planted defects: what check_sorted must reject
def _toy_classic():
    L = U.build_classic("toy", [(6, "all_equal"), (9, "spread"), (0, "spread"), (5, "two_values")], 1000, seed=1, edge_ids=False)
    e = U.expected(L)
    out = U.outputs_before(L)
    out["flat"], out["isect"] = e["flat"].copy(), e["isect"].copy()
    U.check_sorted(L, out, e)
    return L, out


def _toy_segmented():
    L = U.build_segmented("toy_seg", 4, 16, [(6, "all_equal"), (16, "spread"), (0, "spread"), (40, "two_values")], 0, seed=2)
    e = U.expected(L)
    out = U.outputs_before(L)
    out.update({k: e[k].copy() for k in ("flat", "tile_start", "tile_end", "item_end", "item_tile", "cursor")})
    U.check_sorted(L, out, e)
    return L, out


def _swap_equal_depth_neighbours(L, o):
    a = int(L.starts[0])   # tile 0: one depth, the order is by id alone
    o["flat"][[a + 2, a + 3]] = o["flat"][[a + 3, a + 2]]


def _last_key_missing(L, o):
    o["flat"][int(L.ends[1]) - 1] = U.SENT


def _key_in_the_next_tiles_first_slot(L, o):
    o["flat"][int(L.starts[1])] = o["flat"][int(L.ends[0]) - 1]


def _isect_tile_off_by_one(L, o):
    o["isect"][int(L.starts[1]):int(L.ends[1])] += np.int64(1) << np.int64(32)


def _flat_guard(L, o):
    o["flat"][L.capacity + 1] = 0


def _key_guard(L, o):
    o["keys"][L.capacity] ^= U.U64(1)


def _isect_guard(L, o):
    o["isect"][-1] = 0


def _slack_key(L, o):
    o["keys"][L.capacity - 1] = U.U64(0)


def _offsets_written(L, o):
    o["offsets"][1] += 1


def _stale_id_in_place_of_a_key(L, o):
    o["flat"][int(L.starts[0])] = int(L.keys[int(L.ends[0])] & U.U64(0xffffffff))


def _stale_id_behind_the_population(L, o):
    o["flat"][int(L.ends[0])] = int(L.keys[int(L.ends[0])] & U.U64(0xffffffff))


def _stale_slot_rewritten(L, o):
    o["keys"][int(L.ends[0]) + 1] = U.GUARD_KEY


def _table(name, i, v):
    def f(L, o):
        o[name][i] = v
    f.__name__ = f"{name}_{i}_{v}"
    return f


CLASSIC_DEFECTS = [_swap_equal_depth_neighbours, _last_key_missing, _key_in_the_next_tiles_first_slot, _isect_tile_off_by_one,
                   _flat_guard, _key_guard, _isect_guard, _slack_key, _offsets_written]
SEGMENTED_DEFECTS = [_swap_equal_depth_neighbours, _last_key_missing, _key_in_the_next_tiles_first_slot, _flat_guard, _key_guard,
                     _stale_id_in_place_of_a_key, _stale_id_behind_the_population, _stale_slot_rewritten,
                     _table("cursor", 3, 40), _table("tile_start", 2, 0), _table("tile_end", 3, 3 * 16 + 40),
                     _table("item_end", 0, 2), _table("item_tile", 1, 0), _table("item_tile", 4, 3), _table("tile_end", 4, 0)]


@pytest.mark.parametrize("defect", CLASSIC_DEFECTS, ids=lambda f: f.__name__.strip("_"))
def test_planted_defect_classic(defect):
    L, out = _toy_classic()
    defect(L, out)
    with pytest.raises(AssertionError):
        U.check_sorted(L, out)


@pytest.mark.parametrize("defect", SEGMENTED_DEFECTS, ids=lambda f: f.__name__.strip("_"))
def test_planted_defect_segmented(defect):
    L, out = _toy_segmented()
    assert L.item_end.tolist() == [1, 2, 3, 4] and L.max_items == 7   # (item_tile[4] is behind the last item)
    defect(L, out)
    with pytest.raises(AssertionError):
        U.check_sorted(L, out)
