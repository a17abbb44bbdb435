"""Hand-written keys, layouts and the exact reference for the tile sort (csrc/binning.hip, tile_sort_kernel), numpy only.

The sort's outputs are functions of its integer inputs: inside every segment `flatten_ids` / `isect_ids` are those of
np.sort of the segment's uint64 keys (ref_sort), everything else keeps what it held.  tests/test_gpu_sort_keys.py runs
the cases below through eg_sort_pairs / eg_sort_segments and compares with check_sorted; tests/test_sort_host.py checks
on the CPU that every case sits on the boundary it is named for, that the path it is meant to take (bucket + rank, the
in-LDS network, the hybrid network) follows from bucket_model with a margin, and that check_sorted rejects planted defects.

Precondition of the kernel (asserted by every builder): the keys of a segment are unique, none is all ones, ids <= 0x7fffffff.
"""
import dataclasses

import numpy as np

U64 = np.uint64
SMALL_CAP, LARGE_CAP = 4096, 16384   # kSmall, kLarge of launch_tile_sort
MAX_FILL = 96                        # kMaxBucketFill
SORT_BM = 2                          # kSortBM: buckets per thread of the small variants
LARGE_NB = 1024                      # buckets of the large variant
BIG_LIST = 512                       # kBigList
LARGE_GRID = 256                     # workgroups of the large variant: min(T, 256)
SLICE = 128                          # keys per item
GUARD = 64                           # words behind every buffer
SENT = -7                            # pre-fill of every output: no id, tile, range or item number is negative
GUARD_KEY = U64(0xA5A5A5A55A5A5A5A)  # key guards
SLACK_KEY = U64(0x3C3C3C3CC3C3C3C3)  # key slots below `capacity` that no segment owns
REAL_ID0 = 1 << 20                   # real ids are >= this (classic layouts may add 0 and 0x7fffffff) ...
STALE_ID0 = 1                        # ... and the ids of stale slots below it: they may appear in no output
HINTS = (0, 1000, 2000, 4000)


def make_key(depth_bits, gid):
    return (np.asarray(depth_bits).astype(U64) << U64(32)) | np.asarray(gid).astype(U64)


def ref_sort(keys, starts, ends, tiles):
    """per segment: the sorted keys, their ids (flatten_ids) and (tile << 32) | depth bits (isect_ids)"""
    ks, ids, isect = [], [], []
    for a, b, t in zip(starts, ends, tiles):
        k = np.sort(keys[int(a):int(b)])
        ks.append(k)
        ids.append((k & U64(0xffffffff)).astype(np.int64).astype(np.int32))
        isect.append((np.int64(t) << np.int64(32)) | (k >> U64(32)).astype(np.int64))
    return ks, ids, isect


# ---------------------------------------------------------------------------------------------------
# the launch (launch_tile_sort, one view, no "prefix here" tables)
@dataclasses.dataclass(frozen=True)
class Form:
    threads: int    # workgroup of the small variant
    large: bool     # the large variant is launched; else the small one owns every tile

    @property
    def nb(self):
        return SORT_BM * self.threads

    @property
    def small_cap(self):
        return SMALL_CAP if self.large else 0x7fffffff


_FORMS = {0: Form(256, True), 1000: Form(256, False), 2000: Form(512, False), 4000: Form(512, True)}


def launch_form(T, hint, segmented=False):
    """the table of the four hints; above 4096 tiles the small variant keeps 256 threads.  (The segmented layout of
    eg_sort_segments takes the same launch: pairs and the three-batch prefix need the "prefix here" tables.)"""
    f = _FORMS[hint]
    return dataclasses.replace(f, threads=256) if T > 4096 else f


def owner_nb(n, form):
    """buckets of the variant that sorts a tile of n keys"""
    return LARGE_NB if (form.large and n > SMALL_CAP) else form.nb


def bucket_model(depth_bits, NB, scale_factor=1.0):
    """the kernel's fp32 map depth -> bucket: the largest bucket fill"""
    d = np.asarray(depth_bits, dtype=np.uint32)
    if d.size == 0:
        return 0
    dmin, dmax = d.min(), d.max()
    scale = np.float32(NB) / (np.float32(np.uint32(dmax - dmin)) + np.float32(1.0))
    scale = np.float32(scale * np.float32(scale_factor))
    b = np.minimum(NB - 1, ((d - dmin).astype(np.float32) * scale).astype(np.int64))
    return int(np.bincount(b, minlength=NB).max())


MARGINS = (1.0, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20)


def path_of(keys, form):
    """(variant, path, largest fill) of one tile; the path must not depend on how the device rounds `scale`"""
    n = len(keys)
    if n == 0:
        return "none", "empty", 0
    large = form.large and n > SMALL_CAP
    cap, nb = (LARGE_CAP, LARGE_NB) if large else (SMALL_CAP, form.nb)
    variant = "large" if large else f"small{form.threads}"
    if n > cap:
        return variant, "hybrid", 0
    fills = [bucket_model(keys >> U64(32), nb, m) for m in MARGINS]
    verdicts = {f <= MAX_FILL for f in fills}
    assert len(verdicts) == 1, f"the path of a tile of {n} keys hangs on the rounding of one division: fills {fills}"
    return variant, ("bucket" if fills[0] <= MAX_FILL else "network"), fills[0]


# ---------------------------------------------------------------------------------------------------
# depth bits and ids
KINDS = ("spread", "full_range", "all_equal", "two_values", "outlier", "fill96", "fill97", "descending", "ascending")


def gen_depths(kind, n, rng, nb):
    if n == 0:
        return np.zeros(0, np.uint32)
    base = 0x40000000 + int(rng.integers(0, 1 << 20))   # floats a little above 2.0
    if kind in ("spread", "descending", "ascending"):    # a narrow range, like a real tile's
        d = base + rng.integers(0, 1 << 20, n)
    elif kind == "full_range":                           # dmax - dmin + 1 is 2^32 in fp32
        assert n >= 2
        d = rng.integers(0, 1 << 32, n)
        d[rng.choice(n, 2, replace=False)] = (0, 0xffffffff)
    elif kind == "all_equal":
        d = np.full(n, base)
    elif kind == "two_values":
        assert n >= 2
        d = np.where(rng.random(n) < 0.5, base, base + 12345)
        d[0], d[-1] = base, base + 12345
    elif kind == "outlier":                              # one far key squeezes the others into bucket 0
        assert n >= 2
        d = base + rng.integers(0, 256, n)
        d[int(rng.integers(n))] = base + (1 << 31)
    elif kind in ("fill96", "fill97"):
        # m keys at dmin; the range is nb * 256 - 1, so scale is 2^-8 exactly and bucket = offset >> 8; the others sit
        # near the middle of buckets 1 .. nb - 1, dealt round robin, and one at the range's end
        m = 96 if kind == "fill96" else 97
        rest = n - m
        assert rest >= 1
        off = (1 + np.arange(rest) % (nb - 1)) * 256 + 128 + rng.integers(-32, 33, rest)
        off[0] = nb * 256 - 1
        d = base + rng.permutation(np.concatenate([np.zeros(m, np.int64), off]))
    else:
        raise ValueError(kind)
    assert d.min() >= 0 and d.max() <= 0xffffffff
    return d.astype(np.uint32)


def gen_ids(n, rng, edge=False):
    """a random permutation of n consecutive ids, never in the slots' ascending order; edge: the ids 0 and 0x7fffffff among
    them (classic layouts only: the stale slots of a segmented one use the ids below REAL_ID0)"""
    ids = REAL_ID0 + int(rng.integers(0, 1 << 29)) + rng.permutation(n).astype(np.int64)
    if edge and n >= 2:
        ids[rng.choice(n, 2, replace=False)] = (0, 0x7fffffff)
    if n >= 2 and (np.diff(ids) > 0).all():
        ids = ids[::-1].copy()
    return ids


def gen_keys(kind, n, rng, nb, edge=False):
    keys = make_key(gen_depths(kind, n, rng, nb), gen_ids(n, rng, edge))
    if kind == "descending":
        keys = np.sort(keys)[::-1].copy()
    elif kind == "ascending":
        keys = np.sort(keys)
    assert_precondition(keys)
    return keys


def assert_precondition(keys):
    assert len(np.unique(keys)) == len(keys), "keys of a segment must be unique"
    assert not (keys == U64(0xffffffffffffffff)).any() and ((keys & U64(0xffffffff)) <= U64(0x7fffffff)).all()


# ---------------------------------------------------------------------------------------------------
# layouts
@dataclasses.dataclass
class Layout:
    name: str
    hint: int
    form: Form
    T: int
    specs: list            # (population, kind) per tile
    capacity: int          # key slots (classic: the `capacity` argument; segmented: T * seg_cap)
    keys: np.ndarray       # uint64 [capacity + GUARD]
    starts: np.ndarray     # int64 [T]: the segment the sort has to order ...
    ends: np.ndarray       # ... after truncation by capacity / seg_cap
    offsets: np.ndarray = None      # classic: int32 [T + 1 + GUARD]
    seg_cap: int = 0                # segmented from here on
    cursor: np.ndarray = None       # int32 [T + GUARD]: the populations (may exceed seg_cap)
    item_first: np.ndarray = None   # int32 [T + GUARD]
    item_end: np.ndarray = None     # int64 [T]: expected
    max_items: int = 0
    stale_ids: np.ndarray = None

    @property
    def kept(self):
        return self.ends - self.starts

    def segment_keys(self, t):
        return self.keys[int(self.starts[t]):int(self.ends[t])]

    def paths(self):
        return [path_of(self.segment_keys(t), self.form) for t in range(self.T)]


def _guarded(a, fill, dtype):
    return np.concatenate([np.asarray(a, dtype=dtype), np.full(GUARD, fill, dtype=dtype)])


def build_classic(name, specs, hint, seed, capacity=None, slack=5, edge_ids=True):
    """keys laid out by offsets[T + 1]; capacity < offsets[T] truncates: only the first `capacity` keys exist"""
    T = len(specs)
    form = launch_form(T, hint)
    rng = np.random.default_rng(seed)
    pops = np.array([n for n, _k in specs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(pops)])
    assert offs[-1] < 2 ** 31
    capacity = int(offs[-1]) + slack if capacity is None else int(capacity)
    starts, ends = np.minimum(offs[:-1], capacity), np.minimum(offs[1:], capacity)
    keys = np.full(capacity + GUARD, GUARD_KEY, dtype=U64)
    keys[:capacity] = SLACK_KEY
    for t, (n, kind) in enumerate(specs):
        k = int(ends[t] - starts[t])   # the keys a truncated tile stores
        if k > 0:
            # (built for the variant that sorts the TRUNCATED tile; a tile the cut moves below 4097 keys changes owner)
            keys[starts[t]:starts[t] + k] = gen_keys(kind, n, rng, owner_nb(k, form), edge=edge_ids and t % 3 == 0)[:k]
    return Layout(name, hint, form, T, list(specs), capacity, keys, starts, ends, offsets=_guarded(offs, SENT, np.int32))


def build_segmented(name, T, seg_cap, specs, hint, seed, max_items=None):
    """tile t owns keys[t * seg_cap ...), its population sits in cursor[t] (above seg_cap: only seg_cap keys were stored),
    item_first is what the scan of eg_project_emit leaves; slots behind a population hold stale keys SMALLER than the
    tile's real ones, with ids of their own"""
    assert len(specs) == T
    form = launch_form(T, hint, segmented=True)
    rng = np.random.default_rng(seed)
    pops = np.array([n for n, _k in specs], dtype=np.int64)
    kept = np.minimum(pops, seg_cap)
    starts = np.arange(T, dtype=np.int64) * seg_cap
    keys = np.full(T * seg_cap + GUARD, GUARD_KEY, dtype=U64)
    stale_next = STALE_ID0
    for t, (n, kind) in enumerate(specs):
        k = int(kept[t])
        real = gen_keys(kind, k, rng, owner_nb(k, form))
        keys[starts[t]:starts[t] + k] = real
        ns = seg_cap - k
        dmin = int(real.min() >> U64(32)) if k else 0xffffffff
        stale = make_key(rng.integers(0, dmin + 1, ns), stale_next + np.arange(ns))
        stale_next += ns
        assert k == 0 or ns == 0 or stale.max() < real.min()
        keys[starts[t] + k:starts[t] + seg_cap] = stale
    assert stale_next <= REAL_ID0
    items = np.maximum(1, (kept + SLICE - 1) // SLICE)
    total = int(items.sum())
    max_items = total + 3 if max_items is None else int(max_items)
    first = np.minimum(np.cumsum(items) - items, max_items)
    item_end = first + np.minimum(items, np.maximum(0, max_items - first))
    return Layout(name, hint, form, T, list(specs), T * seg_cap, keys, starts, starts + kept, seg_cap=seg_cap,
                  cursor=_guarded(pops, SENT, np.int32), item_first=_guarded(first, SENT, np.int32), item_end=item_end,
                  max_items=max_items, stale_ids=np.arange(STALE_ID0, stale_next))


# ---------------------------------------------------------------------------------------------------
# what the sort must leave, and the comparer
def expected(L):
    """everything the outputs must equal, guards included; `inside`: the key slots the sort may rewrite"""
    n = L.capacity + GUARD
    flat, isect = np.full(n, SENT, np.int32), np.full(n, SENT, np.int64)
    inside = np.zeros(n, bool)
    _ks, ids, isc = ref_sort(L.keys, L.starts, L.ends, range(L.T))
    for t in range(L.T):
        a, b = int(L.starts[t]), int(L.ends[t])
        flat[a:b], isect[a:b], inside[a:b] = ids[t], isc[t], True
    e = dict(flat=flat, isect=isect, inside=inside)
    if L.seg_cap:
        T = L.T
        first = L.item_first[:T].astype(np.int64)
        item_tile = np.full(L.max_items + GUARD, SENT, np.int32)
        for t in range(T):
            item_tile[first[t]:L.item_end[t]] = t
        e.update(tile_start=_guarded(L.starts, SENT, np.int32), tile_end=_guarded(L.ends, SENT, np.int32),
                 item_end=_guarded(L.item_end, SENT, np.int32), item_tile=item_tile,
                 cursor=_guarded(np.zeros(T), SENT, np.int32), item_first=L.item_first)
    return e


def outputs_before(L, with_isect=True):
    """the buffers a call starts from (numpy): outputs pre-filled with the sentinel"""
    n = L.capacity + GUARD
    o = dict(keys=L.keys.copy(), flat=np.full(n, SENT, np.int32))
    if L.seg_cap:
        o.update(cursor=L.cursor.copy(), item_first=L.item_first.copy(),
                 item_tile=np.full(L.max_items + GUARD, SENT, np.int32),
                 **{k: np.full(L.T + GUARD, SENT, np.int32) for k in ("tile_start", "tile_end", "item_end")})
    else:
        o["offsets"] = L.offsets.copy()
        if with_isect:
            o["isect"] = np.full(n, SENT, np.int64)
    return o


def _where(L, i):
    t = int(np.searchsorted(L.starts, i, side="right")) - 1
    if i >= L.capacity:
        return f"guard word {i - L.capacity}"
    if t >= 0 and L.starts[t] <= i < L.ends[t]:
        return f"slot {i - int(L.starts[t])} of tile {t} ({L.specs[t][0]} keys, {L.specs[t][1]}, {L.paths()[t][:2]})"
    return f"slot {i}, outside every segment (behind tile {t})"


def check_sorted(L, out, exp=None):
    """bit-exact, nothing excluded: `out` maps buffer names to what the device left (numpy, guards included)"""
    e = expected(L) if exp is None else exp
    who = f"{L.name}, hint {L.hint}"
    flat = out["flat"]
    if L.stale_ids is not None and L.stale_ids.size:
        hit = np.isin(flat, L.stale_ids)
        assert not hit.any(), f"{who}: the id of a stale slot appears in flatten_ids at {_where(L, int(np.argmax(hit)))}"
    names = ["flat"] + (["isect"] if out.get("isect") is not None else [])
    for nm in names:
        bad = out[nm] != e[nm]
        if bad.any():
            i = int(np.argmax(bad))
            raise AssertionError(f"{who}: {nm} differs in {int(bad.sum())} words, first at {_where(L, i)}: "
                                 f"{int(out[nm][i]):#x} instead of {int(e[nm][i]):#x}")
    bad = (out["keys"] != L.keys) & ~e["inside"]
    assert not bad.any(), f"{who}: a key outside every segment lost its bits at {_where(L, int(np.argmax(bad)))}"
    if L.seg_cap:
        for nm in ("tile_start", "tile_end", "item_end", "item_tile", "cursor", "item_first"):
            bad = out[nm] != e[nm]
            assert not bad.any(), (f"{who}: {nm} differs in {int(bad.sum())} words, first at {int(np.argmax(bad))}: "
                                   f"{int(out[nm][int(np.argmax(bad))])} instead of {int(e[nm][int(np.argmax(bad))])}")
    else:
        assert np.array_equal(out["offsets"], L.offsets), f"{who}: offsets were written"


def figures(L):
    """per case: keys, tiles per (variant, path), the model's largest fill per path"""
    f = dict(case=L.name, hint=L.hint, tiles=L.T, keys=int(L.kept.sum()), largest_tile=int(L.kept.max(initial=0)))
    for variant, path, fill in L.paths():
        if path != "empty":
            k = f"{variant}_{path}"
            f[k] = f.get(k, 0) + 1
            if path != "hybrid":
                f[k + "_max_fill"] = max(f.get(k + "_max_fill", 0), fill)
    return f


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_sort_keys.py
SMALL_N = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 4095, 4096)
SMALL_HYBRID_N = (4097, 8191, 8192, 8193, 12289, 16385, 20000)
LARGE_N = (4097, 5000, 16383, 16384)
LARGE_HYBRID_N = (16385, 32768, 32769, 40000)


def _big(i):
    return 4097 + (i * 7) % 104   # 4097 .. 4200 keys


def _list_case(T, is_small):
    return [((i * 13) % 900, "spread") if is_small(i) else (_big(i), "spread") for i in range(T)]


CLASSIC = {
    # ---- the small variant alone (hint 1000: 256 threads, hint 2000: 512 threads)
    "small_sizes": dict(hints=(1000, 2000), tiles=[(n, k) for n in SMALL_N for k in ("spread", "all_equal")]),
    "small_kinds": dict(hints=(1000, 2000), tiles=[(4096, k) for k in ("fill96", "fill97", "outlier", "full_range", "descending",
                                                                       "ascending", "two_values")]
                        + [(300, "fill96"), (300, "fill97"), (2, "two_values"), (2, "full_range"), (1000, "two_values")]),
    "small_hybrid": dict(hints=(1000, 2000), tiles=[(n, k) for n in SMALL_HYBRID_N for k in ("spread", "all_equal", "descending")]),
    # ---- the large variant (hint 0: behind 256 threads, hint 4000: behind 512)
    "large_bucket": dict(hints=(0, 4000), tiles=[(n, "spread") for n in LARGE_N] + [(16384, "full_range"), (16384, "fill96")]),
    "large_network": dict(hints=(0, 4000), tiles=[(n, k) for n in LARGE_N for k in ("all_equal", "fill97", "outlier")]),
    "large_hybrid": dict(hints=(0, 4000), tiles=[(n, k) for n in LARGE_HYBRID_N for k in ("spread", "descending")]),
    # ---- who owns a tile
    "handover": dict(hints=(0, 4000), tiles=[(4096, "spread"), (4097, "spread"), (0, "spread"), (0, "spread"), (4097, "all_equal"),
                                             (4096, "all_equal"), (0, "spread"), (4096, "fill97"), (4097, "fill97"),
                                             (4096, "fill96"), (4097, "fill96")]),
    "t1_4096": dict(hints=HINTS, tiles=[(4096, "spread")]),
    "t1_4097": dict(hints=HINTS, tiles=[(4097, "spread")]),
    "t37": dict(hints=(0,), tiles=[[(4096, "spread"), (4097, "spread"), (0, "spread"), (100, "spread"), (4097, "all_equal"),
                                    (1, "spread"), (5000, "spread")][i % 7] for i in range(37)]),
    # ---- the large variant's list of oversized tiles (kBigList = 512 entries, min(T, 256) workgroups)
    "list_3_of_40": dict(hints=(0, 4000), tiles=[{5: (4097, "spread"), 17: (9000, "spread"), 39: (16385, "spread")}.get(
        i, ((i * 37) % 700, "spread")) for i in range(40)]),
    "list_300_of_300": dict(hints=(0,), tiles=_list_case(300, lambda i: False)),
    "list_300_of_340": dict(hints=(0, 4000), tiles=_list_case(340, lambda i: i % 17 in (3, 11))),
    "list_512_of_520": dict(hints=(0,), tiles=_list_case(520, lambda i: i % 65 == 7)),
    "stride_513_of_520": dict(hints=(0,), tiles=_list_case(520, lambda i: i % 65 == 7 and i != 7)),
    # ---- offsets[T] > capacity: the cut tile keeps its first capacity - start keys, the tiles behind it write nothing
    "cut_small": dict(hints=(0, 1000), capacity=300 + 5000 + 350,
                      tiles=[(300, "spread"), (5000, "spread"), (700, "spread"), (200, "spread"), (4500, "spread"), (0, "spread"),
                             (50, "all_equal")]),
    "cut_big": dict(hints=(0, 1000), capacity=900 + 4500,
                    tiles=[(300, "spread"), (600, "all_equal"), (6000, "spread"), (200, "spread"), (4500, "spread")]),
    "cut_big_to_small": dict(hints=(0, 1000), capacity=900 + 3000,   # the cut hands an oversized tile to the small variant
                             tiles=[(300, "spread"), (600, "all_equal"), (6000, "spread"), (200, "spread"), (4500, "spread")]),
}

_S40 = [(0, "spread"), (1, "spread"), (2, "all_equal"), (63, "spread"), (64, "all_equal"), (65, "spread"), (127, "spread"),
        (128, "spread"), (129, "spread"), (255, "all_equal"), (128, "fill96"), (128, "fill97"), (128, "all_equal"),
        (300, "spread"), (0, "spread"), (96, "all_equal"), (97, "all_equal"), (128, "outlier"), (128, "full_range"),
        (128, "descending"), (128, "ascending"), (100, "two_values")] + [((7 * i) % 129, "spread") for i in range(18)]
_S9 = [(0, "spread"), (127, "spread"), (128, "spread"), (129, "spread"), (1023, "all_equal"), (4095, "spread"), (4096, "spread"),
       (5000, "spread"), (4096, "fill97")]
_S7 = [(4096, "spread"), (4097, "spread"), (5000, "spread"), (6000, "all_equal"), (0, "spread"), (300, "fill96"), (4999, "outlier")]
_S3 = [(16384, "spread"), (20000, "spread"), (25000, "descending")]

SEGMENTED = {
    "seg_40_128": dict(T=40, seg_cap=128, tiles=_S40),
    "seg_9_4096": dict(T=9, seg_cap=4096, tiles=_S9),
    "seg_7_5000": dict(T=7, seg_cap=5000, tiles=_S7),
    "seg_3_20000": dict(T=3, seg_cap=20000, tiles=_S3),
    # max_items below the item total: the clip falls inside tile 6 (32 items), tiles 7 and 8 keep none
    "seg_9_4096_clip": dict(T=9, seg_cap=4096, tiles=_S9, max_items=1 + 1 + 1 + 2 + 8 + 32 + 5),
}

CLASSIC_RUNS = [(name, h) for name, c in CLASSIC.items() for h in c["hints"]]
SEGMENTED_RUNS = [(name, h) for name in SEGMENTED for h in HINTS]


def _seed(name, hint):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 4 + HINTS.index(hint)


def classic_case(name, hint):
    c = CLASSIC[name]
    return build_classic(name, c["tiles"], hint, _seed(name, hint), capacity=c.get("capacity"))


def segmented_case(name, hint):
    c = SEGMENTED[name]
    return build_segmented(name, c["T"], c["seg_cap"], c["tiles"], hint, _seed(name, hint), max_items=c.get("max_items"))
