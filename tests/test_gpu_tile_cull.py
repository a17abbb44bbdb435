"""The training path's tile cull per (Gaussian, tile) pair: every kernel that evaluates tile_box_tight / splat_hits_tile
(csrc/common.h) or consumes the <= 32-tile mask, against the float64 references of tests/cull_util.py evaluated from the
device's OWN fp32 records (the cases, the references' tightness, the fp32 model and its planted defects are checked on
the CPU by tests/test_cull_host.py).

Assertions per producer: (1) must_keep <= emitted, no allowance, no excluded row; (2) emitted <= may_keep <= box, no pair
twice; (3) may_keep exceeds must_keep by at most 3 % (references alone; `grazing` counts its sides instead); (4)
tiles_per_gauss, tile_counts, cursor populations, total[0], total[3] and tile_mask bit-exact against the emitted set; (5)
the producers emit the same set and write the same records.

Which test reaches which kernel instantiation:

  project_fwd_kernel<LDS_COUNT = true>   (eg_project_fwd with tiles_per_gauss + tile_counts; eg_project_bin with the mask
                                          and the fused scan)   test_producers[every case up to 16 384 tiles]
  project_fwd_kernel<false>              (T = 16 641)           test_producers[grid_2064]
  tile_emit_kernel<LDS = true>, mask     (eg_tile_emit)         test_producers[every case up to 8192 tiles]
  tile_emit_kernel<true>, re-test        (tile_mask = NULL)     the same, and test_emit_from_hand_made_records (records no
                                                                projection writes: exact grazing ratios, det <= 0, radius 0)
  tile_emit_kernel<false>, mask / re-test (2 T > 16 384)        test_producers[grid_1456 | grid_2064 | grid_1456_n65537]
  project_emit_kernel<LDS_HIST = true, 256>                     test_producers[N <= 65 536, up to 8192 tiles]
  project_emit_kernel<true, 512>          (pe_small false)      test_producers[n65537]
  project_emit_kernel<false, 256>                               test_producers[grid_1456 | grid_2064]
  project_emit_kernel<false, 512>                               test_producers[grid_1456_n65537]
  adam_emit kernel<LDS, 256>  (EdgeTrainer.apply_adam(next_view)) test_tail_of_apply_adam[4000 | 33000]
  adam_emit kernel<LDS, 512>                                    test_tail_of_apply_adam[65537]
  backward_fused.hip's tail   (eg_backward_is_fused == 1)       test_tail_of_a_run_of_steps[4000]
  project_bwd_emit_kernel<LDS, HOIST, 256> (is_fused == 0)      test_tail_of_a_run_of_steps[33000]
  project_bwd_emit_kernel<LDS, HOIST, 512>                      test_tail_of_a_run_of_steps[65537]
  project_emit_kernel<LDS, 512>, gridDim.y = 2 views            test_batched_projection
  quad_hit / quad_hit_staged / hitq[] (8 x 8 quadrants)         the `grazing` forward case of tests/test_gpu_step_composite.py

Not reached: the no-LDS forms (more than 8192 tiles) of the adam_emit kernel, of project_bwd_emit_kernel and their
HOIST = false forms (above 160 000 Gaussians); EG_FLAG_FRONT_PREFIX (grids above 2560 tiles inside a trainer).  They inline the same
emit_body / splat_hits_tile source.

The tails are compared with eg_project_emit on the parameters read back: the records bit for bit, the pair sets equal,
and that set against the float64 references.  test_tail_of_a_run_of_steps reads the parameters after step 0 from a
second trainer that runs step 0 alone (the two backward forms give the same parameters bit for bit:
tests/test_gpu_parity.py); the record comparison would show a difference.

Measured on the MI355X (recorded per case through tests.util.record as tile_cull_producers / tile_cull_hand_made /
tile_cull_tails; box / must_keep / may_keep / emitted, largest band of a may_keep pair at BAND_FACTOR = 4):
  thin 156 617 / 14 442 / 14 612 / 14 612, 0.013      grazing 10 720 / 1 690 / 1 833 / 1 821, 0.005
  mask_a 1 028 / 381 / 381 / 381    mask_b 204 / 64 / 64 / 64    mask_c 594 / 226 / 226 / 226    dead 1 554 / 0 / 0 / 0
  n1 72 / 5 / 5 / 5    n255 9 825 / 1 012 / 1 020 / 1 020    n256 9 245 / 922 / 934 / 934    n257 9 410 / 950 / 961 / 961
  n511 19 972 / 1 921 / 1 953 / 1 953    n513 20 488 / 2 019 / 2 034 / 2 034    n65537 76 242 / 7 116 / 7 179 / 7 178, 0.012
  grid_1456 and grid_1456_n65537 49 136 / 2 060 / 2 091 / 2 091, 0.020    grid_2064 45 806 / 1 777 / 1 786 / 1 786, 0.028
  the tails (apply_adam and the run of steps alike): 156 644 / 14 395 / 14 552 / 14 552 at 4000 rows, 14 387 / 14 541 /
  14 541 at 33 000, 14 390 / 14 543 / 14 543 at 65 537; the batched views 14 442 / 14 612 / 14 612 and 14 431 / 14 605 / 14 603
No must_keep pair was dropped and no pair outside may_keep was kept anywhere; no row needed the second reading of its tight
box; through the projection no emitted pair needed any band at all.  On the hand-made records (`thin` 14 693 pairs,
`grazing` 1 831) the device kept exactly the pairs of the fp32 numpy model, and like it needed a band factor of 0.089 on
`grazing`.  Through the device's projection the designed grazing ratios are met on the designed side for every row up to
k = 3 and for all but the long_diag rows at k = 4, 5 (there the conic's cancellation moves the ratio by more than 1e-4; the
hand-made records hold those exactly).

The first run of test_producers found that eg_tile_offsets counted one item for each of its 1024 - T % 1024 idle threads
into item_offsets[T] and total[2] (1083 against the fused scan's 176 on the 117-tile grid); csrc/binning.hip now counts
none.  The tile cull itself needed no change.
"""
import math

import numpy as np
import pytest
import torch

from tests import cull_util as U
from tests.util import record

pytestmark = pytest.mark.gpu

FLAGS = 1 | 2 | 4 | 8          # log-scales, logit opacities, antialiased, tight tiles
FILL = -1                      # keys are pre-filled with all ones: an id of 0xffffffff is a slot nobody wrote


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    assert FLAGS == _lib.FLAG_LOG_SCALES | _lib.FLAG_LOGIT_OPACITIES | _lib.FLAG_ANTIALIASED | _lib.FLAG_TIGHT_TILES
    return _lib


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()


def _zeros(n, dtype=torch.int32):
    return torch.zeros(n, dtype=dtype, device="cuda")


class _Scene:
    def __init__(self, p, view=0, tensors=None):
        self.W, self.H, self.N = p.W, p.H, p.means.shape[0]
        self.tw, self.th = U.tiles_of(p.W, p.H)
        self.T = self.tw * self.th
        self.t = tensors if tensors is not None else [_dev(p.means), _dev(p.quats), _dev(p.log_scales), _dev(p.logit_opacities)]
        self.vm, self.K = _dev(p.viewmats[view]), _dev(p.Ks[view])

    def args(self):
        from edgegaussians_amd._lib import ptr
        return [ptr(t) for t in self.t] + [ptr(self.vm), ptr(self.K), self.N, self.W, self.H]


def _ids_and_depths(keys):
    k = keys.astype(np.int64)
    return k & 0xFFFFFFFF, (k >> 32) & 0xFFFFFFFF


def _check_keys(ids, depths, rec, name):
    assert (ids < rec.shape[0]).all(), f"{name}: a slot inside a tile's population was never written"
    want = np.ascontiguousarray(rec[:, 6]).view(np.uint32).astype(np.int64)[ids]
    assert np.array_equal(depths, want), f"{name}: a key does not carry its Gaussian's depth bits"


def _project_fwd(sc):
    from edgegaussians_amd._lib import call, ptr, stream
    splat = torch.full((sc.N, 8), float("nan"), device="cuda")
    tpg, counts = torch.full((sc.N,), -7, dtype=torch.int32, device="cuda"), _zeros(sc.T)
    call("eg_project_fwd", *sc.args(), 0.01, 1e10, 0.3, 0.0, FLAGS, ptr(splat), None, None, None, None, None, ptr(tpg),
         ptr(counts), None, stream())
    torch.cuda.synchronize()
    return splat.cpu().numpy(), tpg.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64)


def _classic_pairs(keys, offsets, rec, T, name):
    offs = offsets.astype(np.int64)
    assert offs[0] == 0 and (np.diff(offs) >= 0).all()
    ids, depths = _ids_and_depths(keys[:offs[-1]])
    _check_keys(ids, depths, rec, name)
    return ids * T + np.repeat(np.arange(T), np.diff(offs))


def _project_bin_emit(sc, name):
    """eg_project_bin, eg_tile_offsets, eg_tile_emit with the mask and with tile_mask = NULL"""
    from edgegaussians_amd._lib import call, ptr, stream
    splat = torch.full((sc.N, 8), float("nan"), device="cuda")
    counts, mask = _zeros(sc.T), torch.full((sc.N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    offsets, item_offsets, total, ticket = _zeros(sc.T + 1), _zeros(sc.T + 1), _zeros(4), _zeros(1)
    call("eg_project_bin", *sc.args(), FLAGS, ptr(splat), ptr(counts), ptr(mask), 1 << 30, ptr(offsets), ptr(item_offsets),
         ptr(total), ptr(ticket), stream())
    torch.cuda.synchronize()
    assert int(ticket[0]) == 0, "the scan's ticket is handed back zeroed"
    tot = total.cpu().numpy().astype(np.int64)
    pops = counts.cpu().numpy().astype(np.int64)
    offs2, items2, total2 = _zeros(sc.T + 1), _zeros(sc.T + 1), _zeros(4)
    call("eg_tile_offsets", ptr(counts), sc.T, 1 << 30, ptr(offs2), ptr(items2), ptr(total2), stream())
    torch.cuda.synchronize()
    assert torch.equal(offs2, offsets) and torch.equal(items2, item_offsets) and torch.equal(total2, total), \
        f"{name}: the fused scan of eg_project_bin and eg_tile_offsets disagree"
    M = int(tot[0])
    assert M == int(pops.sum()) == int(offsets[-1]) and int(tot[1]) == 0
    rec = splat.cpu().numpy()
    out = {}
    for form, m in (("mask", mask), ("retest", None)):
        cur = _dev(pops.astype(np.int32))
        keys = torch.full((max(M, 1),), FILL, dtype=torch.int64, device="cuda")
        call("eg_tile_emit", None, None, None, ptr(splat), FLAGS, sc.N, sc.W, sc.H, ptr(offsets), ptr(cur), M, ptr(keys),
             None if m is None else ptr(m), stream())
        torch.cuda.synchronize()
        assert not cur.any(), f"{name}: eg_tile_emit ({form}) does not count the tile counters back to zero"
        out[form] = _classic_pairs(keys.cpu().numpy(), offsets.cpu().numpy(), rec, sc.T, f"{name} eg_tile_emit ({form})")
    return rec, pops, mask.cpu().numpy(), tot, out["mask"], out["retest"]


def _segment_pairs(keys, pops, seg_cap, rec, T, name):
    assert (pops >= 0).all() and (pops <= seg_cap).all(), f"{name}: a population outside its segment"
    slot = np.repeat(np.arange(T) * seg_cap, pops) + (np.arange(int(pops.sum())) - np.repeat(np.cumsum(pops) - pops, pops))
    ids, depths = _ids_and_depths(keys[slot])
    _check_keys(ids, depths, rec, name)
    return ids * T + np.repeat(np.arange(T), pops)


def _project_emit(sc, seg_cap, name):
    from edgegaussians_amd._lib import call, ptr, stream
    splat = torch.full((sc.N, 8), float("nan"), device="cuda")
    cursor, item_first, total, ticket = _zeros(sc.T), _zeros(sc.T), _zeros(4), _zeros(sc.T + 2)
    keys = torch.full((sc.T * seg_cap,), FILL, dtype=torch.int64, device="cuda")
    max_items = sc.T * (seg_cap // 128 + 1)
    call("eg_project_emit", *sc.args(), FLAGS, ptr(splat), ptr(cursor), seg_cap, ptr(keys), ptr(item_first), max_items,
         ptr(total), ptr(ticket), stream())
    torch.cuda.synchronize()
    assert int(ticket[0]) == 0
    rec, pops = splat.cpu().numpy(), cursor.cpu().numpy().astype(np.int64)
    return rec, pops, total.cpu().numpy().astype(np.int64), _segment_pairs(keys.cpu().numpy(), pops, seg_cap, rec, sc.T, name)


def _same_records(a, b, name):
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), f"{name}: the records differ in {int((a.view(np.int32) != b.view(np.int32)).any(axis=1).sum())} rows"


def _same_set(a, b, name):
    a, b = np.sort(a), np.sort(b)
    assert np.array_equal(a, b), (f"{name}: the pair sets differ: {np.setdiff1d(a, b).size} pairs only in the first, "
                                  f"{np.setdiff1d(b, a).size} only in the second")


def _grazing_sides(rec, c):
    """through the device's projection the designed ratios are met to about 1e-5: both sides for k <= 4, counted for k = 5"""
    ratio = U.grazing_ratios(rec, c)
    sides = {}
    for g, (geom, _rot, k, side, fam, _tile) in enumerate(c.info):
        if geom != "long_diag" and k <= 4:
            assert np.sign(ratio[g]) == side and 0.5 < abs(ratio[g]) * 10.0 ** k < 2.0, (g, c.info[g], float(ratio[g]))
        key = f"{fam}{'+' if side > 0 else '-'}1e-{k}"
        sides.setdefault(key, [0, 0])[0 if ratio[g] < 0 else 1] += 1
    assert all(v[0] + v[1] == 16 for v in sides.values())
    return sides


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_producers(lib, name):
    c = U.case(name)
    sc = _Scene(c.params)
    rec, pops, mask, tot, e_mask, e_retest = _project_bin_emit(sc, name)
    refs = U.references(rec, sc.W, sc.H)
    seg_cap = 128 * (int(np.bincount(refs.key % sc.T, minlength=sc.T).max(initial=0)) // 128 + 1)   # gsplat's box bounds every tile
    rec_e, pops_e, tot_e, e_seg = _project_emit(sc, seg_cap, f"{name} eg_project_emit")
    rec_f, tpg, counts_f = _project_fwd(sc)
    # (5) one set of records, one set of pairs
    _same_records(rec, rec_e, f"{name}: eg_project_bin against eg_project_emit")
    _same_records(rec, rec_f, f"{name}: eg_project_bin against eg_project_fwd")
    _same_set(e_mask, e_retest, f"{name}: eg_tile_emit with the mask against the re-test")
    _same_set(e_mask, e_seg, f"{name}: eg_tile_emit against eg_project_emit")
    # (1), (2)
    figs = U.check_sets(refs, rec, e_mask, name)
    U.check_sets(refs, rec, e_seg, f"{name} eg_project_emit")
    # (3)
    extra = {}
    if name == "grazing":
        extra["sides"] = _grazing_sides(rec, c)
    elif name == "dead":
        assert e_mask.size == 0 and not mask.any() and not pops.any()
    else:
        extra["share"] = U.check_share(refs, name)
    # (4)
    want_tpg, want_pops = U.counts_of(e_mask, sc.N, sc.tw, sc.th)
    assert np.array_equal(tpg, want_tpg), f"{name}: tiles_per_gauss differs on {int((tpg != want_tpg).sum())} rows"
    for got, what in ((pops, "eg_project_bin's tile_counts"), (counts_f, "eg_project_fwd's tile_counts"), (pops_e, "eg_project_emit's cursors")):
        assert np.array_equal(got, want_pops), f"{name}: {what} differ on {int((got != want_pops).sum())} tiles"
    for t, what in ((tot, "eg_project_bin"), (tot_e, "eg_project_emit")):
        assert t[0] == e_mask.size and t[1] == 0 and t[3] == want_pops.max(initial=0), f"{name}: total of {what} is {t.tolist()}"
        assert t[2] == np.maximum(1, (want_pops + 127) // 128).sum()
    extra["ambiguous_rows"] = U.check_mask(rec, e_mask, mask, sc.W, sc.H, name)
    if name in U.MASK_IMAGES:   # the exact boxes, from the device's records
        box, _amb = U.tight_box64(rec, sc.tw, sc.th)
        for g, want in enumerate(c.info):
            if want is not None:
                tx0, ty0, w, h, kind = want
                assert tuple(int(v[g]) for v in box) == (tx0, ty0, tx0 + w, ty0 + h), (g, want)
                m = int(mask[g]) & U.ALL_ONES
                assert (m == U.ALL_ONES) == (w * h > 32 or kind == "blob" or min(w, h) == 1), (g, want, hex(m))
    if name == "n65537":
        live = np.nonzero(U.radius_of(rec) > 0)[0]
        assert sc.N == 65537 and live[0] == 0 and live[-1] == 65536
    record("tile_cull_producers", case=name, gaussians=sc.N, tiles=sc.T, **figs, **extra)


def _emit_records(rec, W, H, cap):
    """eg_tile_emit on hand-made records, tile_mask = NULL: tile t owns slots [t cap, (t + 1) cap), its counter starts at
    cap and is counted down, so its keys fill the segment's end"""
    from edgegaussians_amd._lib import call, ptr, stream
    tw, th = U.tiles_of(W, H)
    T, N = tw * th, rec.shape[0]
    splat = _dev(rec)
    offsets = _dev((np.arange(T + 1) * cap).astype(np.int32))
    cur = torch.full((T,), cap, dtype=torch.int32, device="cuda")
    keys = torch.full((T * cap,), FILL, dtype=torch.int64, device="cuda")
    call("eg_tile_emit", None, None, None, ptr(splat), FLAGS, N, W, H, ptr(offsets), ptr(cur), T * cap, ptr(keys), None, stream())
    torch.cuda.synchronize()
    left = cur.cpu().numpy().astype(np.int64)
    assert (left >= 0).all(), "more keys than gsplat's box allows"
    pops = cap - left
    k = keys.cpu().numpy()
    slot = np.repeat(np.arange(T) * cap + left, pops) + (np.arange(int(pops.sum())) - np.repeat(np.cumsum(pops) - pops, pops))
    ids, depths = _ids_and_depths(k[slot])
    _check_keys(ids, depths, rec, "eg_tile_emit on hand-made records")
    assert int((k != FILL).sum()) == int(pops.sum()), "keys outside the counted slots"
    return ids * T + np.repeat(np.arange(T), pops)


@pytest.mark.parametrize("name", ["grazing", "dead_records", "thin"])
def test_emit_from_hand_made_records(lib, name):
    """the re-test of tile_emit_kernel on records given as they are: the grazing ratios exact to 1e-7 (o re-solved at the
    record level), det <= 0 and radius == 0 rows, and the host's `thin` records (the fp32 model's own input)"""
    W, H = 200, 136
    if name == "dead_records":
        rec, refs = U.dead_records(90, 5, W, H), None
    else:
        _c, rec, refs = U.host_case(name)
    refs = U.references(rec, W, H) if refs is None else refs
    cap = int(np.bincount(refs.key % (refs.tw * refs.th), minlength=refs.tw * refs.th).max(initial=0)) + 8
    e = _emit_records(np.array(rec), W, H, cap)
    figs = U.check_sets(refs, rec, e, f"hand-made {name}")
    if name == "dead_records":
        assert e.size == 0
    else:   # how far the device is from the fp32 numpy model (hardware rcp / sqrt / log against IEEE): recorded, not asserted
        kept, _m, _b = U.model32(rec, W, H)
        figs["only_device"], figs["only_model"] = int(np.setdiff1d(e, kept).size), int(np.setdiff1d(kept, e).size)
    record("tile_cull_hand_made", case=name, **figs)


# ---------------------------------------------------------------------------------------------------
# (6) the fused tails
def _trainer(p):
    from edgegaussians_amd import EdgeTrainer
    t = torch.from_numpy
    V = p.viewmats.shape[0]
    g = np.random.default_rng(5)
    gt = (g.uniform(0, 1, (V, p.H, p.W)) < 0.1).astype(np.float32)
    tr = EdgeTrainer(t(p.means), t(p.log_scales), t(p.quats), t(p.logit_opacities), t(p.viewmats), t(p.Ks), t(gt), p.W, p.H)
    tr.ensure_capacity()
    assert tr.seg_cap > 0
    return tr


def _wmap(p):
    return torch.full((p.H, p.W), 1.0 / (p.H * p.W), device="cuda")


def _params_of_trainer(tr):
    return [tr.means.clone(), tr.quats.clone(), tr.log_scales.clone(), tr.logit_opacities.clone()]


def _check_tail(name, p, tensors, view, rec_tail, e_tail, seg_cap):
    sc = _Scene(p, view, tensors)
    rec, _pops, _tot, e_ref = _project_emit(sc, seg_cap, f"{name} eg_project_emit")
    _same_records(rec_tail, rec, f"{name}: the tail's records against eg_project_emit on the parameters read back")
    _same_set(e_tail, e_ref, f"{name}: the tail's pairs against eg_project_emit")
    refs = U.references(rec, sc.W, sc.H)
    figs = U.check_sets(refs, rec, e_tail, name)
    assert figs["must_keep"] > 10000
    record("tile_cull_tails", case=name, gaussians=sc.N, **figs)


TAIL_SIZES = [4000, 33000, 65537]


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_tail_of_apply_adam(lib, n):
    """EdgeTrainer.apply_adam(next_view=1): the pending tables (cursors, unsorted key segments, records) of view 1"""
    p = U.tail_scene(n)
    tr = _trainer(p)
    w = _wmap(p)
    tr.grad_step(0, w)
    tr.apply_adam(next_view=1)
    torch.cuda.synchronize()
    assert tr._projected == 1
    tensors = _params_of_trainer(tr)
    assert not torch.equal(tensors[0], torch.from_numpy(p.means).cuda()), "the Adam step moved the means"
    rec = tr.splat.cpu().numpy()
    pops = tr.tile_counts.cpu().numpy().astype(np.int64)
    e_tail = _segment_pairs(tr.keys.cpu().numpy(), pops, tr.seg_cap, rec, tr.T, f"apply_adam[{n}]")
    _check_tail(f"apply_adam[{n}]", p, tensors, 1, rec, e_tail, tr.seg_cap)


@pytest.mark.parametrize("n", TAIL_SIZES)
def test_tail_of_a_run_of_steps(lib, n):
    """train_steps([0, 1]): step 0's last kernel projects and bins view 1 with the parameters it has just written; step
    1's sort leaves those pairs in the tables.  The parameters after step 0 come from a second trainer."""
    p = U.tail_scene(n)
    T = math.prod(U.tiles_of(p.W, p.H))
    assert lib.load().eg_backward_is_fused(n, T) == (1 if n == 4000 else 0)
    w = _wmap(p)
    one = _trainer(p)
    one.train_steps([0], [w])
    one.pop_loss()
    assert not one.overflowed()
    tensors = _params_of_trainer(one)
    two = _trainer(p)
    assert two.fused_backward_active() == (n == 4000)
    two.train_steps([0, 1], [w, w])
    two.pop_loss()
    assert not two.overflowed()
    torch.cuda.synchronize()
    rec = two.splat.cpu().numpy()
    total = two.total.cpu().numpy()
    sc = _Scene(p, 1, tensors)
    rec_ref, pops_ref, _tot, e_ref = _project_emit(sc, two.seg_cap, f"steps[{n}] eg_project_emit")
    # the sorted tables of step 1: tile t's ids at [t seg_cap, tile_end[t]); a tile nothing reaches keeps an older tile_end
    end = two.tile_end.cpu().numpy().astype(np.int64)
    start = np.arange(T) * two.seg_cap
    pops = np.where(pops_ref > 0, end - start, 0)
    assert int(total[0]) == int(pops_ref.sum()) and int(total[1]) == 0, "step 1 counted the pairs eg_project_emit gives"
    assert (pops >= 0).all() and (pops <= two.seg_cap).all()
    flat = two.flatten_ids.cpu().numpy().astype(np.int64)
    slot = np.repeat(start, pops) + (np.arange(int(pops.sum())) - np.repeat(np.cumsum(pops) - pops, pops))
    e_tail = flat[slot] * T + np.repeat(np.arange(T), pops)
    _check_tail(f"steps[{n}]", p, tensors, 1, rec, e_tail, two.seg_cap)


def test_batched_projection(lib):
    """grad_step_batched on two views: project_emit_kernel with gridDim.y = 2 (always its 512-thread form) writes each
    view's records and pairs into that view's own tables; no optimizer step, so the parameters are the scene's"""
    p = U.tail_scene(4000)
    tr = _trainer(p)
    w = _wmap(p)
    tr.grad_step_batched([0, 1], [w, w])
    torch.cuda.synchronize()
    b = tr._batches[2]
    assert not tr.overflowed()
    T = tr.T
    for k in (0, 1):
        sc = _Scene(p, k)
        rec_ref, pops_ref, _tot, e_ref = _project_emit(sc, tr.seg_cap, f"batched view {k} eg_project_emit")
        rec = b["splat"][k].cpu().numpy()
        end = b["tile_end"][k].cpu().numpy().astype(np.int64)
        start = np.arange(T) * tr.seg_cap
        pops = np.where(pops_ref > 0, end - start, 0)    # (a tile nothing reaches keeps the tile_end it was allocated with)
        total = b["total"][k].cpu().numpy()
        assert int(total[0]) == int(pops_ref.sum()) and (pops >= 0).all() and (pops <= tr.seg_cap).all()
        flat = b["flatten_ids"][k].cpu().numpy().astype(np.int64)
        slot = np.repeat(start, pops) + (np.arange(int(pops.sum())) - np.repeat(np.cumsum(pops) - pops, pops))
        e = flat[slot] * T + np.repeat(np.arange(T), pops)
        _same_records(rec, rec_ref, f"batched view {k}")
        _same_set(e, e_ref, f"batched view {k}")
        figs = U.check_sets(U.references(rec, sc.W, sc.H), rec, e, f"batched view {k}")
        record("tile_cull_tails", case=f"batched view {k}", gaussians=sc.N, **figs)
