"""The references and cases of tests/test_gpu_step_composite.py, checked on the CPU with the references alone: the two
float64 routes to the unit-colour gradient agree, every case keeps its borderline share under 3 % and its loose-row share under SU.LOOSE_CAP, every
scene contains what it is for, and the per-row / per-pixel checks reject planted defects that the max-norm
`assert_close(rtol=1e-4)` of tests/test_gpu_oracle_floats.py lets through."""
import numpy as np
import pytest
import torch

from tests import composite_util as CU
from tests import step_composite_util as SU
from tests.util import ROW_LOOSE, assert_close, record_cpu

FWD_CASES = [(l, r) for l in SU.FWD_LENGTHS for r in SU.FWD_REGIMES]
# The two float64 routes sum a row's terms -- at most one per pixel of the image -- in different orders, every term the
# result of some eight rounded operations: 8 n 2^-53 of the row; a row that cancels is granted the same share of ...
ROUTE_TOL = 8 * CU.W * CU.H * 2.0 ** -53
ROUTE_CANCEL = 0.01   # ... this fraction of the tensor's largest row


@pytest.mark.parametrize("lengths,regime", FWD_CASES)
def test_the_two_float64_routes_agree(lengths, regime):
    """the record-driven footprint sum (from the float64 forward's own record image) against autograd through
    CU.ref_composite on the same lists: the reference checking itself, to float64 rounding of each row"""
    c = SU.forward_case(lengths, regime)
    assert SU.lists_sorted(c.rec, c.lst)
    img = SU.RecImg(c.f.gT, c.f.stop_id.astype(np.int64), c.f.stop_depth.astype(np.int64))
    a = SU.ref_backward(c.rec, img, CU.W, CU.H)
    b = SU.ref_autograd(c.rec, c.lst, c.f.v)
    for name, (c0, c1) in CU.G2D_COLS.items():
        sigma = np.abs(b[:, c0:c1]).max(axis=1)
        dev = np.abs(a[:, c0:c1] - b[:, c0:c1]).max(axis=1)
        assert (dev <= ROUTE_TOL * sigma + ROUTE_TOL * ROUTE_CANCEL * sigma.max()).all(), \
            (name, float((dev / np.maximum(sigma, 1e-300)).max()))
        assert (sigma > 0).any()


@pytest.mark.parametrize("lengths,regime", FWD_CASES)
def test_forward_cases_contain_what_they_are_for(lengths, regime):
    c = SU.forward_case(lengths, regime)
    lens = np.diff(c.lst.offsets)
    assert tuple(lens) == SU.FWD_LENGTHS[lengths], "every Gaussian bins into its own tile alone"
    share = float(c.mask.mean())
    stopped = float(c.f.stopped.mean())
    d32 = SU.d32_of(c.rec, c.lst, c.f, c.mask, CU.W, CU.H)
    record_cpu("step_composite_forward_case", case=c.name, borderline_share=share, stopped_share=stopped, d32=d32)
    assert share < SU.BORDER_SHARE_CAP, share
    db = SU.depth_bits(c.rec)
    assert any(np.unique(db[c.lst.flat[c.lst.offsets[t]:c.lst.offsets[t + 1]]]).size < lens[t] for t in range(len(lens))), \
        "ties at bit-equal depth inside a list"
    if regime == "nostop":
        assert stopped == 0.0
    else:
        assert 0.15 <= stopped <= 0.55, stopped
    if lengths == "long":   # on both sides of 256, one anchor (8 slices), two anchors (16), and the 24-slice switch
        assert lens.min() == 0 and {256, 257} <= set(lens.tolist())
        assert 8 * 128 < lens[2] <= 16 * 128 < lens[3] <= 24 * 128 < lens[4]
    else:
        assert {0, 1, 127, 128, 129, 255} == set(lens.tolist())
    if regime == "quadrant" and lengths == "long":
        t = int(np.argmax(lens))
        ty, tx = divmod(t, SU.tiles_of(CU.W, CU.H)[0])
        q = (slice(16 * ty, 16 * ty + 8), slice(16 * tx, 16 * tx + 8))
        assert c.f.stopped[q].all() and (c.f.last_idx[q] - c.lst.offsets[t] < 128).all(), "a quadrant whose pixels all stop in slice 0"


@pytest.mark.parametrize("name", SU.FOOTPRINT_CASES)
def test_footprint_cases_hold_their_conditions(name):
    c = SU.footprint_case(name)
    share = float(c.mask.mean())
    ratios = {k: CU.grad_row_ratio(torch.from_numpy(c.ref[:, a:b]), torch.from_numpy(c.ref[None, :, a:b]), c.kappa[k])
              for k, (a, b) in CU.G2D_COLS.items()}
    loose, over_1e3 = {k: r[1] for k, r in ratios.items()}, {k: r[2] for k, r in ratios.items()}
    record_cpu("step_composite_footprint_case", case=name, borderline_share=share, loose_row_share=loose, over_1e3_row_share=over_1e3,
               live_rows=int((np.abs(c.ref).max(axis=1) > 0).sum()), rows=int(c.rec.shape[0]), row_loose=ROW_LOOSE)
    assert share < SU.BORDER_SHARE_CAP, share
    cap = SU.LOOSE_CAP[name if name in SU.LOOSE_CAP else "n"]
    assert max(loose.values()) <= cap, (loose, cap)
    assert name == "large" or max(over_1e3.values()) <= 0.5 * cap, (over_1e3, cap)   # half of them at most beyond 1e-3
    # (The projection tests cap the share of rows looser than ROW_LOOSE at 3 %.  Like the chunked kernels' cases
    # (tests/test_composite_host.py) these cases cannot hold that cap, and the cap asserted is SU.LOOSE_CAP's, per case: one ulp of an
    # fp32 centre at x = 40 is 4e-6 px, which moves the alpha of a sub-pixel or 30:1 Gaussian by 1e-4 of itself and a
    # first moment that cancels by symmetry by more -- 8 to 87 % of the live rows are loose, every row of the 2304-px
    # image's v_means2d.  A loose row is still held to its own bound ROW_FLOOR + ROW_KAPPA_FACTOR kappa_r.)
    fw, fh, pw = SU.walk_ints(c.rec, c.W, c.H)
    live = np.abs(c.ref).max(axis=1) > 0
    if name == "mix":
        for w0 in range(0, c.rec.shape[0], 8):
            cells = (np.minimum(pw, fw) * fh)[w0:w0 + 8]
            if w0 % 24 == 8:
                assert not live[w0:w0 + 8].any() and (cells[[0, 1, 2, 3]] == 0).all(), "a wave of dead rows"
            else:
                assert cells.max() >= 0.9 * c.W * c.H and np.sort(cells)[-2] <= 16, "one huge footprint beside seven tiny ones"
        assert {int(np.argmax((fw * fh)[w0:w0 + 8])) for w0 in range(0, c.rec.shape[0], 24)} == set(range(8))
    if name == "shear":
        v = fw > 0
        assert (pw[v] % 2 == 0).any() and (pw[v] % 2 == 1).any()
        assert (pw[v] < fw[v]).any() and (pw[v] >= fw[v]).any(), "the sheared walk and the axis-aligned fallback"
        assert {-1, 0, 1} <= set((pw - fw)[v].tolist()), "pw == fw - 1, fw, fw + 1"
        j0, i0, j1, i1 = SU.pixel_boxes(c.rec, c.W, c.H)
        assert ((j0 == 0) & live).any() and ((j1 == c.W) & live).any() and ((i0 == 0) & live).any() and ((i1 == c.H) & live).any()
    if name == "stops":
        db = SU.depth_bits(c.rec)
        assert db[5] == db[0] == db[11] and db[6] == db[5] + 1 and db[7] == db[5] - 1
        named = np.unique(c.img.stop_depth[c.img.stop_id >= 0])
        assert not np.isin(db[16:24], named).any() and live[16:24].all(), "a wave no lane of which ties"
        assert (c.rec[32:40, 5] > CU.AMAX).all() and (c.rec[24:32, 5] > CU.AMAX).sum() == 3
        g32 = c.img.gT.astype(np.float32)
        assert ((g32 == 0) & np.signbit(g32)).any() and ((g32 != 0) & (np.abs(g32) < np.finfo(np.float32).tiny)).any()
        assert (c.img.stop_id == np.arange(c.rec.shape[0])[:, None, None]).any(axis=(1, 2))[[0, 5, 11, 2, 9]].all()
    if name == "large":
        g = int(np.argmax(fw * fh))
        assert g == 3 and fh[g] * ((min(pw[g], fw[g]) + 1) // 2) > 2 ** 21 and c.rec.shape[0] == 9


def _invisible_to_max_norm(got, ref):
    """the defect moves no element by more than half of what assert_close(rtol=1e-4) grants the tensor's largest"""
    return all(np.abs(got[:, a:b] - ref[:, a:b]).max() <= 0.5e-4 * np.abs(ref[:, a:b]).max() for a, b in CU.G2D_COLS.values())


def _row_checks(got, c):
    for name, (c0, c1) in CU.G2D_COLS.items():
        CU.grad_row_check(torch.from_numpy(got[:, c0:c1]), torch.from_numpy(c.ref[None, :, c0:c1]), c.kappa[name], name)


def test_row_check_rejects_a_dropped_footprint_column():
    """one column of one small Gaussian's footprint not walked: invisible to the max-norm, over the row bound"""
    c = SU.footprint_case("n257")
    _row_checks(c.ref.copy(), c)
    hit = 0
    order = np.argsort(np.abs(c.ref).max(axis=1))
    for g in order[np.abs(c.ref).max(axis=1)[order] > 0][:120]:
        got = None
        for dj in (-3, 3, -2, 2, -1, 1, 0):         # an edge column of the footprint first: it carries the least
            j0 = int(np.floor(c.rec[g, 0])) + dj
            if not 0 <= j0 < c.W:
                continue
            img = SU.RecImg(c.img.gT.copy(), c.img.stop_id, c.img.stop_depth)
            img.gT[:, j0] = 0.0
            trial = c.ref.copy()
            trial[g] = SU.ref_backward(c.rec, img, c.W, c.H, only=[g])[g]
            if not np.array_equal(trial[g], c.ref[g]) and _invisible_to_max_norm(trial, c.ref):
                got = trial
                break
        if got is None:
            continue
        for name, (c0, c1) in CU.G2D_COLS.items():
            assert_close(got[:, c0:c1], c.ref[:, c0:c1], rtol=1e-4, name=name)
        with pytest.raises(AssertionError, match="per-row bound"):
            _row_checks(got, c)
        hit += 1
    assert hit >= 3, "several small Gaussians whose missing column only the row check sees"


@pytest.mark.parametrize("name", ["mix", "shear", "n257_onesign"])
def test_row_check_rejects_a_dropped_column_where_the_rows_are_loose(name):
    """The cases whose rows are mostly loose (bound dominated by kappa_r) must still see the defect they exist for: the
    centre column of a tiny row (mix: the sub-pixel Gaussians beside the huge one) or of a thin row (shear: the 30:1
    Gaussians) not walked.  EVERY such row whose reference changes must go over its row bound."""
    c = SU.footprint_case(name)
    _row_checks(c.ref.copy(), c)
    fw, fh, pw = SU.walk_ints(c.rec, c.W, c.H)
    small = np.nonzero((np.abs(c.ref).max(axis=1) > 0) & (np.minimum(fw, pw) * fh <= (16 if name == "mix" else 400)))[0]
    tried = 0
    for g in small:
        j0 = int(np.floor(c.rec[g, 0]))
        if not 0 <= j0 < c.W:
            continue
        img = SU.RecImg(c.img.gT.copy(), c.img.stop_id, c.img.stop_depth)
        img.gT[:, j0] = 0.0
        got = c.ref.copy()
        got[g] = SU.ref_backward(c.rec, img, c.W, c.H, only=[g])[g]
        if np.array_equal(got[g], c.ref[g]):
            continue
        with pytest.raises(AssertionError, match="per-row bound|not exactly zero"):
            _row_checks(got, c)
        tried += 1
    assert tried >= 20, tried


def test_lane_order_model_of_a_centred_screen_filling_footprint():
    """Why the large case's footprint sits off the image's centre.  Centred (a quarter pixel off), its first moments
    cancel to a few 1e-4 of the sum of their terms, and an fp32 sum in the kernel's lane order -- 57 lanes, 74 k terms
    each -- is then further from float64 than assert_close(rtol=1e-4) grants the tensor's largest row, which this row
    is: a property of that case, not of the kernel.  Off centre, as the case is, the same model is well inside."""
    c = SU.footprint_case("large")
    W, H = c.W, c.H
    for centre, inside in (((W / 2 + 0.25, H / 2 - 0.25), False), (tuple(c.rec[3, 0:2]), True)):
        rec = c.rec.copy()
        rec[3, 0:2] = centre
        model, ref = SU.lane_order_model32(rec, 3, c.img, W, H, lanes=57)
        rel = float(np.abs(model - ref).max() / np.abs(ref).max())
        record_cpu("step_composite_lane_order_model", centre=list(map(float, centre)), rel_dev=rel)
        assert (rel <= 0.5e-4) == inside, (centre, rel)


def test_row_check_rejects_a_flipped_tie_rule():
    """(depth bits, id) < instead of <= on the small rows of the stop case: the stop Gaussian itself drops out of its
    own pixels"""
    c = SU.footprint_case("stops")
    flipped = SU.ref_backward(c.rec, c.img, c.W, c.H, tie_lt=True)
    hit = 0
    for g in np.nonzero(np.abs(flipped - c.ref).max(axis=1) > 0)[0]:
        got = c.ref.copy()
        got[g] = flipped[g]
        if not _invisible_to_max_norm(got, c.ref):
            continue
        for name, (c0, c1) in CU.G2D_COLS.items():
            assert_close(got[:, c0:c1], c.ref[:, c0:c1], rtol=1e-4, name=name)
        with pytest.raises(AssertionError, match="per-row bound"):
            _row_checks(got, c)
        hit += 1
    assert hit >= 1, "a row whose flipped tie only the row check sees"


def test_record_check_rejects_planted_defects():
    """stop_depth taken from the wrong Gaussian; a stop id off by one; one pixel's gT off by 1e-3 of itself; two slice
    products folded in swapped order at a stopping pixel (at the tolerance the device gets); a stale record"""
    c = SU.forward_case("long", "third")
    good = SU.device_image(SU.record_of(c.f))
    d32 = SU.d32_of(c.rec, c.lst, c.f, c.mask, CU.W, CU.H)
    assert SU.record_check(good, c.rec, c.f, c.mask, SU.GT_TOL_FLOOR, "clean") <= 2.0 ** -24
    ys, xs = np.nonzero(c.f.stopped & ~c.mask)
    y, x = int(ys[0]), int(xs[0])
    other = (int(c.f.stop_id[y, x]) + 1) % c.rec.shape[0]
    bad = good.copy()
    bad[y, x, 2] = c.rec[other:other + 1, 6].view(np.int32)[0]
    assert bad[y, x, 2] != good[y, x, 2]
    with pytest.raises(AssertionError, match="stop_depth"):
        SU.record_check(bad, c.rec, c.f, c.mask, SU.GT_TOL_FLOOR, "depth")
    bad = good.copy()
    bad[y, x, 1] = other
    bad[y, x, 2] = c.rec[other:other + 1, 6].view(np.int32)[0]
    with pytest.raises(AssertionError, match="stop_id"):
        SU.record_check(bad, c.rec, c.f, c.mask, SU.GT_TOL_FLOOR, "id")
    ys, xs = np.nonzero((c.f.gT != 0) & (np.abs(c.f.gT) < 0.05 * np.abs(c.f.gT).max()) & ~c.mask)
    bad = good.copy()
    bad[ys[0], xs[0], 0] = np.float32(c.f.gT[ys[0], xs[0]] * (1 + 1e-3)).view(np.int32)
    with pytest.raises(AssertionError, match="gT off"):
        SU.record_check(bad, c.rec, c.f, c.mask, SU.GT_TOL_FLOOR, "gT")
    # two slice products folded in swapped order on one stopping pixel: every kept pixel whose stop lies behind slice 0
    n_swapped = 0
    ys, xs = np.nonzero(c.f.stopped & ~c.mask)
    tw = SU.tiles_of(CU.W, CU.H)[0]
    for y, x in zip(ys.tolist(), xs.tolist()):
        t = (y // 16) * tw + x // 16
        k = int(c.f.last_idx[y, x] - c.lst.offsets[t]) // 128 - 1      # the slice in front of the last contributor's
        if k < 0:
            continue
        gT, sid = SU.swapped_slice_record(c.rec, c.lst, CU.W, CU.H, y, x, c.f, k)
        if sid == c.f.stop_id[y, x] and gT == c.f.gT[y, x]:
            continue   # (nothing of slice k reaches this pixel, or its weight is zero: the swap changes nothing)
        bad = good.copy()
        bad[y, x, 0] = np.float32(gT).view(np.int32)
        bad[y, x, 1] = sid
        bad[y, x, 2] = c.rec[sid:sid + 1, 6].view(np.int32)[0] if sid >= 0 else -1
        with pytest.raises(AssertionError, match="stop_id|gT off"):
            SU.record_check(bad, c.rec, c.f, c.mask, max(SU.GT_TOL_FACTOR * d32, SU.GT_TOL_FLOOR), "swapped")
        n_swapped += 1
    assert n_swapped >= 50, n_swapped
    # a stale record in a tile the view leaves empty (1e-5 of the image's largest gT: nothing to the max-norm)
    short = SU.forward_case("short", "third")
    t = int(np.argmin(np.diff(short.lst.offsets)))
    ty, tx = divmod(t, SU.tiles_of(CU.W, CU.H)[0])
    assert np.diff(short.lst.offsets)[t] == 0
    stale = SU.device_image(SU.record_of(short.f))
    stale[16 * ty + 3, 16 * tx + 2, 0] = np.float32(1e-5 * np.abs(short.f.gT).max()).view(np.int32)
    assert_close(SU.image_of_words(stale).gT, short.f.gT, rtol=1e-4, name="gT image")
    with pytest.raises(AssertionError, match="not exactly 0"):
        SU.record_check(stale, short.rec, short.f, short.mask, SU.GT_TOL_FLOOR, "stale")
    # ... none of which the whole-image max-norm sees
    assert_close(SU.image_of_words(bad).gT, c.f.gT, rtol=1e-4, name="gT image")
