"""CPU-only statements behind tests/test_gpu_tile_cull.py: the cases of tests/cull_util.py reach the branches they are
built for, the float64 references are tight (may_keep exceeds must_keep by at most 3 % per case), the fp32 numpy model of
tile_box_tight + splat_hits_tile passes the assertions the kernels are held to, and every planted defect of that model
is caught by them.

Measured here (fp32 model on the host records, BAND_FACTOR = 4):
  case       box pairs   must_keep   may_keep   model keeps   may_keep \\ must_keep
  thin        156 617      14 513     14 693      14 693         1.2 %
  n65537       76 242       7 129      7 192       7 192         0.9 %
  grid_1456    49 136       2 059      2 091       2 091         1.6 %
  grid_2064    45 806       1 781      1 795       1 794         0.8 %
  n1 .. n513: 0 .. 1.5 %; the mask cases 0 % (381 / 64 / 226 pairs); grazing 10 720 / 1 700 / 1 840 / 1 831.
  gsplat's box is 10.7 x may_keep on `thin`.  The largest band of a may_keep pair is 0.013 on `thin` (0.028 on grid_2064,
  where x reaches 2000); the model needs BAND_FACTOR >= 0.089 to stay inside may_keep (test_band_is_what_the_model_needs),
  which is why cull_util's first, a-priori factor of 16 went down to 4.
  grazing, kept by the model per threshold and side (16 rows each): ln(255 o): -1e-2 .. -1e-5 all 16, +1e-2 none, +1e-3 ..
  +1e-5 all 16 (inside the kernel's 0.1 % slack); the kernel's own limit: - side all 16, +1e-2 .. +1e-4 none, +1e-5 3 of 16
  (inside the band).
"""
import numpy as np
import pytest

from tests import cull_util as U
from tests.util import record_cpu

SHARE_CASES = [n for n in U.CASE_NAMES if n not in ("grazing", "dead")]


def _model_checks(name, mutant=None):
    """assertions (1), (2) and (4) on the model's output for one case"""
    c, rec, refs = U.host_case(name)
    kept, mask, _box = U.model32(rec, c.params.W, c.params.H, mutant)
    figs = U.check_sets(refs, rec, kept, f"model {name}")
    figs["ambiguous_rows"] = U.check_mask(rec, kept, mask, c.params.W, c.params.H, f"model {name}")
    return figs


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_model_passes_the_assertions(name):
    figs = _model_checks(name)
    record_cpu("tile_cull_model", case=name, **figs)


@pytest.mark.parametrize("name", SHARE_CASES)
def test_references_are_tight(name):
    """(3): from the references alone.  gsplat's box is several times larger, so a cull that degenerates to it fails (2)."""
    _c, _rec, refs = U.host_case(name)
    share = U.check_share(refs, name)
    record_cpu("tile_cull_share", case=name, share=share, **U.figures(refs))
    if name == "thin":
        assert refs.key.size > 5 * refs.may.sum()


def test_band_is_what_the_model_needs():
    """the smallest BAND_FACTOR under which the model's kept pairs of `thin` and of `grazing` lie inside may_keep"""
    need = 0.0
    for name in ("thin", "grazing"):
        c, rec, refs = U.host_case(name)
        kept, _m, _b = U.model32(rec, c.params.W, c.params.H)
        assert np.isin(kept, refs.key).all()
        need = max(need, U.needed_band_factor(refs, kept))
    record_cpu("tile_cull_band", needed_factor=need, factor=U.BAND_FACTOR)
    assert need <= U.BAND_FACTOR / 2, need


def test_thin_reaches_its_branches():
    c, rec, refs = U.host_case("thin")
    o = rec[:, 5].astype(np.float64)
    live = U.radius_of(rec) > 0
    assert (live & (o < 1.0 / 255.0)).sum() > 50, "thr <= 0 rows"
    assert (live & (o > 1.0 / 255.0)).sum() > 1500
    a, b, cc = (rec[:, k].astype(np.float64) for k in (2, 3, 4))
    with np.errstate(all="ignore"):
        ratio = np.where(live, np.abs(b) / np.sqrt(a * cc), 0.0)
    assert (ratio > 0.99).sum() > 100, "thin diagonals: |b| within 1 % of sqrt(a c)"
    # the cancellation the issue names: terms of 1e4 against a sum of order 1 inside kept pairs
    kept = refs.may
    assert (refs.band[kept] / (U.BAND_FACTOR * 2.0 ** -24) > 1e4).sum() > 50
    x0, y0, x1, y1 = refs.box_xyxy
    assert ((x0 == 0) & live).any() and ((x1 == refs.tw) & live).any() and ((y0 == 0) & live).any() and ((y1 == refs.th) & live).any()
    assert refs.tw == 13 and refs.th == 9, "partial last column and row"


def test_mask_cases_reach_their_boxes():
    seen = set()
    for name in U.MASK_IMAGES:
        c, rec, refs = U.host_case(name)
        tw, th = refs.tw, refs.th
        (x0, y0, x1, y1), amb = U.tight_box64(rec, tw, th)
        assert not amb.any(), "no bound of a mask case sits on a tile border"
        m32 = U.model32(rec, c.params.W, c.params.H)
        assert all(np.array_equal(p, q) for p, q in zip(m32[2], (x0, y0, x1, y1))), "the fp32 model forms the same tight boxes"
        must_mask, _bad = U.mask_of(refs.key[refs.must], (x0, y0, x1, y1), rec.shape[0], tw, th)
        for g, want in enumerate(c.info):
            if want is None:
                continue
            tx0, ty0, w, h, kind = want
            assert (x0[g], y0[g], x1[g], y1[g]) == (tx0, ty0, tx0 + w, ty0 + h), (name, g, want, (x0[g], y0[g], x1[g], y1[g]))
            area = w * h
            n_must = int(((refs.g == g) & refs.must).sum())
            if kind == "blob":
                assert n_must == area, (name, want, n_must)
            elif min(w, h) >= 2:
                assert n_must < area and (area > 32 or int(must_mask[g]) != U.ALL_ONES), (name, want, n_must)
            if kind == "diag" and min(w, h) >= 3:
                assert n_must <= 0.6 * area, (name, want, n_must)
            seen.add((w, h, kind))
        if name == "mask_a":   # boxes clipped by each border
            clipped = [g for g, want in enumerate(c.info) if want is None]
            gx0, gy0, gx1, gy1 = refs.box_xyxy
            sel = np.array(clipped)
            assert (gx0[sel] == 0).any() and (gy0[sel] == 0).any() and (gx1[sel] == tw).any() and (gy1[sel] == th).any()
            assert (x1[sel] > x0[sel]).sum() >= 12
    for shape in ((4, 8), (8, 4), (1, 32), (32, 1), (2, 16), (3, 11), (1, 33), (13, 9)):
        assert (shape + ("blob",)) in seen and (shape + ("diag",)) in seen, shape


def test_grazing_is_on_both_sides_of_each_threshold():
    c, rec, refs = U.host_case("grazing")
    ratio = U.grazing_ratios(rec, c)
    tw, th = refs.tw, refs.th
    kept, _m, _b = U.model32(rec, c.params.W, c.params.H)
    counts = {}
    for g, (geom, _rot, k, side, fam, tile) in enumerate(c.info):
        assert np.sign(ratio[g]) == side and 0.99 < abs(ratio[g]) * 10.0 ** k < 1.01, (g, c.info[g], ratio[g])
        key = U.keys_of(np.array([g]), np.array([tile[0]]), np.array([tile[1]]), tw, th)[0]
        i = np.searchsorted(refs.key, key)
        assert refs.key[i] == key, "the grazed tile lies inside gsplat's box"
        counts.setdefault((geom, k, side, fam), []).append((bool(refs.must[i]), bool(refs.may[i]), bool(np.isin(key, kept))))
        if fam == "alpha" and side > 0:
            assert not refs.must[i], "outside the 1/255 contour no pixel centre counts"
        if fam == "alpha" and geom in ("corner", "long_diag") and side < 0:
            assert refs.must[i], "the corner IS a pixel centre: inside the contour it must be kept"
        if geom == "between":
            assert not refs.must[i], "the ellipse passes between two rows of pixel centres"
        if fam == "alpha" and (side < 0 or k >= 3):
            assert refs.may[i] and np.isin(key, kept), "inside the kernel's slack: kept"
        if side > 0 and k == 2:
            assert not refs.may[i] and not np.isin(key, kept), "1 % outside either threshold: dropped"
    assert len(counts) == len(U.GRAZE_GEOMS) * len(U.GRAZE_KS) * 2 * len(U.GRAZE_FAMILIES) and all(len(v) == 4 for v in counts.values())
    record_cpu("tile_cull_grazing", rows=len(c.info),
               kept_by_side={f"{fam}{'+' if s > 0 else '-'}1e-{k}": sum(x[2] for g in U.GRAZE_GEOMS for x in counts[(g, k, s, fam)])
                             for fam in U.GRAZE_FAMILIES for k in U.GRAZE_KS for s in (-1, 1)})


def test_dead_rows_own_no_pair():
    for rec, W, H in ((U.host_case("dead")[1], 200, 136), (U.dead_records(90, 5, 200, 136), 200, 136)):
        refs = U.references(rec, W, H)
        kept, mask, _b = U.model32(rec, W, H)
        assert refs.may.sum() == 0 and refs.must.sum() == 0 and kept.size == 0 and not mask.any()
    c, rec, _refs = U.host_case("dead")
    r = U.radius_of(rec)
    assert (r == 0).sum() >= 80 and ((r > 0) & (rec[:, 5] < 1.0 / 255.0)).sum() >= 60
    rec2 = U.dead_records(90, 5, 200, 136)
    a, b, cc = (rec2[:, k].astype(np.float64) for k in (2, 3, 4))
    assert ((U.radius_of(rec2) > 0) & (a * cc - b * b <= 0)).sum() >= 20


def test_sizes_and_grids():
    c, rec, refs = U.host_case("n65537")
    live = np.nonzero(U.radius_of(rec) > 0)[0]
    assert rec.shape[0] == 65537 and live[0] == 0 and live[-1] == 65536 and 1000 < live.size <= U.BIG_LIVE
    assert np.isin(live, c.info).all()
    for name, T in (("grid_1456", 8281), ("grid_2064", 16641)):
        _c, _rec, refs = U.host_case(name)
        assert refs.tw * refs.th == T
    assert 2 * 8281 > 16384 >= 8281 and 16641 > 16384


@pytest.mark.parametrize("mutant,where", [("noslack", "thin"), ("x1_no_plus1", "thin"), ("rect16", "thin"), ("mask_bh", "mask_a"),
                                          ("small31", "mask_a"), ("edge_sign", "thin")])
def test_mutants_are_caught(mutant, where):
    with pytest.raises(AssertionError):
        _model_checks(where, mutant)


def test_quadrant_grazing_case_aims_at_its_quadrants():
    """the `grazing` forward case of tests/step_composite_util.py: disjoint supports, the corner pixel's alpha where it was
    designed, and -- on the visible side up to k = 3 -- a pixel with alpha >= (1/255)(1 + 1e-4) inside the aimed quadrant,
    which the ellipse touches at that corner pixel alone"""
    from tests import composite_util as CU
    from tests import step_composite_util as SU
    rec = SU.grazing_quadrant_records()
    al = SU.single_alphas(rec, CU.W, CU.H)
    assert ((al >= SU.AMIN * (1.0 - 1e-3)).sum(axis=0) <= 1).all(), "the supports are disjoint"
    for i, ((qx, qy), (cx, cy), k, side) in enumerate(SU.GRAZE_QUADRANTS):
        px, py = qx + 7 * cx, qy + 7 * cy
        ratio = al[i, py, px] * 255.0 - 1.0
        assert np.sign(ratio) == -side and 0.99 < abs(ratio) * 10.0 ** k < 1.01, (i, ratio)
        quad = al[i, qy:qy + 8, qx:qx + 8]
        assert (quad >= SU.AMIN).sum() == (1 if side < 0 else 0), "the corner pixel alone"
        if side < 0 and k <= 3:
            assert (quad >= SU.AMIN * (1.0 + 1e-4)).any()
        assert abs(float(rec[i, 3])) > 0.4 * float(rec[i, 2]), "diagonal"
    c = SU.forward_case("grazing", "nostop")
    assert not c.f.stopped.any() and (c.f.alphas > 0).sum() > 100
