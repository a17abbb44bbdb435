"""The training step's unit-colour compositing, per pixel and per Gaussian, against the float64 references of
tests/step_composite_util.py (the cases and their conditions are checked on the CPU by tests/test_step_composite_host.py).

Which test runs which kernel:

  footprint_bwd_kernel, one view (footprint_dev.h)          test_footprint_backward_rows_from_synthetic_records
      (eg_composite_bwd_footprint on hand-made records        (sizes 1 .. 257, the one-huge-seven-tiny wave mix with a
      and a hand-made record image)                            dead wave, shear, stops, the 2.10 M-pair footprint),
                                                               test_step_records_and_rows[default]
  footprint_bwd_kernel, batched (gridDim.y = C)             test_batched_step_records_and_rows
  composite_fwd_kernel<1 | 3, UNIT = true> (tile kernel)    test_forward_tile_kernel
  composite_slice_fwd_kernel<1, FUSED = true> +             test_forward_sliced[fused-hint*], test_forward_segments
      composite_rewalk_fwd_kernel
  composite_slice_fwd_kernel<1, false> +                    test_forward_sliced[unfused]
      composite_combine_fwd_kernel + re-walk
  EG_REWALK_SPECULATE (no re-walk launch, miss word)        test_forward_speculate
  eg_composite_fwd_segments (hand-built segment tables)     test_forward_segments
  composite_wave_fwd_kernel, chained, one view              test_step_records_and_rows[default]
  composite_wave_fwd_kernel, speculative, one view          test_step_records_and_rows[speculative]
  composite_chained_fwd_kernel (keep_images=True)           test_step_records_and_rows[keep_images]
  eg_composite_fwd, classic layout (segmented=False)        test_step_records_and_rows[classic]
  composite_wave_fwd_kernel, batched (gridDim.y = C)        test_batched_step_records_and_rows
  ... on a grid above kPrefixHereMaxTiles (2704 tiles)      test_step_records_and_rows[large_grid]
  ... after another view's step on the same trainer         test_second_step_ignores_the_records_an_earlier_view_left
  the quadrant cull (hitq[] / quad_hit) at a grazing corner  test_forward_tile_kernel | _sliced | _segments[grazing-nostop]: eight
                                                             thin diagonals touching an 8 x 8 quadrant at one corner pixel
                                                             (SU.grazing_quadrant_records; tests/test_cull_host.py)

The one-kernel backward (backward_fused.hip) keeps g2d in LDS and runs only inside a run of whole training steps; grad_step
always runs footprint_bwd_kernel.  No test here reaches it: it is tied to the footprint kernel by the bit-identity test of
tests/test_gpu_parity.py (its mixed_footprints case holds the size mix of the footprint cases here).

  composite_fwd_kernel<1 | 3, UNIT = false> +               test_colors_backward_rows
      composite_bwd_colors_kernel<1 | 3> with ModeArgs{}

Bounds.  Backward: every Gaussian row of g2d[:, 0:2], [:, 2:4], [:, 4:7], [:, 7] within CU.grad_row_check's bound with
scale = 1.0 -- the footprint backward reads gT = v T_final from the forward's own T, so no allowance for a stored alpha is
granted -- and rows whose float64 reference is zero exactly zero (g2d is pre-filled with NaN).  Forward: CU.fwd_check
(FWD_ROW_TOL), last contributor exact on touched pixels outside the borderline set, stop_id exact there, stop_depth
bit-equal to splat[stop_id]'s depth everywhere, gT within max(4 d32, 1e-6) relative per pixel, d32 the worst deviation
of the fp32 model of the kernels' two product orders (SU.model32_T) from float64 on the same case -- the rule of
tests/test_gpu_sh.py.  The loss within REG_LOSS_TOL relative plus n 2^-23 sum|terms| (SU.loss_slack).

Measured on the MI355X (recorded per case through tests.util.record; the borderline and loose-row shares of the cases are
recorded by tests/test_step_composite_host.py):

  footprint backward, largest ratio to the row bound over the four column groups, per case:
      n1 0.004, n7 0.004, n8 0.005, n9 0.004, n31 0.011, n32 0.020, n33 0.011, n255 0.011, n257 0.14, n257_onesign 0.13, mix 0.015,
      shear 0.28 (v_conics), stops 0.020, large 0.16 (v_conics); per group at most v_means2d 0.14, absgrad 0.082,
      v_conics 0.28, v_opacities 0.12.  No row that should be zero was touched.
      The large case's footprint is off the image's centre on purpose: centred, its first moments cancel to 4e-4 of their
      terms, and the kernel's 74 k-term fp32 sums per lane were 1.4e-3 off on v_means2d -- as the numpy model of the same
      lane order is (SU.lane_order_model32, asserted by tests/test_step_composite_host.py) -- which is 6.8 x what the
      max-norm clip of the row bound grants that (largest) row.
  forward at the C ABI, per case (d32 / device gT deviation, every launch form alike to two digits):
      short-nostop 2.2e-7 / 2.3e-7, short-third 1.8e-6 / 9.5e-7, short-quadrant 2.5e-6 / 1.2e-6,
      long-nostop 8.7e-7 / 9.7e-7, long-third 2.0e-6 / 1.1e-6, long-quadrant 1.9e-6 / 1.4e-6
      (so the floor of 1e-6 decides only on short-nostop and long-nostop); alphas within 6.4e-6 relative, render rows
      within 6.4e-6 of the row maximum, the loss within 1.7e-7 relative; no stop id, stop depth or last id off.
  through the trainer (d32 / gT deviation / rows from its own records / rows from the reference's records):
      default 1.9e-6 / 1.8e-6 / 0.056 / 0.051 (6000 Gaussians, longest list 2306, 36 % of the pixels stop,
      0.9 % borderline), keep_images and classic 1.9e-6 / 1.6e-6 / 0.057 / 0.056, speculative 1.7e-7 / 2.7e-7 / 0.008 /
      0.007, large_grid 5.1e-7 / 4.5e-7 / 0.016 / 0.016, the batched views 1.7e-6 / 1.7e-6 / 0.051 / 0.055 at worst, the
      second of two steps 1.2e-6 / 1.0e-6 / 0.032 / 0.031; losses within 1.2e-7 relative.
  eg_composite_bwd_colors (device ratio / fp32 model's ratio / allowed = max(1, 2 x model)), dense scene: v_means2d 25 /
      25 / 50 (one channel) and 14 / 14 / 27 (three), v_conics 17 / 17 / 34, v_opacities 17 / 17 / 34, v_colors 11 / 11 /
      22, absgrad 3.1 / 3.1 / 6.1 -- the stored-alpha loss of tests/test_gpu_composite_rows.py, device and model agreeing to
      two digits; sparse scene at most 0.005 of the bound.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import composite_util as CU
from tests import step_composite_util as SU
from tests.util import REG_LOSS_TOL, record

pytestmark = pytest.mark.gpu

NAN = float("nan")
GT_TOL_FACTOR, GT_TOL_FLOOR = SU.GT_TOL_FACTOR, SU.GT_TOL_FLOOR


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    return _lib


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _rows_check(g2d, ref, kappa, name):
    """every column group of a device g2d [N, 8] (host tensor) against the float64 rows; returns {group: ratio}"""
    g = g2d.numpy().astype(np.float64)
    assert np.isfinite(g).all(), f"{name}: {int((~np.isfinite(g)).any(axis=1).sum())} rows were not written (NaN pre-fill)"
    out = {}
    for k, (a, b) in CU.G2D_COLS.items():
        out[k], _ = CU.grad_row_check(torch.from_numpy(g[:, a:b]), torch.from_numpy(ref[None, :, a:b]), kappa[k],
                                      f"{name} {k}", scale=1.0)
    return out


# ---------------------------------------------------------------------------------------------------
# 2. the footprint backward from synthetic records
def _footprint(rec, words, W, H):
    from edgegaussians_amd._lib import call, ptr, stream
    N = rec.shape[0]
    splat, gtstop = _dev(rec), _dev(words)
    assert gtstop.shape == (H, W, 3) and gtstop.dtype == torch.int32 and splat.shape == (N, 8)
    g2d = torch.full((N, 8), NAN, device="cuda")
    call("eg_composite_bwd_footprint", ptr(splat), N, W, H, gtstop.data_ptr(), ptr(g2d), stream())
    torch.cuda.synchronize()
    return g2d.cpu()


@pytest.mark.parametrize("name", SU.FOOTPRINT_CASES)
def test_footprint_backward_rows_from_synthetic_records(lib, name):
    c = SU.footprint_case(name)
    got = _footprint(c.rec, SU.device_image(c.img), c.W, c.H)
    ratios = _rows_check(got, c.ref, c.kappa, f"footprint {name}")
    record("step_composite_footprint_rows", case=name, rows=int(c.rec.shape[0]), ratio_to_row_bound=ratios,
           borderline_share=float(c.mask.mean()))


# ---------------------------------------------------------------------------------------------------
# 3. the forward at the C ABI
def _ctl_words(ws, n_items, T):
    """(tickets + item flags + ctl[0:2], ctl[2], ctl[3], exit_grp) of a workspace carved for (n_items, T)"""
    w = ws.view(torch.int32).cpu().numpy()
    base = T + n_items
    return w[:base + 2], int(w[base + 2]), int(w[base + 3]), w[base + 4:base + 4 + 64 * 16]


def _forward(lib, c, form, channels=1, hint=-1, max_items=None, with_loss=True):
    """one forward of case `c`: form "tile" | "sliced" | "segments".  Returns host arrays."""
    from edgegaussians_amd._lib import call, ptr, stream
    W, H = CU.W, CU.H
    T = math.prod(SU.tiles_of(W, H))
    splat = _dev(c.rec)
    render = torch.full((H, W, channels), NAN, device="cuda")
    alphas = torch.full((H, W), NAN, device="cuda")
    last = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    has = with_loss and c.wmap is not None
    gt, wmap = (_dev(c.gt), _dev(c.wmap)) if has else (None, None)
    vpix = torch.full((H, W), NAN, device="cuda") if has else None
    loss = torch.zeros(1, device="cuda") if has else None
    out = {}
    if form == "tile":
        offs, flat = _dev(c.lst.offsets), _dev(c.lst.flat)
        call("eg_composite_fwd", ptr(splat), None, channels, ptr(offs), ptr(flat), W, H, ptr(render), ptr(alphas), ptr(last),
             ptr(gt), ptr(wmap), c.loss_scale, ptr(vpix), ptr(loss), None, None, 0, None, None, hint, stream())
    else:
        seg = SU.segment_tables(c.lst, seg_cap=3200)
        n_items = seg["n_items"]
        mi = n_items if max_items is None else max_items
        ws = lib.composite_workspace(mi, T, "cuda")
        total = _dev(np.array([c.lst.flat.size, 0, n_items, int(np.diff(c.lst.offsets).max())], np.int32))
        gtstop = torch.full((H, W, 3), 0x7fc00000, dtype=torch.int32, device="cuda")
        if form == "sliced":
            offs, flat = _dev(c.lst.offsets), _dev(c.lst.flat)
            item_offsets = _dev(np.concatenate([seg["item_first"], seg["item_end"][-1:]]).astype(np.int32))
            call("eg_composite_fwd", ptr(splat), None, 1, ptr(offs), ptr(flat), W, H, ptr(render), ptr(alphas), ptr(last),
                 ptr(gt), ptr(wmap), c.loss_scale, ptr(vpix), ptr(loss), ptr(item_offsets), ptr(total), mi, ptr(ws),
                 gtstop.data_ptr(), hint, stream())
        else:
            item_tile = np.zeros(mi, np.int32)
            item_tile[:n_items] = seg["item_tile"]
            t = {k: _dev(seg[k]) for k in ("tile_start", "tile_end", "item_first", "item_end", "flat")}
            call("eg_composite_fwd_segments", ptr(splat), ptr(t["tile_start"]), ptr(t["tile_end"]), ptr(t["item_first"]),
                 ptr(t["item_end"]), ptr(_dev(item_tile)), ptr(t["flat"]), W, H, ptr(render), ptr(alphas), ptr(last), ptr(gt),
                 ptr(wmap), c.loss_scale, ptr(vpix), ptr(loss), ptr(total), mi, ptr(ws), gtstop.data_ptr(), hint, stream())
            out["pos"] = seg["pos"]
        torch.cuda.synchronize()
        out["words"] = gtstop.cpu().numpy()
        out["ctl"] = _ctl_words(ws, mi, T)
    torch.cuda.synchronize()
    out.update(render=render.cpu(), alphas=alphas.cpu(), last=last.cpu().numpy(),
               vpix=None if vpix is None else vpix.cpu().numpy(), loss=None if loss is None else float(loss))
    return out


@functools.lru_cache(maxsize=None)
def _d32(lengths, regime):
    c = SU.forward_case(lengths, regime)
    return SU.d32_of(c.rec, c.lst, c.f, c.mask, CU.W, CU.H)


def _check_forward(c, out, name, d32, speculative=False):
    """the per-pixel statement of one forward; returns the figures it measured"""
    keep = ~c.mask
    f = c.f
    ch = out["render"].shape[-1]
    ref = SU.fwd_ref_dict(f)
    ref["render"] = ref["render"].expand(1, CU.H, CU.W, ch)
    figs = CU.fwd_check(out["render"][None], out["alphas"][None], None, ref, torch.from_numpy(keep)[None], name)
    if c.name.startswith("grazing"):   # disjoint supports: a pixel one Gaussian reaches with alpha >= (1/255)(1 + 1e-4) is not dropped
        seen = (SU.single_alphas(c.rec, CU.W, CU.H) >= SU.AMIN * (1.0 + 1e-4)).any(axis=0)
        assert not (seen & ~keep).any() and (out["alphas"].numpy()[seen] > 0).all(), f"{name}: a quadrant dropped a Gaussian that reaches it"
    touched = keep & (f.last_idx >= 0)
    want_last = f.last_idx if "pos" not in out else out["pos"][np.maximum(f.last_idx, 0)]
    bad = touched & (out["last"] != want_last)
    assert not bad.any(), f"{name}: {int(bad.sum())} kept pixels disagree on the last contributor, first {np.argwhere(bad)[0].tolist()}"
    res = dict(alpha_rel=figs["alpha_rel"], render_row=figs["render_row"], d32=d32)
    if out["vpix"] is not None:
        v = out["vpix"].astype(np.float64)
        assert (np.sign(v)[keep] == np.sign(f.v)[keep]).all(), f"{name}: vpix has the wrong sign on a kept pixel"
        mag = np.float32(c.loss_scale).astype(np.float64) * c.wmap.astype(np.float64)
        live = keep & (f.v != 0)
        assert (np.abs(np.abs(v) - mag)[live] <= 2.0 ** -23 * mag[live]).all(), f"{name}: |vpix| is not loss_scale * w to one rounding"
        slack = SU.loss_slack(f, REG_LOSS_TOL)
        res["loss_rel"] = abs(out["loss"] - f.loss) / abs(f.loss)
        assert abs(out["loss"] - f.loss) <= slack, f"{name}: loss {out['loss']} against {f.loss} (allowed {slack:.3e})"
    if "words" in out:
        tol = max(GT_TOL_FACTOR * d32, GT_TOL_FLOOR)
        res["gT_rel"] = SU.record_check(out["words"], c.rec, f, c.mask, tol, name)
        words, _longest, miss, exit_grp = out["ctl"]
        assert not words.any() and not exit_grp.any(), f"{name}: the workspace's control words are not handed back zeroed"
        assert speculative or miss == 0, f"{name}: the miss word is raised without speculation"
    return res


FWD_CASES = [(l, r) for l in SU.FWD_LENGTHS for r in SU.FWD_REGIMES] + [("grazing", "nostop")]   # (the quadrant cull's case)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("lengths,regime", FWD_CASES)
def test_forward_tile_kernel(lib, lengths, regime, channels):
    c = SU.forward_case(lengths, regime)
    out = _forward(lib, c, "tile", channels=channels)
    res = _check_forward(c, out, f"tile-{c.name}-ch{channels}", _d32(lengths, regime))
    record("step_composite_forward", form=f"tile-ch{channels}", case=c.name, **res)


@pytest.mark.parametrize("form", ["fused-hint-1", "fused-hint0", "fused-hintlen", "unfused"])
@pytest.mark.parametrize("lengths,regime", FWD_CASES)
def test_forward_sliced(lib, lengths, regime, form):
    c = SU.forward_case(lengths, regime)
    hint = {"fused-hint-1": -1, "fused-hint0": 0, "fused-hintlen": int(np.diff(c.lst.offsets).max()), "unfused": -1}[form]
    out = _forward(lib, c, "sliced", hint=hint, max_items=3 * 2048 + 1 if form == "unfused" else None)
    res = _check_forward(c, out, f"sliced-{form}-{c.name}", _d32(lengths, regime))
    record("step_composite_forward", form=form, case=c.name, rewalk_list_word=out["ctl"][1], **res)


@pytest.mark.parametrize("lengths,regime", FWD_CASES)
def test_forward_speculate(lib, lengths, regime):
    """EG_REWALK_SPECULATE: exact and the miss word clear where no pixel stops; the miss word raised where one does"""
    c = SU.forward_case(lengths, regime)
    out = _forward(lib, c, "sliced", hint=lib.REWALK_SPECULATE)
    miss = out["ctl"][2]
    if regime == "nostop":
        assert miss == 0
        res = _check_forward(c, out, f"speculate-{c.name}", _d32(lengths, regime), speculative=True)
        record("step_composite_forward", form="speculate", case=c.name, **res)
    else:
        assert miss != 0, "a pixel stops: control word 3 must be raised"
        assert not out["ctl"][0].any(), "tickets, flags and list counter are handed back zeroed after a missed speculation too"


@pytest.mark.parametrize("lengths,regime", FWD_CASES)
def test_forward_segments(lib, lengths, regime):
    """eg_composite_fwd_segments on hand-built tables (segments shuffled, gaps between them, empty segments, item_tile
    map): the records are the classic layout's, word for word"""
    c = SU.forward_case(lengths, regime)
    out = _forward(lib, c, "segments")
    res = _check_forward(c, out, f"segments-{c.name}", _d32(lengths, regime))
    classic = _forward(lib, c, "sliced")
    assert np.array_equal(out["words"], classic["words"]), "records differ between the segmented and the classic layout"
    assert torch.equal(out["alphas"], classic["alphas"]) and out["loss"] == pytest.approx(classic["loss"], rel=REG_LOSS_TOL)
    record("step_composite_forward", form="segments", case=c.name, **res)


@pytest.mark.parametrize("form", ["tile", "sliced"])
def test_forward_zero_weight_map(lib, form):
    """wmap all zero: every gT exactly 0 (either sign), every vpix 0, the loss exactly 0"""
    c = SU.forward_case("long", "third")
    out = _forward(lib, c._replace(wmap=np.zeros_like(c.wmap)), form)
    assert out["loss"] == 0.0 and not out["vpix"].any()
    if form == "sliced":
        assert not SU.image_of_words(out["words"]).gT.any()


def _colors_id(c):
    return f"{c.scene}-ch{c.channels}-va{int(c.va)}"


@pytest.mark.parametrize("c", CU.COLORS_CASES, ids=_colors_id)
def test_colors_backward_rows(lib, c):
    """eg_composite_fwd with general colours, then eg_composite_bwd_colors from its alphas / last_ids: per pixel and per
    row against CU.ref_composite.  This backward restarts from the stored alpha = 1 - T, so a row may use
    CU.allowed_scale of its bound, exactly as in tests/test_gpu_composite_rows.py."""
    from edgegaussians_amd._lib import call, ptr, stream
    (rec,), (lst,) = CU.scene(c.scene).records, CU.lists(c.scene, c.ts)
    N, ch, W, H = rec.shape[0], c.channels, CU.W, CU.H
    col, _bg, vr, va = CU.case_inputs(c)
    splat, colors, offs, flat = _dev(rec), col.cuda().contiguous(), _dev(lst.offsets), _dev(lst.flat)
    render = torch.full((H, W, ch), NAN, device="cuda")
    alphas = torch.full((H, W), NAN, device="cuda")
    last = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    call("eg_composite_fwd", ptr(splat), ptr(colors), ch, ptr(offs), ptr(flat), W, H, ptr(render), ptr(alphas), ptr(last),
         None, None, 1.0, None, None, None, None, 0, None, None, -1, stream())
    g2d = torch.zeros(N, 8, device="cuda")          # (this kernel accumulates)
    v_colors = torch.zeros(N, ch, device="cuda")
    v_render, v_alphas = vr[0].cuda().contiguous(), None if va is None else va[0].cuda().contiguous()
    call("eg_composite_bwd_colors", ptr(splat), ptr(colors), ch, ptr(offs), ptr(flat), W, H, ptr(alphas), ptr(last),
         ptr(v_render), ptr(v_alphas), ptr(g2d), ptr(v_colors), stream())
    torch.cuda.synchronize()
    ref, kappa = CU.reference(c)
    name = f"bwd_colors-{_colors_id(c)}"
    CU.fwd_check(render.cpu()[None], alphas.cpu()[None], last.cpu()[None], ref, CU.keep_mask(c.scene, c.ts), name)
    got = {k: g2d.cpu()[:, a:b] for k, (a, b) in CU.G2D_COLS.items()}
    got["v_colors"] = v_colors.cpu()
    allowed, model = CU.allowed_scale(c), CU.model_ratio(c)
    ratio = {k: CU.grad_row_ratio(got[k], ref[k], kappa[k])[0] for k in got}
    record("step_composite_colors_rows", case=name, ratio_to_row_bound=ratio, fp32_model_ratio={k: model[k] for k in got},
           allowed_ratio={k: allowed[k] for k in got})
    for k in got:
        CU.grad_row_check(got[k], ref[k], kappa[k], f"{name} {k}", scale=allowed[k])


# ---------------------------------------------------------------------------------------------------
# 4. through the trainer
STEP_W, STEP_H, STEP_N, STEP_SCALE = 200, 136, 6000, 0.036


@functools.lru_cache(maxsize=None)
def _step_scene(regime):
    """stops: spread opacities, Gaussians three times the usual size (the recipe of tests/test_gpu_fullsize.py's small
    case): lists beyond two anchors, about a third of the pixels stop.  nostop: the reference's start (opacity 0.08), sparse."""
    from edgegaussians_amd import synth
    if regime == "stops":
        return synth.make_scene(STEP_N, 3, STEP_W, STEP_H, seed=1, anisotropy=5.0, spread_opacity=True, scale=STEP_SCALE)
    if regime == "stops_small":   # the batched step's: the same recipe with fewer Gaussians (three float64 references),
        # drawn together about the scene's centre so that every view leaves its own border tiles empty
        sc = synth.make_scene(2500, 3, STEP_W, STEP_H, seed=1, anisotropy=5.0, spread_opacity=True, scale=0.6 * STEP_SCALE)
        sc.means[:] = 0.5 + 0.6 * (sc.means - 0.5)
        return sc
    if regime == "grid":     # 52 x 52 = 2704 tiles, above kPrefixHereMaxTiles = 2560: sparse, most tiles empty
        return synth.make_scene(200, 2, 832, 832, seed=3, anisotropy=5.0, spread_opacity=True, scale=0.004)
    if regime == "cluster":  # the scene drawn together about its centre: every view leaves border tiles empty, each its own
        sc = synth.make_scene(1500, 3, STEP_W, STEP_H, seed=4, anisotropy=5.0, spread_opacity=True, scale=0.008)
        sc.means[:] = 0.5 + 0.45 * (sc.means - 0.5)
        return sc
    return synth.make_scene(1500, 3, STEP_W, STEP_H, seed=2, anisotropy=5.0, spread_opacity=False, scale=0.004)


def _trainer(sc, **kw):
    from edgegaussians_amd import EdgeTrainer
    return EdgeTrainer(sc.means, sc.log_scales, sc.quats, sc.logit_opacities, sc.viewmats, sc.Ks, sc.gt, sc.width, sc.height, **kw)


def _lists_of_trainer(tr, b=None, v=0, nonempty=None):
    """(CU.Lists in the classic compact form, pos: compact index -> slot of the device's id array) of a step's tables.
    nonempty: bool [T] from a fresh trainer's step on the same view, where an earlier step has left its own tile_end in
    the tiles this one leaves out."""
    T = tr.T
    if b is not None or tr.seg_cap:
        flat = (b["flatten_ids"][v] if b is not None else tr.flatten_ids).cpu().numpy()
        end = (b["tile_end"][v] if b is not None else tr.tile_end).cpu().numpy().astype(np.int64)
        start = np.arange(T, dtype=np.int64) * tr.seg_cap
        # (the step's sort leaves out the tiles nothing reaches: their tile_end keeps the zero it was allocated with)
        # ... and nothing else may lie outside its tile's segment.  (That every key the step counted is in the tables, and
        # none twice, is asserted below; that the ids are the right ones follows from the float64 walk over them.)
        inside = (end >= start) & (end <= start + tr.seg_cap)
        assert nonempty is not None or (end[~inside] == 0).all(), "a tile_end outside its segment that is not the initial zero"
        end = np.where(inside, end, start)
        if nonempty is not None:
            end = np.where(nonempty, end, start)
        total = (b["total"][v] if b is not None else tr.total).cpu().numpy()
        assert int((end - start).sum()) == int(total[0]) and int(total[1]) == 0, "the tables hold every key the step counted"
    else:
        flat = tr.flatten_ids.cpu().numpy()
        offs = tr.offsets.cpu().numpy().astype(np.int64)
        start, end = offs[:-1], offs[1:]
    lens = end - start
    assert (lens >= 0).all()
    pos = np.concatenate([np.arange(s, e) for s, e in zip(start, end)] + [np.zeros(0, np.int64)])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return CU.Lists(offsets, np.ascontiguousarray(flat[pos], np.int32)), pos


_step_refs = {}


def _step_reference(rec, lst, gt, wmap, loss_scale, W, H):
    """float64 forward, borderline mask (forward + record-driven) and -- from the REFERENCE's record image -- the float64
    rows and kappa, cached on the bytes of the device's records and lists"""
    key = (rec.tobytes(), lst.flat.tobytes(), lst.offsets.tobytes(), None if wmap is None else wmap.tobytes(), gt.tobytes())
    if key not in _step_refs:
        assert SU.lists_sorted(rec, lst), "a tile list is not sorted by (depth bits, id)"
        f = SU.ref_forward(rec, lst, W, H, gt, wmap, loss_scale)
        mask = SU.forward_borderline(rec, lst, W, H, f, gt) | SU.record_borderline(rec, W, H)
        img = SU.record_of(f, mask)
        ref, kappa = SU.record_kappa(rec, img, W, H)
        _step_refs[key] = (f, mask, ref, kappa, SU.d32_of(rec, lst, f, mask, W, H))
    return _step_refs[key]


def _masked_weights(tr, sc, view, read):
    """the weight map of `view` with zero weight on the borderline pixels of the DEVICE's own records and lists: one
    probing step reads those back (they do not depend on the weights)"""
    from edgegaussians_amd import synth
    w = synth.weight_map("weighted", sc.gt[view]).numpy().astype(np.float32)
    rec, lst = read()
    f0 = SU.ref_forward(rec, lst, sc.width, sc.height, sc.gt[view].numpy(), w, tr.loss_scale)
    mask = SU.forward_borderline(rec, lst, sc.width, sc.height, f0, sc.gt[view].numpy()) | SU.record_borderline(rec, sc.width, sc.height)
    assert float(mask.mean()) < SU.BORDER_SHARE_CAP, float(mask.mean())
    return np.where(mask, np.float32(0.0), w)


def _check_step(name, rec, lst, words, g2d, loss, gt, wmap, loss_scale, W, H, empty=None):
    f, mask, ref, kappa, d32 = _step_reference(rec, lst, gt, wmap, loss_scale, W, H)
    assert not wmap[mask].any()
    tol = max(GT_TOL_FACTOR * d32, GT_TOL_FLOOR)
    gT_rel = SU.record_check(words, rec, f, mask, tol, name, empty=empty)
    if empty is not None:    # pixels this step did not write hold nothing, as far as its backward may tell
        words = words.copy()
        words[empty] = (0, -1, -1)
    # (i) the backward from the device's OWN record image (kappa: the reference image's, the two differ by rounding)
    own = SU.ref_backward(rec, SU.image_of_words(words), W, H)
    r_own = _rows_check(g2d, own, kappa, f"{name} from its own records")
    # (ii) ... and from the reference's: closes the loop
    r_ref = _rows_check(g2d, ref, kappa, f"{name} from the reference's records")
    if loss is not None:
        slack = SU.loss_slack(f, REG_LOSS_TOL)
        assert abs(loss - f.loss) <= slack, f"{name}: loss {loss} against {f.loss} (allowed {slack:.3e})"
    res = dict(case=name, gaussians=int(rec.shape[0]), largest_list=int(np.diff(lst.offsets).max()), stopped_share=float(f.stopped.mean()),
               borderline_share=float(mask.mean()), d32=d32, gT_rel=gT_rel, ratio_own_records=r_own, ratio_reference_records=r_ref,
               loss_rel=None if loss is None else abs(loss - f.loss) / abs(f.loss))
    record("step_composite_through_trainer", **res)
    return f, mask, res


STEP_PATHS = {   # name: (scene regime, trainer arguments, journalled with rewalk_hint 0)
    "default": ("stops", {}, False),
    "speculative": ("nostop", {}, True),
    "keep_images": ("stops", dict(keep_images=True), False),
    "classic": ("stops", dict(segmented=False), False),
    "large_grid": ("grid", {}, False),
}


@pytest.mark.parametrize("path", list(STEP_PATHS))
def test_step_records_and_rows(lib, path):
    regime, kw, speculative = STEP_PATHS[path]
    sc = _step_scene(regime)
    W, H, view = sc.width, sc.height, 1
    gt = sc.gt[view].numpy()

    def run(wmap):
        tr = _trainer(sc, **kw)
        tr.ensure_capacity(views=[view])
        if speculative:
            tr.rewalk_hint = 0
            tr._args_cache = {}
            assert tr._rewalk_arg(True) == lib.REWALK_SPECULATE
        tr.g2d.fill_(NAN)
        tr.grad_step(view, _dev(wmap), journalled=speculative)
        torch.cuda.synchronize()
        return tr

    w0 = np.full((H, W), np.float32(1.0 / (H * W)))
    tr = run(w0)
    wmap = _masked_weights(tr, sc, view, lambda: (tr.splat.cpu().numpy(), _lists_of_trainer(tr)[0]))
    tr = run(wmap)
    rec, (lst, pos) = tr.splat.cpu().numpy(), _lists_of_trainer(tr)
    words = tr.gtstop.view(torch.int32).cpu().numpy()
    g2d = tr.g2d.cpu()
    loss = tr.pop_loss()
    assert not tr.overflowed()
    # which path ran, from what the trainer holds afterwards: the layout it binned in, the images it was asked to keep
    assert bool(tr.seg_cap) == bool(kw.get("segmented", True)) and (tr.render is not None) == bool(kw.get("keep_images"))
    if speculative:
        assert tr.rewalk_misses == 0, "the speculative forward saw a stop"
    f, mask, res = _check_step(f"step-{path}", rec, lst, words, g2d, loss, gt, wmap, tr.loss_scale, W, H)
    if regime == "stops":
        assert res["largest_list"] > 16 * 128 and 0.03 < res["stopped_share"] < 0.6, res
    elif regime == "grid":   # the front-prefix record order; empty tiles ARE written; no one-kernel backward up here
        assert tr.T == 2704 and float((np.diff(lst.offsets) == 0).mean()) > 0.5
    else:
        assert res["stopped_share"] == 0.0
    if path == "keep_images":
        out = dict(render=tr.render.cpu()[..., None], alphas=tr.alphas.cpu(), last=tr.last_ids.cpu().numpy())
        ref = SU.fwd_ref_dict(f)
        CU.fwd_check(out["render"][None], out["alphas"][None], None, ref, torch.from_numpy(~mask)[None], "step-keep_images")
        touched = ~mask & (f.last_idx >= 0)
        assert (out["last"][touched] == pos[f.last_idx[touched]]).all(), "last_ids of the chained kernel"


def test_batched_step_records_and_rows(lib):
    """grad_step_batched with three views of different coverage: every view's records and rows on their own"""
    sc = _step_scene("stops_small")
    W, H, views = sc.width, sc.height, [0, 1, 2]

    def run(wmaps):
        tr = _trainer(sc)
        tr.ensure_capacity(views=views)
        tr.grad_step_batched(views, [_dev(w) for w in wmaps])
        torch.cuda.synchronize()
        return tr

    w0 = np.full((H, W), np.float32(1.0 / (H * W)))
    tr = run([w0] * 3)
    b = tr._batches[3]
    wmaps = [_masked_weights(tr, sc, v, lambda k=k: (b["splat"][k].cpu().numpy(), _lists_of_trainer(tr, b, k)[0]))
             for k, v in enumerate(views)]
    tr = run(wmaps)
    b = tr._batches[3]
    total = tr.pop_loss()
    assert not tr.overflowed()
    want = slack = 0.0
    covered = []
    for k, v in enumerate(views):
        rec, (lst, _pos) = b["splat"][k].cpu().numpy(), _lists_of_trainer(tr, b, k)
        words = b["gtstop"][k].view(torch.int32).cpu().numpy()
        f, _mask, _res = _check_step(f"batched-view{v}", rec, lst, words, b["g2d"][k].cpu(), None, sc.gt[v].numpy(), wmaps[k],
                                     tr.loss_scale, W, H)
        want += f.loss
        slack += SU.loss_slack(f, REG_LOSS_TOL)
        covered.append(tuple(np.diff(lst.offsets) > 0))
    assert len(set(covered)) == 3 and not all(all(c) for c in covered), "three views of different coverage"
    assert abs(total - want) <= slack, (total, want, slack)


def test_second_step_ignores_the_records_an_earlier_view_left(lib):
    """Two steps on one trainer, two views: the wave forward does not write the pixels of tiles the current view
    leaves empty, so they keep the first view's records; the second step's g2d must be the float64 backward from a
    record image in which those pixels hold nothing."""
    sc = _step_scene("cluster")
    W, H, first, second = sc.width, sc.height, 0, 2
    from edgegaussians_amd import synth

    def run(steps):
        tr = _trainer(sc)
        tr.ensure_capacity(views=[first, second])
        for v, w in steps:
            tr.g2d.fill_(NAN)
            tr.grad_step(v, _dev(w))
        torch.cuda.synchronize()
        return tr

    w0 = np.full((H, W), np.float32(1.0 / (H * W)))
    tr = run([(second, w0)])
    nonempty = np.diff(_lists_of_trainer(tr)[0].offsets) > 0
    wmap = _masked_weights(tr, sc, second, lambda: (tr.splat.cpu().numpy(), _lists_of_trainer(tr)[0]))
    w_first = synth.weight_map("weighted", sc.gt[first]).numpy().astype(np.float32)
    tr = run([(first, w_first)])
    lens_first = np.diff(_lists_of_trainer(tr)[0].offsets)
    words_first = tr.gtstop.view(torch.int32).cpu().numpy()
    tr = run([(first, w_first), (second, wmap)])
    rec, (lst, _pos) = tr.splat.cpu().numpy(), _lists_of_trainer(tr, nonempty=nonempty)
    words = tr.gtstop.view(torch.int32).cpu().numpy()
    g2d = tr.g2d.cpu()
    tr.pop_loss()
    assert not tr.overflowed()
    tw, th = SU.tiles_of(W, H)
    left = (np.diff(lst.offsets) == 0) & (lens_first > 0)           # tiles the first view covered and the second leaves empty
    assert left.sum() >= 3, "the views must differ in the tiles they cover"
    empty = np.kron((np.diff(lst.offsets) == 0).reshape(th, tw), np.ones((16, 16), bool))[:H, :W]
    stale = np.kron(left.reshape(th, tw), np.ones((16, 16), bool))[:H, :W]
    assert np.array_equal(words[stale], words_first[stale]) and (SU.image_of_words(words_first).gT[stale] != 0).any(), \
        "the pixels of those tiles keep the first view's records, some of them non-zero"
    _check_step("step-second-of-two", rec, lst, words, g2d, None, sc.gt[second].numpy(), wmap, tr.loss_scale, W, H, empty=empty)
