"""What tests/test_gpu_composite_rows.py rests on, shown from the references alone (no GPU).

The scenes of tests/composite_util.py meet the conditions the device tests need (several staging batches in every
tile, last contributors in every batch, stopped / capped / untouched pixels, an empty tile, Gaussians with no gradient);
the case table launches every instantiation of the three chunked compositing families; a plain fp32 evaluation
(oracle.ref_torch.composite in float32 on the same lists) agrees with float64 on every kept pixel's last contributor and
uses at most HALF of every bound; and the row checks reject three planted defects, one of which assert_close passes.

Measured here (fp32 oracle against float64, cases of FP32_CASES): gradients at most 0.21 of the row bound, forward rows
at most 5.4e-6 relative (the alpha of a sparse-scene pixel; 6.3e-7 on the dense scene), rows whose relative bound
ROW_FLOOR + ROW_KAPPA_FACTOR kappa_r exceeds 1e-3 at most 4.2 % of a tensor's live rows on the dense scene (v_opacities,
v_depths) and 2 of 23 rows on the sparse one.  The projection tests cap the share of rows looser than ROW_LOOSE = 1e-4 at
3 %; that cap does NOT hold for compositing -- 12 to 50 % of the dense scene's rows exceed 1e-4, because a Gaussian's
gradient is a signed sum over pixels whose cotangents are signed, and cancels -- so the cap asserted here is 10 % at 1e-3.

The kernels' backward order (CU.walk32, a numpy fp32 model): started from the forward's own T it stays within 0.49 of
the row bound; started from T_final = 1 - alphas, as the entries' interface (and gsplat's) has it, it reaches 30.6 x the
bound on the dense scene (33.3 x over all device cases) and 1.1 x on the two-camera set, and changes nothing on the sparse
scene, which has no pixel at the transmittance stop.  The digits go in ONE operation: alphas = 1 - T is rounded to
2^-25 absolute, which is 3e-4 of a T_final at the 1e-4 stop, and every term of such a pixel carries that factor.
"""
import math

import numpy as np
import pytest
import torch

from tests import composite_util as CU
from tests.util import FWD_ROW_TOL, assert_close, record_cpu

FP32_CASES = (CU.case("ts", 8, 0, 1, 0), CU.case("ts", 8, 2, 1, 1), CU.case("ts", 8, 32, 0, 1),
              CU.case("modes", 16, 1, 1, 0), CU.case("modes", 16, 3, 1, 1), CU.case("wide", 16, 32, 1, 1),
              CU.case("ts", 32, 4, 0, 0), CU.case("ts", 32, 32, 1, 1),
              CU.case("wide", 16, 8, 1, 1, n_real=5), CU.case("ts", 32, 32, 1, 0, n_real=17),
              CU.case("wide", 16, 2, 1, 0, scene="sparse"), CU.case("ts", 32, 32, 1, 1, scene="twocam", per_camera=True))


def _oracle32(c):
    col, bg, vr, va = CU.case_inputs(c)
    return CU.ref_composite(CU.scene(c.scene).records, col, bg, c.depth, CU.lists(c.scene, c.ts), c.ts, vr, va,
                            dtype=torch.float32)


def _tile_max(a, ts):
    tw, th = math.ceil(CU.W / ts), math.ceil(CU.H / ts)
    return np.array([a[ty * ts:(ty + 1) * ts, tx * ts:(tx + 1) * ts].max() for ty in range(th) for tx in range(tw)])


@pytest.mark.parametrize("ts", [8, 16, 32])
def test_scenes_meet_the_conditions_of_the_device_tests(ts):
    stage = CU.STAGE[ts]
    if ts != 16:
        from edgegaussians_amd import _lib
        assert _lib.TS_STAGE_BATCH[ts] == stage
    (dense,), (sparse,) = CU.walks("dense", ts), CU.walks("sparse", ts)
    reach = _tile_max(dense.looked, ts)
    batches = np.unique(dense.last_batch).tolist()
    ref, _ = CU.reference(CU.case("ts", ts, 2, 1, 1))
    zero_rows = int((CU._rows(ref["v_means2d"]).abs().amax(1) == 0).sum())
    pixels = CU.W * CU.H
    rec = dict(tile_size=ts, dense_list_lengths=[int(dense.lens.min()), int(dense.lens.max())],
               shortest_longest_walk_of_a_tile=int(reach.min()), last_contributor_batches=batches,
               stopped_pixels=dense.stopped, capped_contributions=dense.capped, borderline_pixels=int(dense.mask.sum()),
               zero_gradient_rows=zero_rows, sparse_untouched_pixels=int((sparse.last_batch < 0).sum()),
               sparse_list_lengths=[int(sparse.lens.min()), int(sparse.lens.max())],
               twocam_list_lengths=[[int(w.lens.min()), int(w.lens.max())] for w in CU.walks("twocam", ts)])
    record_cpu("composite_scene_conditions", **rec)
    print(rec)
    assert reach.min() > 2 * stage, "every tile's longest walk must enter a third staging batch"
    assert batches == list(range(max(batches) + 1)) and max(batches) >= 2, "every batch must hold a last contributor"
    assert dense.stopped > 0.05 * pixels and dense.capped >= 1 and zero_rows > 0
    assert int(dense.mask.sum()) <= 0.01 * pixels, "borderline set too large to be a useful exclusion"
    assert (sparse.last_batch < 0).sum() > 0.5 * pixels and sparse.lens[0] == 0 and 0 < sparse.lens.max() < stage
    two = CU.walks("twocam", ts)
    assert int(two[0].lens.sum()) != int(two[1].lens.sum()), "the second camera's list base must differ from a multiple of the first"
    for name in ("sparse", "twocam"):
        assert sum(int(w.mask.sum()) for w in CU.walks(name, ts)) <= 0.01 * pixels * len(CU.walks(name, ts))
    # partial tiles on both axes; at 32 whole 16 x 16 quadrants outside the image and others partly outside
    assert CU.W % ts and CU.H % ts
    if ts == 32:
        quads = [(i0, j0) for i0 in range(0, 32 * math.ceil(CU.H / 32), 16) for j0 in range(0, 32 * math.ceil(CU.W / 32), 16)]
        outside = [q for q in quads if q[0] >= CU.H or q[1] >= CU.W]
        partly = [q for q in quads if q not in outside and (q[0] + 16 > CU.H or q[1] + 16 > CU.W)]
        assert len(outside) >= 1 and len(partly) >= 2


def to64(t):
    return t.double().numpy()


def test_untouched_pixels_have_exactly_zero_alpha_in_the_reference():
    for ts in (8, 16, 32):
        ref, _ = CU.reference(CU.case("ts", ts, 2, 1, 1, scene="sparse"))
        (w,) = CU.walks("sparse", ts)
        assert (to64(ref["alphas"])[0][w.last_batch < 0] == 0).all() and (to64(ref["alphas"])[0][w.last_batch >= 0] > 0).all()


def test_case_table_launches_every_instantiation():
    """48 ts kernels with colours + 2 x 2 depth-only, 20 x 2 wide, 7 x 2 mode instantiations: each is the kernel of a
    dense-scene case (forward and backward run in the same case); 2 x 2 mode instantiations without depth and
    background: each the kernel of a CU.COLORS_CASES case on the dense scene."""
    got = {CU.kernel_of(c) for c in CU.DENSE_CASES + CU.COLORS_CASES}
    assert got == CU.DISPATCH
    # (+ 2: the (DEPTH, BG) = (0, 0) mode kernels, which only eg_composite_fwd / eg_composite_bwd_colors reach)
    assert {CU.kernel_of(c) for c in CU.COLORS_CASES} == {("modes", 16, 1, False, False), ("modes", 16, 3, False, False)}
    assert not {CU.kernel_of(c) for c in CU.DENSE_CASES} & {CU.kernel_of(c) for c in CU.COLORS_CASES}
    assert len([k for k in got if k[0] == "ts" and k[2] >= 8]) == 24 and len(got) == 42 + 20 + 7 + 2
    assert all(c.scene == "dense" and c.n_real == c.channels for c in CU.DENSE_CASES)
    for fam in ("ts", "wide", "modes"):  # the cross-section: one narrow and one widest case per family and scene
        for s in ("sparse", "twocam"):
            chs = sorted(c.channels for c in CU.CROSS_CASES if c.family == fam and c.scene == s)
            assert chs[0] <= 2 and chs[-1] == (3 if fam == "modes" else 32)


@pytest.mark.parametrize("c", FP32_CASES, ids=lambda c: f"{c.scene}-{c.ts}-{c.n_real}-d{int(c.depth)}b{int(c.bg)}")
def test_fp32_oracle_uses_at_most_half_of_every_bound(c):
    ref, kappa = CU.reference(c)
    got = _oracle32(c)
    keep = CU.keep_mask(c.scene, c.ts)
    f = CU.fwd_check(got["render"], got["alphas"], got["last_ids"], ref, keep, "fp32 oracle", tol=0.5 * FWD_ROW_TOL)
    rec = dict(scene=c.scene, tile_size=c.ts, channels=c.n_real, depth=c.depth, bg=c.bg, forward=f, ratio={}, loose={},
               over_1e3={})
    for name in CU.grad_names(c):
        ratio, loose = CU.grad_row_check(CU._rows(got[name]), ref[name], kappa[name], f"fp32 oracle {name}", scale=0.5)
        rec["ratio"][name], rec["loose"][name] = ratio, loose
        rec["over_1e3"][name] = CU.grad_row_ratio(CU._rows(got[name]), ref[name], kappa[name])[2]
        assert rec["over_1e3"][name] <= 0.10, f"{name}: {rec['over_1e3'][name]:.3f} of the live rows have a bound above 1e-3"
    record_cpu("composite_fp32_oracle_vs_float64", **rec)
    print(rec)


@pytest.mark.parametrize("c", FP32_CASES, ids=lambda c: f"{c.scene}-{c.ts}-{c.n_real}-d{int(c.depth)}b{int(c.bg)}")
def test_fp32_model_of_the_kernel_order_loses_digits_only_through_the_stored_alpha(c):
    """CU.walk32 -- fp32, front to back, then back to front by T *= 1 / (1 - alpha) -- holds every row bound when its
    backward starts from the forward's own T; started from T_final = 1 - alphas as the kernels' (and gsplat's) interface
    has it, the rows fed by pixels at the transmittance stop exceed the bound (the figure the device is held to twice
    of), and on a scene without stopped pixels nothing changes."""
    ref, kappa = CU.reference(c)
    exact = CU.walk32(c, stored_alpha=False)
    ratio_exact = {k: CU.grad_row_check(CU._rows(exact[k]), ref[k], kappa[k], f"fp32 model from T {k}")[0]
                   for k in CU.grad_names(c)}
    stored = CU.model_ratio(c)
    stopped = sum(w.stopped for w in CU.walks(c.scene, c.ts))
    record_cpu("composite_fp32_model_vs_float64", scene=c.scene, tile_size=c.ts, channels=c.n_real, depth=c.depth,
               bg=c.bg, stopped_pixels=stopped, ratio_from_forward_T=ratio_exact, ratio_from_stored_alpha=stored)
    print(c.scene, c.ts, c.n_real, stopped, ratio_exact, stored)
    if stopped == 0:
        assert all(abs(stored[k] - ratio_exact[k]) <= 0.05 for k in stored) and max(stored.values()) <= 0.5
    elif c.scene == "dense":
        assert min(stored.values()) > 1.0 and max(stored.values()) < 64.0


# ---------------------------------------------------------------------------------------------------
# sensitivity: planted defects on a copy of the fp32 oracle's result
MUT = CU.case("wide", 16, 4, 1, 1)


def _pixel_terms(c, i, j, skip=None):
    """One pixel's forward row, alpha and share of every gradient, fp32 autograd over its tile's list with entry `skip`
    (index into the list) left out of the walk."""
    col, bg, vr, va = CU.case_inputs(c)
    rec = torch.from_numpy(CU.scene(c.scene).records[0])
    l = CU.lists(c.scene, c.ts)[0]
    tw = math.ceil(CU.W / c.ts)
    t = (i // c.ts) * tw + j // c.ts
    ids = [k for k in range(int(l.offsets[t]), int(l.offsets[t + 1])) if k != skip]
    g = torch.from_numpy(l.flat[ids]).long()
    m, con, op, cc, dep = [x.clone().requires_grad_(True) for x in (rec[:, 0:2], rec[:, 2:5], rec[:, 5], col, rec[:, 6])]
    dx, dy = m[g, 0] - (j + 0.5), m[g, 1] - (i + 0.5)
    sigma = 0.5 * (con[g, 0] * dx * dx + con[g, 2] * dy * dy) + con[g, 1] * dx * dy
    alpha = torch.clamp(op[g] * torch.exp(-sigma), max=CU.AMAX)
    with torch.no_grad():
        valid = (sigma >= 0) & (alpha >= CU.AMIN)
        nT = torch.cumprod(1 - torch.where(valid, alpha, torch.zeros_like(alpha)), 0)
        contrib = valid & ~(torch.cummax((nT <= CU.TSTOP).to(torch.int8), 0).values > 0)
    a = torch.where(contrib, alpha, torch.zeros_like(alpha))
    cp = torch.cumprod(1 - a, 0)
    w = a * torch.cat([torch.ones(1), cp[:-1]])
    full = torch.cat([cc[g], dep[g][:, None]], -1) if c.depth else cc[g]
    pix = w @ full + cp[-1] * torch.cat([bg[0], torch.zeros(int(c.depth))])
    loss = (pix * vr[0, i, j]).sum() + (1 - cp[-1]) * va[0, i, j]
    grads = torch.autograd.grad(loss, (m, con, op, cc, dep))
    names = ("v_means2d", "v_conics", "v_opacities", "v_colors", "v_depths")
    out = {n: (gr if gr.dim() == 2 else gr[:, None]).detach()[None] for n, gr in zip(names, grads)}
    out.update(render=pix.detach(), alpha=(1 - cp[-1]).detach(), contrib=contrib, ids=ids)
    return out


def _rejected(got, ref, kappa, names):
    bad = []
    for name in names:
        try:
            CU.grad_row_check(CU._rows(got[name]), ref[name], kappa[name], name)
        except AssertionError:
            bad.append(name)
    return bad


def test_row_checks_reject_planted_defects():
    c = MUT
    ref, kappa = CU.reference(c)
    base = _oracle32(c)
    keep = CU.keep_mask(c.scene, c.ts)
    names = [n for n in CU.GRAD_NAMES if n != "absgrad"]
    assert _rejected(base, ref, kappa, CU.GRAD_NAMES) == []
    CU.fwd_check(base["render"], base["alphas"], base["last_ids"], ref, keep, "fp32 oracle")

    # (a) 1 % on the rows whose maximum is below 1e-3 of the tensor's: invisible to the max-norm check
    mut = {k: v.clone() for k, v in base.items()}
    n_small = {}
    for name in names:
        sig = mut[name].abs().amax(-1, keepdim=True)
        small = (sig > 0) & (sig < 1e-3 * sig.max())
        n_small[name] = int(small.sum())
        mut[name] = torch.where(small, mut[name] * 1.01, mut[name])
        assert_close(mut[name], ref[name], rtol=1e-4, name=name)   # passes
    assert min(n_small.values()) > 0, n_small
    assert _rejected(mut, ref, kappa, names) == names

    # (b) one pixel skips the first entry of its second staging batch
    (walk,) = CU.walks(c.scene, c.ts)
    l = CU.lists(c.scene, c.ts)[0]
    tw = math.ceil(CU.W / c.ts)
    found = None
    for i in range(CU.H):
        for j in range(CU.W):
            if keep[0, i, j] and walk.last_batch[i, j] >= 1:
                t = (i // c.ts) * tw + j // c.ts
                whole = _pixel_terms(c, i, j)
                if whole["contrib"][CU.STAGE[c.ts]]:
                    found = (i, j, int(l.offsets[t]) + CU.STAGE[c.ts], whole)
                    break
        if found:
            break
    assert found, "no kept pixel to which the first entry of a second batch contributes"
    i, j, skip, whole = found
    less = _pixel_terms(c, i, j, skip)
    mut = {k: v.clone() for k, v in base.items()}
    for name in names:
        mut[name] = mut[name] - whole[name] + less[name]
    mut["render"][0, i, j] += less["render"] - whole["render"]
    mut["alphas"][0, i, j] += less["alpha"] - whole["alpha"]
    with pytest.raises(AssertionError):
        CU.fwd_check(mut["render"], mut["alphas"], mut["last_ids"], ref, keep, "skipped entry")
    bad_b = _rejected(mut, ref, kappa, names)
    assert "v_colors" in bad_b and "v_opacities" in bad_b, bad_b

    # (c) one Gaussian's v_colors row misses one tile's share (a lost atomic): the share of the tile that gives it the
    #     least, among those that give at least 1e-3 of the row
    col, bg, vr, va = CU.case_inputs(c)
    gauss = int(np.bincount(l.flat, minlength=col.shape[0]).argmax())
    shares = []
    for t in range(len(l.offsets) - 1):
        if gauss in l.flat[l.offsets[t]:l.offsets[t + 1]]:
            ty, tx = divmod(t, tw)
            sel = torch.zeros(1, CU.H, CU.W)
            sel[0, ty * c.ts:(ty + 1) * c.ts, tx * c.ts:(tx + 1) * c.ts] = 1.0
            part = CU.ref_composite(CU.scene(c.scene).records, col, bg, c.depth, CU.lists(c.scene, c.ts), c.ts,
                                    vr * sel[..., None], va * sel, dtype=torch.float32)["v_colors"][0, gauss]
            shares.append(part)
    row = base["v_colors"][0, gauss]
    shares = [s for s in shares if float(s.abs().max()) >= 1e-3 * float(row.abs().max())]
    assert len(shares) >= 2
    mut = {k: v.clone() for k, v in base.items()}
    mut["v_colors"][0, gauss] -= min(shares, key=lambda s: float(s.abs().max()))
    assert _rejected(mut, ref, kappa, ["v_colors"]) == ["v_colors"]
    record_cpu("composite_planted_defects", small_rows=n_small, skipped_entry_pixel=[i, j], rejected_b=bad_b,
               lost_share_gaussian=gauss, tiles_of_that_gaussian=len(shares))
