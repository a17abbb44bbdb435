"""The conditions the device tests of the orientation regularisers (tests/test_gpu_regularizers.py) rest on, checked on
the CPU with the references alone (tests/util.py: ref_direction_loss, ref_ratio_loss, ref_regulariser_step):

* the float64 references reproduce the reference implementation's own outputs (tests/golden/regularizers.npz);
* every scene reaches the branch it was built for (same-block shares, -1 tails, coincident neighbours, ties, dot == 0),
  and contains no entry on which two correct fp32 evaluations may differ by a whole term (|dot| or a top_k selection
  gap within rounding of zero);
* the fp32 torch evaluation of the reference stays within a quarter of the per-row bound on every scene the device
  tests use, so that a device failure says something about the kernel;
* the elements left out of the Adam delta comparison are at most 0.1 %, and a correct fp32 Adam meets the bound."""
import os

import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import assert_close, record_cpu, rel_err

SCENES = ("curve", "shuffled", "edges", "k32")


def _fp32_rows(m, q, s, nn, top_k, ref):
    l64, gm64, gq64 = ref
    l32, gm32, gq32 = U.ref_direction_loss(m, q, s, nn, top_k, dtype=torch.float32)
    loss_err = abs(float(l32) - float(l64)) / abs(float(l64))
    return loss_err, U.row_rel_ratio(gm32, gm64), U.row_rel_ratio(gq32, gq64)


@pytest.mark.parametrize("tag", ["enforce_full_5", "enforce_full_10", "enforce_half_5", "enforce_half_10"])
def test_references_reproduce_the_reference_functions(golden_dir, tag):
    """ref_direction_loss / ref_ratio_loss in float64 against edge_gs.py:346-380 run by the reference itself (fp32 torch
    autograd, tests/golden/make_golden.py:regularizers), on its own neighbour tables: 1e-4 max-norm."""
    d = np.load(os.path.join(golden_dir, "regularizers.npz"))
    m, q, s = (torch.from_numpy(d[k]) for k in ("means", "quats", "log_scales"))
    k = int(tag.rsplit("_", 1)[1])
    loss, gm, gq = U.ref_direction_loss(m, q, s, d[f"nn_{tag}"], k if tag.startswith("enforce_half") else 0)
    e = {"loss": abs(float(loss) - float(d[f"dir_loss_{tag}"])) / abs(float(d[f"dir_loss_{tag}"])),
         "gmeans": rel_err(d[f"dir_gmeans_{tag}"], gm), "gquats": rel_err(d[f"dir_gquats_{tag}"], gq)}
    r, gs = U.ref_ratio_loss(s)
    e["ratio"] = abs(float(r) - float(d["ratio_loss"])) / float(d["ratio_loss"])
    e["gscales"] = rel_err(d["ratio_gscales"], gs)
    record_cpu("regulariser_references_vs_golden", tag=tag, max_rel_err=e)
    assert e["loss"] <= 1e-6 and e["ratio"] <= 1e-6, e
    assert_close(d[f"dir_gmeans_{tag}"], gm, rtol=1e-4, name="dmeans")
    assert_close(d[f"dir_gquats_{tag}"], gq, rtol=1e-4, name="dquats")
    assert_close(d["ratio_gscales"], gs, rtol=1e-4, name="dlogscales")


def test_scenes_reach_their_branches():
    m, q, s, nn, _ = U.reg_scene("curve")
    share_curve = U.same_block_share(nn)
    assert m.shape[0] == U.REG_BLOCK_N and share_curve >= 0.9, share_curve      # the LDS path carries the sum
    m2, q2, s2, nn2, _ = U.reg_scene("shuffled")
    share_shuffled = U.same_block_share(nn2)
    assert m2.shape[0] == 2048 and share_shuffled <= 0.2, share_shuffled        # the global-atomic path does
    assert torch.equal(torch.sort(m[:, 0]).values, torch.sort(m2[:, 0]).values)  # the same points
    # K = 32 on a synthetic table: the row itself and a repeated index in every row
    _, _, _, nn32, _ = U.reg_scene("k32")
    rows = torch.arange(nn32.shape[0], dtype=torch.int32)
    assert nn32.shape[1] == 32 and (nn32 == rows[:, None]).any(dim=1).all() and (nn32[:, 1] == nn32[:, 2]).all()
    assert int(nn32.min()) >= 0 and int(nn32.max()) < nn32.shape[0]
    # sizes: -1 tails at N = 1 and N = 2, none above K
    neg = {}
    for n in U.REG_SIZES:
        pts = U.reg_scene(f"size{n}")[0]
        for K in U.REG_SIZE_KS:
            t = U.cpu_knn(pts, K)
            neg[(n, K)] = int((t < 0).sum())
            assert neg[(n, K)] == n * max(K - (n - 1), 0)
            assert int(t.max()) < n
    assert neg[(1, 5)] == 5 and neg[(2, 5)] == 8 and neg[(255, 20)] == 0
    record_cpu("regulariser_scene_conditions", same_block_share_curve=share_curve, same_block_share_shuffled=share_shuffled,
               negative_entries={f"{n}x{K}": v for (n, K), v in neg.items()})


def test_edges_scene_holds_every_class():
    m, q, s, nn, rows = U.reg_scene("edges")
    n_curve = m.shape[0] - U.EDGE_PER_CLASS * len(U.EDGE_CLASSES)
    assert set(rows) == set(U.EDGE_CLASSES) and nn.shape == (m.shape[0], U.EDGES_K)
    assert int(nn[:n_curve].max()) < n_curve                      # nobody lists an appended row unless stated
    t = U.ref_direction_terms(m, q, s, nn, 0)
    for r in rows["duplicate"]:                                    # sits exactly on the neighbour of slot 0
        assert torch.equal(m[r], m[nn[r, 0]]) and not t["valid"][r, 0] and t["valid"][r, 1:].all()
    for r in rows["ulp"]:                                          # one ulp apart in x at 0.5, identical otherwise
        j = int(nn[r, 0])
        assert j in rows["ulp"] and abs(float(m[r, 0]) - float(m[j, 0])) == 2.0 ** -24 and torch.equal(m[r, 1:], m[j, 1:])
        assert abs(float(m[r, 0]) - 0.5) <= 2.0 ** -24
    _, gm, gq = U.reg_reference("edges", top_k=0)
    w = 1.0 / (m.shape[0] * U.EDGES_K)
    assert float(gm[rows["ulp"]].abs().max()) / w > 1e6           # raw gradient ~1e7
    for k, r in enumerate(rows["dot_zero"]):                       # dot == 0 exactly: the row is exactly zero
        j = rows["dot_zero_partner"][k]
        assert nn[r].tolist() == [j] + [-1] * (U.EDGES_K - 1)
        assert float(m[r, 0]) == float(m[j, 0]) and float(m[r, 2]) == float(m[j, 2]) and float(m[r, 1]) != float(m[j, 1])
        assert t["valid"][r, 0] and float(t["dot"][r, 0]) == 0.0
        assert not gm[r].any() and not gq[r].any()
    assert not (nn == torch.tensor(rows["dot_zero"])[:, None, None]).any()    # and nobody scatters into it
    nq = q.norm(dim=1)
    assert torch.allclose(nq[rows["quat_tiny"]], torch.tensor(1e-3), rtol=1e-5)
    assert torch.allclose(nq[rows["quat_huge"]], torch.tensor(1e3), rtol=1e-5)
    for r in rows["two_equal_major"]:                              # the maximum is attained twice
        assert int((s[r] == s[r].max()).sum()) == 2
    for r in rows["two_equal_minor"]:
        assert int((s[r] == s[r].min()).sum()) == 2 and int((s[r] == s[r].max()).sum()) == 1
    for r in rows["three_equal"]:
        assert int((s[r] == s[r, 0]).sum()) == 3
    # the ratio loss on the ties: -r to the first maximum, +r to the first of the rest (r = 1 where the maximum is double)
    _, gs = U.ref_ratio_loss(s)
    N = s.shape[0]
    for r, want in ((rows["two_equal_major"][0], [-1.0, 1.0, 0.0]), (rows["two_equal_major"][1], [0.0, -1.0, 1.0]),
                    (rows["three_equal"][0], [-1.0, 1.0, 0.0])):
        assert torch.allclose(gs[r] * N, torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0) and (gs[r] == 0).sum() == 1
    g = gs[rows["two_equal_minor"][0]] * N
    assert float(g[0]) < 0 and float(g[1]) == -float(g[0]) and float(g[2]) == 0.0


@pytest.mark.parametrize("name", SCENES)
def test_fp32_reference_within_a_quarter(name):
    """... of the per-row bound on every (scene, top_k) the device test runs; and no |dot| or selection gap within
    rounding of zero.  `edges`: the small-remainder rows (tests/util.py: REG_SMALL_REMAINDER) are named, at most 1 % of
    the rows, and held to 1e-4 of the tensor's maximum instead -- every other row to the quarter."""
    m, q, s, nn, rows = U.reg_scene(name)
    for top_k in U.reg_top_ks(nn.shape[1]):
        ref = U.reg_reference(name, top_k=top_k)
        min_dot, gap, zero_dots = U.reg_conditions(m, q, s, nn, top_k)
        assert min_dot >= U.REG_MIN_MARGIN and gap >= U.REG_MIN_MARGIN, (name, top_k, min_dot, gap)
        assert zero_dots == (U.EDGE_PER_CLASS if name == "edges" else 0)
        loss_err, (_, _, zm, rm), (_, _, zq, rq) = _fp32_rows(m, q, s, nn, top_k, ref)
        small = [np.zeros(m.shape[0], bool)] * 2
        if name == "edges":
            small = [(sv < U.REG_SMALL_REMAINDER) & (sv > 0) for sv in U.reg_survival(m, q, s, nn, top_k, ref[1:])]
            for sm, g32, g64, what in zip(small, U.ref_direction_loss(m, q, s, nn, top_k, dtype=torch.float32)[1:], ref[1:],
                                          ("dmeans", "dquats")):
                assert sm.mean() <= U.REG_REMAINDER_CAP, (what, int(sm.sum()))
                err = (g32.double() - g64).abs().max(dim=1).values.numpy()
                assert (err[sm] <= 1e-4 * float(g64.abs().max())).all(), what
        worst_m, worst_q = float(rm[~small[0]].max(initial=0.0)), float(rq[~small[1]].max(initial=0.0))
        record_cpu("regulariser_fp32_reference", scene=name, top_k=top_k, loss_rel_err=loss_err, dmeans_ratio_to_bound=worst_m,
                   dquats_ratio_to_bound=worst_q, small_remainder_rows=[int(x.sum()) for x in small], min_abs_dot=min_dot,
                   selection_gap=gap if np.isfinite(gap) else None)
        assert loss_err <= 0.5 * U.REG_LOSS_TOL, (name, top_k, loss_err)   # (1e-6 is 16 ulp of an fp32 loss: no quarter to give)
        assert zm == 0 and zq == 0
        assert worst_m <= U.REG_FP32_SHARE and worst_q <= U.REG_FP32_SHARE, (name, top_k, worst_m, worst_q)
    l64, g64 = U.ref_ratio_loss(s)
    l32, g32 = U.ref_ratio_loss(s, torch.float32)
    worst, _, nonzero, _ = U.row_rel_ratio(g32, g64)
    assert abs(float(l32) - float(l64)) <= 0.5 * U.REG_LOSS_TOL * float(l64) and nonzero == 0 and worst <= U.REG_FP32_SHARE


@pytest.mark.parametrize("n", U.REG_SIZES)
def test_fp32_reference_within_a_quarter_at_every_size(n):
    m, q, s, _, _ = U.reg_scene(f"size{n}")
    for K in U.REG_SIZE_KS:
        nn = U.cpu_knn(m, K)
        for top_k in sorted({0, K // 2}):
            ref = U.reg_reference(f"size{n}", nn, top_k)
            min_dot, gap, zero_dots = U.reg_conditions(m, q, s, nn, top_k)
            assert min_dot >= U.REG_MIN_MARGIN and gap >= U.REG_MIN_MARGIN and zero_dots == 0, (n, K, top_k, min_dot, gap)
            loss_err, (wm, _, zm, _), (wq, _, zq, _) = _fp32_rows(m, q, s, nn, top_k, ref)
            assert loss_err <= 0.5 * U.REG_LOSS_TOL and zm == 0 and zq == 0, (n, K, top_k, loss_err)
            assert wm <= U.REG_FP32_SHARE and wq <= U.REG_FP32_SHARE, (n, K, top_k, wm, wq)
    if n == 1:   # nothing listed: loss exactly 1, gradients exactly zero
        loss, gm, gq = U.reg_reference("size1", U.cpu_knn(m, 5), 0)
        assert float(loss) == 1.0 and not gm.any() and not gq.any()


def test_top_k_at_and_above_k_is_the_full_method():
    for name in SCENES:
        K = U.reg_scene(name)[3].shape[1]
        full = U.reg_reference(name, top_k=0)
        for top_k in (K, K + 1):
            for a, b in zip(U.reg_reference(name, top_k=top_k), full):
                assert torch.equal(a, b)
        assert not torch.equal(U.reg_reference(name, top_k=K // 2)[1], full[1])


@pytest.mark.parametrize("kind,method", U.REG_STEP_CASES)
def test_first_adam_step_conditions(kind, method):
    """The trainer-level cases: an fp32 evaluation of the scaled gradient keeps the first-step moments within a quarter of
    the row bound and the parameter deltas within 1e-4 lr of float64 Adam on the float64 gradient; the elements left
    out of the delta comparison (0 < |g64| < 100 eps) are at most 0.1 %."""
    from edgegaussians_amd import LRSchedule
    sc = U.reg_step_scene()
    lrs = LRSchedule(scales_start=0, quats_start=0, opacities_start=0, **U.REG_STEP_LRS).at(0)
    nn = U.reg_step_table(method)[:, 1:]
    top_k = U.REG_STEP_NN if method == "enforce_half" else 0
    args = (kind, sc.means, sc.quats, sc.log_scales, nn, top_k, U.REG_STEP_AVG_LOSS_SUM, U.REG_STEP_FACTOR)
    loss, g64 = U.ref_regulariser_step(*args)
    _, g32 = U.ref_regulariser_step(*args, dtype=torch.float32)
    if kind == "direction":
        min_dot, gap, _ = U.reg_conditions(sc.means, sc.quats, sc.log_scales, nn, top_k)
        assert min_dot >= U.REG_MIN_MARGIN and gap >= U.REG_MIN_MARGIN, (min_dot, gap)
    params = {"means": sc.means, "quats": sc.quats, "scales": sc.log_scales}
    d64 = U.adam_first_step_deltas(params, g64, lrs)
    d32 = U.adam_first_step_deltas(params, {k: v.double() for k, v in g32.items()}, lrs, dtype=torch.float32)
    rec = {}
    for k in params:
        wm = U.row_rel_ratio(0.1 * g32[k].double(), 0.1 * g64[k])
        wv = U.row_rel_ratio(0.001 * g32[k].double() ** 2, 0.001 * g64[k] ** 2)
        ratio, skipped = U.adam_delta_ratio(d32[k], d64[k], g64[k], lrs[k])
        rec[k] = dict(m=wm[0], v=wv[0], delta=ratio, skipped=skipped)
        assert wm[0] <= U.REG_FP32_SHARE and wv[0] <= U.REG_FP32_SHARE and wm[2] == 0, (k, wm[:3], wv[:3])
        assert skipped <= U.ADAM_SKIP_CAP and ratio <= 1.0, (k, ratio, skipped)
        # 1e-4 lr is above half an ulp of every stored parameter: an fp32 parameter CAN meet the bound
        assert 1e-4 * lrs[k] >= float(params[k].abs().max()) * 2.0 ** -24, k
    record_cpu("regulariser_first_adam_step_conditions", kind=kind, method=method, loss=float(loss), fp32=rec)
