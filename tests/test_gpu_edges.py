"""Parametric-edge sampling and scoring on the GPU (csrc/edges.hip, edgegaussians_amd.edges, the eval command line)
against the reference's own float64 outputs recorded in tests/golden/edge_sampling.npz
(tests/golden/make_golden_edges.py).

Tolerances, derived: counts are integers and the fixture keeps every length 1e-6 resolutions away from a count boundary,
so they must be EQUAL.  Lengths differ from the reference's only in the order of a 10 100-term float64 sum: 1e-12
relative.  Points and directions are evaluated in float64 (error ~1e-15) and rounded once to float32, so they equal
float32(reference) except where that error crosses a rounding boundary: one float32 ulp of the reference value.
"""
import contextlib
import io as _stdio
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import edges
    return edges


@pytest.fixture(scope="module")
def gold(golden_dir):
    g = np.load(os.path.join(golden_dir, "edge_sampling.npz"))
    return {k: g[k] for k in g.files}


def _case(gold, name):
    """(curves, lines, resolution, reference lengths, counts, points, directions)"""
    if name == "short":
        return (np.zeros((0, 4, 3)), gold["short_lines"], 0.005, gold["short_lengths"], gold["short_counts"],
                gold["short_points"], gold["short_dirs"])
    r = {"mixed_0.005": 0.005, "mixed_0.02": 0.02}[name]
    return (gold["mixed_curves"], gold["mixed_lines"], r, gold["mixed_lengths"], gold[f"mixed_{r}_counts"],
            np.concatenate([gold[f"mixed_{r}_curve_points"], gold[f"mixed_{r}_line_points"]]),
            np.concatenate([gold[f"mixed_{r}_curve_dirs"], gold[f"mixed_{r}_line_dirs"]]))


def _within_one_ulp(got32, ref64, what):
    ref32 = ref64.astype(np.float32)
    assert got32.dtype == np.float32 and got32.shape == ref32.shape, (what, got32.shape, ref32.shape)
    assert np.isfinite(got32).all(), what
    err = np.abs(got32.astype(np.float64) - ref32.astype(np.float64))
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    print(f"{what}: {int((err > 0).sum())} of {err.size} values differ from float32(reference), worst {float((err / ulp).max()):.2f} ulp")
    assert (err <= ulp).all(), (what, float((err / ulp).max()))


def _mixed(gold):
    return {"curves_ctl_pts": gold["mixed_curves"].reshape(-1, 12).tolist(), "lines_end_pts": gold["mixed_lines"].reshape(-1, 6).tolist()}


@pytest.mark.parametrize("name", ["mixed_0.005", "mixed_0.02", "short"])
def test_fixture_case(env, gold, name):
    curves, lines, r, ref_len, ref_counts, ref_pts, ref_dirs = _case(gold, name)
    t = env.sample_tables((curves, lines), r, return_directions=True, return_ids=True)
    counts, offsets = t["counts"].cpu().numpy(), t["offsets"].cpu().numpy().astype(np.int64)
    lengths = t["lengths"].cpu().numpy()
    assert t["counts"].dtype == torch.int32 and t["lengths"].dtype == torch.float64 and t["points"].is_cuda
    assert np.array_equal(counts, ref_counts), (counts, ref_counts)
    rel = np.abs(lengths - ref_len) / np.maximum(ref_len, 1e-300)
    print(f"{name}: worst relative length error {rel.max():.3e}")
    assert (np.abs(lengths - ref_len) <= 1e-12 * ref_len).all(), rel.max()
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(ref_counts)]))
    Nc = len(curves)
    assert t["n_curve_points"] == ref_counts[:Nc].sum()
    # order: curves, then lines -- the reference arrays are concatenated in that order
    _within_one_ulp(t["points"].cpu().numpy(), ref_pts, f"{name} points")
    _within_one_ulp(t["directions"].cpu().numpy(), ref_dirs, f"{name} directions")
    ids = t["prim_ids"].cpu().numpy()
    assert t["prim_ids"].dtype == torch.int32
    assert np.array_equal(ids, np.repeat(np.arange(len(ref_counts)), ref_counts))
    assert ((offsets[ids] <= np.arange(len(ids))) & (np.arange(len(ids)) < offsets[ids + 1])).all()


def test_exact_tangent(env, gold):
    """tangent="exact" against the true derivative 3 [(1-t)^2 (P1-P0) + 2 (1-t) t (P2-P1) + t^2 (P3-P2)] in float64."""
    curves, lines, counts = gold["mixed_curves"], gold["mixed_lines"], gold["mixed_0.005_counts"]
    pts_r, n_curve, dirs_r = env.sample((curves, lines), 0.005, tangent="reference", return_directions=True)
    pts_e, n_curve_e, dirs_e = env.sample((curves, lines), 0.005, tangent="exact", return_directions=True)
    assert n_curve == n_curve_e and torch.equal(pts_r, pts_e)
    ref = []
    for P, n in zip(curves, counts[:7]):
        t = np.linspace(0, 1, n)[:, None]
        d = 3 * ((1 - t) ** 2 * (P[1] - P[0]) + 2 * (1 - t) * t * (P[2] - P[1]) + t ** 2 * (P[3] - P[2]))
        ref.append(d / np.linalg.norm(d, axis=1, keepdims=True))
    ref = np.concatenate(ref)
    assert np.isfinite(ref).all()
    _within_one_ulp(dirs_e[:n_curve].cpu().numpy(), ref, "exact tangent")
    assert torch.equal(dirs_e[n_curve:], dirs_r[n_curve:])  # lines: the same in both modes
    assert not torch.equal(dirs_e[:n_curve], dirs_r[:n_curve])  # the reference's formula is not the tangent


def test_edge_shapes(env, gold):
    curves, lines = gold["mixed_curves"], gold["mixed_lines"]
    pts, n_curve, dirs, ids = env.sample({"curves_ctl_pts": [], "lines_end_pts": []}, return_directions=True, return_ids=True)
    assert pts.shape == (0, 3) and pts.dtype == torch.float32 and pts.is_cuda and n_curve == 0
    assert dirs.shape == (0, 3) and ids.shape == (0,)
    c = gold["mixed_0.005_counts"]
    pts, n_curve = env.sample((curves, np.zeros((0, 2, 3))))  # curves only
    assert n_curve == pts.shape[0] == c[:7].sum()
    _within_one_ulp(pts.cpu().numpy(), gold["mixed_0.005_curve_points"], "curves only")
    pts, n_curve = env.sample({"curves_ctl_pts": [], "lines_end_pts": lines.tolist()})  # lines only
    assert n_curve == 0 and pts.shape[0] == c[7:].sum()
    _within_one_ulp(pts.cpu().numpy(), gold["mixed_0.005_line_points"], "lines only")
    # a single one-sample line: t = 0, the first end point
    pts, n_curve, dirs, ids = env.sample((np.zeros((0, 4, 3)), lines[2:3]), return_directions=True, return_ids=True)
    assert pts.shape == (1, 3) and n_curve == 0 and ids.tolist() == [0]
    assert np.array_equal(pts.cpu().numpy()[0], lines[2, 0].astype(np.float32))
    # the degenerate curve alone: no samples, no nan anywhere
    t = env.sample_tables((curves[6:7], np.zeros((0, 2, 3))), return_directions=True)
    assert t["points"].shape == (0, 3) and t["directions"].shape == (0, 3) and t["n_curve_points"] == 0
    assert t["lengths"].tolist() == [0.0] and t["counts"].tolist() == [0] and t["offsets"].tolist() == [0, 0]


def test_capacity(env, gold):
    import ctypes
    from edgegaussians_amd import _lib
    curves, lines = gold["mixed_curves"], gold["mixed_lines"]
    S = int(gold["mixed_0.005_counts"].sum())
    full = env.sample_tables((curves, lines), 0.005, return_directions=True, return_ids=True)
    fits = env.sample_tables((curves, lines), 0.005, return_directions=True, return_ids=True, capacity=S + 5)
    for k in ("points", "directions", "prim_ids", "lengths", "counts", "offsets"):
        assert torch.equal(full[k], fits[k]), k
    assert fits["n_curve_points"] == full["n_curve_points"]
    exact = env.sample((curves, lines), 0.005, capacity=S)
    assert torch.equal(exact[0], full["points"])
    with pytest.raises(RuntimeError, match="capacity"):
        env.sample((curves, lines), 0.005, capacity=S - 1)
    # the entry itself: negative code, a message, and nothing written -- neither inside the buffer nor behind it
    cap, guard = S - 1, 64
    dev = "cuda"
    dc, dl = torch.from_numpy(curves).to(dev), torch.from_numpy(lines).to(dev)
    P = len(curves) + len(lines)
    lengths, counts = torch.empty(P, dtype=torch.float64, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    offsets, total = torch.empty(P + 1, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    points = torch.full((cap + guard, 3), -7.0, device=dev)
    dirs = torch.full((cap + guard, 3), -7.0, device=dev)
    ids = torch.full((cap + guard,), -7, dtype=torch.int32, device=dev)
    host = (ctypes.c_int32 * 2)()
    h = _lib.load()
    rc = h.eg_edge_sample(dc.data_ptr(), len(curves), dl.data_ptr(), len(lines), 0.005, cap, 0, lengths.data_ptr(),
                          counts.data_ptr(), offsets.data_ptr(), total.data_ptr(), points.data_ptr(), dirs.data_ptr(),
                          ids.data_ptr(), host, _lib.stream())
    torch.cuda.synchronize()
    assert rc == -4 and b"capacity" in h.eg_last_error_string()
    assert list(host) == [S, 1] and total.tolist() == [S, 1]
    assert (points == -7.0).all() and (dirs == -7.0).all() and (ids == -7).all()
    # the two-call form with too few rows: the emission stops at the capacity
    total.zero_()
    _lib.call("eg_edge_sample_count", dc.data_ptr(), len(curves), dl.data_ptr(), len(lines), 0.005, -1,
              lengths.data_ptr(), counts.data_ptr(), offsets.data_ptr(), total.data_ptr(), _lib.stream())
    _lib.call("eg_edge_sample_emit", dc.data_ptr(), len(curves), dl.data_ptr(), len(lines), counts.data_ptr(),
              offsets.data_ptr(), total.data_ptr(), cap, 0, points.data_ptr(), dirs.data_ptr(), ids.data_ptr(), _lib.stream())
    assert total.tolist() == [S, 0]
    assert torch.equal(points[:cap], full["points"][:cap]) and (points[cap:] == -7.0).all()
    assert (dirs[cap:] == -7.0).all() and (ids[cap:] == -7).all()


def test_two_runs_give_the_same_bits(env, gold):
    a = env.sample_tables(_mixed(gold), 0.005, return_directions=True)
    b = env.sample_tables(_mixed(gold), 0.005, return_directions=True)
    for k in ("lengths", "counts", "points", "directions"):
        assert torch.equal(a[k], b[k]), k


def test_mirrors_return_the_references_shapes(env, gold, tmp_path):
    c = gold["mixed_0.005_counts"]
    path = str(tmp_path / "parametric_edges.json")
    with open(path, "w") as f:
        json.dump(_mixed(gold), f)
    for out in (env.get_pred_points_and_directions_from_dict(_mixed(gold), 0.005), env.get_pred_points_and_directions(path)):
        cp, lp, cd, ld = out
        assert isinstance(cp, np.ndarray) and cp.shape == (c[:7].sum(), 3) and cp.dtype == np.float64
        assert isinstance(lp, np.ndarray) and lp.shape == (c[7:].sum(), 3) and lp.dtype == np.float64
        assert isinstance(cd, list) and len(cd) == len(cp) and cd[0].shape == (3,)
        assert isinstance(ld, list) and len(ld) == len(lp) and ld[0].shape == (3,)
        _within_one_ulp(cp.astype(np.float32), gold["mixed_0.005_curve_points"], "mirror curve points")
        _within_one_ulp(np.array(ld, dtype=np.float32), gold["mixed_0.005_line_dirs"], "mirror line directions")
    cp, lp, cd, ld = env.get_pred_points_and_directions_from_dict({"curves_ctl_pts": [], "lines_end_pts": []})
    assert cp.shape == (0, 3) and lp.shape == (0, 3) and cd == [] and ld == []


def _metrics_equal(got, ref, n_pred):
    assert sorted(got) == sorted(list(ref) + ["n_pred"])
    assert got["n_pred"] == n_pred
    for k, v in ref.items():
        print(f"{k}: {got[k]!r} (reference samples: {v!r})")
    for k, v in ref.items():
        if k in ("acc", "comp", "chamfer"):
            assert abs(got[k] - v) <= 1e-6, (k, got[k], v)
        else:
            assert got[k] == v, (k, got[k], v)


def test_evaluate_edges_against_the_references_samples(env, gold):
    from edgegaussians_amd import metrics
    gt = torch.from_numpy(gold["gt"]).cuda()
    ref_pts = np.concatenate([gold["mixed_0.005_curve_points"], gold["mixed_0.005_line_points"]]).astype(np.float32)
    ref = metrics.evaluate(torch.from_numpy(ref_pts).cuda(), gt)
    got = env.evaluate_edges(_mixed(gold), gt)
    _metrics_equal(got, ref, len(ref_pts))
    with pytest.raises(ValueError, match="No points found"):
        env.evaluate_edges({"curves_ctl_pts": [], "lines_end_pts": gold["mixed_lines"][1:2].tolist()}, gt)


def test_eval_command_line(env, gold, tmp_path):
    from edgegaussians_amd import eval as eg_eval
    from edgegaussians_amd import io
    pred, gt_path, out_ply = str(tmp_path / "parametric_edges.json"), str(tmp_path / "gt.ply"), str(tmp_path / "s.ply")
    with open(pred, "w") as f:
        json.dump(_mixed(gold), f)
    io.write_points_ply(gold["gt"], gt_path)
    want = env.evaluate_edges(_mixed(gold), torch.from_numpy(gold["gt"]).cuda())
    buf = _stdio.StringIO()
    with contextlib.redirect_stdout(buf):
        ret = eg_eval.main(["--pred", pred, "--gt", gt_path, "--json", "--save_sampled_points", out_ply])
    printed = json.loads(buf.getvalue().strip().splitlines()[-1])
    assert printed == want and ret == want
    sampled = env.sample(_mixed(gold))[0].cpu().numpy()
    assert np.array_equal(io.read_points_ply(out_ply), sampled.astype(np.float64))
    # key: value lines without --json; a .ply of points as the prediction
    buf = _stdio.StringIO()
    with contextlib.redirect_stdout(buf):
        ret = eg_eval.main(["--pred", out_ply, "--gt", gt_path, "--thresholds", "0.005", "0.01", "0.02"])
    assert ret == want
    lines = dict(l.split(": ") for l in buf.getvalue().strip().splitlines())
    assert sorted(lines) == sorted(want) and float(lines["chamfer"]) == want["chamfer"] and int(lines["n_pred"]) == want["n_pred"]
