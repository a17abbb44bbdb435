"""The cross-set nearest-neighbour search (eg_nn_query_small / eg_nn_query_auto), the metrics built on it and the
statistical outlier filter, on the GPU.

The reference for every distance and index is scipy's cKDTree in FLOAT64 on the same fp32 coordinates, computed here
and never taken from the code under test.

Distance tolerance, derived: the inputs are exact fp32; three subtractions, three products / fmas and one square root
round once each, so the relative error of d is below 4 * 2^-24 = 2.4e-7; rtol 1e-6 leaves 4x over that bound (atol
1e-12 for exact zeros).  Counts (precision / recall, the filter's verdicts) must be EQUAL once the queries within
1e-5 * t of a threshold t -- 10x the distance tolerance, so no correct implementation can flip any other -- are set
aside; the tests assert that those are at most 0.1 % of the distances.
"""
import inspect
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-12
METHODS = ("auto", "exhaustive", "grid")


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import filtering, metrics
    return metrics, filtering


def _reference(queries, targets):
    """(distance, index) of the nearest target, float64, from the fp32 coordinates."""
    q64, t64 = queries.numpy().astype(np.float64), targets.numpy().astype(np.float64)
    if len(q64) == 0:
        return np.zeros(0), np.zeros(0, np.int64)
    d, i = cKDTree(t64).query(q64, k=1)
    return d, i


def _check_nearest(metrics, queries, targets, label, methods=METHODS):
    """Distances at rtol 1e-6 and EVERY index: the float64 distance to the returned target is within (1 + 1e-6) of the
    float64 minimum.  Returns the results per method."""
    d_ref, i_ref = _reference(queries, targets)
    t64, q64 = targets.numpy().astype(np.float64), queries.numpy().astype(np.float64)
    out = {}
    for method in methods:
        dist, idx = metrics.nearest(queries.cuda(), targets.cuda(), method=method)
        assert dist.shape == (len(queries),) and dist.dtype == torch.float32 and dist.is_cuda
        assert idx.shape == (len(queries),) and idx.dtype == torch.int32 and idx.is_cuda
        d, i = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
        assert ((i >= 0) & (i < len(targets))).all(), (label, method)
        err = np.abs(d - d_ref) - (ATOL + RTOL * np.abs(d_ref))
        assert (err <= 0).all(), (label, method, float(err.max()), int((err > 0).sum()))
        d_mine = np.linalg.norm(q64 - t64[i], axis=1)  # float64 distance to the target the kernel returned
        bad = d_mine > d_ref * (1 + RTOL) + ATOL
        assert not bad.any(), (label, method, int(bad.sum()))
        share = float((i == i_ref).mean()) if len(i) else 1.0
        print(f"{label:40s} {method:10s} Q {len(queries):7d} M {len(targets):7d}  indices equal to cKDTree's: {share:.6f}")
        out[method] = (dist, idx)
    return out


def _clustered(n, g):
    """The clustered-segments-plus-floaters cloud of test_knn_matches_sklearn."""
    t = torch.rand(n, 1, generator=g)
    seg = torch.randint(0, 6, (n,), generator=g)
    a, b = torch.rand(6, 3, generator=g), torch.rand(6, 3, generator=g)
    pts = a[seg] * (1 - t) + b[seg] * t + 0.003 * torch.randn(n, 3, generator=g)
    pts[n // 2:] = torch.rand(n - n // 2, 3, generator=g) * 1.3 - 0.15
    return pts


def _gt_points(golden_dir):
    return torch.from_numpy(np.load(os.path.join(golden_dir, "abc_00004926_train.npz"))["gt_points"]).float().contiguous()


def _fixture_clouds(golden_dir):
    """gt (4000 points), pred = 3000 of them + 0.01 noise, and pred + 1000 floaters, from one CPU generator."""
    gt = _gt_points(golden_dir)
    assert gt.shape == (4000, 3)
    g = torch.Generator().manual_seed(0)
    perm = torch.randperm(4000, generator=g)[:3000]
    pred = (gt[perm] + 0.01 * torch.randn(3000, 3, generator=g)).contiguous()
    floaters = torch.rand(1000, 3, generator=g) * 1.3 - 0.15
    return gt, pred, torch.cat([pred, floaters]).contiguous()


def test_nearest_distances_and_indices_against_float64(env, golden_dir):
    metrics, _ = env
    g = torch.Generator().manual_seed(21)
    box = torch.tensor([1.0, 0.6, 0.3])
    # uniform clouds, either side of the auto crossover
    _check_nearest(metrics, torch.rand(5000, 3, generator=g) * box, torch.rand(6000, 3, generator=g) * box, "uniform")
    _check_nearest(metrics, torch.rand(50000, 3, generator=g) * box, torch.rand(60000, 3, generator=g) * box, "uniform")
    # clustered segments + floaters, as queries and as targets
    cl, cl2 = _clustered(6000, g), _clustered(9000, g)
    _check_nearest(metrics, cl2, cl, "clustered -> clustered")
    _check_nearest(metrics, torch.rand(7000, 3, generator=g), cl, "uniform -> clustered")
    _check_nearest(metrics, cl, torch.rand(7000, 3, generator=g), "clustered -> uniform")
    _check_nearest(metrics, _clustered(120000, g), _clustered(90000, g), "clustered -> clustered (large)")
    # the fixture's ground-truth edge points
    gt = _gt_points(golden_dir)
    noisy = gt[:3000] + 0.01 * torch.randn(3000, 3, generator=g)
    _check_nearest(metrics, noisy, gt, "noisy -> gt_points")
    _check_nearest(metrics, gt, noisy, "gt_points -> noisy")
    _check_nearest(metrics, torch.rand(20000, 3, generator=g), gt, "uniform -> gt_points")
    # Q >> M, Q << M, M = 1
    _check_nearest(metrics, torch.rand(100000, 3, generator=g), torch.rand(50, 3, generator=g), "Q >> M")
    _check_nearest(metrics, torch.rand(40, 3, generator=g), torch.rand(200000, 3, generator=g), "Q << M")
    _check_nearest(metrics, torch.rand(1000, 3, generator=g), torch.rand(1, 3, generator=g), "M = 1")
    _check_nearest(metrics, torch.rand(1, 3, generator=g), torch.rand(1, 3, generator=g), "Q = M = 1")
    # Q = 0
    for method in METHODS:
        dist, idx = metrics.nearest(torch.zeros(0, 3).cuda(), torch.rand(10, 3, generator=g).cuda(), method=method)
        assert dist.shape == (0,) and idx.shape == (0,) and dist.dtype == torch.float32 and idx.dtype == torch.int32
    with pytest.raises(ValueError):
        metrics.nearest(torch.rand(4, 3).cuda(), torch.zeros(0, 3).cuda())


@pytest.mark.parametrize("n", [4000, 60000])
def test_nearest_with_queries_outside_the_targets_box(env, n):
    """The walk starts in a boundary cell; the search must stop by the distance from the query's REAL position."""
    metrics, _ = env
    g = torch.Generator().manual_seed(22)
    box = torch.tensor([1.0, 0.6, 0.3])
    targets = torch.rand(n, 3, generator=g) * box
    queries = torch.rand(n, 3, generator=g) * box
    _check_nearest(metrics, queries + torch.tensor([3.0 * 1.0, 0.0, 0.0]), targets, "+3 extents on x")
    _check_nearest(metrics, queries + torch.tensor([0.0, 3.0 * 0.6, 0.0]), targets, "+3 extents on y")
    _check_nearest(metrics, queries - 0.5, targets, "-0.5 on all three")
    _check_nearest(metrics, queries * 1.2 - 0.1, targets, "a box 20 % larger")
    _check_nearest(metrics, _clustered(n, g) + torch.tensor([0.0, 0.0, 1.5]), _clustered(n, g), "clustered, +1.5 on z")


def test_nearest_with_degenerate_target_boxes(env):
    metrics, _ = env
    g = torch.Generator().manual_seed(23)
    for n in (3000, 30000):
        queries = torch.rand(n, 3, generator=g)
        line = torch.rand(n, 3, generator=g)
        line[:, 1:] = 0.25  # all on one line
        _check_nearest(metrics, queries, line, "targets on a line")
        _check_nearest(metrics, line, queries, "queries on a line")
        spot = torch.rand(1, 3, generator=g).repeat(n, 1).contiguous()  # all in one spot: every distance ties
        res = _check_nearest(metrics, queries, spot, "targets in one spot")
        for method in METHODS:
            assert int(res[method][1].abs().max()) == 0  # ... and the lowest index wins
        _check_nearest(metrics, spot, queries, "queries in one spot")


def test_tie_rule_and_agreement_of_the_two_entries(env):
    """10 % of the targets duplicated exactly: the exhaustive and the grid search return the same bits, and a query that
    coincides with a duplicated target gets the LOWEST of the duplicates -- at sizes either side of the auto crossover."""
    metrics, _ = env
    g = torch.Generator().manual_seed(24)
    sizes = ((500, 700), (3000, 4000), (9000, 7000), (8000, 8000), (20000, 30000), (100000, 100000))
    assert min(q * m for q, m in sizes) < metrics.NN_EXHAUSTIVE_MAX_PAIRS < max(q * m for q, m in sizes)
    for q, m in sizes:
        targets = torch.rand(m, 3, generator=g)
        tenth = m // 10
        targets[:tenth] = targets[tenth: 2 * tenth]  # target i + tenth is an exact duplicate of target i
        queries = torch.rand(q, 3, generator=g)
        ncoin = min(tenth, q // 2)
        queries[:ncoin] = targets[tenth: tenth + ncoin]  # coincide with the HIGHER-indexed duplicate
        qd, td = queries.cuda(), targets.cuda()
        d2e, ie = metrics.nearest(qd, td, method="exhaustive", squared=True)
        d2g, ig = metrics.nearest(qd, td, method="grid", squared=True)
        d2a, ia = metrics.nearest(qd, td, method="auto", squared=True)
        assert torch.equal(ie, ig) and torch.equal(d2e, d2g), (q, m, int((ie != ig).sum()), int((d2e != d2g).sum()))
        assert torch.equal(ie, ia) and torch.equal(d2e, d2a), (q, m)
        assert torch.equal(ie[:ncoin].cpu(), torch.arange(ncoin, dtype=torch.int32)), (q, m)
        assert float(d2e[:ncoin].abs().max()) == 0.0
        # no returned index is the higher of a duplicated pair
        assert not ((ie >= tenth) & (ie < 2 * tenth)).any(), (q, m)
        _check_nearest(metrics, queries, targets, f"duplicates {q} x {m}", methods=("grid",))


def test_self_consistency_with_shifted_and_identical_sets(env):
    metrics, _ = env
    g = torch.Generator().manual_seed(25)
    for n in (3000, 40000):
        pts = torch.rand(n, 3, generator=g)
        assert len(np.unique(pts.numpy(), axis=0)) == n  # duplicate-free
        shift = torch.tensor([0.013, -0.007, 0.021])
        _check_nearest(metrics, pts + shift, pts, "pts + c -> pts")
        for method in METHODS:
            dist, idx = metrics.nearest(pts.cuda(), pts.cuda(), method=method)
            assert torch.equal(idx.cpu(), torch.arange(n, dtype=torch.int32)), (n, method)
            assert float(dist.abs().max()) == 0.0


def test_evaluate_on_the_fixture(env, golden_dir):
    """acc / comp / chamfer at rtol 1e-6; every count -- and so precision, recall, F-score and IoU -- EQUAL to the
    float64 reference's once the borderline distances (|d64 - t| <= 1e-5 t) are set aside."""
    metrics, _ = env
    gt, pred, _ = _fixture_clouds(golden_dir)
    thresholds = (0.005, 0.01, 0.02)
    a_ref, _ = _reference(pred, gt)  # pred -> gt
    b_ref, _ = _reference(gt, pred)  # gt -> pred
    got = metrics.evaluate(pred.cuda(), gt.cuda())
    print({k: round(v, 6) for k, v in got.items()})
    assert got["acc"] == pytest.approx(a_ref.mean(), rel=RTOL)
    assert got["comp"] == pytest.approx(b_ref.mean(), rel=RTOL)
    assert got["chamfer"] == pytest.approx(a_ref.mean() + b_ref.mean(), rel=RTOL)
    a_dev, _ = metrics.nearest(pred.cuda(), gt.cuda())
    b_dev, _ = metrics.nearest(gt.cuda(), pred.cuda())
    assert got == metrics.summarize(a_dev, b_dev, thresholds)
    for t in thresholds:
        border_a, border_b = np.abs(a_ref - t) <= 1e-5 * t, np.abs(b_ref - t) <= 1e-5 * t
        nb = int(border_a.sum() + border_b.sum())
        print(f"t = {t}: {nb} borderline distances of {len(a_ref) + len(b_ref)}")
        assert nb <= 1e-3 * (len(a_ref) + len(b_ref))
        keep_a, keep_b = torch.from_numpy(~border_a), torch.from_numpy(~border_b)
        sub = metrics.summarize(a_dev.cpu()[keep_a], b_dev.cpu()[keep_b], (t,))
        ar, br = a_ref[~border_a], b_ref[~border_b]
        cp, cg = int((ar < t).sum()), int((br < t).sum())
        p, r = cp / len(ar), cg / len(br)
        assert sub[f"precision_{t}"] == p and sub[f"recall_{t}"] == r, (t, sub, p, r)
        assert sub[f"fscore_{t}"] == 2 * p * r / (p + r)
        assert sub[f"IOU_{t}"] == min(cp, cg) / (len(ar) + len(br) - max(cp, cg))
        # ... and what evaluate() itself counted differs from the reference by borderline distances only
        cp_all, cg_all = int((a_ref < t).sum()), int((b_ref < t).sum())
        assert abs(round(got[f"precision_{t}"] * len(a_ref)) - cp_all) <= int(border_a.sum())
        assert abs(round(got[f"recall_{t}"] * len(b_ref)) - cg_all) <= int(border_b.sum())
        if nb == 0:
            pa, ra = cp_all / len(a_ref), cg_all / len(b_ref)
            assert got[f"precision_{t}"] == pa and got[f"recall_{t}"] == ra
            assert got[f"fscore_{t}"] == 2 * pa * ra / (pa + ra)
            assert got[f"IOU_{t}"] == min(cp_all, cg_all) / (len(a_ref) + len(b_ref) - max(cp_all, cg_all))


def _stat_outliers_reference(pts, num_nn, std_multiplier):
    """Open3D 0.18 remove_statistical_outlier restated in float64: (inlier indices, avg, threshold)."""
    p64 = pts.numpy().astype(np.float64)
    k = min(num_nn, len(p64))
    d, _ = cKDTree(p64).query(p64, k=k)  # self included, at distance 0
    d = d.reshape(len(p64), k)
    avg = d.sum(axis=1) / k
    mean = avg.mean()
    std = np.sqrt(((avg - mean) ** 2).sum() / (len(avg) - 1))
    thr = mean + std_multiplier * std
    return np.nonzero((avg > 0) & (avg < thr))[0].astype(np.int64), avg, thr


def _check_filter(filtering, pts, num_nn, std_multiplier, label):
    ref, avg, thr = _stat_outliers_reference(pts, num_nn, std_multiplier)
    got = filtering.filter_stat_outliers(pts.cuda(), num_nn, std_multiplier)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.ndim == 1
    assert (np.diff(got) > 0).all()
    border = np.abs(avg - thr) <= 1e-5 * thr
    print(f"{label}: ({num_nn}, {std_multiplier}) keeps {len(got)} of {len(pts)} (reference {len(ref)}), "
          f"{int(border.sum())} borderline, closest {float(np.abs(avg - thr).min() / thr):.2e} thr away")
    assert border.sum() <= 1e-3 * len(pts)
    clear = np.nonzero(~border)[0]
    assert np.array_equal(np.intersect1d(got, clear), np.intersect1d(ref, clear)), label
    return got, ref


def test_filter_stat_outliers_against_float64_restatement(env, golden_dir):
    _, filtering = env
    _, _, cloud = _fixture_clouds(golden_dir)
    assert cloud.shape == (4000, 3)
    for num_nn, mult in ((25, 2.0), (10, 3.0)):
        got, ref = _check_filter(filtering, cloud, num_nn, mult, "pred + floaters")
        assert 0 < len(got) < len(cloud)  # it removes something, and not everything
    # an exact duplicate pair: avg > 0 still holds for both (their other neighbours are at a distance)
    g = torch.Generator().manual_seed(26)
    pts = torch.rand(500, 3, generator=g)
    pts[1] = pts[0]
    got, ref = _check_filter(filtering, pts, 10, 3.0, "duplicate pair")
    assert 0 in ref and 1 in ref and 0 in got and 1 in got
    # fewer points than num_nn: the mean is taken over what exists
    pts = torch.rand(5, 3, generator=g)
    got, ref = _check_filter(filtering, pts, 10, 3.0, "5 points")
    assert np.array_equal(got, ref)
    assert filtering.filter_stat_outliers(torch.zeros(0, 3).cuda(), 10, 3.0).shape == (0,)


def test_nearest_does_not_wait_for_the_device(env):
    """No host sync on the call path: with the stream kept busy by earlier work, `nearest` returns before the device
    gets to it (an event recorded after the call is still pending), and nothing on the path reads a tensor back."""
    metrics, _ = env
    for fn in (metrics.nearest, metrics._query_buffers, metrics._check_points):
        src = inspect.getsource(fn)
        for needle in (".tolist(", ".item(", ".cpu(", ".numpy(", "synchronize", ".any(", ".all(", "bool("):
            assert needle not in src, (fn.__name__, needle)
    g = torch.Generator().manual_seed(27)
    n = 200000
    queries, targets = torch.rand(n, 3, generator=g).cuda(), torch.rand(n, 3, generator=g).cuda()
    expect = metrics.nearest(queries, targets)  # (warm: code objects loaded, scratch cached)
    ballast = torch.ones(1 << 28, device="cuda")  # 1 GiB per pass
    torch.cuda.synchronize()
    for _ in range(200):
        ballast.mul_(1.0000001)
    dist, idx = metrics.nearest(queries, targets)
    ev = torch.cuda.Event()
    ev.record()
    pending = not ev.query()
    torch.cuda.synchronize()
    assert pending, "metrics.nearest waited for the device"
    assert torch.equal(idx, expect[1]) and torch.equal(dist, expect[0])
