"""The references, the row check and the named scenes of tests/knn_util.py, on the CPU.

The chunked float64 search equals tests.util.cpu_knn; every named scene reaches the branch of csrc/knn.hip it is named for
(ring_trace, with the counts); lattice scenes have exact fp32 distances; an fp32 model of the search uses at most half of
KNN_D2_TOL on every general scene; and five mutants of a correct table -- the faults tests/test_gpu_knn.py is there to
catch -- each fail the row check on every scene they apply to."""
import numpy as np
import pytest
import torch

from tests import knn_util as KU
from tests.util import cpu_knn, record_cpu

GENERAL = tuple(n for n in KU.SCENE_NAMES if KU.scene(n).kind == "general")
LATTICE = tuple(n for n in KU.SCENE_NAMES if KU.scene(n).kind == "lattice")


def test_chunked_reference_equals_cpu_knn():
    for name, k in (("exhaustive_1", 3), ("exhaustive_7", 32), ("exhaustive_193", 6), ("host_5x4x3", 32),
                    ("fullscan_sparse", 1), ("kth_lattice", 6)):
        pts = KU.scene(name).pts[:1500]
        want = cpu_knn(pts, k)
        idx, d2 = KU.knn_ref(pts, k, chunk=97)
        assert torch.equal(idx, want)
        assert torch.equal(d2 == float("inf"), want < 0)
        rows = np.arange(pts.shape[0])[::3]
        sub, d2s = KU.knn_ref(pts, k, rows=rows)
        assert torch.equal(sub, want[::3]) and torch.equal(d2s, d2[::3])
        p = pts.double()
        live = idx >= 0
        g = p[idx.long().clamp(min=0)]
        assert torch.equal(((p[:, None, :] - g) ** 2).sum(-1)[live], d2[live])
        assert bool((d2[:, 1:] >= d2[:, :-1]).all())
    # the sliced, cached form the tests use
    for name in ("exhaustive_33", "host_7x3x1", "auto_clustered_k21"):
        sc = KU.scene(name)
        k = sc.ks[-1]
        idx, d2 = KU.reference(name, k)
        idx2, d22 = KU.knn_ref(sc.pts, k, rows=sc.rows)
        assert torch.equal(idx, idx2) and torch.equal(d2, d22)


def test_scene_sizes_follow_the_kernels_constants():
    assert KU.r_brute_of(374) == 1 and KU.r_brute_of(375) == 1 and KU.r_brute_of(376) == 2
    assert KU.r_brute_of(4335) == 4 and KU.r_brute_of(KU.FAR_N) == 8 and KU.FAR_N == 4336
    assert KU.auto_dims(20000, 6) == 18 and KU.auto_dims(20000, 21) == 14
    assert [d[0] * d[1] * d[2] for d in KU.SCAN_DIMS] == [4095, 4096, 8192, 32768]
    assert [-(-(d[0] * d[1] * d[2] + 1) // 4096) for d in KU.SCAN_DIMS] == [1, 2, 3, 9]   # scan workgroups
    assert KU.scene("auto_two_bbox_workgroups").N == 2049
    for name in KU.SCAN_SCENES + ("fullscan_sparse",):
        assert KU.scene(name).N == 200
    for n in (4095, 4096, 4097, 16383, 16384, 16385):
        rows = KU.scene(f"exhaustive_{n}").rows
        r = np.arange(n)
        must = np.concatenate([r[:64], r[-64:], r[r % 64 < 4]])
        assert np.isin(must, rows).all() and rows.shape[0] >= must.shape[0] + 400 and (np.diff(rows) > 0).all()
    for name in KU.SCENE_NAMES:
        sc = KU.scene(name)
        assert all(1 <= k <= KU.K_MAX for k in sc.ks) and torch.isfinite(sc.pts).all()
    assert {KU.scene(n).ks for n in KU.EXHAUSTIVE_SCENES} == {KU.K_LIST, (32,)}
    nz = KU.scene("auto_negative_zero").pts
    assert bool(torch.signbit(nz[:, 2].min())) and float(nz[:, 2].min()) == 0.0 and bool((nz[:, 2] >= 0).all())
    assert bool((KU.scene("auto_all_negative").pts < 0).all())
    te = KU.scene("auto_tiny_extent").pts
    assert float((te.max(0).values - te.min(0).values).max()) < 0.021 and float(te.min()) > 999.98


def test_general_scenes_keep_coordinate_differences_off_the_underflow():
    for name in GENERAL:
        gap = KU.min_coordinate_gap(KU.scene(name).pts.numpy())
        assert gap > 1e-12, (name, gap)
    base = KU.scene("clamped_base")
    from edgegaussians_amd.regularizers import make_grid
    moved, which = KU.clamped_points(base.pts, make_grid(base.pts, margin=0.0))
    assert KU.min_coordinate_gap(moved.numpy()) > 1e-12


def test_lattice_scenes_have_exact_fp32_distances():
    for name in LATTICE:
        sc = KU.scene(name)
        rows = torch.arange(0, sc.N, max(1, sc.N // 300))
        q = sc.pts[rows]
        d32 = KU.d2_f32_emulated(q, sc.pts)
        d64 = ((q.double()[:, None, :] - sc.pts.double()[None, :, :]) ** 2).sum(-1)
        assert torch.equal(d32, d64), name                                       # the model rounds nowhere ...
        e = sc.pts[None, :, :] - q[:, None, :]                                   # ... and neither does plain fp32
        plain = (e[..., 2] * e[..., 2] + (e[..., 1] * e[..., 1] + e[..., 0] * e[..., 0])).double()
        assert torch.equal(plain, d64), name
        # exact ties that only the index rule decides, in the checked tables themselves
        k = sc.ks[-1]
        _, d2 = KU.reference(name, k, extra=1)
        tied = float((d2[:, k - 1] == d2[:, k]).double().mean()) if sc.N > k + 1 else 0.0
        record_cpu("knn_lattice_ties", scene=name, k=k, rows_tied_at_the_kth_place=tied)
        if name == "kth_lattice" or name.startswith("host_"):
            assert tied > 0.2, (name, tied)


def test_host_grid_scenes_reach_every_first_block():
    """first blocks of 1, 3, 4, 6 and 9 rows all occur; queries sit in corner, edge, face and interior cells; every cell
    holds a point; the long cell is the last of the sorted records"""
    seen = {}
    for name in KU.HOST_SCENES:
        sc = KU.scene(name)
        cells = KU.cells_of(sc.pts.numpy(), sc.grid)
        dims = sc.grid[2]
        ids = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
        counts = np.bincount(ids, minlength=dims[0] * dims[1] * dims[2])
        assert (counts >= 1).all(), name
        assert counts[-1] >= KU.LONG_CELL and counts[:-1].max(initial=0) <= 3, name
        tr = KU.trace(name, 6)
        rows, n = np.unique(tr.first_rows, return_counts=True)
        for r, c in zip(rows.tolist(), n.tolist()):
            seen[r] = seen.get(r, 0) + c
        record_cpu("knn_ring_trace", scene=name, k=6, first_block_rows=dict(zip(map(str, rows.tolist()), n.tolist())),
                   full_scan_queries=tr.full_scans, blocks_per_query_max=max(len(r) for r in tr.radii))
    assert set(seen) >= {1, 3, 4, 6, 9} and all(seen[r] >= 10 for r in (1, 3, 4, 6, 9)), seen
    sc = KU.scene("host_5x4x3")
    kinds = np.bincount(KU.boundary_axes(sc.pts.numpy(), sc.grid), minlength=4)
    assert (kinds >= 2).all(), kinds            # interior, face, edge, corner
    record_cpu("knn_ring_trace_cells", scene="host_5x4x3", interior=int(kinds[0]), face=int(kinds[1]), edge=int(kinds[2]),
               corner=int(kinds[3]))


def test_edge_scenes_fill_workgroups_raggedly():
    assert [n % 16 for n in KU.EDGE_N] == [15, 0, 1, 15, 0, 1, 1] and [n % 4 for n in KU.EDGE_N] == [3, 0, 1, 3, 0, 1, 1]
    for name in KU.EDGE_SCENES:
        tr = KU.trace(name, 6)
        record_cpu("knn_ring_trace", scene=name, k=6, full_scan_queries=tr.full_scans,
                   blocks_per_query_max=max(len(r) for r in tr.radii))


def test_full_scan_scenes_reach_the_full_scan():
    sc = KU.scene("fullscan_sparse")
    assert min(sc.grid[2]) >= 8 and KU.r_brute_of(sc.N) == 1
    tr = KU.trace("fullscan_sparse", 6)
    record_cpu("knn_ring_trace", scene="fullscan_sparse", k=6, full_scan_queries=tr.full_scans, queries=sc.N)
    assert tr.full_scans >= sc.N / 10
    assert all(r == (1,) for r, f in zip(tr.radii, tr.full_scan) if f)     # radius 2..7 asked for: scan instead

    sc = KU.scene("fullscan_outlier")
    assert tuple(sc.grid[2]) == (12, 12, 12) and KU.r_brute_of(sc.N) == 8
    assert tuple(KU.cells_of(sc.pts.numpy(), sc.grid)[0]) == (0, 0, 0)
    tr = KU.ring_trace(sc.pts, sc.grid, KU.FAR_K, rows=[0])
    assert tr.radii[0] == (1, 2, 4, 8) and bool(tr.full_scan[0]), tr.radii[0]
    d = (sc.pts[1:1 + KU.FAR_K + 2].double() - sc.pts[0].double()).norm(dim=1)
    assert 9.0 < float(d.min()) and float(d.max()) < 11.0                   # about ten cells, inside the block of radius 8
    assert bool((KU.cells_of(sc.pts.numpy(), sc.grid)[1:1 + KU.FAR_K + 2] == np.array([7, 7, 0])).all())
    full = KU.trace("fullscan_outlier", KU.FAR_K)
    record_cpu("knn_ring_trace", scene="fullscan_outlier", k=KU.FAR_K, outlier_radii=list(tr.radii[0]),
               full_scan_queries=full.full_scans, queries=sc.N)
    assert full.full_scans == 1

    sc = KU.scene("empty_growth")
    tr = KU.ring_trace(sc.pts, sc.grid, KU.FAR_K, rows=[0])
    assert tr.radii[0] == (1, 2, 4, 8, 12) and not tr.full_scan[0], tr.radii[0]
    record_cpu("knn_ring_trace", scene="empty_growth", k=KU.FAR_K, outlier_radii=list(tr.radii[0]), full_scan_queries=0)


def test_ring_border_scene_needs_the_second_block():
    """a search that settles at a K-th distance up to 10 % beyond the first block's reach returns a wrong row there"""
    sc = KU.scene("ring_border")
    assert KU.r_brute_of(sc.N) == 4
    tr = KU.trace("ring_border", 6)
    kth = KU.reference("ring_border", 6)[1][:, 5].numpy()
    second = np.array([len(r) >= 2 for r in tr.radii]) & ~tr.full_scan
    short = tr.first_tau.astype(np.float64) > kth * (1.0 + 1e-5)        # a nearer point lies outside the first block
    early = short & (tr.first_tau <= np.float32(1.21))                  # ... and the block's own K-th is within 1.1 cells
    record_cpu("knn_ring_trace", scene="ring_border", k=6, queries=sc.N, second_block=int(second.sum()),
               first_block_misses_a_neighbour=int(short.sum()), of_those_kth_within_1p1_reach=int(early.sum()),
               full_scan_queries=tr.full_scans)
    assert second.sum() >= sc.N / 5 and short.sum() >= 100 and early.sum() >= 20
    assert not (short & ~second & ~tr.full_scan).any()                   # (the restated search itself never stops short)


def test_scan_chain_scenes_are_nearly_empty_grids():
    for name in KU.SCAN_SCENES:
        sc = KU.scene(name)
        cells = KU.cells_of(sc.pts.numpy(), sc.grid)
        dims = sc.grid[2]
        ids = (cells[:, 2] * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
        C = dims[0] * dims[1] * dims[2]
        assert np.unique(ids).shape[0] <= 200 < C / 20
        assert ids.max() > C - C // 8 and ids.min() < C // 8       # records on either side of every scan workgroup's carry
        tr = KU.trace(name, 6)
        record_cpu("knn_ring_trace", scene=name, k=6, cells=C, full_scan_queries=tr.full_scans, queries=sc.N)


def test_clamped_scene_leaves_the_grid_on_every_side():
    from edgegaussians_amd.regularizers import make_grid
    base = KU.scene("clamped_base")
    grid = make_grid(base.pts, margin=0.0)
    moved, which = KU.clamped_points(base.pts, grid)
    assert which.sum() == base.N // 10 and torch.equal(moved[~torch.from_numpy(which)], base.pts[~torch.from_numpy(which)])
    lo = np.asarray(grid[0])
    hi = lo + np.asarray(grid[2]) * grid[1]
    out = (moved.double().numpy() - lo) / grid[1], (moved.double().numpy() - hi) / grid[1]
    below, above = -out[0], out[1]          # in cells, positive = outside
    for a in range(3):
        assert (below[:, a] > 0).sum() >= 10 and (above[:, a] > 0).sum() >= 10
    far = np.maximum(below, above).max(axis=1)[which]
    assert (far > 0).all() and ((far > 0.009) & (far < 0.016)).sum() >= 30 and ((far > 49) & (far < 76)).sum() >= 30
    assert (far > 999).sum() == 2
    tr = KU.ring_trace(moved, grid, 6)
    record_cpu("knn_ring_trace", scene="clamped", k=6, moved=int(which.sum()), full_scan_queries=tr.full_scans,
               blocks_per_query_max=max(len(r) for r in tr.radii), dims=list(grid[2]))


def test_device_grid_scenes_trace():
    """the device-chosen grid of the eg_knn_auto scenes, restated: where their queries end"""
    for name in KU.AUTO_SCENES:
        sc = KU.scene(name)
        k = sc.ks[0]
        origin, cell, inv, D = KU.auto_grid(sc.pts.numpy(), k)
        assert D == KU.auto_dims(sc.N, k) and cell > 0 and np.isfinite(origin).all()
        cells = KU.cells_of(sc.pts.numpy(), KU.auto_host_grid(sc.pts.numpy(), k))
        raw = np.floor((sc.pts.numpy() - origin[None, :]) * inv)
        assert (raw >= 0).all() and (raw <= D - 1).all(), name       # the inflated box holds every point unclamped
        tr = KU.trace(name, k, grid=KU.auto_host_grid(sc.pts.numpy(), k))
        record_cpu("knn_ring_trace", scene=name, k=k, D=D, occupied_cells=int(np.unique(cells, axis=0).shape[0]),
                   rows_traced=int(tr.rows.shape[0]), full_scan_queries=tr.full_scans,
                   blocks_per_query_max=max(len(r) for r in tr.radii))
    assert KU.auto_dims(2049, 6) == 9 and -(-2049 // 2048) == 2       # two bbox workgroups


def _fp32_table(name, k):
    sc = KU.scene(name)
    key = ("fp32", name)
    if key not in KU._cache:
        KU._cache[key] = KU.knn_ref(sc.pts, KU.K_MAX, rows=sc.rows, fp32=True)
    idx, d2 = KU._cache[key]
    return idx[:, :k], d2[:, :k]


@pytest.mark.parametrize("name", GENERAL)
def test_fp32_model_uses_at_most_half_the_tolerance(name):
    # (the model rounds a fused add twice, through float64: it is a witness that SOME fp32 search fits, not the oracle)
    sc = KU.scene(name)
    for k in sc.ks:
        idx, d2 = _fp32_table(name, k)
        res = KU.row_check(sc.pts, k, idx, d2.sqrt().float(), KU.reference(name, k), rows=sc.rows)
        differ = float((idx != KU.reference(name, k)[0]).double().mean()) if idx.numel() else 0.0
        record_cpu("knn_fp32_model", scene=name, k=k, rows_checked=res.rows_checked, worst_d2_ratio_to_bound=res.worst,
                   entries_ordered_differently=differ)
        assert res.ok, (name, k, res.failures)
        assert res.worst <= 0.5, (name, k, res.worst)


def _mutants(sc, k, idx, dist, d2x):
    """(name, mutated idx, mutated dist) for every mutant that applies; d2x: the reference distances at k + 1 columns"""
    N, R = sc.N, idx.shape[0]
    out = []
    d2 = d2x[:, :k]
    gap = 1.0 + 4.0 * KU.KNN_D2_TOL
    # a swap of two entries with distinct distances
    b = min(k, N - 1) - 1            # the last place that holds a neighbour
    if b >= 1:
        ok = d2[:, b] > d2[:, 0] * gap
        if ok.any():
            r = int(np.nonzero(ok)[0][0])
            i2, s2 = idx.copy(), dist.copy()
            i2[r, [0, b]], s2[r, [0, b]] = idx[r, [b, 0]], dist[r, [b, 0]]
            out.append(("swap", i2, s2))
    # one neighbour replaced by the (K+1)-th
    if N - 1 >= k + 1:
        ok = d2x[:, k] > d2x[:, k - 1] * gap
        if ok.any():
            r = int(np.nonzero(ok)[0][-1])
            i2, s2 = idx.copy(), dist.copy()
            i2[r, k - 1], s2[r, k - 1] = sc.extra_idx[r], np.sqrt(d2x[r, k])
            out.append(("k_plus_first", i2, s2))
    # one entry duplicated
    if min(k, N - 1) >= 2:
        r = R // 2
        i2, s2 = idx.copy(), dist.copy()
        i2[r, 1], s2[r, 1] = idx[r, 0], dist[r, 0]
        out.append(("duplicate", i2, s2))
    # self inserted
    if N >= 2:
        r = R - 1
        rows = np.arange(N) if sc.rows is None else sc.rows
        i2, s2 = idx.copy(), dist.copy()
        i2[r, 0], s2[r, 0] = rows[r], 0.0
        out.append(("self", i2, s2))
    # a tail -1 filled
    if N - 1 < k and N >= 2:
        i2, s2 = idx.copy(), dist.copy()
        i2[0, N - 1], s2[0, N - 1] = idx[0, 0], dist[0, N - 2]
        out.append(("tail_filled", i2, s2))
    return out


def test_mutants_of_a_correct_table_fail_the_row_check():
    applied = {}
    for name in KU.SCENE_NAMES:
        sc = KU.scene(name)
        for k in sc.ks:
            ridx, rd2 = KU.reference(name, k)
            xidx, xd2 = KU.reference(name, k, extra=1)
            idx, d2 = ridx.numpy().astype(np.int64), rd2.numpy()
            dist = np.sqrt(np.where(np.isfinite(d2), d2, 9.0e76)).astype(np.float32).astype(np.float64)
            good = KU.row_check(sc.pts, k, idx, dist, (ridx, rd2), rows=sc.rows)
            assert good.ok and good.worst <= 0.13, (name, k, good.failures, good.worst)   # fp32 rounding of the root
            sc.extra_idx = xidx.numpy()[:, k]
            for mname, i2, s2 in _mutants(sc, k, idx, dist, xd2.numpy()):
                res = KU.row_check(sc.pts, k, i2, s2, (ridx, rd2), rows=sc.rows)
                assert not res.ok, f"mutant {mname} passes the row check on {name}, k = {k}"
                applied[mname] = applied.get(mname, 0) + 1
    record_cpu("knn_mutants", cases_each_failed_on=applied)
    assert set(applied) == {"swap", "k_plus_first", "duplicate", "self", "tail_filled"} and min(applied.values()) >= 3, applied
