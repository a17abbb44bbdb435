"""Every neighbour search of csrc/knn.hip, row by row against the float64 brute-force search of tests/knn_util.py.

knn_wave_kernel<2|4|8> (eg_knn_small), knn_grid_wave_kernel<4> on a caller's grid (eg_knn) and on the grid the device
chooses (eg_knn_auto: knn_bbox_kernel), over knn_count / scan / scatter.  Lattice scenes (exact fp32 distances, ties
everywhere) must EQUAL tests.util.cpu_knn; general scenes pass knn_util.row_check on every checked row, no entry left
out, within KNN_D2_TOL = 2^-20 (derived there).  That each scene reaches the branch it is named for -- first blocks of
1, 3, 4, 6, 9 rows, the full-scan fallback, the radius that runs up to rmax, the scan chain over 1, 2, 3, 9 workgroups,
points clamped into boundary cells -- is asserted on the host (tests/test_knn_host.py, ring_trace).  After every grid
call the cached cell counts are all zero again; after every device-grid call the ticket words are zero and the grid
words equal knn_util.auto_grid.  Measured: profiles/knn_parity.txt."""
import pytest
import torch

from tests import knn_util as KU
from tests.util import cpu_knn, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import regularizers
    return regularizers


def scratch_after(R, pts, ncell, k=None, device_grid=False):
    """cell_counts back to zero; after a device-grid call the extrema and the ticket too, the grid words as auto_grid says"""
    b = R._knn_scratch[(pts.shape[0], ncell, str(pts.device))]
    assert int(torch.count_nonzero(b[1])) == 0, "cell_counts are not all zero after the call"
    if device_grid:
        words = b[4].cpu().numpy()
        assert not words[:8].any(), f"extrema / ticket words not handed back zeroed: {words[:8]}"
        bad = KU.auto_grid_words_match(words[8:16], pts.cpu().numpy(), k)
        assert not bad, bad


def search(R, sc, pts, k, entry, grid=None, **kw):
    """(idx, dist, after) of one entry; `after` asserts the scratch contracts the call must have kept (check runs it
    once the case's figures are recorded)"""
    if entry == "exhaustive":
        return R.knn(pts, k, want_dist=True, method="exhaustive", **kw) + (lambda: None,)
    if entry == "grid":
        D = KU.auto_dims(pts.shape[0], k)
        assert D == int(R.load().eg_knn_auto_dims(pts.shape[0], k))
        return R.knn(pts, k, want_dist=True, method="grid", **kw) + (lambda: scratch_after(R, pts, D ** 3, k, device_grid=True),)
    grid = grid if grid is not None else sc.grid
    return R.knn(pts, k, want_dist=True, grid=grid, **kw) + (lambda: scratch_after(R, pts, grid[2][0] * grid[2][1] * grid[2][2]),)


def lattice_table(name, k):
    """cpu_knn itself up to 2000 points, its chunked form (equal to it: tests/test_knn_host.py) above"""
    key = ("cpu_knn", name, k)
    if key not in KU._cache:
        sc = KU.scene(name)
        KU._cache[key] = cpu_knn(sc.pts, k) if sc.N <= 2000 else KU.reference(name, k)[0]
    return KU._cache[key]


def full_scans(sc, k, entry, pts=None, grid=None):
    if entry == "exhaustive":
        return None
    if entry == "grid":
        return KU.trace(sc.name, k, grid=KU.auto_host_grid(sc.pts.numpy(), k)).full_scans
    if grid is not None:
        return KU.ring_trace(pts, grid, k).full_scans
    return KU.trace(sc.name, k).full_scans


def check(sc, k, entry, idx, dist, pts=None, ref=None, grid=None, label=None, after=None):
    """record, then assert: equality with cpu_knn on a lattice scene, the row check on every checked row otherwise"""
    pts = sc.pts if pts is None else pts
    ref = KU.reference(sc.name, k) if ref is None else ref
    rows = sc.rows
    idx_c, dist_c = idx.cpu(), dist.cpu()
    sel = slice(None) if rows is None else torch.from_numpy(rows)
    res = KU.row_check(pts, k, idx_c[sel].numpy(), dist_c[sel].numpy(), ref, rows=rows)
    case = label or f"{sc.name}/{entry}/k{k}"
    record("knn_rows", case=case, worst_d2_ratio_to_bound=res.worst, rows_checked=res.rows_checked,
           full_scan_queries=full_scans(sc, k, entry, pts, grid))
    if after is not None:
        after()
    assert idx.shape == (pts.shape[0], k) and idx.dtype == torch.int32
    if sc.kind == "lattice":
        want = lattice_table(sc.name, k)
        wrong = int((idx_c != want).sum())
        assert torch.equal(idx_c, want), f"{case}: {wrong} entries differ from cpu_knn, first rows {(idx_c != want).any(1).nonzero()[:5].view(-1).tolist()}"
    assert res.ok, f"{case}: " + "; ".join(res.failures)


def run_scene(R, name):
    sc = KU.scene(name)
    pts = sc.pts.cuda()
    for k in sc.ks:
        for entry in sc.entries:
            idx, dist, after = search(R, sc, pts, k, entry)
            check(sc, k, entry, idx, dist, after=after)


@pytest.mark.parametrize("name", KU.EXHAUSTIVE_SCENES)
def test_exhaustive_search(R, name):
    """knn_wave_kernel<2> up to 4095 points, <4> from 4096, <8> from 16384; K = 1, 2, 6, 31, 32"""
    run_scene(R, name)


@pytest.mark.parametrize("name", KU.HOST_SCENES)
def test_host_grids_of_every_first_block(R, name):
    run_scene(R, name)


@pytest.mark.parametrize("name", KU.EDGE_SCENES)
def test_grid_search_workgroup_edges(R, name):
    run_scene(R, name)


@pytest.mark.parametrize("name", ("ring_border", "fullscan_sparse", "fullscan_outlier", "empty_growth"))
def test_full_scan_fallback_and_empty_growth(R, name):
    """the second block (ring_border: hundreds of rows whose first block misses a neighbour), the full scan behind
    r > r_brute && r < rmax, and the radius that runs up to rmax on an infinite K-th distance"""
    run_scene(R, name)


@pytest.mark.parametrize("name", KU.SCAN_SCENES)
def test_scan_chain(R, name):
    run_scene(R, name)


@pytest.mark.parametrize("name", KU.AUTO_SCENES)
def test_device_grid(R, name):
    run_scene(R, name)


def test_points_clamped_into_a_reused_grid(R):
    """make_grid's claim: points that have left a reused grid are clamped into boundary cells and the search stays exact"""
    base = KU.scene("clamped_base")
    grid = R.make_grid(base.pts, margin=0.0)
    idx, dist, after = search(R, base, base.pts.cuda(), 6, "host", grid=grid)
    check(base, 6, "host", idx, dist, grid=grid, label="clamped_base/host/k6", after=after)
    moved, which = KU.clamped_points(base.pts, grid)
    ref = KU.knn_ref(moved, 6)
    idx, dist, after = search(R, base, moved.cuda(), 6, "host", grid=grid)
    check(base, 6, "host", idx, dist, pts=moved, ref=ref, grid=grid, label="clamped_moved/host/k6", after=after)


def knn_auto_raw(R, pts, k, kth=None, slack=1.2):
    """eg_knn_auto as regularizers.knn calls it, with the SQUARED distances as the kernel wrote them"""
    from edgegaussians_amd._lib import call, load, ptr, stream
    N = pts.shape[0]
    D = int(load().eg_knn_auto_dims(N, k))
    cell_of, counts, start, order, gs = R._grid_buffers(N, D * D * D, pts.device)
    idx = torch.empty(N, k, dtype=torch.int32, device=pts.device)
    d2 = torch.empty(N, k, device=pts.device)
    call("eg_knn_auto", ptr(pts), N, k, ptr(cell_of), ptr(counts), ptr(start), ptr(order), ptr(gs), ptr(idx), ptr(d2),
         ptr(kth) if kth is not None else None, float(slack), stream())
    return idx, d2, lambda: scratch_after(R, pts, D ** 3, k, device_grid=True)


def test_entry_bound_of_the_previous_search(R):
    """kth: written as the K-th squared distance bit for bit; read as an INCLUSIVE bound (slack 1.0 on an identical lattice
    cloud with ties at the K-th place keeps the lowest index); too small, NaN, inf, negative or denormal-small bounds
    change nothing"""
    sc = KU.scene("kth_lattice")
    k = KU.KTH_K
    pts = sc.pts.cuda()
    want = lattice_table(sc.name, k)
    kth = torch.zeros(sc.N, device="cuda")
    idx, d2, after = knn_auto_raw(R, pts, k, kth)
    check(sc, k, "grid", idx, d2.sqrt(), label="kth_lattice/from_zeros", after=after)
    assert torch.equal(kth.view(torch.int32), d2[:, k - 1].contiguous().view(torch.int32))
    kth0 = kth.clone()
    _, d2ref = KU.reference(sc.name, k, extra=1)
    assert float((d2ref[:, k - 1] == d2ref[:, k]).double().mean()) > 0.2     # ties AT the bound, decided by the index
    junk = torch.tensor([float("nan"), float("inf"), -1.0, 1e-30, -float("inf"), 0.0], device="cuda").repeat(sc.N // 6)
    for label, bound, slack in (("slack_1.0", kth0.clone(), 1.0), ("slack_0.5", kth0.clone(), 0.5), ("junk", junk, 1.2),
                                ("slack_1.2", kth0.clone(), 1.2)):
        got, dist, after = search(R, sc, pts, k, "grid", kth=bound, kth_slack=slack)
        check(sc, k, "grid", got, dist, label=f"kth_lattice/{label}", after=after)
        assert torch.equal(got.cpu(), want) and torch.equal(got, idx)
        assert torch.equal(bound.view(torch.int32), kth0.view(torch.int32)), f"{label}: the output kth differs"
    # fewer than K other points: 0 = unknown
    few = KU.scene("exhaustive_7")
    kth = torch.full((7,), 5.0, device="cuda")
    got, dist, after = search(R, few, few.pts.cuda(), 32, "grid", kth=kth)
    check(few, 32, "grid", got, dist, label="exhaustive_7/grid_with_kth/k32", after=after)
    assert bool((kth == 0).all())


def test_out_buffer_is_filled_and_returned(R):
    sc = KU.scene("host_5x4x3")
    pts = sc.pts.cuda()
    want = lattice_table(sc.name, 6)
    for kw in (dict(method="exhaustive"), dict(method="grid"), dict(grid=sc.grid)):
        buf = torch.full((sc.N, 6), -7, dtype=torch.int32, device="cuda")
        got, dist = R.knn(pts, 6, out=buf, **kw)
        assert got is buf and dist is None and torch.equal(buf.cpu(), want), kw


def test_reference_nn_indices_columns(R):
    """update_nearest_neighbors' table: columns 2 .. k+1 of the float64 search (enforce_full), 2 .. 2k+1 (enforce_half)"""
    sc = KU.scene("host_5x4x3")
    pts = sc.pts.cuda()
    for nn, how, cols in ((5, "enforce_full", 6), (5, "enforce_half", 11), (1, "enforce_full", 2)):
        want = lattice_table(sc.name, cols)[:, 1:]
        for kw in (dict(), dict(method="grid"), dict(method="exhaustive"), dict(grid=sc.grid)):
            got = R.reference_nn_indices(pts, nn, how, **kw)
            assert got.shape == (sc.N, cols - 1) and got.is_contiguous() and torch.equal(got.cpu(), want), (nn, how, kw)


def test_two_runs_are_bit_equal(R):
    for name, k in (("auto_two_bbox_workgroups", 6), ("exhaustive_4097", 31), ("fullscan_outlier", 6), ("host_5x4x3", 32)):
        sc = KU.scene(name)
        pts = sc.pts.cuda()
        grid = sc.grid if sc.grid is not None else R.make_grid(sc.pts, margin=0.05)
        for kw in (dict(method="exhaustive"), dict(method="grid"), dict(grid=grid)):
            a, da = R.knn(pts, k, want_dist=True, **kw)
            b, db = R.knn(pts, k, want_dist=True, **kw)
            assert torch.equal(a, b) and torch.equal(da.view(torch.int32), db.view(torch.int32)), (name, kw)


def test_grid_too_fine_is_an_error_and_leaves_the_library_usable(R):
    one = torch.tensor([[0.5, 0.5, 0.5]], device="cuda")
    with pytest.raises(RuntimeError, match="grid too fine for the number of points"):
        R.knn(one, 1, grid=([0.0, 0.0, 0.0], 1.0 / 256.0, [256, 256, 256]))
    scratch_after(R, one, 256 ** 3)
    run_scene(R, "edge_65")
