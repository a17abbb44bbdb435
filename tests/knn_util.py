"""The float64 statement of the neighbour search (csrc/knn.hip), the per-row check and the named scenes shared by
tests/test_knn_host.py (which asserts the conditions on the scenes with the references alone) and tests/test_gpu_knn.py.
Torch and numpy only.

Two kinds of scene.
  lattice   coordinates are small integers times a power of two: every squared distance is exact in fp32, exact ties are
            everywhere, and the device table must EQUAL tests.util.cpu_knn (float64, stable (distance, index) order).
  general   random fp32 coordinates: two correct evaluations may order near-ties differently, so every row is held to
            row_check below, entry by entry, no entry left out.

KNN_D2_TOL = 2^-20 is derived, not measured: one dist2 (csrc/knn.hip) carries at most five roundings of 2^-24 -- the
three differences (each doubled by squaring), one multiply and two fused adds, all terms positive -- i.e. < 3.0e-7
relative; two swapped near-ties differ by at most twice that, 6e-7; 2^-20 ~ 9.5e-7 leaves the rest as margin.  General
scenes keep coordinate differences above 1e-12 or exactly zero (min_coordinate_gap), so that no term underflows."""
import math

import numpy as np
import torch

KNN_D2_TOL = 2.0 ** -20
K_MAX = 32          # the entries accept 1 <= K <= 32
K_LIST = (1, 2, 6, 31, 32)


# ---------------------------------------------------------------------------------------------------
# references
def d2_f32_emulated(q, p):
    """[R,N] dist2(p - q) with the kernel's rounding sequence (three fp32 differences, fp32 multiply, two fp32 fused
    adds), emulated through float64: each difference and the product are exact in float64 and rounded once; the sum
    inside a fused add is rounded to float64 BEFORE it is rounded to fp32 (double rounding), so this is a model of an fp32
    search, not the oracle."""
    e = (p.double()[None, :, :] - q.double()[:, None, :]).float().double()
    m = (e[..., 0] * e[..., 0]).float().double()
    m = (e[..., 1] * e[..., 1] + m).float().double()
    return (e[..., 2] * e[..., 2] + m).float().double()


def knn_ref(points, k, rows=None, chunk=128, fp32=False):
    """tests.util.cpu_knn in chunks of query rows, with the distances: (idx [R,k] int32, d2 [R,k] float64) of the query
    rows `rows` (default all) against ALL points, self excluded, ascending (distance, index) by a stable sort; -1 / inf
    where fewer than k other points exist.  fp32: distances from d2_f32_emulated instead of float64."""
    p = points.double()
    N = p.shape[0]
    rows = torch.arange(N) if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.long)
    R = rows.shape[0]
    idx = torch.full((R, k), -1, dtype=torch.int32)
    d2o = torch.full((R, k), float("inf"), dtype=torch.float64)
    have = min(k, N - 1)
    for a in range(0, R, chunk):
        r = rows[a:a + chunk]
        q = p[r]
        d2 = d2_f32_emulated(q, p) if fp32 else ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        d2[torch.arange(r.shape[0]), r] = float("inf")
        vals, order = torch.sort(d2, dim=1, stable=True)
        idx[a:a + chunk, :have] = order[:, :have].int()
        d2o[a:a + chunk, :have] = vals[:, :have]
    return idx, d2o


def min_coordinate_gap(points):
    """smallest nonzero |difference| between two points' coordinates on one axis (inf if there is none)"""
    p = np.asarray(points, dtype=np.float64)
    best = math.inf
    for a in range(3):
        d = np.diff(np.sort(p[:, a]))
        d = d[d > 0]
        if d.size:
            best = min(best, float(d.min()))
    return best


class RowResult:
    def __init__(self, failures, worst, rows_checked):
        self.failures, self.worst, self.rows_checked = failures, worst, rows_checked

    @property
    def ok(self):
        return not self.failures


def row_check(points, k, idx, dist, ref, rows=None):
    """The general-scene check of a [R,k] table (`idx` int, `dist` = the returned distances, NOT squared) for the query
    rows `rows` (default all: R = N) against `ref` = knn_ref(points, k, rows).  A row passes when
      * an index is -1 exactly where the reference's is (only where fewer than k other points exist:
        max(k - (N - 1), 0) of them, at the tail);
      * no index is the row itself, none is repeated, every other one is in [0, N);
      * the returned distances are non-decreasing;
      * at every place p the float64 squared distance from the query to idx[i, p] is within KNN_D2_TOL (relative) of
        the reference's p-th float64 squared distance (exactly 0 where that is 0);
      * the returned distance is within KNN_D2_TOL (relative) of the square root of the former.
    Returns RowResult(failures, worst ratio of an error to its bound, rows checked)."""
    p = np.asarray(points, dtype=np.float64)
    N = p.shape[0]
    rows = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    idx = np.asarray(idx).astype(np.int64)
    dist = np.asarray(dist).astype(np.float64)
    ref_idx, ref_d2 = np.asarray(ref[0]).astype(np.int64), np.asarray(ref[1]).astype(np.float64)
    assert idx.shape == (rows.shape[0], k) == dist.shape == ref_idx.shape == ref_d2.shape
    fails = []
    if rows.shape[0] == 0:
        return RowResult(fails, 0.0, 0)
    valid = idx >= 0
    want_neg = max(k - (N - 1), 0)
    if ((idx == -1).sum(1) != want_neg).any():
        fails.append(f"{int(((idx == -1).sum(1) != want_neg).sum())} rows do not hold exactly {want_neg} entries of -1")
    if (valid != (ref_idx >= 0)).any():
        fails.append("an entry of -1 is not at the tail")
    if ((idx < -1) | (idx >= N)).any():
        fails.append(f"{int(((idx < -1) | (idx >= N)).sum())} indices outside [0, N)")
        return RowResult(fails, math.inf, rows.shape[0])
    if (idx == rows[:, None]).any():
        fails.append(f"{int((idx == rows[:, None]).any(1).sum())} rows list themselves")
    s = np.sort(np.where(valid, idx, -1 - np.arange(k)[None, :]), axis=1)
    if (s[:, 1:] == s[:, :-1]).any():
        fails.append(f"{int((s[:, 1:] == s[:, :-1]).any(1).sum())} rows repeat an index")
    dd = np.where(valid, dist, np.inf)
    if (dd[:, 1:] < dd[:, :-1]).any() or np.isnan(dist[valid]).any():
        fails.append(f"{int((dd[:, 1:] < dd[:, :-1]).any(1).sum())} rows with decreasing distances")
    both = valid & (ref_idx >= 0)
    g = p[np.where(valid, idx, 0)]
    d2 = ((p[rows][:, None, :] - g) ** 2).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e1 = np.abs(d2 - ref_d2)
        r1 = np.where(ref_d2 > 0, e1 / (ref_d2 * KNN_D2_TOL), np.where(e1 == 0, 0.0, np.inf))
        sq = np.sqrt(d2)
        e2 = np.abs(dist - sq)
        r2 = np.where(sq > 0, e2 / (sq * KNN_D2_TOL), np.where(e2 == 0, 0.0, np.inf))
    r1, r2 = np.where(both, r1, 0.0), np.where(both, r2, 0.0)
    worst = float(max(r1.max(initial=0.0), r2.max(initial=0.0)))
    if not r1.max(initial=0.0) <= 1.0:
        i, c = np.unravel_index(np.argmax(r1), r1.shape)
        fails.append(f"{int((r1 > 1).sum())} entries ({int((r1 > 1).any(1).sum())} rows) are not the reference's neighbour "
                     f"of their place within KNN_D2_TOL; worst {r1[i, c]:.3g} x at row {int(rows[i])} place {int(c)}: "
                     f"index {int(idx[i, c])} at d2 {d2[i, c]:.9g}, reference {int(ref_idx[i, c])} at {ref_d2[i, c]:.9g}")
    if not r2.max(initial=0.0) <= 1.0:
        fails.append(f"{int((r2 > 1).sum())} returned distances off their index's distance, worst {r2.max():.3g} x")
    return RowResult(fails, worst, int(rows.shape[0]))


# ---------------------------------------------------------------------------------------------------
# the grids
def r_brute_of(N):
    """knn_grid_search: the block radius beyond which the full scan settles a query"""
    r = 1
    while (2 * (2 * r) + 1) * (2 * (2 * r) + 1) * 15 < N:
        r *= 2
    return r


def auto_dims(N, K):
    """eg_knn_auto_dims"""
    per_cell = 4 if K <= 12 else 8
    D = 1
    while D * D * D * per_cell < N and D < 256:
        D += 1
    return D


def auto_grid(points, K):
    """The grid eg_knn_auto chooses (knn_bbox_kernel), in fp32 numpy: D x D x D cubic cells over the largest extent
    inflated by 0.2 %, the origin 0.1 % of it below the minima.  Returns (origin [3] f32, cell f32, inv_cell f32, D)."""
    p = np.asarray(points, dtype=np.float32)
    D = auto_dims(p.shape[0], K)
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = np.float32(max(np.float32(1e-6), (hi - lo).max()))
    cell = np.float32(np.float32(ext * np.float32(1.002)) / np.float32(D))
    inv = np.float32(np.float32(1.0) / cell)
    origin = (lo - np.float32(np.float32(0.001) * ext)).astype(np.float32)
    return origin, cell, inv, D


def auto_grid_words_match(words, points, K):
    """The eight words the device leaves behind the ticket (Grid: ox oy oz inv_cell cell nx ny nz, int32 view) against
    auto_grid.  inv_cell and cell within one ulp; an origin within one ulp of the larger of the minimum and the shift
    it is the difference of (the compiler may fuse lo - 0.001 ext, which saves the product's rounding).  Returns a list
    of mismatches."""
    w = np.asarray(words, dtype=np.int32)
    f = w.view(np.float32)
    origin, cell, inv, D = auto_grid(points, K)
    lo = np.asarray(points, dtype=np.float32).min(axis=0)
    shift = np.float32(0.001) * np.float32(max(np.float32(1e-6), (np.asarray(points, np.float32).max(axis=0) - lo).max()))
    bad = []
    for a in range(3):
        ulp = float(np.spacing(np.float32(max(abs(lo[a]), abs(shift), abs(origin[a])))))
        if not abs(float(f[a]) - float(origin[a])) <= ulp:
            bad.append(f"origin[{a}] {f[a]!r} != {origin[a]!r}")
    for name, got, want in (("inv_cell", f[3], inv), ("cell", f[4], cell)):
        if not abs(float(got) - float(want)) <= float(np.spacing(want)):
            bad.append(f"{name} {got!r} != {want!r}")
    if tuple(int(x) for x in w[5:8]) != (D, D, D):
        bad.append(f"dims {w[5:8].tolist()} != {D}")
    return bad


def cells_of(points, grid):
    """cell_of_point for a host grid (origin, cell, dims) with fp32 cell arithmetic: int64 [N,3], clamped into the grid"""
    origin, cell, dims = grid
    p = np.asarray(points, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(cell)
    f = np.floor((p - np.asarray(origin, dtype=np.float32)[None, :]) * inv)
    return np.clip(f, 0, np.asarray(dims, dtype=np.float32)[None, :] - 1).astype(np.int64)


def boundary_axes(points, grid):
    """per point: on how many axes its cell is the first or the last of the grid (3 corner, 2 edge, 1 face, 0 interior)"""
    c = cells_of(points, grid)
    d = np.asarray(grid[2], dtype=np.int64)[None, :]
    return ((c == 0) | (c == d - 1)).sum(1)


class Trace:
    """ring_trace's answer: per traced query the block radii, the row count of the first block, the K-th squared
    distance inside the first block (3e38: fewer than K points there), full-scan flag"""
    def __init__(self, rows, radii, first_rows, full_scan, first_tau):
        self.rows, self.radii, self.first_rows, self.full_scan, self.first_tau = rows, radii, first_rows, full_scan, first_tau

    @property
    def full_scans(self):
        return int(self.full_scan.sum())


def ring_trace(points, grid, K, rows=None):
    """A plain restatement of the control flow of knn_grid_wave_kernel for the host grid (origin, cell, dims) of eg_knn
    (or the device's, from auto_grid), with fp32 cell arithmetic: which blocks a query scans and whether it ends in the
    full scan.  The K-th distance inside a block comes from brute force over the points of the block's cells
    (d2_f32_emulated).  Only ever used to assert that a scene REACHES the branch it was built for -- never as the
    expected result of a search."""
    origin, cell, dims = grid
    p = np.asarray(points, dtype=np.float32)
    N = p.shape[0]
    cells = cells_of(p, grid)
    cellf, inv = np.float32(cell), np.float32(1.0) / np.float32(cell)
    nx, ny, nz = (int(d) for d in dims)
    rmax, r_brute = max(nx, ny, nz), r_brute_of(N)
    rows = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    pt = torch.from_numpy(p)
    radii, first_rows, full = [], np.zeros(rows.shape[0], np.int64), np.zeros(rows.shape[0], bool)
    first_tau = np.zeros(rows.shape[0], np.float32)
    for n, i in enumerate(rows):
        c = cells[i]
        seq, settled, r = [], False, 1
        while not settled:
            if r > r_brute and r < rmax:
                break
            if not seq:
                rows_y = min(c[1] + r, ny - 1) - max(c[1] - r, 0) + 1
                rows_z = min(c[2] + r, nz - 1) - max(c[2] - r, 0) + 1
                first_rows[n] = rows_y * rows_z
            seq.append(r)
            inside = (np.abs(cells - c[None, :]) <= r).all(1)
            inside[i] = False
            cand = np.nonzero(inside)[0]
            tau = np.float32(3.0e38)
            if cand.size >= K:
                d2 = d2_f32_emulated(pt[i:i + 1], pt[cand])[0].numpy()
                tau = np.float32(np.partition(d2, K - 1)[K - 1])
            if len(seq) == 1:
                first_tau[n] = tau
            reach = np.float32(r) * cellf
            settled = bool(tau <= reach * reach) or r >= rmax
            if not settled:
                r_need = int(math.ceil(np.float32(np.sqrt(tau)) * inv)) if tau < np.float32(1.0e38) else 2 * r
                r = min(max(r_need, r + 1), max(rmax, r + 1))
        radii.append(tuple(seq))
        full[n] = not settled
    return Trace(rows, radii, first_rows, full, first_tau)


# ---------------------------------------------------------------------------------------------------
# the named scenes: built once per process, seeds fixed here
class Scene:
    """pts fp32 [N,3]; kind "lattice" | "general"; ks: the K of its searches; entries: which of "exhaustive" (eg_knn_small),
    "grid" (eg_knn_auto) and "host" (eg_knn on `grid` = (origin, cell, dims)) apply; rows: the checked query rows (None =
    all)."""
    def __init__(self, name, pts, kind, ks, entries, grid=None, rows=None, note=None):
        self.name, self.pts, self.kind, self.ks, self.entries = name, pts.contiguous(), kind, tuple(ks), tuple(entries)
        self.grid, self.rows, self.note = grid, rows, note or {}
        assert pts.dtype == torch.float32 and pts.shape[1] == 3
        self.N = pts.shape[0]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def general_cloud(n, seed):
    """random fp32 points in a 1 x 0.6 x 0.3 box, a tenth of them exact copies of other rows (from seven points on)"""
    pts = torch.rand(n, 3, generator=_gen(seed)) * torch.tensor([1.0, 0.6, 0.3])
    if n >= 7:
        m = max(n // 10, 1)
        pts[:m] = pts[m:2 * m]
    return pts


def switch_rows(n, seed):
    """the rows checked at the Q = 4 / Q = 8 switches: the first and last 64, index 0..3 mod 64 throughout, 512 random"""
    r = np.arange(n)
    pick = np.concatenate([r[:64], r[-64:], r[(r % 64) < 4], np.random.default_rng(seed).choice(n, 512, replace=False)])
    return np.unique(pick)


EXHAUSTIVE_N = (1, 2, 3, 7, 9, 32, 33, 63, 64, 65, 127, 128, 129, 193, 4095, 4096, 4097, 16383, 16384, 16385)


def _exhaustive(n):
    ks = (32,) if n in (32, 33) else K_LIST
    rows = switch_rows(n, 700 + n) if n >= 4095 else None
    return Scene(f"exhaustive_{n}", general_cloud(n, 100 + n), "general", ks, ("exhaustive",), rows=rows)


LATTICE_SHIFT = 3        # lattice scenes: integers times 2^-3, cells of edge 1
LONG_CELL = 300          # coincident-or-tied points of the last cell
HOST_DIMS = ((1, 1, 1), (2, 2, 2), (9, 1, 1), (1, 1, 7), (5, 4, 3), (7, 3, 1))
HOST_ORIGIN = (-2.0, 1.0, 0.5)


def _host_lattice(dims):
    """one to three lattice points in EVERY cell of a dims grid of unit cells, corners included, and LONG_CELL points on
    three tied positions of the last cell (the last records of the cell-sorted array: the long-row loop runs ~40 rounds
    and its prefetch ends clamped at N - 1); rows shuffled, so that index order is not cell order"""
    rng = np.random.default_rng(1000 + dims[0] * 100 + dims[1] * 10 + dims[2])
    q = 1 << LATTICE_SHIFT
    pts = []
    for z in range(dims[2]):
        for y in range(dims[1]):
            for x in range(dims[0]):
                for _ in range(int(rng.integers(1, 4))):
                    pts.append(np.array([x, y, z]) * q + rng.integers(0, q, 3))
    last = (np.array(dims) - 1) * q
    spots = last[None, :] + np.array([[3, 3, 3], [4, 3, 3], [3, 4, 3]])
    pts.extend(spots[rng.integers(0, 3, LONG_CELL)])
    ints = np.stack(pts)[rng.permutation(len(pts))]
    xyz = ints.astype(np.float32) * np.float32(2.0 ** -LATTICE_SHIFT) + np.asarray(HOST_ORIGIN, np.float32)[None, :]
    return Scene("host_%dx%dx%d" % dims, torch.from_numpy(xyz), "lattice", (1, 6, 32), ("host", "grid", "exhaustive"),
                 grid=(list(HOST_ORIGIN), 1.0, list(dims)))


EDGE_N = (15, 16, 17, 63, 64, 65, 257)


def _edge(n):
    """n lattice points in a 4 x 4 x 4 grid of unit cells: four queries per wavefront, sixteen per workgroup, up to a
    ragged last workgroup"""
    rng = np.random.default_rng(2000 + n)
    ints = rng.integers(0, 4 << LATTICE_SHIFT, (n, 3))
    xyz = ints.astype(np.float32) * np.float32(2.0 ** -LATTICE_SHIFT)
    return Scene(f"edge_{n}", torch.from_numpy(xyz), "lattice", (1, 6), ("grid", "host", "exhaustive"),
                 grid=([0.0, 0.0, 0.0], 1.0, [4, 4, 4]))


def _fullscan_sparse():
    """200 points on 8 x 8 x 8 cells (r_brute = 1: N < 375): most queries need a second block of radius 2..7 and take
    the full scan instead"""
    pts = torch.rand(200, 3, generator=_gen(31))
    return Scene("fullscan_sparse", pts, "general", (6,), ("host",), grid=([0.0, 0.0, 0.0], 0.125, [8, 8, 8]))


FAR_N = 4336   # the smallest N with r_brute = 8: 17 * 17 * 15 = 4335 < N
FAR_K = 6


def _far_corner(near):
    """12 x 12 x 12 unit cells, the bulk in the cells 9..11 of every axis, one outlier (row 0) in cell (0, 0, 0): nothing
    within its blocks of radius 1, 2, 4.  near: K + 2 points in cell (7, 7, 0), about ten cells away on a face diagonal --
    found by the block of radius 8 but beyond its reach, radius 10 or 11 needed: the full scan.  Without them the K-th
    distance stays infinite and the radius runs 1, 2, 4, 8, 12 = rmax."""
    g = _gen(41 if near else 43)
    n_near = FAR_K + 2 if near else 0
    bulk = 9.0 + 3.0 * torch.rand(FAR_N - 1 - n_near, 3, generator=g)
    out = torch.tensor([[0.4, 0.6, 0.5]])
    parts = [out]
    if near:
        parts.append(torch.tensor([7.2, 7.2, 0.2]) + 0.6 * torch.rand(n_near, 3, generator=g))
    pts = torch.cat(parts + [bulk]).float()
    return Scene("fullscan_outlier" if near else "empty_growth", pts, "general", (FAR_K,), ("host",),
                 grid=([0.0, 0.0, 0.0], 1.0, [12, 12, 12]))


def _ring_border():
    """2000 points on 12 x 12 x 12 unit cells (1.2 per cell: the sixth neighbour sits about 1.06 cells away), half of
    the coordinates within 0.05 of a cell face: for many queries the K-th distance of the first block is just beyond
    its reach while a nearer point lies just behind the block's nearest face -- a search that settles a little early
    is wrong on those rows"""
    g = _gen(37)
    n = 2000
    cell = torch.randint(0, 12, (n, 3), generator=g).float()
    frac = torch.rand(n, 3, generator=g)
    near = 0.05 * torch.rand(n, 3, generator=g)
    side = torch.rand(n, 3, generator=g)
    frac = torch.where(side < 0.25, near, torch.where(side < 0.5, 1.0 - near, frac))
    pts = (cell + frac).clamp(0.0, 11.999)
    return Scene("ring_border", pts, "general", (6,), ("host", "grid"), grid=([0.0, 0.0, 0.0], 1.0, [12, 12, 12]))


SCAN_DIMS = ((15, 13, 21), (16, 16, 16), (16, 16, 32), (32, 32, 32))   # 4095, 4096, 8192 and 32768 cells


def _scan(dims):
    """200 points on a grid whose C + 1 scan entries end in another thread / workgroup of knn_scan_kernel each time:
    one workgroup (start[C] from thread 255), two (thread 0 of the second), three, nine"""
    cell = 1.0 / 16.0
    pts = torch.rand(200, 3, generator=_gen(50 + dims[2])) * (torch.tensor(dims, dtype=torch.float32) * cell)
    return Scene("scan_%dx%dx%d" % dims, pts.float(), "general", (6,), ("host",), grid=([0.0, 0.0, 0.0], cell, list(dims)))


def clustered_cloud(n, seed=11):
    """the clustered-plus-floaters cloud of test_knn_matches_sklearn: half the points along six segments with 0.003
    noise, half spread through the volume"""
    g = _gen(seed)
    t = torch.rand(n, 1, generator=g)
    seg = torch.randint(0, 6, (n,), generator=g)
    a, b = torch.rand(6, 3, generator=g), torch.rand(6, 3, generator=g)
    pts = a[seg] * (1 - t) + b[seg] * t + 0.003 * torch.randn(n, 3, generator=g)
    pts[n // 2:] = torch.rand(n - n // 2, 3, generator=g) * 1.3 - 0.15
    return pts


def _auto(name):
    g = _gen(60 + sum(map(ord, name)))
    kind, ks, rows, n = "general", (6,), None, 600
    if name == "two_bbox_workgroups":
        n = 2049
        pts = torch.rand(n, 3, generator=g) * torch.tensor([1.0, 0.6, 0.3])
    elif name == "all_negative":
        pts = -0.25 - torch.rand(n, 3, generator=g)
    elif name == "mixed_sign":
        pts = torch.rand(n, 3, generator=g) * 2.0 - 1.0
    elif name == "negative_zero":
        pts = torch.rand(n, 3, generator=g) * 2.0 - 1.0
        pts[:200, 0] = -0.0
        pts[100:300, 1] = 0.0
        pts[:, 2] = pts[:, 2].abs()
        pts[300:400, 2] = -0.0     # the minimum of an axis that has no negative number
    elif name == "tiny_extent":
        pts = (1000.0 + (torch.rand(n, 3, generator=g) * 0.02 - 0.01)).float()
    elif name == "line":
        pts = torch.rand(n, 3, generator=g)
        pts[:, 1:] = 0.25
    elif name == "plane":
        pts = torch.rand(n, 3, generator=g)
        pts[:, 2] = -0.5
    elif name == "spot":
        pts, kind = torch.full((n, 3), 0.25), "lattice"
    elif name in ("clustered_k6", "clustered_k21"):
        n = 20000
        pts, ks = clustered_cloud(n), ((6,) if name.endswith("k6") else (21,))
        rows = np.sort(np.random.default_rng(77).choice(n, 2048, replace=False))
    else:
        raise KeyError(name)
    return Scene("auto_" + name, pts.float(), kind, ks, ("grid",), rows=rows)


AUTO_NAMES = ("two_bbox_workgroups", "all_negative", "mixed_sign", "negative_zero", "tiny_extent", "line", "plane", "spot",
              "clustered_k6", "clustered_k21")

KTH_N, KTH_K = 6000, 6


def _kth_lattice():
    """6000 points on the 24^3 sites of a lattice of pitch 1/4: squared distances are small integers / 16, so that
    several candidates tie at the K-th place of nearly every row, and some sites hold two points"""
    rng = np.random.default_rng(91)
    xyz = rng.integers(0, 24, (KTH_N, 3)).astype(np.float32) * np.float32(0.25)
    return Scene("kth_lattice", torch.from_numpy(xyz), "lattice", (KTH_K,), ("grid",))


def _clamp_base():
    return Scene("clamped_base", torch.rand(1000, 3, generator=_gen(71)) * torch.tensor([1.0, 0.6, 0.3]), "general", (6,),
                 ("host",))


def clamped_points(pts, grid):
    """A tenth of the points moved OUT of `grid` (made for `pts` with margin 0), through every one of its six sides:
    by 0.01 cells, by 50 cells, and two of them by 1000 cells.  Returns (moved fp32 [N,3], bool [N] which)."""
    origin, cell, dims = grid
    lo = np.asarray(origin, np.float64)
    hi = lo + np.asarray(dims, np.float64) * cell
    p = pts.double().numpy().copy()
    rng = np.random.default_rng(72)
    which = rng.choice(p.shape[0], p.shape[0] // 10, replace=False)
    for n, i in enumerate(which):
        axis, up = n % 3, (n // 3) % 2
        by = 1000.0 if n < 2 else (0.01 if (n // 6) % 2 == 0 else 50.0)
        by *= 1.0 + 0.5 * rng.random()
        p[i, axis] = hi[axis] + by * cell if up else lo[axis] - by * cell
    moved = np.zeros(p.shape[0], bool)
    moved[which] = True
    return torch.from_numpy(p).float(), moved


_BUILDERS = {}
for _n in EXHAUSTIVE_N:
    _BUILDERS[f"exhaustive_{_n}"] = (_exhaustive, _n)
for _d in HOST_DIMS:
    _BUILDERS["host_%dx%dx%d" % _d] = (_host_lattice, _d)
for _n in EDGE_N:
    _BUILDERS[f"edge_{_n}"] = (_edge, _n)
_BUILDERS["ring_border"] = (_ring_border,)
_BUILDERS["fullscan_sparse"] = (_fullscan_sparse,)
_BUILDERS["fullscan_outlier"] = (_far_corner, True)
_BUILDERS["empty_growth"] = (_far_corner, False)
for _d in SCAN_DIMS:
    _BUILDERS["scan_%dx%dx%d" % _d] = (_scan, _d)
for _a in AUTO_NAMES:
    _BUILDERS["auto_" + _a] = (_auto, _a)
_BUILDERS["kth_lattice"] = (_kth_lattice,)
_BUILDERS["clamped_base"] = (_clamp_base,)

SCENE_NAMES = tuple(_BUILDERS)
HOST_SCENES = tuple("host_%dx%dx%d" % d for d in HOST_DIMS)
EDGE_SCENES = tuple(f"edge_{n}" for n in EDGE_N)
SCAN_SCENES = tuple("scan_%dx%dx%d" % d for d in SCAN_DIMS)
AUTO_SCENES = tuple("auto_" + a for a in AUTO_NAMES)
EXHAUSTIVE_SCENES = tuple(f"exhaustive_{n}" for n in EXHAUSTIVE_N)
_cache = {}


def scene(name):
    if ("scene", name) not in _cache:
        b = _BUILDERS[name]
        _cache[("scene", name)] = b[0](*b[1:])
    return _cache[("scene", name)]


def reference(name, k, extra=0):
    """knn_ref of the scene's checked rows, computed once per scene at K_MAX + 1 columns and sliced (a stable sort's
    first k columns do not depend on how many are taken): (idx [R,k+extra], d2 [R,k+extra])."""
    sc = scene(name)
    if ("ref", name) not in _cache:
        _cache[("ref", name)] = knn_ref(sc.pts, K_MAX + 1, rows=sc.rows)
    idx, d2 = _cache[("ref", name)]
    assert k + extra <= K_MAX + 1
    return idx[:, :k + extra], d2[:, :k + extra]


def trace(name, k, grid=None):
    """ring_trace of the scene's checked rows on its host grid (or `grid`), cached"""
    sc = scene(name)
    key = ("trace", name, k, None if grid is None else repr(grid))
    if key not in _cache:
        _cache[key] = ring_trace(sc.pts, grid if grid is not None else sc.grid, k, rows=sc.rows)
    return _cache[key]


def auto_host_grid(pts, k):
    """auto_grid in the (origin, cell, dims) form ring_trace takes"""
    origin, cell, _, D = auto_grid(pts, k)
    return ([float(x) for x in origin], float(cell), [D, D, D])
