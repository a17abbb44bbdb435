"""edgegaussians_amd.edges / the point-cloud PLY reader without a GPU: argument validation and the refusal of the CPU,
the C ABI of the three edge-sampling entries (exported, bound, arguments validated before any HIP call),
`io.read_points_ply` / `write_points_ply`, and the conditions tests/golden/edge_sampling.npz was generated under."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

ENTRIES = ("eg_edge_sample_count", "eg_edge_sample_emit", "eg_edge_sample")
LINES = {"curves_ctl_pts": [], "lines_end_pts": [[0, 0, 0, 0.1, 0, 0]]}


def test_sample_validates_its_arguments_before_touching_a_device():
    from edgegaussians_amd import edges
    with pytest.raises(ValueError, match="no CPU path"):
        edges.sample(LINES, device="cpu")
    with pytest.raises(ValueError, match="no CPU path"):
        edges.evaluate_edges(LINES, torch.rand(10, 3))
    with pytest.raises(ValueError, match="no CPU path"):
        edges.evaluate_edges(LINES, np.zeros((10, 3), np.float32))
    for bad in (0, 0.0, -0.005, float("nan"), float("inf"), "0.005"):
        with pytest.raises(ValueError, match="sample_resolution"):
            edges.sample(LINES, sample_resolution=bad)
    with pytest.raises(ValueError, match="tangent"):
        edges.sample(LINES, tangent="true")
    # wrong last dimensions: rows of 2, a curve of 3 control points, a line of 3 end points
    with pytest.raises(ValueError, match="lines_end_pts"):
        edges.sample((np.zeros((0, 4, 3)), np.zeros((3, 2, 2))))
    with pytest.raises(ValueError, match="curves_ctl_pts"):
        edges.sample({"curves_ctl_pts": np.zeros((1, 3, 3)).tolist(), "lines_end_pts": []})
    with pytest.raises(ValueError, match="lines_end_pts"):
        edges.sample({"curves_ctl_pts": [], "lines_end_pts": np.zeros((1, 3, 3)).tolist()})
    # non-finite control points
    c = np.zeros((2, 4, 3))
    c[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        edges.sample((c, np.zeros((0, 2, 3))))
    with pytest.raises(ValueError, match="non-finite"):
        edges.sample((torch.zeros(0, 4, 3), torch.full((1, 2, 3), float("inf"))))
    with pytest.raises(ValueError, match="capacity"):
        edges.sample(LINES, capacity=-1)


def test_the_module_is_exported():
    import edgegaussians_amd
    assert "edges" in edgegaussians_amd.__all__ and hasattr(edgegaussians_amd.edges, "evaluate_edges")
    for name in ("sample", "get_pred_points_and_directions", "get_pred_points_and_directions_from_dict"):
        assert callable(getattr(edgegaussians_amd.edges, name))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    return _lib


def test_edge_entries_are_exported_and_bound(lib):
    h = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(h, name), name
        assert name in lib.EXPORTS and name in lib._SIGS
    assert [len(lib._SIGS[n]) for n in ENTRIES] == [11, 13, 16]


def test_edge_entries_validate_arguments_without_launching(lib):
    h = lib.load(require_device=False)
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)  # a non-null pointer: never dereferenced, every call below is refused or has nothing to do
    host = (ctypes.c_int32 * 2)()
    count = lambda c, nc, l, nl, res, le, cn, of, to: h.eg_edge_sample_count(c, nc, l, nl, res, -1, le, cn, of, to, None)  # noqa: E731
    emit = lambda c, nc, l, nl, cn, of, to, cap, tan, pts: h.eg_edge_sample_emit(c, nc, l, nl, cn, of, to, cap, tan, pts, None, None, None)  # noqa: E731
    both = lambda c, nc, l, nl, res, cap, tan, le, cn, of, to, pts, th: h.eg_edge_sample(c, nc, l, nl, res, cap, tan, le, cn, of, to, pts, None, None, th, None)  # noqa: E731

    def refused(rc, name, what):
        assert rc == -1, (name, rc)
        msg = h.eg_last_error_string()
        assert name.encode() in msg and what in msg, msg

    # sizes
    for nc, nl in ((-1, 2), (2, -1), (1 << 30, 0)):
        refused(count(p, nc, p, nl, 0.005, p, p, p, p), "eg_edge_sample_count", b"bad sizes")
        refused(emit(p, nc, p, nl, p, p, p, 8, 0, p), "eg_edge_sample_emit", b"bad sizes")
        refused(both(p, nc, p, nl, 0.005, 8, 0, p, p, p, p, p, host), "eg_edge_sample", b"bad sizes")
    for res in (0.0, -1.0, float("nan"), float("inf")):
        refused(count(p, 1, p, 1, res, p, p, p, p), "eg_edge_sample_count", b"resolution")
        refused(both(p, 1, p, 1, res, 8, 0, p, p, p, p, p, host), "eg_edge_sample", b"resolution")
    refused(emit(p, 1, p, 1, p, p, p, -1, 0, p), "eg_edge_sample_emit", b"capacity")
    refused(emit(p, 1, p, 1, p, p, p, 1 << 31, 0, p), "eg_edge_sample_emit", b"capacity")
    refused(both(p, 1, p, 1, 0.005, -1, 0, p, p, p, p, p, host), "eg_edge_sample", b"capacity")
    refused(emit(p, 1, p, 1, p, p, p, 8, 2, p), "eg_edge_sample_emit", b"tangent")
    refused(both(p, 1, p, 1, 0.005, 8, 7, p, p, p, p, p, host), "eg_edge_sample", b"tangent")
    # null pointers (a side without primitives may be null)
    for args in ((None, 1, p, 1, 0.005, p, p, p, p), (p, 1, None, 1, 0.005, p, p, p, p), (p, 1, p, 1, 0.005, None, p, p, p),
                 (p, 1, p, 1, 0.005, p, None, p, p), (p, 1, p, 1, 0.005, p, p, None, p), (p, 1, p, 1, 0.005, p, p, p, None),
                 (None, 0, None, 0, 0.005, None, None, None, p)):
        refused(count(*args), "eg_edge_sample_count", b"null pointer")
    for args in ((None, 1, p, 1, p, p, p, 8, 0, p), (p, 1, None, 1, p, p, p, 8, 0, p), (p, 1, p, 1, None, p, p, 8, 0, p),
                 (p, 1, p, 1, p, None, p, 8, 0, p), (p, 1, p, 1, p, p, None, 8, 0, p), (p, 1, p, 1, p, p, p, 8, 0, None)):
        refused(emit(*args), "eg_edge_sample_emit", b"null pointer")
    for args in ((None, 1, p, 1, 0.005, 8, 0, p, p, p, p, p, host), (p, 1, p, 1, 0.005, 8, 0, None, p, p, p, p, host),
                 (p, 1, p, 1, 0.005, 8, 0, p, p, None, p, p, host), (p, 1, p, 1, 0.005, 8, 0, p, p, p, None, p, host),
                 (p, 1, p, 1, 0.005, 8, 0, p, p, p, p, None, host), (p, 1, p, 1, 0.005, 8, 0, p, p, p, p, p, None)):
        refused(both(*args), "eg_edge_sample", b"null pointer")
    # nothing to emit: no launch, whatever the pointers
    assert emit(None, 0, None, 0, None, None, None, 8, 0, None) == 0
    assert emit(p, 1, p, 1, None, None, None, 0, 0, None) == 0


# ---- PLY point clouds

def _write(path, header_lines, payload):
    with open(path, "wb") as f:
        f.write(("\n".join(header_lines) + "\n").encode("ascii"))
        f.write(payload)


def test_read_points_ply_open3d_layout(tmp_path):
    """double x y z + uchar red green blue, binary little endian: the reference's groundtruth/sampled_pts files."""
    from edgegaussians_amd import io
    rng = np.random.default_rng(0)
    rec = np.zeros(37, dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    xyz = rng.random((37, 3))
    rec["x"], rec["y"], rec["z"] = xyz.T
    rec["red"], rec["green"], rec["blue"] = rng.integers(0, 256, (3, 37))
    path = str(tmp_path / "o3d.ply")
    _write(path, ["ply", "format binary_little_endian 1.0", "comment Created by Open3D", "element vertex 37",
                  "property double x", "property double y", "property double z", "property uchar red",
                  "property uchar green", "property uchar blue", "end_header"], rec.tobytes())
    got = io.read_points_ply(path)
    assert got.dtype == np.float64 and got.shape == (37, 3) and np.array_equal(got, xyz)
    with pytest.raises(KeyError):  # (what the issue reports of the Gaussian reader: it stays as it is)
        io.read_gaussian_params_from_ply(path)
    # big endian, coordinates in another order, a trailing face element with a list property
    rec_be = np.zeros(5, dtype=[("z", ">f4"), ("nx", ">i2"), ("x", ">f4"), ("y", ">f8")])
    rec_be["x"], rec_be["y"], rec_be["z"], rec_be["nx"] = [1, 2, 3, 4, 5], [.5, .25, 0, -1, -2], [9, 8, 7, 6, 5], 7
    path = str(tmp_path / "be.ply")
    _write(path, ["ply", "format binary_big_endian 1.0", "element vertex 5", "property float z", "property short nx",
                  "property float32 x", "property float64 y", "element face 0", "property list uchar int vertex_indices",
                  "end_header"], rec_be.tobytes())
    assert np.array_equal(io.read_points_ply(path), np.stack([rec_be["x"], rec_be["y"], rec_be["z"]], 1).astype(np.float64))


def test_read_points_ply_ascii_and_extra_float_properties(tmp_path):
    from edgegaussians_amd import io
    path = str(tmp_path / "a.ply")
    _write(path, ["ply", "format ascii 1.0", "element vertex 3", "property float x", "property float y",
                  "property float z", "property uchar red", "end_header"],
           b"0.5 1.25 -2 255\n1e-3 0 7.5 0\n3 4 5 17\n")
    assert np.array_equal(io.read_points_ply(path), [[0.5, 1.25, -2], [1e-3, 0, 7.5], [3, 4, 5]])
    # the Gaussian file of write_gaussian_params_as_ply: float x y z + 8 more float properties
    rng = np.random.default_rng(1)
    means = rng.random((11, 3)).astype(np.float32)
    path = str(tmp_path / "g.ply")
    io.write_gaussian_params_as_ply(means, rng.random((11, 3)), rng.random((11, 4)), rng.random((11, 1)), path)
    got = io.read_points_ply(path)
    assert got.dtype == np.float64 and np.array_equal(got, means.astype(np.float64))


def test_points_ply_round_trip(tmp_path):
    from edgegaussians_amd import io
    pts = np.random.default_rng(2).normal(size=(101, 3))
    path = str(tmp_path / "p.ply")
    io.write_points_ply(pts, path)
    assert np.array_equal(io.read_points_ply(path), pts)
    head = open(path, "rb").read(200).decode("ascii", "replace")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex 101\nproperty double x\n")
    io.write_points_ply(torch.from_numpy(pts.astype(np.float32)), path)  # tensors too
    assert np.array_equal(io.read_points_ply(path), pts.astype(np.float32).astype(np.float64))
    io.write_points_ply(np.zeros((0, 3)), path)
    assert io.read_points_ply(path).shape == (0, 3)


def test_read_points_ply_refuses_lists_and_missing_coordinates(tmp_path):
    from edgegaussians_amd import io
    path = str(tmp_path / "l.ply")
    _write(path, ["ply", "format ascii 1.0", "element vertex 1", "property float x", "property float y",
                  "property float z", "property list uchar int n", "end_header"], b"0 0 0 1 5\n")
    with pytest.raises(ValueError, match="list property"):
        io.read_points_ply(path)
    path = str(tmp_path / "m.ply")
    _write(path, ["ply", "format ascii 1.0", "element vertex 1", "property float x", "property float y", "end_header"],
           b"0 0\n")
    with pytest.raises(ValueError, match="no z"):
        io.read_points_ply(path)


# ---- the fixture

def test_fixture_conditions_hold(golden_dir):
    path = os.path.join(golden_dir, "edge_sampling.npz")
    assert os.path.getsize(path) < 200_000
    g = np.load(path)
    curves, lines, lengths = g["mixed_curves"], g["mixed_lines"], g["mixed_lengths"]
    assert curves.shape == (7, 4, 3) and lines.shape == (7, 2, 3) and g["short_lines"].shape == (300, 2, 3)
    assert int(g["seed"].reshape(-1)[0]) >= 0
    assert (curves[6] == curves[6, 0]).all() and lengths[6] == 0.0  # the degenerate curve
    assert np.array_equal(lengths[7:10], [0.1, 0.003, 0.0051])       # the constructed lines, exactly
    assert ((curves >= 0) & (curves <= 1)).all()
    sl = g["short_lengths"]
    assert sl.min() >= 0.006 - 1e-12 and sl.max() <= 0.05 + 1e-12
    free = np.ones(14, bool)
    free[6:10] = False
    for r in (0.005, 0.02):
        counts = g[f"mixed_{r}_counts"]
        # 1. no length within 1e-6 (in units of the resolution) of a count boundary
        q = lengths / r
        assert np.abs(q - np.round(q))[free].min() >= 1e-6
        assert np.array_equal(counts[free], np.floor(q[free]).astype(np.int32))
        assert counts[6] == 0
        assert counts[:7].sum() == len(g[f"mixed_{r}_curve_points"]) == len(g[f"mixed_{r}_curve_dirs"])
        assert counts[7:].sum() == len(g[f"mixed_{r}_line_points"]) == len(g[f"mixed_{r}_line_dirs"])
        # 2. the reference's curve direction before normalisation (eval_utils.py:322-364) is nowhere near zero
        for P, n in zip(curves[:6], counts[:6]):
            t = np.linspace(0, 1, n)
            d = np.outer(3 * t ** 2, -3 * P[0] + 9 * P[1] - 9 * P[2] + 3 * P[3]) \
                + np.outer(2 * t, 6 * P[0] - 12 * P[1] + 6 * P[2]) + (-3 * P[0] + 3 * P[1])
            assert np.linalg.norm(d, axis=1).min() > 0.1
    assert list(g["mixed_0.005_counts"][7:10]) == [20, 0, 1]  # (as the reference gives them)
    q = sl / 0.005
    assert np.abs(q - np.round(q)).min() >= 1e-6
    assert np.array_equal(g["short_counts"], np.floor(q).astype(np.int32)) and g["short_counts"].min() >= 1
    assert g["short_counts"].sum() == len(g["short_points"]) == len(g["short_dirs"])
    # 3. no nearest-neighbour distance within 1e-5 of a threshold, both ways, in float64
    pred = np.concatenate([g["mixed_0.005_curve_points"], g["mixed_0.005_line_points"]]).astype(np.float32).astype(np.float64)
    gt = g["gt"]
    assert gt.dtype == np.float32 and gt.shape[1] == 3
    gt = gt.astype(np.float64)
    d1, _ = cKDTree(gt).query(pred, k=1)
    d2, _ = cKDTree(pred).query(gt, k=1)
    for t in g["thresholds"]:
        assert np.abs(d1 - t).min() > 1e-5 and np.abs(d2 - t).min() > 1e-5
        assert 0 < (d1 < t).sum() and 0 < (d2 < t).sum()  # the distances straddle the thresholds
    assert (d1 < 0.005).sum() < len(d1) and (d2 < 0.005).sum() < len(d2)
