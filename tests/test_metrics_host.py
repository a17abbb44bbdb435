"""edgegaussians_amd.metrics / filter_stat_outliers without a GPU: the arithmetic of `summarize` against an inline numpy
restatement of eval_utils.py:400-438 / :456-494, the C ABI of the cross-set nearest-neighbour entries (exported, bound,
arguments validated before any HIP call), and the refusal of CPU tensors."""
import ctypes
import math

import numpy as np
import pytest
import torch


def _numpy_summary(a, b, thresholds):
    """The reference's formulas on two numpy distance vectors (a: pred -> gt, b: gt -> pred)."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    out = {"acc": a.mean(), "comp": b.mean()}
    out["chamfer"] = out["acc"] + out["comp"]
    for t in thresholds:
        cp, cg = np.sum(a < t), np.sum(b < t)
        p, r = cp / len(a), cg / len(b)
        with np.errstate(invalid="ignore", divide="ignore"):
            f = 2 * p * r / (p + r)
        out[f"precision_{t}"], out[f"recall_{t}"], out[f"fscore_{t}"] = p, r, f
        out[f"IOU_{t}"] = min(cp, cg) / (len(a) + len(b) - max(cp, cg))
    return out


def _same(got, ref):
    assert sorted(got) == sorted(ref)
    for k, v in ref.items():
        if math.isnan(v):
            assert math.isnan(got[k]), (k, got[k])
        else:
            assert got[k] == pytest.approx(float(v), rel=1e-12, abs=0), (k, got[k], v)


def test_summarize_matches_the_numpy_restatement():
    from edgegaussians_amd import metrics
    rng = np.random.default_rng(3)
    thresholds = (0.005, 0.01, 0.02)
    for q, m in ((3000, 4000), (17, 5), (1, 1000)):
        a = (rng.random(q) ** 2 * 0.05).astype(np.float32)
        b = (rng.random(m) ** 2 * 0.03).astype(np.float32)
        got = metrics.summarize(torch.from_numpy(a), torch.from_numpy(b), thresholds)
        _same(got, _numpy_summary(a, b, thresholds))
        assert all(isinstance(v, float) for v in got.values())
    # float64 sums: a float32 accumulator loses the small terms behind a large one
    a = np.concatenate([[1.0e4], np.full(100000, 1.0e-4)]).astype(np.float32)
    got = metrics.summarize(torch.from_numpy(a), torch.from_numpy(a[:10]), (0.02,))
    assert got["acc"] == pytest.approx(a.astype(np.float64).mean(), rel=1e-12)


def test_summarize_nothing_under_the_threshold():
    from edgegaussians_amd import metrics
    a, b = torch.full((7,), 0.5), torch.full((11,), 0.25)
    got = metrics.summarize(a, b, (0.02, 0.25))  # strict <: 0.25 is not under 0.25
    for t in (0.02, 0.25):
        assert got[f"precision_{t}"] == 0.0 and got[f"recall_{t}"] == 0.0
        assert math.isnan(got[f"fscore_{t}"])
        assert got[f"IOU_{t}"] == 0.0 / (7 + 11)
    assert got["acc"] == 0.5 and got["comp"] == 0.25 and got["chamfer"] == 0.75
    _same(got, _numpy_summary(a.numpy(), b.numpy(), (0.02, 0.25)))


def test_summarize_iou_is_the_references_min_over_max_form():
    """cp = 3 of 4, cg = 1 of 5: IOU = min(3, 1) / (4 + 5 - max(3, 1)) = 1 / 6 -- not a set IoU."""
    from edgegaussians_amd import metrics
    a = torch.tensor([0.001, 0.002, 0.003, 0.5])
    b = torch.tensor([0.001, 0.5, 0.6, 0.7, 0.8])
    got = metrics.summarize(a, b, (0.02,))
    assert got["precision_0.02"] == 3 / 4 and got["recall_0.02"] == 1 / 5
    assert got["IOU_0.02"] == 1 / (9 - 3)
    assert got["fscore_0.02"] == pytest.approx(2 * 0.75 * 0.2 / 0.95, rel=1e-15)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    return _lib


def test_nn_query_entries_are_exported_and_bound(lib):
    h = ctypes.CDLL(lib.LIB_PATH)
    for name in ("eg_nn_query_small", "eg_nn_query_auto"):
        assert hasattr(h, name), name
        assert name in lib.EXPORTS and name in lib._SIGS
    assert len(lib._SIGS["eg_nn_query_small"]) == 7 and len(lib._SIGS["eg_nn_query_auto"]) == 13


def test_nn_query_argument_validation_without_launching(lib):
    h = lib.load(require_device=False)
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)  # a non-null pointer: never dereferenced, every call below is refused or has nothing to do
    big = (1 << 29) + 1
    small = lambda q, nq, t, nt, oi, od: h.eg_nn_query_small(q, nq, t, nt, oi, od, None)  # noqa: E731
    auto = lambda q, nq, t, nt, s, oi, od: h.eg_nn_query_auto(q, nq, t, nt, s, s, s, s, s, s, oi, od, None)  # noqa: E731
    # sizes first
    for nq, nt in ((-1, 4), (4, 0), (4, -3), (big, 4), (4, big), (1 << 40, 4)):
        assert small(p, nq, p, nt, p, p) == -1, (nq, nt)
        assert b"eg_nn_query_small" in h.eg_last_error_string()
        assert auto(p, nq, p, nt, p, p, p) == -1, (nq, nt)
        assert b"eg_nn_query_auto" in h.eg_last_error_string()
    # Q == 0: nothing to do, whatever the pointers
    assert small(None, 0, None, 4, None, None) == 0
    assert auto(None, 0, None, 4, None, None, None) == 0
    # null pointers
    for args in ((None, 4, p, 4, p, p), (p, 4, None, 4, p, p), (p, 4, p, 4, None, p), (p, 4, p, 4, p, None)):
        assert small(*args) == -1, args
        assert b"null pointer" in h.eg_last_error_string()
    for args in ((None, 4, p, 4, p, p, p), (p, 4, None, 4, p, p, p), (p, 4, p, 4, None, p, p), (p, 4, p, 4, p, None, p),
                 (p, 4, p, 4, p, p, None)):
        assert auto(*args) == -1, args
        assert b"null pointer" in h.eg_last_error_string()
    # the exhaustive entry refuses a pair count it would take minutes over
    assert small(p, 1 << 21, p, 1 << 21, p, p) == -1
    assert b"2^40" in h.eg_last_error_string()


def test_cpu_tensors_are_refused():
    from edgegaussians_amd import filtering, metrics
    pts = torch.rand(50, 3)
    with pytest.raises(ValueError, match="no CPU path"):
        metrics.nearest(pts, pts)
    with pytest.raises(ValueError, match="no CPU path"):
        metrics.evaluate(pts, pts)
    with pytest.raises(ValueError, match="no CPU path"):
        filtering.filter_stat_outliers(pts, 10, 3.0)
    with pytest.raises(ValueError, match="no CPU path"):
        filtering.filter_stat_outliers(pts.numpy(), 10, 3.0)
