"""The entries of csrc/tiles.hip (tile sizes 8 and 32) are exported with the signatures include/edgegs.h declares and
reject a bad tile size or bad sizes before any HIP call; the scene discipline of the device tests (tests/tile_util.py)
keeps its caps on the scene they use.  No device is touched: this runs without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, EMIT, FWD, BWD = "eg_tile_count_ts", "eg_tile_emit_sort_ts", "eg_composite_fwd_ts_cams", "eg_composite_bwd_ts_cams"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    return _lib


def _declared_args(name):
    """The C parameter types of `name` in the header, pointers as 'ptr'."""
    src = open(os.path.join(ROOT, "include", "edgegs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, name
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append("ptr" if ("*" in a or a.startswith("eg_stream_t")) else a.rsplit(" ", 1)[0])
    return out


def test_entries_are_exported_and_bound_as_declared(lib):
    h = ctypes.CDLL(lib.LIB_PATH)
    for name in (COUNT, EMIT, FWD, BWD):
        assert hasattr(h, name), name
        assert name in lib.EXPORTS
        bound = ["int32_t" if t is ctypes.c_int32 else "ptr" for t in lib._SIGS[name]]
        assert bound == _declared_args(name), name
    # the wide entries' arguments with the tile size behind `height`
    for ts_entry, wide in ((FWD, "eg_composite_fwd_wide_cams"), (BWD, "eg_composite_bwd_wide_cams")):
        w = lib._SIGS[wide]
        assert lib._SIGS[ts_entry] == w[:12] + [ctypes.c_int32] + w[12:]


def test_bad_tile_sizes_and_sizes_are_rejected_before_any_hip_call(lib):
    h = lib.load(require_device=False)
    buf = (ctypes.c_float * 64)()  # a non-null host address: it is never dereferenced
    q = ctypes.cast(buf, ctypes.c_void_p)
    ranges = (ctypes.c_int64 * 2)(0, 4)
    ms = (ctypes.c_int64 * 1)(4)

    def count(ts=8, C=1, width=32, height=32, rng=ranges):
        return h.eg_tile_count_ts(q, q, rng, C, width, height, ts, q, q, None)

    def emit(ts=8, C=1, width=32, height=32, rng=ranges):
        return h.eg_tile_emit_sort_ts(q, q, q, rng, C, width, height, ts, q, q, ms, q, q, q, None, 0, None)

    def fwd(ts=8, C=1, width=32, height=32, channels=4, n_real=4, depth=0, ps=4):
        return h.eg_composite_fwd_ts_cams(C, q, 4, q, 0, channels, depth, None, q, q, width, height, ts, q, q, q, n_real, 4,
                                          ps, None)

    def bwd(ts=8, C=1, width=32, height=32, channels=4, n_real=4, depth=0, ps=4, v_depths=None):
        return h.eg_composite_bwd_ts_cams(C, q, 4, q, 0, channels, depth, None, q, q, width, height, ts, q, q, q, None, q, q,
                                          v_depths, n_real, 4, ps, None)

    for f, name in ((count, COUNT), (emit, EMIT), (fwd, FWD), (bwd, BWD)):
        for ts in (12, 0, -8, 7, 64, 16):  # (16 has its own entries)
            assert f(ts=ts) != 0 and name.encode() in h.eg_last_error_string(), (name, ts)
            assert b"tile_size" in h.eg_last_error_string()
        assert f(width=0) != 0 and b"bad sizes" in h.eg_last_error_string()
        assert f(height=-1) != 0 and b"bad sizes" in h.eg_last_error_string()
        assert f(C=0) != 0 and b"bad sizes" in h.eg_last_error_string()
    # the cameras' ranges: present, ascending
    assert count(rng=None) != 0 and b"null pointer" in h.eg_last_error_string()
    assert emit(rng=(ctypes.c_int64 * 2)(4, 0)) != 0 and b"bad ranges" in h.eg_last_error_string()
    # the chunk: 0 .. 32 channels; the depth-only form needs the depth channel and has no real colour channel
    for f in (fwd, bwd):
        assert f(channels=33, n_real=33) != 0
        assert f(channels=4, n_real=5) != 0
        assert f(channels=0, n_real=0, depth=0) != 0 and b"depth" in h.eg_last_error_string()
        assert f(channels=0, n_real=1, depth=1, **({"v_depths": q} if f is bwd else {})) != 0
        assert f(channels=4, n_real=4, depth=1, ps=4, **({"v_depths": q} if f is bwd else {})) != 0  # no fifth column
    assert bwd(channels=0, n_real=0, depth=1, ps=1, v_depths=None) != 0 and b"v_depths" in h.eg_last_error_string()


def test_binning_entries_keep_their_error_strings(lib):
    """The entries over the shared counting / emission kernels and the per-camera binning step (csrc/binning.hip) each
    keep their own checks and messages.  Every call below is invalid, so none of them reaches a launch."""
    h = lib.load(require_device=False)
    buf = (ctypes.c_float * 64)()  # a non-null host address: it is never dereferenced
    q = ctypes.cast(buf, ctypes.c_void_p)
    err = h.eg_last_error_string

    def i64(*v):
        return (ctypes.c_int64 * len(v))(*v)

    def ptrs(*v):
        return (ctypes.c_void_p * len(v))(*v)

    def count(N=4, width=32, height=32, means2d=q, radii=q, counts=q):
        return h.eg_tile_count(means2d, radii, N, width, height, q, counts, None)

    def emit(N=4, width=32, height=32, capacity=8, means2d=q, radii=q, depths=q, splat=None, offsets=q, cursor=q, keys=q):
        return h.eg_tile_emit(means2d, radii, depths, splat, 0, N, width, height, offsets, cursor, capacity, keys, None, None)

    def cams(N=4, C=1, width=32, height=32, means2d=q, offsets=q, M=(5,), keys=ptrs(q), flat=ptrs(q), no_M=False):
        return h.eg_tile_emit_sort_cams(means2d, q, q, N, C, width, height, offsets, q, None if no_M else i64(*M), keys, flat,
                                        None, None, None)

    def count_ts(ts=8, C=1, width=32, height=32, rng=(0, 4), means2d=q, counts=q):
        return h.eg_tile_count_ts(means2d, q, i64(*rng) if rng else None, C, width, height, ts, q, counts, None)

    def emit_ts(ts=8, C=1, width=32, height=32, rng=(0, 4), M=(5,), means2d=q, offsets=q, keys=q, flat=q, rebase=0, no_M=False):
        return h.eg_tile_emit_sort_ts(means2d, q, q, i64(*rng) if rng else None, C, width, height, ts, offsets, q,
                                      None if no_M else i64(*M), keys, flat, q, None, rebase, None)

    def packed(indptr=(0, 4), M=(5,), C=1, width=32, height=32, means2d=q, offsets=q, keys=q):
        return h.eg_packed_bin(means2d, q, q, i64(*indptr) if indptr else None, C, width, height, offsets, q, i64(*M), keys, q,
                               q, None, None)

    def said(rc, text):
        assert rc == -1 and text in err(), (rc, text, err())

    # bad sizes
    for kw in (dict(N=-1), dict(width=0), dict(height=-16)):
        said(count(**kw), b"eg_tile_count: bad sizes")
        said(emit(**kw), b"eg_tile_emit: bad sizes")
        said(cams(**kw), b"eg_tile_emit_sort_cams: bad sizes")
    said(emit(capacity=-1), b"eg_tile_emit: bad sizes")
    for kw in (dict(C=0), dict(C=65536), dict(width=0), dict(height=-16)):
        said(count_ts(**kw), b"eg_tile_count_ts: bad sizes")
        said(emit_ts(**kw), b"eg_tile_emit_sort_ts: bad sizes")
    said(cams(C=0), b"eg_tile_emit_sort_cams: bad sizes")
    for kw in (dict(C=0), dict(width=0), dict(height=-16), dict(M=(-1,)), dict(indptr=(0, 1 << 31)), dict(indptr=(0, -1))):
        said(packed(**kw), b"eg_packed_bin: bad sizes")
    said(emit_ts(M=(-1,)), b"eg_tile_emit_sort_ts: bad sizes")
    said(emit_ts(rng=(1 << 31, (1 << 31) + 4), rebase=1), b"eg_tile_emit_sort_ts: bad sizes")  # past the int32 ids
    said(emit_ts(width=1 << 20, height=1 << 20), b"eg_tile_emit_sort_ts: bad sizes")           # 2^34 tiles
    # null pointers
    for kw in (dict(means2d=None), dict(radii=None), dict(counts=None)):
        said(count(**kw), b"eg_tile_count: null pointer")
    for kw in (dict(offsets=None), dict(cursor=None), dict(keys=None)):
        said(emit(**kw), b"eg_tile_emit: null pointer")
    for kw in (dict(means2d=None), dict(radii=None), dict(depths=None)):
        said(emit(**kw), b"eg_tile_emit: need splat or (means2d, radii, depths)")
    for kw in (dict(means2d=None), dict(offsets=None), dict(no_M=True), dict(keys=None), dict(flat=None)):
        said(cams(**kw), b"eg_tile_emit_sort_cams: null pointer")
    said(cams(keys=ptrs(None)), b"eg_tile_emit_sort_cams: null isect array")
    said(cams(flat=ptrs(None)), b"eg_tile_emit_sort_cams: null isect array")
    said(cams(M=(-1,)), b"eg_tile_emit_sort_cams: null isect array")
    for kw in (dict(rng=None), dict(means2d=None), dict(counts=None)):
        said(count_ts(**kw), b"eg_tile_count_ts: null pointer")
    for kw in (dict(rng=None), dict(offsets=None), dict(no_M=True), dict(means2d=None), dict(keys=None), dict(flat=None),
               dict(rng=(0, 0))):  # (the last: intersections of an empty range)
        said(emit_ts(**kw), b"eg_tile_emit_sort_ts: null pointer")
    for kw in (dict(indptr=None), dict(offsets=None), dict(means2d=None), dict(keys=None), dict(indptr=(0, 0))):
        said(packed(**kw), b"eg_packed_bin: null pointer")
    # bad ranges
    for f, name in ((count_ts, b"eg_tile_count_ts"), (emit_ts, b"eg_tile_emit_sort_ts")):
        said(f(rng=(-1, 4)), name + b": bad ranges")
        said(f(rng=(4, 0)), name + b": bad ranges")
        said(f(rng=(0, 1 << 31)), name + b": bad ranges")  # a camera's range past the int32 ids
        said(f(C=2, rng=(0, 4, 2)), name + b": bad ranges")
    said(packed(indptr=(1, 4)), b"eg_packed_bin: indptr must start at 0")
    # 16 stays with the entries of its own
    said(count_ts(ts=16), b"eg_tile_count_ts: tile_size must be 8 or 32 (16: eg_tile_count, eg_tile_emit)")
    said(emit_ts(ts=16), b"eg_tile_emit_sort_ts: tile_size must be 8 or 32 (16: eg_tile_count, eg_tile_emit)")


def test_staging_batches_are_the_kernels(lib):
    """The batch sizes the device tests size their lists by are the named constants of csrc/tiles.hip."""
    src = open(os.path.join(ROOT, "edgegaussians_amd", "csrc", "tiles.hip")).read()
    for ts, name in ((8, "kStage8"), (32, "kStage32")):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src)
        assert m and int(m.group(1)) == lib.TS_STAGE_BATCH[ts], name


def test_rasterization_refuses_other_tile_sizes_by_name():
    import torch
    from edgegaussians_amd import rasterization
    a = (torch.zeros(4, 3), torch.zeros(4, 4), torch.zeros(4, 3), torch.zeros(4), torch.ones(4, 3), torch.eye(4)[None],
         torch.eye(3)[None], 32, 32)
    for ts in (12, 4, 64, 0):
        with pytest.raises(NotImplementedError, match=r"8, 16 or 32"):  # (before anything looks at the tensors)
            rasterization(*a, tile_size=ts, packed=False)


@pytest.mark.parametrize("ts", [8, 32])
@pytest.mark.parametrize("cams", [(1,), (0, 2, 3)], ids=["C1", "C3"])
@pytest.mark.parametrize("mode", ["classic", "antialiased"])
def test_scene_discipline_keeps_its_caps(lib, ts, cams, mode):
    """The conditions the device tests assert, on their scene, cameras and modes, without a device: few Gaussians
    removed, few borderline pixels, the transmittance stop exercised, lists several staging batches long, partial tiles
    on both axes."""
    from tests import tile_util as TU
    sc0 = TU.scene()
    assert sc0.width % 32 and sc0.height % 32 and sc0.width % 8 and sc0.height % 8
    sc, keep, removed, n0, longest, stopped = TU.setup(ts, cams, mode)
    assert removed <= TU.removed_cap(n0), (removed, n0)
    assert float((~keep).float().mean()) < TU.BORDER_CAP
    assert stopped > 0.1 * keep.numel()  # (3 600 - 4 300 of a camera's 28 560 pixels reach the stop)
    assert longest > 2 * lib.TS_STAGE_BATCH[ts]
    # a Gaussian the cleaning keeps has a tile box that does not hinge on rounding
    import numpy as np
    radii, m2d = TU._project(sc, cams[-1])[:2]
    assert not TU.tile_box_borderline(m2d.numpy(), radii.numpy(), ts).any()
    assert TU.tile_box_borderline(np.array([[ts * 3.0 - 1.0, 5.3]]), np.array([1]), ts).all()  # (x + r) / ts == 3
