"""The entries of csrc/packed.hip (packed projection) are exported with the signatures include/edgegs.h declares, and
reject bad arguments with a negative code before any HIP call (no device is touched: this runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("eg_packed_count", "eg_packed_write", "eg_packed_bin", "eg_packed_bwd", "eg_packed_bwd_sparse")
CTYPE = {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_uint32: "uint32_t", ctypes.c_float: "float"}


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


def test_entries_are_exported_with_the_declared_signatures(lib):
    h = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRIES:
        assert name in lib.EXPORTS and name in lib._SIGS, name
        assert hasattr(h, name), name
        bound = ["ptr" if (t is ctypes.c_void_p or hasattr(t, "contents")) else CTYPE[t] for t in lib._SIGS[name]]
        assert bound == _declared_args(name), name
    assert lib.PACKED_STRIDE == 0
    assert re.search(r"#define\s+EG_PACKED_STRIDE\s+0\b", open(os.path.join(ROOT, "include", "edgegs.h")).read())


def test_bad_arguments_are_rejected_before_any_hip_call(lib):
    """Every call below is invalid, so none of them reaches a launch."""
    h = lib.load(require_device=False)
    buf = (ctypes.c_float * 64)()  # a non-null host address: it is never dereferenced
    q = ctypes.cast(buf, ctypes.c_void_p)
    err = h.eg_last_error_string

    def count(N=8, C=1, width=32, height=32, viewmats=q, indptr=q, means=q, block_base=q):
        return h.eg_packed_count(means, q, q, q, viewmats, q, N, C, width, height, 0.01, 1e10, 0.3, 0.0, 0, block_base, indptr,
                                 None)

    def write(N=8, C=1, width=32, height=32, nnz=4, splat=q, camera_ids=q, tile_counts=q, means=q):
        return h.eg_packed_write(means, q, q, q, q, q, N, C, width, height, 0.01, 1e10, 0.3, 0.0, 0, q, nnz, splat, q, q, q, q,
                                 q, q, camera_ids, q, tile_counts, None)

    def bwd(N=8, C=1, width=32, height=32, nnz=4, indptr=q, g2d=q, v_means=q, gaussian_ids=q):
        return h.eg_packed_bwd(q, q, q, q, q, q, N, C, width, height, 0.3, 0, indptr, nnz, gaussian_ids, g2d, q, None, v_means, q,
                               q, None)

    def sparse(N=8, C=1, width=32, height=32, nnz=4, camera_ids=q, g2d=q, v_quats=q):
        return h.eg_packed_bwd_sparse(q, q, q, q, q, q, N, C, width, height, 0.3, 0, nnz, camera_ids, q, g2d, q, None, q, v_quats,
                                      q, None)

    for name, f in (("eg_packed_count", count), ("eg_packed_write", write), ("eg_packed_bwd", bwd),
                    ("eg_packed_bwd_sparse", sparse)):
        assert f(C=0) == -1 and name.encode() in err() and b"bad sizes" in err(), name
        assert f(C=-3) == -1, name
        assert f(N=-1) == -1 and name.encode() in err(), name
        assert f(width=0) == -1 and f(height=-16) == -1, name
    for name, f in (("eg_packed_write", write), ("eg_packed_bwd", bwd), ("eg_packed_bwd_sparse", sparse)):
        assert f(nnz=-1) == -1 and name.encode() in err() and b"nnz" in err(), name
        assert f(nnz=9, N=8, C=1) == -1 and b"nnz" in err(), name      # more pairs than (camera, Gaussian) combinations
    assert count(viewmats=None) == -1 and b"eg_packed_count: null pointer" in err()
    assert count(indptr=None) == -1 and count(means=None) == -1 and count(block_base=None) == -1
    assert write(splat=None) == -1 and b"eg_packed_write: null pointer" in err()
    assert write(camera_ids=None) == -1 and write(tile_counts=None) == -1 and write(means=None) == -1
    assert bwd(indptr=None) == -1 and b"eg_packed_bwd: null pointer" in err()
    assert bwd(g2d=None) == -1 and bwd(v_means=None) == -1 and bwd(gaussian_ids=None) == -1
    assert sparse(camera_ids=None) == -1 and b"eg_packed_bwd_sparse: null pointer" in err()
    assert sparse(g2d=None) == -1 and sparse(v_quats=None) == -1

    def bins(indptr=(0, 4, 9), M=(5, 7), C=2, width=32, height=32, means2d=q, offsets=q, keys=q, flat=q, no_indptr=False):
        ip = (ctypes.c_int64 * len(indptr))(*indptr)
        ms = (ctypes.c_int64 * len(M))(*M)
        return h.eg_packed_bin(means2d, q, q, None if no_indptr else ip, C, width, height, offsets, q, ms, keys, flat, q, None,
                               None)

    assert bins(C=0) == -1 and b"eg_packed_bin: bad sizes" in err()
    assert bins(width=-1) == -1 and bins(height=0) == -1
    assert bins(no_indptr=True) == -1 and b"eg_packed_bin: null pointer" in err()
    assert bins(offsets=None) == -1
    assert bins(indptr=(1, 4, 9)) == -1 and b"indptr" in err()
    assert bins(indptr=(0, 9, 4)) == -1 and b"bad sizes" in err()      # a descending range
    assert bins(indptr=(0, 4, 1 << 31)) == -1                          # past the int32 ids of the sort
    assert bins(M=(5, -1)) == -1
    assert bins(indptr=(0, 0, 9), M=(5, 7)) == -1                      # intersections of an empty range
    assert bins(means2d=None) == -1 and b"null pointer" in err()
    assert bins(keys=None) == -1 and bins(flat=None) == -1             # the LAST camera's check, still before any launch
