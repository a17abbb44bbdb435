"""The two wide entries of csrc/tiles.hip are exported with the signatures include/edgegs.h declares, and reject bad
arguments with a negative code before any HIP call (no device is touched: this runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = "eg_composite_fwd_wide_cams", "eg_composite_bwd_wide_cams"


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
    for name in (FWD, BWD):
        assert hasattr(h, name), name
        bound = ["ptr" if t is ctypes.c_void_p else {ctypes.c_int32: "int32_t"}[t] for t in lib._SIGS[name]]
        assert bound == _declared_args(name), name
    # the arguments of the mode entries, then the real channel count and the two row strides, then the stream
    for wide, modes in ((FWD, "eg_composite_fwd_modes_cams"), (BWD, "eg_composite_bwd_modes_cams")):
        assert lib._SIGS[wide] == lib._SIGS[modes][:-1] + [ctypes.c_int32] * 3 + [ctypes.c_void_p]


def test_bad_arguments_are_rejected_before_any_hip_call(lib):
    h = lib.load(require_device=False)
    buf = (ctypes.c_float * 64)()  # a non-null host address: it is never dereferenced
    q = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(channels=8, n_real=8, cs=8, ps=8, colors=q, depth=0, splat=q):
        return h.eg_composite_fwd_wide_cams(1, splat, 4, colors, 0, channels, depth, None, q, q, 32, 32, q, q, q, n_real,
                                            cs, ps, None)

    def bwd(channels=8, n_real=8, cs=8, ps=8, colors=q, depth=0, v_depths=None, g2d=q):
        return h.eg_composite_bwd_wide_cams(1, q, 4, colors, 0, channels, depth, None, q, q, 32, 32, q, q, q, None, g2d, q,
                                            v_depths, n_real, cs, ps, None)

    for f, name in ((fwd, FWD), (bwd, BWD)):
        assert f(channels=0, n_real=0) < 0 and name.encode() in h.eg_last_error_string()
        assert f(channels=33, n_real=33, cs=64, ps=64) < 0          # wider than one launch takes
        assert f(channels=8, n_real=9, cs=16, ps=16) < 0            # more real channels than the chunk is wide
        assert f(channels=8, n_real=0) < 0
        assert f(colors=None) < 0 and b"null colors" in h.eg_last_error_string()
        assert f(cs=7) < 0 and b"stride" in h.eg_last_error_string()
        assert f(ps=7) < 0 and b"stride" in h.eg_last_error_string()
        assert f(ps=8, depth=1, **({"v_depths": q} if f is bwd else {})) < 0   # the depth channel needs a ninth column
    assert fwd(splat=None) < 0 and b"null pointer" in h.eg_last_error_string()
    assert bwd(g2d=None) < 0
    assert bwd(depth=1, ps=9, v_depths=None) < 0 and b"v_depths" in h.eg_last_error_string()
    assert h.eg_composite_fwd_wide_cams(0, q, 4, q, 0, 8, 0, None, q, q, 32, 32, q, q, q, 8, 8, 8, None) < 0  # no camera
