"""Camera-pose gradient of the projection, the part that needs no GPU:

* the entry eg_project_bwd_viewmats (csrc/viewmat_grad.hip) is declared in include/edgegs.h, exported with that
  signature and bound in the ctypes table, and refuses null pointers and bad sizes with -1 before any device call;
* the references the device tests (tests/test_gpu_viewmat_grad.py) use, checked against each other: the sum of the
  float64 per-pair contributions is the float64 whole-call gradient, the bottom row is exactly zero, entries no pair
  reaches are exactly zero, and the fp32 oracle stays within an eighth of the bound on every case and n the device
  tests use (the measured worst ratios are recorded: tests.viewmat_util.TAU / TAU_SMALL are 8 x the worst on the whole
  scenes / on their first n rows, rounded up to a power of two)."""
import ctypes
import os
import re

import pytest
import torch

from tests import util as U
from tests import viewmat_util as V
from tests.util import record_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "eg_project_bwd_viewmats"
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
    assert m, f"{name} is not declared in include/edgegs.h"
    out = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        out.append("ptr" if ("*" in a or a.startswith("eg_stream_t")) else a.rsplit(" ", 1)[0])
    return out


def test_entry_is_declared_exported_and_bound(lib):
    declared = _declared_args(ENTRY)
    assert ENTRY in lib.EXPORTS and ENTRY in lib._SIGS
    h = ctypes.CDLL(lib.LIB_PATH)
    assert hasattr(h, ENTRY)
    bound = ["ptr" if (t is ctypes.c_void_p or hasattr(t, "contents")) else CTYPE[t] for t in lib._SIGS[ENTRY]]
    assert bound == declared


def test_bad_arguments_are_rejected_before_any_hip_call(lib):
    """Every call below is invalid, so none of them reaches a launch."""
    h = lib.load(require_device=False)
    buf = (ctypes.c_float * 64)()  # a non-null host address: it is never dereferenced
    q = ctypes.cast(buf, ctypes.c_void_p)
    err = h.eg_last_error_string

    def dense(N=8, C=1, width=32, height=32, nnz=0, splat=q, indptr=None, ids=None, means=q, viewmats=q, g2d=q, v_comps=q,
              scratch=q, blocks=1, out=q):
        return h.eg_project_bwd_viewmats(means, q, q, q, viewmats, q, N, C, width, height, 0.3, 0, splat, indptr, nnz, ids, g2d,
                                         v_comps, None, scratch, blocks, out, None)

    def packed(nnz=4, indptr=q, ids=q, **kw):
        return dense(nnz=nnz, splat=None, indptr=indptr, ids=ids, **kw)

    for f in (dense, packed):
        assert f(C=0) == -1 and ENTRY.encode() in err() and b"bad sizes" in err()
        assert f(C=65536) == -1 and f(C=-3) == -1
        assert f(N=-1) == -1 and ENTRY.encode() in err()
        assert f(width=0) == -1 and f(height=-16) == -1
        assert f(viewmats=None) == -1 and (ENTRY + ": null pointer").encode() in err()
        assert f(out=None) == -1 and f(means=None) == -1 and f(g2d=None) == -1 and f(v_comps=None) == -1
        assert f(scratch=None) == -1 and b"null pointer" in err()
        assert f(blocks=0) == -1 and b"scratch" in err()
    assert packed(nnz=-1) == -1 and ENTRY.encode() in err() and b"nnz" in err()
    assert packed(nnz=9, N=8, C=1) == -1 and b"nnz" in err()     # more pairs than (camera, Gaussian) combinations
    assert packed(indptr=None) == -1 and ENTRY.encode() in err()   # neither layout
    assert packed(ids=None) == -1 and b"null pointer" in err()
    assert dense(nnz=4) == -1 and dense(indptr=q) == -1 and b"not both" in err()
    assert dense(N=600, blocks=2) == -1 and b"scratch" in err()    # 600 Gaussians are three workgroups
    assert packed(N=600, C=2, nnz=700, blocks=2) == -1             # at most min(nnz, N) = 600 pairs per camera


def _fp32_ratios(case):
    """{(cotangent, n): |g32 - g64| / S, worst entry} for the fp32 oracle on every n the device tests use on `case`,
    with the checks on the references themselves on the way."""
    ref = U.projection_reference(case)
    pc = V.pair_contributions(case)
    assert pc["bottom"] == 0.0                                    # autograd's bottom row: exactly zero
    assert torch.equal(pc["vis"], torch.from_numpy(ref["vis"]))   # one Gaussian per call decides as the whole call does
    out = {}
    for cot in ref["cots"]:
        for n in V.case_sizes(case):
            g64, r64 = V.whole_call_gradient(case, cot, n, torch.float64)
            assert not g64[:, 3].any()
            ref64, S = V.reference(case, cot, n)
            assert bool((S > 0).any()), (case, cot, n)
            # the per-pair contributions add up to the whole-call float64 gradient (another summation order: 1e-12 of S)
            whole, nonzero = V.bound_ratio(g64, ref64, S)
            assert whole <= 1e-12 and nonzero == 0, (case, cot, n, whole, nonzero)
            # the fp32 oracle, without the pairs whose cull decision differs between fp32 and float64 (borderline ones)
            r32 = V.whole_call_gradient(case, cot, n, torch.float32)[1]
            drop = ((r32 > 0) != (r64 > 0)).numpy()
            assert not (drop & ~ref["border"][:, :n]).any()
            g32, _ = V.whole_call_gradient(case, cot, n, torch.float32, drop=drop)
            ref64, S = V.reference(case, cot, n, drop=drop)
            assert g32.dtype == torch.float32 and not g32[:, 3].any()
            ratio, nonzero = V.bound_ratio(g32, ref64, S)
            assert nonzero == 0, (case, cot, n)                   # exact zeros where no pair contributes (S == 0)
            out[(cot, n)] = ratio
            if cot == "depths":  # the depth cotangent reaches the third row alone
                assert not S[:, :2].any() and bool(S[:, 2].any())
    return out


def _worst(ratios, whole):
    N = max(n for _cot, n in ratios)
    return max([v for (_cot, n), v in ratios.items() if (n == N) == whole], default=0.0)


@pytest.mark.parametrize("case", V.CASES)
def test_fp32_oracle_stays_within_an_eighth_of_the_bound(case):
    ratios = _fp32_ratios(case)
    whole, part = _worst(ratios, True), _worst(ratios, False)
    print(f"{case}: worst |g32 - g64| / S = {whole:.3e} on the whole scene, {part:.3e} on its first n rows",
          {f"{k[0]}:{k[1]}": f"{v:.2e}" for k, v in ratios.items()})
    record_cpu("viewmat_grad_fp32_oracle", case=case, worst_ratio_whole=whole, worst_ratio_part=part, tau=V.TAU,
               tau_small=V.TAU_SMALL, ratios={f"{k[0]}:{k[1]}": v for k, v in ratios.items()})
    assert whole <= V.TAU / 8, (case, whole)
    assert part <= V.TAU_SMALL / 8, (case, part)


def test_the_bounds_are_the_smallest_powers_of_two_above_eight_oracle_errors():
    assert V.TAU / 2 < 8 * V.FP32_WORST <= V.TAU
    assert V.TAU_SMALL / 2 < 8 * V.FP32_WORST_SMALL <= V.TAU_SMALL
    ratios = [_fp32_ratios(case) for case in V.CASES]
    whole, part = max(_worst(r, True) for r in ratios), max(_worst(r, False) for r in ratios)
    # (the constants are the measured worst ratios, rounded up in the third digit: 6.33e-8 and 2.833e-6)
    assert 0.5 * V.FP32_WORST <= whole <= V.FP32_WORST, whole
    assert 0.5 * V.FP32_WORST_SMALL <= part <= V.FP32_WORST_SMALL, part


@pytest.mark.parametrize("case", V.CASES)
def test_classic_mode_compensation_cotangent_reaches_nothing(case):
    ref64, S = V.reference(case, "compensations", mode="classic")
    assert tuple(ref64.shape) == (len(U.PROJ_CASES[case]["cams"]), 3, 4)
    assert not ref64.any() and not S.any()
