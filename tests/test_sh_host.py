"""Spherical-harmonics colours without a GPU: the two C entries check their arguments before any HIP call, and the
float64 oracle the GPU tests compare against (tests/sh_oracle.py) is pinned on its own."""
import math

import numpy as np
import pytest
import torch

from tests import sh_oracle


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    return _lib


# degree, K, C, N, dirs, means, campos, coeffs, coeffs_per_camera, masks, clamp
GOOD = dict(degree=2, K=9, C=1, N=4, dirs=None, means=1, campos=1, coeffs=1, cpc=0, masks=None, clamp=1)


def _fwd(h, colors=1, **kw):
    a = {**GOOD, **kw}
    return h.eg_sh_fwd(a["degree"], a["K"], a["C"], a["N"], a["dirs"], a["means"], a["campos"], a["coeffs"], a["cpc"],
                       a["masks"], a["clamp"], colors, None)


def _bwd(h, v_colors=1, v_coeffs=1, v_dirs=None, v_means=None, **kw):
    a = {**GOOD, **kw}
    return h.eg_sh_bwd(a["degree"], a["K"], a["C"], a["N"], a["dirs"], a["means"], a["campos"], a["coeffs"], a["cpc"],
                       a["masks"], a["clamp"], v_colors, v_coeffs, v_dirs, v_means, None)


BAD = {
    "degree_high": dict(degree=5, K=36), "degree_negative": dict(degree=-1), "K_small": dict(degree=3, K=15),
    "C_zero": dict(C=0), "N_negative": dict(N=-1), "null_coeffs": dict(coeffs=None), "flag": dict(cpc=2),
    "null_means": dict(means=None), "null_campos": dict(campos=None), "both_directions": dict(dirs=1),
}


@pytest.mark.parametrize("case", list(BAD) + ["null_colors"])
def test_forward_rejects_bad_arguments(lib, case):
    h = lib.load(require_device=False)
    kw = dict(colors=None) if case == "null_colors" else BAD[case]
    assert _fwd(h, **kw) == -1
    assert b"eg_sh_fwd" in h.eg_last_error_string()


@pytest.mark.parametrize("case", list(BAD) + ["null_v_colors", "null_v_coeffs", "v_dirs_without_dirs",
                                              "v_means_without_means"])
def test_backward_rejects_bad_arguments(lib, case):
    h = lib.load(require_device=False)
    kw = {"null_v_colors": dict(v_colors=None), "null_v_coeffs": dict(v_coeffs=None), "v_dirs_without_dirs": dict(v_dirs=1),
          "v_means_without_means": dict(dirs=1, means=None, campos=None, v_means=1)}.get(case) or BAD[case]
    assert _bwd(h, **kw) == -1
    assert b"eg_sh_bwd" in h.eg_last_error_string()


def test_empty_input_returns_without_a_launch(lib):
    h = lib.load(require_device=False)  # (no device here: a launch would fail)
    assert _fwd(h, N=0) == 0
    assert _bwd(h, N=0, v_means=1) == 0
    assert _fwd(h, N=0, dirs=1, means=None, campos=None, degree=4, K=30, cpc=1, C=3) == 0


def _sphere_quadrature():
    """Gauss-Legendre in cos(theta) (16 nodes) x 32 uniform phi nodes: exact for polynomials of degree <= 31 in
    cos(theta) and trigonometric degree < 32 in phi -- products of two degree-4 harmonics have degree 8."""
    ct, w = np.polynomial.legendre.leggauss(16)
    phi = (np.arange(32) + 0.5) * (2 * math.pi / 32)
    ct, phi = np.meshgrid(ct, phi, indexing="ij")
    st = np.sqrt(1 - ct * ct)
    d = np.stack([st * np.cos(phi), st * np.sin(phi), ct], -1).reshape(-1, 3)
    wt = np.repeat(w[:, None], 32, 1).reshape(-1) * (2 * math.pi / 32)
    return torch.from_numpy(d), torch.from_numpy(wt)


def test_oracle_basis_is_orthonormal():
    d, w = _sphere_quadrature()
    assert abs(float(w.sum()) - 4 * math.pi) < 1e-12
    Y = sh_oracle.sh_basis(d)
    assert Y.dtype == torch.float64 and Y.shape == (512, 25)
    G = (Y * w[:, None]).T @ Y
    assert float((G - torch.eye(25, dtype=torch.float64)).abs().max()) < 1e-12


def test_oracle_low_degrees_sign_and_constant():
    x, y, z = 0.36, 0.48, 0.8  # a unit vector with every product non-zero and xx != yy
    Y = sh_oracle.sh_basis(torch.tensor([x, y, z], dtype=torch.float64)).tolist()
    c1, c2 = 0.4886025119029199, 1.0925484305920792
    want = [0.28209479177387814, -c1 * y, c1 * z, -c1 * x, c2 * x * y, -c2 * y * z,
            0.31539156525252005 * (2 * z * z - x * x - y * y), -c2 * x * z, 0.5462742152960396 * (x * x - y * y)]
    for k, v in enumerate(want):
        assert abs(Y[k] - v) < 1e-15, (k, Y[k], v)


def test_oracle_eval_masks_and_ignores_rows_above_the_degree():
    g = torch.Generator().manual_seed(0)
    dirs = torch.randn(7, 3, generator=g, dtype=torch.float64) * 10
    co = torch.randn(7, 25, 3, generator=g, dtype=torch.float64)
    m = torch.tensor([True, False, True, True, False, True, True])
    a = sh_oracle.sh_eval(2, dirs, co, m)
    b = sh_oracle.sh_eval(2, dirs * 0.01, co[:, :9], None)  # the length of a direction does not matter
    assert torch.equal(a[~m], torch.zeros(2, 3, dtype=torch.float64))
    assert float((a[m] - b[m]).abs().max()) < 1e-13
