"""The test oracle of the spherical-harmonics colours: the 25 real spherical harmonics of degrees 0..4 in plain torch,
in the dtype of their input (float64 for the reference, float32 to measure what that format alone costs).

Written from the table of real spherical harmonics in Cartesian form (each entry a polynomial in x, y, z and
r^2 = x^2 + y^2 + z^2) times (-1)^m, the 3DGS / gsplat sign convention; index k = l*l + l + m.
tests/test_sh_host.py pins it: orthonormal over the sphere, and the low degrees against their closed forms."""
import math

import torch

PI = math.pi


def sh_basis(d, degree=4):
    """d [..., 3] unit vectors -> [..., (degree + 1)^2]; nothing above `degree` is evaluated."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz = x * x, y * y, z * z
    r2 = xx + yy + zz
    s = math.sqrt
    Y = [0.5 * s(1 / PI) * torch.ones_like(x)]
    Y += [
        # l = 1: m = -1, 0, 1
        -s(3 / (4 * PI)) * y,
        s(3 / (4 * PI)) * z,
        -s(3 / (4 * PI)) * x,
    ] if degree >= 1 else []
    Y += [
        # l = 2: m = -2 .. 2
        0.5 * s(15 / PI) * x * y,
        -0.5 * s(15 / PI) * y * z,
        0.25 * s(5 / PI) * (3 * zz - r2),
        -0.5 * s(15 / PI) * x * z,
        0.25 * s(15 / PI) * (xx - yy),
    ] if degree >= 2 else []
    Y += [
        # l = 3: m = -3 .. 3
        -0.25 * s(35 / (2 * PI)) * y * (3 * xx - yy),
        0.5 * s(105 / PI) * x * y * z,
        -0.25 * s(21 / (2 * PI)) * y * (5 * zz - r2),
        0.25 * s(7 / PI) * z * (5 * zz - 3 * r2),
        -0.25 * s(21 / (2 * PI)) * x * (5 * zz - r2),
        0.25 * s(105 / PI) * (xx - yy) * z,
        -0.25 * s(35 / (2 * PI)) * x * (xx - 3 * yy),
    ] if degree >= 3 else []
    Y += [
        # l = 4: m = -4 .. 4
        0.75 * s(35 / PI) * x * y * (xx - yy),
        -0.75 * s(35 / (2 * PI)) * y * z * (3 * xx - yy),
        0.75 * s(5 / PI) * x * y * (7 * zz - r2),
        -0.75 * s(5 / (2 * PI)) * y * z * (7 * zz - 3 * r2),
        (3 / 16) * s(1 / PI) * (35 * zz * zz - 30 * zz * r2 + 3 * r2 * r2),
        -0.75 * s(5 / (2 * PI)) * x * z * (7 * zz - 3 * r2),
        (3 / 8) * s(5 / PI) * (xx - yy) * (7 * zz - r2),
        -0.75 * s(35 / (2 * PI)) * x * z * (xx - 3 * yy),
        (3 / 16) * s(35 / PI) * (xx * (xx - 3 * yy) - yy * (3 * xx - yy)),
    ] if degree >= 4 else []
    return torch.stack(Y, dim=-1)


def sh_eval(degree, dirs, coeffs, masks=None):
    """gsplat's `spherical_harmonics`: dirs [..., 3] (normalised here), coeffs [..., K, 3], masks [...] bool or None
    -> [..., 3], zero where masked.  Differentiable in dirs and coeffs."""
    ku = (degree + 1) ** 2
    d = dirs / dirs.norm(dim=-1, keepdim=True)
    out = (sh_basis(d, degree)[..., None] * coeffs[..., :ku, :]).sum(-2)
    if masks is not None:
        out = torch.where(masks[..., None], out, torch.zeros_like(out))
    return out
