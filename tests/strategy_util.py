"""Float64 statements, numpy-fp32 models and error bounds for edgegaussians_amd/strategy and relocation.py
(tests/test_strategy_host.py holds them to each other on the CPU, tests/test_gpu_strategy.py holds the kernels to them).

Statements (`*64`): the issue's formulas in float64 on numpy arrays, the random draws passed in.
Models (`*32_model`): the kernels' statement order (csrc/strategy.hip) in numpy float32, with named mutants -- the faults
the device tests are there to catch.
Bounds: derived from the formulas in units of U = 2^-24 (half an fp32 ulp at 1), never from a kernel's output.  Each has
ONE calibrated constant, fixed here as 4 x the largest ratio the fp32 MODEL shows against float64 on the test inputs of
this file (the measured ratio stands next to it; test_strategy_host.py re-measures it and fails if 4 x it exceeds the
constant).
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
N_MAX = 51
EPS32 = float(np.finfo(np.float32).eps)
F32_MIN = float(np.finfo(np.float32).tiny)  # 2^-126: below it the gate of the noise flushes or loses bits

# ---- calibrated constants (4 x measured, rounded up to an integer) -----------------------------------------------
C_RELOC = 5    # measured on relocation_inputs(): 1.02 (the |dx| / U term; the den term stays below 0: T kappa covers it)
K_NOISE = 267  # measured on noise_inputs(), scaler 1: 66.6 (the gate: its exponent carries 100 x the rounding of 1 - sigmoid)
C_STATS = 2    # measured on stats_inputs(): -1.2, i.e. the C additions alone cover every row; 2 is the derived worst case
               # of a term's own roundings ((C - 1) additions + 3 U per term), which is what stands here


def binoms64(n_max: int = N_MAX) -> np.ndarray:
    b = np.zeros((n_max, n_max))
    for n in range(n_max):
        for k in range(n + 1):
            b[n, k] = math.comb(n, k)
    return b


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def logit(p):
    return np.log(p / (1.0 - p))


# ==================================================================================================== compute_relocation
def relocation_inputs(seed: int = 0, N: int = 4096 + 37):
    """The GPU test's rows: opacities {0.005, 0.01, 0.1, 0.5, 0.9, 0.99} and U(0.005, 0.99); every ratio 1 .. 51 against
    every fixed opacity, then 0, -3 and 60 (the clamps), then random pairs.  fp32 opacities / scales, int64 ratios."""
    rng = np.random.default_rng(seed)
    fixed = np.array([0.005, 0.01, 0.1, 0.5, 0.9, 0.99])
    o = np.concatenate([np.repeat(fixed, N_MAX), fixed, fixed, fixed])
    r = np.concatenate([np.tile(np.arange(1, N_MAX + 1), fixed.size), np.full(6, 0), np.full(6, -3), np.full(6, 60)])
    n_rand = N - o.size
    o = np.concatenate([o, rng.uniform(0.005, 0.99, n_rand)])
    r = np.concatenate([r, rng.integers(1, N_MAX + 1, n_rand)])
    scales = np.exp(rng.uniform(-6.0, 0.0, (N, 3)))
    return o.astype(np.float32), scales.astype(np.float32), r.astype(np.int64)


def relocation_inputs_near_one(seed: int = 1):
    """The second, small set: opacities up to 1 - 1e-6, where kappa reaches ~1e4."""
    rng = np.random.default_rng(seed)
    o = 1.0 - 10.0 ** -np.repeat(np.array([2.5, 3.0, 4.0, 5.0, 6.0]), 8)
    r = np.tile(np.array([1, 2, 3, 7, 20, 35, 50, 51]), 5)
    scales = np.exp(rng.uniform(-6.0, 0.0, (o.size, 3)))
    return o.astype(np.float32), scales.astype(np.float32), r.astype(np.int64)


def relocation64(opacities, scales, ratios, binoms):
    """x, den, new_scales in float64, with T = r (r + 1) / 2 and kappa = sum |t| / |sum t| of the double sum."""
    o = np.asarray(opacities, dtype=np.float64)
    s = np.asarray(scales, dtype=np.float64)
    b = np.asarray(binoms, dtype=np.float64)
    n_max = b.shape[0]
    r = np.clip(np.asarray(ratios, dtype=np.int64), 1, n_max)
    x = 1.0 - (1.0 - o) ** (1.0 / r)
    den, mag = np.zeros_like(o), np.zeros_like(o)
    for i in range(1, n_max + 1):
        active = r >= i
        if not active.any():
            break
        for k in range(i):
            t = np.where(active, b[i - 1, k] * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1), 0.0)
            den += t
            mag += np.abs(t)
    return {"r": r, "x": x, "den": den, "new_scales": (o / den)[:, None] * s, "T": r * (r + 1) // 2,
            "kappa": mag / np.abs(den)}


def relocation32_model(opacities, scales, ratios, binoms, mutant=None):
    """compute_relocation_kernel's statement order in numpy fp32.  Mutants: "binoms_row" reads binoms[i, k] for
    binoms[i-1, k]; "no_sqrt" divides by (k + 1) for sqrt(k + 1)."""
    f = np.float32
    o, s, b = np.asarray(opacities, dtype=f), np.asarray(scales, dtype=f), np.asarray(binoms, dtype=f)
    n_max = b.shape[0]
    r = np.clip(np.asarray(ratios, dtype=np.int64), 1, n_max)
    x = (f(1) - np.power(f(1) - o, f(1) / r.astype(f), dtype=f)).astype(f)
    den = np.zeros_like(o)
    for i in range(1, n_max + 1):
        active = r >= i
        if not active.any():
            break
        row = b[min(i, n_max - 1)] if mutant == "binoms_row" else b[i - 1]
        xp, sign = x.copy(), f(1)
        for k in range(i):
            d = f(k + 1) if mutant == "no_sqrt" else np.sqrt(f(k + 1))
            term = ((row[k] * sign) * xp / d).astype(f)
            den = np.where(active, (den + term).astype(f), den)
            xp = (xp * x).astype(f)
            sign = -sign
    c = (o / den).astype(f)
    return {"x": x, "den": den, "new_scales": (c[:, None] * s).astype(f)}


def relocation_bounds(ref, c: float = C_RELOC):
    """|dx| <= c U absolute (x = 1 - y with y <= 1: the rounding of 1 / r, of the power and of the subtraction are each at
    most ~U in y).  den: T terms added one after the other cost at most T U sum|t| = T kappa U |den|, each term's own
    roundings (product, running power, root, division) c U |t|, and dx moves the leading term r x by c U / x relative:
    rel(den) <= ((T + c) kappa + c / x) U.  new_scales = (o / den) s adds one division and one product: + c U."""
    rel_den = ((ref["T"] + c) * ref["kappa"] + c / ref["x"]) * U
    return {"x": np.full_like(ref["x"], c * U), "den_rel": rel_den, "scales_rel": rel_den + c * U}


def relocation_ratio(model, ref):
    """The largest c a row of `model` needs (<= 0 for the den term where T kappa alone covers the row)."""
    need_x = np.abs(model["x"].astype(np.float64) - ref["x"]) / U
    rel = np.abs(model["den"].astype(np.float64) - ref["den"]) / np.abs(ref["den"])
    need_den = (rel / U - ref["T"] * ref["kappa"]) / (ref["kappa"] + 1.0 / ref["x"])
    return float(max(need_x.max(), need_den.max()))


def relocation_excess(out_x, out_scales, ref, scales, c: float = C_RELOC):
    """Per row: the largest error / bound of x and of the three new scales (<= 1 passes), and the relative bound."""
    bd = relocation_bounds(ref, c)
    ex = np.abs(np.asarray(out_x, dtype=np.float64) - ref["x"]) / bd["x"]
    es = np.abs(np.asarray(out_scales, dtype=np.float64) - ref["new_scales"]) / (bd["scales_rel"][:, None] * np.abs(ref["new_scales"]))
    return np.maximum(ex, es.max(axis=1)), bd["scales_rel"]


# ============================================================================================== inject_noise_to_position
def noise_inputs(seed: int = 2, N: int = 1000 + 19):
    """Unnormalised quats scaled by U(0.1, 10), log-scales U(-6, 0), logits on both sides of the gate at opacity 0.005
    (logit(0.005) = -5.29), means N(0, 1), the draw z.  All fp32."""
    rng = np.random.default_rng(seed)
    quats = rng.standard_normal((N, 4)) * rng.uniform(0.1, 10.0, (N, 1))
    log_scales = rng.uniform(-6.0, 0.0, (N, 3))
    logits = np.concatenate([rng.uniform(-5.6, -5.0, N // 2), rng.uniform(-9.0, 4.0, N - N // 2)])
    means = rng.standard_normal((N, 3))
    z = rng.standard_normal((N, 3))
    return tuple(a.astype(np.float32) for a in (means, quats, log_scales, logits, z))


def _rot(q, xp=np.float64):
    q = q.astype(xp)
    n = np.sqrt((q * q).sum(-1, keepdims=True, dtype=xp)).astype(xp)
    w, x, y, z = ((q / n).astype(xp)[:, i] for i in range(4))
    one, two = xp(1), xp(2)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                  two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                  two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=-1)
    return R.reshape(-1, 3, 3).astype(xp)


def noise64(means, quats, log_scales, logits, z, scaler, slope=100.0):
    """New means in float64, and what the bound needs: mag[n, i] = sum_j |Sigma_ij z_j g scaler| and the same sum
    without the gate (for the fp32 floor of the gate)."""
    m, ls, lo, zz = (np.asarray(a, dtype=np.float64) for a in (means, log_scales, logits, z))
    R = _rot(np.asarray(quats))
    s2 = np.exp(ls) ** 2
    cov = np.einsum("nik,nk,njk->nij", R, s2, R)
    g = 1.0 / (1.0 + np.exp(-slope * ((1.0 - sigmoid(lo)) - 0.995)))
    v = zz * g[:, None] * scaler
    ungated = np.einsum("nij,nj->ni", np.abs(cov), np.abs(zz) * abs(scaler))
    return {"means": m + np.einsum("nij,nj->ni", cov, v), "mag": ungated * g[:, None], "ungated": ungated, "gate": g}


def noise32_model(means, quats, log_scales, logits, z, scaler, mutant=None):
    """inject_noise_kernel's statement order in numpy fp32.  Mutants: "RSRt" forms R diag(s) R^T for R diag(s^2) R^T;
    "slope10" gives the gate a slope of 10 for 100."""
    f = np.float32
    m, ls, lo, zz = (np.asarray(a, dtype=f) for a in (means, log_scales, logits, z))
    R = _rot(np.asarray(quats, dtype=f), f)
    s = np.exp(ls).astype(f)
    M = (R * (np.sqrt(s) if mutant == "RSRt" else s)[:, None, :]).astype(f)
    cov = np.zeros((m.shape[0], 3, 3), dtype=f)
    for i in range(3):
        for j in range(3):
            cov[:, i, j] = ((M[:, i, 0] * M[:, j, 0] + M[:, i, 1] * M[:, j, 1]).astype(f) + M[:, i, 2] * M[:, j, 2]).astype(f)
    opac = (f(1) / (f(1) + np.exp(-lo).astype(f))).astype(f)
    slope = f(10) if mutant == "slope10" else f(100)
    with np.errstate(over="ignore"):
        gate = (f(1) / (f(1) + np.exp((-slope * ((f(1) - opac) - f(0.995))).astype(f)).astype(f))).astype(f)
    v = ((zz * gate[:, None]).astype(f) * f(scaler)).astype(f)
    out = np.empty_like(m)
    for i in range(3):
        out[:, i] = m[:, i] + ((cov[:, i, 0] * v[:, 0] + cov[:, i, 1] * v[:, 1]).astype(f) + cov[:, i, 2] * v[:, 2]).astype(f)
    return out.astype(f)


def noise_bound(ref, K: float = K_NOISE):
    """Per entry: K U sum_j |Sigma_ij z_j g scaler| for the roundings of the rotation, the covariance, the gate and the
    three products; U |mean| for the final addition; and 2^-126 sum_j |Sigma_ij z_j scaler|: below the smallest normal
    fp32 the gate itself (down to e^-99.5 = 6e-44 for opaque Gaussians) is flushed or loses its bits."""
    return K * U * ref["mag"] + U * np.abs(ref["means"]) + F32_MIN * ref["ungated"]


def noise_ratio(out, ref):
    """The largest K a row of `out` needs."""
    err = np.abs(np.asarray(out, dtype=np.float64) - ref["means"]) - U * np.abs(ref["means"]) - F32_MIN * ref["ungated"]
    return float((err / (U * ref["mag"])).max())


def noise_excess(out, ref, K: float = K_NOISE):
    return np.abs(np.asarray(out, dtype=np.float64) - ref["means"]) / noise_bound(ref, K)


# ================================================================================================ running statistics
def stats_inputs(seed: int = 3, C: int = 3, N: int = 300):
    """Dense gradients [C,N,2] over six decades and radii [C,N] with culled pairs (0) -- a stand-in for a rasterization
    call's (the device test takes them from a real call)."""
    rng = np.random.default_rng(seed)
    grads = rng.standard_normal((C, N, 2)) * 10.0 ** rng.uniform(-7, -1, (C, N, 1))
    radii = rng.integers(1, 40, (C, N))
    radii[rng.random((C, N)) < 0.3] = 0
    return grads.astype(np.float32), radii.astype(np.int32)


def stats64(grads, radii, width, height, n_cameras, grad2d=None, count=None, radii_state=None):
    """The dense state update in float64: (grad2d, count, radii_state) [N]."""
    g, r = np.asarray(grads, dtype=np.float64), np.asarray(radii)
    N = g.shape[1]
    grad2d = np.zeros(N) if grad2d is None else np.asarray(grad2d, dtype=np.float64).copy()
    count = np.zeros(N) if count is None else np.asarray(count, dtype=np.float64).copy()
    rs = np.zeros(N) if radii_state is None else np.asarray(radii_state, dtype=np.float64).copy()
    vis = r > 0
    norm = np.sqrt((g[..., 0] * (width / 2.0 * n_cameras)) ** 2 + (g[..., 1] * (height / 2.0 * n_cameras)) ** 2)
    grad2d += np.where(vis, norm, 0.0).sum(0)
    count += vis.sum(0)
    rs = np.maximum(rs, np.where(vis, r / float(max(width, height)), 0.0).max(0))
    return grad2d, count, rs


def packed_to_dense(grads, radii, gaussian_ids, camera_ids, C, N):
    """Scatters packed pairs into the dense layout (absent pairs: radius 0)."""
    g, r = np.zeros((C, N, 2), dtype=np.asarray(grads).dtype), np.zeros((C, N), dtype=np.int32)
    g[camera_ids, gaussian_ids] = grads
    r[camera_ids, gaussian_ids] = radii
    return g, r


def stats32_model(grads, radii, width, height, n_cameras, mutant=None):
    """strategy_update_kernel's statement order in numpy fp32 from a zero state.  Mutants: "no_C" scales by W / 2 without
    the number of cameras; "ge0" takes radii >= 0 for radii > 0."""
    f = np.float32
    g, r = np.asarray(grads, dtype=f), np.asarray(radii)
    C, N = r.shape
    k = 1 if mutant == "no_C" else n_cameras
    sx, sy, md = f(width / 2.0 * k), f(height / 2.0 * k), f(max(width, height))
    grad2d, count, rs = np.zeros(N, dtype=f), np.zeros(N, dtype=f), np.zeros(N, dtype=f)
    for c in range(C):
        vis = (r[c] >= 0) if mutant == "ge0" else (r[c] > 0)
        a, b = (g[c, :, 0] * sx).astype(f), (g[c, :, 1] * sy).astype(f)
        n = np.sqrt(((a * a).astype(f) + (b * b).astype(f)).astype(f)).astype(f)
        grad2d = np.where(vis, (grad2d + n).astype(f), grad2d)
        count = np.where(vis, count + f(1), count)
        rs = np.where(vis, np.maximum(rs, (r[c].astype(f) / md).astype(f)), rs)
    return grad2d, count, rs


def stats_bound_rel(n_added: int, c: float = C_STATS):
    """A sum of `n_added` non-negative terms added one after the other: n_added U for the additions, c U for the terms'
    own roundings (two products, two squares, one addition, one root): relative, kappa = 1.  The count is exact (small
    integers); radii / max_dim is one division, inside the same c U."""
    return (n_added + c) * U


def stats_ratio(model_grad2d, ref_grad2d, n_added):
    ok = ref_grad2d > 0
    rel = np.abs(np.asarray(model_grad2d, dtype=np.float64)[ok] - ref_grad2d[ok]) / ref_grad2d[ok]
    return float((rel / U - n_added).max())


# ========================================================================================================= the torch ops
def quat_rot64(quats):
    return _rot(np.asarray(quats, dtype=np.float64))


def duplicate64(P, sel):
    return {k: np.concatenate([v, v[sel]]) for k, v in P.items()}


def remove64(P, keep):
    return {k: v[keep] for k, v in P.items()}


def reset_opa64(P, value):
    out = dict(P)
    out["opacities"] = np.minimum(P["opacities"], logit(value))
    return out


def split64(P, sel, rest, z, revised_opacity=False):
    """`split` on a dict of float64 arrays with the draw z [2, n_sel, 3]."""
    s = np.exp(P["scales"][sel])
    R = quat_rot64(P["quats"][sel])
    samples = np.einsum("nij,nj,bnj->bni", R, s, np.asarray(z, dtype=np.float64))
    out = {}
    for name, p in P.items():
        if name == "means":
            new = (p[sel][None] + samples).reshape(-1, 3)
        elif name == "scales":
            new = np.tile(np.log(s / 1.6), (2, 1))
        elif name == "opacities" and revised_opacity:
            new = np.tile(logit(1.0 - np.sqrt(1.0 - sigmoid(p[sel]))), 2)
        else:
            new = np.concatenate([p[sel], p[sel]])
        out[name] = np.concatenate([p[rest], new])
    return out


def relocation_update64(P, sampled, binoms, min_opacity):
    o = sigmoid(P["opacities"])
    ratios = np.bincount(sampled, minlength=o.shape[0])[sampled] + 1
    ref = relocation64(o[sampled], np.exp(P["scales"])[sampled], ratios, binoms)
    new_o = np.clip(ref["x"], min_opacity, 1.0 - EPS32)
    return logit(new_o), np.log(ref["new_scales"]), ref


def relocate64(P, dead, sampled, binoms, min_opacity=0.005):
    """`relocate` on a dict of float64 arrays with the draw `sampled` (row indices, one per dead row)."""
    lo, ls, ref = relocation_update64(P, sampled, binoms, min_opacity)
    out = {k: v.copy() for k, v in P.items()}
    out["opacities"][sampled] = lo
    out["scales"][sampled] = ls
    for k in out:
        out[k][dead] = out[k][sampled]
    return out, ref


def sample_add64(P, sampled, binoms, min_opacity=0.005):
    lo, ls, ref = relocation_update64(P, sampled, binoms, min_opacity)
    out = {k: v.copy() for k, v in P.items()}
    out["opacities"][sampled] = lo
    out["scales"][sampled] = ls
    return {k: np.concatenate([v, v[sampled]]) for k, v in out.items()}, ref
