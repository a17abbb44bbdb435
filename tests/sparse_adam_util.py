"""torch.optim.SparseAdam's and gsplat's SelectiveAdam's update, stated once in float64, modelled once in fp32, and bounded
element by element -- tests/adam_util.py's scheme for the row update of csrc/adam_sparse.hip (adam_row1).

Both forms step the rows a call names and no others:

    m' = b1 m + (1 - b1) g;   v' = b2 v + (1 - b2) g^2;   p' = p - step m' / (sqrt(v') + eps)

eps is added to the UNCORRECTED root.  SparseAdam: the rows are those of the gradient's index list, g is the sum of a
row's values -- formed in fp32 in the order of the values tensor, first to last, and taken into the float64 reference as
that fp32 number -- and step = lr sqrt(1 - b2^t) / (1 - b1^t).  SelectiveAdam: the rows are those of a bool mask, g is the
dense gradient and step = lr (no bias correction).  Rows that are not named keep p, m and v bit for bit.

Bounds on a named row, with u = 2^-24, S = |b1 m| + |(1 - b1) g|, denom = sqrt(v'_ref) + eps, everything on the right in
float64 (the forms of tests/adam_util.py):

    |m' - m'_ref| <= C_M u S
    |v' - v'_ref| <= C_V u v'_ref
    |p' - p'_ref| <= C_P u (|upd| + step S / denom) + u max(|p|, |p'_ref|)

Exact cases: step == 0 (lr == 0) leaves p bit-identical; S == 0 gives m' == 0; v'_ref == 0 gives v' == 0.  Domain as in
adam_util: every g^2 and v' is 0 or within [1e-30, 1e30].

The constants are measured as adam_util's are: C_M and C_V are 2 x the worst ratio the fp32 model (row_adam32_model: the
kernel's statement order, every operation rounded once, correctly rounded sqrt and reciprocal) shows on
adam_util.designed inputs over MODEL_CASES, rounded up; C_P is the same plus 4 for the kernel's 1-ulp v_sqrt_f32 /
v_rcp_f32 (2 u each on the update).  tests/test_sparse_adam_host.py::test_model_is_within_the_bounds_and_sets_the_constants
asserts that derivation.
"""
import math

import numpy as np

from tests import adam_util as AU

U = AU.U
BETAS, EPS = AU.BETAS, AU.EPS

MODEL_RATIOS = dict(m=2.34, v=3.31, p=2.17)   # worst |error| / (u x scale) of row_adam32_model on MODEL_CASES (asserted to 0.1)
C_M, C_V, C_P = 5, 7, 9                    # ceil(2 x ratio), ceil(2 x ratio), ceil(2 x ratio) + 4
MODEL_N, MODEL_SEED = AU.MODEL_N, AU.MODEL_SEED
# (t, lr, eps); t None = the selective form (step = lr)
MODEL_CASES = [(t, lr, eps) for t in (1, 2, 10, 1000, 100000, None) for lr in (2e-3, 1e-4, 0.03, 0.0) for eps in (1e-8, 1e-6)]


def step_scalar(lr, b1, b2, t):
    """The scalar in front of m' / (sqrt(v') + eps), in double: SparseAdam's at count t, SelectiveAdam's (t None) lr."""
    return lr if t is None else lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


# --------------------------------------------------------------------------------------------- the row update
def row_adam64(p, g, m, v, step, b1, b2, eps):
    """The update of every element in float64 from fp32 inputs: (p', m', v', upd, denom)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v1) + eps
    upd = step * m1 / denom
    return p - upd, m1, v1, upd, denom


def row_adam32_model(p, g, m, v, step, b1, b2, eps, mutant=None, dense_t=None):
    """adam_row1's statements in numpy fp32: host scalars formed in double and cast, sqrt and reciprocal correctly
    rounded.  Returns (p', m', v') fp32.  Mutants: "eps_inside_sqrt"; "dense_denominator" (optim.Adam's
    sqrt(v) / sqrt(1 - b2^t) + eps under lr / (1 - b1^t), t = dense_t)."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    b1f, omb1, b2f, omb2, epsf, stepf = f(b1), f(1.0 - b1), f(b2), f(1.0 - b2), f(eps), f(step)
    with np.errstate(all="ignore"):
        m1 = m * b1f + g * omb1
        v1 = v * b2f + (g * g) * omb2
        if mutant == "eps_inside_sqrt":
            denom = np.sqrt(v1 + epsf)
        elif mutant == "dense_denominator":
            denom = np.sqrt(v1) * f(1.0 / math.sqrt(1.0 - b2 ** dense_t)) + epsf
        else:
            denom = np.sqrt(v1) + epsf
        p1 = p - stepf * (m1 * (f(1.0) / denom))
    return p1.astype(f), m1.astype(f), v1.astype(f)


# --------------------------------------------------------------------------------------------- duplicates
def ordered_sum(idx, vals, N, dtype=np.float32, order="forward"):
    """(G [N, w] of `dtype`, touched [N] bool): per row the sum of its values in the order of the values tensor, every
    addition rounded to `dtype`.  order "reverse" adds last to first, "last" keeps the last value alone (mutants)."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals)
    vals = vals.reshape(idx.size, int(np.prod(vals.shape[1:]))).astype(dtype)
    G = np.zeros((N, vals.shape[1]), dtype=dtype)
    touched = np.zeros(N, dtype=bool)
    if idx.size == 0:
        return G, touched
    touched[idx] = True
    if order == "reverse":
        idx, vals = idx[::-1], vals[::-1]
    perm = np.argsort(idx, kind="stable")
    srt = idx[perm]
    first = np.r_[True, srt[1:] != srt[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(srt.size), 0))
    rank = np.arange(srt.size) - start                      # the k-th occurrence of its row, in tensor order
    for k in range(int(rank.max()) + 1):                    # each pass names a row at most once
        sel = perm[rank == k]
        if order == "last" or k == 0:
            G[idx[sel]] = vals[sel]
        else:
            G[idx[sel]] = (G[idx[sel]] + vals[sel]).astype(dtype)
    return G, touched


# --------------------------------------------------------------------------------------------- float64 references
def _rows(x, N):
    return np.asarray(x).reshape(N, -1)


def _reference(p, G, m, v, touched, step, b1, b2, eps):
    N = touched.size
    p, m, v = (_rows(x, N).astype(np.float64) for x in (p, m, v))
    p1, m1, v1, upd, denom = row_adam64(p, G, m, v, step, b1, b2, eps)
    t = touched[:, None]
    return dict(p=np.where(t, p1, p), m=np.where(t, m1, m), v=np.where(t, v1, v), upd=upd, denom=denom, touched=touched,
                g=np.asarray(G, np.float64), step=step)


def sparse_adam64(p, idx, vals, m, v, lr, b1, b2, eps, t, sum_dtype=np.float32):
    """One torch.optim.SparseAdam step at count t in float64 from the fp32 state; duplicates summed in `sum_dtype` in the
    order of the values tensor first.  Dict of [N, w] arrays p, m, v (untouched rows: the inputs), upd, denom, g, and
    touched [N]."""
    N = np.asarray(p).shape[0]
    G, touched = ordered_sum(idx, vals, N, sum_dtype)
    return _reference(p, G, m, v, touched, step_scalar(lr, b1, b2, t), b1, b2, eps)


def selective_adam64(p, g, m, v, vis, lr, b1, b2, eps):
    """One SelectiveAdam step in float64 from the fp32 state: rows where vis [N] is true, no bias correction."""
    vis = np.asarray(vis, dtype=bool).reshape(-1)
    return _reference(p, _rows(g, vis.size), m, v, vis, lr, b1, b2, eps)


# --------------------------------------------------------------------------------------------- fp32 models
def _model(p, G, m, v, touched, step, b1, b2, eps, mutant, dense_t=None):
    N = touched.size
    p, m, v = (_rows(x, N).astype(np.float32) for x in (p, m, v))
    p1, m1, v1 = row_adam32_model(p, G, m, v, step, b1, b2, eps, mutant, dense_t)
    t = touched[:, None]
    if mutant == "untouched_rows_decay":
        return np.where(t, p1, p), np.where(t, m1, m * np.float32(b1)), np.where(t, v1, v * np.float32(b2))
    return np.where(t, p1, p), np.where(t, m1, m), np.where(t, v1, v)


def sparse_adam32_model(p, idx, vals, m, v, lr, b1, b2, eps, t, mutant=None):
    """The kernel's walk in numpy fp32: ordered fp32 sums of duplicates, then the row update; (p', m', v') [N, w].
    Mutants: those of row_adam32_model, "no_bias_correction", "untouched_rows_decay", "last_value_wins",
    "reverse_order_sum"."""
    N = np.asarray(p).shape[0]
    order = {"last_value_wins": "last", "reverse_order_sum": "reverse"}.get(mutant, "forward")
    G, touched = ordered_sum(idx, vals, N, np.float32, order)
    step = step_scalar(lr, b1, b2, t)
    if mutant == "no_bias_correction":
        step = lr
    if mutant == "dense_denominator":
        step = lr / (1.0 - b1 ** t)
    return _model(p, G, m, v, touched, step, b1, b2, eps, mutant, t)


def selective_adam32_model(p, g, m, v, vis, lr, b1, b2, eps, mutant=None, t=1):
    """Mutant "bias_correction": SparseAdam's scalar at count t in place of lr."""
    vis = np.asarray(vis, dtype=bool).reshape(-1)
    step = step_scalar(lr, b1, b2, t) if mutant == "bias_correction" else lr
    return _model(p, _rows(g, vis.size).astype(np.float32), m, v, vis, step, b1, b2, eps, mutant)


# --------------------------------------------------------------------------------------------- the bounds
def step_ratios(got, p, m, v, ref, b1):
    """got = (p', m', v') fp32 of one step from the fp32 state (p, m, v); ref = sparse_adam64 / selective_adam64 of the
    same state.  {"m", "v", "p"}: the worst error over the NAMED rows in units of u x its scale -- to be held against C_M,
    C_V, C_P -- with the exact cases (rows that are not named, step == 0) folded in as 0 (met) or inf (broken).  Every
    element takes part."""
    touched = ref["touched"]
    N = touched.size
    gp, gm, gv, p, m, v = (_rows(x, N).astype(np.float32) for x in (*got, p, m, v))
    out = {}
    t, r = touched, ~touched
    still = {"p": AU.bits_equal(gp[r], p[r]), "m": AU.bits_equal(gm[r], m[r]), "v": AU.bits_equal(gv[r], v[r])}
    p64, m64 = p[t].astype(np.float64), m[t].astype(np.float64)
    S = np.abs(b1 * m64) + np.abs((1.0 - b1) * ref["g"][t])
    out["m"] = AU.ratio(np.abs(gm[t].astype(np.float64) - ref["m"][t]), S)
    out["v"] = AU.ratio(np.abs(gv[t].astype(np.float64) - ref["v"][t]), ref["v"][t])
    if ref["step"] == 0:
        out["p"] = 0.0 if AU.bits_equal(gp[t], p[t]) else np.inf
    else:
        own = U * np.maximum(np.abs(p64), np.abs(ref["p"][t]))      # the rounding of p' itself
        err = np.maximum(np.abs(gp[t].astype(np.float64) - ref["p"][t]) - own, 0.0)
        out["p"] = AU.ratio(err, np.abs(ref["upd"][t]) + ref["step"] * S / ref["denom"][t])
    return {q: (x if still[q] else np.inf) for q, x in out.items()}


def over_bounds(r):
    """The ratios of step_ratios against the constants, as multiples of the bound (<= 1 passes)."""
    return {"m": r["m"] / C_M, "v": r["v"] / C_V, "p": r["p"] / C_P}


def assert_within(r, label):
    ob = over_bounds(r)
    for q in ("m", "v", "p"):
        assert ob[q] <= 1.0, f"{label}: {q}' at {ob[q]:.3g} x its bound ({r[q]:.3g} u, constant {dict(m=C_M, v=C_V, p=C_P)[q]})"
    return ob


def finite(ob):
    return {k: (float(x) if np.isfinite(x) else "inf") for k, x in ob.items()}
