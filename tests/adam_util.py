"""torch.optim.Adam's update, stated once in float64, modelled once in fp32, and bounded element by element.

adam1 (csrc/project_dev.h) is inlined into seven kernels; tests/test_gpu_adam.py drives each of them and compares every
element of p', m' and v' with `adam64` of the device's own pre-step fp32 state -- a per-step reference: nothing
accumulates.  tests/test_adam_host.py holds `adam64` to torch.optim.Adam in float64, `adam32_model` (a numpy fp32 walk in
adam1's statement order, correctly rounded sqrt and reciprocal) to the bounds, and shows that the bounds reject the
faults they are there for.

Bounds, with u = 2^-24, S = |b1 m| + |(1 - b1) g|, step = lr / (1 - b1^t), everything on the right in float64:

    |m' - m'_ref| <= C_M u S
    |v' - v'_ref| <= C_V u v'_ref
    |p' - p'_ref| <= C_P u (|upd| + step S / denom) + u max(|p|, |p'_ref|)

(m' is a sum of two rounded products that may cancel: its error follows the terms, not the result; the update inherits
that error through step / denom; the last term is the rounding of p' itself.)  Exact cases: a group that does not step is
bit-identical in p, m and v; lr == 0 leaves p bit-identical while m and v obey the bounds; S == 0 gives m' == 0 and
v'_ref == 0 gives v' == 0.  Domain: every g^2 and v' is 0 or within [1e-30, 1e30] -- fp32 denormals and overflow are not
part of the claim.

The constants are measured: C_M and C_V are 2 x the worst ratio the fp32 model shows on the designed inputs, rounded up;
C_P is the same plus 4, for the kernel's 1-ulp v_sqrt_f32 / v_rcp_f32 (2 u each on the update).
tests/test_adam_host.py::test_model_is_within_the_bounds_and_sets_the_constants asserts that derivation.
"""
import math

import numpy as np

U = 2.0 ** -24
GROUPS = ("means", "scales", "quats", "opac")          # eg_adam_hyper's order = the moment blocks' order
GRAD_ORDER = ("means", "quats", "scales", "opac")      # EdgeTrainer.grads' block order
WIDTH = dict(means=3, scales=3, quats=4, opac=1)
BETAS, EPS = (0.9, 0.999), 1e-8

MODEL_RATIOS = dict(m=2.34, v=3.31, p=2.96)   # worst |error| / (u x scale) of adam32_model on MODEL_CASES (asserted to 0.1)
C_M, C_V, C_P = 5, 7, 10                   # ceil(2 x ratio), ceil(2 x ratio), ceil(2 x ratio) + 4
MODEL_N, MODEL_SEED = 22000, 20
MODEL_CASES = [(t, lr, eps) for t in (1, 2, 10, 1000, 100000) for lr in (2e-3, 1e-4, 0.03, 0.0) for eps in (1e-8, 1e-6)]
DOMAIN = (1e-30, 1e30)


# --------------------------------------------------------------------------------------------- inputs
def designed(n, seed, b1=BETAS[0], tame=False):
    """(p, g, m, v) fp32 [n]: |g| log-uniform in 1e-12 .. 1e6 with mixed signs, 1/17 exactly 0; half of the m drawn like g,
    the other half within 1e-3 of -(1 - b1) g / b1 (m' cancels), 1/13 exactly 0; v log-uniform in 1e-24 .. 1e12, 1/11
    exactly 0; rows with m != 0, v == 0 and g == 0 keep |m| <= 1e-9 (a finite update); |p| in 1e-3 .. 1e2.
    tame: v is raised to (|m| / 30)^2 where it is below -- |m| / sqrt(v) <= 30, as in any state Adam itself produced -- for
    the tests whose updated parameters go on into a projection: an update stays within ~40 learning rates."""
    r = np.random.default_rng(seed)
    logu = lambda lo, hi: 10.0 ** r.uniform(lo, hi, n)                  # noqa: E731
    sign = lambda: np.where(r.random(n) < 0.5, -1.0, 1.0)               # noqa: E731
    every = lambda k: (r.permutation(n) + r.integers(k)) % k == 0       # noqa: E731  (1 / k of the elements, at random)
    g = (sign() * logu(-12, 6)).astype(np.float32)
    g[every(17)] = 0.0
    m = sign() * logu(-12, 6)
    cancel = every(2)
    m[cancel] = (-(1.0 - b1) * g.astype(np.float64) / b1 * (1.0 + r.uniform(-1e-3, 1e-3, n)))[cancel]
    m = m.astype(np.float32)
    m[every(13)] = 0.0
    v = logu(-24, 12).astype(np.float32)
    v[every(11)] = 0.0
    bare = (m != 0) & (v == 0) & (g == 0)
    m[bare] = np.sign(m[bare]) * np.minimum(np.abs(m[bare]), np.float32(1e-9))
    if tame:
        v = np.maximum(v, ((m.astype(np.float64) / 30.0) ** 2 * (1.0 + 1e-6)).astype(np.float32))
    p = (sign() * logu(-3, 2)).astype(np.float32)
    return p, g, m, v


def in_domain(g, v_new):
    """Every g^2 and v' (float64) is 0 or within DOMAIN."""
    ok = lambda x: bool(np.all((x == 0) | ((x >= DOMAIN[0]) & (x <= DOMAIN[1]))))  # noqa: E731
    return ok(np.asarray(g, np.float64) ** 2) and ok(np.asarray(v_new, np.float64))


def split(flat, N, order):
    """Flat [11 N] blocks in `order` -> {name: [N, w]} (views)."""
    out, o = {}, 0
    for k in order:
        out[k] = flat[o:o + WIDTH[k] * N].reshape(N, WIDTH[k])
        o += WIDTH[k] * N
    assert o == 11 * N
    return out


def join(d, order):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in order])


# --------------------------------------------------------------------------------------------- float64 reference
def group_counts(step, group_steps):
    """The step count of each of the four optimizers in one call, None = it does not step (eg_adam_hyper.group_steps:
    0 = the shared `step`, > 0 = its own count, < 0 = skipped)."""
    out = []
    for gs in group_steps:
        t = step if gs == 0 else gs
        out.append(int(t) if t > 0 else None)
    return out


def adam64(p, g, m, v, lr, b1, b2, eps, t):
    """One torch.optim.Adam step (no weight decay, no amsgrad) in float64 from the fp32 inputs: (p', m', v', upd, denom)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v1) / math.sqrt(1.0 - b2 ** t) + eps
    upd = lr / (1.0 - b1 ** t) * m1 / denom
    return p - upd, m1, v1, upd, denom


def adam64_groups(P, G, M, V, lrs, b1, b2, eps, step, group_steps):
    """The four optimizers on {name: array} state: {name: (p', m', v', upd, denom) or None for a skipped group}."""
    out = {}
    for k, lr, t in zip(GROUPS, lrs, group_counts(step, group_steps)):
        out[k] = None if t is None else adam64(P[k], G[k], M[k], V[k], lr, b1, b2, eps, t)
    return out


# --------------------------------------------------------------------------------------------- fp32 model
def adam32_model(p, g, m, v, lr, b1, b2, eps, t, mutant=None):
    """adam1's statements in numpy fp32 (every operation rounded once, no contraction): host scalars formed in double
    and cast (make_adamk), sqrt and reciprocal correctly rounded.  Returns (p', m', v') fp32.  `mutant` names a fault."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    tb = t + 1 if mutant == "bias_count_off_by_one" else t
    b1f, omb1, b2f, omb2, epsf = f(b1), f(1.0 - b1), f(b2), f(1.0 - b2), f(eps)
    step_size = f(lr / (1.0 - math.pow(b1, float(tb))))
    inv_bc2_sqrt = f(1.0 / math.sqrt(1.0 - math.pow(b2, float(tb))))
    if mutant == "betas_swapped":
        b1f, omb1 = omb1, b1f
    with np.errstate(all="ignore"):
        m1 = m * b1f + g * omb1
        v1 = v * b2f + (g if mutant == "v_of_g" else g * g) * omb2
        if mutant == "eps_inside_sqrt":
            denom = np.sqrt(v1 + epsf) * inv_bc2_sqrt
        else:
            denom = np.sqrt(v1) * inv_bc2_sqrt + epsf
        p1 = p - step_size * (m1 * (f(1.0) / denom))
    return p1.astype(f), m1.astype(f), v1.astype(f)


def adam32_model_groups(P, G, m_flat, v_flat, lrs, b1, b2, eps, step, group_steps, mutant=None):
    """The 11 N form as the kernels see it: parameters and gradients per tensor, moments as flat [3N | 3N | 4N | N]
    blocks.  Returns ({name: p'}, m_flat', v_flat')."""
    N = P["means"].shape[0]
    lrs, counts = list(lrs), group_counts(step, group_steps)
    order = GROUPS
    if mutant == "moment_blocks_swapped":
        order = ("means", "quats", "scales", "opac")
    if mutant == "lrs_swapped":
        lrs[1], lrs[2] = lrs[2], lrs[1]
    m_flat, v_flat = m_flat.copy(), v_flat.copy()
    Mv, Vv = split(m_flat, N, order), split(v_flat, N, order)
    out = {}
    for i, k in enumerate(GROUPS):
        t = counts[i]
        if mutant == "lr_zero_skips" and lrs[i] == 0:
            t = None
        if t is None:
            out[k] = P[k].copy()
            if mutant == "skipped_group_advances_m":
                Mv[k][...] = adam32_model(P[k], G[k], Mv[k], Vv[k], lrs[i], b1, b2, eps, 1)[1]
            continue
        out[k], m1, v1 = adam32_model(P[k], G[k], Mv[k].copy(), Vv[k].copy(), lrs[i], b1, b2, eps, t, mutant)
        Mv[k][...], Vv[k][...] = m1, v1
    return out, m_flat, v_flat


# --------------------------------------------------------------------------------------------- the bounds
def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def ratio(err, scale):
    """max err / (u scale) over the elements; an element whose scale is 0 must be exact; NaN counts as infinite."""
    err, scale = np.asarray(err, np.float64).reshape(-1), np.asarray(scale, np.float64).reshape(-1)
    if err.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        r = np.where(scale > 0, err / (U * np.where(scale > 0, scale, 1.0)), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def step_ratios(got, p, g, m, v, lr, b1, b2, eps, t):
    """got = (p', m', v') fp32 of one optimizer's step from the fp32 state (p, g, m, v); t None: the group did not step.
    Returns {"m", "v", "p"}: the worst error of each tensor in units of u x its scale -- to be held against C_M, C_V, C_P --
    with the exact cases folded in as 0 (met) or inf (broken).  Every element takes part."""
    gp, gm, gv = (np.asarray(x, dtype=np.float32) for x in got)
    if t is None:
        return {"m": 0.0 if bits_equal(gm, m) else np.inf, "v": 0.0 if bits_equal(gv, v) else np.inf,
                "p": 0.0 if bits_equal(gp, p) else np.inf}
    p1, m1, v1, upd, denom = adam64(p, g, m, v, lr, b1, b2, eps, t)
    p64, g64, m64 = (np.asarray(x, np.float64) for x in (p, g, m))
    S = np.abs(b1 * m64) + np.abs((1.0 - b1) * g64)
    out = {"m": ratio(np.abs(gm.astype(np.float64) - m1), S), "v": ratio(np.abs(gv.astype(np.float64) - v1), v1)}
    if lr == 0:
        out["p"] = 0.0 if bits_equal(gp, p) else np.inf
    else:
        own = U * np.maximum(np.abs(p64), np.abs(p1))      # the rounding of p' itself
        err = np.maximum(np.abs(gp.astype(np.float64) - p1) - own, 0.0)
        out["p"] = ratio(err, np.abs(upd) + lr / (1.0 - b1 ** t) * S / denom)
    return out


def over_bounds(r):
    """The ratios of step_ratios against the constants: {"m", "v", "p"} as multiples of the bound (<= 1 passes)."""
    return {"m": r["m"] / C_M, "v": r["v"] / C_V, "p": r["p"] / C_P}


def groups_ratios(got_P, got_m, got_v, P, G, m_flat, v_flat, lrs, b1, b2, eps, step, group_steps):
    """step_ratios for each optimizer of an 11 N step: {name: {"m", "v", "p"}}; moments in the flat block layout."""
    N = P["means"].shape[0]
    Mg, Vg, M0, V0 = (split(np.asarray(x, np.float32), N, GROUPS) for x in (got_m, got_v, m_flat, v_flat))
    return {k: step_ratios((got_P[k], Mg[k], Vg[k]), P[k], G[k], M0[k], V0[k], lr, b1, b2, eps, t)
            for k, lr, t in zip(GROUPS, lrs, group_counts(step, group_steps))}


def worst(per_group):
    """{name: {"m","v","p"}} -> {"m","v","p"} maxima."""
    return {q: max(r[q] for r in per_group.values()) for q in ("m", "v", "p")}


def assert_within(per_group, label):
    """Every tensor of every optimizer within its bound; returns the worst multiples of the bound per tensor kind."""
    for k, r in per_group.items():
        ob = over_bounds(r)
        for q in ("m", "v", "p"):
            assert ob[q] <= 1.0, f"{label}: {k} {q}' at {ob[q]:.3g} x its bound ({r[q]:.3g} u, constant {dict(m=C_M, v=C_V, p=C_P)[q]})"
    return over_bounds(worst(per_group))


def designed_groups(N, seed, tame=False):
    """Designed inputs of an 11 N step: ({name: p}, {name: g}, m_flat, v_flat), moments in [3N | 3N | 4N | N]."""
    p, g, m, v = designed(11 * N, seed, tame=tame)
    return ({k: a.copy() for k, a in split(p, N, GROUPS).items()}, {k: a.copy() for k, a in split(g, N, GROUPS).items()},
            m, v)
