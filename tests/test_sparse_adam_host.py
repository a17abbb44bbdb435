"""SparseAdam and SelectiveAdam on the CPU: the float64 statements, the fp32 model and the bounds of
tests/sparse_adam_util.py, the classes' constructor surface, and the two C entries' argument checks.

sparse_adam64 is held to torch.optim.SparseAdam in float64; row_adam32_model (adam_row1's statement order in numpy fp32)
stays within the bounds on adam_util's designed inputs, which is where C_M, C_V and C_P come from; every mutant -- the
faults the device tests of tests/test_gpu_sparse_adam.py are there to catch -- exceeds a bound."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import adam_util as AU
from tests import sparse_adam_util as SU
from tests.util import record_cpu

B1, B2 = SU.BETAS
SHAPES = {"1": (), "3": (3,), "4": (4,), "9x3": (9, 3)}


def three_runs(N, rng, share=0.7):
    """Three ascending runs, each over `share` of the rows: the index list of a packed three-camera call."""
    return np.concatenate([np.sort(rng.choice(N, max(1, int(share * N)), replace=False)) for _ in range(3)])


# ============================================================================================= 1: reference against torch
@pytest.mark.parametrize("width", list(SHAPES))
def test_sparse_adam64_matches_torch_sparse_adam_in_float64(width):
    """Six steps, another index set in each: unique sorted, three ascending runs, shuffled with duplicates, EMPTY,
    a single row, three runs again; float64 sums of duplicates on both sides.  p, exp_avg, exp_avg_sq to 1e-13 relative,
    rows outside a step's index list exactly equal before and after."""
    rng = np.random.default_rng(5)
    N, dense = 61, SHAPES[width]
    w = int(np.prod(dense)) if dense else 1
    ref = torch.nn.Parameter(torch.from_numpy(rng.standard_normal((N,) + dense)))
    opt = torch.optim.SparseAdam([ref], lr=2e-3, betas=(B1, B2), eps=1e-8)
    p, m, v = ref.detach().numpy().reshape(N, w).copy(), np.zeros((N, w)), np.zeros((N, w))
    lists = [np.sort(rng.choice(N, 20, replace=False)), three_runs(N, rng), rng.integers(0, N, 90),
             np.zeros(0, dtype=np.int64), np.array([17]), three_runs(N, rng)]
    for t, idx in enumerate(lists, start=1):
        vals = rng.standard_normal((idx.size,) + dense) * 10.0 ** rng.integers(-4, 2)
        ref.grad = torch.sparse_coo_tensor(torch.from_numpy(idx)[None], torch.from_numpy(vals), size=(N,) + dense)
        st = opt.state[ref]
        before = {"p": ref.detach().numpy().reshape(N, w).copy(),
                  "exp_avg": st["exp_avg"].numpy().reshape(N, w).copy() if st else np.zeros((N, w)),
                  "exp_avg_sq": st["exp_avg_sq"].numpy().reshape(N, w).copy() if st else np.zeros((N, w))}
        opt.step()
        out = SU.sparse_adam64(p, idx, vals, m, v, 2e-3, B1, B2, 1e-8, t, sum_dtype=np.float64)
        away = ~out["touched"]
        assert away.sum() == N - np.unique(idx).size
        for name, old, new in (("p", p, out["p"]), ("m", m, out["m"]), ("v", v, out["v"])):
            assert np.array_equal(old[away], new[away]), (t, name)
        p, m, v = out["p"], out["m"], out["v"]
        st = opt.state[ref]
        assert st["step"] == t   # (also for the empty gradient)
        for name, mine, theirs in (("p", p, ref.detach()), ("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"])):
            theirs = theirs.numpy().reshape(N, w)
            err = np.abs(mine - theirs).max() / np.abs(theirs).max()
            assert err <= 1e-13, (t, name, err)
            assert np.array_equal(theirs[away], before[name][away]), (t, name)   # torch leaves them alone too


def test_ordered_sum_adds_in_tensor_order_in_fp32():
    idx = np.array([4, 2, 4, 4, 2, 0])
    vals = np.array([1.0, 3.0, 1e8, -1e8, 0.5, 7.0], dtype=np.float32)[:, None]
    G, touched = SU.ordered_sum(idx, vals, 6)
    assert touched.tolist() == [True, False, True, False, True, False]
    assert G[:, 0].tolist() == [7.0, 0.0, 3.5, 0.0, 0.0, 0.0]          # (1 + 1e8) - 1e8 = 0 in fp32
    assert SU.ordered_sum(idx, vals, 6, order="reverse")[0][4, 0] == 1.0     # (-1e8 + 1e8) + 1
    assert SU.ordered_sum(idx, vals, 6, order="last")[0][:, 0].tolist() == [7.0, 0.0, 0.5, 0.0, -1e8, 0.0]
    assert SU.ordered_sum(idx, vals, 6, np.float64)[0][4, 0] == 1.0


def test_selective_adam64_steps_the_visible_rows_without_bias_correction():
    p, g, m, v = (x.reshape(50, 4) for x in AU.designed(200, 3, tame=True))
    vis = np.arange(50) % 3 == 0
    out = SU.selective_adam64(p, g, m, v, vis, 1e-3, B1, B2, 1e-8)
    assert np.array_equal(out["p"][~vis], p[~vis]) and np.array_equal(out["m"][~vis], m[~vis])
    m1 = B1 * m.astype(np.float64) + (1 - B1) * g.astype(np.float64)
    v1 = B2 * v.astype(np.float64) + (1 - B2) * g.astype(np.float64) ** 2
    want = p.astype(np.float64) - 1e-3 * m1 / (np.sqrt(v1) + 1e-8)
    assert np.allclose(out["p"][vis], want[vis], rtol=1e-13, atol=0) and out["step"] == 1e-3


# ============================================================================================= 2: the fp32 model
def _model_ratios():
    p, g, m, v = AU.designed(SU.MODEL_N, SU.MODEL_SEED)
    N = p.size
    everything = np.ones(N, dtype=bool)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for t, lr, eps in SU.MODEL_CASES:
        if t is None:
            ref = SU.selective_adam64(p, g, m, v, everything, lr, B1, B2, eps)
            got = SU.selective_adam32_model(p, g, m, v, everything, lr, B1, B2, eps)
        else:
            ref = SU.sparse_adam64(p, np.arange(N), g, m, v, lr, B1, B2, eps, t)
            got = SU.sparse_adam32_model(p, np.arange(N), g, m, v, lr, B1, B2, eps, t)
        r = SU.step_ratios(got, p, m, v, ref, B1)
        worst = {q: max(worst[q], r[q]) for q in worst}
    return worst


def test_model_is_within_the_bounds_and_sets_the_constants():
    """row_adam32_model against the float64 statement on adam_util's designed inputs, t in {1, 2, 10, 1000, 100000} and
    the selective form x lr in {2e-3, 1e-4, 0.03, 0} x eps in {1e-8, 1e-6}: the constants are 2 x the worst ratio rounded
    up (C_P: + 4 for the 1-ulp sqrt and reciprocal)."""
    w = _model_ratios()
    record_cpu("sparse_adam_model_ratios", model=w, constants=dict(C_M=SU.C_M, C_V=SU.C_V, C_P=SU.C_P), elements=SU.MODEL_N,
               cases=len(SU.MODEL_CASES))
    print("row_adam32_model worst ratios (u x scale):", w)
    for q in w:
        assert abs(w[q] - SU.MODEL_RATIOS[q]) <= 0.1, (q, w[q], SU.MODEL_RATIOS[q])
    assert SU.C_M == math.ceil(2 * w["m"]) and SU.C_V == math.ceil(2 * w["v"]) and SU.C_P == math.ceil(2 * w["p"]) + 4
    assert max(SU.over_bounds(w).values()) <= 0.5 + 1e-9


def sparse_case(N=700, w=3, seed=8, kind="runs"):
    """Designed state [N, w] and an index list with duplicates; the values are designed gradients, so the sums are too."""
    rng = np.random.default_rng(seed)
    p, g, m, v = (x.reshape(N, w) for x in AU.designed(N * w, seed))
    idx = three_runs(N, rng) if kind == "runs" else rng.integers(0, N, 2 * N)
    vals = (g[idx] * rng.uniform(0.5, 2.0, (idx.size, 1))).astype(np.float32)
    return p, m, v, idx, vals


@pytest.mark.parametrize("kind", ("runs", "shuffled"))
def test_model_with_duplicates_is_within_the_bounds(kind):
    p, m, v, idx, vals = sparse_case(kind=kind)
    assert np.unique(idx).size < idx.size and np.unique(idx).size < p.shape[0]
    for t, lr in ((1, 2e-3), (10, 0.03), (1000, 0.0)):
        ref = SU.sparse_adam64(p, idx, vals, m, v, lr, B1, B2, 1e-8, t)
        got = SU.sparse_adam32_model(p, idx, vals, m, v, lr, B1, B2, 1e-8, t)
        ob = SU.assert_within(SU.step_ratios(got, p, m, v, ref, B1), f"model {kind} t={t}")
        assert max(ob.values()) <= 0.5 + 1e-9


def test_exact_cases_are_reported_as_infinite_when_broken():
    p, m, v, idx, vals = sparse_case()
    ref = SU.sparse_adam64(p, idx, vals, m, v, 0.0, B1, B2, 1e-8, 10)
    got = SU.sparse_adam32_model(p, idx, vals, m, v, 0.0, B1, B2, 1e-8, 10)
    assert AU.bits_equal(got[0], p) and max(SU.step_ratios(got, p, m, v, ref, B1).values()) < np.inf
    away = int(np.flatnonzero(~ref["touched"])[0])
    near = int(np.flatnonzero(ref["touched"])[0])
    for row, q, k in ((away, "p", 0), (away, "m", 1), (away, "v", 2), (near, "p", 0)):
        bad = [x.copy() for x in got]
        bad[k][row, 1] = np.nextafter(bad[k][row, 1], np.float32(np.inf))
        assert SU.step_ratios(bad, p, m, v, ref, B1)[q] == np.inf, (row, q)


def small_v_case(N=600, w=3, seed=12):
    """sqrt(v') around 1e-10, two orders below eps = 1e-8: where eps sits decides the update."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.5, 2.0, (N, w)).astype(np.float32)
    m = (rng.uniform(1e-11, 1e-9, (N, w)) * rng.choice([-1.0, 1.0], (N, w))).astype(np.float32)
    v = rng.uniform(1e-21, 1e-19, (N, w)).astype(np.float32)
    idx = np.sort(rng.choice(N, N // 2, replace=False))
    vals = (rng.uniform(1e-11, 1e-9, (idx.size, w)) * rng.choice([-1.0, 1.0], (idx.size, w))).astype(np.float32)
    return p, m, v, idx, vals


def order_case(N=300, w=3, seed=13):
    """Every named row three times with values (a, 1e8 a, -1e8 a): first to last the fp32 sum is 0, last to first a."""
    rng = np.random.default_rng(seed)
    p, _, m, v = (x.reshape(N, w) for x in AU.designed(N * w, seed, tame=True))
    rows = np.sort(rng.choice(N, N // 2, replace=False))
    a = rng.uniform(0.5, 2.0, (rows.size, w)).astype(np.float32)
    big = (a * np.float32(2.0 ** 27)).astype(np.float32)
    idx = np.concatenate([rows, rows, rows])
    vals = np.concatenate([a, big, -big])
    fwd, rev = SU.ordered_sum(idx, vals, N)[0], SU.ordered_sum(idx, vals, N, order="reverse")[0]
    assert not np.array_equal(fwd, rev) and (fwd[rows] == 0).all() and np.array_equal(rev[rows], a)
    return p, m, v, idx, vals


SPARSE_MUTANTS = [("eps_inside_sqrt", sparse_case, 10), ("dense_denominator", small_v_case, 10),
                  ("no_bias_correction", sparse_case, 10), ("untouched_rows_decay", sparse_case, 10),
                  ("last_value_wins", sparse_case, 10), ("reverse_order_sum", order_case, 10)]


@pytest.mark.parametrize("mutant,case,t", SPARSE_MUTANTS, ids=[x[0] for x in SPARSE_MUTANTS])
def test_a_sparse_mutant_exceeds_a_bound(mutant, case, t):
    p, m, v, idx, vals = case()
    lr = 2e-3
    ref = SU.sparse_adam64(p, idx, vals, m, v, lr, B1, B2, 1e-8, t)
    sound = SU.over_bounds(SU.step_ratios(SU.sparse_adam32_model(p, idx, vals, m, v, lr, B1, B2, 1e-8, t), p, m, v, ref, B1))
    assert max(sound.values()) <= 1.0, sound
    ob = SU.over_bounds(SU.step_ratios(SU.sparse_adam32_model(p, idx, vals, m, v, lr, B1, B2, 1e-8, t, mutant), p, m, v, ref, B1))
    record_cpu("sparse_adam_mutant", mutant=mutant, over_bounds=SU.finite(ob))
    assert max(ob.values()) > 1.0, f"{mutant} passes every bound: {ob}"


@pytest.mark.parametrize("mutant", ("bias_correction", "untouched_rows_decay", "eps_inside_sqrt"))
def test_a_selective_mutant_exceeds_a_bound(mutant):
    N, w = 500, 4
    p, g, m, v = (x.reshape(N, w) for x in AU.designed(N * w, 21))
    vis = np.random.default_rng(2).random(N) < 0.5
    ref = SU.selective_adam64(p, g, m, v, vis, 2e-3, B1, B2, 1e-8)
    sound = SU.over_bounds(SU.step_ratios(SU.selective_adam32_model(p, g, m, v, vis, 2e-3, B1, B2, 1e-8), p, m, v, ref, B1))
    assert max(sound.values()) <= 1.0, sound
    got = SU.selective_adam32_model(p, g, m, v, vis, 2e-3, B1, B2, 1e-8, mutant, t=1000)
    ob = SU.over_bounds(SU.step_ratios(got, p, m, v, ref, B1))
    record_cpu("selective_adam_mutant", mutant=mutant, over_bounds=SU.finite(ob))
    assert max(ob.values()) > 1.0, f"{mutant} passes every bound: {ob}"


# ============================================================================================= 3: constructor surface
def test_constructor_surface_and_schedulers():
    from edgegaussians_amd.optim import SelectiveAdam, SparseAdam
    p = torch.nn.Parameter(torch.zeros(8, 3))
    o = SparseAdam([p])
    t = torch.optim.SparseAdam([torch.nn.Parameter(torch.zeros(8, 3))])
    assert isinstance(o, torch.optim.Optimizer)
    assert {k: v for k, v in o.param_groups[0].items() if k != "params"} == {k: v for k, v in t.param_groups[0].items() if k != "params"}
    assert o.param_groups[0]["params"][0] is p and len(o.state) == 0
    assert o.state_dict()["param_groups"] == t.state_dict()["param_groups"]
    o.load_state_dict(t.state_dict())
    t.load_state_dict(o.state_dict())
    o = SparseAdam([p], lr=2e-3)
    sch = torch.optim.lr_scheduler.MultiStepLR(o, milestones=[1], gamma=0.1)
    with pytest.warns(UserWarning):  # (torch's own warning: scheduler stepped before the optimizer)
        sch.step()
    assert abs(o.param_groups[0]["lr"] - 2e-4) < 1e-12
    s = SelectiveAdam([{"params": [p], "lr": 1e-2}], eps=1e-15, betas=(0.9, 0.999))
    assert isinstance(s, torch.optim.Optimizer)
    g = s.param_groups[0]
    assert g["lr"] == 1e-2 and g["eps"] == 1e-15 and tuple(g["betas"]) == (0.9, 0.999)
    assert SelectiveAdam([p], 1e-8, (0.9, 0.999), lr=3e-3).param_groups[0]["lr"] == 3e-3
    sch = torch.optim.lr_scheduler.MultiStepLR(s, milestones=[1], gamma=0.1)
    with pytest.warns(UserWarning):
        sch.step()
    assert abs(s.param_groups[0]["lr"] - 1e-3) < 1e-12
    assert SparseAdam.step.hooked and SelectiveAdam.step.hooked


def test_unsupported_options_raise():
    from edgegaussians_amd.optim import SelectiveAdam, SparseAdam
    p = torch.nn.Parameter(torch.zeros(8, 3))
    with pytest.raises(NotImplementedError):
        SparseAdam([p], maximize=True)
    with pytest.raises(NotImplementedError):
        SparseAdam([p], lr=torch.tensor(1e-3))
    for bad in (dict(lr=-1.0), dict(lr=0.0), dict(eps=0.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0))):  # torch's own
        with pytest.raises(ValueError):
            SparseAdam([p], **bad)
        with pytest.raises(ValueError):
            torch.optim.SparseAdam([p], **bad)
    for o, args in ((SparseAdam([p]), ()), (SelectiveAdam([p], 1e-8, (0.9, 0.999)), (torch.ones(8, dtype=torch.bool),))):
        with pytest.raises(NotImplementedError):
            o.step(*args, closure=lambda: 0.0)
        with pytest.raises(NotImplementedError):
            o.register_step_pre_hook(lambda *a: None)
        with pytest.raises(NotImplementedError):
            o.register_step_post_hook(lambda *a: None)
    with pytest.raises(NotImplementedError):
        SelectiveAdam([p], 1e-8, (0.9, 0.999), lr=torch.tensor(1e-3))


def test_the_gsplat_shim_exports_the_packages_class():
    from gsplat.optimizers import SelectiveAdam
    import edgegaussians_amd.optim
    assert SelectiveAdam is edgegaussians_amd.optim.SelectiveAdam


def sparse_grad(N=5, w=3):
    return torch.sparse_coo_tensor(torch.tensor([[1, 3, 3]]), torch.ones(3, w), size=(N, w))


def test_zero_grad_semantics():
    from edgegaussians_amd.optim import SparseAdam
    p = torch.nn.Parameter(torch.zeros(5, 3))
    o = SparseAdam([p])
    p.grad = sparse_grad()
    o.zero_grad(set_to_none=False)
    assert p.grad is not None and p.grad.is_sparse and p.grad._nnz() == 0 and p.grad.shape == (5, 3)
    ref = torch.nn.Parameter(torch.zeros(5, 3))
    ref.grad = sparse_grad()
    torch.optim.SparseAdam([ref]).zero_grad(set_to_none=False)
    assert ref.grad.is_sparse and ref.grad._nnz() == 0     # torch does the same
    p.grad = sparse_grad()
    o.zero_grad()
    assert p.grad is None


# ============================================================================================= 4: no GPU
@pytest.mark.skipif(torch.cuda.is_available(), reason="the loud failure is the no-GPU behaviour")
def test_step_without_the_hip_library_raises():
    from edgegaussians_amd.optim import SelectiveAdam, SparseAdam
    p = torch.nn.Parameter(torch.zeros(5, 3))
    o = SparseAdam([p])
    p.grad = sparse_grad()
    with pytest.raises(RuntimeError):
        o.step()
    assert float(p.detach().abs().sum()) == 0.0 and len(o.state) == 0  # nothing was updated by some fallback
    s = SelectiveAdam([p], 1e-8, (0.9, 0.999))
    p.grad = torch.ones(5, 3)
    with pytest.raises(RuntimeError):
        s.step(torch.ones(5, dtype=torch.bool))
    assert float(p.detach().abs().sum()) == 0.0 and len(s.state) == 0


# ============================================================================================= 5: the two entries
@pytest.fixture(scope="module")
def h():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    return _lib.load(require_device=False)


def test_sparse_rows_entry_checks_its_arguments(h):
    """Sizes first, `nothing to do` next, then the pointers one by one, by name -- all before any device call (the
    non-null stand-ins below are host addresses that are never handed to a kernel: the last pointer stays null)."""
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    hyper = (1e-3, 0.9, 0.999, 1e-8)

    def call(ptrs, nnz=4, N=8, w=3, step=1):
        return h.eg_adam_sparse_rows(*ptrs, nnz, N, w, *hyper, step, None)

    for kw in (dict(nnz=-1), dict(N=-1), dict(w=0), dict(w=-3), dict(step=0), dict(nnz=2 ** 31 // 3, w=3)):
        assert call([None] * 6, **kw) == -1, kw
        assert b"eg_adam_sparse_rows" in h.eg_last_error_string()
    assert call([None] * 6, nnz=0) == 0 and call([None] * 6, N=0) == 0     # nothing to do: EG_OK without a launch
    names = ("param", "exp_avg", "exp_avg_sq", "values", "sorted_indices")
    for k, name in enumerate(names):
        assert call([a] * k + [None] * (6 - k)) == -1
        msg = h.eg_last_error_string()
        assert name.encode() + b" is null" in msg, (name, msg)


def test_masked_rows_entry_checks_its_arguments(h):
    buf = ctypes.create_string_buffer(64)
    a = ctypes.addressof(buf)
    hyper = (1e-3, 0.9, 0.999, 1e-8)

    def call(ptrs, N=8, M=3):
        return h.eg_adam_masked_rows(*ptrs, N, M, *hyper, None)

    for kw in (dict(N=-1), dict(M=0), dict(M=-1), dict(N=2 ** 31 // 4, M=4)):
        assert call([None] * 5, **kw) == -1, kw
        assert b"eg_adam_masked_rows" in h.eg_last_error_string()
    assert call([None] * 5, N=0) == 0
    for k, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq", "visibility")):
        assert call([a] * k + [None] * (5 - k)) == -1
        msg = h.eg_last_error_string()
        assert name.encode() + b" is null" in msg, (name, msg)
