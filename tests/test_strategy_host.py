"""gsplat's densification strategies on the CPU: the float64 statements, fp32 models, bounds and mutants of
tests/strategy_util.py; the torch ops (duplicate, remove, split, reset_opa, _update_param_with_optimizer) on CPU tensors
with a stepped torch.optim.Adam; the schedules of DefaultStrategy and MCMCStrategy with the ops replaced by recorders;
check_sanity, defaults, exports, the C entries' argument checks and the refusals of the kernel-backed functions."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import strategy_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B32 = SU.binoms64().astype(np.float32)


# ============================================================================================= bounds, models, mutants
@pytest.fixture(scope="module")
def reloc():
    o, s, r = SU.relocation_inputs()
    return o, s, r, SU.relocation64(o, s, r, B32)


def test_relocation_inputs_cover_what_the_device_test_needs(reloc):
    o, s, r, ref = reloc
    assert o.size == 4096 + 37
    for fixed in (0.005, 0.01, 0.1, 0.5, 0.9, 0.99):
        rows = o == np.float32(fixed)
        assert set(range(1, 52)) <= set(r[rows].tolist())
    assert {0, -3, 60} <= set(r.tolist())
    assert ref["r"].min() == 1 and ref["r"].max() == 51
    # the clamps: 0 and -3 are r = 1 (x = o, den = x, scales unchanged), 60 is r = 51
    low = r <= 0
    assert np.allclose(ref["x"][low], o[low].astype(np.float64), rtol=1e-15)
    assert np.allclose(ref["new_scales"][low], s[low].astype(np.float64), rtol=1e-12)
    assert ref["kappa"].max() <= 24.0     # (o <= 0.99, every r <= 51)
    # no row of this set may be left out: the derived bound stays below 1e-2 everywhere (float64 alone shows it)
    assert (SU.relocation_bounds(ref)["scales_rel"] <= 1e-2).all()


def test_relocation_statement_special_cases():
    b = SU.binoms64()
    assert b[0, 0] == 1 and b[4, 2] == 6 and b[50, 25] == math.comb(50, 25) and b[3, 4] == 0
    # r = 1: den = x = o; r = 2: x = 1 - sqrt(1 - o), den = 2 x - x^2 / sqrt 2
    ref = SU.relocation64(np.array([0.36, 0.36]), np.ones((2, 3)), np.array([1, 2]), b)
    assert abs(ref["x"][1] - 0.2) < 1e-15 and abs(ref["den"][1] - (0.4 - 0.04 / math.sqrt(2))) < 1e-15
    assert abs(ref["den"][0] - 0.36) < 1e-15 and ref["T"].tolist() == [1, 3]


def test_relocation_model_inside_bound_and_constant_is_four_times_measured(reloc):
    o, s, r, ref = reloc
    m = SU.relocation32_model(o, s, r, B32)
    ratio = SU.relocation_ratio(m, ref)
    assert 4.0 * ratio <= SU.C_RELOC <= math.ceil(4.0 * ratio) + 1, ratio
    excess, _ = SU.relocation_excess(m["x"], m["new_scales"], ref, s)
    assert excess.max() <= 1.0, excess.max()


@pytest.mark.parametrize("mutant", ["binoms_row", "no_sqrt"])
def test_relocation_mutants_exceed_the_bound_tenfold(reloc, mutant):
    o, s, r, ref = reloc
    m = SU.relocation32_model(o, s, r, B32, mutant)
    excess, _ = SU.relocation_excess(m["x"], m["new_scales"], ref, s)
    assert excess.max() >= 10.0, excess.max()


def test_relocation_near_one_kappa_and_model():
    o, s, r = SU.relocation_inputs_near_one()
    ref = SU.relocation64(o, s, r, B32)
    assert 5e3 <= ref["kappa"].max() <= 2e4     # (~9e3 at o = 1 - 1e-6, r = 51)
    m = SU.relocation32_model(o, s, r, B32)
    excess, _ = SU.relocation_excess(m["x"], m["new_scales"], ref, s)
    assert excess.max() <= 1.0 and np.isfinite(m["new_scales"]).all() and (m["new_scales"] > 0).all()


@pytest.fixture(scope="module")
def noise():
    a = SU.noise_inputs()
    return a, SU.noise64(*a, 1.0)


def test_noise_inputs_span_the_gate(noise):
    a, ref = noise
    assert a[0].shape == (1019, 3)
    op = SU.sigmoid(a[3].astype(np.float64))
    assert (op < 0.005).sum() > 100 and (op > 0.005).sum() > 100
    assert ref["gate"].min() < 1e-30 and ref["gate"].max() > 0.5
    n = np.linalg.norm(a[1], axis=1)
    assert n.min() < 0.5 and n.max() > 5.0     # unnormalised


def test_noise_model_inside_bound_and_constant_is_four_times_measured(noise):
    a, ref = noise
    m = SU.noise32_model(*a, 1.0)
    ratio = SU.noise_ratio(m, ref)
    assert 4.0 * ratio <= SU.K_NOISE <= math.ceil(4.0 * ratio) + 1, ratio
    assert SU.noise_excess(m, ref).max() <= 1.0


@pytest.mark.parametrize("mutant", ["RSRt", "slope10"])
def test_noise_mutants_exceed_the_bound_tenfold(noise, mutant):
    a, ref = noise
    assert SU.noise_excess(SU.noise32_model(*a, 1.0, mutant), ref).max() >= 10.0


def test_stats_model_inside_bound_and_mutants_outside():
    g, rad = SU.stats_inputs()
    W, H, C = 64, 48, 3
    ref = SU.stats64(g, rad, W, H, C)
    m = SU.stats32_model(g, rad, W, H, C)
    assert 4.0 * SU.stats_ratio(m[0], ref[0], C) <= SU.C_STATS
    ok = ref[0] > 0
    assert (np.abs(m[0][ok] - ref[0][ok]) <= SU.stats_bound_rel(C) * ref[0][ok]).all()
    assert np.array_equal(m[0][~ok], ref[0][~ok]) and np.array_equal(m[1], ref[1])
    assert (np.abs(m[2] - ref[2]) <= SU.stats_bound_rel(0) * ref[2]).all()
    no_c = SU.stats32_model(g, rad, W, H, C, "no_C")
    assert (np.abs(no_c[0][ok] - ref[0][ok]) / (SU.stats_bound_rel(C) * ref[0][ok])).max() >= 10.0
    ge0 = SU.stats32_model(g, rad, W, H, C, "ge0")
    assert np.abs(ge0[1] - ref[1]).max() >= 1.0     # (the count is exact: any difference is outside)
    # the packed layout scatters back to the dense one
    cam, gid = np.nonzero(rad > 0)
    gd, rd = SU.packed_to_dense(g[cam, gid], rad[cam, gid], gid, cam, C, rad.shape[1])
    assert np.array_equal(rd, rad) and np.array_equal(gd[rad > 0], g[rad > 0])


# =========================================================================================== the torch ops on the CPU
def make_params(N=23, seed=0, device="cpu", extra=True):
    g = torch.Generator().manual_seed(seed)
    p = {"means": torch.randn(N, 3, generator=g), "scales": torch.rand(N, 3, generator=g) * 3 - 4,
         "quats": torch.randn(N, 4, generator=g) * 3, "opacities": torch.randn(N, generator=g) * 2}
    if extra:
        p["sh0"] = torch.rand(N, 1, 3, generator=g)
    return {k: torch.nn.Parameter(v.to(device)) for k, v in p.items()}


def stepped(params, cls=torch.optim.Adam, seed=1, **kw):
    """One optimizer per key after ONE real step: non-zero moments."""
    opts = {k: cls([p], lr=1e-2, **kw) for k, p in params.items()}
    g = torch.Generator().manual_seed(seed)
    for k, p in params.items():
        p.grad = torch.randn(p.shape, generator=g).to(p.device)
        opts[k].step()
        p.grad = None
    return opts


def snapshot(params, opts):
    return ({k: v.detach().clone() for k, v in params.items()},
            {k: {n: (t.clone() if isinstance(t, torch.Tensor) else t) for n, t in o.state[params[k]].items()}
             for k, o in opts.items()})


def check_keyed_on_new(params, opts, old_params, N_new):
    for k, o in opts.items():
        p = params[k]
        assert isinstance(p, torch.nn.Parameter) and p.is_leaf and p.requires_grad and p.shape[0] == N_new
        assert len(o.param_groups) == 1 and len(o.param_groups[0]["params"]) == 1 and o.param_groups[0]["params"][0] is p
        assert list(o.state.keys()) == [p]
        assert all(q is not p for q in old_params.values())
        st = o.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert float(st["step"]) == 1.0


def test_update_param_with_optimizer_contract():
    from edgegaussians_amd.strategy.ops import _update_param_with_optimizer
    params = make_params()
    opts = stepped(params)
    fresh = torch.optim.Adam([params["sh0"]], lr=1e-2)     # no state yet
    opts["sh0"] = fresh
    p0, s0 = snapshot(params, {k: o for k, o in opts.items() if k != "sh0"})
    seen = []

    def param_fn(name, p):
        return torch.nn.Parameter(p * 2, requires_grad=p.requires_grad)

    def opt_fn(key, v):
        seen.append(key)
        return v + 1

    _update_param_with_optimizer(param_fn, opt_fn, params, opts, names=["means", "sh0"])
    assert sorted(seen) == ["exp_avg", "exp_avg_sq"]     # never "step"
    assert torch.equal(params["means"], p0["means"] * 2) and torch.equal(params["scales"], p0["scales"])
    st = opts["means"].state[params["means"]]
    assert torch.equal(st["exp_avg"], s0["means"]["exp_avg"] + 1) and float(st["step"]) == 1.0
    assert list(opts["means"].state.keys()) == [params["means"]]
    assert len(fresh.state) == 0 and fresh.param_groups[0]["params"][0] is params["sh0"]     # stays without state
    assert opts["scales"].param_groups[0]["params"][0] is params["scales"]     # untouched names keep theirs


def test_duplicate_remove_reset_on_cpu():
    from edgegaussians_amd.strategy import ops
    params = make_params()
    opts = stepped(params)
    N = 23
    state = {"grad2d": torch.arange(N, dtype=torch.float32), "count": torch.ones(N), "scene_scale": 2.0}
    p0, s0 = snapshot(params, opts)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[[2, 5, 22]] = True
    ops.duplicate(params, opts, state, mask)
    check_keyed_on_new(params, opts, p0, N + 3)
    ref = SU.duplicate64({k: v.double().numpy() for k, v in p0.items()}, np.array([2, 5, 22]))
    assert all(np.array_equal(params[k].detach().double().numpy(), ref[k]) for k in params)
    for k in params:
        assert torch.equal(params[k][:N], p0[k]) and torch.equal(params[k][N:], p0[k][[2, 5, 22]]), k
        st = opts[k].state[params[k]]
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(st[m][:N], s0[k][m]) and not st[m][N:].any() and s0[k][m].any(), (k, m)
    assert torch.equal(state["grad2d"], torch.cat([torch.arange(N, dtype=torch.float32), torch.tensor([2., 5., 22.])]))
    assert state["scene_scale"] == 2.0 and state["count"].shape == (N + 3,)
    # remove: the kept rows bit for bit
    p1, s1 = snapshot(params, opts)
    mask = torch.zeros(N + 3, dtype=torch.bool)
    mask[[0, 7, N + 1]] = True
    keep = torch.where(~mask)[0]
    ops.remove(params, opts, state, mask)
    check_keyed_on_new(params, opts, p1, N)
    ref = SU.remove64({k: v.double().numpy() for k, v in p1.items()}, keep.numpy())
    assert all(np.array_equal(params[k].detach().double().numpy(), ref[k]) for k in params)
    for k in params:
        assert torch.equal(params[k], p1[k][keep]), k
        assert torch.equal(opts[k].state[params[k]]["exp_avg_sq"], s1[k]["exp_avg_sq"][keep]), k
    assert state["grad2d"].shape == (N,)
    # reset_opa: clamp from above, that optimizer's moments zeroed, the others untouched
    p2, s2 = snapshot(params, opts)
    ops.reset_opa(params, opts, state, value=0.25)
    lim = math.log(0.25 / 0.75)
    assert torch.allclose(params["opacities"], p2["opacities"].clamp(max=lim), rtol=0, atol=1e-6)
    assert (p2["opacities"] > lim).any() and (p2["opacities"] < lim).any()
    ref = SU.reset_opa64({k: v.double().numpy() for k, v in p2.items()}, 0.25)
    assert all(np.allclose(params[k].detach().double().numpy(), ref[k], rtol=0, atol=1e-6) for k in params)
    st = opts["opacities"].state[params["opacities"]]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and float(st["step"]) == 1.0
    assert opts["opacities"].param_groups[0]["params"][0] is params["opacities"]
    assert params["means"] is not None and torch.equal(opts["means"].state[params["means"]]["exp_avg"], s2["means"]["exp_avg"])
    # the next optimizer step works on the new leaves
    for k, p in params.items():
        p.grad = torch.ones_like(p)
        opts[k].step()
        assert float(opts[k].state[p]["step"]) == 2.0


@pytest.mark.parametrize("revised", [False, True])
def test_split_matches_its_float64_statement_under_the_same_draw(revised):
    from edgegaussians_amd.strategy import ops
    params = make_params()
    opts = stepped(params)
    N = 23
    state = {"grad2d": torch.arange(N, dtype=torch.float32), "scene_scale": 1.0}
    p0, s0 = snapshot(params, opts)
    mask = torch.zeros(N, dtype=torch.bool)
    mask[[1, 4, 9, 20]] = True
    sel, rest = torch.where(mask)[0].numpy(), torch.where(~mask)[0].numpy()
    torch.manual_seed(77)
    z = torch.randn(2, 4, 3)
    after_draw = torch.rand(1)
    torch.manual_seed(77)
    ops.split(params, opts, state, mask, revised_opacity=revised)
    assert torch.equal(torch.rand(1), after_draw)     # exactly ONE randn(2, n_sel, 3) was drawn
    ref = SU.split64({k: v.double().numpy() for k, v in p0.items()}, sel, rest, z.numpy(), revised)
    check_keyed_on_new(params, opts, p0, N - 4 + 8)
    for k in params:
        got = params[k].detach().double().numpy()
        assert np.array_equal(got[:N - 4], p0[k].double().numpy()[rest]), k     # kept rows bit for bit
        assert np.allclose(got, ref[k], rtol=2e-6, atol=2e-6), k
        st = opts[k].state[params[k]]
        assert torch.equal(st["exp_avg"][:N - 4], s0[k]["exp_avg"][rest]) and not st["exp_avg"][N - 4:].any()
    if not revised:     # copied keys are copies: [copy 0 of all selected | copy 1 of all selected]
        assert torch.equal(params["opacities"][N - 4:], p0["opacities"][sel].repeat(2))
    else:
        assert (params["opacities"][N - 4:] < p0["opacities"][sel].repeat(2)).all()
    assert torch.equal(params["sh0"][N - 4:], p0["sh0"][sel].repeat(2, 1, 1))
    assert torch.equal(state["grad2d"][N - 4:], torch.tensor([1., 4., 9., 20.]).repeat(2))
    # the two copies of a row differ (two draws), and the means moved by at most a few sigma
    assert not torch.equal(params["means"][N - 4:N], params["means"][N:])


# ======================================================================================================== the schedules
class Recorder:
    def __init__(self, monkeypatch, mod):
        self.log = []
        for name in ("duplicate", "split", "remove", "reset_opa", "relocate", "sample_add", "inject_noise_to_position",
                     "_update_grad_stats"):
            monkeypatch.setattr(mod, name, self._make(name))
        self.step = None

    def _make(self, name):
        def f(*a, **k):
            self.log.append((self.step, name))
        return f

    def steps(self, name):
        return [s for s, n in self.log if n == name]


class FakeMeans2d:
    grad = torch.zeros(1, 4, 2)
    absgrad = torch.zeros(1, 4, 2)
    retained = 0

    def retain_grad(self):
        self.retained += 1


def tiny_params():
    return {"means": torch.nn.Parameter(torch.zeros(4, 3)), "scales": torch.nn.Parameter(torch.zeros(4, 3)),
            "quats": torch.nn.Parameter(torch.ones(4, 4)), "opacities": torch.nn.Parameter(torch.zeros(4))}


def test_default_strategy_schedule(monkeypatch):
    import edgegaussians_amd.strategy as S
    rec = Recorder(monkeypatch, S)
    grown, pruned = [], []
    monkeypatch.setattr(S.DefaultStrategy, "_grow_gs", lambda self, p, o, st, step: (grown.append(step), (0, 0))[1])
    monkeypatch.setattr(S.DefaultStrategy, "_prune_gs", lambda self, p, o, st, step: (pruned.append(step), 0)[1])
    strat = S.DefaultStrategy(refine_start_iter=4, refine_every=3, reset_every=12, refine_stop_iter=31,
                              pause_refine_after_reset=2)
    state = strat.initialize_state()
    assert state == {"grad2d": None, "count": None, "scene_scale": 1.0}
    m2d = FakeMeans2d()
    info = {"means2d": m2d, "width": 8, "height": 8, "n_cameras": 1, "radii": torch.ones(1, 4, dtype=torch.int32),
            "gaussian_ids": None}
    params = tiny_params()
    for step in range(41):
        rec.step = step
        strat.step_pre_backward(params, {}, state, step, info)
        strat.step_post_backward(params, {}, state, step, info)
    assert m2d.retained == 41
    assert rec.steps("_update_grad_stats") == list(range(31))     # returns at once from refine_stop_iter on
    # step > 4, step % 3 == 0, step % 12 >= 2, step < 31: 6, 9, 15, 18, 21, 27, 30 (12, 24 paused: 12 % 12 = 0 < 2)
    assert grown == [6, 9, 15, 18, 21, 27, 30] and pruned == grown
    assert rec.steps("reset_opa") == [0, 12, 24]     # (36 is past refine_stop_iter)
    assert state["grad2d"].shape == (4,) and state["count"].shape == (4,) and "radii" not in state
    # without the pause, the reset steps refine too; refine happens before the reset
    rec.log.clear(), grown.clear()
    strat = S.DefaultStrategy(refine_start_iter=4, refine_every=3, reset_every=12, refine_stop_iter=31)
    state = strat.initialize_state()
    for step in range(41):
        rec.step = step
        strat.step_post_backward(params, {}, state, step, info)
    assert grown == [6, 9, 12, 15, 18, 21, 24, 27, 30]
    st = S.DefaultStrategy(refine_scale2d_stop_iter=5).initialize_state(scene_scale=3.0)
    assert st == {"grad2d": None, "count": None, "scene_scale": 3.0, "radii": None}


def test_default_strategy_grow_and_prune_masks_on_cpu(monkeypatch):
    """_grow_gs / _prune_gs with the real torch ops on CPU state: duplicate first, the duplicates are not split, prune by
    opacity, by 3-D scale only after the first reset, by screen radius only before refine_scale2d_stop_iter."""
    import edgegaussians_amd.strategy as S
    N = 6
    params = make_params(N, extra=False)
    with torch.no_grad():
        params["scales"].copy_(torch.log(torch.tensor([[.001] * 3, [.001] * 3, [.5] * 3, [.5] * 3, [.001] * 3, [.02] * 3])))
        params["opacities"].copy_(torch.tensor([2., 2., 2., 2., -8., 2.]))
    opts = stepped(params)
    strat = S.DefaultStrategy(refine_scale2d_stop_iter=100)
    state = {"grad2d": torch.tensor([1., 0., 1., 0., 0., 0.]), "count": torch.tensor([2., 0., 1., 1., 0., 1.]),
             "radii": torch.tensor([0., 0., 0., 0., 0., 0.2]), "scene_scale": 1.0}
    torch.manual_seed(0)
    assert strat._grow_gs(params, opts, state, step=50) == (1, 2)     # row 0 duplicated; rows 2 (grad) and 5 (radius) split
    assert len(params["means"]) == 6 + 1 - 2 + 4 and state["grad2d"].shape == (9,)
    assert strat._prune_gs(params, opts, state, step=50) == 1     # only the transparent row: step <= reset_every
    assert len(params["means"]) == 8
    n_big = int((torch.exp(params["scales"]).max(-1).values > 0.1).sum())
    n_wide = int((state["radii"] > 0.15).sum())
    assert n_big == 3 and n_wide == 2     # row 3 and the halves of row 2 (0.5 / 1.6); the halves of row 5 keep its radius
    assert strat._prune_gs(params, opts, state, step=3050) == n_big     # past refine_scale2d_stop_iter: 3-D only
    assert S.DefaultStrategy(refine_scale2d_stop_iter=10 ** 6)._prune_gs(params, opts, state, step=3050) == n_wide


def test_mcmc_strategy_schedule(monkeypatch):
    import edgegaussians_amd.strategy as S
    rec = Recorder(monkeypatch, S)
    strat = S.MCMCStrategy(refine_start_iter=5, refine_every=4, refine_stop_iter=30, cap_max=50)
    state = strat.initialize_state()
    b = state["binoms"]
    assert b.shape == (51, 51) and b.dtype == torch.float32
    assert torch.equal(b, torch.from_numpy(SU.binoms64().astype(np.float32)))
    params = make_params(40, extra=False)     # int(1.05 * 40) = 42: two rows to add at every refinement (the recorder adds none)
    with torch.no_grad():
        params["opacities"][1] = -20.0     # one dead row
    for step in range(41):
        rec.step = step
        strat.step_post_backward(params, {}, state, step, {}, lr=1e-3)
    refine = [8, 12, 16, 20, 24, 28]     # 5 < step < 30, step % 4 == 0
    assert rec.steps("relocate") == refine and rec.steps("sample_add") == refine
    assert rec.steps("inject_noise_to_position") == list(range(41))
    # the number added: max(0, min(cap_max, int(1.05 N)) - N)
    for n, cap, want in ((4, 5, 0), (100, 1000, 5), (100, 103, 3), (100, 90, 0)):
        calls = []
        monkeypatch.setattr(S, "sample_add", lambda **k: calls.append(k["n"]))
        p = {"means": torch.zeros(n, 3)}
        assert S.MCMCStrategy(cap_max=cap)._add_new_gs(p, {}, b) == want
        assert calls == ([want] if want else [])


def test_mcmc_schedule_records_sample_add_only_when_rows_are_added(monkeypatch):
    import edgegaussians_amd.strategy as S
    rec = Recorder(monkeypatch, S)
    strat = S.MCMCStrategy(refine_start_iter=5, refine_every=4, refine_stop_iter=30, cap_max=4)
    state = strat.initialize_state()
    params = tiny_params()     # nothing dead, already at the cap
    for step in range(41):
        rec.step = step
        strat.step_post_backward(params, {}, state, step, {}, lr=1e-3)
    assert rec.steps("relocate") == [] and rec.steps("sample_add") == []
    assert rec.steps("inject_noise_to_position") == list(range(41))


def test_check_sanity_failures():
    from edgegaussians_amd.strategy import DefaultStrategy, MCMCStrategy, Strategy
    params = tiny_params()
    opts = {k: torch.optim.Adam([p], lr=1e-3) for k, p in params.items()}
    for cls in (Strategy, DefaultStrategy, MCMCStrategy):
        cls().check_sanity(params, opts)
    missing = {k: v for k, v in params.items() if k != "quats"}
    with pytest.raises(AssertionError, match="quats"):
        DefaultStrategy().check_sanity(missing, {k: v for k, v in opts.items() if k != "quats"})
    two = dict(opts)
    two["means"] = torch.optim.Adam([{"params": [params["means"]]}, {"params": [torch.nn.Parameter(torch.zeros(1))]}], lr=1e-3)
    with pytest.raises(AssertionError, match="one param group"):
        MCMCStrategy().check_sanity(params, two)
    with pytest.raises(AssertionError, match="same keys"):
        DefaultStrategy().check_sanity(params, {k: v for k, v in opts.items() if k != "scales"})
    extra = dict(params)
    extra["sh0"] = torch.nn.Parameter(torch.zeros(4, 1, 3))
    with pytest.raises(AssertionError, match="same keys"):
        DefaultStrategy().check_sanity(extra, opts)
    frozen = dict(params)
    frozen["features"] = torch.nn.Parameter(torch.zeros(4, 8), requires_grad=False)     # not trainable: needs no optimizer
    DefaultStrategy().check_sanity(frozen, opts)
    both = dict(opts)
    both["means"] = torch.optim.Adam([params["means"], params["scales"]], lr=1e-3)
    with pytest.raises(AssertionError, match="exactly one parameter"):
        DefaultStrategy().check_sanity(params, both)


def test_defaults_exports_and_bindings():
    import edgegaussians_amd
    import gsplat
    import gsplat.relocation
    import gsplat.strategy
    import gsplat.strategy.ops
    from edgegaussians_amd import _lib, relocation, strategy
    d = strategy.DefaultStrategy()
    assert (d.prune_opa, d.grow_grad2d, d.grow_scale3d, d.grow_scale2d, d.prune_scale3d, d.prune_scale2d) == \
        (0.005, 0.0002, 0.01, 0.05, 0.1, 0.15)
    assert (d.refine_scale2d_stop_iter, d.refine_start_iter, d.refine_stop_iter, d.reset_every, d.refine_every,
            d.pause_refine_after_reset) == (0, 500, 15000, 3000, 100, 0)
    assert (d.absgrad, d.revised_opacity, d.verbose, d.key_for_gradient) == (False, False, False, "means2d")
    m = strategy.MCMCStrategy()
    assert (m.cap_max, m.noise_lr, m.refine_start_iter, m.refine_stop_iter, m.refine_every, m.min_opacity, m.verbose) == \
        (1_000_000, 5e5, 500, 25000, 100, 0.005, False)
    assert "strategy" in edgegaussians_amd.__all__ and edgegaussians_amd.strategy is strategy
    for name in ("Strategy", "DefaultStrategy", "MCMCStrategy"):
        assert name in gsplat.__all__ and getattr(gsplat, name) is getattr(strategy, name)
        assert getattr(gsplat.strategy, name) is getattr(strategy, name)
    assert "compute_relocation" in gsplat.__all__ and gsplat.compute_relocation is relocation.compute_relocation
    assert gsplat.relocation.compute_relocation is relocation.compute_relocation
    for name in ("duplicate", "remove", "split", "reset_opa", "relocate", "sample_add", "inject_noise_to_position",
                 "_update_param_with_optimizer"):
        assert getattr(gsplat.strategy.ops, name) is getattr(strategy.ops, name)
    header = open(os.path.join(ROOT, "include", "edgegs.h")).read()
    for name in ("eg_compute_relocation", "eg_inject_noise", "eg_strategy_update", "eg_strategy_update_packed"):
        assert name in _lib._SIGS and re.search(r"\bint " + name + r"\(", header), name
    from edgegaussians_amd import build
    assert "strategy.hip" in build.SOURCES


def test_c_entries_check_arguments_before_any_launch():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    h = _lib.load(require_device=False)
    assert h.eg_compute_relocation(None, None, None, None, 0, 51, None, None, None) == 0     # nothing to do
    assert h.eg_compute_relocation(None, None, None, None, -1, 51, None, None, None) == -1
    assert h.eg_compute_relocation(None, None, None, None, 4, 0, None, None, None) == -1
    assert h.eg_compute_relocation(None, None, None, None, 4, 51, None, None, None) == -1
    assert b"eg_compute_relocation" in h.eg_last_error_string() and b"opacities" in h.eg_last_error_string()
    assert h.eg_inject_noise(None, None, None, None, None, ctypes.c_float(1.0), 0, None) == 0
    assert h.eg_inject_noise(None, None, None, None, None, ctypes.c_float(1.0), 5, None) == -1
    assert b"means is null" in h.eg_last_error_string()
    assert h.eg_strategy_update(None, None, 1, 0, 8, 8, None, None, None, None) == 0
    assert h.eg_strategy_update(None, None, 0, 4, 8, 8, None, None, None, None) == -1
    assert h.eg_strategy_update(None, None, 1, 4, 8, 8, None, None, None, None) == -1
    assert h.eg_strategy_update_packed(None, None, None, None, 0, 2, 4, 8, 8, None, None, None, None) == 0
    assert h.eg_strategy_update_packed(None, None, None, None, -1, 2, 4, 8, 8, None, None, None, None) == -1
    assert h.eg_strategy_update_packed(None, None, None, None, 3, 2, 4, 8, 0, None, None, None, None) == -1
    assert h.eg_strategy_update_packed(None, None, None, None, 3, 2, 4, 8, 8, None, None, None, None) == -1


def test_kernel_backed_functions_refuse_cpu_and_wrong_dtypes():
    """ValueError for a CPU tensor, TypeError for a wrong dtype -- as rasterizer._check; checked in that order, so a
    float64 CPU tensor is a ValueError.  The dtype refusals need a device tensor and live in the device tests."""
    from edgegaussians_amd.relocation import compute_relocation
    from edgegaussians_amd.strategy import ops
    b = torch.from_numpy(B32)
    with pytest.raises(ValueError, match="no CPU path"):
        compute_relocation(torch.rand(4), torch.rand(4, 3), torch.ones(4, dtype=torch.int64), b)
    with pytest.raises(ValueError, match="no CPU path"):
        compute_relocation(torch.rand(4).double(), torch.rand(4, 3), torch.ones(4, dtype=torch.int64), b)
    params = tiny_params()
    before = params["means"].detach().clone()
    with pytest.raises(ValueError, match="no CPU path"):
        ops.inject_noise_to_position(params, {}, {}, 1.0)
    assert torch.equal(params["means"], before)     # nothing moved: no torch fallback
    with pytest.raises(ValueError, match="no CPU path"):
        ops._update_grad_stats(torch.zeros(4), torch.zeros(4), None, torch.zeros(1, 4, 2), torch.ones(1, 4, dtype=torch.int32),
                               8, 8, 1)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.relocate(params, {}, {}, torch.tensor([True, False, False, False]), b)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.sample_add(params, {}, {}, 2, b)
    meta = {k: torch.nn.Parameter(torch.zeros(v.shape, dtype=torch.float64, device="meta")) for k, v in params.items()}
    with pytest.raises(ValueError):     # (not a device tensor either)
        ops.inject_noise_to_position(meta, {}, {}, 1.0)
