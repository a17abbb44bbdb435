"""edgegaussians_amd.strategy and relocation.py on the device: the three kernels per row / element / Gaussian against the
float64 statements and derived bounds of tests/strategy_util.py (constants fixed on the fp32 model by
tests/test_strategy_host.py), the ops with torch's and the project's optimizers under replayed draws, and the two
strategies end to end on invariants (no claim about the loss).

  test_compute_relocation_*     4133 rows (every ratio 1..51 x six opacities, the clamps, random pairs), no row left out;
                                opacities up to 1 - 1e-6; N = 0, N = 1, non-contiguous inputs; refusals
  test_inject_noise_*           1019 rows per element, the draw replayed; rows independent; only `means` changes
  test_state_update_*           a real three-camera rasterization call: dense and packed against float64, dense == packed
                                and run == run bit for bit, accumulation over two calls, C = 1 packed
  test_relocate_and_sample_add  torch.optim.Adam and optim.Adam, the multinomial draw replayed
  test_torch_ops_on_device      duplicate / split / remove / reset_opa with Adam, optim.Adam and optim.SelectiveAdam + a step
  test_default_strategy_* / test_mcmc_strategy_*   40 steps from 200 Gaussians, 2 cameras 64 x 64

Measured on the MI355X, worst error / bound over all rows: compute_relocation 0.20 (0.20 up to o = 1 - 1e-6), the noise
0.91 (the gate: the device's expf is one ulp where the model's is half), the statistics 0.37 (0.31 over two calls).
"""
import math

import numpy as np
import pytest
import torch

from tests import strategy_util as SU
from tests.test_strategy_host import check_keyed_on_new, make_params, snapshot

pytestmark = pytest.mark.gpu

DEV = "cuda"
B32 = SU.binoms64().astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    return _lib


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def f64(t):
    return t.detach().double().cpu().numpy()


# ==================================================================================================== compute_relocation
def test_compute_relocation_every_row_against_float64(lib):
    from edgegaussians_amd.relocation import compute_relocation
    o, s, r = SU.relocation_inputs()
    ref = SU.relocation64(o, s, r, B32)
    new_o, new_s = compute_relocation(dev(o), dev(s), dev(r), dev(B32))
    assert new_o.shape == (o.size,) and new_s.shape == (o.size, 3) and new_o.dtype == torch.float32
    excess, bound = SU.relocation_excess(f64(new_o), f64(new_s), ref, s)
    left_out = bound > 1e-2
    print(f"compute_relocation: worst error / bound {excess.max():.3f}, largest bound {bound.max():.2e}, left out {left_out.sum()}")
    assert left_out.sum() == 0
    assert (excess <= 1.0).all(), (excess.max(), int(excess.argmax()), o[excess.argmax()], r[excess.argmax()])
    # int32 ratios and a second run: the same bits
    again_o, again_s = compute_relocation(dev(o), dev(s), dev(r, torch.int32), dev(B32))
    assert torch.equal(again_o, new_o) and torch.equal(again_s, new_s)


def test_compute_relocation_near_one_empty_single_and_strided(lib):
    from edgegaussians_amd.relocation import compute_relocation
    o, s, r = SU.relocation_inputs_near_one()
    ref = SU.relocation64(o, s, r, B32)
    b = dev(B32)
    new_o, new_s = compute_relocation(dev(o), dev(s), dev(r), b)
    assert torch.isfinite(new_o).all() and torch.isfinite(new_s).all() and (new_o > 0).all() and (new_s > 0).all()
    excess, bound = SU.relocation_excess(f64(new_o), f64(new_s), ref, s)
    print(f"compute_relocation near one: worst error / bound {excess.max():.3f}, largest bound {bound.max():.2e}")
    assert (excess <= 1.0).all(), excess.max()
    e_o, e_s = compute_relocation(torch.empty(0, device=DEV), torch.empty(0, 3, device=DEV),
                                  torch.empty(0, dtype=torch.int64, device=DEV), b)
    assert e_o.shape == (0,) and e_s.shape == (0, 3)
    one_o, one_s = compute_relocation(dev(o[5:6]), dev(s[5:6]), dev(r[5:6]), b)
    assert torch.equal(one_o, new_o[5:6]) and torch.equal(one_s, new_s[5:6])
    # non-contiguous views of wider tensors give the bits of their contiguous copies
    wide_o, wide_s, wide_r = dev(np.stack([o, o * 0], 1)), dev(np.concatenate([s, s], 1)), dev(np.stack([r, r + 1], 1))
    wide_b = dev(np.concatenate([B32, B32], 1))
    assert not wide_o[:, 0].is_contiguous() and not wide_s[:, :3].is_contiguous() and not wide_b[:, :51].is_contiguous()
    st_o, st_s = compute_relocation(wide_o[:, 0], wide_s[:, :3], wide_r[:, 0], wide_b[:, :51])
    assert torch.equal(st_o, new_o) and torch.equal(st_s, new_s)


def test_kernel_backed_functions_refuse_wrong_dtypes_and_shapes(lib):
    from edgegaussians_amd.relocation import compute_relocation
    from edgegaussians_amd.strategy import ops
    b = dev(B32)
    o, s, r = torch.rand(4, device=DEV), torch.rand(4, 3, device=DEV), torch.ones(4, dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError):
        compute_relocation(o.double(), s, r, b)
    with pytest.raises(TypeError):
        compute_relocation(o, s, r.float(), b)
    with pytest.raises(TypeError):
        compute_relocation(o, s, r, b.double())
    with pytest.raises(ValueError):
        compute_relocation(o, s[:3], r, b)
    with pytest.raises(ValueError, match="no CPU path"):
        compute_relocation(o, s, r, b.cpu())
    params = make_params(8, device=DEV, extra=False)
    params["quats"] = torch.nn.Parameter(params["quats"].detach().double())
    before = params["means"].detach().clone()
    with pytest.raises(TypeError):
        ops.inject_noise_to_position(params, {}, {}, 1.0)
    assert torch.equal(params["means"], before)
    z = torch.zeros(8, device=DEV)
    with pytest.raises(TypeError):
        ops._update_grad_stats(z, z.clone(), None, torch.zeros(1, 8, 2, device=DEV), torch.ones(1, 8, device=DEV), 8, 8, 1)
    with pytest.raises(ValueError):
        ops._update_grad_stats(z, z.clone(), None, torch.zeros(2, 8, 2, device=DEV),
                               torch.ones(1, 8, dtype=torch.int32, device=DEV), 8, 8, 1)


# ============================================================================================== inject_noise_to_position
def test_inject_noise_per_element_rows_independent_only_means_change(lib, monkeypatch):
    from edgegaussians_amd.strategy import ops
    means, quats, log_scales, logits, _ = SU.noise_inputs()
    names = ("means", "quats", "scales", "opacities")

    def fresh(perm=None):
        arrs = [a if perm is None else a[perm] for a in (means, quats, log_scales, logits)]
        return {k: torch.nn.Parameter(dev(a)) for k, a in zip(names, arrs)}

    params = fresh()
    opts = {k: torch.optim.Adam([p], lr=0.0) for k, p in params.items()}     # lr 0: moments without moving the inputs
    for k, p in params.items():
        p.grad = torch.ones_like(p)
        opts[k].step()
    p0, s0 = snapshot(params, opts)
    assert torch.equal(p0["quats"], dev(quats)) and s0["means"]["exp_avg"].any()
    state = {"grad2d": torch.ones(1019, device=DEV)}
    torch.manual_seed(11)
    z = torch.randn_like(params["means"])     # the op's only draw, replayed
    after = torch.rand(1, device=DEV)
    torch.manual_seed(11)
    ops.inject_noise_to_position(params, opts, state, 1.0)
    assert torch.equal(torch.rand(1, device=DEV), after)
    ref = SU.noise64(p0["means"].cpu().numpy(), quats, log_scales, logits, z.cpu().numpy(), 1.0)
    got = params["means"].detach()
    excess = SU.noise_excess(f64(got), ref)
    moved = (got != p0["means"]).any(1).float().mean().item()
    print(f"inject_noise: worst error / bound {excess.max():.3f}; rows moved {moved:.2f}")
    assert (excess <= 1.0).all(), (excess.max(), np.unravel_index(excess.argmax(), excess.shape))
    assert 0.2 < moved < 1.0     # both sides of the gate are there
    # only `means` changed; no optimizer state, no state tensor, and the parameter objects are the same leaves
    for k in names[1:]:
        assert torch.equal(params[k], p0[k]), k
    for k in names:
        assert opts[k].param_groups[0]["params"][0] is params[k]
        for m in ("exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(opts[k].state[params[k]][m], s0[k][m]), (k, m)
    assert torch.equal(state["grad2d"], torch.ones(1019, device=DEV))
    # rows are independent: permuted rows with the permuted draw give the permuted result, bit for bit
    perm = np.random.default_rng(0).permutation(1019)
    pp = fresh(perm)
    tperm = dev(perm)

    monkeypatch.setattr(torch, "randn_like", lambda t, **k: z[tperm].clone())     # the permuted draw
    ops.inject_noise_to_position(pp, {}, {}, 1.0)
    monkeypatch.undo()
    assert torch.equal(pp["means"].detach(), got[tperm])
    # scaler 0 moves nothing; an empty set is no launch
    p2 = fresh()
    ops.inject_noise_to_position(p2, {}, {}, 0.0)
    assert torch.equal(p2["means"].detach(), dev(means))
    empty = {k: torch.nn.Parameter(v[:0].detach().clone()) for k, v in p2.items()}
    ops.inject_noise_to_position(empty, {}, {}, 1.0)


# ==================================================================================================== the state update
W3, H3, C3, N3 = 64, 48, 3, 300


@pytest.fixture(scope="module")
def raster_call(lib):
    """One scene, 3 cameras at 64 x 48, 300 Gaussians of which rows 0..39 are thrown far out (behind some cameras,
    off-screen for others); dense and packed rasterization with absgrad and a backward of ONE random cotangent."""
    from edgegaussians_amd import rasterization, synth
    sc = synth.make_scene(N3, C3, W3, H3, seed=4, spread_opacity=True, scale=0.03)
    g = torch.Generator().manual_seed(9)
    means = sc.means.clone()
    d = torch.randn(40, 3, generator=g)
    means[:40] = 0.5 + 6.0 * d / d.norm(dim=1, keepdim=True)
    cot = torch.randn(C3, H3, W3, 3, generator=g).to(DEV)
    colors = torch.rand(N3, 3, generator=g).to(DEV)
    out = {}
    for packed in (False, True):
        p = [t.clone().to(DEV).requires_grad_(True) for t in (means, sc.quats, sc.log_scales, sc.logit_opacities)]
        render, alpha, info = rasterization(p[0], p[1], torch.exp(p[2]), torch.sigmoid(p[3]).reshape(-1), colors,
                                            sc.viewmats.to(DEV), sc.Ks.to(DEV), W3, H3, packed=packed, absgrad=True)
        info["means2d"].retain_grad()
        (render * cot).sum().backward()
        out[packed] = info
    radii = out[False]["radii"]
    vis = (radii > 0)
    assert 0 < int((~vis).sum()) and int(vis.any(0).sum()) < N3 and int(vis.sum()) == out[True]["gaussian_ids"].numel()
    return out


def ref_stats(info, absgrad, packed, prior=None):
    m2d = info["means2d"]
    g = (m2d.absgrad if absgrad else m2d.grad).detach().cpu().numpy()
    r = info["radii"].cpu().numpy()
    if packed:
        g, r = SU.packed_to_dense(g, r, info["gaussian_ids"].cpu().numpy(), info["camera_ids"].cpu().numpy(), C3, N3)
    prior = prior or (None, None, None)
    return SU.stats64(g, r, W3, H3, C3, *prior)


def check_stats(state, ref, n_added, with_radii, what):
    g, c = f64(state["grad2d"]), f64(state["count"])
    assert np.array_equal(c, ref[1]), what
    ok = ref[0] > 0
    assert np.array_equal(g[~ok], ref[0][~ok]), what
    rel = np.abs(g[ok] - ref[0][ok]) / ref[0][ok]
    worst = (rel / SU.stats_bound_rel(n_added)).max()
    assert worst <= 1.0, (what, worst)
    if with_radii:
        rs = f64(state["radii"])
        assert (np.abs(rs - ref[2]) <= SU.stats_bound_rel(0) * ref[2]).all(), what
        assert (rs[ref[1] > 0] > 0).all()
    else:
        assert "radii" not in state
    return worst


@pytest.mark.parametrize("with_radii", [False, True])
@pytest.mark.parametrize("absgrad", [False, True])
def test_state_update_dense_and_packed_against_float64(raster_call, absgrad, with_radii):
    from edgegaussians_amd.strategy import DefaultStrategy
    strat = DefaultStrategy(absgrad=absgrad, refine_scale2d_stop_iter=100 if with_radii else 0)
    params = {"means": torch.zeros(N3, 3, device=DEV)}
    states = {}
    for packed in (False, True):
        info = raster_call[packed]
        st = strat.initialize_state()
        strat._update_state(params, st, info, packed=packed)
        ref = ref_stats(info, absgrad, packed)
        assert 0 < (ref[1] > 0).sum() < N3 and ref[1].max() == C3
        worst = check_stats(st, ref, C3, with_radii, ("packed" if packed else "dense"))
        # a second run from zeros: the same bits; a second call on top: exact against float64 of the two calls
        st2 = strat.initialize_state()
        strat._update_state(params, st2, info, packed=packed)
        for k in ("grad2d", "count") + (("radii",) if with_radii else ()):
            assert torch.equal(st[k], st2[k]), (packed, k)
        strat._update_state(params, st2, info, packed=packed)
        ref2 = ref_stats(info, absgrad, packed, prior=ref)
        worst2 = check_stats(st2, ref2, 2 * C3, with_radii, "two calls")
        print(f"state update packed={packed} absgrad={absgrad}: worst error / bound {worst:.3f}, two calls {worst2:.3f}")
        states[packed] = st
    # the packed KERNEL on the dense call's own numbers gathered at the visible pairs: the dense kernel's bits
    from edgegaussians_amd.strategy.ops import _update_grad_stats
    info = raster_call[False]
    m2d = info["means2d"]
    gd = (m2d.absgrad if absgrad else m2d.grad).detach()
    cam, gid = torch.nonzero(info["radii"] > 0, as_tuple=True)
    z = [torch.zeros(N3, device=DEV) for _ in range(3)]
    _update_grad_stats(z[0], z[1], z[2] if with_radii else None, gd[cam, gid], info["radii"][cam, gid], W3, H3, C3,
                       gaussian_ids=gid, camera_ids=cam)
    assert torch.equal(z[0], states[False]["grad2d"]) and torch.equal(z[1], states[False]["count"])
    if with_radii:
        assert torch.equal(z[2], states[False]["radii"])
    # the two real calls: the same pairs are visible
    assert torch.equal(states[True]["count"], states[False]["count"])
    # (their sums are NOT compared bit for bit: the two calls' means2d gradients come from two compositing layouts and
    #  differ in the last bits themselves; the statistics of the SAME numbers in both layouts are compared above)


def test_state_update_packed_one_camera(lib):
    from edgegaussians_amd import rasterization, synth
    from edgegaussians_amd.strategy import DefaultStrategy
    N = 300
    sc = synth.make_scene(N, 1, 64, 48, seed=5, spread_opacity=True, scale=0.03)
    means = sc.means.clone()
    means[:30] += 5.0
    p = [t.clone().to(DEV).requires_grad_(True) for t in (means, sc.quats, sc.log_scales, sc.logit_opacities)]
    cot = torch.randn(1, 48, 64, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    render, alpha, info = rasterization(p[0], p[1], torch.exp(p[2]), torch.sigmoid(p[3]).reshape(-1),
                                        torch.ones(N, 3, device=DEV), sc.viewmats.to(DEV), sc.Ks.to(DEV), 64, 48, packed=True)
    info["means2d"].retain_grad()
    (render * cot).sum().backward()
    assert info["n_cameras"] == 1 and 0 < info["gaussian_ids"].numel() < N
    strat = DefaultStrategy(refine_scale2d_stop_iter=10)
    st = strat.initialize_state()
    strat._update_state({"means": p[0]}, st, info, packed=True)
    g, r = SU.packed_to_dense(info["means2d"].grad.cpu().numpy(), info["radii"].cpu().numpy(),
                              info["gaussian_ids"].cpu().numpy(), info["camera_ids"].cpu().numpy(), 1, N)
    ref = SU.stats64(g, r, 64, 48, 1)
    ok = ref[0] > 0
    assert np.array_equal(f64(st["count"]), ref[1]) and ref[1].max() == 1 and ref[1].min() == 0
    assert (np.abs(f64(st["grad2d"])[ok] - ref[0][ok]) <= SU.stats_bound_rel(1) * ref[0][ok]).all()
    assert (np.abs(f64(st["radii"]) - ref[2]) <= SU.stats_bound_rel(0) * ref[2]).all()
    # the dense kernel on the scattered pairs: the same bits
    from edgegaussians_amd.strategy.ops import _update_grad_stats
    z = [torch.zeros(N, device=DEV) for _ in range(3)]
    _update_grad_stats(z[0], z[1], z[2], dev(g), dev(r), 64, 48, 1)
    assert torch.equal(z[0], st["grad2d"]) and torch.equal(z[1], st["count"]) and torch.equal(z[2], st["radii"])


# ===================================================================================================== ops on the device
def opt_classes():
    from edgegaussians_amd import optim
    return {"torch": torch.optim.Adam, "native": optim.Adam}


def stepped_dev(params, kind, seed=1):
    from edgegaussians_amd import optim
    g = torch.Generator().manual_seed(seed)
    opts = {}
    for k, p in params.items():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
        if kind == "selective":
            opts[k] = optim.SelectiveAdam([p], eps=1e-8, betas=(0.9, 0.999), lr=1e-2)
            opts[k].step(torch.ones(p.shape[0], dtype=torch.bool, device=DEV))
        else:
            opts[k] = opt_classes()[kind]([p], lr=1e-2)
            opts[k].step()
        p.grad = None
    return opts


def activation_slack(p_before, sampled, ref):
    """What the op's own fp32 sigmoid costs against a float64 statement that starts from the logits: o is rounded by up
    to U absolute, that is 1 - o by U / (1 - o) relative; x = 1 - (1 - o)^(1/r) and den follow with at most that over
    x, and logit / log pass it on: 8 U / ((1 - o) x) per drawn row (it reaches 5e-3 at logit 9)."""
    o = SU.sigmoid(f64(p_before["opacities"]))[sampled.cpu().numpy()]
    return 8 * SU.U / ((1 - o) * ref["x"])


def whole_op_close(params, ref64, tol):
    """Every key against the float64 statement of the WHOLE op: 1e-5 for the fp32 exp / log / logit on the op's side,
    plus activation_slack on the drawn rows and their copies.  (The rigorous check of the drawn rows starts from the
    op's fp32 activations: check_sources.)"""
    for k, p in params.items():
        got, ref = f64(p), ref64[k]
        t = tol.reshape((-1,) + (1,) * (ref.ndim - 1))
        assert (np.abs(got - ref) <= t * (1 + np.abs(ref))).all(), k


@pytest.mark.parametrize("kind", ["torch", "native"])
def test_relocate_and_sample_add_with_replayed_draw(lib, kind):
    from edgegaussians_amd.strategy import ops
    N, n_dead, min_op = 157, 31, 0.005
    params = make_params(N, seed=3, device=DEV)
    with torch.no_grad():
        params["opacities"][:n_dead] = -7.0     # dead: sigmoid = 9e-4
        params["opacities"][n_dead:n_dead + 6] = torch.tensor([-5.0, -4.5, 6.0, 9.0, 0.0, 1.0], device=DEV)
        # the rest barely alive (0.0055 .. 0.0095): drawn once they fall below min_opacity (x ~ o / 2), the lower clamp
        params["opacities"][n_dead + 6:] = torch.linspace(-5.2, -4.65, N - n_dead - 6, device=DEV)
    opts = stepped_dev(params, kind)
    b = dev(B32)
    U = SU.U

    def tolerances(ref, new_o64):
        x = new_o64
        lg = np.abs(SU.logit(x))
        tol_logit = SU.C_RELOC * U / (x * (1 - x)) + 2 * U * (2 + 1 / (1 - x) + lg)
        tol_log = (SU.relocation_bounds(ref)["scales_rel"][:, None] + 2 * U * (1 + np.abs(np.log(ref["new_scales"]))))
        return tol_logit, tol_log

    def check_sources(p_after, p_before, sampled, what):
        # float64 of the activations the op itself feeds the kernel (fp32 sigmoid / exp of the parameters: plumbing)
        o32 = torch.sigmoid(p_before["opacities"])[sampled].cpu().numpy()
        s32 = torch.exp(p_before["scales"])[sampled].cpu().numpy()
        ratios = np.bincount(sampled.cpu().numpy(), minlength=N)[sampled.cpu().numpy()] + 1
        ref = SU.relocation64(o32, s32, ratios, B32)
        new_o = np.clip(ref["x"], min_op, 1 - SU.EPS32)
        tol_logit, tol_log = tolerances(ref, new_o)
        got_logit, got_log = f64(p_after["opacities"][sampled]), f64(p_after["scales"][sampled])
        assert (np.abs(got_logit - SU.logit(new_o)) <= tol_logit).all(), what
        assert (np.abs(got_log - np.log(ref["new_scales"])) <= tol_log).all(), what
        act = f64(torch.sigmoid(p_after["opacities"][sampled]))
        assert (act >= min_op * (1 - 8 * U)).all() and (act <= 1 - SU.EPS32 / 2).all(), what
        assert (ref["x"] < min_op).any(), "no row reaches the lower clamp"
        return ratios

    # ---- relocate
    p0, s0 = snapshot(params, opts)
    mask = torch.sigmoid(params["opacities"].detach()) <= min_op
    assert int(mask.sum()) == n_dead
    dead, alive = mask.nonzero(as_tuple=True)[0], (~mask).nonzero(as_tuple=True)[0]
    torch.manual_seed(21)
    sampled = alive[torch.multinomial(torch.sigmoid(p0["opacities"])[alive], n_dead, replacement=True)]
    after = torch.rand(1, device=DEV)
    torch.manual_seed(21)
    state = {"grad2d": torch.arange(N, dtype=torch.float32, device=DEV) + 1}
    ops.relocate(params, opts, state, mask, b, min_opacity=min_op)
    assert torch.equal(torch.rand(1, device=DEV), after)     # one multinomial and nothing else
    check_keyed_on_new(params, opts, p0, N)
    ratios = check_sources(params, p0, sampled, "relocate")
    assert ratios.max() >= 2
    # every key against the float64 statement of the whole op (fp32 activations and logit / log on the op's side: 1e-5)
    ref64, r64 = SU.relocate64({k: f64(v) for k, v in p0.items()}, dead.cpu().numpy(), sampled.cpu().numpy(), B32, min_op)
    tol = np.full(N, 1e-5)
    tol[sampled.cpu().numpy()] += activation_slack(p0, sampled, r64)
    tol[dead.cpu().numpy()] += activation_slack(p0, sampled, r64)
    whole_op_close(params, ref64, tol)
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[sampled] = True
    for k in params:
        assert torch.equal(params[k][dead], params[k][sampled]), k     # the dead rows equal their sources in every key
        away = ~(touched | mask)
        assert torch.equal(params[k][away], p0[k][away]), k
        if k not in ("opacities", "scales"):
            assert torch.equal(params[k][sampled], p0[k][sampled]), k
        st = opts[k].state[params[k]]
        for m in ("exp_avg", "exp_avg_sq"):
            assert not st[m][sampled].any() and torch.equal(st[m][~touched], s0[k][m][~touched]) and s0[k][m][sampled].any()
    assert not state["grad2d"][sampled].any() and torch.equal(state["grad2d"][~touched], (torch.arange(N, device=DEV) + 1.0)[~touched])
    # ---- sample_add
    p1, s1 = snapshot(params, opts)
    n_add = 40
    torch.manual_seed(22)
    sampled = torch.multinomial(torch.sigmoid(p1["opacities"]), n_add, replacement=True)
    torch.manual_seed(22)
    state = {"grad2d": torch.ones(N, device=DEV)}
    ops.sample_add(params, opts, state, n_add, b, min_opacity=min_op)
    check_keyed_on_new(params, opts, p1, N + n_add)
    ref64, r64 = SU.sample_add64({k: f64(v) for k, v in p1.items()}, sampled.cpu().numpy(), B32, min_op)
    tol = np.full(N + n_add, 1e-5)
    tol[sampled.cpu().numpy()] += activation_slack(p1, sampled, r64)
    tol[N:] += activation_slack(p1, sampled, r64)
    whole_op_close(params, ref64, tol)
    touched = torch.zeros(N, dtype=torch.bool, device=DEV)
    touched[sampled] = True
    o32 = torch.sigmoid(p1["opacities"])[sampled].cpu().numpy()
    ratios = np.bincount(sampled.cpu().numpy(), minlength=N)[sampled.cpu().numpy()] + 1
    ref = SU.relocation64(o32, torch.exp(p1["scales"])[sampled].cpu().numpy(), ratios, B32)
    new_o = np.clip(ref["x"], min_op, 1 - SU.EPS32)
    tol_logit, tol_log = tolerances(ref, new_o)
    assert (np.abs(f64(params["opacities"][:N][sampled]) - SU.logit(new_o)) <= tol_logit).all()
    assert (np.abs(f64(params["scales"][:N][sampled]) - np.log(ref["new_scales"])) <= tol_log).all()
    for k in params:
        assert torch.equal(params[k][N:], params[k][:N][sampled]), k
        assert torch.equal(params[k][:N][~touched], p1[k][~touched]), k
        st = opts[k].state[params[k]]
        for m in ("exp_avg", "exp_avg_sq"):
            assert not st[m][N:].any() and not st[m][:N][sampled].any()
            assert torch.equal(st[m][:N][~touched], s1[k][m][~touched])
    assert torch.equal(state["grad2d"], torch.cat([torch.ones(N, device=DEV), torch.zeros(n_add, device=DEV)]))
    # one further step moves every row and keeps the new leaves
    for k, p in params.items():
        before = p.detach().clone()
        p.grad = torch.ones_like(p)
        opts[k].step()
        assert (p.detach() != before).all() and float(opts[k].state[p]["step"]) == 2.0, k


@pytest.mark.parametrize("kind", ["torch", "native", "selective"])
def test_torch_ops_on_device_and_a_further_step(lib, kind):
    from edgegaussians_amd.strategy import ops
    N = 23
    params = make_params(N, device=DEV)
    opts = stepped_dev(params, kind)
    n_step = 0.0 if kind == "selective" else 1.0     # SelectiveAdam never advances "step"

    def keyed(old, n):
        for k, o in opts.items():
            p = params[k]
            assert p.is_leaf and p.requires_grad and p.is_cuda and p.shape[0] == n
            assert o.param_groups[0]["params"] == [p] or o.param_groups[0]["params"][0] is p
            assert list(o.state.keys()) == [p] and float(o.state[p]["step"]) == n_step
            assert o.state[p]["exp_avg"].shape == p.shape and all(q is not p for q in old.values())

    state = {"grad2d": torch.arange(N, dtype=torch.float32, device=DEV), "scene_scale": 1.0}
    p0, s0 = snapshot(params, opts)
    mask = torch.zeros(N, dtype=torch.bool, device=DEV)
    mask[[2, 5, 22]] = True
    ops.duplicate(params, opts, state, mask)
    keyed(p0, N + 3)
    for k in params:
        assert torch.equal(params[k][:N], p0[k]) and torch.equal(params[k][N:], p0[k][[2, 5, 22]]), k
        st = opts[k].state[params[k]]
        assert torch.equal(st["exp_avg"][:N], s0[k]["exp_avg"]) and not st["exp_avg_sq"][N:].any() and s0[k]["exp_avg"].any()
    # split under a replayed draw against the float64 statement
    p1, s1 = snapshot(params, opts)
    mask = torch.zeros(N + 3, dtype=torch.bool, device=DEV)
    mask[[1, 4, 9, 24]] = True
    sel, rest = torch.where(mask)[0].cpu().numpy(), torch.where(~mask)[0].cpu().numpy()
    torch.manual_seed(5)
    z = torch.randn(2, 4, 3, device=DEV)
    torch.manual_seed(5)
    ops.split(params, opts, state, mask, revised_opacity=True)
    keyed(p1, N + 3 - 4 + 8)
    ref = SU.split64({k: f64(v) for k, v in p1.items()}, sel, rest, f64(z), True)
    for k in params:
        assert torch.equal(params[k][:N - 1], p1[k][dev(rest)]), k
        assert np.allclose(f64(params[k]), ref[k], rtol=2e-6, atol=2e-6), k
        assert not opts[k].state[params[k]]["exp_avg"][N - 1:].any()
    assert state["grad2d"].shape == (N + 7,)
    # remove, then reset_opa
    p2, s2 = snapshot(params, opts)
    mask = torch.zeros(N + 7, dtype=torch.bool, device=DEV)
    mask[[0, 7, N + 5]] = True
    keep = torch.where(~mask)[0]
    ops.remove(params, opts, state, mask)
    keyed(p2, N + 4)
    for k in params:
        assert torch.equal(params[k], p2[k][keep]) and torch.equal(opts[k].state[params[k]]["exp_avg_sq"], s2[k]["exp_avg_sq"][keep])
    p3, _ = snapshot(params, opts)
    ops.reset_opa(params, opts, state, value=0.25)
    lim = math.log(0.25 / 0.75)
    assert torch.allclose(params["opacities"], p3["opacities"].clamp(max=lim), rtol=0, atol=1e-6)
    assert (p3["opacities"] > lim).any() and float(params["opacities"].detach().max()) <= lim + 1e-6
    assert not opts["opacities"].state[params["opacities"]]["exp_avg"].any()
    # one further optimizer step: SelectiveAdam moves only the visible rows, the others every row
    vis = torch.arange(N + 4, device=DEV) % 2 == 0
    for k, p in params.items():
        before = p.detach().clone()
        p.grad = torch.ones_like(p)
        if kind == "selective":
            opts[k].step(vis)
            assert (p.detach()[vis] != before[vis]).all() and torch.equal(p.detach()[~vis], before[~vis]), k
        else:
            opts[k].step()
            assert (p.detach() != before).all() and float(opts[k].state[p]["step"]) == 2.0, k


# ============================================================================================================ end to end
def e2e_setup(n=200, seed=6):
    from edgegaussians_amd import rasterization, synth
    W = H = 64
    sc = synth.make_scene(n, 2, W, H, seed=seed, spread_opacity=True, scale=0.012)
    g = torch.Generator().manual_seed(seed)
    params = {"means": sc.means.clone(), "scales": sc.log_scales.clone(), "quats": sc.quats.clone(),
              "opacities": sc.logit_opacities.reshape(-1).clone(), "colors": torch.rand(n, 3, generator=g)}
    params = {k: torch.nn.Parameter(v.to(DEV).contiguous()) for k, v in params.items()}
    vm, Ks = sc.viewmats.to(DEV), sc.Ks.to(DEV)

    def render(p, **kw):
        return rasterization(p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]),
                             torch.sigmoid(p["colors"]), vm, Ks, W, H, **kw)

    tsc = synth.make_scene(150, 2, W, H, seed=seed + 1, spread_opacity=True, scale=0.05)
    with torch.no_grad():
        target = rasterization(tsc.means.to(DEV), tsc.quats.to(DEV), torch.exp(tsc.log_scales).to(DEV),
                               torch.sigmoid(tsc.logit_opacities).reshape(-1).to(DEV), torch.rand(150, 3, generator=g).to(DEV),
                               vm, Ks, W, H, packed=False)[0]
    return params, render, target


def check_invariants(params, opts, state, step):
    n = len(params["means"])
    for k, p in params.items():
        assert p.shape[0] == n and p.is_leaf and torch.isfinite(p).all(), (step, k)
        o = opts[k]
        assert o.param_groups[0]["params"][0] is p and len(o.state) <= 1, (step, k)
        for key, v in o.state.get(p, {}).items():
            if key != "step":
                assert v.shape == p.shape and torch.isfinite(v).all(), (step, k, key)
    for k, v in state.items():
        if isinstance(v, torch.Tensor) and k != "binoms":
            assert v.shape == (n,) and torch.isfinite(v).all(), (step, k)
    return n


@pytest.mark.parametrize("absgrad", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_default_strategy_end_to_end(lib, packed, absgrad):
    from edgegaussians_amd.strategy import DefaultStrategy
    params, render, target = e2e_setup()
    opts = {k: torch.optim.Adam([p], lr=1e-2 if k != "means" else 1e-3) for k, p in params.items()}
    strat = DefaultStrategy(refine_start_iter=5, refine_every=5, reset_every=20, grow_grad2d=0.0,
                            refine_scale2d_stop_iter=30, absgrad=absgrad)
    strat.check_sanity(params, opts)
    state = strat.initialize_state()
    torch.manual_seed(0)
    sizes, lim = [], math.log(0.01 / 0.99)
    for step in range(40):
        out, alpha, info = render(params, packed=packed, absgrad=absgrad)
        strat.step_pre_backward(params, opts, state, step, info)
        (out - target).abs().mean().backward()
        strat.step_post_backward(params, opts, state, step, info, packed=packed)
        if step == 20:
            assert float(params["opacities"].detach().max()) <= lim + 1e-6     # the reset at step 20
        for o in opts.values():
            o.step()
            o.zero_grad(set_to_none=True)
        sizes.append(check_invariants(params, opts, state, step))
    assert len(set(sizes)) > 1, sizes     # N changed
    assert sizes[:10] == [200] * 10 and sizes[10] != 200     # the first refinement is step 10 (> 5, % 5 == 0)
    out, _, _ = render(params, packed=packed)     # the next call succeeds
    assert torch.isfinite(out).all()


def test_mcmc_strategy_end_to_end(lib, monkeypatch):
    import edgegaussians_amd.strategy as S
    from edgegaussians_amd import optim
    params, render, target = e2e_setup()
    with torch.no_grad():
        params["opacities"][:10] = -10.0
    opts = {k: optim.Adam([p], lr=1e-2 if k != "means" else 1e-3) for k, p in params.items()}
    strat = S.MCMCStrategy(cap_max=260, refine_start_iter=2, refine_every=5)
    strat.check_sanity(params, opts)
    state = strat.initialize_state()
    seen = {"dead": None, "checked": 0, "noise": 0}
    real_noise = S.inject_noise_to_position

    def noise(params, optimizers, state, scaler):
        """Between the refinement and the noise of the first refining step: every formerly dead row sits on an alive row."""
        if seen["dead"] is not None:
            dead, n_before = seen["dead"], seen["dead"].numel()
            means = params["means"].detach()[:n_before]
            assert (means[dead][:, None, :] == means[~dead][None]).all(-1).any(-1).all()
            assert (torch.sigmoid(params["opacities"].detach()) >= strat.min_opacity * (1 - 1e-6)).all()
            seen["dead"], seen["checked"] = None, seen["checked"] + 1
        seen["noise"] += 1
        assert scaler == 1e-3 * strat.noise_lr
        real_noise(params=params, optimizers=optimizers, state=state, scaler=scaler)

    monkeypatch.setattr(S, "inject_noise_to_position", noise)
    torch.manual_seed(0)
    sizes = []
    for step in range(40):
        out, alpha, info = render(params, packed=False)
        strat.step_pre_backward(params, opts, state, step, info)
        (out - target).abs().mean().backward()
        if step == 5:     # the first refinement: 2 < step, step % 5 == 0
            seen["dead"] = torch.sigmoid(params["opacities"].detach()) <= strat.min_opacity
            assert int(seen["dead"].sum()) >= 10
        before = params["means"].detach().clone()
        strat.step_post_backward(params, opts, state, step, info, lr=1e-3)
        assert state["binoms"].is_cuda
        if step < 5:     # no refinement yet: the noise alone; above opacity 0.5 the gate is below e^-49, far under an ulp
            moved = (params["means"].detach() != before).any(1)
            assert not moved[torch.sigmoid(params["opacities"].detach()) > 0.5].any() and moved[:10].all()
        for o in opts.values():
            o.step()
            o.zero_grad(set_to_none=True)
        sizes.append(check_invariants(params, opts, state, step))
    assert seen["checked"] == 1 and seen["noise"] == 40
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and max(sizes) <= 260 and sizes[-1] == 260, sizes
    assert sizes[4] == 200 and sizes[5] == 210     # int(1.05 * 200) at the first refinement
    out, _, _ = render(params, packed=False)
    assert torch.isfinite(out).all()
