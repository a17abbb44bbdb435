"""The float64 statement of Adam, the fp32 model and the element-wise bounds of tests/adam_util.py, on the CPU.

adam64 is held to torch.optim.Adam in float64; adam32_model (adam1's statement order in numpy fp32) stays within the
bounds on the designed inputs, which is where C_M, C_V and C_P come from; every mutant of the model -- the faults the
device tests of tests/test_gpu_adam.py are there to catch -- exceeds a bound on the same inputs."""
import math

import numpy as np
import pytest
import torch

from tests import adam_util as AU
from tests.util import record_cpu

B1, B2 = AU.BETAS


def test_designed_inputs_stay_inside_the_stated_domain():
    for n, seed in ((AU.MODEL_N, AU.MODEL_SEED), (11 * 333, 3), (1, 0), (5, 1)):
        p, g, m, v = AU.designed(n, seed)
        assert all(x.dtype == np.float32 and x.shape == (n,) and np.isfinite(x).all() for x in (p, g, m, v))
        for t in (1, 1000):
            p1, m1, v1, upd, denom = AU.adam64(p, g, m, v, 0.03, B1, B2, 1e-8, t)
            assert AU.in_domain(g, v1) and np.isfinite(p1).all() and np.abs(p1).max() < 1e30
        assert (v >= 0).all() and (np.abs(p) >= 1e-3 * (1 - 1e-6)).all() and (np.abs(p) <= 1e2).all()
        bare = (m != 0) & (v == 0) & (g == 0)
        assert (np.abs(m[bare]) <= 1e-9).all()
    p, g, m, v = AU.designed(AU.MODEL_N, AU.MODEL_SEED)
    n = AU.MODEL_N
    assert abs((g == 0).sum() - n / 17) <= 1 and abs((v == 0).sum() - n / 11) <= 1 and (m == 0).sum() >= n // 13
    assert (g > 0).sum() > n / 3 and (g < 0).sum() > n / 3
    nz = g != 0
    assert np.abs(g[nz]).min() < 1e-11 and np.abs(g[nz]).max() > 1e5 and v[v > 0].min() < 1e-23 and v.max() > 1e11
    m1 = AU.adam64(p, g, m, v, 0.0, B1, B2, 1e-8, 1)[1]
    S = np.abs(B1 * m.astype(np.float64)) + np.abs((1 - B1) * g.astype(np.float64))
    assert ((np.abs(m1) < 2e-3 * S) & (S > 0)).sum() > n / 3, "the cancelling half is missing"
    assert ((m != 0) & (v == 0) & (g == 0)).sum() > 0 and ((m == 0) & (g == 0)).sum() > 0


def test_adam64_matches_torch_adam_in_float64():
    """Eight steps with changing gradients, an lr change at step 4 and one lr = 0 phase: parameters, exp_avg and
    exp_avg_sq to 1e-13 relative."""
    gen = torch.Generator().manual_seed(4)
    n = 257
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=2e-3, betas=(B1, B2), eps=1e-8)
    p, m, v = p0.numpy().copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 9):
        lr = {1: 2e-3, 2: 2e-3, 3: 2e-3, 4: 5e-4, 5: 5e-4, 6: 0.0, 7: 0.0, 8: 5e-4}[t]
        for grp in opt.param_groups:
            grp["lr"] = lr
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** float(torch.randint(-6, 2, (1,), generator=gen))
        ref.grad = g.clone()
        before = ref.data.clone()
        opt.step()
        p, m, v, _, _ = AU.adam64(p, g.numpy(), m, v, lr, B1, B2, 1e-8, t)
        st = opt.state[ref]
        for name, mine, theirs in (("p", p, ref.data), ("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"])):
            err = np.abs(mine - theirs.numpy()).max() / np.abs(theirs.numpy()).max()
            assert err <= 1e-13, (t, name, err)
        if lr == 0:
            assert torch.equal(before, ref.data)


def test_adam64_groups_matches_four_torch_optimizers_with_their_own_counts():
    """group_steps [7, 5, 5, 3]: each optimizer is brought to one step short of its count, then all four step once."""
    gen = torch.Generator().manual_seed(5)
    N, counts, lrs = 19, [7, 5, 5, 3], [2e-3, 1e-4, 1e-3, 0.03]
    ref = {k: torch.nn.Parameter(torch.randn(N, AU.WIDTH[k], generator=gen, dtype=torch.float64)) for k in AU.GROUPS}
    opts = {k: torch.optim.Adam([ref[k]], lr=lr, betas=(B1, B2), eps=1e-8) for k, lr in zip(AU.GROUPS, lrs)}
    for k, c in zip(AU.GROUPS, counts):
        for _ in range(c - 1):
            ref[k].grad = torch.randn(N, AU.WIDTH[k], generator=gen, dtype=torch.float64) * 1e-2
            opts[k].step()
    P = {k: ref[k].data.numpy().copy() for k in AU.GROUPS}
    M = {k: opts[k].state[ref[k]]["exp_avg"].numpy().copy() for k in AU.GROUPS}
    V = {k: opts[k].state[ref[k]]["exp_avg_sq"].numpy().copy() for k in AU.GROUPS}
    G = {k: torch.randn(N, AU.WIDTH[k], generator=gen, dtype=torch.float64) * 1e-3 for k in AU.GROUPS}
    for k in AU.GROUPS:
        ref[k].grad = G[k].clone()
        opts[k].step()
    out = AU.adam64_groups(P, {k: G[k].numpy() for k in G}, M, V, lrs, B1, B2, 1e-8, 99, counts)
    for k in AU.GROUPS:
        st = opts[k].state[ref[k]]
        for name, mine, theirs in (("p", out[k][0], ref[k].data), ("m", out[k][1], st["exp_avg"]), ("v", out[k][2], st["exp_avg_sq"])):
            err = np.abs(mine - theirs.numpy()).max() / np.abs(theirs.numpy()).max()
            assert err <= 1e-13, (k, name, err)
    # 0 = the shared count, < 0 = skipped: the inputs come back
    assert AU.group_counts(6, [0, 0, 0, 0]) == [6, 6, 6, 6] and AU.group_counts(6, [4, 0, -1, 9]) == [4, 6, None, 9]
    assert AU.adam64_groups(P, {k: G[k].numpy() for k in G}, M, V, lrs, B1, B2, 1e-8, 6, [4, 4, 4, -1])["opac"] is None


def _model_ratios():
    p, g, m, v = AU.designed(AU.MODEL_N, AU.MODEL_SEED)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for t, lr, eps in AU.MODEL_CASES:
        got = AU.adam32_model(p, g, m, v, lr, B1, B2, eps, t)
        r = AU.step_ratios(got, p, g, m, v, lr, B1, B2, eps, t)
        worst = {q: max(worst[q], r[q]) for q in worst}
    return worst


def test_model_is_within_the_bounds_and_sets_the_constants():
    """adam32_model against adam64 on the designed inputs, t in {1, 2, 10, 1000, 100000} x lr in {2e-3, 1e-4, 0.03, 0} x
    eps in {1e-8, 1e-6}: the constants are 2 x the worst ratio rounded up (C_P: + 4 for the 1-ulp sqrt and reciprocal)."""
    w = _model_ratios()
    record_cpu("adam_model_ratios", model=w, constants=dict(C_M=AU.C_M, C_V=AU.C_V, C_P=AU.C_P), elements=AU.MODEL_N,
               cases=len(AU.MODEL_CASES))
    print("adam32_model worst ratios (u x scale):", w)
    for q in w:
        assert abs(w[q] - AU.MODEL_RATIOS[q]) <= 0.1, (q, w[q], AU.MODEL_RATIOS[q])
    assert AU.C_M == math.ceil(2 * w["m"]) and AU.C_V == math.ceil(2 * w["v"]) and AU.C_P == math.ceil(2 * w["p"]) + 4
    ob = AU.over_bounds(w)
    assert max(ob.values()) <= 0.5 + 1e-9


def test_exact_cases_of_the_model():
    p, g, m, v = AU.designed(4096, 7)
    p1, m1, v1 = AU.adam32_model(p, g, m, v, 0.0, B1, B2, 1e-8, 10)
    assert AU.bits_equal(p1, p) and not AU.bits_equal(m1, m) and not AU.bits_equal(v1, v)
    z = (m == 0) & (g == 0)
    assert z.any() and (m1[z] == 0).all() and (v1[(v == 0) & (g == 0)] == 0).all()
    # a broken exact case is reported as infinite, never averaged away
    bad = p.copy(); bad[5] = np.nextafter(bad[5], np.float32(np.inf))
    assert AU.step_ratios((bad, m1, v1), p, g, m, v, 0.0, B1, B2, 1e-8, 10)["p"] == np.inf
    assert AU.step_ratios((bad, m, v), p, g, m, v, 1e-3, B1, B2, 1e-8, None)["p"] == np.inf
    nan = m1.copy(); nan[3] = np.nan
    assert AU.step_ratios((p1, nan, v1), p, g, m, v, 0.0, B1, B2, 1e-8, 10)["m"] == np.inf


ELEMENT_MUTANTS = [("bias_count_off_by_one", 1000, 2e-3), ("eps_inside_sqrt", 10, 2e-3), ("betas_swapped", 10, 2e-3),
                   ("v_of_g", 10, 2e-3)]


@pytest.mark.parametrize("mutant,t,lr", ELEMENT_MUTANTS, ids=[m[0] for m in ELEMENT_MUTANTS])
def test_an_element_mutant_exceeds_a_bound(mutant, t, lr):
    p, g, m, v = AU.designed(AU.MODEL_N, AU.MODEL_SEED)
    sound = AU.over_bounds(AU.step_ratios(AU.adam32_model(p, g, m, v, lr, B1, B2, 1e-8, t), p, g, m, v, lr, B1, B2, 1e-8, t))
    assert max(sound.values()) <= 1.0
    ob = AU.over_bounds(AU.step_ratios(AU.adam32_model(p, g, m, v, lr, B1, B2, 1e-8, t, mutant), p, g, m, v, lr, B1, B2, 1e-8, t))
    record_cpu("adam_mutant", mutant=mutant, over_bounds={k: (x if np.isfinite(x) else "inf") for k, x in ob.items()})
    assert max(ob.values()) > 1.0, f"{mutant} passes every bound: {ob}"


def test_bias_count_mutant_is_rejected_broadly():
    """Off by one at t = 1000 moves the second bias correction by 3.6e-4 relative: far outside the bound wherever the
    update is not dominated by cancellation."""
    p, g, m, v = AU.designed(AU.MODEL_N, AU.MODEL_SEED)
    t, lr = 1000, 2e-3
    p1 = AU.adam32_model(p, g, m, v, lr, B1, B2, 1e-8, t, "bias_count_off_by_one")[0]
    ref, _, _, upd, denom = AU.adam64(p, g, m, v, lr, B1, B2, 1e-8, t)
    S = np.abs(B1 * m.astype(np.float64)) + np.abs((1 - B1) * g.astype(np.float64))
    bound = AU.C_P * AU.U * (np.abs(upd) + lr / (1 - B1 ** t) * S / denom) + AU.U * np.maximum(np.abs(p), np.abs(ref))
    share = float((np.abs(p1 - ref) > bound).mean())
    assert share > 0.1, share


GROUP_MUTANTS = [  # name, (step, group_steps), schedule epoch
    ("moment_blocks_swapped", (6, [0, 0, 0, 0]), 40), ("lrs_swapped", (6, [7, 5, 5, 3]), 40),
    ("skipped_group_advances_m", (6, [4, 4, 4, -1]), 40), ("lr_zero_skips", (6, [7, 5, 5, 3]), 0)]


@pytest.mark.parametrize("mutant,counts,epoch", GROUP_MUTANTS, ids=[m[0] for m in GROUP_MUTANTS])
def test_a_group_mutant_exceeds_a_bound(mutant, counts, epoch):
    from edgegaussians_amd.trainer import LRSchedule
    lr = LRSchedule().at(epoch)
    lrs = [lr["means"], lr["scales"], lr["quats"], lr["opacities"]]
    N = 333
    P, G, m, v = AU.designed_groups(N, 9)
    step, gs = counts

    def run(mut):
        gp, gm, gv = AU.adam32_model_groups(P, G, m, v, lrs, B1, B2, 1e-8, step, gs, mut)
        return AU.groups_ratios(gp, gm, gv, P, G, m, v, lrs, B1, B2, 1e-8, step, gs)

    AU.assert_within(run(None), "the unmutated model")
    with pytest.raises(AssertionError):
        AU.assert_within(run(mutant), mutant)
