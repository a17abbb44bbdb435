"""The orientation regularisers (csrc/knn.hip: direction_loss_kernel<false / true>, ratio_loss_kernel,
eg_regulariser_step[_fixed] with the fused launch_adam_regulariser of csrc/project.hip) against float64 torch autograd of
the reference's formulas (tests/util.py: ref_direction_loss, ref_ratio_loss, ref_regulariser_step), ROW BY ROW: every
gradient row within 1e-4 of its own maximum in the float64 reference, exactly zero where the reference row is zero, the
loss within 1e-6 -- under a tensor-wide tolerance a row a hundredth of the largest may be entirely wrong.

Scenes (tests/util.py): points in order along curves (the LDS path carries the sum) and the same points shuffled (the
global atomics do); every size round the 256-row workgroup with the device's own neighbour table, -1 tails at N = 1, 2;
K = 32 on a synthetic table with the row itself and repeated indices; top_k = 0, K/2, K, K + 1; coincident and one-ulp
neighbours, dot == 0, quaternion norms 1e-3 and 1e3, scale ties.  Then one step of EdgeTrainer.regulariser_step from zero
moments on the float and the fixed-point path: the first-step moments are linear and quadratic in the scaled gradient
and expose w, lambda, nn_offset and nn_stride, which the sign-like first parameter delta does not.

tests/test_regularizers_host.py asserts, with the references alone, that every scene reaches its branch and that the
fp32 torch evaluation of the reference stays within a quarter of every row bound used here."""
import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import regularizers
    return regularizers


def _direction(R, m, q, s, nn, top_k):
    loss, gm, gq = R.direction_loss(m.cuda(), q.cuda(), s.cuda(), nn.cuda().contiguous(), top_k)
    torch.cuda.synchronize()
    return float(loss), gm.cpu(), gq.cpu()


def _compare(label, got, ref, small=None, **info):
    """loss at 1e-6, dmeans / dquats row by row; `small`: per-tensor bool rows held to 1e-4 of the tensor's maximum
    instead (the `edges` scene's small-remainder rows only).  Prints and records before it asserts."""
    loss, gm, gq = got
    l64, gm64, gq64 = ref
    loss_err = abs(loss - float(l64)) / abs(float(l64))
    cells, fails = {}, []
    for name, g, g64, sm in (("dmeans", gm, gm64, None if small is None else small[0]),
                             ("dquats", gq, gq64, None if small is None else small[1])):
        _, _, nonzero, ratio = U.row_rel_ratio(g, g64)
        sm = np.zeros(ratio.shape[0], bool) if sm is None else sm
        worst = float(ratio[~sm].max(initial=0.0))
        cells[name] = worst
        if sm.any():
            err = (g.double() - g64).abs().max(dim=1).values.numpy()[sm] / (1e-4 * float(g64.abs().max()))
            cells[name + "_small_remainder_vs_tensor_max"] = float(err.max())
            if err.max() > 1.0:
                fails.append(f"{name}: a small-remainder row misses 1e-4 of the tensor's maximum by {err.max():.2f} x")
        if nonzero:
            fails.append(f"{name}: {nonzero} rows are not exactly zero where the float64 reference is")
        if worst > 1.0:
            fails.append(f"{name}: {int((ratio[~sm] > 1).sum())} rows over 1e-4 of their own maximum, the worst by {worst:.2f} x")
    left_out = 0.0 if small is None else float(max(s.mean() for s in small))
    print(f"{label}: loss err {loss_err:.2e}, worst row ratio {cells}, rows left out {left_out:.4f}")
    record("regulariser_rows", case=label, loss_rel_err=loss_err, worst_row_ratio_to_bound=cells, rows_left_out=left_out, **info)
    assert loss_err <= U.REG_LOSS_TOL, (label, loss, float(l64))
    assert not fails, (label, fails)


@pytest.mark.parametrize("name", ["curve", "shuffled", "k32"])
def test_direction_loss_rows(R, name):
    m, q, s, nn, _ = U.reg_scene(name)
    K = nn.shape[1]
    full = None
    for top_k in U.reg_top_ks(K):
        got = _direction(R, m, q, s, nn, top_k)
        _compare(f"{name} K={K} top_k={top_k}", got, U.reg_reference(name, top_k=top_k), same_block_share=U.same_block_share(nn))
        if top_k == 0:
            full = got
        elif top_k >= K:    # the same launch arguments up to top_k: the dquats rows (one thread each) are bit-equal
            assert torch.equal(got[2], full[2])


def test_direction_loss_rows_on_the_edge_cases(R):
    m, q, s, nn, rows = U.reg_scene("edges")
    for top_k in U.reg_top_ks(U.EDGES_K):
        ref = U.reg_reference("edges", top_k=top_k)
        small = [(sv < U.REG_SMALL_REMAINDER) & (sv > 0) for sv in U.reg_survival(m, q, s, nn, top_k, ref[1:])]
        assert max(x.mean() for x in small) <= U.REG_REMAINDER_CAP
        for x in small:     # the classes built for this scene are compared like any other row
            assert not x[sum((r for c, r in rows.items()), [])].any()
        got = _direction(R, m, q, s, nn, top_k)
        _compare(f"edges K={U.EDGES_K} top_k={top_k}", got, ref, small=small)
        for r in rows["dot_zero"]:
            assert not got[1][r].any() and not got[2][r].any()


@pytest.mark.parametrize("K", U.REG_SIZE_KS)
@pytest.mark.parametrize("n", U.REG_SIZES)
def test_direction_loss_rows_at_every_size(R, n, K):
    """The device's own neighbour table (regularizers.knn): -1 tails at N = 1 and N = 2."""
    m, q, s, _, _ = U.reg_scene(f"size{n}")
    nn, _ = R.knn(m.cuda(), K)
    nn = nn.cpu()
    assert int((nn < 0).sum()) == n * max(K - (n - 1), 0) and int(nn.max()) < n
    for top_k in sorted({0, K // 2}):
        ref = U.ref_direction_loss(m, q, s, nn, top_k)
        _compare(f"size N={n} K={K} top_k={top_k}", _direction(R, m, q, s, nn, top_k), ref, negative_entries=int((nn < 0).sum()))


@pytest.mark.parametrize("name", ["curve", "edges", "size1", "size257"])
def test_ratio_loss_rows(R, name):
    s = U.reg_scene(name)[2]
    l64, g64 = U.ref_ratio_loss(s)
    loss, g = R.ratio_loss(s.cuda())
    loss_err = abs(float(loss) - float(l64)) / float(l64)
    worst, over, nonzero, _ = U.row_rel_ratio(g.cpu(), g64)
    print(f"ratio {name}: loss err {loss_err:.2e}, worst row ratio {worst:.4f}")
    record("regulariser_rows", case=f"ratio {name}", loss_rel_err=loss_err, worst_row_ratio_to_bound={"dlogscales": worst}, rows_left_out=0.0)
    assert loss_err <= U.REG_LOSS_TOL
    U.row_rel_check(g.cpu(), g64, f"ratio {name}")
    # exactly one zero per row, also on the tie rows (-r to the first maximum, +r to the first of the rest)
    assert torch.equal((g.cpu() == 0), (g64 == 0))


# ------------------------------------------------------------------ through EdgeTrainer.regulariser_step
def _step(kind, method, fixed):
    from edgegaussians_amd import EdgeTrainer, LRSchedule
    sc = U.reg_step_scene()
    sched = LRSchedule(scales_start=0, quats_start=0, opacities_start=0, **U.REG_STEP_LRS)
    tr = EdgeTrainer(sc.means, sc.log_scales, sc.quats, sc.logit_opacities, sc.viewmats, sc.Ks, sc.gt, sc.width, sc.height,
                     schedule=sched)
    tr.deterministic_regularisers = fixed
    opac_before = tr.logit_opacities.clone()
    value = tr.regulariser_step(kind, U.REG_STEP_AVG_LOSS_SUM, U.REG_STEP_FACTOR, U.REG_STEP_NN, method)
    torch.cuda.synchronize()
    return tr, value, opac_before, sched.at(0)


@pytest.mark.parametrize("fixed", [False, True], ids=["float", "fixed"])
@pytest.mark.parametrize("kind,method", U.REG_STEP_CASES)
def test_first_step_moments_and_deltas(kind, method, fixed):
    sc = U.reg_step_scene()
    N = sc.means.shape[0]
    tr, value, opac_before, lrs = _step(kind, method, fixed)
    top_k = U.REG_STEP_NN if method == "enforce_half" else 0
    nn = None
    if kind == "direction":
        table = tr.nn_table.cpu()
        assert table.shape == (N, (2 if method == "enforce_half" else 1) * U.REG_STEP_NN + 1)
        nn = table[:, 1:]    # the reference drops the nearest neighbour (edge_gs.py:344): nn_offset 1, nn_stride K + 1
    loss64, g64 = U.ref_regulariser_step(kind, sc.means, sc.quats, sc.log_scales, nn, top_k, U.REG_STEP_AVG_LOSS_SUM,
                                         U.REG_STEP_FACTOR)
    loss_err = abs(value - float(loss64)) / float(loss64)
    m_blocks, v_blocks = tr._moment_views(tr.adam_m), tr._moment_views(tr.adam_v)
    params = {"means": (tr.means, sc.means), "scales": (tr.log_scales, sc.log_scales), "quats": (tr.quats, sc.quats)}
    d64 = U.adam_first_step_deltas({k: v[1] for k, v in params.items()}, g64, lrs)
    cells, fails = {}, []
    for k, (mine, init) in params.items():
        m, v = m_blocks[k].cpu(), v_blocks[k].cpu()
        if not g64[k].any():   # outside the loss: zero gradient, exactly zero moments, the parameter untouched
            if m.any() or v.any() or not torch.equal(mine.cpu(), init):
                fails.append(f"{k}: outside the loss but moments or parameter moved")
            continue
        wm, _, zm, _ = U.row_rel_ratio(m, 0.1 * g64[k])
        wv, _, zv, _ = U.row_rel_ratio(v, 0.001 * g64[k] ** 2)
        ratio, skipped = U.adam_delta_ratio(mine.cpu().double() - init.double(), d64[k], g64[k], lrs[k])
        cells[k] = dict(m=wm, v=wv, delta_over_1e_4_lr=ratio, delta_elements_left_out=skipped)
        if zm or zv:
            fails.append(f"{k}: {zm + zv} moment rows not exactly zero where the reference is")
        if wm > 1.0 or wv > 1.0:
            fails.append(f"{k}: moments off by {wm:.2f} / {wv:.2f} x the row bound")
        if ratio > 1.0 or skipped > U.ADAM_SKIP_CAP:
            fails.append(f"{k}: delta off by {ratio:.2f} x 1e-4 lr ({skipped:.2e} of the elements left out)")
    label = f"step {kind} {method} {'fixed' if fixed else 'float'}"
    print(f"{label}: loss err {loss_err:.2e}, {cells}")
    record("regulariser_step_rows", case=label, loss_rel_err=loss_err, worst_row_ratio_to_bound=cells,
           rows_left_out=max([c["delta_elements_left_out"] for c in cells.values()], default=0.0))
    assert loss_err <= U.REG_LOSS_TOL, (value, float(loss64))
    assert not fails, fails
    # the opacity optimizer does not step: parameter and moments bit-identical to before, the step counts as stated
    assert torch.equal(tr.logit_opacities, opac_before)
    assert not m_blocks["opacities"].any() and not v_blocks["opacities"].any()
    assert tr.group_steps == [1, 1, 1, 0] and tr.adam_step == 0
    if fixed:
        assert int(tr._reg_fixed.abs().sum()) == 0, "the fixed-point scratch is handed back zeroed"


@pytest.mark.parametrize("kind,method", U.REG_STEP_CASES)
def test_two_fixed_runs_are_bit_equal(kind, method):
    a, va, _, _ = _step(kind, method, True)
    b, vb, _, _ = _step(kind, method, True)
    assert va == vb
    for x, y in ((a.means, b.means), (a.quats, b.quats), (a.log_scales, b.log_scales), (a.adam_m, b.adam_m), (a.adam_v, b.adam_v)):
        assert torch.equal(x, y)
