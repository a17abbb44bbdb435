"""edgegaussians_amd.optim.SparseAdam and SelectiveAdam on the device, element by element against float64.

Every comparison starts from the device's own pre-step fp32 state and holds every element of p', m' and v' to the bounds
of tests/sparse_adam_util.py (constants measured on the fp32 model, tests/test_sparse_adam_host.py); rows a step does not
name are bit-identical in all three, lr == 0 leaves p bit-identical.  Parameters and moments sit between 64 NaN floats
that must come back untouched.  No test feeds an index outside [0, N) to the device.  Measured on the MI355X: every case
within 0.49 of a bound (m' 0.47, v' 0.49, p' 0.24).

  test_coalesced_gradients     one launch per tensor and no sort; N x width x index pattern x t x lr
  test_duplicates              three camera runs / shuffled / one row 100 times: ordered fp32 sums, one sort, same bits twice
  test_sort_sharing_and_...    one sort per index storage, one batched sort for copies; values that cancel only in tensor order
  test_real_gradients          the three sparse gradients of a packed three-camera rasterization: ONE sort for the three
  test_drop_in_sparse_adam...  31 steps next to torch.optim.SparseAdam with state_dict hand-overs in both directions
  test_selective_adam*         the mask form, and `visibility` from info["radii"] of a packed=False call
  test_refusals_on_device_tensors
"""
import copy

import numpy as np
import pytest
import torch

from tests import adam_util as AU
from tests import sparse_adam_util as SU
from tests.util import record, rel_err

pytestmark = pytest.mark.gpu

PAD = 64
NAN_BITS = 0x7fc00000
B1, B2 = SU.BETAS
EPS = SU.EPS
SHAPES = {"1": (), "3": (3,), "4": (4,), "9x3": (9, 3)}


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    return _lib


@pytest.fixture
def counts(lib, monkeypatch):
    """Counts the native calls (by entry name) and the index sorts of the optimizer module."""
    from edgegaussians_amd import optim
    seen = {"sort": 0}
    real_call, real_sort = lib.call, optim._stable_sort

    def call(name, *a):
        seen[name] = seen.get(name, 0) + 1
        return real_call(name, *a)

    def sort(rows):
        seen["sort"] += 1
        return real_sort(rows)

    monkeypatch.setattr(lib, "call", call)
    monkeypatch.setattr(optim, "_stable_sort", sort)
    return seen


def padded(a):
    """fp32 array -> (device view of its shape, storage): 64 NaN floats on either side."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    store = torch.full((PAD + a.size + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    view = store[PAD:PAD + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view, store


def assert_pads(stores, label):
    for k, store in enumerate(stores):
        bits = store.view(torch.int32)
        assert bool((bits[:PAD] == NAN_BITS).all()) and bool((bits[-PAD:] == NAN_BITS).all()), f"{label}: pads of buffer {k} written"


def host(t):
    return t.detach().cpu().numpy().copy()


def state_of(N, dense, seed):
    """(p, g, m, v) [N, *dense] from adam_util.designed(tame=True): non-zero moments, mixed magnitudes."""
    n = N * (int(np.prod(dense)) if dense else 1)
    return tuple(x.reshape((N,) + tuple(dense)) for x in AU.designed(n, seed, tame=True))


def sparse_setup(p, m, v, lr, t):
    """A SparseAdam over one padded parameter whose state is (m, v) at count t - 1."""
    from edgegaussians_amd.optim import SparseAdam
    (pv, ps), (mv, ms), (vv, vs) = padded(p), padded(m), padded(v)
    P = torch.nn.Parameter(pv)
    opt = SparseAdam([P], lr=2e-3, betas=(B1, B2), eps=EPS)
    opt.param_groups[0]["lr"] = lr
    opt.state[P] = {"step": t - 1, "exp_avg": mv, "exp_avg_sq": vv}
    return opt, P, (ps, ms, vs)


def sparse_step(p, m, v, idx, vals, lr, t, coalesced):
    opt, P, stores = sparse_setup(p, m, v, lr, t)
    P.grad = torch.sparse_coo_tensor(torch.from_numpy(np.asarray(idx, np.int64)).cuda()[None], torch.from_numpy(vals).cuda(),
                                     size=p.shape, is_coalesced=coalesced)
    assert P.grad.is_coalesced() == coalesced
    opt.step()
    torch.cuda.synchronize()
    assert_pads(stores, "sparse step")
    st = opt.state[P]
    assert st["step"] == t and set(st) == {"step", "exp_avg", "exp_avg_sq"}
    return host(P), host(st["exp_avg"]), host(st["exp_avg_sq"])


def merge(worst, ob):
    return {q: max(worst[q], ob[q]) for q in worst}


# ============================================================================================= 1: coalesced gradients
def coalesced_patterns(N, rng):
    return {"all": np.arange(N), "every_third": np.arange(0, N, 3), "single": np.array([N // 2]),
            "random_40": np.sort(rng.choice(N, max(1, int(0.4 * N)), replace=False))}


@pytest.mark.parametrize("width", list(SHAPES))
@pytest.mark.parametrize("N", (1, 65, 257, 1000))
def test_coalesced_gradients(lib, counts, N, width):
    """Unique ascending indices marked coalesced: one eg_adam_sparse_rows per tensor, no sort, nothing else native;
    t in {1, 10, 1000} x lr in {2e-3, 0}; named rows within the bounds, every other row bit-identical in p, m and v."""
    dense = SHAPES[width]
    rng = np.random.default_rng(100 + N)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    steps = 0
    for name, idx in coalesced_patterns(N, rng).items():
        for t in (1, 10, 1000):
            for lr in (2e-3, 0.0):
                p, g, m, v = state_of(N, dense, 1000 + 7 * steps + N)
                vals = np.ascontiguousarray(g[idx])
                got = sparse_step(p, m, v, idx, vals, lr, t, True)
                steps += 1
                assert counts == {"sort": 0, "eg_adam_sparse_rows": steps}, counts
                ref = SU.sparse_adam64(p, idx, vals, m, v, lr, B1, B2, EPS, t)
                assert ref["touched"].sum() == idx.size and (N == 1 or name == "all" or not ref["touched"].all())
                r = SU.step_ratios(got, p, m, v, ref, B1)
                worst = merge(worst, SU.assert_within(r, f"coalesced N={N} w={width} {name} t={t} lr={lr}"))
                if lr == 0:
                    assert AU.bits_equal(got[0], p)
    record("sparse_adam_parity", kernel="adam_sparse_rows_kernel (coalesced)", N=N, width=width, over_bounds=SU.finite(worst))


# ============================================================================================= 2: duplicates
def duplicate_patterns(N, rng):
    runs = np.concatenate([np.sort(rng.choice(N, int(0.7 * N), replace=False)) for _ in range(3)])
    shuffled = rng.integers(0, N, 2 * N)
    shuffled = shuffled[shuffled % 5 != 0]                          # (rows 0, 5, 10, ... stay absent)
    uniq = rng.choice(N, N // 2, replace=False)
    hot = np.concatenate([uniq, np.full(100, uniq[0])])
    return {"three_runs": runs, "shuffled": shuffled, "one_row_100_times": rng.permutation(hot)}


@pytest.mark.parametrize("width", ("3", "4"))
@pytest.mark.parametrize("N", (257, 1000))
def test_duplicates(lib, counts, N, width):
    """Uncoalesced index lists: the values of a row are added in fp32 in the order of the values tensor (the reference's
    ordered sum), one sort and one launch per step, the same bits in a second run, absent rows untouched."""
    dense = SHAPES[width]
    rng = np.random.default_rng(200 + N)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for k, (name, idx) in enumerate(duplicate_patterns(N, rng).items()):
        p, g, m, v = state_of(N, dense, 2000 + k + N)
        vals = (g[idx] * rng.uniform(0.5, 2.0, (idx.size,) + (1,) * len(dense))).astype(np.float32)
        t, lr = (1, 10, 1000)[k], 2e-3
        before = dict(counts)
        got = sparse_step(p, m, v, idx, vals, lr, t, False)
        assert counts["sort"] == before["sort"] + 1 and counts["eg_adam_sparse_rows"] == before.get("eg_adam_sparse_rows", 0) + 1
        ref = SU.sparse_adam64(p, idx, vals, m, v, lr, B1, B2, EPS, t)
        assert 0 < ref["touched"].sum() < N and np.unique(idx).size < idx.size
        if name == "one_row_100_times":
            assert np.bincount(idx).max() == 101
        worst = merge(worst, SU.assert_within(SU.step_ratios(got, p, m, v, ref, B1), f"duplicates N={N} w={width} {name}"))
        again = sparse_step(p, m, v, idx, vals, lr, t, False)
        for a, b, q in zip(got, again, "pmv"):
            assert AU.bits_equal(a, b), f"{name}: {q}' differs between two runs"
    record("sparse_adam_parity", kernel="adam_sparse_rows_kernel (duplicates)", N=N, width=width, over_bounds=SU.finite(worst))


def ordered_triples(N, rows, w, rng):
    """Every named row three times, in shuffled positions that keep the triple's order, with values (a, 2^27 a, -2^27 a):
    added first to last the fp32 sum is exactly 0, in any other order it is a or -(2^27) a-sized."""
    a = rng.uniform(0.5, 2.0, (rows.size, w)).astype(np.float32)
    big = (a * np.float32(2.0 ** 27)).astype(np.float32)
    slots = np.sort(rng.permutation(3 * rows.size).reshape(rows.size, 3), axis=1)
    idx, vals = np.empty(3 * rows.size, np.int64), np.empty((3 * rows.size, w), np.float32)
    for k, x in enumerate((a, big, -big)):
        idx[slots[:, k]] = rows
        vals[slots[:, k]] = x
    G = SU.ordered_sum(idx, vals, N)[0]
    assert (G[rows] == 0).all() and (SU.ordered_sum(idx, vals, N, order="reverse")[0][rows] != 0).all()
    return idx, vals


@pytest.mark.parametrize("N,share", ((257, 0.6), (3000, 0.75)))
def test_sort_sharing_and_summation_order(lib, counts, N, share):
    """One step() over five parameters: two gradients on ONE index storage and two on copies of it -- one batched sort for
    the lot -- plus one of another length -- a second sort.  The values cancel to exactly 0 only when a row's values are
    added in the order of the values tensor, so m' = b1 m and v' = b2 v to the bounds: the order holds through the
    single and the batched sort, below and above 4096 entries per list (N = 3000: 6750)."""
    from edgegaussians_amd.optim import SparseAdam
    rng = np.random.default_rng(600 + N)
    rows = np.sort(rng.choice(N, int(share * N), replace=False))
    idx, vals3 = ordered_triples(N, rows, 3, rng)
    vals4 = np.ascontiguousarray(np.concatenate([vals3, vals3[:, :1]], axis=1))
    idx_s, vals_s = ordered_triples(N, rows[: rows.size // 2], 3, rng)
    assert (idx.size > 4096) == (N == 3000)
    shared = torch.from_numpy(idx).cuda()[None]
    plan = [(idx, vals3, shared), (idx, vals4, shared), (idx, vals3, shared.clone()), (idx, vals4, shared.clone()),
            (idx_s, vals_s, torch.from_numpy(idx_s).cuda()[None])]
    pre, live, stores = [], [], []
    for k, (_, vals, i_dev) in enumerate(plan):
        p, _, m, v = state_of(N, (vals.shape[1],), 6000 + k + N)
        (pv, ps), (mv, ms), (vv, vs) = padded(p), padded(m), padded(v)
        q = torch.nn.Parameter(pv)
        q.grad = torch.sparse_coo_tensor(i_dev, torch.from_numpy(vals).cuda(), size=p.shape)
        assert q.grad._indices().data_ptr() == i_dev.data_ptr() and not q.grad.is_coalesced()
        pre.append((p, m, v))
        live.append((q, mv, vv))
        stores += [ps, ms, vs]
    opt = SparseAdam([q for q, _, _ in live], lr=2e-3, betas=(B1, B2), eps=EPS)
    for q, mv, vv in live:
        opt.state[q] = {"step": 9, "exp_avg": mv, "exp_avg_sq": vv}
    opt.step()
    torch.cuda.synchronize()
    assert counts == {"sort": 2, "eg_adam_sparse_rows": 5}, counts
    assert_pads(stores, "sort sharing")
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for k, ((p, m, v), (i_np, vals, _), (q, mv, vv)) in enumerate(zip(pre, plan, live)):
        ref = SU.sparse_adam64(p, i_np, vals, m, v, 2e-3, B1, B2, EPS, 10)
        assert (ref["g"][ref["touched"]] == 0).all() and 0 < ref["touched"].sum() < N
        worst = merge(worst, SU.assert_within(SU.step_ratios((host(q), host(mv), host(vv)), p, m, v, ref, B1), f"sort sharing tensor {k}"))
    record("sparse_adam_parity", kernel="adam_sparse_rows_kernel (shared sorts)", N=N, nnz=int(idx.size), over_bounds=SU.finite(worst))


# ============================================================================================= 3: real gradients
def packed_sparse_gradients():
    """means, quats, scales and their sparse gradients from rasterization(packed=True, sparse_grad=True) on the
    500-Gaussian, three-camera, 70 x 52 pinhole scene, with a loss on the projection's outputs (no atomics)."""
    from edgegaussians_amd import rasterization
    from tests.test_gpu_ortho import _packed_scene
    leaves, fixed, w, N = _packed_scene(ortho=False)
    assert N == 500 and fixed["near_plane"] == 3.7 and fixed["radius_clip"] == 3.5 and fixed["viewmats"].shape[0] == 3
    params = [torch.nn.Parameter(t.clone().cuda()) for t in leaves[:3]]
    rest = [t.clone().cuda() for t in leaves[3:]]
    _, _, info = rasterization(*params, *rest, packed=True, sparse_grad=True, **fixed)
    cam, gid = info["camera_ids"], info["gaussian_ids"]
    loss = sum((info[k] * w[k][cam, gid]).sum() for k in ("means2d", "depths", "conics", "opacities"))
    loss.backward()
    torch.cuda.synchronize()
    return params, N


def real_step():
    from edgegaussians_amd.optim import SparseAdam
    params, N = packed_sparse_gradients()
    opt = SparseAdam(params, lr=2e-3, betas=(B1, B2), eps=EPS)
    pre = []
    for k, P in enumerate(params):
        _, _, m, v = state_of(N, tuple(P.shape[1:]), 3000 + k)
        opt.state[P] = {"step": 9, "exp_avg": torch.from_numpy(m).cuda(), "exp_avg_sq": torch.from_numpy(v).cuda()}
        g = P.grad
        assert g.is_sparse and g.sparse_dim() == 1 and not g.is_coalesced()
        pre.append((host(P), m, v, host(g._indices()[0]), host(g._values())))
    opt.step()
    torch.cuda.synchronize()
    post = [(host(P), host(opt.state[P]["exp_avg"]), host(opt.state[P]["exp_avg_sq"])) for P in params]
    assert all(opt.state[P]["step"] == 10 for P in params)
    return pre, post, N


def test_real_gradients(lib, counts):
    """One SparseAdam over means, quats and scales with the gradients of a packed three-camera call: every element within
    the bounds against the reference built from the gradients read back; the Gaussians no camera kept are bit-identical
    in parameter and moments (11 of the 500, 2.2 %); ONE sort and three launches for the three tensors -- autograd hands
    each parameter its own copy of the indices, so the three go through one batched call; a second run gives the same
    bits."""
    pre, post, N = real_step()
    assert counts["sort"] == 1 and counts["eg_adam_sparse_rows"] == 3, counts
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for k, ((p, m, v, idx, vals), got) in enumerate(zip(pre, post)):
        assert np.array_equal(idx, pre[0][3]) and idx.size == vals.shape[0] and np.unique(idx).size < idx.size
        ref = SU.sparse_adam64(p, idx, vals, m, v, 2e-3, B1, B2, EPS, 10)
        worst = merge(worst, SU.assert_within(SU.step_ratios(got, p, m, v, ref, B1), f"real gradients tensor {k}"))
        away = ~ref["touched"]
        for a, b, q in zip(got, (p, m, v), "pmv"):
            assert AU.bits_equal(a[away], b[away]), f"tensor {k}: {q} of an unseen Gaussian moved"
    share = float(away.mean())
    print(f"unseen share {share:.4f}, nnz {pre[0][3].size}")
    assert 0.01 <= share <= 0.1, share
    _, post2, _ = real_step()
    for a3, b3 in zip(post, post2):
        for a, b in zip(a3, b3):
            assert AU.bits_equal(a, b), "a second identical run gives other bits"
    record("sparse_adam_parity", kernel="adam_sparse_rows_kernel (packed gradients)", N=N, nnz=int(pre[0][3].size),
           unseen_share=share, over_bounds=SU.finite(worst))


# ============================================================================================= 4: drop-in
def test_drop_in_sparse_adam_equals_torch_sparse_adam(lib):
    """31 steps next to torch.optim.SparseAdam on the device with the same changing sparse gradients (unique, three runs,
    shuffled duplicates, empty), an lr change, a state_dict hand-over from torch's class to ours at step 12 and from
    ours to torch's at step 22, the reference's in-place state surgery at step 26: parameters and moments agree to 2e-6
    of their scale (tests.util.rel_err), the bar of test_drop_in_adam_equals_torch_adam.  Measured on the MI355X: 3.5e-7
    (the record line sparse_adam_drop_in carries the current figure)."""
    from edgegaussians_amd.optim import SparseAdam
    gen = np.random.default_rng(11)
    shapes = [(1000, 3), (1000, 4), (257,), (65, 9, 3)]
    init = [gen.standard_normal(s).astype(np.float32) for s in shapes]
    mk = lambda cls: cls([torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in init], lr=2e-3)  # noqa: E731
    ours, theirs = mk(SparseAdam), mk(torch.optim.SparseAdam)
    for k in range(31):
        if k == 12:
            ours.load_state_dict(copy.deepcopy(theirs.state_dict()))   # (a state_dict refers to the live moment tensors)
        if k == 22:
            theirs.load_state_dict(copy.deepcopy(ours.state_dict()))
        if k == 15:
            for o in (ours, theirs):
                o.param_groups[0]["lr"] *= 0.1
        if k == 26:   # the reference's remove_from_optim (edge_gs.py:384-402), applied to both: cull rows, swap the parameter
            for o in (ours, theirs):
                param = o.param_groups[0]["params"][0]
                keep = (torch.arange(param.shape[0], device="cuda") % 3) != 0
                new = torch.nn.Parameter(param.detach()[keep].clone())
                state = o.state.pop(param)
                state["exp_avg"], state["exp_avg_sq"] = state["exp_avg"][keep], state["exp_avg_sq"][keep]
                o.param_groups[0]["params"][0] = new
                o.state[new] = state
        for po, pt in zip(ours.param_groups[0]["params"], theirs.param_groups[0]["params"]):
            N = po.shape[0]
            kind = k % 4
            idx = (np.sort(gen.choice(N, N // 3, replace=False)) if kind == 0 else
                   np.concatenate([np.sort(gen.choice(N, int(0.7 * N), replace=False)) for _ in range(3)]) if kind == 1 else
                   gen.integers(0, N, N) if kind == 2 else np.zeros(0, np.int64) if k == 7 else gen.integers(0, N, 5))
            vals = (gen.standard_normal((idx.size,) + tuple(po.shape[1:])) * (0.1 + k % 3)).astype(np.float32)
            i, x = torch.from_numpy(idx).cuda()[None], torch.from_numpy(vals).cuda()
            po.grad = torch.sparse_coo_tensor(i, x, size=po.shape, is_coalesced=(kind == 0))
            pt.grad = torch.sparse_coo_tensor(i.clone(), x.clone(), size=pt.shape, is_coalesced=(kind == 0))
        ours.step()
        theirs.step()
        ours.zero_grad()
        theirs.zero_grad()
    torch.cuda.synchronize()
    worst = 0.0
    for po, pt in zip(ours.param_groups[0]["params"], theirs.param_groups[0]["params"]):
        so, st = ours.state[po], theirs.state[pt]
        assert set(so) == {"step", "exp_avg", "exp_avg_sq"} and so["step"] == st["step"] == 31
        errs = [rel_err(po.detach(), pt.detach()), rel_err(so["exp_avg"], st["exp_avg"]), rel_err(so["exp_avg_sq"], st["exp_avg_sq"])]
        worst = max(worst, *errs)
    record("sparse_adam_drop_in", steps=31, worst_rel_err=worst)
    print("drop-in worst rel_err", worst)
    assert worst <= 2e-6, worst


# ============================================================================================= 5: SelectiveAdam
def selective_step(p, g, m, v, vis, lr):
    from edgegaussians_amd.optim import SelectiveAdam
    (pv, ps), (mv, ms), (vv, vs) = padded(p), padded(m), padded(v)
    P = torch.nn.Parameter(pv)
    opt = SelectiveAdam([P], eps=EPS, betas=(B1, B2), lr=lr)
    step = torch.tensor(0.0)
    opt.state[P] = {"step": step, "exp_avg": mv, "exp_avg_sq": vv}
    P.grad = torch.from_numpy(g).cuda()
    opt.step(torch.from_numpy(vis).cuda())
    torch.cuda.synchronize()
    assert_pads((ps, ms, vs), "selective step")
    assert opt.state[P]["step"] is step and float(step) == 0.0
    assert AU.bits_equal(host(P.grad), g)
    return host(P), host(mv), host(vv)


@pytest.mark.parametrize("M", (1, 3, 4))
@pytest.mark.parametrize("N", (1, 65, 1000))
def test_selective_adam(lib, counts, N, M):
    """Masks none / all / a random half, lr 2e-3 and 0: visible rows within the bounds of the selective form (no bias
    correction), masked-out rows bit-identical in p, m and v, state["step"] still 0.0, one launch per tensor."""
    rng = np.random.default_rng(300 + N + M)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    masks = {"none": np.zeros(N, bool), "all": np.ones(N, bool), "half": rng.random(N) < 0.5}
    for k, (name, vis) in enumerate(masks.items()):
        for lr in (2e-3, 0.0):
            p, g, m, v = state_of(N, (M,) if M > 1 else (), 4000 + 3 * k + N + M)
            got = selective_step(p, g, m, v, vis, lr)
            ref = SU.selective_adam64(p, g, m, v, vis, lr, B1, B2, EPS)
            worst = merge(worst, SU.assert_within(SU.step_ratios(got, p, m, v, ref, B1), f"selective N={N} M={M} {name} lr={lr}"))
            if name == "none" or lr == 0:
                assert AU.bits_equal(got[0], p)
    assert counts == {"sort": 0, "eg_adam_masked_rows": 6}, counts
    # a fresh optimizer creates the state itself: step is the float tensor 0.0 and stays there
    from edgegaussians_amd.optim import SelectiveAdam
    P = torch.nn.Parameter(torch.zeros(N, 3, device="cuda"))
    opt = SelectiveAdam([P], eps=EPS, betas=(B1, B2), lr=1e-2)
    P.grad = torch.ones(N, 3, device="cuda")
    opt.step(torch.ones(N, dtype=torch.bool, device="cuda"))
    st = opt.state[P]
    assert isinstance(st["step"], torch.Tensor) and st["step"].dtype == torch.float32 and float(st["step"]) == 0.0
    assert torch.allclose(P.detach(), torch.full_like(P, -1e-2 * 0.1 / (0.001 ** 0.5 + EPS)), rtol=1e-5)
    record("sparse_adam_parity", kernel="adam_masked_rows_kernel", N=N, M=M, over_bounds=SU.finite(worst))


def test_selective_adam_with_visibility_from_radii(lib):
    """End to end: a packed=False rasterization, an image loss, visibility = (info["radii"] > 0).any(0); one SelectiveAdam
    with a group per tensor; against the reference built from the gradients read back."""
    from edgegaussians_amd import rasterization
    from edgegaussians_amd.optim import SelectiveAdam
    from tests.test_gpu_ortho import _packed_scene
    leaves, fixed, w, N = _packed_scene(ortho=False)
    params = [torch.nn.Parameter(t.clone().cuda()) for t in leaves[:3]]
    rest = [t.clone().cuda() for t in leaves[3:]]
    render, alpha, info = rasterization(*params, *rest, packed=False, **fixed)
    ((render * w["render"]).sum() + (alpha * w["alpha"]).sum()).backward()
    visibility = (info["radii"] > 0).any(0)
    assert visibility.shape == (N,) and visibility.dtype == torch.bool
    opt = SelectiveAdam([{"params": [P], "lr": lr} for P, lr in zip(params, (2e-3, 1e-3, 5e-3))], eps=1e-15, betas=(B1, B2))
    pre = []
    for k, P in enumerate(params):
        _, _, m, v = state_of(N, tuple(P.shape[1:]), 5000 + k)
        opt.state[P] = {"step": torch.tensor(0.0), "exp_avg": torch.from_numpy(m).cuda(), "exp_avg_sq": torch.from_numpy(v).cuda()}
        pre.append((host(P), host(P.grad), m, v))
    opt.step(visibility)
    torch.cuda.synchronize()
    vis = host(visibility)
    assert 0 < vis.sum() < N
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for (p, g, m, v), P, lr in zip(pre, params, (2e-3, 1e-3, 5e-3)):
        got = (host(P), host(opt.state[P]["exp_avg"]), host(opt.state[P]["exp_avg_sq"]))
        ref = SU.selective_adam64(p, g, m, v, vis, lr, B1, B2, 1e-15)
        worst = merge(worst, SU.assert_within(SU.step_ratios(got, p, m, v, ref, B1), "selective end to end"))
        assert float(opt.state[P]["step"]) == 0.0
    record("sparse_adam_parity", kernel="adam_masked_rows_kernel (radii)", N=N, visible=int(vis.sum()), over_bounds=SU.finite(worst))


# ============================================================================================= 6: refusals
def test_refusals_on_device_tensors(lib, counts):
    """A dense gradient (torch's wording), sparse_dim() == 2, an fp64 parameter, a state of another shape: each raises
    before anything is launched or counted, and a sound parameter in the same step is not stepped either."""
    from edgegaussians_amd.optim import SparseAdam
    idx = torch.tensor([[1, 3]], device="cuda")

    def attempt(bad, exc, match=None, state=None):
        good = torch.nn.Parameter(torch.ones(5, 3, device="cuda"))
        good.grad = torch.sparse_coo_tensor(idx, torch.ones(2, 3, device="cuda"), size=(5, 3))
        opt = SparseAdam([good, bad])
        if state is not None:
            opt.state[bad] = state
        with pytest.raises(exc, match=match):
            opt.step()
        torch.cuda.synchronize()
        assert bool((good == 1).all()) and len(opt.state[good]) == 0

    dense = torch.nn.Parameter(torch.ones(5, 3, device="cuda"))
    dense.grad = torch.ones(5, 3, device="cuda")
    attempt(dense, RuntimeError, "SparseAdam does not support dense gradients, please consider Adam instead")
    two = torch.nn.Parameter(torch.ones(5, 3, device="cuda"))
    two.grad = torch.sparse_coo_tensor(torch.tensor([[1, 3], [0, 2]], device="cuda"), torch.ones(2, device="cuda"), size=(5, 3))
    attempt(two, NotImplementedError, "sparse_dim")
    f64 = torch.nn.Parameter(torch.ones(5, 3, device="cuda", dtype=torch.float64))
    f64.grad = torch.sparse_coo_tensor(idx, torch.ones(2, 3, device="cuda", dtype=torch.float64), size=(5, 3))
    attempt(f64, NotImplementedError, "fp32")
    odd = torch.nn.Parameter(torch.ones(5, 3, device="cuda"))
    odd.grad = torch.sparse_coo_tensor(idx, torch.ones(2, 3, device="cuda"), size=(5, 3))
    attempt(odd, RuntimeError, "does not match", state={"step": 1, "exp_avg": torch.zeros(4, 3, device="cuda"),
                                                        "exp_avg_sq": torch.zeros(5, 3, device="cuda")})
    assert counts == {"sort": 0}, counts
