"""Every kernel that carries adam1 (csrc/project_dev.h), element by element against float64 Adam.

Each comparison starts from the device's own pre-step fp32 state and holds every element of p', m' and v' to the bounds
of tests/adam_util.py (constants measured on the fp32 model, tests/test_adam_host.py); groups that do not step, lr == 0
and zero terms are exact.  No element is left out anywhere.  Measured on the MI355X (profiles/adam_parity.txt): every
kernel within 0.51 of a bound (m' 0.48, v' 0.51, p' 0.28), no exact case broken, no pad touched.

Part A, synthetic gradients at the C ABI, every buffer between 64 NaN floats that must come back untouched:
  test_adam_tensor_*            adam_tensor_kernel (eg_adam_tensor): vector path, scalar tail, misaligned pointers, grid-stride lap
  test_adam_multi               adam_multi_kernel (eg_adam_multi): both block layouts, per-group counts, skipped groups, lr 0
  test_adam_emit_*              adam_emit_kernel<LDS, 256 / 512> (eg_adam_emit through EdgeTrainer.apply_adam(next_view=v))
Part B, kernels that form the gradient themselves; a twin trainer with betas (0, 0) and lr 0 returns that gradient bit for
bit in its adam_m:
  test_single_step[single-*]    project_bwd_kernel<true> (eg_project_bwd_adam, EdgeTrainer.train_step)
  test_single_step[batched-*]   project_bwd_batched_kernel<true> (eg_train_step_batched)
  test_native_run_moments[fused]        phase 2 of gaussian_bwd_fused_kernel (csrc/backward_fused.hip)
  test_native_run_moments[two_kernel]   project_bwd_emit_kernel<LDS, HOIST = true, 256>
  test_native_run_moments_late_loads    project_bwd_emit_kernel<LDS, HOIST = false, 512> (more than 160 000 Gaussians)
  test_native_run_equals_single_steps   both native backward variants against the single steps checked above, bit for bit
"""
import numpy as np
import pytest
import torch

from tests import adam_util as AU
from tests.util import assert_close, assert_elementwise, record

pytestmark = pytest.mark.gpu

PAD = 64
NAN_BITS = 0x7fc00000
B1, B2 = AU.BETAS
EPS = AU.EPS
GROUP_STEPS = ((6, (0, 0, 0, 0)), (6, (7, 5, 5, 3)), (6, (4, 4, 4, -1)), (6, (-1, 2, -1, 9)))
EPOCHS = (0, 25, 40)   # the shipped schedule: three, one and no groups at lr 0


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    return _lib


def lrs_at(epoch):
    from edgegaussians_amd import LRSchedule
    lr = LRSchedule().at(epoch)
    return [lr["means"], lr["scales"], lr["quats"], lr["opacities"]]


def padded(a, lead=0):
    """fp32 array -> (device view of its shape, storage): 64 NaN floats on either side, `lead` more in front (lead = 1:
    the view starts 4 bytes off a 16-byte boundary)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    store = torch.full((PAD + lead + a.size + PAD,), float("nan"), dtype=torch.float32, device="cuda")
    view = store[PAD + lead:PAD + lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * lead) % 16 and view.is_contiguous()
    return view, store


def assert_pads(stores, label):
    for name, (store, n, lead) in stores.items():
        bits = store.view(torch.int32)
        assert bool((bits[:PAD + lead] == NAN_BITS).all()) and bool((bits[PAD + lead + n:] == NAN_BITS).all()), \
            f"{label}: the pads of {name} were written"
        assert bits.numel() == 2 * PAD + lead + n


def host(t):
    return t.detach().cpu().numpy().copy()


def finite(ob):
    return {k: (float(x) if np.isfinite(x) else "inf") for k, x in ob.items()}


# ============================================================================================= part A: eg_adam_tensor
TENSOR_SIZES = (1, 3, 4, 5, 255, 1023, 1024, 1025, 4 * 256 * 3 + 2, 2100003)   # the last: > 4 x 256 x 2048, a second lap
TENSOR_CASES = ((1, 2e-3, 0), (10, 2e-3, 1), (1000, 0.03, 0), (10, 0.0, 1), (1, 1e-4, 1), (1000, 0.0, 0))  # t, lr, zero_grad


def run_adam_tensor(vals, lr, t, zero_grad, leads=(0, 0, 0, 0)):
    from edgegaussians_amd._lib import call, ptr, stream
    n = vals[0].size
    bufs = [padded(a, lead) for a, lead in zip(vals, leads)]
    call("eg_adam_tensor", *[ptr(b[0]) for b in bufs], n, lr, B1, B2, EPS, t, zero_grad, stream())
    torch.cuda.synchronize()
    assert_pads({k: (b[1], n, lead) for k, b, lead in zip("pgmv", bufs, leads)}, f"adam_tensor n={n}")
    return [host(b[0]) for b in bufs]


@pytest.mark.parametrize("n", TENSOR_SIZES)
def test_adam_tensor_sizes(lib, n):
    """adam_tensor_kernel: float4 body, scalar tail and (n = 2 100 003) the grid-stride loop's second lap; t in {1, 10, 1000},
    lr == 0 leaves p bit-identical, zero_grad clears g[0:n] or leaves it bit-untouched."""
    assert n != 2100003 or n > 4 * 256 * 2048
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for i, (t, lr, zg) in enumerate(TENSOR_CASES[1:4] if n > 1000000 else TENSOR_CASES):  # (the large size: t 10, 1000, lr 0)
        p, g, m, v = AU.designed(n, 1000 + 7 * i + n % 997)
        p1, g1, m1, v1 = run_adam_tensor((p, g, m, v), lr, t, zg)
        assert (not g1.any()) if zg else AU.bits_equal(g1, g), f"n={n} t={t}: zero_grad={zg} not honoured"
        r = {"only": AU.step_ratios((p1, m1, v1), p, g, m, v, lr, B1, B2, EPS, t)}
        ob = AU.assert_within(r, f"adam_tensor n={n} t={t} lr={lr}")
        worst = {q: max(worst[q], ob[q]) for q in worst}
    record("adam_parity", kernel="adam_tensor_kernel", n=n, over_bounds=finite(worst))


@pytest.mark.parametrize("which", range(4), ids=["p", "g", "m", "v"])
def test_adam_tensor_misaligned_pointer_takes_the_scalar_path(lib, which):
    """n = 1025 with exactly one pointer 4 bytes off a 16-byte boundary: the same result bits as the aligned run."""
    n, t, lr = 1025, 10, 2e-3
    vals = AU.designed(n, 77)
    for zg in (0, 1):
        aligned = run_adam_tensor(vals, lr, t, zg)
        leads = tuple(1 if k == which else 0 for k in range(4))
        off = run_adam_tensor(vals, lr, t, zg, leads)
        for name, a, b in zip("pgmv", aligned, off):
            assert AU.bits_equal(a, b), f"{name} differs between the vector and the scalar path"
        AU.assert_within({"only": AU.step_ratios((off[0], off[2], off[3]), *vals, lr, B1, B2, EPS, t)}, "adam_tensor misaligned")


# ============================================================================================= part A: eg_adam_multi
def hyper_of(lib, lrs, step, group_steps, betas=AU.BETAS, eps=EPS):
    h = lib.AdamHyper(lrs[0], lrs[1], lrs[2], lrs[3], betas[0], betas[1], eps, step)
    for i, x in enumerate(group_steps):
        h.group_steps[i] = x
    return h


def grads_flat(G, inc):
    """{name: g} + absgrad increment -> EdgeTrainer.grads' layout [means 3N | quats 4N | scales 3N | opac N | inc N]."""
    return np.concatenate([AU.join(G, AU.GRAD_ORDER), inc]).astype(np.float32)


def absgrad_pair(N, seed):
    r = np.random.default_rng(seed)
    return (10.0 ** r.uniform(-6, 2, N)).astype(np.float32), (10.0 ** r.uniform(-8, 1, N)).astype(np.float32)


@pytest.mark.parametrize("N", (1, 63, 64, 65, 257, 1000, 47701))
def test_adam_multi(lib, N):
    """adam_multi_kernel: gradients at the pointers of the [means | quats | scales | opac] buffer, moments in [3N | 3N | 4N |
    N]; shared / own / skipped step counts x the shipped learning rates of epochs 0, 25, 40; N = 47 701 laps the grid-stride
    loop (11 N > 256 x 2048); absgrads += increment bit for bit, or untouched when NULL."""
    from edgegaussians_amd._lib import call, ptr, stream
    assert N != 47701 or 11 * N > 256 * 2048
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for ci, ((step, gs), epoch) in enumerate((a, b) for a in GROUP_STEPS for b in EPOCHS):
        with_abs = ci % 2 == 0
        lrs = lrs_at(epoch)
        P, G, m, v = AU.designed_groups(N, 300 + 13 * ci + N % 101)
        a0, inc = absgrad_pair(N, ci)
        gflat = grads_flat(G, inc)
        dP = {k: padded(P[k]) for k in AU.GROUPS}
        dg, dm, dv, da = padded(gflat), padded(m), padded(v), padded(a0)
        g0 = dg[0].data_ptr()
        call("eg_adam_multi", ptr(dP["means"][0]), ptr(dP["scales"][0]), ptr(dP["quats"][0]), ptr(dP["opac"][0]),
             g0, g0 + 4 * 7 * N, g0 + 4 * 3 * N, g0 + 4 * 10 * N, ptr(dm[0]), ptr(dv[0]), N, hyper_of(lib, lrs, step, gs),
             g0 + 4 * 11 * N, ptr(da[0]) if with_abs else None, stream())
        torch.cuda.synchronize()
        label = f"adam_multi N={N} group_steps={gs} epoch={epoch}"
        stores = {k: (dP[k][1], P[k].size, 0) for k in AU.GROUPS}
        stores.update(g=(dg[1], 12 * N, 0), m=(dm[1], 11 * N, 0), v=(dv[1], 11 * N, 0), absgrads=(da[1], N, 0))
        assert_pads(stores, label)
        assert AU.bits_equal(host(dg[0]), gflat), f"{label}: the gradients were written"
        assert AU.bits_equal(host(da[0]), a0 + inc if with_abs else a0), f"{label}: absgrads"
        r = AU.groups_ratios({k: host(dP[k][0]) for k in AU.GROUPS}, host(dm[0]), host(dv[0]), P, G, m, v, lrs, B1, B2, EPS, step, gs)
        ob = AU.assert_within(r, label)
        worst = {q: max(worst[q], ob[q]) for q in worst}
    record("adam_parity", kernel="adam_multi_kernel", N=N, over_bounds=finite(worst))


# ============================================================================================= trainers
ZERO_LR = dict(means_lr=0.0, scales_lr=0.0, quats_lr=0.0, opacities_lr=0.0)
STATE = ("means", "log_scales", "quats", "logit_opacities", "adam_m", "adam_v", "absgrads")
PARAMS = dict(means="means", scales="log_scales", quats="quats", opac="logit_opacities")


def make_trainer(sc, schedule=None, betas=AU.BETAS, pad=False):
    from edgegaussians_amd import EdgeTrainer
    tr = EdgeTrainer(sc.means, sc.log_scales, sc.quats, sc.logit_opacities, sc.viewmats, sc.Ks, sc.gt, sc.width, sc.height,
                     schedule=schedule, betas=betas, eps=EPS)
    tr.ensure_capacity()
    stores = {}
    if pad:  # the state and the gradient buffer between NaN pads (nothing holds their pointers yet)
        for name in STATE + ("grads",):
            t = getattr(tr, name)
            view, store = padded(host(t))
            setattr(tr, name, view)
            stores[name] = (store, t.numel(), 0)
        tr._args_cache = {}
    return tr, stores


def seed_state(tr, sc, m, v, absg, group_steps, adam_step, epoch, grads=None):
    """The scene's parameters, the given moments / absgrads / counts, in place (cached argument blocks keep their pointers)."""
    tr.flush()
    for name, src in (("means", sc.means), ("log_scales", sc.log_scales), ("quats", sc.quats),
                      ("logit_opacities", sc.logit_opacities.reshape(-1))):
        getattr(tr, name).copy_(src)
    tr.adam_m.copy_(torch.from_numpy(m)); tr.adam_v.copy_(torch.from_numpy(v)); tr.absgrads.copy_(torch.from_numpy(absg))
    if grads is not None:
        tr.grads.view(-1).copy_(torch.from_numpy(grads))
    tr.group_steps, tr.adam_step, tr.epoch = list(group_steps), adam_step, epoch


def read_state(tr):
    tr.flush()
    torch.cuda.synchronize()
    N = tr.N
    return dict(P={k: host(getattr(tr, a)).reshape(N, AU.WIDTH[k]) for k, a in PARAMS.items()}, m=host(tr.adam_m),
                v=host(tr.adam_v), absgrads=host(tr.absgrads))


def scene_params(sc):
    N = sc.means.shape[0]
    return {k: host(getattr(sc, a)).reshape(N, AU.WIDTH[k]).astype(np.float32) for k, a in PARAMS.items()}


def weight_maps(sc):
    from edgegaussians_amd import synth
    return [synth.weight_map(("weighted", "whole", "bg_edge_ratio")[v % 3], sc.gt[v], generator=torch.Generator().manual_seed(v)).cuda()
            for v in range(sc.viewmats.shape[0])]


# ============================================================================================= part A: eg_adam_emit
def emit_case(sc, ta, tb, stores, step, gs, epoch, view, seed, wm):
    """apply_adam(next_view=view) (eg_adam_emit) on ta, apply_adam() (eg_adam_multi) on tb from the same designed state:
    the Adam half against float64, then grad_step(view) of both -- projected by the emit kernel / by the step itself.
    Returns (worst multiples of the bounds, largest tile population of the view)."""
    N = ta.N
    lrs = lrs_at(epoch)
    _, G, m, v = AU.designed_groups(N, seed, tame=True)
    P = scene_params(sc)
    a0, inc = absgrad_pair(N, seed)
    gflat = grads_flat(G, inc)
    for tr in (ta, tb):  # (_advance_all counts every optimizer up by one before the call)
        seed_state(tr, sc, m, v, a0, [x - 1 for x in gs], step - 1, epoch, grads=gflat)
    ta.apply_adam(next_view=view)
    tb.apply_adam()
    assert ta._projected == view and tb._projected is None
    sa, sb = read_state(ta), read_state(tb)
    label = f"adam_emit N={N} group_steps={gs} epoch={epoch}"
    assert_pads(stores, label)
    assert AU.bits_equal(host(ta.grads).reshape(-1), gflat), f"{label}: the gradients were written"
    assert AU.bits_equal(sa["absgrads"], a0 + inc), f"{label}: absgrads"
    ob = AU.assert_within(AU.groups_ratios(sa["P"], sa["m"], sa["v"], P, G, m, v, lrs, B1, B2, EPS, step, gs), label)
    for k in AU.GROUPS:
        assert AU.bits_equal(sa["P"][k], sb["P"][k]), f"{label}: {k} differs from eg_adam_multi's"
    assert AU.bits_equal(sa["m"], sb["m"]) and AU.bits_equal(sa["v"], sb["v"]) and AU.bits_equal(sa["absgrads"], sb["absgrads"])
    # the projection half: the step that consumes the emit kernel's projection equals the one that projects itself
    ga, gb = host(ta.grad_step(view, wm[view])), host(tb.grad_step(view, wm[view]))
    la, lb = ta.pop_loss(), tb.pop_loss()
    assert not ta.overflowed() and not tb.overflowed()
    assert np.isfinite(ga).all() and np.abs(ga.reshape(-1)[:11 * N]).max() > 0
    assert AU.bits_equal(ga, gb), f"{label}: grad_step after eg_adam_emit differs from grad_step after eg_adam_multi"
    # (the loss terms of a tile's 128-Gaussian slices meet in float atomics, one address per tile and wave: up to two slices
    # per tile the sum does not depend on their order; beyond, its last bits do)
    largest_tile = max(ta.total.tolist()[3], tb.total.tolist()[3])
    if largest_tile <= 256:
        assert np.float32(la).tobytes() == np.float32(lb).tobytes(), (la, lb)
    else:
        assert abs(la - lb) <= 1e-6 * abs(la), (la, lb)
    return ob, largest_tile


def test_adam_emit_small(lib):
    """adam_emit_kernel<LDS, 256>: 333 Gaussians on a 64 x 48 frame, every step-count form x the epochs 0, 25, 40."""
    from edgegaussians_amd import LRSchedule, synth
    sc = synth.make_scene(333, 4, 64, 48, seed=21, scale=0.02, spread_opacity=True)   # (at most two slices per tile: below)
    (ta, stores), (tb, _) = make_trainer(sc, LRSchedule(), pad=True), make_trainer(sc, LRSchedule())
    wm = weight_maps(sc)
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for ci, ((step, gs), epoch) in enumerate((a, b) for a in GROUP_STEPS for b in EPOCHS):
        ob, largest_tile = emit_case(sc, ta, tb, stores, step, gs, epoch, view=(ci % 4), seed=500 + ci, wm=wm)
        assert 0 < largest_tile <= 256, "the small scene is the one whose loss sums are compared bit for bit"
        worst = {q: max(worst[q], ob[q]) for q in worst}
    record("adam_parity", kernel="adam_emit_kernel<LDS,256>", N=333, over_bounds=finite(worst))


def test_adam_emit_512_thread_variant(lib):
    """adam_emit_kernel<LDS, 512>: 65 537 Gaussians (above kPESmallMaxGaussians) on the same frame."""
    from edgegaussians_amd import LRSchedule, synth
    sc = synth.make_scene(65537, 4, 64, 48, seed=22, spread_opacity=True)
    (ta, stores), (tb, _) = make_trainer(sc, LRSchedule(), pad=True), make_trainer(sc, LRSchedule())
    ob, _ = emit_case(sc, ta, tb, stores, 6, (7, 5, 5, 3), 40, view=1, seed=540, wm=weight_maps(sc))
    record("adam_parity", kernel="adam_emit_kernel<LDS,512>", N=65537, over_bounds=finite(ob))


# ============================================================================================= part B
SEED_GROUP_STEPS, SEED_ADAM_STEP = [7, 5, 5, 3], 3
N_BEHIND = 20


def part_b_scene(n=333, w=64, h=48, seed=31, scale=0.05):
    """The scene of part B: twenty of its means sit behind the camera of view 0 (culled there: zero gradient, moments
    that must still advance)."""
    from edgegaussians_amd import synth
    sc = synth.make_scene(n, 4, w, h, seed=seed, scale=scale, spread_opacity=True)
    R, t = sc.viewmats[0, :3, :3], sc.viewmats[0, :3, 3]
    centre = -R.T @ t
    gen = torch.Generator().manual_seed(seed)
    depth = 0.5 + torch.rand(N_BEHIND, 1, generator=gen)
    sc.means[:N_BEHIND] = centre[None] - depth * R[2][None] + 0.2 * (torch.rand(N_BEHIND, 3, generator=gen) - 0.5)
    return sc


def seeded(N, seed, positive_v=False):
    """Designed moments and absgrads of a trainer.  positive_v: the exact zeros of v become 1e-24, the smallest designed
    magnitude -- then v' >= b2 1e-24 stays inside the domain of the claim whatever gradient the kernel forms (a v of 0 under
    a gradient below 3e-14 would leave it; exact zeros are covered by part A and by the 333-Gaussian scene)."""
    _, _, m, v = AU.designed_groups(N, seed, tame=True)
    if positive_v:
        v = np.where(v == 0, np.float32(1e-24), v).astype(np.float32)
    return m, v, absgrad_pair(N, seed)[0]


def twin_of(sc):
    """betas (0, 0) and four learning rates of 0: after a step adam_m is the gradient the kernel formed (m 0 + g 1), adam_v
    its fp32 square, the parameters untouched."""
    from edgegaussians_amd import LRSchedule
    return make_trainer(sc, LRSchedule(**ZERO_LR), betas=(0.0, 0.0))[0]


def twin_gradient(twin, sc, run, label):
    """Runs `run(twin)` from zero moments; returns ({name: g}, absgrad increment) after asserting the twin's own claims."""
    N = twin.N
    seed_state(twin, sc, np.zeros(11 * N, np.float32), np.zeros(11 * N, np.float32), np.zeros(N, np.float32),
               SEED_GROUP_STEPS, SEED_ADAM_STEP, 0)
    run(twin)
    st = read_state(twin)
    assert not twin.overflowed()
    P0 = scene_params(sc)
    for k in AU.GROUPS:
        assert AU.bits_equal(st["P"][k], P0[k]), f"{label}: the twin's {k} moved"
    assert np.isfinite(st["m"]).all() and AU.bits_equal(st["v"], st["m"] * st["m"]), f"{label}: twin adam_v is not the square of adam_m"
    return {k: a.copy() for k, a in AU.split(st["m"], N, AU.GROUPS).items()}, st["absgrads"]


def culled_rows(tr, sc, view, wm):
    tr.grad_step(view, wm[view])
    tr.flush()
    radius = host(tr.splat.view(torch.int32)[:, 7])
    tr.pop_loss()
    return radius <= 0


def reference_grads(twin, sc, views, wm):
    """grad_step's gradient (EdgeTrainer.grads' block order) of `views`, summed in fp32 like the batched kernel sums them."""
    N = twin.N
    acc = None
    for v in views:
        g = host(twin.grad_step(v, wm[v])).reshape(-1)[:11 * N]
        acc = g if acc is None else (acc + g).astype(np.float32)
    twin.pop_loss()
    return {k: a for k, a in AU.split(acc, N, AU.GRAD_ORDER).items()}


@pytest.fixture(scope="module")
def part_b(lib):
    sc = part_b_scene()
    wm = weight_maps(sc)
    twin = twin_of(sc)
    culled = culled_rows(twin, sc, 0, wm)
    assert culled[:N_BEHIND].all() and (~culled).sum() > 100, "the scene needs culled and visible rows in view 0"
    return dict(sc=sc, wm=wm, twin=twin, culled=culled)


@pytest.mark.parametrize("epoch", EPOCHS)
@pytest.mark.parametrize("kind", ("single", "batched"))
def test_single_step(lib, part_b, kind, epoch):
    """project_bwd_kernel<true> (train_step, view 0) and project_bwd_batched_kernel<true> (train_step_batched, views 0 + 2)
    from nonzero moments, diverged counts and the shipped schedule: p', m', v' of every element against adam64 of (seeded
    state, the kernel's own gradient); that gradient against grad_step's; the absgrad increment against the twin's."""
    from edgegaussians_amd import LRSchedule
    sc, wm, twin, culled = part_b["sc"], part_b["wm"], part_b["twin"], part_b["culled"]
    N = sc.means.shape[0]
    views = [0] if kind == "single" else [0, 2]
    run = (lambda t: t.train_step(0, wm[0])) if kind == "single" else (lambda t: t.train_step_batched(views, [wm[v] for v in views]))
    label = f"{kind} step, epoch {epoch}"
    G, inc = twin_gradient(twin, sc, run, label)
    if kind == "single":
        for k in AU.GROUPS:
            assert not G[k][culled].any(), f"{label}: a culled row has a {k} gradient"
    assert sum(int(np.count_nonzero(G[k])) for k in AU.GROUPS) > 3 * N
    # the wiring: the fused kernel's gradient is grad_step's, block for block
    ref = reference_grads(twin, sc, views, wm)
    for k in AU.GROUPS:
        assert_close(G[k], ref[k], rtol=1e-4, name=f"{label} gradient {k}")
    assert_elementwise(G, ref, AU.GROUPS, label)
    differing = {k: int((G[k].view(np.uint32) != ref[k].view(np.uint32)).sum()) for k in AU.GROUPS}
    # main
    main = make_trainer(sc, LRSchedule())[0]
    m0, v0, a0 = seeded(N, 600 + epoch)
    seed_state(main, sc, m0, v0, a0, SEED_GROUP_STEPS, SEED_ADAM_STEP, epoch)
    run(main)
    st = read_state(main)
    assert not main.overflowed() and main.group_steps == [8, 6, 6, 4] and main.adam_step == 4
    P0, lrs = scene_params(sc), lrs_at(epoch)
    v1 = B2 * v0.astype(np.float64) + (1 - B2) * AU.join(G, AU.GROUPS).astype(np.float64) ** 2
    assert AU.in_domain(0.0, v1), f"{label}: a second moment leaves the domain of the claim"
    ob = AU.assert_within(AU.groups_ratios(st["P"], st["m"], st["v"], P0, G, m0, v0, lrs, B1, B2, EPS, 4, [8, 6, 6, 4]), label)
    assert AU.bits_equal(st["absgrads"], a0 + inc), f"{label}: the absgrad increment differs from the twin's"
    record("adam_parity", kernel="project_bwd_kernel<true>" if kind == "single" else "project_bwd_batched_kernel<true>",
           epoch=epoch, over_bounds=finite(ob), gradient_elements_not_bit_equal_to_grad_step=differing, elements=11 * N)


def moments_recurrence(m0, v0, grads):
    """K steps of the float64 moment recurrence from the fp32 state and the summed per-step scales of the bounds."""
    m, v = m0.astype(np.float64), v0.astype(np.float64)
    sm, sv = np.zeros_like(m), np.zeros_like(v)
    for g in grads:
        g = g.astype(np.float64)
        sm += np.abs(B1 * m) + np.abs((1 - B1) * g)
        m = B1 * m + (1 - B1) * g
        v = B2 * v + (1 - B2) * g * g
        sv += v
    return m, v, sm, sv


def native_moments_check(sc, wm, twin, views, two_kernel, label, want_fused=None, positive_v=False):
    """train_steps(views) with every learning rate 0 on main as well: the parameters stay put, so each view's gradient is
    the twin's single step; adam_m / adam_v against the K-step float64 recurrence within the summed bounds."""
    from edgegaussians_amd import LRSchedule
    N, K = sc.means.shape[0], len(views)
    grads = [AU.join(twin_gradient(twin, sc, lambda t, v=v: t.train_step(v, wm[v]), label)[0], AU.GROUPS) for v in views]
    main = make_trainer(sc, LRSchedule(**ZERO_LR))[0]
    main.two_kernel_backward = two_kernel
    if want_fused is not None:
        assert main.fused_backward_active() == want_fused
    m0, v0, a0 = seeded(N, 700 + K, positive_v)
    seed_state(main, sc, m0, v0, a0, SEED_GROUP_STEPS, SEED_ADAM_STEP, 0)
    main.train_steps(views, [wm[v] for v in views])
    st = read_state(main)
    assert not main.overflowed()
    assert main.group_steps == [x + K for x in SEED_GROUP_STEPS] and main.adam_step == SEED_ADAM_STEP + K
    P0 = scene_params(sc)
    for k in AU.GROUPS:
        assert AU.bits_equal(st["P"][k], P0[k]), f"{label}: {k} moved at lr 0"
    m64, v64, sm, sv = moments_recurrence(m0, v0, grads)
    assert AU.in_domain(0.0, v64)
    r = {"m": AU.ratio(np.abs(st["m"] - m64), sm) / AU.C_M, "v": AU.ratio(np.abs(st["v"] - v64), sv) / AU.C_V}
    assert r["m"] <= 1.0 and r["v"] <= 1.0, f"{label}: moments at {r} x the summed bounds"
    return r


@pytest.mark.parametrize("variant", ("fused", "two_kernel"))
def test_native_run_moments(lib, part_b, variant):
    """Phase 2 of gaussian_bwd_fused_kernel (two_kernel_backward = 0) and project_bwd_emit_kernel<LDS, HOIST, 256>
    (two_kernel_backward = 1) inside train_steps([0, 2, 1]): counts 8/6/6/4 -> 10/8/8/6."""
    two = variant == "two_kernel"
    r = native_moments_check(part_b["sc"], part_b["wm"], part_b["twin"], [0, 2, 1], int(two), f"native run ({variant})",
                             want_fused=not two)
    record("adam_parity", kernel="gaussian_bwd_fused_kernel phase 2" if not two else "project_bwd_emit_kernel<LDS,HOIST,256>",
           steps=3, over_summed_bounds=finite(r))


def test_native_run_moments_late_loads(lib):
    """project_bwd_emit_kernel<LDS, HOIST = false, 512>: 163 841 Gaussians (above 160 000 the moments are loaded after the
    `radius > 0` branch) on a 96 x 64 frame, two steps."""
    sc = part_b_scene(n=163841, w=96, h=64, seed=33, scale=0.004)
    wm = weight_maps(sc)
    twin = twin_of(sc)
    culled = culled_rows(twin, sc, 0, wm)
    assert culled[:N_BEHIND].all() and (~culled).sum() > 1000
    r = native_moments_check(sc, wm, twin, [0, 2], 0, "native run (late loads)", want_fused=False, positive_v=True)
    record("adam_parity", kernel="project_bwd_emit_kernel<LDS,!HOIST,512>", steps=2, N=163841, over_summed_bounds=finite(r))


@pytest.mark.parametrize("epoch", (25, 40))
@pytest.mark.parametrize("variant", ("fused", "two_kernel"))
def test_native_run_equals_single_steps(lib, part_b, variant, epoch):
    """From the seeded state at epoch 25 (means and opacities move, scales and quats at lr 0) and at epoch 40 (all four move,
    at four different rates), train_steps of three views equals three train_step calls bit for bit: parameters, moments,
    absgrads, counts."""
    from edgegaussians_amd import LRSchedule
    sc, wm = part_b["sc"], part_b["wm"]
    N, views = sc.means.shape[0], [0, 2, 1]
    ta, tb = make_trainer(sc, LRSchedule())[0], make_trainer(sc, LRSchedule())[0]
    tb.two_kernel_backward = int(variant == "two_kernel")
    assert tb.fused_backward_active() == (variant == "fused")
    m0, v0, a0 = seeded(N, 800)
    for t in (ta, tb):
        seed_state(t, sc, m0, v0, a0, SEED_GROUP_STEPS, SEED_ADAM_STEP, epoch)
    for v in views:
        ta.train_step(v, wm[v])
    tb.train_steps(views, [wm[v] for v in views])
    sa, sb = read_state(ta), read_state(tb)
    assert not ta.overflowed() and not tb.overflowed()
    assert ta.group_steps == tb.group_steps == [10, 8, 8, 6] and ta.adam_step == tb.adam_step == 6
    assert ta.absgrads_normalize_factor == tb.absgrads_normalize_factor
    P0 = scene_params(sc)
    for k in AU.GROUPS:
        assert AU.bits_equal(sa["P"][k], sb["P"][k]), f"{variant}: {k} differs from the single steps"
        assert AU.bits_equal(sa["P"][k], P0[k]) == (epoch == 25 and k in ("scales", "quats")), f"{k}: lr 0 groups stay, the others move"
    for k in ("m", "v", "absgrads"):
        assert AU.bits_equal(sa[k], sb[k]), f"{variant}: {k} differs from the single steps"
    assert not AU.bits_equal(sa["m"], m0) and not AU.bits_equal(sa["absgrads"], a0)
