"""The densify / cull kernels (csrc/densify.hip: mask_scan_kernel, compact_rows_kernel, append_rows_kernel,
project_hits_kernel, project_visibility_kernel) through their C entries, against torch index arithmetic and the
float64 vote references of tests/util.py.  Index work: everything here is EXACT.

Sizes round the scan's 64-lane waves and 1024-row chunks (the carry between chunks, all 16 waves), a row mover on more
elements than one grid-stride pass holds, guard rows past every output, non-zero mask bytes other than 1, accumulators
that are non-zero on entry, an image with W != H, and a block of rows whose projection is exact in fp32 (half-integer
pixels, c < 0, c == 0).  Then cull -> duplicate -> cull_not_projecting on an EdgeTrainer in both row orders against a
torch boolean-index / cat emulation on the CPU.  tests/test_densify_host.py validates the references and the scenes."""
import pytest
import torch

from tests import util as U
from tests.util import record

pytestmark = pytest.mark.gpu

W, H = U.VOTE_SIZE
MASK_NAMES = ("zeros", "ones", "half", "sparse", "last", "byte1024", "values")


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    return _lib


def _scan(lib, mask):
    n = mask.shape[0]
    keep = mask.cuda()
    pos = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")     # (one guard word past the end)
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    lib.call("eg_mask_scan", lib.ptr(keep), n, lib.ptr(pos), lib.ptr(cnt), lib.stream())
    return keep, pos, cnt


@pytest.mark.parametrize("n", U.SCAN_SIZES)
def test_mask_scan(lib, n):
    for name, mask in U.scan_masks(n).items():
        keep, pos, cnt = _scan(lib, mask)
        want, total = U.ref_mask_scan(mask)
        assert torch.equal(pos[:n].cpu(), want), (n, name)
        assert cnt.tolist() == [total, -7] and int(pos[n]) == -7, (n, name)


@pytest.mark.parametrize("dim", [1, 3, 4])
@pytest.mark.parametrize("n", U.SCAN_SIZES)
def test_compact_rows(lib, n, dim):
    _compact(lib, n, dim, MASK_NAMES)


def test_compact_rows_takes_a_second_stride_pass(lib):
    n, dim = 140000, 4
    assert n * dim > 2048 * 256
    _compact(lib, n, dim, ("half", "last"))


def _compact(lib, n, dim, names):
    gen = torch.Generator().manual_seed(3 * n + dim)
    rows = torch.randn(n, dim, generator=gen)
    masks = U.scan_masks(n)
    rows_d = rows.cuda()
    for name in names:
        mask = masks[name]
        keep, pos, cnt = _scan(lib, mask)
        n_keep = int(cnt[0])
        out = torch.full((n_keep + 1, dim), float("nan"), device="cuda")   # one guard row of NaN past n_keep
        lib.call("eg_compact_rows", lib.ptr(rows_d), lib.ptr(keep), lib.ptr(pos), n, dim, lib.ptr(out), lib.stream())
        assert torch.equal(out[:n_keep].cpu(), rows[mask.bool()]), (n, dim, name)
        assert torch.isnan(out[n_keep]).all(), (n, dim, name)


@pytest.mark.parametrize("copies", [0, 1, 2, 4])
@pytest.mark.parametrize("n,dim", [(0, 3), (1, 1), (65, 4), (1025, 3), (2049, 1), (5000, 3), (140000, 4)])
def test_append_rows(lib, n, dim, copies):
    gen = torch.Generator().manual_seed(5 * n + dim + copies)
    rows = torch.randn(n, dim, generator=gen)
    masks = U.scan_masks(n)
    rows_d = rows.cuda()
    for name in (("half", "zeros") if n == 140000 else ("half", "sparse", "values", "zeros", "ones")):
        sel_mask = masks[name]
        sel, pos, cnt = _scan(lib, sel_mask)
        n_sel = int(cnt[0])
        picked = rows[sel_mask.bool()]
        for with_noise in (False, True):
            for fill_zero in (0.0, 1.0):
                noise = torch.randn(copies * n_sel, dim, generator=gen) * 0.05 if with_noise else None
                noise_d = noise.cuda() if with_noise else None
                out = torch.full((copies * n_sel + 1, dim), float("nan"), device="cuda")   # guard row past the end
                lib.call("eg_append_rows", lib.ptr(rows_d), lib.ptr(sel), lib.ptr(pos), n, n_sel, dim, copies, lib.ptr(noise_d),
                         fill_zero, lib.ptr(out), lib.stream())
                # copy k of the j-th selected row lands at k * n_sel + j
                want = torch.cat([torch.zeros_like(picked) if fill_zero else picked] * copies) if copies else picked[:0]
                if with_noise:
                    want = want + noise
                assert torch.equal(out[:copies * n_sel].cpu(), want), (n, dim, copies, name, with_noise, fill_zero)
                assert torch.isnan(out[copies * n_sel:]).all(), (n, dim, copies, name)
                if n_sel == 0:
                    assert torch.isnan(out).all()


def _hits(lib, means, P, masks, hits_in):
    guard = torch.full((hits_in.numel() + 1,), -7, dtype=torch.int32, device="cuda")
    guard[:-1] = hits_in.cuda()
    means_d, P_d, masks_d = means.cuda(), P.cuda().contiguous(), masks.cuda()
    lib.call("eg_project_hits", lib.ptr(means_d), means.shape[0], lib.ptr(P_d), P.shape[0], lib.ptr(masks_d), W, H, lib.ptr(guard),
             lib.stream())
    assert int(guard[-1]) == -7
    return guard[:-1].cpu()


def _visibility(lib, means, cams, maps, visib_in):
    guard = torch.full((visib_in.numel() + 1,), -7.0, dtype=torch.float64, device="cuda")
    guard[:-1] = visib_in.cuda()
    means_d, cams_d, maps_d = means.cuda(), cams.cuda(), maps.cuda()
    lib.call("eg_project_visibility", lib.ptr(means_d), means.shape[0], lib.ptr(cams_d), cams.shape[0], lib.ptr(maps_d), W, H,
             lib.ptr(guard), lib.stream())
    assert float(guard[-1]) == -7.0
    return guard[:-1].cpu()


@pytest.mark.parametrize("V", [1, 4])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_projection_votes(lib, n, V):
    """hits and visib are non-zero on entry (the kernels accumulate); rows whose rounding or division is borderline in
    float64 (<= 1 % of the rows, asserted) are left out, every other row is exact."""
    means, P, cams, masks, maps = U.vote_scene(n, V)
    gen = torch.Generator().manual_seed(n + V)
    hits_in = torch.randint(1, 50, (n,), generator=gen, dtype=torch.int32)
    votes, border = U.ref_project_hits(means, P, masks, W, H)
    got = _hits(lib, means, P, masks, hits_in)
    assert border.sum() <= U.VOTE_MAX_BORDER * n
    ok = torch.from_numpy(~border)
    assert torch.equal(got[ok].long(), (hits_in.long() + torch.from_numpy(votes))[ok]), (n, V)
    vis_in = torch.rand(n, generator=gen, dtype=torch.float64) + 0.5
    vis, border_v = U.ref_project_visibility(means, cams, maps, W, H, vis_in)
    got_v = _visibility(lib, means, cams, maps, vis_in)
    assert border_v.sum() <= U.VOTE_MAX_BORDER * n
    ok_v = torch.from_numpy(~border_v)
    assert torch.equal(got_v[ok_v], torch.from_numpy(vis)[ok_v]), (n, V)
    record("densify_projection_votes", rows=n, views=V, rows_left_out=float(border.mean()), rows_left_out_visibility=float(border_v.mean()),
           mismatches_inside_the_borderline_set=int((got.long() != hits_in.long() + torch.from_numpy(votes)).sum()))


def test_projection_votes_exact_block(lib):
    """Every product exact in fp32: half-integer pixels round to even, -0.5 lands on pixel 0, W - 0.5 falls outside,
    c < 0 votes where it lands, c == 0 does not vote.  No row is left out."""
    means, P, cams, mask, votes, _ = U.exact_vote_block()
    n = means.shape[0]
    hits_in = torch.arange(3, 3 + n, dtype=torch.int32)
    assert torch.equal(_hits(lib, means, P, mask, hits_in).long(), hits_in.long() + votes)
    vis_in = torch.arange(n, dtype=torch.float64) + 0.25
    assert torch.equal(_visibility(lib, means, cams, mask.float().contiguous(), vis_in), vis_in + votes.double())
    # mask byte 255 counts once, like 1
    assert torch.equal(_hits(lib, means, P, (mask * 255).contiguous(), hits_in).long(), hits_in.long() + votes)
    record("densify_projection_votes_exact_block", rows=n, votes=int(votes.sum()), rows_left_out=0.0)


# ------------------------------------------------------------------ trainer level
def _load(tr, state):
    """the reference-order state into the trainer's own row order (internal row r holds reference row ref_index[r])"""
    idx = tr.ref_index if tr.ref_index is not None else torch.arange(tr.N, device="cuda")
    N = tr.N
    for name, attr in (("means", "means"), ("scales", "log_scales"), ("quats", "quats")):
        setattr(tr, attr, state[name].cuda()[idx].contiguous())
    tr.logit_opacities = state["opacities"].cuda()[idx].reshape(-1).contiguous()
    tr.adam_m = torch.cat([state["m_" + k].cuda()[idx].reshape(-1) for k in U.DENSIFY_NAMES]).contiguous()
    tr.adam_v = torch.cat([state["v_" + k].cuda()[idx].reshape(-1) for k in U.DENSIFY_NAMES]).contiguous()
    tr.absgrads = state["absgrads"].cuda()[idx].contiguous()
    assert tr.adam_m.numel() == 11 * N


def _dump(tr):
    """the 13 per-Gaussian arrays in the reference's row order"""
    out = {k: tr._in_reference_order(v).cpu() for k, v in tr._params().items()}
    for pre, t in (("m_", tr.adam_m), ("v_", tr.adam_v)):
        for k, v in tr._moment_views(t).items():
            out[pre + k] = tr._in_reference_order(v.contiguous()).cpu()
    out["absgrads"] = tr._in_reference_order(tr.absgrads).cpu()
    return out


def _to_internal(tr, mask_ref):
    m = mask_ref.cuda()
    return m if tr.ref_index is None else m[tr.ref_index]


@pytest.mark.parametrize("spatial_order", [False, True])
def test_trainer_cull_duplicate_cull_not_projecting(lib, spatial_order):
    from edgegaussians_amd import EdgeTrainer
    case = U.densify_case()
    sc = case["scene"]
    want, hinge = U.emulate_densify(case)
    assert not hinge.any()
    tr = EdgeTrainer(sc.means, sc.log_scales, sc.quats, sc.logit_opacities, sc.viewmats, sc.Ks, sc.gt, W, H,
                     spatial_order=spatial_order)
    assert (tr.ref_index is not None) == spatial_order and tr.N == 2500
    _load(tr, case["state"])
    before = _dump(tr)
    for k, v in case["state"].items():
        assert torch.equal(before[k].reshape(v.shape), v), k
    events = (lambda: tr.cull(_to_internal(tr, case["cull_mask"])),
              lambda: tr.duplicate(_to_internal(tr, case["dup_mask"]), 3, 0.05, noise=case["noise"]),
              lambda: tr.cull_not_projecting(case["masks"].cuda()))
    for event, expect, name in zip(events, want, ("cull", "duplicate", "cull_not_projecting")):
        event()
        got = _dump(tr)
        assert len(got) == 13 and tr.N == expect["means"].shape[0], (name, tr.N)
        for k, v in expect.items():
            assert torch.equal(got[k].reshape(v.shape), v), (name, k, spatial_order)
    assert tr.absgrads_normalize_factor == 1
    record("densify_trainer_events", spatial_order=spatial_order, rows=[2500] + [w["means"].shape[0] for w in want], rows_left_out=0.0)
