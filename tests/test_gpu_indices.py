"""Per-pixel intersection lists on the device (functional.rasterize_to_indices_in_range / accumulate; csrc/indices.hip)
against the float64 references of tests/indices_util.py, on its screen-space scenes (40 x 36, two cameras; S8_16 at
tile sizes 8 and 16, S32 -- 1300 centres in the first 32-pixel tile -- at 32), thin and thick opacities.

The id lists are compared per pixel, exactly, outside the borderline set of the call (tests/test_indices_host.py
asserts with the references alone that the set is at most BORDER_CAP of the pixels in every case used here, that no
pixel stops in the thin regime, that many stop in the thick one -- some before their tile's last batch -- and that a pixel
which stopped in batch 0 resumes in batch 1).  The images and gradients of `accumulate` are held to the project's
default bound (tests.util.assert_close, 1e-4 of the reference's maximum), the one test_chain_equals_rasterization
applies to the same gradients."""
import math

import numpy as np
import pytest
import torch

from tests import indices_util as IU
from tests.tile_util import BORDER_CAP
from tests.util import assert_close, record, rel_err

pytestmark = pytest.mark.gpu

TS = (8, 16, 32)
W, H, C = IU.W, IU.H, IU.C


@pytest.fixture(scope="module")
def G():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    import gsplat
    return gsplat


def _inputs(ts, regime):
    name = IU.SCENE_OF[ts]
    m, con, op = (t.cuda() for t in IU.tensors(name, regime))
    offs, flat = (t.cuda() for t in IU.device_lists(name, ts))
    return m, con, op, offs, flat


def _ids(G, ts, regime, r, T=None):
    m, con, op, offs, flat = _inputs(ts, regime)
    T = torch.ones(C, H, W, device="cuda") if T is None else T
    return G.rasterize_to_indices_in_range(r[0], r[1], T, m, con, op, W, H, ts, offs, flat)


def _check_ids(got, want, label):
    """dtypes, the (camera, pixel) order and, outside the call's borderline set, every pixel's segment as a sequence"""
    for t in got:
        assert t.dtype == torch.int64 and t.dim() == 1 and t.shape == got[0].shape
    g = tuple(t.cpu().numpy() for t in got)
    key = g[2] * IU.HW + g[1]
    assert np.all(np.diff(key) >= 0), f"{label}: rows are not in (camera, pixel) order"
    bad = IU.same_segments(g, (want.gaussian_ids, want.pixel_ids, want.camera_ids), ~want.mask)
    record("indices_vs_reference", case=label, rows=int(g[0].size), rows_ref=int(want.gaussian_ids.size),
           borderline=int(want.mask.sum()), bad_pixels=bad)
    assert bad == 0, f"{label}: {bad} non-borderline pixels list other entries than the reference"
    if not want.mask.any():
        assert g[0].size == want.gaussian_ids.size


@pytest.mark.parametrize("regime", IU.REGIMES)
@pytest.mark.parametrize("ts", TS)
def test_full_range(G, ts, regime):
    """(0, 10**10) from T = 1: the reference's lists; int64; ordered; two runs give the same bits."""
    got = _ids(G, ts, regime, IU.FULL)
    _check_ids(got, IU.call(ts, regime, *IU.FULL), f"ts={ts} {regime} full")
    again = _ids(G, ts, regime, IU.FULL)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("r", IU.SLICES, ids=lambda r: f"{r[0]}-{min(r[1], 99)}")
@pytest.mark.parametrize("regime", IU.REGIMES)
@pytest.mark.parametrize("ts", TS)
def test_slices(G, ts, regime, r):
    """A slice of batches from the T the reference carries to it (float64, rounded to fp32, given to both sides).  In
    the thick regime (1, 2) holds pixels that stopped in batch 0 and resume in batch 1: the stop is per call.  At
    (5, 9) every tile is exhausted: three empty int64 tensors."""
    T = torch.from_numpy(IU.start_T(ts, regime, r[0])).cuda()
    got = _ids(G, ts, regime, r, T)
    want = IU.call(ts, regime, *r)
    _check_ids(got, want, f"ts={ts} {regime} {r}")
    if r == (5, 9):
        assert all(t.numel() == 0 for t in got)


def _colors(ts, D):
    return IU.colors(IU.SCENE_OF[ts], D).cuda()


@pytest.mark.parametrize("D", [1, 3, 35])
@pytest.mark.parametrize("regime", IU.REGIMES)
@pytest.mark.parametrize("ts", TS)
def test_accumulate_forward(G, ts, regime, D):
    """`accumulate` on the device's own full-range lists.  Thin regime: against reference (b) on the same lists and
    against rasterize_to_pixels on the same inputs, every pixel.  Thick regime: against rasterize_to_pixels with the
    borderline share allowed (a pixel whose stop falls differently composites another list)."""
    m, con, op, offs, flat = _inputs(ts, regime)
    col = _colors(ts, D)
    ids = _ids(G, ts, regime, IU.FULL)
    renders, alphas = G.accumulate(m, con, op, col, *ids, W, H)
    assert renders.shape == (C, H, W, D) and alphas.shape == (C, H, W, 1)
    r_px, a_px = G.rasterize_to_pixels(m, con, col, op, W, H, ts, offs, flat)
    assert float(a_px.mean()) > 0.05
    e = {"render_vs_pixels": rel_err(renders, r_px), "alphas_vs_pixels": rel_err(alphas, a_px)}
    if regime == "thin":
        r64, a64 = IU.ref_accumulate(m.double().cpu(), con.double().cpu(), op.double().cpu(), col.double().cpu(),
                                     *(t.cpu().numpy() for t in ids))
        e.update(render_vs_ref=rel_err(renders, r64), alphas_vs_ref=rel_err(alphas, a64))
    record("accumulate_forward", tile_size=ts, regime=regime, channels=D, max_rel_err=e)
    cap = 0.0 if regime == "thin" else BORDER_CAP
    if regime == "thin":
        assert_close(renders, r64, name="renders vs reference (b)")
        assert_close(alphas, a64, name="alphas vs reference (b)")
    assert_close(renders, r_px, max_bad=cap, name="renders vs rasterize_to_pixels")
    assert_close(alphas, a_px, max_bad=cap, name="alphas vs rasterize_to_pixels")


@pytest.mark.parametrize("D", [3, 35])
@pytest.mark.parametrize("ts", TS)
def test_accumulate_backward(G, ts, D):
    """Thin regime, random cotangents for renders and alphas: the gradients of means2d, conics, opacities and colors
    against reference (b)'s float64 autograd on the device's lists, and against rasterize_to_pixels' own gradients."""
    regime = "thin"
    m0, con0, op0, offs, flat = _inputs(ts, regime)
    col0 = _colors(ts, D)
    gen = torch.Generator().manual_seed(77)
    wr, wa = torch.rand(C, H, W, D, generator=gen), torch.rand(C, H, W, 1, generator=gen)
    ids = _ids(G, ts, regime, IU.FULL)
    names = ("means2d", "conics", "opacities", "colors")

    def grads(fn, dev, dtype):
        p = [t.detach().to(dev, dtype).clone().requires_grad_(True) for t in (m0, con0, op0, col0)]
        r, a = fn(*p)
        ((r * wr.to(dev, dtype)).sum() + (a * wa.to(dev, dtype)).sum()).backward()
        assert all(t.grad is not None for t in p)
        return dict(zip(names, (t.grad.detach() for t in p)))

    got = grads(lambda m, con, op, col: G.accumulate(m, con, op, col, *ids, W, H), "cuda", torch.float32)
    ids_np = tuple(t.cpu().numpy() for t in ids)
    ref = grads(lambda m, con, op, col: IU.ref_accumulate(m, con, op, col, *ids_np), "cpu", torch.float64)
    pix = grads(lambda m, con, op, col: G.rasterize_to_pixels(m, con, col, op, W, H, ts, offs, flat), "cuda", torch.float32)
    e = {f"{k}_vs_ref": rel_err(got[k], ref[k]) for k in names}
    e.update({f"{k}_vs_pixels": rel_err(got[k], pix[k]) for k in names})
    record("accumulate_backward", tile_size=ts, channels=D, max_rel_err=e)
    for k in names:
        assert float(ref[k].abs().max()) > 0
        assert_close(got[k], ref[k], name=f"grad {k} vs reference (b)")
        assert_close(got[k], pix[k], name=f"grad {k} vs rasterize_to_pixels")


@pytest.mark.parametrize("ts", TS)
def test_slice_loop_equals_rasterize_to_pixels(G, ts):
    """gsplat's use of the pair: one batch per call, accumulate, carry T.  Thin regime, on the device's own binning
    (isect_tiles -> isect_offset_encode) of the scene."""
    name = IU.SCENE_OF[ts]
    sc = IU.scene(name)
    m, con, op = (t.cuda() for t in IU.tensors(name, "thin"))
    col = _colors(ts, 3)
    tw, th = IU.grid(ts)
    radii, depths = torch.from_numpy(sc.radii).cuda(), torch.from_numpy(sc.depths).cuda()
    _tpg, isect_ids, flat = G.isect_tiles(m, radii, depths, ts, tw, th)
    offs = G.isect_offset_encode(isect_ids, C, tw, th)
    T = torch.ones(C, H, W, device="cuda")
    render = torch.zeros(C, H, W, 3, device="cuda")
    alpha = torch.zeros(C, H, W, 1, device="cuda")
    steps = 0
    for step in range(16):
        ids = G.rasterize_to_indices_in_range(step, step + 1, T, m, con, op, W, H, ts, offs, flat)
        if ids[0].numel() == 0:
            break
        r, a = G.accumulate(m, con, op, col, *ids, W, H)
        render = render + r * T[..., None]
        alpha = alpha + a * T[..., None]
        T = T * (1.0 - a[..., 0])
        steps += 1
    else:
        pytest.fail("the loop did not run out of batches")
    assert steps >= 2
    r_px, a_px = G.rasterize_to_pixels(m, con, col, op, W, H, ts, offs, flat)
    assert_close(render, r_px, name="render")
    assert_close(alpha, a_px, name="alphas")


def test_corners(G):
    ts = 16
    name = IU.SCENE_OF[ts]
    sc = IU.scene(name)
    m, con, op, offs, flat = _inputs(ts, "thick")
    ones = torch.ones(C, H, W, device="cuda")
    tw, th = IU.grid(ts)
    # N == 0
    z = lambda *s: torch.zeros(*s, device="cuda")
    got = G.rasterize_to_indices_in_range(0, 10 ** 10, ones, z(C, 0, 2), z(C, 0, 3), z(C, 0), W, H, ts,
                                          torch.zeros(C, th, tw, dtype=torch.int32, device="cuda"),
                                          torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert all(t.dtype == torch.int64 and t.shape == (0,) for t in got)
    # an empty list under offsets that point past it
    got = G.rasterize_to_indices_in_range(0, 10 ** 10, ones, m, con, op, W, H, ts, offs, flat[:0])
    assert all(t.dtype == torch.int64 and t.shape == (0,) for t in got)

    # a camera with all radii 0: its pixels list nothing
    from oracle import ref_torch as O
    ls = []
    for c in range(C):
        radii = sc.radii[c] if c == 0 else np.zeros_like(sc.radii[c])
        _tpg, ids, fl = O.isect_tiles(sc.means2d[c], radii, sc.depths[c], ts, tw, th)
        ls.append(IU.Lists(fl.astype(np.int64), np.concatenate([O.isect_offset_encode(ids, tw, th).reshape(-1).astype(np.int64),
                                                                [fl.shape[0]]])))
    M0 = ls[0].flat.size
    assert ls[1].flat.size == 0 and M0 > 0
    offs1 = torch.from_numpy(np.stack([ls[0].offsets[:-1], np.full(tw * th, M0)]).reshape(C, th, tw).astype(np.int32)).cuda()
    flat1 = torch.from_numpy(ls[0].flat.astype(np.int32)).cuda()
    got = G.rasterize_to_indices_in_range(0, 10 ** 10, ones, m, con, op, W, H, ts, offs1, flat1)
    want = IU.walk_call(sc.means2d, sc.conics, IU.opacities(name, "thick"), ls, ts, 0, 10 ** 10)
    _check_ids(got, want, "camera 1 sees nothing")
    assert got[0].numel() > 0 and int(got[2].max()) == 0

    # offsets beyond the list: they are read clamped into [0, M] (the form rasterize_to_pixels prepares), the call
    # returns, and every row names an entry of the list.  One camera; the last three tiles' offsets point past the end
    o = IU.lists(name, ts)[0]
    M = o.flat.size
    bad = o.offsets[:-1].copy()
    bad[-3:] += 10 ** 6
    offs_bad = torch.from_numpy(bad.reshape(1, th, tw).astype(np.int32)).cuda()
    flat0 = torch.from_numpy(o.flat.astype(np.int32)).cuda()
    got = G.rasterize_to_indices_in_range(0, 10 ** 10, ones[:1], m[:1], con[:1], op[:1], W, H, ts, offs_bad, flat0)
    ls_bad = IU.local_lists(bad.reshape(1, th, tw), o.flat, sc.N)
    assert ls_bad[0].offsets.max() == M
    want = IU.walk_call(sc.means2d[:1], sc.conics[:1], IU.opacities(name, "thick")[:1], ls_bad, ts, 0, 10 ** 10)
    _check_ids(got, want, "offsets beyond the list")
    assert int(got[0].min()) >= 0 and int(got[0].max()) < sc.N and int(got[1].max()) < IU.HW

    # accumulate with M == 0: zeros, and zero gradients
    p = [t.clone().requires_grad_(True) for t in (m, con, op, _colors(ts, 3))]
    e = torch.zeros(0, dtype=torch.int64, device="cuda")
    r, a = G.accumulate(*p, e, e, e, W, H)
    assert r.shape == (C, H, W, 3) and a.shape == (C, H, W, 1) and not r.any() and not a.any()
    (r.sum() + a.sum()).backward()
    assert all(t.grad is not None and not t.grad.any() for t in p)
