"""rasterization(tile_size=8 | 32) (csrc/tiles.hip) against the oracle, which takes the tile size all the way through
(oracle.ref_torch tile_bounds, isect_tiles, composite): parity of every output and gradient, the binning tensors bit for
bit, packed against dense, edge shapes and the routing.  Scene discipline as in the 16-pixel parity tests, formed for
the tile size under test (tests/tile_util.py): tile-box-borderline Gaussians are taken out, pixels within a margin of a
float threshold get zero upstream gradient, both sets are capped."""
import math

import numpy as np
import pytest
import torch

from tests import tile_util as TU
from tests.util import assert_close, record, rel_err

pytestmark = pytest.mark.gpu

W, H = TU.SCENE_ARGS["width"], TU.SCENE_ARGS["height"]
NEW = ("eg_tile_count_ts", "eg_tile_emit_sort_ts", "eg_composite_fwd_ts_cams", "eg_composite_bwd_ts_cams")


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    return synth, O


def oracle_rasterization(O, ts, means, quats, scales, opacities, colors, viewmats, Ks, width, height, backgrounds=None,
                         render_mode="RGB", absgrad=True, rasterize_mode="antialiased", channel_chunk=32):
    """tests/test_gpu_render_modes.py's oracle_rasterization with `ts` in place of its three 16s -- gsplat 1.0.0
    `rasterization` (packed=False) on the CPU from ref_torch's projection, binning and compositing.  The colours are
    composited in chunks of `channel_chunk` channels with the depth channel on the last one, as
    tests/test_gpu_channels.py's oracle does: with one chunk (every case but the wide ones) that is the render-modes
    oracle to the letter, with several the abs-gradient is the sum of the chunks' abs-gradients, which is what
    `rasterization` documents for D > channel_chunk."""
    C, N = viewmats.shape[0], means.shape[0]
    D = colors.shape[-1]
    chunk = min(channel_chunk, 32)
    tw, th = math.ceil(width / ts), math.ceil(height / ts)
    proj = [O.project(means, quats, scales, viewmats[c], Ks[c], width, height) for c in range(C)]
    m2d_all = torch.stack([p[1] for p in proj])
    depths_all = torch.stack([p[2] for p in proj])
    cols = colors.expand(C, N, D) if colors.dim() == 2 else colors
    with_depth = render_mode in ("RGB+D", "RGB+ED")
    renders, alphas, bufs, lasts = [], [], [], []
    for c in range(C):
        radii, _, depths, conics, comp = proj[c]
        op = opacities * comp if rasterize_mode == "antialiased" else opacities
        _tpg, ids, flat = O.isect_tiles(m2d_all[c].detach().numpy(), radii.numpy(), depths.detach().numpy(), ts, tw, th)
        offs = O.isect_offset_encode(ids, tw, th)
        buf = torch.zeros(N, 2) if absgrad else None
        bufs.append(buf)
        if render_mode in ("D", "ED"):  # the depth is the only channel, its background is 0
            pieces = [(depths_all[c][:, None], None)]
        else:
            pieces = []
            for c0 in range(0, D, chunk):
                w = min(chunk, D - c0)
                cc = cols[c][:, c0:c0 + w]
                bg = backgrounds[c, c0:c0 + w] if backgrounds is not None else None
                if with_depth and c0 + w == D:
                    cc = torch.cat([cc, depths_all[c][:, None]], dim=-1)
                    if bg is not None:
                        bg = torch.cat([bg, torch.zeros(1, dtype=bg.dtype)])
                pieces.append((cc, bg))
        parts = []
        for k, (cc, bg) in enumerate(pieces):
            r, a, last = O.composite(m2d_all[c], conics, cc, op, width, height, ts, offs, flat, buf)
            if bg is not None:
                r = r + (1.0 - a) * bg
            parts.append(r)
            if k == 0:  # alphas and last_ids are the first chunk's
                alphas.append(a)
                lasts.append(last)
        renders.append(torch.cat(parts, dim=-1))
    if absgrad and m2d_all.requires_grad:
        def _set_absgrad(grad, t=m2d_all):
            t.absgrad = torch.stack(bufs).clone()
            return None
        m2d_all.register_hook(_set_absgrad)
    render, alpha = torch.stack(renders), torch.stack(alphas)
    if render_mode in ("ED", "RGB+ED"):
        render = torch.cat([render[..., :-1], render[..., -1:] / alpha.clamp(min=1e-10)], dim=-1)
    return render, alpha, {"means2d": m2d_all, "depths": depths_all, "last_ids": torch.stack(lasts)}


def _setup(ts, cams, mode):
    """The shared, cached scene of (ts, cameras, rasterize_mode) with its caps and the multi-batch condition asserted."""
    from edgegaussians_amd import _lib
    sc, keep, removed, n0, longest, stopped = TU.setup(ts, tuple(cams), mode)
    assert removed <= TU.removed_cap(n0), (removed, n0)
    assert float((~keep).float().mean()) < TU.BORDER_CAP
    assert longest > 2 * _lib.TS_STAGE_BATCH[ts], (longest, ts)   # the walk of the fullest tile takes several batches
    assert stopped > 0                                            # ... and the transmittance stop is exercised
    return sc, keep, removed


def _colors(kind, C, N):
    g = torch.Generator().manual_seed(11)
    shape = {"N3": (N, 3), "N1": (N, 1), "CN3": (C, N, 3), "N5": (N, 5), "CN5": (C, N, 5)}[kind]
    return 0.2 + 0.8 * torch.rand(*shape, generator=g)


def _kw(sc, cams, dev, p, col, bg, render_mode, mode):
    return dict(means=p[0], quats=p[1], scales=torch.exp(p[2]), opacities=torch.sigmoid(p[3]).squeeze(-1), colors=col,
                viewmats=sc.viewmats[cams].to(dev), Ks=sc.Ks[cams].to(dev), width=sc.width, height=sc.height, backgrounds=bg,
                render_mode=render_mode, absgrad=True, rasterize_mode=mode)


def _run(env, ts, sc, cams, colors0, bg0, render_mode, mode, loss_fn, chunk=32, seen=None):
    synth, O = env
    from edgegaussians_amd import rasterization
    outs = []
    for dev in ("cpu", "cuda"):
        p = [t.clone().to(dev).requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
        col = colors0.clone().to(dev).requires_grad_(True)
        bg = bg0.clone().to(dev).requires_grad_(True) if bg0 is not None else None
        kw = _kw(sc, cams, dev, p, col, bg, render_mode, mode)
        if dev == "cpu":
            render, alpha, info = oracle_rasterization(O, ts, channel_chunk=chunk, **kw)
        else:
            if seen is not None:
                seen.clear()
            render, alpha, info = rasterization(tile_size=ts, packed=False, channel_chunk=chunk, **kw)
        info["means2d"].retain_grad()
        loss = loss_fn(render, alpha, dev)
        loss.backward()
        outs.append(dict(render=render, alpha=alpha, info=info, p=p, col=col, bg=bg, loss=loss))
    return outs


CASES = [  # (render_mode, rasterize_mode, cameras, colours, backgrounds, channel_chunk)
    ("RGB", "antialiased", [1], "N3", False, 32),
    ("RGB", "classic", [0, 2, 3], "CN3", True, 32),
    ("RGB", "antialiased", [0, 2, 3], "N1", True, 32),
    ("RGB", "classic", [1], "N5", False, 2),            # three chunks, the last one ragged
    ("RGB+D", "antialiased", [0, 2, 3], "CN5", True, 2),  # ... with the depth channel on the last chunk
    ("RGB+ED", "classic", [1], "N3", False, 32),
    ("ED", "antialiased", [1], "N3", True, 32),
    ("D", "classic", [0, 2, 3], "N1", False, 32),
]


@pytest.mark.parametrize("ts", [8, 32])
@pytest.mark.parametrize("render_mode,mode,cams,ckind,with_bg,chunk", CASES,
                         ids=[f"{r}-{m}-C{len(c)}-{k}-{'bg' if b else 'nobg'}-chunk{ch}" for r, m, c, k, b, ch in CASES])
def test_tile_sizes_match_oracle(env, ts, render_mode, mode, cams, ckind, with_bg, chunk, monkeypatch):
    """Every element at tests.util.assert_close's default (1e-4): render and alphas on the kept pixels, the loss, the
    gradients of every input, means2d's grad and absgrad; last_ids exact on the kept pixels."""
    from edgegaussians_amd import rasterizer as R
    sc, keep, removed = _setup(ts, cams, mode)
    C, N = len(cams), sc.means.shape[0]
    colors0 = _colors(ckind, C, N)
    D = colors0.shape[-1]
    bg0 = torch.rand(C, D, generator=torch.Generator().manual_seed(12)) if with_bg else None
    depth = render_mode != "RGB"
    colourless = render_mode in ("D", "ED")
    Dout = (0 if colourless else D) + int(depth)
    wr = torch.rand(C, H, W, Dout, generator=torch.Generator().manual_seed(13)) * keep[..., None]
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])

    def loss_fn(render, alpha, dev):
        return (render * wr.to(dev)).sum() * 1e-3 + ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3

    cpu, gpu = _run(env, ts, sc, cams, colors0, bg0, render_mode, mode, loss_fn, chunk=chunk, seen=seen)
    assert gpu["render"].shape == cpu["render"].shape == (C, H, W, Dout)
    assert gpu["alpha"].shape == (C, H, W, 1)
    gi = gpu["info"]
    assert (gi["tile_size"], gi["tile_width"], gi["tile_height"]) == (ts, math.ceil(W / ts), math.ceil(H / ts))
    ok = keep
    e = {}
    e["render"] = rel_err(gpu["render"].detach().cpu()[ok], cpu["render"].detach()[ok])
    e["alpha"] = rel_err(gpu["alpha"].detach().cpu()[ok], cpu["alpha"].detach()[ok])
    e["loss"] = abs(float(gpu["loss"].detach()) - float(cpu["loss"].detach())) / abs(float(cpu["loss"].detach()))
    grads = [(name, a.grad, b.grad) for name, a, b in zip(("means", "quats", "scales", "opacities"), gpu["p"], cpu["p"])]
    if not colourless:
        grads.append(("colors", gpu["col"].grad, cpu["col"].grad))
        if with_bg:
            grads.append(("backgrounds", gpu["bg"].grad, cpu["bg"].grad))
    grads.append(("v_means2d", gi["means2d"].grad, cpu["info"]["means2d"].grad))
    grads.append(("absgrad", gi["means2d"].absgrad, cpu["info"]["means2d"].absgrad))
    for name, a, b in grads:
        e[name] = rel_err(a, b)
    last_equal = bool(torch.equal(gi["last_ids"].cpu()[ok], cpu["info"]["last_ids"][ok]))
    print(f"ts={ts} {render_mode} {mode} C={C} {ckind} bg={with_bg} chunk={chunk}: removed={removed} "
          f"borderline={int((~keep).sum())} last_ids_equal={last_equal} errors={e}")
    record("tile_size_vs_torch_oracle", tile_size=ts, render_mode=render_mode, mode=mode, cameras=C, colors=ckind,
           backgrounds=with_bg, channel_chunk=chunk, removed_borderline_gaussians=removed,
           borderline_pixels=int((~keep).sum()), last_ids_equal=last_equal, max_rel_err=e)
    assert_close(gpu["render"].detach().cpu()[ok], cpu["render"].detach()[ok], name="render")
    assert_close(gpu["alpha"].detach().cpu()[ok], cpu["alpha"].detach()[ok], name="alpha")
    assert abs(float(gpu["loss"]) - float(cpu["loss"])) <= 1e-4 * abs(float(cpu["loss"]))
    for name, a, b in grads:
        assert_close(a.cpu(), b, name=f"grad {name}")
    if colourless:  # the colours take no part; gsplat replaces the backgrounds with zeros
        assert gpu["col"].grad is None and cpu["col"].grad is None
        assert not with_bg or (gpu["bg"].grad is None and cpu["bg"].grad is None)
    assert last_equal, "last_ids differ on kept pixels"
    # one native call per stage for the C cameras (compositing: per chunk), none of the 16-pixel entries behind the projection
    n_chunks = 1 if colourless else math.ceil(D / min(chunk, 32))
    want = {"eg_project_fwd_cams": 1, "eg_tile_count_ts": 1, "eg_tile_offsets_cams": 1, "eg_tile_emit_sort_ts": 1,
            "eg_composite_fwd_ts_cams": n_chunks, "eg_composite_bwd_ts_cams": n_chunks, "eg_project_bwd_cams": 1}
    assert {n: seen.count(n) for n in set(seen)} == want, seen


def _expected_binning(O, info, ts, width, height, rows):
    """ref_torch's binning on the call's own means2d / radii / depths (host copies): integer work on identical floats.
    rows: per camera the (start, end) of its entries in the flat per-Gaussian tensors."""
    tw, th = math.ceil(width / ts), math.ceil(height / ts)
    tile_bits = int(math.floor(math.log2(tw * th))) + 1
    m2d = info["means2d"].detach().cpu().reshape(-1, 2).numpy()
    radii = info["radii"].cpu().reshape(-1).numpy()
    depths = info["depths"].detach().cpu().reshape(-1).numpy()
    tpg, ids, flat, offs, base = [], [], [], [], 0
    for c, (a, b) in enumerate(rows):
        t, i, f = O.isect_tiles(m2d[a:b], radii[a:b], depths[a:b], ts, tw, th)
        tpg.append(t)
        ids.append(i | (c << (32 + tile_bits)))
        flat.append(f.astype(np.int64) + a)
        offs.append(O.isect_offset_encode(i, tw, th).astype(np.int64) + base)
        base += i.shape[0]
    return (np.concatenate(tpg), np.concatenate(ids), np.concatenate(flat), np.stack(offs), tw, th)


def _assert_binning(O, info, ts, width, height, rows):
    tpg, ids, flat, offs, tw, th = _expected_binning(O, info, ts, width, height, rows)
    assert (info["tile_size"], info["tile_width"], info["tile_height"]) == (ts, tw, th)
    assert np.array_equal(info["tiles_per_gauss"].cpu().reshape(-1).numpy(), tpg)
    assert np.array_equal(info["isect_ids"].cpu().numpy(), ids)
    assert np.array_equal(info["flatten_ids"].cpu().numpy().astype(np.int64), flat)
    assert info["isect_offsets"].shape == offs.shape and np.array_equal(info["isect_offsets"].cpu().numpy(), offs)
    return int(ids.shape[0])


def _plain_kw(sc, cams, colors):
    return dict(means=sc.means.cuda(), quats=sc.quats.cuda(), scales=torch.exp(sc.log_scales).cuda(),
                opacities=torch.sigmoid(sc.logit_opacities).squeeze(-1).cuda(), colors=colors.cuda(),
                viewmats=sc.viewmats[cams].cuda(), Ks=sc.Ks[cams].cuda(), width=sc.width, height=sc.height)


@pytest.mark.parametrize("ts", [8, 16, 32])
@pytest.mark.parametrize("cams", [[1], [0, 2, 3]], ids=["C1", "C3"])
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_binning_bit_for_bit(env, ts, cams, packed):
    from edgegaussians_amd import rasterization
    synth, O = env
    sc = TU.scene()
    N, C = sc.means.shape[0], len(cams)
    with torch.no_grad():
        _r, _a, info = rasterization(tile_size=ts, packed=packed, **_plain_kw(sc, cams, _colors("N3", C, N)))
    if packed:
        cid = info["camera_ids"].cpu().numpy()
        bounds = np.searchsorted(cid, np.arange(C + 1))
        rows = [(int(bounds[c]), int(bounds[c + 1])) for c in range(C)]
    else:
        rows = [(c * N, (c + 1) * N) for c in range(C)]
    M = _assert_binning(O, info, ts, sc.width, sc.height, rows)
    assert M > 0


@pytest.mark.parametrize("ts,width,height", [(8, 1024, 1032), (8, 1024, 768), (16, 2048, 2064), (16, 2048, 1536)],
                         ids=["16512-tiles", "12288-tiles", "ts16-16512-tiles", "ts16-12288-tiles"])
def test_binning_beyond_the_lds_histogram(env, ts, width, height):
    """16 512 tiles (ts = 8 on 1024 x 1032, ts = 16 on 2048 x 2064): more than the counting kernel's LDS histogram holds
    (direct atomics in the counting and the emission); 12 288 tiles (1024 x 768, 2048 x 1536): LDS counting with
    direct-atomic emission.  The scene's Gaussians are sized in world units, so the 16-pixel cases on images twice as
    large keep the 8-pixel cases' `scale`: the same boxes in tiles (the oracle's own M > N, checked on the CPU)."""
    from edgegaussians_amd import rasterization
    synth, O = env
    sc = synth.make_scene(3000, 2, width, height, seed=1, spread_opacity=True, scale=0.004)
    N = sc.means.shape[0]
    with torch.no_grad():
        _r, _a, info = rasterization(tile_size=ts, packed=False, **_plain_kw(sc, [0], _colors("N3", 1, N)))
    assert info["tile_width"] * info["tile_height"] == (width // ts) * math.ceil(height / ts)
    M = _assert_binning(O, info, ts, width, height, [(0, N)])
    assert M > N


@pytest.mark.parametrize("ts", [8, 32])
def test_packed_equals_dense(env, ts):
    from edgegaussians_amd import rasterization
    cams = [0, 2, 3]
    sc, keep, _ = _setup(ts, cams, "antialiased")
    C, N = len(cams), sc.means.shape[0]
    colors0 = _colors("N3", C, N)
    bg0 = torch.rand(C, 3, generator=torch.Generator().manual_seed(12))
    wr = (torch.rand(C, H, W, 4, generator=torch.Generator().manual_seed(13)) * keep[..., None]).cuda()
    out = {}
    for name, packed, sparse in (("dense", False, False), ("packed", True, False), ("sparse", True, True)):
        p = [t.clone().cuda().requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
        col = colors0.clone().cuda().requires_grad_(True)
        bg = bg0.clone().cuda().requires_grad_(True)
        render, alpha, info = rasterization(tile_size=ts, packed=packed, sparse_grad=sparse,
                                            **_kw(sc, cams, "cuda", p, col, bg, "RGB+D", "antialiased"))
        ((render * wr).sum() * 1e-3 + (alpha ** 2).sum() * 1e-3).backward()
        out[name] = dict(render=render.detach(), alpha=alpha.detach(), info=info, p=p, col=col, bg=bg)
    d = out["dense"]
    for name in ("packed", "sparse"):
        q = out[name]
        assert torch.equal(q["render"], d["render"]) and torch.equal(q["alpha"], d["alpha"]), name
        assert torch.equal(q["info"]["last_ids"], d["info"]["last_ids"]), name
        cid, gid = q["info"]["camera_ids"], q["info"]["gaussian_ids"]
        assert cid.shape[0] == int((d["info"]["radii"] > 0).sum()) > 0
        for k in ("radii", "means2d", "depths", "conics", "opacities", "tiles_per_gauss"):
            assert torch.equal(q["info"][k].detach(), d["info"][k].detach()[cid, gid]), (name, k)
        assert q["info"]["tile_size"] == ts and q["info"]["isect_offsets"].shape == d["info"]["isect_offsets"].shape
        assert torch.equal(q["info"]["isect_offsets"], d["info"]["isect_offsets"])
        assert torch.equal(q["info"]["isect_ids"], d["info"]["isect_ids"])
        e = {}
        for k, a, b in zip(("means", "quats", "scales", "opacities"), q["p"], d["p"]):
            g = a.grad.to_dense() if a.grad.is_sparse else a.grad
            assert (name == "sparse" and k != "opacities") == a.grad.is_sparse, (name, k)
            e[k] = rel_err(g, b.grad)
            assert_close(g.cpu(), b.grad.cpu(), name=f"{name} grad {k}")
        assert_close(q["col"].grad.cpu(), d["col"].grad.cpu(), name=f"{name} grad colors")
        assert_close(q["bg"].grad.cpu(), d["bg"].grad.cpu(), name=f"{name} grad backgrounds")
        record("tile_size_packed_vs_dense", tile_size=ts, layout=name, max_rel_err=e)


def test_one_partial_tile(env):
    """20 x 9 at ts = 32: one tile, two of whose four 16 x 16 quadrants hold pixels, neither of them whole."""
    synth, O = env
    from edgegaussians_amd import rasterization
    sc0 = synth.make_scene(300, 2, 20, 9, seed=2, spread_opacity=True, scale=0.05, anisotropy=3.0)
    sc, _removed = TU.clean_scene_ts(sc0, [0], 32)
    keep = ~TU.borderline_pixels_ts(sc, 0, 32, False)[0]
    assert float(keep.float().mean()) > 0.95
    N = sc.means.shape[0]
    colors0 = _colors("N3", 1, N)
    wr = torch.rand(1, 9, 20, 3, generator=torch.Generator().manual_seed(13)) * keep[None, ..., None]
    res = []
    for dev in ("cpu", "cuda"):
        p = [t.clone().to(dev).requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
        kw = _kw(sc, [0], dev, p, colors0.clone().to(dev), None, "RGB", "classic")
        if dev == "cpu":
            render, alpha, info = oracle_rasterization(O, 32, **kw)
        else:
            render, alpha, info = rasterization(tile_size=32, packed=False, **kw)
            assert (info["tile_width"], info["tile_height"]) == (1, 1) and info["isect_offsets"].shape == (1, 1, 1)
        ((render * wr.to(dev)).sum() * 1e-3 + ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3).backward()
        res.append((render.detach().cpu()[0][keep], alpha.detach().cpu()[0][keep], [t.grad.cpu() for t in p],
                    info["last_ids"].cpu()[0][keep]))
    (rc, ac, gc, lc), (rg, ag, gg, lg) = res
    assert float(ac.max()) > 0.1  # something is drawn
    e = {"render": rel_err(rg, rc), "alpha": rel_err(ag, ac)}
    for k, a, b in zip(("means", "quats", "scales", "opacities"), gg, gc):
        e[k] = rel_err(a, b)
    print("20x9 at ts=32:", e)
    record("tile_size_one_partial_tile", borderline_pixels=int((~keep).sum()), max_rel_err=e)
    assert_close(rg, rc, name="render")
    assert_close(ag, ac, name="alpha")
    assert torch.equal(lg, lc)
    for k, a, b in zip(("means", "quats", "scales", "opacities"), gg, gc):
        assert_close(a, b, name=f"grad {k}")


def test_packed_call_without_visible_pairs(env):
    from edgegaussians_amd import rasterization
    sc = TU.scene()
    cams = [0, 2]
    C, N = len(cams), sc.means.shape[0]
    p = [t.clone().cuda().requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    col = _colors("N3", C, N).cuda().requires_grad_(True)
    bg = torch.rand(C, 3, generator=torch.Generator().manual_seed(12)).cuda().requires_grad_(True)
    kw = _kw(sc, cams, "cuda", p, col, bg, "RGB+D", "antialiased")
    render, alpha, info = rasterization(tile_size=8, packed=True, near_plane=1e6, **kw)  # everything in front of the near plane
    assert info["camera_ids"].shape == (0,) and info["gaussian_ids"].shape == (0,)
    assert info["means2d"].shape == (0, 2) and info["radii"].shape == (0,) and info["tiles_per_gauss"].shape == (0,)
    assert info["flatten_ids"].shape == (0,) and info["isect_ids"].shape == (0,)
    assert info["tile_size"] == 8 and info["isect_offsets"].shape == (C, math.ceil(H / 8), math.ceil(W / 8))
    assert not info["isect_offsets"].any()
    assert not alpha.detach().any() and not info["last_ids"].any()
    assert torch.equal(render.detach()[..., :3], bg.detach()[:, None, None, :].expand(C, H, W, 3))
    assert not render.detach()[..., 3].any()
    (render.sum() + alpha.sum()).backward()
    for t in p + [col]:
        assert t.grad is not None and not t.grad.any()
    assert torch.equal(bg.grad, torch.full((C, 3), float(H * W), device="cuda"))


def test_other_tile_sizes_are_refused(env):
    from edgegaussians_amd import rasterization
    sc = TU.scene()
    kw = _plain_kw(sc, [1], _colors("N3", 1, sc.means.shape[0]))
    for packed in (False, True):
        with pytest.raises(NotImplementedError, match=r"8, 16 or 32"):
            rasterization(tile_size=12, packed=packed, **kw)


def test_routing(env, monkeypatch):
    """ts = 8 never reaches a 16-pixel compositing entry or the fast path and makes one call per stage for three cameras;
    tile_size = 16 names exactly the entries it names without the argument."""
    from edgegaussians_amd import rasterization
    from edgegaussians_amd import rasterizer as R
    sc = TU.scene()
    cams = [0, 2, 3]
    C, N = len(cams), sc.means.shape[0]
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])

    def names(colors, packed, **extra):
        seen.clear()
        p = sc.means.clone().cuda().requires_grad_(True)
        kw = _plain_kw(sc, cams, colors)
        kw["means"] = p
        render, alpha, _info = rasterization(packed=packed, **kw, **extra)
        (render.sum() + alpha.sum()).backward()
        return list(seen)

    old = ("eg_operator_fwd", "eg_operator_bwd", "eg_composite_fwd_cams", "eg_composite_bwd_colors",
           "eg_composite_bwd_footprint_cams", "eg_composite_fwd_modes_cams", "eg_composite_bwd_modes_cams",
           "eg_composite_fwd_wide_cams", "eg_composite_bwd_wide_cams", "eg_tile_emit_sort_cams", "eg_packed_bin",
           "eg_tile_count", "eg_tile_emit")
    unit = torch.ones(N, 3)  # the reference's own colours: at 16 they take the unit-colour kernels
    for colors in (unit, _colors("N3", C, N)):
        got = names(colors, False, tile_size=8)
        assert not [n for n in got if n in old], got
        assert got == ["eg_project_fwd_cams", "eg_tile_count_ts", "eg_tile_offsets_cams", "eg_tile_emit_sort_ts",
                       "eg_composite_fwd_ts_cams", "eg_composite_bwd_ts_cams", "eg_project_bwd_cams"], got
    got = names(_colors("N3", C, N), True, tile_size=8)
    assert not [n for n in got if n in old], got
    assert got == ["eg_packed_count", "eg_packed_write", "eg_tile_count_ts", "eg_tile_offsets_cams", "eg_tile_emit_sort_ts",
                   "eg_composite_fwd_ts_cams", "eg_composite_bwd_ts_cams", "eg_packed_bwd"], got
    # one camera, unit colours: the fast path at 16 (and by default), the general path at 8
    for colors, packed, extra in ((unit, False, {}), (_colors("N3", C, N), False, {}), (_colors("N5", C, N), False, {}),
                                  (_colors("N3", C, N), True, {}), (unit, False, {"render_mode": "RGB+D"})):
        with_arg = names(colors, packed, tile_size=16, **extra)
        without = names(colors, packed, **extra)
        assert with_arg == without and not [n for n in with_arg if n in NEW], (with_arg, without)
    # one camera with the reference's own unit colours: the general path at 8, whatever 16 takes
    seen.clear()
    with torch.no_grad():
        rasterization(packed=False, tile_size=8, **_plain_kw(sc, [1], unit))
    assert "eg_operator_fwd" not in seen and seen.count("eg_composite_fwd_ts_cams") == 1, seen
