"""Colours of any channel count through `rasterization` (the wide entries of csrc/tiles.hip), against a dense PyTorch oracle built
here from oracle.ref_torch's projection, binning and compositing plus gsplat 1.0.0's mode and background rules (autograd
backward).  Scene discipline of the render-mode tests: integer-borderline Gaussians are taken out, pixels within a margin
of a float threshold get zero upstream gradient.  200 x 136 has partial tiles on both edges and tiles deeper than one
256-entry batch.  With several chunks the oracle composites once per chunk on one shared abs-gradient buffer, and the
alpha of the loss is the first chunk's, as in the product."""
import math

import numpy as np
import pytest
import torch

from tests.util import assert_close, borderline_pixel_mask, clean_scene, record, rel_err

pytestmark = pytest.mark.gpu

W, H = 200, 136
WIDE = ("eg_composite_fwd_wide_cams", "eg_composite_bwd_wide_cams")
OLD = ("eg_operator_fwd", "eg_composite_fwd_cams", "eg_composite_bwd_colors", "eg_composite_bwd_footprint_cams",
       "eg_composite_fwd_modes_cams", "eg_composite_bwd_modes_cams")


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    from oracle import c_oracle as CO
    return synth, O, CO


_SCENES = {}


def _setup(env, cams, mode):
    """(clean scene, kept-pixel mask [C,H,W], removed Gaussians) -- computed once per (cameras, rasterize mode)."""
    key = (tuple(cams), mode)
    if key not in _SCENES:
        synth, O, CO = env
        sc0 = synth.make_scene(2500, 5, W, H, seed=0, spread_opacity=True, scale=0.02, anisotropy=5.0)
        sc, removed = clean_scene(sc0, cams)
        N = sc.means.shape[0]
        keep = []
        for v in cams:  # this rasterize_mode's own borderline pixels (the opacities differ between the two modes)
            fw = CO.rasterize(sc.means.numpy(), sc.quats.numpy(), torch.exp(sc.log_scales).numpy(),
                              torch.sigmoid(sc.logit_opacities).squeeze(-1).numpy(), np.ones((N, 1), np.float32),
                              sc.viewmats[v].numpy(), sc.Ks[v].numpy(), W, H, antialiased=(mode == "antialiased"))
            keep.append(~borderline_pixel_mask(fw))
        _SCENES[key] = (sc, torch.stack(keep), removed)
    return _SCENES[key]


def oracle_rasterization(O, means, quats, scales, opacities, colors, viewmats, Ks, width, height, backgrounds=None,
                         render_mode="RGB", absgrad=True, rasterize_mode="antialiased", channel_chunk=32):
    """gsplat 1.0.0 `rasterization` (packed=False) on the CPU for colours of any width, composited chunk by chunk."""
    C, N = viewmats.shape[0], means.shape[0]
    D = colors.shape[-1]
    chunk = min(channel_chunk, 32)
    tw, th = math.ceil(width / 16), math.ceil(height / 16)
    proj = [O.project(means, quats, scales, viewmats[c], Ks[c], width, height) for c in range(C)]
    m2d_all = torch.stack([p[1] for p in proj])
    depths_all = torch.stack([p[2] for p in proj])
    cols = colors.expand(C, N, D) if colors.dim() == 2 else colors
    with_depth = render_mode in ("RGB+D", "RGB+ED")
    renders, alphas, bufs, lasts = [], [], [], []
    for c in range(C):
        radii, _, depths, conics, comp = proj[c]
        op = opacities * comp if rasterize_mode == "antialiased" else opacities
        _tpg, ids, flat = O.isect_tiles(m2d_all[c].detach().numpy(), radii.numpy(), depths.detach().numpy(), 16, tw, th)
        offs = O.isect_offset_encode(ids, tw, th)
        buf = torch.zeros(N, 2) if absgrad else None
        bufs.append(buf)
        parts = []
        for c0 in range(0, D, chunk):
            w = min(chunk, D - c0)
            cc = cols[c][:, c0:c0 + w]
            bg = backgrounds[c, c0:c0 + w] if backgrounds is not None else None
            if with_depth and c0 + w == D:  # the depth channel rides on the last chunk; its background is 0
                cc = torch.cat([cc, depths_all[c][:, None]], dim=-1)
                if bg is not None:
                    bg = torch.cat([bg, torch.zeros(1, dtype=bg.dtype)])
            r, a, last = O.composite(m2d_all[c], conics, cc, op, width, height, 16, offs, flat, buf)
            if bg is not None:
                r = r + (1.0 - a) * bg
            parts.append(r)
            if c0 == 0:  # alphas and last_ids are the first chunk's
                alphas.append(a)
                lasts.append(last)
        renders.append(torch.cat(parts, dim=-1))
    if absgrad and m2d_all.requires_grad:
        def _set_absgrad(grad, t=m2d_all):
            t.absgrad = torch.stack(bufs).clone()
            return None
        m2d_all.register_hook(_set_absgrad)
    render, alpha = torch.stack(renders), torch.stack(alphas)
    if render_mode == "RGB+ED":
        render = torch.cat([render[..., :-1], render[..., -1:] / alpha.clamp(min=1e-10)], dim=-1)
    return render, alpha, {"means2d": m2d_all, "depths": depths_all, "last_ids": torch.stack(lasts)}


def _colors(per_camera, C, N, D):
    g = torch.Generator().manual_seed(11)
    return 0.2 + 0.8 * torch.rand(*((C, N, D) if per_camera else (N, D)), generator=g)


def _gpu_kwargs(sc, cams, col, bg, render_mode, mode, p=None):
    p = p if p is not None else [t.cuda() for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    return dict(means=p[0], quats=p[1], scales=torch.exp(p[2]), opacities=torch.sigmoid(p[3]).squeeze(-1), colors=col,
                viewmats=sc.viewmats[cams].cuda(), Ks=sc.Ks[cams].cuda(), width=W, height=H, backgrounds=bg,
                render_mode=render_mode, absgrad=True, rasterize_mode=mode, tile_size=16, packed=False)


def _run_gpu(sc, cams, colors0, bg0, render_mode, mode, loss_fn, channel_chunk=32):
    from edgegaussians_amd import rasterization
    p = [t.clone().cuda().requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    col = colors0.clone().cuda().requires_grad_(True)
    bg = bg0.clone().cuda().requires_grad_(True) if bg0 is not None else None
    render, alpha, info = rasterization(channel_chunk=channel_chunk, **_gpu_kwargs(sc, cams, col, bg, render_mode, mode, p))
    info["means2d"].retain_grad()
    loss = loss_fn(render, alpha, "cuda")
    loss.backward()
    return dict(render=render, alpha=alpha, info=info, p=p, col=col, bg=bg, loss=loss)


def _run_cpu(env, sc, cams, colors0, bg0, render_mode, mode, loss_fn, channel_chunk=32):
    O = env[1]
    p = [t.clone().requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    col = colors0.clone().requires_grad_(True)
    bg = bg0.clone().requires_grad_(True) if bg0 is not None else None
    render, alpha, info = oracle_rasterization(
        O, means=p[0], quats=p[1], scales=torch.exp(p[2]), opacities=torch.sigmoid(p[3]).squeeze(-1), colors=col,
        viewmats=sc.viewmats[cams], Ks=sc.Ks[cams], width=W, height=H, backgrounds=bg, render_mode=render_mode,
        rasterize_mode=mode, channel_chunk=channel_chunk)
    info["means2d"].retain_grad()
    loss = loss_fn(render, alpha, "cpu")
    loss.backward()
    return dict(render=render, alpha=alpha, info=info, p=p, col=col, bg=bg, loss=loss)


def _loss(wr, keep):
    # (the alpha term: a v_alphas handed to every chunk instead of the first would count it ceil(D / chunk) times)
    return lambda render, alpha, dev: ((render * wr.to(dev)).sum() * 1e-3 +
                                       ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3)


CASES = [  # (D, channel_chunk, render_mode, rasterize_mode, cameras, colours per camera, backgrounds)
    (2, 32, "RGB", "classic", [1], False, False),
    (4, 32, "RGB+D", "antialiased", [0, 2, 3], True, True),
    (5, 32, "RGB", "antialiased", [1], False, True),
    (8, 32, "RGB+ED", "classic", [0, 2, 3], False, False),
    (16, 32, "RGB", "antialiased", [1], True, False),
    (17, 32, "RGB+D", "classic", [1], False, True),
    (32, 32, "RGB", "antialiased", [0, 2, 3], False, True),
    (33, 32, "RGB+ED", "antialiased", [1], False, False),
    (40, 16, "RGB+D", "classic", [1], True, True),
]


@pytest.mark.parametrize("D,chunk,render_mode,mode,cams,per_cam,with_bg", CASES,
                         ids=[f"D{d}-chunk{k}-{r}-{m}-C{len(c)}-{'CND' if pc else 'ND'}-{'bg' if b else 'nobg'}"
                              for d, k, r, m, c, pc, b in CASES])
def test_channels_match_oracle(env, D, chunk, render_mode, mode, cams, per_cam, with_bg, monkeypatch):
    from edgegaussians_amd import rasterizer as R
    sc, keep, removed = _setup(env, cams, mode)
    C, N = len(cams), sc.means.shape[0]
    colors0 = _colors(per_cam, C, N, D)
    bg0 = torch.rand(C, D, generator=torch.Generator().manual_seed(12)) if with_bg else None
    Dout = D + int(render_mode != "RGB")
    wr = torch.rand(C, H, W, Dout, generator=torch.Generator().manual_seed(13)) * keep[..., None]
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])

    loss_fn = _loss(wr, keep)
    cpu = _run_cpu(env, sc, cams, colors0, bg0, render_mode, mode, loss_fn, chunk)
    gpu = _run_gpu(sc, cams, colors0, bg0, render_mode, mode, loss_fn, chunk)
    assert gpu["render"].shape == cpu["render"].shape == (C, H, W, Dout)
    assert gpu["alpha"].shape == (C, H, W, 1)
    ok = keep
    e = {}
    e["render"] = rel_err(gpu["render"].detach().cpu()[ok], cpu["render"].detach()[ok])
    e["alpha"] = rel_err(gpu["alpha"].detach().cpu()[ok], cpu["alpha"].detach()[ok])
    lg, lc = float(gpu["loss"].detach()), float(cpu["loss"].detach())
    e["loss"] = abs(lg - lc) / abs(lc)
    for name, a, b in zip(("means", "quats", "scales", "opacities"), gpu["p"], cpu["p"]):
        e[name] = rel_err(a.grad, b.grad)
    e["colors"] = rel_err(gpu["col"].grad, cpu["col"].grad)
    if with_bg:
        e["backgrounds"] = rel_err(gpu["bg"].grad, cpu["bg"].grad)
    e["v_means2d"] = rel_err(gpu["info"]["means2d"].grad, cpu["info"]["means2d"].grad)
    e["absgrad"] = rel_err(gpu["info"]["means2d"].absgrad, cpu["info"]["means2d"].absgrad)
    print("max relative errors:", e)
    record("channels_vs_torch_oracle", D=D, channel_chunk=chunk, render_mode=render_mode, mode=mode, cameras=C,
           colors_per_camera=per_cam, backgrounds=with_bg, removed_borderline_gaussians=removed,
           borderline_pixels=int((~keep).sum()), max_rel_err=e)

    assert_close(gpu["render"].detach().cpu()[ok], cpu["render"].detach()[ok], name="render")
    assert_close(gpu["alpha"].detach().cpu()[ok], cpu["alpha"].detach()[ok], name="alpha")
    assert torch.equal(gpu["info"]["last_ids"].cpu()[ok], cpu["info"]["last_ids"][ok])
    assert abs(lg - lc) <= 1e-4 * abs(lc)
    for name, a, b in zip(("means", "quats", "scales", "opacities"), gpu["p"], cpu["p"]):
        assert_close(a.grad.cpu(), b.grad, name=f"grad {name}")
    assert gpu["col"].grad.shape == colors0.shape
    assert_close(gpu["col"].grad.cpu(), cpu["col"].grad, name="grad colors")
    if with_bg:
        assert_close(gpu["bg"].grad.cpu(), cpu["bg"].grad, name="grad backgrounds")
    assert_close(gpu["info"]["means2d"].grad.cpu(), cpu["info"]["means2d"].grad, name="v_means2d")
    assert_close(gpu["info"]["means2d"].absgrad.cpu(), cpu["info"]["means2d"].absgrad, name="absgrad")
    # projection, binning and the sort once per call; ceil(D / chunk) launches of each wide entry; no other compositing
    for stage in ("eg_project_fwd_cams", "eg_tile_offsets_cams", "eg_tile_emit_sort_cams", "eg_project_bwd_cams"):
        assert seen.count(stage) == 1, (stage, seen)
    for stage in WIDE:
        assert seen.count(stage) == math.ceil(D / min(chunk, 32)), (stage, seen)
    assert not [n for n in seen if n in OLD], seen


def test_three_channels_record_no_wide_entry(env, monkeypatch):
    from edgegaussians_amd import rasterizer as R
    cams = [1]
    sc, keep, _ = _setup(env, cams, "antialiased")
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    wr = torch.rand(1, H, W, 3, generator=torch.Generator().manual_seed(13))
    _run_gpu(sc, cams, _colors(False, 1, sc.means.shape[0], 3), None, "RGB", "antialiased", _loss(wr, keep))
    assert seen and not [n for n in seen if n in WIDE], seen


def test_chunking_is_invisible(env):
    """D = 16 in one, two and four launches: the same last_ids, everything else within the tolerance; the same `info`
    as the three-channel call on the scene."""
    from edgegaussians_amd import rasterization
    cams = [0, 2, 3]
    sc, keep, _ = _setup(env, cams, "antialiased")
    C, N, D = len(cams), sc.means.shape[0], 16
    colors0 = _colors(False, C, N, D)
    bg0 = torch.rand(C, D, generator=torch.Generator().manual_seed(12))
    wr = torch.rand(C, H, W, D + 1, generator=torch.Generator().manual_seed(13)) * keep[..., None]
    runs = {k: _run_gpu(sc, cams, colors0, bg0, "RGB+D", "antialiased", _loss(wr, keep), channel_chunk=k) for k in (32, 8, 4)}
    ref = runs[32]
    e = {}
    for k in (8, 4):
        r = runs[k]
        assert torch.equal(r["info"]["last_ids"], ref["info"]["last_ids"])
        pairs = {"alpha": (r["alpha"], ref["alpha"]), "render": (r["render"], ref["render"]),
                 "colors": (r["col"].grad, ref["col"].grad), "backgrounds": (r["bg"].grad, ref["bg"].grad),
                 "v_means2d": (r["info"]["means2d"].grad, ref["info"]["means2d"].grad)}
        for name, a, b in zip(("means", "quats", "scales", "opacities"), r["p"], ref["p"]):
            pairs[name] = (a.grad, b.grad)
        e[k] = {n: rel_err(a.detach(), b.detach()) for n, (a, b) in pairs.items()}
        print(f"channel_chunk={k} vs 32, max relative errors:", e[k])
        for n, (a, b) in pairs.items():
            assert_close(a.detach().cpu(), b.detach().cpu(), name=f"chunk {k}: {n}")
    record("channels_chunking_invisible", D=D, max_rel_err={str(k): v for k, v in e.items()})
    with torch.no_grad():
        col3 = _colors(False, C, N, 3).cuda()
        _, _, i3 = rasterization(**_gpu_kwargs(sc, cams, col3, None, "RGB", "antialiased"))
    for k in (32, 8, 4):
        iw = runs[k]["info"]
        assert list(iw.keys()) == list(i3.keys())
        for key in ("radii", "depths", "isect_ids", "flatten_ids", "isect_offsets", "tiles_per_gauss"):
            assert torch.equal(iw[key], i3[key]), key


def test_padding_channels_are_never_touched(env):
    """A five-channel chunk inside eight-wide tensors through the two entries themselves (it runs in the kernels of
    width 8): NaN colours in columns 5..7 reach no result, and render / v_colors keep their sentinels there.  Then the
    same through `rasterization`: eight channels cut 5 + 3, whose first chunk has the second one's data where its
    padding would be."""
    from edgegaussians_amd import rasterization
    from edgegaussians_amd._lib import call, ptr, stream
    cams = [1]
    sc, keep, _ = _setup(env, cams, "classic")
    N, D, S = sc.means.shape[0], 5, 8
    colors0 = _colors(False, 1, N, D)
    wr = torch.rand(1, H, W, D, generator=torch.Generator().manual_seed(13)) * keep[..., None]
    sentinel = torch.full_like(colors0, 7.0).cuda()
    p = [t.clone().cuda() for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
    col = colors0.clone().cuda().requires_grad_(True)
    col.grad = sentinel.clone()  # (autograd adds to it: a write outside the five columns has nowhere to go unseen)
    render, alpha, info = rasterization(**_gpu_kwargs(sc, cams, col, None, "RGB", "classic", p))
    (render * wr.cuda()).sum().backward()
    v_col_ref = col.grad - sentinel
    assert tuple(col.grad.shape) == (N, D) and bool(torch.isfinite(col.grad).all())

    # the same chunk, addressed inside eight-wide tensors
    dev = col.device
    splat = torch.cat([info["means2d"], info["conics"][..., 0:2], info["conics"][..., 2:3], info["opacities"][..., None],
                       info["depths"][..., None], info["radii"].view(torch.float32)[..., None]], dim=-1).detach().contiguous()
    M = info["flatten_ids"].shape[0]
    offsets = torch.cat([info["isect_offsets"].reshape(-1), torch.tensor([M], dtype=torch.int32, device=dev)])[None].contiguous()
    flat = info["flatten_ids"].contiguous()
    wide_col = torch.full((N, S), float("nan"), device=dev)
    wide_col[:, :D] = col.detach()
    wide_render = torch.full((1, H, W, S), -3.0, device=dev)
    alphas = torch.empty(1, H, W, device=dev)
    last = torch.empty(1, H, W, dtype=torch.int32, device=dev)
    call("eg_composite_fwd_wide_cams", 1, ptr(splat), N, ptr(wide_col), 0, D, 0, None, ptr(offsets), ptr(flat), W, H,
         ptr(wide_render), ptr(alphas), ptr(last), D, S, S, stream())
    assert torch.equal(wide_render[..., :D], render.detach())
    assert bool((wide_render[..., D:] == -3.0).all())
    assert torch.equal(alphas[..., None], alpha.detach()) and torch.equal(last, info["last_ids"])
    v_render = torch.full((1, H, W, S), float("nan"), device=dev)
    v_render[..., :D] = wr.cuda()
    g2d = torch.zeros(1, N, 8, device=dev)
    v_col = torch.zeros(1, N, S, device=dev)
    v_col[..., D:] = 7.0
    call("eg_composite_bwd_wide_cams", 1, ptr(splat), N, ptr(wide_col), 0, D, 0, None, ptr(offsets), ptr(flat), W, H,
         ptr(alphas), ptr(last), ptr(v_render), None, ptr(g2d), ptr(v_col), None, D, S, S, stream())
    assert bool((v_col[..., D:] == 7.0).all())
    assert bool(torch.isfinite(g2d).all())
    assert_close(v_col[0, :, :D].cpu(), v_col_ref.cpu(), name="v_colors inside a wider tensor")

    # 8 channels cut 5 + 3 against one launch
    col8 = _colors(False, 1, N, 8)
    wr8 = torch.rand(1, H, W, 8, generator=torch.Generator().manual_seed(14)) * keep[..., None]
    a = _run_gpu(sc, cams, col8, None, "RGB", "classic", _loss(wr8, keep), channel_chunk=32)
    b = _run_gpu(sc, cams, col8, None, "RGB", "classic", _loss(wr8, keep), channel_chunk=5)
    assert_close(b["render"].detach().cpu(), a["render"].detach().cpu(), name="5 + 3: render")
    assert_close(b["col"].grad.cpu(), a["col"].grad.cpu(), name="5 + 3: grad colors")
    for name, x, y in zip(("means", "quats", "scales", "opacities"), b["p"], a["p"]):
        assert_close(x.grad.cpu(), y.grad.cpu(), name=f"5 + 3: grad {name}")


def test_arguments(env):
    from edgegaussians_amd import rasterization
    cams = [1]
    sc, _, _ = _setup(env, cams, "classic")
    N = sc.means.shape[0]
    col = _colors(False, 1, N, 6).cuda()
    for bad in (0, -1, 2.5, "8", None, True):
        with pytest.raises(ValueError, match="channel_chunk"):
            rasterization(channel_chunk=bad, **_gpu_kwargs(sc, cams, col, None, "RGB", "classic"))
    with pytest.raises(ValueError, match="backgrounds must have shape"):
        rasterization(**_gpu_kwargs(sc, cams, col, torch.zeros(1, 3).cuda(), "RGB", "classic"))
    with torch.no_grad():
        render, alpha, _ = rasterization(channel_chunk=4, **_gpu_kwargs(sc, cams, col, None, "RGB", "classic"))
    assert render.shape == (1, H, W, 6) and alpha.shape == (1, H, W, 1)
