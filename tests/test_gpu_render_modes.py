"""gsplat's render modes ("D", "ED", "RGB+D", "RGB+ED") and backgrounds through `rasterization`, against a dense PyTorch
oracle built here from oracle.ref_torch's projection, binning and compositing plus gsplat 1.0.0's mode and background
rules (autograd backward).  Same scene discipline as the three-camera parity test: integer-borderline Gaussians are
taken out, pixels within a margin of a float threshold get zero upstream gradient."""
import math

import numpy as np
import pytest
import torch

from tests.util import assert_close, borderline_pixel_mask, clean_scene, record, rel_err

pytestmark = pytest.mark.gpu

W, H = 200, 136


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    from oracle import c_oracle as CO
    return synth, O, CO


def oracle_rasterization(O, means, quats, scales, opacities, colors, viewmats, Ks, width, height, backgrounds=None,
                         render_mode="RGB", absgrad=True, rasterize_mode="antialiased"):
    """gsplat 1.0.0 `rasterization` (packed=False) on the CPU: ref_torch's pieces + the render-mode / background rules."""
    C, N = viewmats.shape[0], means.shape[0]
    tw, th = math.ceil(width / 16), math.ceil(height / 16)
    proj = [O.project(means, quats, scales, viewmats[c], Ks[c], width, height) for c in range(C)]
    m2d_all = torch.stack([p[1] for p in proj])
    depths_all = torch.stack([p[2] for p in proj])
    cols = colors.expand(C, N, colors.shape[-1]) if colors.dim() == 2 else colors
    bgs = backgrounds
    if render_mode in ("RGB+D", "RGB+ED"):
        cols = torch.cat([cols, depths_all[..., None]], dim=-1)
        if bgs is not None:
            bgs = torch.cat([bgs, torch.zeros(C, 1, dtype=bgs.dtype)], dim=-1)
    elif render_mode in ("D", "ED"):
        cols = depths_all[..., None]
        if bgs is not None:
            bgs = torch.zeros(C, 1, dtype=bgs.dtype)
    renders, alphas, bufs, lasts = [], [], [], []
    for c in range(C):
        radii, _, depths, conics, comp = proj[c]
        op = opacities * comp if rasterize_mode == "antialiased" else opacities
        _tpg, ids, flat = O.isect_tiles(m2d_all[c].detach().numpy(), radii.numpy(), depths.detach().numpy(), 16, tw, th)
        offs = O.isect_offset_encode(ids, tw, th)
        buf = torch.zeros(N, 2) if absgrad else None
        bufs.append(buf)
        r, a, last = O.composite(m2d_all[c], conics, cols[c], op, width, height, 16, offs, flat, buf)
        if bgs is not None:
            r = r + (1.0 - a) * bgs[c]
        renders.append(r)
        alphas.append(a)
        lasts.append(last)
    if absgrad and m2d_all.requires_grad:
        def _set_absgrad(grad, t=m2d_all):
            t.absgrad = torch.stack(bufs).clone()
            return None
        m2d_all.register_hook(_set_absgrad)
    render, alpha = torch.stack(renders), torch.stack(alphas)
    if render_mode in ("ED", "RGB+ED"):
        render = torch.cat([render[..., :-1], render[..., -1:] / alpha.clamp(min=1e-10)], dim=-1)
    return render, alpha, {"means2d": m2d_all, "depths": depths_all, "last_ids": torch.stack(lasts)}


def _setup(env, cams, mode):
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
    return sc, torch.stack(keep), removed


def _colors(kind, C, N):
    g = torch.Generator().manual_seed(11)
    shape = {"N3": (N, 3), "N1": (N, 1), "CN3": (C, N, 3)}[kind]
    return 0.2 + 0.8 * torch.rand(*shape, generator=g)


def _run(env, sc, cams, colors0, bg0, render_mode, mode, loss_fn, colors_grad=True, seen=None):
    synth, O, CO = env
    from edgegaussians_amd import rasterization
    outs = []
    for dev in ("cpu", "cuda"):
        p = [t.clone().to(dev).requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
        col = colors0.clone().to(dev).requires_grad_(colors_grad)
        bg = bg0.clone().to(dev).requires_grad_(True) if bg0 is not None else None
        kw = dict(means=p[0], quats=p[1], scales=torch.exp(p[2]), opacities=torch.sigmoid(p[3]).squeeze(-1), colors=col,
                  viewmats=sc.viewmats[cams].to(dev), Ks=sc.Ks[cams].to(dev), width=W, height=H, backgrounds=bg,
                  render_mode=render_mode, absgrad=True, rasterize_mode=mode)
        if dev == "cpu":
            render, alpha, info = oracle_rasterization(O, **kw)
        else:
            if seen is not None:
                seen.clear()
            render, alpha, info = rasterization(tile_size=16, packed=False, **kw)
        info["means2d"].retain_grad()
        loss = loss_fn(render, alpha, dev)
        loss.backward()
        outs.append(dict(render=render, alpha=alpha, info=info, p=p, col=col, bg=bg, loss=loss))
    return outs


CASES = [  # (render_mode, rasterize_mode, cameras, colours, backgrounds)
    ("RGB+D", "antialiased", [1], "N3", False),
    ("RGB+D", "classic", [0, 2, 3], "CN3", True),
    ("RGB+D", "antialiased", [0, 2, 3], "N1", False),
    ("RGB+ED", "antialiased", [0, 2, 3], "N1", True),
    ("RGB+ED", "classic", [1], "N3", False),
    ("D", "antialiased", [0, 2, 3], "N3", False),
    ("D", "classic", [1], "N1", True),
    ("ED", "antialiased", [1], "CN3", True),
    ("ED", "classic", [0, 2, 3], "N3", False),
    ("RGB", "antialiased", [1], "N1", True),
    ("RGB", "classic", [0, 2, 3], "CN3", True),
    ("RGB", "antialiased", [0, 2, 3], "N3", True),
]


@pytest.mark.parametrize("render_mode,mode,cams,ckind,with_bg", CASES,
                         ids=[f"{r}-{m}-C{len(c)}-{k}-{'bg' if b else 'nobg'}" for r, m, c, k, b in CASES])
def test_render_modes_match_oracle(env, render_mode, mode, cams, ckind, with_bg, monkeypatch):
    from edgegaussians_amd import rasterizer as R
    sc, keep, removed = _setup(env, cams, mode)
    C, N = len(cams), sc.means.shape[0]
    colors0 = _colors(ckind, C, N)
    D = colors0.shape[-1]
    bg0 = torch.rand(C, D, generator=torch.Generator().manual_seed(12)) if with_bg else None
    depth = render_mode != "RGB"
    Dout = (0 if render_mode in ("D", "ED") else D) + int(depth)
    wr = torch.rand(C, H, W, Dout, generator=torch.Generator().manual_seed(13)) * keep[..., None]
    seen = []
    real_call = R.call
    monkeypatch.setattr(R, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])

    def loss_fn(render, alpha, dev):
        return (render * wr.to(dev)).sum() * 1e-3 + ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3

    cpu, gpu = _run(env, sc, cams, colors0, bg0, render_mode, mode, loss_fn, seen=seen)
    assert gpu["render"].shape == cpu["render"].shape == (C, H, W, Dout)
    assert gpu["alpha"].shape == (C, H, W, 1)
    ok = keep
    e = {}
    e["render"] = rel_err(gpu["render"].detach().cpu()[ok], cpu["render"].detach()[ok])
    e["alpha"] = rel_err(gpu["alpha"].detach().cpu()[ok], cpu["alpha"].detach()[ok])
    assert_close(gpu["render"].detach().cpu()[ok], cpu["render"].detach()[ok], name="render")
    assert_close(gpu["alpha"].detach().cpu()[ok], cpu["alpha"].detach()[ok], name="alpha")
    assert abs(float(gpu["loss"]) - float(cpu["loss"])) <= 1e-4 * abs(float(cpu["loss"]))
    for name, a, b in zip(("means", "quats", "scales", "opacities"), gpu["p"], cpu["p"]):
        e[name] = rel_err(a.grad, b.grad)
        assert_close(a.grad.cpu(), b.grad, name=f"grad {name}")
    if render_mode in ("D", "ED"):  # the colours take no part
        assert gpu["col"].grad is None and cpu["col"].grad is None
    else:
        e["colors"] = rel_err(gpu["col"].grad, cpu["col"].grad)
        assert_close(gpu["col"].grad.cpu(), cpu["col"].grad, name="grad colors")
    if with_bg:
        if render_mode in ("D", "ED"):  # gsplat replaces the backgrounds with zeros
            assert gpu["bg"].grad is None and cpu["bg"].grad is None
        else:
            e["backgrounds"] = rel_err(gpu["bg"].grad, cpu["bg"].grad)
            assert_close(gpu["bg"].grad.cpu(), cpu["bg"].grad, name="grad backgrounds")
    e["v_means2d"] = rel_err(gpu["info"]["means2d"].grad, cpu["info"]["means2d"].grad)
    e["absgrad"] = rel_err(gpu["info"]["means2d"].absgrad, cpu["info"]["means2d"].absgrad)
    assert_close(gpu["info"]["means2d"].grad.cpu(), cpu["info"]["means2d"].grad, name="v_means2d")
    assert_close(gpu["info"]["means2d"].absgrad.cpu(), cpu["info"]["means2d"].absgrad, name="absgrad")
    # one native call per stage for the C cameras, none of the RGB-only compositing entries
    for stage in ("eg_project_fwd_cams", "eg_tile_offsets_cams", "eg_tile_emit_sort_cams", "eg_composite_fwd_modes_cams",
                  "eg_composite_bwd_modes_cams", "eg_project_bwd_cams"):
        assert seen.count(stage) == 1, (stage, seen)
    assert not [n for n in seen if n in ("eg_operator_fwd", "eg_composite_fwd_cams", "eg_composite_bwd_colors",
                                         "eg_composite_bwd_footprint_cams")], seen
    record("render_modes_vs_torch_oracle", render_mode=render_mode, mode=mode, cameras=C, colors=ckind, backgrounds=with_bg,
           removed_borderline_gaussians=removed, borderline_pixels=int((~keep).sum()), max_rel_err=e)


@pytest.mark.parametrize("render_mode", ["D", "RGB+ED"])
def test_depth_only_loss_reaches_the_means(env, render_mode):
    """A loss on the depth channel alone, colours without grad: the whole gradient comes through v_depths (and the
    depth channel's share of v_alpha)."""
    cams = [0, 2, 3]
    sc, keep, _ = _setup(env, cams, "antialiased")
    C, N = len(cams), sc.means.shape[0]
    colors0 = _colors("N3", C, N)
    wd = torch.rand(C, H, W, generator=torch.Generator().manual_seed(14)) * keep

    def loss_fn(render, alpha, dev):
        return (render[..., -1] * wd.to(dev)).sum() * 1e-3

    cpu, gpu = _run(env, sc, cams, colors0, None, render_mode, "antialiased", loss_fn, colors_grad=False)
    g = gpu["p"][0].grad
    assert g is not None and float(g.abs().max()) > 0
    e = {}
    for name, a, b in zip(("means", "quats", "scales", "opacities"), gpu["p"], cpu["p"]):
        e[name] = rel_err(a.grad, b.grad)
        assert_close(a.grad.cpu(), b.grad, name=f"depth-only grad {name}")
    record("render_modes_depth_only_loss", render_mode=render_mode, max_rel_err=e)


def test_rgb_plus_depth_colour_channels_equal_rgb(env):
    """The colour channels of "RGB+D" are the "RGB" render of the same non-unit colours, bit for bit; so are the alphas."""
    from edgegaussians_amd import rasterization
    synth, O, CO = env
    cams = [0, 2, 3]
    sc, _, _ = _setup(env, cams, "antialiased")
    C, N = len(cams), sc.means.shape[0]
    col = _colors("N3", C, N).cuda()
    kw = dict(means=sc.means.cuda(), quats=sc.quats.cuda(), scales=torch.exp(sc.log_scales).cuda(),
              opacities=torch.sigmoid(sc.logit_opacities).squeeze(-1).cuda(), colors=col, viewmats=sc.viewmats[cams].cuda(),
              Ks=sc.Ks[cams].cuda(), width=W, height=H, packed=False, rasterize_mode="antialiased")
    with torch.no_grad():
        r_rgb, a_rgb, i_rgb = rasterization(render_mode="RGB", **kw)
        r_d, a_d, i_d = rasterization(render_mode="RGB+D", **kw)
    assert r_d.shape == (C, H, W, 4)
    assert torch.equal(r_d[..., :3], r_rgb)
    assert torch.equal(a_d, a_rgb)
    assert torch.equal(i_d["last_ids"], i_rgb["last_ids"])
    assert list(i_d.keys()) == list(i_rgb.keys())  # the same `info`, binning included
    for k in ("radii", "depths", "isect_ids", "flatten_ids", "isect_offsets", "tiles_per_gauss"):
        assert torch.equal(i_d[k], i_rgb[k]), k
    assert float(r_d[..., 3].abs().max()) > 0
