"""Spherical-harmonics colours on the GPU (csrc/sh.hip): `spherical_harmonics` against the float64 oracle of
tests/sh_oracle.py, and `rasterization(sh_degree=L)` against the dense PyTorch oracle of tests/test_gpu_render_modes.py
fed with the oracle's colours.

The bound of the operator test is measured, not fixed: the same oracle evaluated in float32 torch on the CPU deviates
from float64 by d32 (largest absolute deviation per output kind: values, gradient of the directions, gradient of the
coefficients); the kernel may deviate by 4 * d32 (its operation order differs from torch's), with a floor of 1e-6.
d32 is taken over all the sizes and leading shapes of one (degree, K) case together, as is the kernel's deviation: the
largest of a handful of values (N = 1 has three) does not estimate what a number format costs."""
import functools

import pytest
import torch

from tests import sh_oracle
from tests.util import assert_close, record, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    from edgegaussians_amd import synth
    from oracle import ref_torch as O
    from oracle import c_oracle as CO
    return synth, O, CO


def _operator_inputs(L, K, lead, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(*lead, 3, generator=g, dtype=torch.float64)
    norms = 10.0 ** (torch.rand(*lead, 1, generator=g, dtype=torch.float64) * 4 - 2)  # 1e-2 .. 1e2
    dirs = (d / d.norm(dim=-1, keepdim=True) * norms).float()
    coeffs = torch.randn(*lead, K, 3, generator=g)
    masks = torch.rand(*lead, generator=g) > 1 / 3
    v = torch.randn(*lead, 3, generator=g)
    return dirs, coeffs, masks, v


def _oracle_run(L, dirs, coeffs, masks, v, dtype):
    d = dirs.detach().clone().to(dtype).requires_grad_(True)
    c = coeffs.detach().clone().to(dtype).requires_grad_(True)
    out = sh_oracle.sh_eval(L, d, c, masks)
    out.backward(v.to(dtype))
    v_dirs = d.grad if d.grad is not None else torch.zeros_like(d)  # (degree 0 does not depend on the direction)
    return out.detach().double(), v_dirs.double(), c.grad.double()


SIZES = (1, 63, 64, 257, 1000)  # below, at and across a wave (64) and a workgroup (128)


@pytest.mark.parametrize("L,K", [(0, 1), (1, 4), (2, 9), (3, 16), (4, 25), (2, 25)])
def test_spherical_harmonics_match_the_float64_oracle(env, L, K):
    from edgegaussians_amd import spherical_harmonics
    import gsplat
    assert gsplat.spherical_harmonics is spherical_harmonics
    ku = (L + 1) ** 2
    kinds = ("values", "v_dirs", "v_coeffs")
    d32 = dict.fromkeys(kinds, 0.0)
    dk = dict.fromkeys(kinds, 0.0)
    for N in SIZES:
        for lead in ((N,), (3, N)):
            dirs, coeffs, masks, v = _operator_inputs(L, K, lead, seed=1000 * L + K + N + len(lead))
            ref = _oracle_run(L, dirs, coeffs, masks, v, torch.float64)
            f32 = _oracle_run(L, dirs, coeffs, masks, v, torch.float32)
            dg = dirs.cuda().requires_grad_(True)
            cg = coeffs.cuda().requires_grad_(True)
            out = spherical_harmonics(L, dg, cg, masks.cuda())
            assert out.shape == lead + (3,) and out.dtype == torch.float32
            out.backward(v.cuda())
            got = (out.detach().cpu().double(), dg.grad.cpu().double(), cg.grad.cpu().double())
            for kind, r, a, b in zip(kinds, ref, f32, got):
                assert torch.isfinite(b).all(), (kind, N, lead)
                d32[kind] = max(d32[kind], float((a - r).abs().max()))
                dk[kind] = max(dk[kind], float((b - r).abs().max()))
            # exact zeros: masked outputs, their gradients, the coefficient rows above the degree's
            assert float(got[0][~masks].abs().max() if (~masks).any() else 0.0) == 0.0
            assert float(got[1][~masks].abs().max() if (~masks).any() else 0.0) == 0.0
            assert float(got[2][~masks].abs().max() if (~masks).any() else 0.0) == 0.0
            assert float(got[2][..., ku:, :].abs().max() if K > ku else 0.0) == 0.0
            if masks.any() and L > 0:
                assert float(got[1][masks].abs().max()) > 0.0
            # without a mask the same values where it was true
            out2 = spherical_harmonics(L, dirs.cuda(), coeffs.cuda())
            assert torch.equal(out2[masks.cuda()], out.detach()[masks.cuda()])
    line = f"degree {L} K {K}: " + ", ".join(
        f"{k} float32-torch {d32[k]:.3e} kernel {dk[k]:.3e} bound {max(4 * d32[k], 1e-6):.3e}" for k in kinds)
    print(line)
    record("sh_vs_float64_oracle", degree=L, K=K, float32_torch=d32, kernel=dk, line=line)  # -> profiles/sh_parity.txt
    for k in kinds:
        assert dk[k] <= max(4 * d32[k], 1e-6), line


def test_backward_with_shared_coefficients_is_deterministic(env):
    from edgegaussians_amd import sh
    g = torch.Generator().manual_seed(5)
    N, C = 1000, 3
    means = torch.randn(N, 3, generator=g).cuda()
    vm = torch.eye(4).repeat(C, 1, 1)
    vm[:, :3, 3] = torch.randn(C, 3, generator=g) * 3
    coeffs = torch.randn(N, 16, 3, generator=g).cuda()
    radii = torch.randint(-1, 4, (C, N), generator=g, dtype=torch.int32).cuda()
    v = torch.randn(C, N, 3, generator=g).cuda()
    runs = []
    for _ in range(2):
        m, c = means.clone().requires_grad_(True), coeffs.clone().requires_grad_(True)
        col = sh.view_colors(m, vm.cuda(), c, radii, 3)
        col.backward(v)
        runs.append((col.detach(), m.grad, c.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][2].abs().max()) > 0 and float(runs[0][1].abs().max()) > 0
    assert float(runs[0][0][radii <= 0].abs().max()) == 0.0


# ---- rasterization(sh_degree=L) against the dense oracle ---------------------------------------------------------------
from tests.test_gpu_render_modes import H, W, _setup, oracle_rasterization  # noqa: E402

CLAMP_MARGIN = 1e-5
SEED = 21


@functools.lru_cache(maxsize=None)
def _scene(env, cams, mode):
    return _setup(env, list(cams), mode)


def _coefficients(L, K, shape_lead, seed=SEED):
    """Normal coefficients scaled so that the unclamped colour has a standard deviation of 0.5 around its 0.5 offset
    (sum_k Y_k^2 = (L+1)^2 / 4 pi): about one colour in six clamps at 0."""
    g = torch.Generator().manual_seed(seed)
    sigma = 0.5 * (4 * torch.pi / (L + 1) ** 2) ** 0.5
    return torch.randn(*shape_lead, K, 3, generator=g) * sigma


def _oracle_colors(O, L, means, coeffs, viewmats, Ks, quats, scales):
    """[C, N, 3] float32 colours with autograd to means / coeffs, evaluated in float64; + the raw values and the mask."""
    C = viewmats.shape[0]
    with torch.no_grad():
        radii = torch.stack([O.project(means, quats, scales, viewmats[c], Ks[c], W, H)[0] for c in range(C)])
        campos = torch.linalg.inv(viewmats.double())[:, :3, 3]
    dirs = means.double()[None] - campos[:, None]
    co = coeffs.double()
    co = co[None].expand(C, *co.shape) if co.dim() == 3 else co
    raw = sh_oracle.sh_eval(L, dirs, co) + 0.5
    vis = radii > 0
    col = torch.where(vis[..., None], raw.clamp_min(0.0), torch.zeros_like(raw))
    return col.float(), raw.detach(), vis


SH_CASES = [  # (degree, K, per-camera coefficients, cameras, render_mode, rasterize_mode, backgrounds)
    (0, 1, False, (1,), "RGB", "antialiased", False),
    (3, 16, False, (1,), "RGB", "antialiased", False),
    (3, 16, False, (0, 2, 3), "RGB", "antialiased", False),
    (2, 9, True, (0, 2, 3), "RGB", "classic", False),
    (3, 16, False, (0, 2, 3), "RGB+ED", "antialiased", True),
]


@pytest.mark.parametrize("L,K,per_cam,cams,render_mode,mode,with_bg", SH_CASES,
                         ids=[f"L{c[0]}-K{c[1]}-{'CNK3' if c[2] else 'NK3'}-C{len(c[3])}-{c[4]}-{c[5]}" for c in SH_CASES])
def test_rasterization_with_sh_degree_matches_oracle(env, L, K, per_cam, cams, render_mode, mode, with_bg):
    from edgegaussians_amd import rasterization
    synth, O, CO = env
    sc, keep, removed = _scene(env, cams, mode)
    cams = list(cams)
    C, N = len(cams), sc.means.shape[0]
    coeffs0 = _coefficients(L, K, (C, N) if per_cam else (N,))
    bg0 = torch.rand(C, 3, generator=torch.Generator().manual_seed(12)) if with_bg else None
    Dout = 3 + int(render_mode != "RGB")
    wr = torch.rand(C, H, W, Dout, generator=torch.Generator().manual_seed(13)) * keep[..., None]

    def loss_fn(render, alpha, dev):
        return (render * wr.to(dev)).sum() * 1e-3 + ((alpha[..., 0] ** 2) * keep.to(dev)).sum() * 1e-3

    outs = []
    for dev in ("cpu", "cuda"):
        p = [t.clone().to(dev).requires_grad_(True) for t in (sc.means, sc.quats, sc.log_scales, sc.logit_opacities)]
        co = coeffs0.clone().to(dev).requires_grad_(True)
        bg = bg0.clone().to(dev).requires_grad_(True) if bg0 is not None else None
        kw = dict(means=p[0], quats=p[1], scales=torch.exp(p[2]), opacities=torch.sigmoid(p[3]).squeeze(-1),
                  viewmats=sc.viewmats[cams].to(dev), Ks=sc.Ks[cams].to(dev), width=W, height=H, backgrounds=bg,
                  render_mode=render_mode, absgrad=True, rasterize_mode=mode)
        extra = {}
        if dev == "cpu":
            col, raw, vis = _oracle_colors(O, L, p[0], co, kw["viewmats"], kw["Ks"], p[1].detach(), kw["scales"].detach())
            render, alpha, info = oracle_rasterization(O, colors=col, **kw)
            extra = dict(raw=raw, vis=vis)
        else:
            render, alpha, info = rasterization(colors=co, sh_degree=L, tile_size=16, packed=False, **kw)
        loss = loss_fn(render, alpha, dev)
        loss.backward()
        outs.append(dict(render=render.detach().cpu(), alpha=alpha.detach().cpu(), p=p, co=co, bg=bg, loss=float(loss),
                         info=info, **extra))
    cpu, gpu = outs
    # both sides of the clamp are exercised, and almost nothing sits on it
    raw, vis = cpu["raw"], cpu["vis"]
    seen = raw[vis]
    clamped, free = float((seen < 0).float().mean()), float((seen > 0).float().mean())
    assert clamped > 0.02 and free > 0.02, (clamped, free)
    near = ((raw.abs() < CLAMP_MARGIN) & vis[..., None]).any(-1).any(0)  # [N]
    assert float(near.float().mean()) <= 0.01
    ok = ~near
    assert torch.equal(gpu["info"]["radii"].cpu() > 0, vis)
    e = {}
    assert gpu["render"].shape == cpu["render"].shape == (C, H, W, Dout)
    for name in ("render", "alpha"):
        e[name] = rel_err(gpu[name][keep], cpu[name][keep])
        assert_close(gpu[name][keep], cpu[name][keep], name=name)
    assert abs(gpu["loss"] - cpu["loss"]) <= 1e-4 * abs(cpu["loss"])
    for name, a, b in zip(("means", "quats", "scales", "opacities"), gpu["p"], cpu["p"]):
        ga, gb = (a.grad.cpu()[ok], b.grad[ok]) if name == "means" else (a.grad.cpu(), b.grad)
        e[name] = rel_err(ga, gb)
        assert_close(ga, gb, name=f"grad {name}")
    ga, gb = gpu["co"].grad.cpu(), cpu["co"].grad
    assert ga.shape == coeffs0.shape
    ga, gb = (ga[:, ok], gb[:, ok]) if per_cam else (ga[ok], gb[ok])
    assert float(gb.abs().max()) > 0
    e["coeffs"] = rel_err(ga, gb)
    assert_close(ga, gb, name="grad coeffs")
    if with_bg:
        e["backgrounds"] = rel_err(gpu["bg"].grad, cpu["bg"].grad)
        assert_close(gpu["bg"].grad.cpu(), cpu["bg"].grad, name="grad backgrounds")
    record("sh_rasterization_vs_torch_oracle", degree=L, K=K, per_camera=per_cam, cameras=C, render_mode=render_mode, mode=mode,
           backgrounds=with_bg, removed_borderline_gaussians=removed, clamped_share=clamped,
           gaussians_near_clamp=int(near.sum()), max_rel_err=e)


def _device_scene(env, cams=(0, 2, 3)):
    sc, _, _ = _scene(env, tuple(cams), "antialiased")
    cams = list(cams)
    return sc, dict(means=sc.means.cuda(), quats=sc.quats.cuda(), scales=torch.exp(sc.log_scales).cuda(),
                    opacities=torch.sigmoid(sc.logit_opacities).squeeze(-1).cuda(), viewmats=sc.viewmats[cams].cuda(),
                    Ks=sc.Ks[cams].cuda(), width=W, height=H, packed=False, rasterize_mode="antialiased")


def test_depth_mode_never_evaluates_the_harmonics(env, monkeypatch):
    from edgegaussians_amd import rasterization
    from edgegaussians_amd import sh
    sc, kw = _device_scene(env)
    N = sc.means.shape[0]
    seen = []
    real_call = sh.call
    monkeypatch.setattr(sh, "call", lambda name, *a: (seen.append(name), real_call(name, *a))[1])
    co = _coefficients(2, 9, (N,)).cuda().requires_grad_(True)
    means = kw.pop("means").requires_grad_(True)
    r_sh, a_sh, _ = rasterization(means=means, colors=co, sh_degree=2, render_mode="D", **kw)
    with torch.no_grad():
        r, a, _ = rasterization(means=means, colors=torch.ones(N, 3, device="cuda"), render_mode="D", **kw)
    assert torch.equal(r_sh.detach(), r) and torch.equal(a_sh.detach(), a)
    r_sh.sum().backward()
    assert co.grad is None and means.grad is not None
    assert not seen, seen


@pytest.mark.parametrize("case", ["K_too_small", "degree_5", "last_dimension_4", "rank_2"])
def test_sh_degree_validation(env, case):
    from edgegaussians_amd import rasterization
    sc, kw = _device_scene(env)
    N = sc.means.shape[0]
    colors, L = {"K_too_small": (torch.zeros(N, 8, 3), 2), "degree_5": (torch.zeros(N, 36, 3), 5),
                 "last_dimension_4": (torch.zeros(N, 9, 4), 2), "rank_2": (torch.zeros(N, 3), 0)}[case]
    with pytest.raises(ValueError):
        rasterization(colors=colors.cuda(), sh_degree=L, **kw)
