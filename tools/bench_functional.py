"""Times the kernels behind the functional API that have no other caller (csrc/functional.hip) and writes
profiles/functional_timing.txt.

    python tools/bench_functional.py [--out profiles/functional_timing.txt] [--n 100000] [--m 265000] [--windows 9] [--calls 200]

N Gaussians in front of one 800 x 800 camera (C = 1), every entry through the C ABI on preallocated buffers, each as the
median over `--windows` windows of `--calls` back-to-back calls between two device events (warm-up first; the
configurations are alternated window by window so that a drift of the machine hits them alike):

  covars fwd / fwd+bwd   eg_project_covars_fwd_cams (+ eg_project_covars_bwd_cams), compensations and all four cotangents
  quats  fwd / fwd+bwd   eg_project_fwd_cams (+ eg_project_bwd_cams) on the same Gaussians, without its tile counting:
                         the yardstick in the same process
  qs2cp  fwd / fwd+bwd   eg_quat_scale_to_covar_preci_fwd (+ _bwd), both outputs, upper triangle
  offset_encode          eg_isect_offset_encode on M sorted ids over a 50 x 50 tile grid

Bytes are the algorithmic ones per Gaussian (or per id), listed next to each figure."""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "functional_timing.txt"))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--m", type=int, default=265000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    from edgegaussians_amd import _lib, synth
    from edgegaussians_amd._lib import call, ptr, stream
    _lib.load()  # raises without the library or the GPU: no fallback
    N, M, Wd, Hd = args.n, args.m, 800, 800
    sc = synth.make_scene(N, 1, Wd, Hd, seed=0)
    means, quats = sc.means.cuda(), sc.quats.cuda()
    scales = torch.exp(sc.log_scales).cuda()
    opac = torch.full((N,), 0.5, device="cuda")
    vm, K = sc.viewmats.cuda().contiguous(), sc.Ks.cuda().contiguous()
    f32 = dict(device="cuda")
    i32 = dict(device="cuda", dtype=torch.int32)
    g = torch.Generator().manual_seed(0)
    # ---- quat_scale_to_covar_preci
    cov6, pre6 = torch.empty(N, 6, **f32), torch.empty(N, 6, **f32)
    v_cov6, v_pre6 = torch.randn(N, 6, generator=g).cuda(), torch.randn(N, 6, generator=g).cuda()
    vq, vs = torch.empty(N, 4, **f32), torch.empty(N, 3, **f32)

    def qs_fwd():
        call("eg_quat_scale_to_covar_preci_fwd", ptr(quats), ptr(scales), N, 1, ptr(cov6), ptr(pre6), stream())

    def qs_fb():
        qs_fwd()
        call("eg_quat_scale_to_covar_preci_bwd", ptr(quats), ptr(scales), N, 1, ptr(v_cov6), ptr(v_pre6), ptr(vq), ptr(vs), stream())

    qs_fwd()
    # ---- the two projections
    radii, m2d, dep = torch.empty(1, N, **i32), torch.empty(1, N, 2, **f32), torch.empty(1, N, **f32)
    con, comp = torch.empty(1, N, 3, **f32), torch.empty(1, N, **f32)
    v_m2d, v_dep = torch.randn(1, N, 2, generator=g).cuda(), torch.randn(1, N, generator=g).cuda()
    v_con, v_comp = torch.randn(1, N, 3, generator=g).cuda(), torch.randn(1, N, generator=g).cuda()
    v_means, v_cov = torch.empty(N, 3, **f32), torch.empty(N, 6, **f32)
    splat = torch.empty(1, N, 8, **f32)
    g2d = torch.cat([v_m2d, torch.zeros(1, N, 2, **f32), v_con, torch.zeros(1, N, 1, **f32)], dim=-1).contiguous()
    v_quats, v_scales = torch.empty(N, 4, **f32), torch.empty(N, 3, **f32)
    AA = _lib.FLAG_ANTIALIASED

    def cov_fwd():
        call("eg_project_covars_fwd_cams", ptr(means), ptr(cov6), ptr(vm), ptr(K), N, 1, Wd, Hd, 0.01, 1e10, 0.3, 0.0, ptr(radii),
             ptr(m2d), ptr(dep), ptr(con), ptr(comp), stream())

    def cov_fb():
        cov_fwd()
        call("eg_project_covars_bwd_cams", ptr(means), ptr(cov6), ptr(vm), ptr(K), N, 1, Wd, Hd, 0.3, ptr(radii), ptr(v_m2d),
             ptr(v_dep), ptr(v_con), ptr(v_comp), ptr(v_means), ptr(v_cov), stream())

    def quat_fwd():
        call("eg_project_fwd_cams", ptr(means), ptr(quats), ptr(scales), ptr(opac), ptr(vm), ptr(K), N, 1, Wd, Hd, 0.01, 1e10,
             0.3, 0.0, AA, ptr(splat), ptr(radii), ptr(m2d), ptr(dep), ptr(con), ptr(comp), None, None, stream())

    def quat_fb():
        quat_fwd()
        call("eg_project_bwd_cams", ptr(means), ptr(quats), ptr(scales), ptr(opac), ptr(vm), ptr(K), N, 1, Wd, Hd, 0.3, AA,
             ptr(splat), ptr(g2d), ptr(v_comp), ptr(v_dep), ptr(v_means), ptr(v_quats), ptr(v_scales), stream())

    quat_fwd()
    torch.cuda.synchronize()
    visible = int((radii > 0).sum())
    # ---- isect_offset_encode
    tw = th = 50
    T = tw * th
    tile_bits = int(math.floor(math.log2(T))) + 1
    cells = torch.sort(torch.randint(0, T, (M,), generator=g)).values
    depth = (torch.rand(M, generator=g) + 0.5).view(torch.int32).to(torch.int64)
    ids = torch.sort((cells << 32) | depth).values.cuda()
    offsets = torch.empty(T, **i32)
    assert tile_bits == 12

    def enc():
        call("eg_isect_offset_encode", ptr(ids), M, 1, tw, th, ptr(offsets), stream())

    fns = {"covars fwd": (cov_fwd, 36 + 32), "covars fwd+bwd": (cov_fb, 36 + 32 + 36 + 4 + 28 + 36),
           "quats fwd": (quat_fwd, 44 + 64), "quats fwd+bwd": (quat_fb, 44 + 64 + 44 + 32 + 32 + 8 + 40),
           "qs2cp fwd": (qs_fwd, 28 + 48), "qs2cp fwd+bwd": (qs_fb, 28 + 48 + 28 + 48 + 28)}
    for fn, _ in list(fns.values()) + [(enc, 0)]:  # warm-up: code objects
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in list(fns) + ["offset_encode"]}
    for _ in range(args.windows):
        for k, (fn, _) in fns.items():
            t[k].append(timed(fn, args.calls))
        t["offset_encode"].append(timed(enc, args.calls))
    lines = [f"functional-API kernels, N = {N} ({visible} visible), C = 1, {Wd} x {Hd}, fp32, {torch.cuda.get_device_name(0)}; "
             f"microseconds per call, median of {args.windows} windows of {args.calls} calls (min .. max)"]
    for k, (_, per) in fns.items():
        xs = t[k]
        med = statistics.median(xs)
        lines.append(f"  {k:15s} {med:9.2f} us  ({min(xs):.2f} .. {max(xs):.2f})   {per * N / med * 1e-3:8.1f} GB/s of "
                     f"{per * N / 1e6:.2f} MB algorithmic ({per} B per Gaussian)")
    xs = t["offset_encode"]
    med = statistics.median(xs)
    nbytes = 8 * M + 4 * T
    lines.append(f"  {'offset_encode':15s} {med:9.2f} us  ({min(xs):.2f} .. {max(xs):.2f})   {nbytes / med * 1e-3:8.1f} GB/s of "
                 f"{nbytes / 1e6:.2f} MB algorithmic (M = {M} ids, T = {T} tiles)")
    for kind in ("fwd", "fwd+bwd"):
        a, b = statistics.median(t[f"covars {kind}"]), statistics.median(t[f"quats {kind}"])
        lines.append(f"  {kind}: quats / covars = {b / a:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
