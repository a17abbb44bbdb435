"""Times the spherical-harmonics operator (csrc/sh.hip) against the float32 torch-eager evaluation of the same formula
on the same GPU and writes profiles/sh_timing.txt.

    python tools/bench_sh.py [--out profiles/sh_timing.txt] [--n 100000] [--windows 9] [--calls 200]

N Gaussians, C = 1, K = 16 coefficient rows, degrees 0 and 3.  Per configuration three things are timed, each as the
median over `--windows` windows of `--calls` back-to-back calls between two device events (warm-up first; the three
are alternated window by window so that a drift of the machine hits them alike):

  kernel    eg_sh_fwd / eg_sh_fwd + eg_sh_bwd through the C ABI on preallocated buffers -- the kernels themselves
  operator  edgegaussians_amd.spherical_harmonics (+ .backward) -- what a caller pays, allocation and autograd included
  eager     tests/sh_oracle.sh_eval in float32 torch eager (+ .backward) -- the yardstick

Bytes are the algorithmic ones: forward reads 12 (L+1)^2 N of coefficients and 12 N of directions and writes 12 N;
the backward reads the same plus 12 N of v_colors and writes 12 K N of v_coeffs and 12 N of v_dirs."""
import argparse
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sh_timing.txt"))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    from edgegaussians_amd import _lib, spherical_harmonics
    from edgegaussians_amd._lib import call, ptr, stream
    from tests import sh_oracle
    _lib.load()  # raises without the library or the GPU: no fallback
    N, K = args.n, 16
    g = torch.Generator().manual_seed(0)
    dirs = torch.randn(N, 3, generator=g).cuda()
    coeffs = torch.randn(N, K, 3, generator=g).cuda()
    v = torch.randn(N, 3, generator=g).cuda()
    colors, v_coeffs, v_dirs = torch.empty(N, 3, device="cuda"), torch.empty_like(coeffs), torch.empty_like(dirs)
    lines = [f"spherical harmonics, N = {N}, C = 1, K = {K}, fp32, {torch.cuda.get_device_name(0)}; microseconds per call, "
             f"median of {args.windows} windows of {args.calls} calls (min .. max)"]
    for L in (0, 3):
        ku = (L + 1) ** 2
        bytes_f = 12 * ku * N + 24 * N
        bytes_fb = bytes_f + (12 * ku * N + 24 * N) + 12 * K * N + 12 * N
        dg, cg = dirs.clone().requires_grad_(True), coeffs.clone().requires_grad_(True)

        def k_fwd():
            call("eg_sh_fwd", L, K, 1, N, ptr(dirs), None, None, ptr(coeffs), 0, None, 0, ptr(colors), stream())

        def k_fb():
            k_fwd()
            call("eg_sh_bwd", L, K, 1, N, ptr(dirs), None, None, ptr(coeffs), 0, None, 0, ptr(v), ptr(v_coeffs), ptr(v_dirs),
                 None, stream())

        def op_fwd():
            with torch.no_grad():
                spherical_harmonics(L, dirs, coeffs)

        def op_fb():
            dg.grad = cg.grad = None
            spherical_harmonics(L, dg, cg).backward(v)

        def eager_fwd():
            with torch.no_grad():
                sh_oracle.sh_eval(L, dirs, coeffs)

        def eager_fb():
            dg.grad = cg.grad = None
            sh_oracle.sh_eval(L, dg, cg).backward(v)

        # the three compute the same thing (the eager one in another operation order)
        ref = sh_oracle.sh_eval(L, dirs.double(), coeffs.double())
        err_k = float((spherical_harmonics(L, dirs, coeffs).double() - ref).abs().max())
        err_e = float((sh_oracle.sh_eval(L, dirs, coeffs).double() - ref).abs().max())
        fns = {"kernel fwd": k_fwd, "kernel fwd+bwd": k_fb, "operator fwd": op_fwd, "operator fwd+bwd": op_fb,
               "eager fwd": eager_fwd, "eager fwd+bwd": eager_fb}
        for fn in fns.values():  # warm-up: code objects, the allocator's pools
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(args.windows):
            for k, fn in fns.items():
                t[k].append(timed(fn, args.calls))
        lines.append(f"degree {L}: max |value - float64| kernel {err_k:.2e}, eager {err_e:.2e}")
        for k, xs in t.items():
            med = statistics.median(xs)
            nbytes = bytes_fb if "bwd" in k else bytes_f
            lines.append(f"  {k:17s} {med:9.2f} us  ({min(xs):.2f} .. {max(xs):.2f})   {nbytes / med * 1e-3:8.1f} GB/s of "
                         f"{nbytes / 1e6:.2f} MB algorithmic")
        for kind in ("fwd", "fwd+bwd"):
            a, b, c = (statistics.median(t[f"{w} {kind}"]) for w in ("kernel", "operator", "eager"))
            lines.append(f"  {kind}: eager / kernel = {c / a:.2f}, eager / operator = {c / b:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
