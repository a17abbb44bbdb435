"""Times fused SSIM (csrc/ssim.hip through edgegaussians_amd.ssim.fused_ssim) against the float32 torch conv formulation
of the same formulas on the same GPU and writes profiles/ssim_timing.txt.

    python tools/bench_ssim.py [--out profiles/ssim_timing.txt] [--calls 50] [--warmup 10]

Sizes 1x3x512x512, 1x3x800x800 and 1x3x1200x1600; layouts NCHW and the permute(0, 3, 1, 2) view of a contiguous
[B, H, W, C] (what rasterization's render gives; the torch formulation takes its .contiguous() copy first, inside the
timed region, as a trainer would).  Per configuration: forward (no gradient wanted) and forward + backward of the scalar,
each the median over `--calls` calls, every call between two device events of its own, after `--warmup` calls.

Bytes are the algorithmic ones per pixel-channel: the forward reads 8 (two inputs) and writes 4 (the map) in evaluation
mode, 16 with the three derivative maps; the backward reads 4 (v) + 12 (the maps) + 8 (the inputs) and writes 4."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed_calls(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)  # microseconds
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_timing.txt"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from edgegaussians_amd import _lib
    from edgegaussians_amd.ssim import fused_ssim
    from tests import ssim_util as SU
    _lib.load()  # raises without the library or the GPU: no fallback
    win = SU.window(dtype=torch.float32).cuda()

    def torch_ssim(x1, x2):
        x1, x2 = x1.contiguous(), x2.contiguous()
        return SU.ssim_map_ref(x1, x2, blur_fn=lambda t: SU.blur(t, win)).mean()

    lines = [f"fused SSIM, fp32, {torch.cuda.get_device_name(0)}; microseconds per call, median of {args.calls} calls "
             f"(min .. max), each between two device events, after {args.warmup} warm-up calls"]
    g = torch.Generator().manual_seed(0)
    for shape in ((1, 3, 512, 512), (1, 3, 800, 800), (1, 3, 1200, 1600)):
        base1, base2 = (torch.rand(shape, generator=g) ** 6).cuda(), (torch.rand(shape, generator=g) ** 6).cuda()
        n = base1.numel()
        for layout in SU.LAYOUTS:
            x1 = SU.as_layout(base1, layout).requires_grad_(True)
            x2 = SU.as_layout(base2, layout)

            def fused_fwd():
                fused_ssim(x1, x2, train=False)

            def fused_fb():
                x1.grad = None
                fused_ssim(x1, x2).backward()

            def torch_fwd():
                with torch.no_grad():
                    torch_ssim(x1, x2)

            def torch_fb():
                x1.grad = None
                torch_ssim(x1, x2).backward()

            diff = abs(float(fused_ssim(x1, x2, train=False)) - float(torch_ssim(x1.detach(), x2)))
            lines.append(f"{'x'.join(map(str, shape))} {layout}: |fused - torch| of the scalar {diff:.2e}")
            med = {}
            for name, fn, nbytes in (("fused fwd", fused_fwd, 12 * n), ("fused fwd+bwd", fused_fb, (24 + 28) * n),
                                     ("torch fwd", torch_fwd, 12 * n), ("torch fwd+bwd", torch_fb, (24 + 28) * n)):
                xs = timed_calls(fn, args.calls, args.warmup)
                med[name] = statistics.median(xs)
                lines.append(f"  {name:14s} {med[name]:9.1f} us  ({min(xs):.1f} .. {max(xs):.1f})   "
                             f"{nbytes / med[name] * 1e-3:7.1f} GB/s of {nbytes / 1e6:.1f} MB algorithmic")
            lines.append(f"  torch / fused: fwd {med['torch fwd'] / med['fused fwd']:.2f}, "
                         f"fwd+bwd {med['torch fwd+bwd'] / med['fused fwd+bwd']:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
