"""Times the fused bilateral grid (edgegaussians_amd.bilagrid) against the torch compositions it replaces, on the same
GPU in the same run, and writes profiles/bilagrid_timing.txt.

    python tools/bench_bilagrid.py [--out profiles/bilagrid_timing.txt] [--calls 100] [--warmup 20]

* slice, forward + backward down to render.grad and grids.grad, on a [1, 1200, 1600, 3] render with one 16x16x8 grid,
  and on [4, 800, 800, 3] with 4 of 50 grids, against float32 F.grid_sample + permute + the batched 3x4 product.
* total_variation_loss, forward + backward, on [200, 12, 8, 16, 16], against the three-axis slice / subtract / square /
  mean chain.

The method is tools/bench_losses.py's: device time between two device events per call, fused and composed calls
alternating, median (min .. max) over `--calls` calls after `--warmup` calls of each -- the call as a trainer pays it,
host dispatch included -- and kernel launches per direction with the sum of the kernels' durations from a
torch.profiler trace of ten calls, taken after the timing; for the fused form also every kernel's own duration.

Bytes are the algorithmic ones.  Per sample the fused slice forward reads 12 (rgb) + 8 (xy) and writes 12; its backward
reads 12 + 8 + 12 (the cotangent) for each of its two kernels and writes 12 (v_rgb); the grid (96 KiB at 16x16x8) and its
gradient stay on chip.  The torch composition writes and re-reads the [B, 12, H, W] slice (48 B per sample) forward
and its cotangent backward on top of that: >= 12 + 8 + 2 * 48 + 12 forward and >= 12 + 2 * 48 + 12 + 12 + 8 backward.
The TV loss reads 4 bytes per cell forward, and reads 4 and writes 4 backward, where each of the chain's three axes reads
and writes the whole tensor several times."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from bench_losses import TRACED_CALLS, alternating, kernel_launches  # noqa: E402

GW = (0.299, 0.587, 0.114)


def torch_slice(grids, xy, rgb, idx):
    """the composition the fused slice replaces, float32"""
    B, H, W, _ = rgb.shape
    gray = (GW[0] * rgb[..., 0] + GW[1] * rgb[..., 1]) + GW[2] * rgb[..., 2]
    coords = torch.cat([2.0 * xy - 1.0, 2.0 * gray[..., None] - 1.0], dim=-1).view(B, 1, H, W, 3)
    A = F.grid_sample(grids[idx], coords, mode="bilinear", align_corners=True, padding_mode="border")
    A = A.view(B, 12, H, W).permute(0, 2, 3, 1).reshape(B, H, W, 3, 4)
    return (A[..., :3] @ rgb[..., None]).squeeze(-1) + A[..., 3]


def torch_tv(x):
    return (((x[:, :, 1:] - x[:, :, :-1]) ** 2).mean() + ((x[:, :, :, 1:] - x[:, :, :, :-1]) ** 2).mean()
            + ((x[..., 1:] - x[..., :-1]) ** 2).mean())


def kernel_times(fn):
    """{short kernel name: microseconds per call} of the device kernels of fn, from a trace of TRACED_CALLS calls"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(TRACED_CALLS):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.lower().startswith(("memcpy", "memset")):
            own = re.search(r"(\w+_kernel(?:<\w+>)?)\(", e.name)
            name = own.group(1) if own and "at::native" not in e.name else e.name.replace("void at::native::", "")[:48]
            out[name] = out.get(name, 0.0) + e.time_range.elapsed_us() / TRACED_CALLS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilagrid_timing.txt"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from edgegaussians_amd import _lib, bilagrid
    _lib.load()  # raises without the library or the GPU: no fallback
    g = torch.Generator().manual_seed(0)
    lines = [f"fused bilateral grid, fp32, {torch.cuda.get_device_name(0)}; forward + backward, microseconds of device time "
             f"per call, median of {args.calls} calls (min .. max), each between two device events, fused and composed "
             f"alternating, after {args.warmup} warm-up calls of each"]

    def report(title, fns, nbytes, parts, own):
        xs = alternating(fns, args.calls, args.warmup)
        lines.append(title)
        med = {}
        for k, v in xs.items():
            med[k] = statistics.median(v)
            lines.append(f"  {k:10s} {med[k]:9.1f} us  ({min(v):.1f} .. {max(v):.1f})   "
                         f"{nbytes[k] / med[k] * 1e-3:7.1f} GB/s of {nbytes[k] / 1e6:.1f} MB algorithmic")
        lines.append(f"  composed / fused: {med['composed'] / med['fused']:.2f}")
        for k, (fwd, bwd) in parts.items():
            try:
                nf, names_f, us_f = kernel_launches(fwd)
                nb, names_b, us_b = kernel_launches(lambda: bwd(fwd()))
                nb, names_b, us_b = nb - nf, names_b[nf:], us_b - us_f   # (the trace of the backward holds its forward)
            except Exception as e:  # the timing above stands; the counts are then not measured
                lines.append(f"  {k:10s} kernel launches: not measured (torch.profiler: {type(e).__name__}: {e})")
                continue
            lines.append(f"  {k:10s} kernel launches: forward {nf}, backward {nb}; kernel time (sum of the kernels' durations "
                         f"in a trace of {TRACED_CALLS} calls, per call): forward {us_f:.1f} us, backward {us_b:.1f} us, "
                         f"together {us_f + us_b:.1f} us")
            if k == "fused":
                mine = [sum(own in x for x in names) for names in (names_f, names_b)]
                lines.append(f"             of them kernels of the fused entry: forward {mine[0]}, backward {mine[1]} (the rest: "
                             f"the zeroing of v_grids, autograd's accumulation into the leaves)")
                try:
                    per = kernel_times(lambda: bwd(fwd()))
                    lines.append("             per kernel, forward + backward: " + ", ".join(f"{n} {us:.1f} us" for n, us in per.items()))
                except Exception as e:
                    lines.append(f"             per kernel: not measured ({type(e).__name__}: {e})")

    eye = torch.tensor([1., 0, 0, 0, 0, 1., 0, 0, 0, 0, 1., 0]).view(1, 12, 1, 1, 1)
    for B, H, W, N in ((1, 1200, 1600, 1), (4, 800, 800, 50)):
        grids = (eye + 0.1 * torch.randn(N, 12, 8, 16, 16, generator=g)).cuda().requires_grad_(True)
        render = (torch.rand(B, H, W, 3, generator=g) ** 2).cuda().requires_grad_(True)
        ys, xs_ = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        xy = torch.stack([xs_, ys], dim=-1).cuda()[None].expand(B, H, W, 2)      # one mesh grid, stride 0 over the batch
        idx = torch.arange(0, N, max(N // B, 1))[:B].cuda()
        v = torch.randn(B, H, W, 3, generator=g).cuda()

        def fused_fwd():
            return bilagrid.slice(grids, xy, render, idx, check_idx=False)["rgb"]

        def composed_fwd():
            return torch_slice(grids, xy, render, idx)

        def fb(fwd):
            def run():
                render.grad = None
                grids.grad = None
                fwd().backward(v)
            return run

        with torch.no_grad():
            diff = float((fused_fwd() - composed_fwd()).abs().max())
        n = B * H * W
        report(f"slice [{B}, {H}, {W}, 3], {B} of {N} grids 16x16x8 vs F.grid_sample + permute + affine product: "
               f"max |fused - composed| {diff:.2e}",
               {"fused": fb(fused_fwd), "composed": fb(composed_fwd)},
               {"fused": (32 + 2 * 32 + 12) * n, "composed": (128 + 140) * n},
               {"fused": (fused_fwd, lambda o: o.backward(v)), "composed": (composed_fwd, lambda o: o.backward(v))}, "slice_")
        del grids, render, xy, v

    x = torch.randn(200, 12, 8, 16, 16, generator=g).cuda().requires_grad_(True)
    one = torch.ones((), device="cuda")

    def fb(fwd):
        def run():
            x.grad = None
            fwd().backward()
        return run

    with torch.no_grad():
        diff = abs(float(bilagrid.total_variation_loss(x)) - float(torch_tv(x)))
    report(f"total_variation_loss [200, 12, 8, 16, 16] vs the three-axis torch chain: |fused - chain| {diff:.2e}",
           {"fused": fb(lambda: bilagrid.total_variation_loss(x)), "composed": fb(lambda: torch_tv(x))},
           {"fused": 12 * x.numel(), "composed": 12 * x.numel()},
           {"fused": (lambda: bilagrid.total_variation_loss(x), lambda l: l.backward(one)),
            "composed": (lambda: torch_tv(x), lambda l: l.backward(one))}, "tv_")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
