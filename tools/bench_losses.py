"""Times the fused scalar losses (edgegaussians_amd.losses) against the compositions they replace, on the same GPU in the
same run, and writes profiles/losses_timing.txt.

    python tools/bench_losses.py [--out profiles/losses_timing.txt] [--calls 100] [--warmup 20]

* projection_loss at 1x800x800 on channel 0 of a [1, 800, 800, 3] render (the reference's native image size), read in
  place, against the reference's torch chain: clamp, channel selection, subtract, abs, multiply by the weight mask, mean
  (edge_gs.py: get_outputs + compute_projection_loss, strategy "weighted").
* photometric_loss at 1x3x1200x1600 on the permuted view of a [1, 1200, 1600, 3] render and on NCHW, against
  0.8 * l1 + 0.2 * (1 - fused_ssim) with torch's L1 and edgegaussians_amd.ssim.fused_ssim.

Per configuration: forward + backward of the scalar down to the render's gradient, device time between two device
events per call, fused and composed calls alternating, median (min .. max) over `--calls` calls after `--warmup`
calls of each: the call as a trainer pays it, host dispatch included.  Kernel launches per direction, and the time
the device spends in them (the sum of the kernels' durations), come from a torch.profiler trace of ten calls, taken
after the timing.

Bytes are the algorithmic ones: the pointwise forward reads 4 (x) + 4 (y) + 4 (w) per element and the backward the same
and writes 4; the photometric forward reads 8 and writes 12 (three derivative maps), its backward reads 12 + 8 and
writes 4 per pixel-channel."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def alternating(fns, calls, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            out[k].append(timed(fn))
    return out


TRACED_CALLS = 10


def kernel_launches(fn):
    """(device kernels one call of fn enqueues, their names, the sum of their durations in microseconds per call) from
    a trace of TRACED_CALLS calls"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(TRACED_CALLS):
            fn()
        torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
              and not e.name.lower().startswith(("memcpy", "memset"))]
    names = [e.name for e in events]
    return len(names) // TRACED_CALLS, names[:len(names) // TRACED_CALLS], sum(e.time_range.elapsed_us() for e in events) / TRACED_CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_timing.txt"))
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from edgegaussians_amd import _lib, losses, synth
    from edgegaussians_amd.ssim import fused_ssim
    _lib.load()  # raises without the library or the GPU: no fallback
    g = torch.Generator().manual_seed(0)
    one = torch.ones((), device="cuda")  # the cotangent of the launch counts: given, so that autograd fills none
    lines = [f"fused scalar losses, fp32, {torch.cuda.get_device_name(0)}; forward + backward, microseconds of device time "
             f"per call, median of {args.calls} calls (min .. max), each between two device events, fused and composed "
             f"alternating, after {args.warmup} warm-up calls of each"]

    def report(title, fns, nbytes, parts):
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
                own = [sum(("loss_" in x or "photometric_" in x) for x in names) for names in (names_f, names_b)]
                lines.append(f"             of them kernels of the fused entry: forward {own[0]}, backward {own[1]} (the rest "
                             f"is autograd's backward of the caller's view of the render)")
                lines.append(f"             forward: {', '.join(names_f)}")
                lines.append(f"             backward: {', '.join(names_b)}")

    # ---- projection loss, 1 x 800 x 800 from a [1, 800, 800, 3] render
    H = W = 800
    render = (torch.rand(1, H, W, 3, generator=g) * 1.2 - 0.1).cuda().requires_grad_(True)
    gt_cpu = (torch.rand(H, W, generator=g) > 0.95).float()
    gt = gt_cpu.cuda()
    wmap = synth.weight_map("weighted", gt_cpu).cuda()          # sum_p w_p |.| form: weight_mask / HW
    weight_mask = (wmap * (H * W)).contiguous()                  # the reference's weight mask

    def fused_fwd():
        return losses.projection_loss(render[0, ..., 0], gt, wmap)

    def chain_fwd():
        rgb = torch.clamp(render[:, ..., :3], 0.0, 1.0).squeeze(0)
        return torch.mean(weight_mask * torch.abs(rgb[..., 0] - gt))

    def fb(fwd):
        def run():
            render.grad = None
            fwd().backward()
        return run

    diff = abs(float(fused_fwd()) - float(chain_fwd()))
    n = H * W
    report(f"projection_loss 1x{H}x{W} on render[0, ..., 0] of [1, {H}, {W}, 3] vs the reference's torch chain: "
           f"|fused - chain| {diff:.2e}",
           {"fused": fb(fused_fwd), "composed": fb(chain_fwd)}, {"fused": (12 + 16) * n, "composed": (12 + 16) * n},
           {"fused": (fused_fwd, lambda l: l.backward(one)), "composed": (chain_fwd, lambda l: l.backward(one))})

    # ---- photometric loss, 1 x 3 x 1200 x 1600
    H, W = 1200, 1600
    for layout in ("channels_last", "nchw"):
        shape = (1, H, W, 3) if layout == "channels_last" else (1, 3, H, W)
        leaf = (torch.rand(shape, generator=g) ** 6).cuda().requires_grad_(True)
        target = (torch.rand(shape, generator=g) ** 6).cuda()

        def views():
            return (leaf.permute(0, 3, 1, 2), target.permute(0, 3, 1, 2)) if layout == "channels_last" else (leaf, target)

        def fused_fwd():
            x1, x2 = views()
            return losses.photometric_loss(x1, x2, 0.2)

        def composed_fwd():
            x1, x2 = views()
            return 0.8 * (x1 - x2).abs().mean() + 0.2 * (1.0 - fused_ssim(x1, x2))

        def fb(fwd):
            def run():
                leaf.grad = None
                fwd().backward()
            return run

        diff = abs(float(fused_fwd()) - float(composed_fwd()))
        n = 3 * H * W
        report(f"photometric_loss 1x3x{H}x{W} {layout} vs 0.8 l1 + 0.2 (1 - fused_ssim): |fused - composed| {diff:.2e}",
               {"fused": fb(fused_fwd), "composed": fb(composed_fwd)},
               {"fused": (20 + 24) * n, "composed": (20 + 24) * n},
               {"fused": (fused_fwd, lambda l: l.backward(one)), "composed": (composed_fwd, lambda l: l.backward(one))})
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
