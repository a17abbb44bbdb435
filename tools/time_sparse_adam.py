"""Times one optimizer step on the sparse gradients of a packed rasterization call, three ways:

  (a) torch.optim.SparseAdam                     (coalesce, sparse_mask, sparse constructors, element-wise launches)
  (b) edgegaussians_amd.optim.Adam               on the gradient ALREADY densified to [N, w] (the densify is not timed)
  (c) edgegaussians_amd.optim.SparseAdam         (one launch; a stable sort of the indices first when uncoalesced)

Cells: N = 100 000 rows of width 3 and 4; 10 / 50 / 100 % of the rows visible per camera; one camera (a coalesced
gradient) and three cameras (three ascending runs, uncoalesced).  One process; after a warm-up the candidates alternate
step by step, each step between two device events on the current stream, so a figure is the time the stream spends on a
step INCLUDING the gaps in which the device waits for the host to dispatch.  For (c) the table also gives the bytes its
algorithm has to move per step -- 7 x 4 x w per stepped row (p, m, v read and written, the summed gradient read once),
the values of duplicate rows, and 8 per index entry (16 with the permutation) -- over the measured time: an ALGORITHMIC
rate, not a measured traffic.

    python tools/time_sparse_adam.py [--steps 200] [--warmup 20] [--out FILE]

Needs the GPU: there is nothing to time without it.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_cell(N, w, share, cams, seed):
    rng = np.random.default_rng(seed)
    k = max(1, int(round(share * N)))
    idx = np.concatenate([np.sort(rng.choice(N, k, replace=False)) for _ in range(cams)])
    vals = (rng.standard_normal((idx.size, w)) * 1e-3).astype(np.float32)
    i, x = torch.from_numpy(idx).cuda()[None], torch.from_numpy(vals).cuda()
    sparse = torch.sparse_coo_tensor(i, x, size=(N, w), is_coalesced=(cams == 1))
    dense = torch.zeros(N, w, device="cuda").index_add_(0, i[0], x)
    return sparse, dense, int(np.unique(idx).size), int(idx.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/time_sparse_adam.py needs the GPU")
    if args.steps < 200:
        sys.exit("at least 200 timed steps per cell")
    from edgegaussians_amd import optim

    N = 100000
    lines = [f"{torch.cuda.get_device_name(0)}; N = {N}; {args.warmup} warm-up + {args.steps} timed steps per cell and candidate, "
             "alternating; median us per step between device events (host dispatch gaps included)",
             "(a) torch.optim.SparseAdam   (b) optim.Adam on the densified gradient   (c) optim.SparseAdam",
             f"{'w':>2} {'cams':>4} {'visible':>7} {'nnz':>7} {'rows':>7} | {'(a) us':>8} {'(b) us':>8} {'(c) us':>8} | {'a/c':>6} {'b/c':>6} | "
             f"{'(c) algorithmic MB':>18} {'GB/s':>7}"]
    for w in (3, 4):
        for cams in (1, 3):
            for share in (0.1, 0.5, 1.0):
                sparse, dense, rows, nnz = make_cell(N, w, share, cams, 7)
                init = torch.randn(N, w, device="cuda")
                ps = [torch.nn.Parameter(init.clone()) for _ in range(3)]
                opts = [torch.optim.SparseAdam([ps[0]], lr=1e-3), optim.Adam([ps[1]], lr=1e-3), optim.SparseAdam([ps[2]], lr=1e-3)]
                grads = [sparse, dense, sparse]
                ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                      for _ in range(3)]
                for s in range(-args.warmup, args.steps):
                    for c in range(3):
                        ps[c].grad = grads[c]
                        if s >= 0:
                            ev[c][s][0].record()
                        opts[c].step()
                        if s >= 0:
                            ev[c][s][1].record()
                torch.cuda.synchronize()
                us = [1e3 * float(np.median([a.elapsed_time(b) for a, b in ev[c]])) for c in range(3)]
                mb = (rows * 6 * 4 * w + nnz * 4 * w + nnz * (8 if cams == 1 else 16)) / 1e6
                lines.append(f"{w:>2} {cams:>4} {int(100 * share):>6}% {nnz:>7} {rows:>7} | {us[0]:>8.1f} {us[1]:>8.1f} {us[2]:>8.1f} | "
                             f"{us[0] / us[2]:>6.2f} {us[1] / us[2]:>6.2f} | {mb:>18.3f} {mb * 1e6 / (us[2] * 1e-6) / 1e9:>7.1f}")
                agree = float((ps[0].detach() - ps[2].detach()).abs().max())
                assert agree < 1e-4, f"(a) and (c) disagree: {agree}"
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
