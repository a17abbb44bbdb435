"""Records the g2d words a build of libedgegs.so computes for the home-phase cases of the footprint backward
(tests/footprint_home_util.py) -- the yardstick of tests/test_gpu_footprint_home_phase.py, which asks a later build for
the very same words.

    python tools/record_footprint_golden.py --lib OTHER_TREE/edgegaussians_amd/libedgegs.so --out tests/golden/footprint_g2d_parent.npz

--lib: the library to record, by default this tree's own; to pin a change of the kernel to its parent commit, build the
parent in a checkout of its own and point --lib at its library.  Needs the GPU.  One uint32 array [N, 8] per case.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from edgegaussians_amd import _lib
    if args.lib is not None:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    _lib.load()
    from edgegaussians_amd._lib import call, ptr, stream
    from tests import footprint_home_util as U
    from tests import step_composite_util as SU
    out = {}
    for name in U.CASES:
        c = U.case(name)
        N = c.rec.shape[0]
        splat = torch.from_numpy(np.ascontiguousarray(c.rec)).cuda().contiguous()
        gtstop = torch.from_numpy(SU.device_image(c.img)).cuda().contiguous()
        g2d = torch.full((N, 8), float("nan"), device="cuda")
        call("eg_composite_bwd_footprint", ptr(splat), N, c.W, c.H, gtstop.data_ptr(), ptr(g2d), stream())
        torch.cuda.synchronize()
        words = np.ascontiguousarray(g2d.cpu().numpy()).view(np.uint32)
        assert np.isfinite(words.view(np.float32)).all(), f"{name}: rows left unwritten"
        out[U.golden_key(name)] = words
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"{len(out)} cases, {sum(v.shape[0] for v in out.values())} rows from {_lib.LIB_PATH} -> {args.out}")


if __name__ == "__main__":
    main()
