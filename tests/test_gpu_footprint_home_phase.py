"""The home phase of the footprint backward (csrc/footprint_dev.h): the sizing lanes of a workgroup size its footprints, deal
every wave's 64 lanes to its 8 Gaussians (csrc/deal_rule.h) and stage the Gaussians' records in LDS; behind the barrier a
lane takes its Gaussian, its place and its record from there.  The cases (tests/footprint_home_util.py, their premises
checked on the host by tests/test_footprint_home_host.py) are those at which the dealing or the staging can go wrong:
ragged last waves and workgroups, a screen-filling footprint among seven tiny ones, dead Gaussians between live ones, a
wave without any footprint between live waves, equal footprints (the slack goes to the first groups), one-cell footprints
(lanes without a pair), record images with zeros, stops and depth ties on the stop Gaussian; on 64 x 48 and 40 x 24 images.

Each case runs eg_composite_bwd_footprint (footprint_bwd_kernel) and is checked two ways:
  1. every Gaussian and column group against the float64 footprint sum, within the row bound of
     tests/test_gpu_step_composite.py (CU.grad_row_check, scale 1.0, rows whose reference is zero exactly zero);
  2. word for word against tests/golden/footprint_g2d_parent.npz: the g2d words of the build in which every wave dealt its own
     lanes and every lane gathered its record from global memory (tools/record_footprint_golden.py, recorded on an
     MI355X).  The home phase moves where the dealing runs, not what it computes: not a bit may change.

The one-kernel backward (backward_fused.hip) runs the same device functions and keeps g2d in LDS: a run of steps on a
37-Gaussian scene of mixed footprint sizes must leave the very parameters, moments and absgrads the two-kernel path leaves.

Measured on the MI355X: all 36 cases word-identical to the recorded build; largest ratio to the row bound 0.023
(stops_ties-64x48, v_opacities).
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import footprint_home_util as U
from tests import step_composite_util as SU
from tests.test_gpu_step_composite import _footprint, _rows_check
from tests.util import record

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "footprint_g2d_parent.npz")


@pytest.fixture(scope="module")
def lib():
    from edgegaussians_amd import _lib
    _lib.load()  # raises if the .so or the GPU is missing: no fallback
    return _lib


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", U.CASES)
def test_rows_equal_float64_sums_and_the_recorded_words(lib, golden, name):
    c, r = U.case(name), U.reference(name)
    got = _footprint(c.rec, SU.device_image(c.img), c.W, c.H)
    ratios = _rows_check(got, r.ref, r.kappa, f"home phase {name}")
    words = np.ascontiguousarray(got.numpy()).view(np.uint32)
    want = golden[U.golden_key(name)]
    assert want.dtype == np.uint32 and want.shape == words.shape, (want.dtype, want.shape, words.shape)
    diff = words != want
    print(f"{name}: ratio to the row bound {ratios}, {int(diff.sum())} of {diff.size} words differ")
    record("footprint_home_phase_rows", case=name, rows=int(c.rec.shape[0]), ratio_to_row_bound=ratios,
           words_differing=int(diff.sum()))
    assert not diff.any(), (f"{name}: {int(diff.sum())} g2d words differ from the recorded build's, first (row, column) "
                            f"{np.argwhere(diff)[0].tolist()}: {words[diff][0]:#010x} != {want[diff][0]:#010x}")


def test_one_kernel_backward_equals_the_two_kernels_on_37_gaussians(lib):
    """9 steps on 37 Gaussians (one ragged workgroup of either kernel, 3 x 2 tiles of a 40 x 24 image) whose log-scales
    spread over three decades: waves that hold an image-filling footprint beside sub-pixel ones."""
    from edgegaussians_amd import EdgeTrainer, LRSchedule, synth
    sc = synth.make_scene(37, 4, 40, 24, seed=5, scale=0.05, spread_opacity=True)
    sc.log_scales += math.log(10.0) * (3.0 * torch.rand(37, 1, generator=torch.Generator().manual_seed(50)) - 1.5)
    sched = LRSchedule(scales_start=0, quats_start=0, opacities_start=0)
    mk = lambda: EdgeTrainer(sc.means, sc.log_scales, sc.quats, sc.logit_opacities, sc.viewmats, sc.Ks, sc.gt,  # noqa: E731
                             sc.width, sc.height, schedule=sched)
    ta, tb = mk(), mk()
    ta.two_kernel_backward = 1
    ta.ensure_capacity(); tb.ensure_capacity()
    assert tb.fused_backward_active() and not ta.fused_backward_active()
    views = [(3 * i + 1) % 4 for i in range(9)]
    wm = [synth.weight_map(("weighted", "whole", "bg_edge_ratio")[i % 3], sc.gt[v], generator=torch.Generator().manual_seed(i)).cuda()
          for i, v in enumerate(views)]
    for t in (ta, tb):
        t.train_steps(views[:4], wm[:4])
        t.train_steps(views[4:], wm[4:])
    la, lb = ta.pop_loss(), tb.pop_loss()
    assert abs(la - lb) <= 1e-6 * abs(la), (la, lb)  # (the loss terms meet in float atomics)
    assert not ta.overflowed() and not tb.overflowed()
    assert float(ta.absgrads.abs().sum()) > 0.0, "the scene must reach the image"
    for k, v in ta.state_dict().items():
        assert torch.equal(tb.state_dict()[k], v), f"one-kernel backward: {k} differs from the two-kernel path"
    for name in ("absgrads", "adam_m", "adam_v"):
        assert torch.equal(getattr(tb, name), getattr(ta, name)), name
