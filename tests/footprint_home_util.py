"""Cases of the footprint backward's home phase (csrc/footprint_dev.h: the sizing lanes size the workgroup's footprints, deal
every wave's 64 lanes to its 8 Gaussians and stage the Gaussians' records in LDS): hand-built splat records and record
images at which the dealing or the staging can go wrong.  Shared by tests/test_gpu_footprint_home_phase.py and
tools/record_footprint_golden.py (which records the g2d words a library computes for them); numpy only, no device.

Every case is built once (lru_cache) and never modified.  Images: 64 x 48 and 40 x 24 (not a multiple of the 16-pixel tile).
Sizes: N in SIZES -- one lane's worth, a ragged and a full wave, a wave and a workgroup plus one, 37, two workgroups of
the two-kernel path / one of the one-kernel path, and that plus one.
"""
import collections
import functools

import numpy as np

from tests import step_composite_util as SU

IMAGES = ((64, 48), (40, 24))
SIZES = (1, 7, 8, 9, 31, 32, 33, 37, 64, 65)
SPECIAL = ("huge_among_tiny", "dead_alternating", "dead_wave", "equal7", "equal8", "one_cell8", "one_cell3", "stops_ties")
CASES = tuple(f"{kind}-{W}x{H}" for W, H in IMAGES for kind in tuple(f"n{n}" for n in SIZES) + SPECIAL)

HomeCase = collections.namedtuple("HomeCase", "name rec W H img")
RefCase = collections.namedtuple("RefCase", "ref kappa")


def _dead(rec, rows):
    """rows of `rec` made invisible: radius 0 and opacity below 1 / 255 in turn"""
    for i, k in enumerate(rows):
        if i % 2 == 0:
            rec[k, 7] = np.int32(0).view(np.float32)
        else:
            rec[k, 5] = np.float32(0.0035)
    return rec


def _equal(n, W, H, sigma, op):
    """n round Gaussians of one shape whose centres differ by whole pixels, all inside the image and one tile box class:
    the same footprint, cell for cell"""
    xy = np.array([(8.5 + 3.0 * (k % 4), 8.5 + 3.0 * (k // 4)) for k in range(n)])
    return SU.ellipse_records(xy, np.full(n, sigma), np.ones(n), np.zeros(n), np.full(n, op), 1.0 + 0.25 * np.arange(n))


def cells_of(rec, W, H):
    """cells of every footprint as walk_of sizes it (numpy fp32 model: SU.walk_ints)"""
    fw, fh, pw = SU.walk_ints(rec, W, H)
    return np.minimum(pw, fw) * fh


@functools.lru_cache(maxsize=None)
def case(name):
    kind, size = name.split("-")
    W, H = (int(t) for t in size.split("x"))
    seed = 1000 + 17 * CASES.index(name)
    kw = {}
    if kind.startswith("n"):
        n = int(kind[1:])
        rec = SU.random_records(n, seed, W, H, sigma=(0.6, 4.0))
        if n == 1:
            rec[0, 0:2] = (W * 0.4 + 0.3, H * 0.6 - 0.2)
    elif kind == "huge_among_tiny":
        # four waves: one screen-filling Gaussian among seven of about a pixel, at lane group 0, 3, 7 and 5
        rec = np.concatenate([SU.mix_wave(pos, seed + pos, W, H) for pos in (0, 3, 7, 5)])
    elif kind == "dead_alternating":
        rec = SU.random_records(32, seed, W, H, sigma=(0.8, 3.0), capped_share=0.0)
        rec[:, 0] = np.clip(rec[:, 0], 4.0, W - 4.0)
        rec[:, 1] = np.clip(rec[:, 1], 4.0, H - 4.0)
        _dead(rec, list(range(0, 8, 2)) + list(range(9, 16, 2)) + [16, 17, 20, 21] + [25, 26, 27, 30])
    elif kind == "dead_wave":
        # 31 rows: a live wave, a wave without any footprint (total == 0), a live wave, a ragged live wave
        rec = SU.random_records(31, seed, W, H, sigma=(0.8, 3.0), capped_share=0.0)
        rec[:, 0] = np.clip(rec[:, 0], 4.0, W - 4.0)
        rec[:, 1] = np.clip(rec[:, 1], 4.0, H - 4.0)
        _dead(rec, range(8, 16))
    elif kind == "equal7":
        rec = _equal(7, W, H, 1.3, 0.6)    # 57 spare lanes over 7: 8 each and a slack of one, to the first group
    elif kind == "equal8":
        rec = _equal(8, W, H, 1.3, 0.6)    # 56 spare lanes over 8: the factor 1 - 1e-5 rounds 7 down to 6, a slack of 8
    elif kind == "one_cell8":
        rec = _equal(8, W, H, 0.35, 0.005)  # o just above 1 / 255: the ellipse holds its own pixel only
    elif kind == "one_cell3":
        rec = _equal(3, W, H, 0.35, 0.005)  # 61 spare lanes on three pairs: 63 lanes, most of them without a pair
    elif kind == "stops_ties":
        # (no fp32 denormals in this image, SU.random_image's `special`: under 60 % stops and 30 % zeros a Gaussian may see
        # nothing else, and sums of denormal size have a few bits -- no relative row bound fits them;
        # tests/test_footprint_home_host.py asks every row of every case for an ordinary magnitude)
        rec = SU.random_records(37, seed, W, H, sigma=(2.0, 9.0), opacity_lo=0.05, capped_share=0.1, tie_every=3)
        kw = dict(stop_share=0.6, zero_share=0.3)
    else:
        raise ValueError(name)
    img = SU.random_image(rec, W, H, seed + 1, **kw)
    return HomeCase(name, rec, W, H, SU.masked(img, SU.record_borderline(rec, W, H)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 footprint sums [N, 8] and the row bounds' kappa of a case"""
    c = case(name)
    return RefCase(*SU.record_kappa(c.rec, c.img, c.W, c.H))


def golden_key(name):
    return name.replace("-", "_")


def lanes_of(cells):
    """the dealing rule (csrc/deal_rule.h) on one wave's cell counts, exact division in place of the device's reciprocal:
    (n, first) per group -- for the host-side premises of the cases only"""
    cells = np.asarray(cells, np.int64)
    live, total = int((cells > 0).sum()), int(cells.sum())
    if total == 0:
        return np.zeros(8, np.int64), np.zeros(8, np.int64)
    share = np.float32(np.float32(64 - live) * np.float32(1.0 - 1e-5)) * (np.float32(1.0) / np.float32(total))
    n = np.where(cells > 0, 1 + (cells.astype(np.float32) * share).astype(np.int64), 0)
    slack = 64 - int(n.sum())
    rank = np.cumsum(cells > 0) - (cells > 0)
    first = np.cumsum(n) - n + np.minimum(rank, slack)
    return n + ((cells > 0) & (rank < slack)), first

