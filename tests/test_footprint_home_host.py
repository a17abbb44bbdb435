"""Host side of the home-phase tests of the footprint backward: the premises of the cases of tests/footprint_home_util.py
(what tests/test_gpu_footprint_home_phase.py runs on the device), the recorded words' file, and the lane dealing rule
(csrc/deal_rule.h) through its stand-alone test program tests/host/deal_rule_test.cpp."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import footprint_home_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _waves(name):
    c = U.case(name)
    cells = U.cells_of(c.rec, c.W, c.H)
    return np.concatenate([cells, np.zeros((-len(cells)) % 8, np.int64)]).reshape(-1, 8)


def test_the_sizes_and_images_the_cases_cover():
    assert U.SIZES == (1, 7, 8, 9, 31, 32, 33, 37, 64, 65) and U.IMAGES == ((64, 48), (40, 24))
    for name in U.CASES:
        c = U.case(name)
        assert (c.W, c.H) in U.IMAGES and c.rec.shape[0] in U.SIZES + (3,), name
        assert (c.img.gT == 0.0).any() and (c.img.gT != 0.0).any(), f"{name}: the image needs zeros beside weights"
        assert (c.img.stop_id >= 0).any() and (c.img.stop_id < 0).any(), f"{name}: stopped beside unstopped pixels"
        a = np.abs(U.reference(name).ref[:, 2:4]).max(axis=1)   # (the absgrad sums: no cancellation)
        assert ((a == 0.0) | (a > 1e-20)).all(), f"{name}: a row of fp32-denormal size has no relative bound"


@pytest.mark.parametrize("size", ["64x48", "40x24"])
def test_case_premises(size):
    W, H = (int(t) for t in size.split("x"))
    for w in _waves(f"huge_among_tiny-{size}"):
        n, _ = U.lanes_of(w)
        assert w.max() == W * H and np.sort(w)[-2] <= 9, "one screen-filling footprint among seven of a few cells"
        assert n.max() >= 54 and (n >= 1).all() and n.sum() == 64
    waves = _waves(f"dead_alternating-{size}")
    assert all(((w > 0).sum() == 4) for w in waves) and ((waves[0] > 0) != (waves[1] > 0)).all()
    waves = _waves(f"dead_wave-{size}")
    assert (waves[0] > 0).all() and (waves[1] == 0).all() and (waves[2] > 0).all() and (waves[3][:7] > 0).all()
    w7, w8 = _waves(f"equal7-{size}")[0], _waves(f"equal8-{size}")[0]
    assert len(set(w7[:7])) == 1 and w7[7] == 0 and list(U.lanes_of(w7)[0]) == [10, 9, 9, 9, 9, 9, 9, 0]
    assert len(set(w8)) == 1 and list(U.lanes_of(w8)[0]) == [8] * 8       # 6.9999 rounds down: a slack of 8 = live
    assert list(_waves(f"one_cell8-{size}")[0]) == [1] * 8
    w3 = _waves(f"one_cell3-{size}")[0]
    assert list(w3) == [1, 1, 1, 0, 0, 0, 0, 0] and list(U.lanes_of(w3)[0][:3]) == [22, 21, 21]   # 64 lanes, 3 pairs
    c = U.case(f"stops_ties-{size}")
    dbits = c.rec[:, 6].view(np.uint32)
    stopped = c.img.stop_id >= 0
    assert stopped.mean() > 0.4 and len(set(dbits.tolist())) < len(dbits), "stops, and depths that tie bit for bit"
    assert (c.img.stop_depth[stopped] == dbits[c.img.stop_id[stopped]]).all()


def test_recorded_words_cover_every_case():
    path = os.path.join(ROOT, "tests", "golden", "footprint_g2d_parent.npz")
    assert os.path.getsize(path) < 256 * 1024
    with np.load(path) as z:
        assert sorted(z.files) == sorted(U.golden_key(n) for n in U.CASES)
        for name in U.CASES:
            a = z[U.golden_key(name)]
            assert a.dtype == np.uint32 and a.shape == (U.case(name).rec.shape[0], 8), name
            assert np.isfinite(a.view(np.float32)).all(), name


def test_deal_rule_program(tmp_path):
    """builds tests/host/deal_rule_test.cpp (plain; the sanitizer build is the command in its header) and runs it"""
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "deal_rule_test")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "edgegaussians_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "deal_rule_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
