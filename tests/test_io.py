"""PLY / state-dict hand-off (reference io_utils.py:4-39, edge_gs.py:625-642)."""
import json
import os

import numpy as np
import torch

from edgegaussians_amd import io as egio


def test_ply_roundtrip_and_layout(tmp_path):
    g = np.random.default_rng(0)
    n = 37
    means, scales = g.normal(size=(n, 3)).astype(np.float32), g.uniform(0.001, 0.1, (n, 3)).astype(np.float32)
    quats, op = g.normal(size=(n, 4)).astype(np.float32), g.uniform(0, 1, (n, 1)).astype(np.float32)
    p = str(tmp_path / "g.ply")
    egio.write_gaussian_params_as_ply(means, scales, quats, op, p)
    raw = open(p, "rb").read()
    head, body = raw.split(b"end_header\n")
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 37\nproperty float x\n")
    assert [ln.split()[-1] for ln in head.decode().splitlines() if ln.startswith("property")] == \
        ["x", "y", "z", "scale1", "scale2", "scale3", "quat1", "quat2", "quat3", "quat4", "opacity"]
    assert len(body) == n * 11 * 4
    rec = np.frombuffer(body, dtype="<f4").reshape(n, 11)
    assert np.array_equal(rec[:, :3], means) and np.array_equal(rec[:, 6:10], quats) and np.array_equal(rec[:, 10:], op)
    pos, s2, q2, o2 = egio.read_gaussian_params_from_ply(p)
    assert np.array_equal(pos, means) and np.array_equal(s2, scales) and np.array_equal(q2, quats) and np.array_equal(o2, op)


def test_export_from_state_dict_applies_activations(tmp_path):
    st = {"gauss_params.means": torch.randn(5, 3), "gauss_params.scales": torch.full((5, 3), float(np.log(0.004))),
          "gauss_params.quats": torch.randn(5, 4), "gauss_params.opacities": torch.logit(torch.full((5, 1), 0.08))}
    p = str(tmp_path / "e.ply")
    egio.export_as_ply(st, p)
    pos, sc, q, op = egio.read_gaussian_params_from_ply(p)
    assert np.allclose(sc, 0.004, rtol=1e-6) and np.allclose(op, 0.08, rtol=1e-6) and op.shape == (5, 1)
    assert np.allclose(pos, st["gauss_params.means"].numpy()) and np.allclose(q, st["gauss_params.quats"].numpy())


def test_reads_what_the_reference_reader_expects(tmp_path, golden_dir):
    """The reference's reader indexes the vertex element by these exact property names (tests/golden/
    ply_reader_fields.json: the keys its read_gaussian_params_from_ply asked a logging stub for, make_golden.py)."""
    asked = json.load(open(os.path.join(golden_dir, "ply_reader_fields.json")))["read_gaussian_params_from_ply"]
    for name in egio._PLY_DTYPE.names:
        assert name in asked
    assert sorted(asked) == sorted(egio._PLY_DTYPE.names)
