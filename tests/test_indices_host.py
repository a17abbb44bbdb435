"""Per-pixel intersection lists without a device: the exports, the argument checks of the new entries and functions,
the float64 references of tests/indices_util.py against oracle.ref_torch.composite, and -- with the references alone --
the conditions the device tests (tests/test_gpu_indices.py) rest on."""
import numpy as np
import pytest
import torch

from tests import indices_util as IU
from tests.tile_util import BORDER_CAP

NAMES = ("rasterize_to_indices_in_range", "accumulate")
TS = (8, 16, 32)
CASES = [(ts, regime, r) for ts in TS for regime in IU.REGIMES for r in (IU.FULL,) + IU.SLICES]


def test_exported_by_the_shim_the_package_and_both_all():
    import edgegaussians_amd
    import gsplat
    from edgegaussians_amd import functional
    for name in NAMES:
        assert name in functional.__all__ and name in gsplat.__all__, name
        assert getattr(gsplat, name) is getattr(functional, name) is getattr(edgegaussians_amd.functional, name)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from edgegaussians_amd import _lib
    return _lib.load(require_device=False)


def test_entries_reject_null_pointers_by_name_and_accept_zero_sizes(lib):
    p = 64  # (a non-null address nothing reads: every check comes before the first device call)
    big = 2 ** 31 - 1
    assert lib.eg_indices_count(1, 4, None, p, p, p, p, p, 0, 8, 8, 16, 0, big, p, None) == -1
    assert b"eg_indices_count" in lib.eg_last_error_string()
    assert lib.eg_indices_count(1, 4, p, p, p, p, p, p, 0, 8, 8, 16, 0, big, None, None) == -1
    assert lib.eg_indices_count(1, 4, p, p, p, p, p, p, 0, 8, 8, 12, 0, big, p, None) == -1          # tile size
    assert lib.eg_indices_count(1, 4, p, p, p, p, p, p, 0, 8, 8, 16, -1, big, p, None) == -1         # range
    assert lib.eg_indices_count(0, 4, p, p, p, p, p, p, 0, 8, 8, 16, 0, big, p, None) == 0           # C H W == 0
    assert lib.eg_indices_count(1, 4, p, p, p, p, p, p, 0, 8, 0, 16, 0, big, p, None) == 0
    assert lib.eg_indices_count(1, 0, p, p, p, p, p, p, 0, 8, 8, 16, 0, big, p, None) == 0           # N == 0
    assert lib.eg_indices_write(1, 4, p, p, p, p, p, p, 0, 8, 8, 32, 0, 1, None, 0, p, p, p, None) == -1
    assert b"eg_indices_write" in lib.eg_last_error_string()
    assert lib.eg_indices_write(1, 4, p, p, p, p, p, p, 0, 8, 8, 32, 0, 1, p, 0, p, p, None, None) == -1
    assert lib.eg_indices_write(1, 4, p, p, p, p, p, p, 0, 8, 8, 32, 0, 1, p, -1, p, p, p, None) == -1
    assert lib.eg_indices_write(1, 0, p, p, p, p, p, p, 0, 8, 8, 32, 0, 1, p, 0, p, p, p, None) == 0
    assert lib.eg_accumulate_fwd(None, p, 3, 3, p, p, 4, 9, p, 3, None, None, None) == -1
    assert b"eg_accumulate_fwd" in lib.eg_last_error_string()
    assert lib.eg_accumulate_fwd(p, p, 3, 33, p, p, 4, 9, p, 3, None, None, None) == -1              # chunk width
    assert lib.eg_accumulate_fwd(p, p, 2, 3, p, p, 4, 9, p, 3, None, None, None) == -1               # stride < channels
    assert lib.eg_accumulate_fwd(p, p, 3, 3, p, p, 0, 9, p, 3, None, None, None) == 0                # P == 0
    assert lib.eg_accumulate_bwd(p, p, 3, 3, p, p, 4, 9, None, p, 3, None, p, 0, p, None) == -1
    assert b"eg_accumulate_bwd" in lib.eg_last_error_string()
    assert lib.eg_accumulate_bwd(p, p, 3, 3, p, p, 0, 9, p, p, 3, None, p, 0, p, None) == 0


def test_functions_refuse_cpu_tensors_and_bad_arguments():
    from edgegaussians_amd import functional as Fn
    Cn, N, Wd, Ht = 1, 3, 16, 16
    T, m, con, op = torch.ones(Cn, Ht, Wd), torch.zeros(Cn, N, 2), torch.ones(Cn, N, 3), torch.ones(Cn, N)
    offs, flat = torch.zeros(Cn, 1, 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="tile_size"):
        Fn.rasterize_to_indices_in_range(0, 1, T, m, con, op, Wd, Ht, 12, offs, flat)
    with pytest.raises(ValueError, match="range_start"):
        Fn.rasterize_to_indices_in_range(-1, 1, T, m, con, op, Wd, Ht, 16, offs, flat)
    # a huge range_end passes the range check (the next thing refused is the CPU tensor) and is clamped for the int32
    with pytest.raises(ValueError, match="device tensor"):
        Fn.rasterize_to_indices_in_range(0, 10 ** 10, T, m, con, op, Wd, Ht, 16, offs, flat)
    assert Fn._clamp_range(3, 10 ** 10) == (3, 2 ** 31 - 1) and Fn._clamp_range(10 ** 12, 10 ** 13)[0] < 2 ** 31
    with pytest.raises(ValueError, match="means2d"):
        Fn.rasterize_to_indices_in_range(0, 1, T, m[0], con, op, Wd, Ht, 16, offs, flat)
    ids = torch.zeros(0, dtype=torch.int64)
    with pytest.raises(ValueError, match="device tensor"):
        Fn.accumulate(m, con, op, torch.ones(Cn, N, 3), ids, ids, ids, Wd, Ht)
    if torch.cuda.is_available():
        d = lambda t: t.cuda()
        with pytest.raises(TypeError, match="flatten_ids"):
            Fn.rasterize_to_indices_in_range(0, 1, d(T), d(m), d(con), d(op), Wd, Ht, 16, d(offs), d(flat).long())
        with pytest.raises(ValueError, match="transmittances"):
            Fn.rasterize_to_indices_in_range(0, 1, d(T)[:, :8], d(m), d(con), d(op), Wd, Ht, 16, d(offs), d(flat))
        with pytest.raises(ValueError, match="colors"):
            Fn.accumulate(d(m), d(con), d(op), d(torch.ones(Cn, N)), d(ids), d(ids), d(ids), Wd, Ht)
        with pytest.raises(TypeError, match="gaussian_ids"):
            Fn.accumulate(d(m), d(con), d(op), d(torch.ones(Cn, N, 3)), d(ids).int(), d(ids), d(ids), Wd, Ht)


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", IU.REGIMES)
@pytest.mark.parametrize("ts", TS)
def test_references_against_the_oracle_composite(ts, regime):
    """Reference (a) on the full range lists, per pixel, exactly the entries oracle.ref_torch.composite composites (its
    last_ids names the pixel's last listed Gaussian, its alphas are 1 - the walk's final T), and reference (b) on those
    lists gives the oracle's image and alphas, all in float64."""
    from oracle import ref_torch as O
    name = IU.SCENE_OF[ts]
    sc, ls = IU.scene(name), IU.lists(name, ts)
    k = IU.call(ts, regime, *IU.FULL)
    m, con, op = IU.tensors(name, regime, torch.float64)
    col = IU.colors(name, 3).double()
    tw, th = IU.grid(ts)
    starts, counts = IU.segments(k)
    assert counts.sum() == k.gaussian_ids.size and np.array_equal(counts.reshape(IU.C, IU.H, IU.W), k.counts)
    r_b, a_b = IU.ref_accumulate(m, con, op, col, k.gaussian_ids, k.pixel_ids, k.camera_ids)
    for c in range(IU.C):
        offs = ls[c].offsets[:-1].reshape(th, tw).astype(np.int32)
        render, alphas, last_ids = O.composite(m[c], con[c], col[c], op[c], IU.W, IU.H, ts, offs, ls[c].flat.astype(np.int32))
        cnt = counts[c * IU.HW:(c + 1) * IU.HW]
        st = starts[c * IU.HW:(c + 1) * IU.HW]
        has = cnt > 0
        last_gid = k.gaussian_ids[(st + cnt - 1)[has]]
        lid = last_ids.reshape(-1).numpy()
        assert np.array_equal(ls[c].flat[lid[has]], last_gid)
        assert np.all(lid[~has] == 0) and np.all(alphas.reshape(-1).numpy()[~has] == 0.0)
        assert np.abs(alphas[..., 0].numpy() - (1.0 - k.T_out[c])).max() <= 1e-12
        assert (r_b[c] - render).abs().max() <= 1e-12 and (a_b[c] - alphas).abs().max() <= 1e-12


def _tile_batches(ts):
    """int [C,H,W]: the number of batches of the list of each pixel's tile"""
    ls = IU.lists(IU.SCENE_OF[ts], ts)
    tw, _th = IU.grid(ts)
    ii, jj = np.meshgrid(np.arange(IU.H), np.arange(IU.W), indexing="ij")
    tile = (ii // ts) * tw + jj // ts
    return np.stack([-(-np.diff(l.offsets)[tile] // (ts * ts)) for l in ls])


def test_conditions_of_the_device_tests():
    for ts, regime, r in CASES:
        k = IU.call(ts, regime, *r)
        assert k.mask.mean() <= BORDER_CAP, (ts, regime, r, float(k.mask.mean()))
    for ts in TS:
        lens = np.stack([np.diff(l.offsets) for l in IU.lists(IU.SCENE_OF[ts], ts)])
        nb = _tile_batches(ts)
        thin, thick = IU.call(ts, "thin", *IU.FULL), IU.call(ts, "thick", *IU.FULL)
        assert not thin.stopped.any()
        assert thin.gaussian_ids.size > 0 and (thin.counts == 0).any()
        # entries on both sides of the 1/255 cut: the walk looks at more entries than it records
        assert (thin.looked > thin.counts).any()
        assert thick.stopped.mean() >= 0.10
        assert (thick.stopped & (thick.stop_batch < nb - 1)).any()
        # the slices: several batches, every tile exhausted at batch 5, a pixel that stopped in batch 0 resumes in batch 1
        assert lens.max() > ts * ts and lens.max() <= 5 * ts * ts
        for regime in IU.REGIMES:
            assert IU.call(ts, regime, 5, 9).gaussian_ids.size == 0
            assert IU.call(ts, regime, 1, 2).gaussian_ids.size > 0
        k0, k1 = IU.call(ts, "thick", 0, 1), IU.call(ts, "thick", 1, 2)
        assert (k0.stopped & (k1.counts > 0)).any()
        if ts == 8:
            assert (lens == 0).any() and lens.max() > 2 * 64
        if ts == 32:
            assert (lens[:, 0] > 1024).all() and (lens[:, 1:] < 1024).all()
    # the cameras see different subsets, and some depths tie exactly
    for name in IU.SCENES:
        sc = IU.scene(name)
        assert ((sc.radii[0] > 0) != (sc.radii[1] > 0)).any()
        assert all(np.unique(sc.depths[c]).size < sc.N for c in range(IU.C))


def test_local_lists_reads_the_global_offsets_like_the_oracle_lists():
    """The clamped per-camera form (what the device reads) of the scenes' global offsets is the oracle's lists."""
    for ts in TS:
        name = IU.SCENE_OF[ts]
        offs, flat = IU.device_lists(name, ts)
        base = 0
        for got, want in zip(IU.local_lists(offs.numpy(), flat.numpy(), IU.scene(name).N), IU.lists(name, ts)):
            assert np.array_equal(got.offsets - base, want.offsets)
            assert np.array_equal(got.flat[base:base + want.flat.size], want.flat)
            base += want.flat.size
