"""The conditions the device tests of the densify / cull kernels (tests/test_gpu_densify.py) rest on, checked on the CPU
with the references alone (tests/util.py): the float64 projection-vote references reproduce the reference
implementation's own outputs (tests/golden/densify_cull.npz, filter_projection.npz); on every vote scene the rows whose
rounding or division is borderline are at most 1 %, so that a wrong kernel cannot hide among them; the exact block means
what it says; the trainer-level case has no borderline row at all and every event moves rows."""
import os

import numpy as np
import pytest
import torch

from tests import util as U
from tests.util import record_cpu

W, H = U.VOTE_SIZE
VOTE_CASES = [(n, V) for n in (1, 255, 256, 257, 1000) for V in (1, 4)]


def test_vote_reference_reproduces_the_not_projecting_cull(golden_dir):
    d = np.load(os.path.join(golden_dir, "densify_cull.npz"))
    cams = np.load(os.path.join(golden_dir, "cameras_00004926.npz"))
    edges = np.load(os.path.join(golden_dir, "edges_00004926.npz"))
    views = list(edges["views"])
    h, w = int(cams["height"]), int(cams["width"])
    masks = np.zeros((len(views), h * w), np.uint8)
    for i, k in enumerate(views):
        masks[i, edges[f"idx_{k}"]] = (edges[f"val_{k}"].astype(np.float32) / np.float32(255.0)) >= 0.5
    P = torch.bmm(torch.from_numpy(cams["Ks"][views]), torch.from_numpy(cams["viewmats"][views])[:, :3, :4])
    votes, border = U.ref_project_hits(d["np_means_before"], P, masks.reshape(len(views), h, w), w, h)
    kept = np.nonzero(~(votes.astype(np.float32) / np.float32(len(views)) < 0.1))[0]
    assert np.array_equal(kept, d["np_kept_index"])
    record_cpu("densify_vote_reference_vs_golden", rows=int(votes.size), kept=int(kept.size), borderline=int(border.sum()))


def test_visibility_reference_reproduces_filter_by_projection(golden_dir):
    from edgegaussians_amd.filtering import pack_cameras
    d, images, cameras = U.filter_fixture(golden_dir)
    h, w = int(cameras[0]["h"]), int(cameras[0]["w"])
    vis, border = U.ref_project_visibility(d["means"], pack_cameras(cameras, "cpu"), np.stack(images), w, h)
    for thr in (0.1, 0.3):
        assert np.array_equal(vis / float(len(images)) > thr, d[f"inliers_{thr}"])
    assert border.mean() <= U.VOTE_MAX_BORDER


@pytest.mark.parametrize("n,V", VOTE_CASES)
def test_vote_scenes_have_few_borderline_rows_and_reach_every_outcome(n, V):
    means, P, cams, masks, maps = U.vote_scene(n, V)
    votes, border = U.ref_project_hits(means, P, masks, W, H)
    vis, border_v = U.ref_project_visibility(means, cams, maps, W, H)
    assert border.sum() <= U.VOTE_MAX_BORDER * n and border_v.sum() <= U.VOTE_MAX_BORDER * n, (int(border.sum()), int(border_v.sum()))
    assert set(np.unique(masks.numpy())) == {0, 1, 255}
    if n >= 255:
        h = (means.double() @ P[0, :, :3].double().T + P[0, :, 3].double()).numpy()
        u, v, c = h[:, 0] / h[:, 2], h[:, 1] / h[:, 2], h[:, 2]
        inside = (np.rint(u) >= 0) & (np.rint(u) < W) & (np.rint(v) >= 0) & (np.rint(v) < H)
        # inside and outside the image on every side, in front of and behind the camera, with and without a vote
        assert inside.sum() >= 50 and (u < -1).sum() >= 10 and (u > W).sum() >= 10 and (v < -1).sum() >= 10 and (v > H).sum() >= 10
        assert (c < 0).sum() >= 5 and ((c < 0) & inside).sum() >= 1
        assert (votes > 0).sum() >= 20 and (votes == 0).sum() >= 20 and (vis > 0).sum() >= 20
    record_cpu("densify_vote_scene", rows=n, views=V, borderline_share=float(border.mean()), borderline_share_visibility=float(border_v.mean()),
               rows_voting=int((votes > 0).sum()))


def test_exact_block_is_exact_and_the_references_agree_with_it():
    means, P, cams, mask, votes, pix = U.exact_vote_block()
    # every product of the projection is exact in fp32: the fp32 and the float64 evaluation agree to the last bit
    h32 = means @ P[0, :, :3].T + P[0, :, 3]
    h64 = means.double() @ P[0, :, :3].double().T + P[0, :, 3].double()
    assert torch.equal(h32.double(), h64)
    got, _ = U.ref_project_hits(means, P, mask, W, H)
    assert np.array_equal(got, votes.numpy())
    vis, _ = U.ref_project_visibility(means, cams, mask.float(), W, H)
    assert np.array_equal(vis, votes.numpy().astype(np.float64))
    u = (h64[:, 0] / h64[:, 2]).numpy()
    front = h64[:, 2].numpy() == 1.0
    for val, px in ((0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0)):        # half to even, -0.5 -> -0 -> pixel 0
        sel = front & (u == val)
        assert sel.sum() >= 4 and (pix[sel, 0].numpy() == px).all()
    assert (pix[front & (u == W - 0.5), 0].numpy() == -1).all() and (front & (u == W - 0.5)).sum() == 1 and W % 2 == 0
    behind, flat = h64[:, 2].numpy() < 0, h64[:, 2].numpy() == 0
    assert behind.sum() == 3 and (pix[behind, 0].numpy() >= 0).all() and votes[behind].sum() >= 1    # c < 0 votes where it lands
    assert flat.sum() == 2 and (h64[flat, 0].numpy() != 0).all() and (pix[flat, 0].numpy() == -1).all()
    # the block tells rintf from roundf, and x from y in the mask index: rounding half away from zero changes the votes
    away = np.sign(u) * np.floor(np.abs(u) + 0.5)
    assert (away[front] != np.rint(u[front])).sum() >= 8
    assert votes.sum() >= 8 and (votes == 0).sum() >= 8


def test_scan_reference_and_masks():
    for n in U.SCAN_SIZES:
        masks = U.scan_masks(n)
        assert set(masks) == {"zeros", "ones", "half", "sparse", "last", "byte1024", "values"}
        pos, cnt = U.ref_mask_scan(masks["values"])
        assert cnt == int((masks["values"] != 0).sum()) and (n == 0 or int(pos[-1]) == cnt - int(masks["values"][-1] != 0))
        assert U.ref_mask_scan(masks["ones"])[1] == n and U.ref_mask_scan(masks["last"])[1] == min(n, 1)
        assert U.ref_mask_scan(masks["byte1024"])[1] == (1 if n > 1024 else 0)
    v = U.scan_masks(5000)["values"]
    assert {2, 255} <= set(v.tolist())


def test_trainer_case_moves_rows_at_every_event_and_has_no_borderline_vote():
    case = U.densify_case()
    after, border = U.emulate_densify(case)
    n0 = case["state"]["means"].shape[0]
    n1, n2, n3 = (a["means"].shape[0] for a in after)
    assert n0 == 2500 and n1 == int((~case["cull_mask"]).sum()) < n0
    assert n2 == n1 + 2 * int(case["dup_mask"].sum()) > n1 and 0.3 * n2 < n3 < 0.95 * n2
    assert not border.any(), int(border.sum())      # no cull decision of the vote hinges on a borderline view
    assert all(len(a) == 13 for a in after)
    assert float(after[0]["opacities"].max()) <= 0.08 and float(case["state"]["opacities"].max()) > 0.08
    assert after[0]["m_means"].any() and after[0]["absgrads"].any() and not after[1]["absgrads"].any()
    record_cpu("densify_trainer_case", rows=[n0, n1, n2, n3], borderline_votes=int(border.sum()))
