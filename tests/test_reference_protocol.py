"""The reference's OWN model class driven through the operator surface this repo implements, replayed from a fixture.

tests/golden/make_golden.py (`--only-protocol`) ran the reference's `EdgeGaussianSplatting` with `gsplat.rasterization`
bound to the CPU ORACLE -- whose signature, returns and `info` contract are the same as the HIP drop-in's
(tests/test_gpu_parity.py checks the two against each other on the GPU) -- for forward -> compute_projection_loss ->
backward -> update_absgrads -> 4x Adam over three steps, then the densify path that consumes absgrads (edge_gs.py:197-324,
544-613; train_gaussians.py:81-106).  It recorded every input the class handed across the boundary and everything that
came back.  This test takes the same steps from those inputs with the oracle, the weight-map form of the losses and four
torch Adams, and must arrive where the reference's class arrived: the boundary protocol against the real caller."""
import json
import os

import numpy as np
import torch

from oracle import ref_torch as O


def test_reference_model_class_runs_a_training_step(golden_dir):
    d = np.load(os.path.join(golden_dir, "reference_protocol.npz"))
    kw = {k: v for k, v in json.load(open(os.path.join(golden_dir, "boundary_trace.json")))["kwargs"].items()
          if not isinstance(v, dict) and k not in ("width", "height")}  # (the call's scalar arguments)
    names = ["means", "scales", "quats", "opacities"]
    P = {k: torch.nn.Parameter(torch.from_numpy(d[f"init_{k}"].copy())) for k in names}
    opts = {k: torch.optim.Adam([P[k]], lr=float(d["adam_lr"][i]), betas=tuple(float(b) for b in d["adam_betas"][i]),
                                eps=float(d["adam_eps"][i])) for i, k in enumerate(names)}
    gt = torch.from_numpy(d["gt"])
    edge = torch.from_numpy(d["edge_masks"])
    N = P["means"].shape[0]
    H, W = gt.shape[1:]
    absgrads = torch.zeros(N)
    before = P["means"].detach().clone()
    for step, (idx, strategy) in enumerate(zip(d["steps_view"].tolist(), d["steps_strategy"].tolist())):
        render, alpha, info = O.rasterization(
            means=P["means"], quats=P["quats"], scales=torch.exp(P["scales"]), opacities=torch.sigmoid(P["opacities"]).squeeze(-1),
            colors=torch.ones(N, 3), viewmats=torch.from_numpy(d["viewmats"][step]), Ks=torch.from_numpy(d["Ks"][step]),
            width=W, height=H, **kw)
        assert render.shape == (1, H, W, 3) and alpha.shape == (1, H, W, 1)   # out["rgb"] / out["accumulation"]
        assert info["radii"].dtype == torch.int32 and info["means2d"].shape == (1, N, 2)
        assert str(info["radii"].dtype) == str(d["radii_dtype"]) and list(info["means2d"].shape) == d["xys_shape"].tolist()
        info["means2d"].retain_grad()
        sel = None
        if strategy == "bg_edge_ratio":  # the reference's own draw (CPU default RNG), unravelled as it does it
            s = torch.from_numpy(d["bg_draw_step2"]) % (H * W)
            sel = torch.zeros(H, W, dtype=torch.bool)
            sel[s // W, s % W] = True
        loss = O.edge_step_loss(render[0, ..., 0], gt[idx], O.loss_weight_map(strategy, edge[idx], sel))
        loss.backward()
        assert abs(float(loss) - float(d["losses"][step])) <= 1e-5 * abs(float(d["losses"][step])), (step, strategy)
        absgrads += info["means2d"].absgrad[0].norm(dim=-1)             # update_absgrads (edge_gs.py:607-613)
        for o in opts.values():
            o.step()
            o.zero_grad()
    assert int(d["model_step"]) == 3 and float(d["absgrads_normalize_factor"]) == 4
    assert float(absgrads.max()) > 0
    assert np.allclose(absgrads.numpy(), d["absgrads"], rtol=1e-5, atol=1e-9)
    for k in names:
        assert np.allclose(P[k].detach().numpy(), d[f"final_{k}"], rtol=1e-5, atol=1e-7), k
    assert float((P["means"].detach() - before).abs().max()) > 0
    # the densify event that consumes the accumulated absgrads ('absolute' threshold 0.5 on the min-max normalised mean,
    # dup_factor 3: two new copies of each selected Gaussian)
    g = absgrads / float(d["absgrads_normalize_factor"])
    dup = ((g - g.min()) / (g.max() - g.min())).numpy() > 0.5
    assert np.array_equal(dup, d["dup_mask"]) and dup.sum() > 0
    n0 = int(d["n_before_densify"])
    assert n0 == N and int(d["n_after_densify"]) == n0 + 2 * int(dup.sum()) == int(d["absgrads_len_after_densify"])
