"""GPU: `TrainConfig.mask` through the harness trainer -- the fused masked heads against the reference's torch
multiplies inside the same loop, a masked run that learns, and the co-gs depth head with a silhouette mask."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SMALL = dict(num_gaussians=5_000, width=160, height=96, num_views=4, eval_views=2, sh_degree=3, log_every=1)


def test_one_masked_step_fused_heads_equal_torch_multiplies():
    from harness.train import TrainConfig, train

    fused = train(TrainConfig(mask="box", iters=1, fused_loss=True, **SMALL), DEV)
    plain = train(TrainConfig(mask="box", iters=1, fused_loss=False, **SMALL), DEV)
    bare = train(TrainConfig(iters=1, fused_loss=True, **SMALL), DEV)
    print(fused["losses"], plain["losses"], bare["losses"])
    assert fused["mask"] == "box" and bare["mask"] == "none" and "psnr_masked_start" not in bare
    assert abs(fused["losses"][0] - plain["losses"][0]) < 1e-5
    assert fused["losses"][0] < 0.9 * bare["losses"][0]  # three quarters of both images are black
    assert np.isfinite(fused["psnr_masked_start"]) and np.isfinite(fused["psnr_masked_end"])


def test_short_masked_run_improves_psnr_inside_the_mask():
    """The configuration of test_gpu_train.test_short_training_run_improves_psnr, with and without the box mask: a
    quarter of the pixels supervise, and the PSNR over them gains at least half of what the whole image gains in the
    unmasked run (a sanity bound measured against that run, not a fixed number)."""
    from harness.train import TrainConfig, train

    kw = dict(num_gaussians=20_000, width=320, height=180, num_views=8, iters=120, sh_degree=3, sh_degree_interval=30,
              log_every=10)
    ref = train(TrainConfig(**kw), DEV)
    res = train(TrainConfig(mask="box", **kw), DEV)
    gain_ref = ref["psnr_end"] - ref["psnr_start"]
    gain = res["psnr_masked_end"] - res["psnr_masked_start"]
    print(f"unmasked gain {gain_ref:.2f} dB; masked run: {gain:.2f} dB inside the mask, "
          f"{res['psnr_end'] - res['psnr_start']:.2f} dB whole image; losses {res['losses'][0]:.5f} -> {res['losses'][-1]:.5f}")
    assert gain_ref > 3.0
    assert gain >= 0.5 * gain_ref, (gain, gain_ref)
    assert np.isfinite(res["losses"]).all() and res["losses"][-1] < res["losses"][0]
    assert np.isfinite(res["param_checksum"])


def test_cogs_silhouette_mask_fused_depth_head_equals_torch_ops():
    """co-gs with mask="alpha": the first loss that carries the depth term, with the fused masked depth head and with
    the reference's torch multiplies and `depth_l1`."""
    from harness.train import TrainConfig, train

    kw = dict(model="co-gs", mask="alpha", iters=4, depth_loss_start_iteration=0, scene_scale=(0.03, 0.15), **SMALL)
    a = train(TrainConfig(fused_depth=True, **kw), DEV)
    b = train(TrainConfig(fused_depth=False, **kw), DEV)
    print(a["losses"], b["losses"])
    assert a["mask"] == b["mask"] == "alpha"
    first = 1  # step > depth_loss_start_iteration
    assert a["losses"][first] > a["losses"][0]  # the depth term (non-negative, in scene units) joined
    assert abs(a["losses"][first] - b["losses"][first]) <= 1e-5 * abs(b["losses"][first])
    assert np.isfinite(a["psnr_masked_end"]) and np.isfinite(a["param_checksum"])


@pytest.mark.parametrize("graph", [False, True])
def test_masked_run_through_the_one_op_render_and_the_graph(graph):
    """The mask reaches the loss on the `render_gaussians` path and, as a second static target, inside a replayed HIP
    graph: same first loss as the separate ops to 1e-5 (same kernels behind both), and the run learns."""
    from harness.train import TrainConfig, train

    kw = dict(mask="box", iters=30, sh_degree_interval=10, **SMALL)
    ref = train(TrainConfig(**kw), DEV)
    res = train(TrainConfig(fused_render=True, use_graph=graph, **kw), DEV)
    print(ref["losses"][0], res["losses"][0], ref["psnr_masked_end"], res["psnr_masked_end"])
    assert res["render"] == ("hip graph per view" if graph else "one fused op")
    assert abs(res["losses"][0] - ref["losses"][0]) < 1e-5
    assert res["losses"][-1] < res["losses"][0]
    assert res["psnr_masked_end"] > res["psnr_masked_start"]
