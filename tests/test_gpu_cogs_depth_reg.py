"""GPU: `use_depth_regularization` of the co-gs model through the harness -- `optional_depth_terms` returns the term
computed from the device Canny mask, equal to the float64 restatement fed the oracle's mask, and the co-gs loop of
`harness.train` runs with the switch on."""
import numpy as np
import pytest
import torch

import canny_reference as CR
import depth_reg_reference as D
from test_gpu_depth_reg import TOL_LOSS, TOL_GRAD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Cfg:
    use_pearson_depth = False
    local_patch_size = 16
    depth_loss_stop_iteration = 100
    use_scaled_est_depth = False
    use_depth_regularization = True
    using_tv_loss = False


@pytest.mark.parametrize("trailing_one", [False, True])
def test_optional_depth_terms_returns_the_term_on_cuda_tensors(trailing_one):
    from harness import cogs_losses as CL

    H, W = 48, 64
    img = CR.smooth_random(H, W, 3)
    rng = np.random.default_rng(4)
    pred = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    pred[rng.uniform(size=(H, W)) < 0.1] = 0.0
    gt = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    mask = CR.image2canny(img, 50, 150, isEdge1=False)
    assert 0.5 < mask.mean() < 1.0
    loss64, grad64 = D.depth_reg(pred, mask)
    p = torch.from_numpy(pred[..., None] if trailing_one else pred).to(DEV).requires_grad_(True)
    terms = CL.optional_depth_terms(_Cfg, 50, p, torch.from_numpy(gt).to(DEV), torch.from_numpy(img).to(DEV))
    assert set(terms) == {"depth_reg_loss"}
    terms["depth_reg_loss"].backward()
    assert abs(float(terms["depth_reg_loss"]) - loss64) <= TOL_LOSS * loss64
    grad = p.grad.cpu().numpy().reshape(H, W)
    assert np.abs(grad - grad64).max() <= TOL_GRAD * np.abs(grad64).max()

    class All(_Cfg):
        use_scaled_est_depth = True
        using_tv_loss = True

    names = list(CL.optional_depth_terms(All, 50, p, torch.from_numpy(gt).to(DEV), torch.from_numpy(img).to(DEV),
                                         mono_scale_shift=(1.0, 0.0)))
    assert names == ["log_depth", "depth_reg_loss", "tv_loss"]   # the order of depth_gs.py:492-531


def test_cogs_loop_trains_with_the_switch_on():
    import harness.train as HT

    seen = []
    real = HT.cogs_losses.optional_depth_terms

    def terms(cfg, step, *a, **k):
        out = real(cfg, step, *a, **k)
        seen.append((step, {n: float(v) for n, v in out.items()}))
        return out

    HT.cogs_losses.optional_depth_terms = terms
    try:
        cfg = HT.TrainConfig(model="co-gs", num_gaussians=2000, width=96, height=64, num_views=4, iters=20, sh_degree=1,
                             sh_degree_interval=10, eval_views=2, depth_loss_start_iteration=4,
                             background_color="random", densify=False, use_est_depth=True, use_scaled_est_depth=True,
                             use_depth_regularization=True, using_tv_loss=True, log_every=1)
        res = HT.train(cfg, torch.device("cuda", 0))
    finally:
        HT.cogs_losses.optional_depth_terms = real
    assert [s for s, _ in seen] == list(range(5, 20))
    for _, t in seen:
        assert set(t) == {"log_depth", "depth_reg_loss", "tv_loss"}
        assert all(np.isfinite(v) for v in t.values()) and t["depth_reg_loss"] >= 0.0
    assert any(t["depth_reg_loss"] > 0 for _, t in seen)
    assert np.isfinite(res["param_checksum"]) and all(np.isfinite(v) for v in res["losses"])
