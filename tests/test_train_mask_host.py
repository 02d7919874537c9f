"""CPU: `TrainConfig.mask` of the harness trainer on the oracle-backed stand-ins of the native ops
(tests/cpu_standins.py): what the masks are, how they follow the resolution schedule, and that the loop multiplies
them into both images as the models do (vanilla_gs.py:915-924, surface_gs.py:917-925)."""
import numpy as np
import pytest
import torch



@pytest.fixture()
def standins(monkeypatch):
    import cpu_standins as SI
    import harness.pipeline as HP
    import harness.train as HT
    from oracle import oracle as O

    O.set_threads(4)
    monkeypatch.setattr(HP, "project_gaussians", SI.project_gaussians)
    monkeypatch.setattr(HP, "spherical_harmonics", SI.spherical_harmonics)
    monkeypatch.setattr(HP, "rasterize_gaussians", SI.rasterize_gaussians)
    return HT


def test_box_and_alpha_masks():
    import harness.train as HT

    (m,) = HT.view_masks("box", 10, 18, [None], "cpu")
    assert m.shape == (10, 18, 1) and m.dtype == torch.float32
    want = np.zeros((10, 18), np.float32)
    want[2:7, 4:13] = 1.0  # rows H//4 .. 3H//4 - 1, columns W//4 .. 3W//4 - 1
    assert np.array_equal(m[..., 0].numpy(), want)
    a = torch.tensor([[0.2, 0.5], [0.50001, 1.0]])[..., None]
    (s,) = HT.view_masks("alpha", 2, 2, [a], "cpu")
    assert s.shape == (2, 2, 1) and s[..., 0].tolist() == [[0.0, 0.0], [1.0, 1.0]]
    with pytest.raises(ValueError):
        HT.view_masks("circle", 4, 4, [None], "cpu")


def test_downscaled_mask_is_the_images_resize_and_fractional():
    import harness.train as HT

    (m,) = HT.view_masks("box", 20, 36, [None], "cpu")
    assert HT.downscale_mask(m, 1) is m
    small = HT.downscale_mask(m, 2)
    assert small.shape == (10, 18, 1)
    assert torch.equal(small, HT.downscale_image(m.expand(20, 36, 3), 2)[..., :1])
    vals = set(np.unique(small.numpy()).tolist())
    assert {0.0, 1.0} < vals and vals <= {0.0, 0.25, 0.5, 1.0}  # the box's edges fall inside 2x2 cells: fractions


def test_masked_loop_multiplies_the_mask_into_both_images(standins):
    HT = standins
    kw = dict(num_gaussians=300, width=48, height=32, num_views=2, eval_views=2, iters=3, sh_degree=1, log_every=1,
              scene_scale=(0.03, 0.15))
    seen = []
    real = HT.ssim

    def spy(a, b):
        seen.append((a.detach().clone(), b.detach().clone()))
        return real(a, b)

    HT.ssim = spy
    try:
        res = HT.train(HT.TrainConfig(mask="box", **kw), torch.device("cpu"))
    finally:
        HT.ssim = real
    assert res["mask"] == "box" and len(seen) == 3
    (box,) = HT.view_masks("box", 32, 48, [None], "cpu")
    out = (box[..., 0] == 0)
    for pred, target in seen:
        assert float(pred[out].abs().max()) == 0.0 and float(target[out].abs().max()) == 0.0
        assert float(target[~out].abs().max()) > 0.0
    assert np.isfinite(res["psnr_masked_start"]) and np.isfinite(res["psnr_masked_end"])
    assert np.isfinite(res["losses"]).all()
    bare = HT.train(HT.TrainConfig(**kw), torch.device("cpu"))
    assert bare["mask"] == "none" and "psnr_masked_end" not in bare
    assert res["losses"][0] < bare["losses"][0]
    with pytest.raises(ValueError, match="mask"):
        HT.train(HT.TrainConfig(mask="circle", **kw), torch.device("cpu"))


def test_masked_cogs_loop_runs_on_the_stand_ins(standins):
    HT = standins
    cfg = HT.TrainConfig(model="co-gs", mask="alpha", num_gaussians=300, width=48, height=32, num_views=2, eval_views=2,
                         iters=4, sh_degree=1, log_every=1, scene_scale=(0.03, 0.15), depth_loss_start_iteration=1)
    res = HT.train(cfg, torch.device("cpu"))
    assert res["mask"] == "alpha" and np.isfinite(res["losses"]).all()
    assert res["losses"][2] > res["losses"][1]  # the masked depth term joined at step 2
    assert np.isfinite(res["psnr_masked_end"])
