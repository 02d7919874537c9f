"""Host: `TrainConfig(dataset=...)` on the CPU stand-ins of the native ops (tests/cpu_standins.py).  The two target
kernels have no CPU path either; they are stood in for twice -- by the float32 restatement of tests/target_reference.py
and by the torch path the trainer has used so far (`downscale_image` / `downscale_depth` / `composite_with_background`
fed `u8.float() / 255`) -- and the same step is run on both.  The targets are the only place the two runs differ:

  * the image target and the resized mask differ by at most tol = 2^-21 + max(H,W) * 2^-22 per element
    (tests/test_target_host.py), the depth target by tol times the largest depth zmax.  co-gs' loss is
    (1 - lambda) * mean|target * m - pred * m| plus, with the depth term on, mean|gt_depth * m - depth * m| over the
    measured pixels (both non-negative, both below ZFAR = 8: the cameras orbit at 6 +- 0.6 around a scene of radius
    1.5) -- means of absolute differences, so a change dt of the target and dm of the mask moves a term by at most
    dt + dm * max|target - pred|: the first step's loss moves by at most (1 - lambda) * 2 tol + tol * zmax + tol * ZFAR;
  * `psnr_start` = -10 log10(mse): |d mse| <= 2 * tol (errors are at most 1), so it moves by at most
    10 / ln(10) * 2 * tol / mse.
Later steps are not compared: Adam's update is lr * g / (|g| + 1e-15), so a gradient element near zero whose sign
differs between the runs moves a parameter by 2 lr whatever the size of the difference."""
import math
import os
import sys

import pytest
import torch

import target_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
VIEWS, W, H = 12, 48, 32
ZFAR = 8.0


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    import make_synthetic_dataset as M

    out = str(tmp_path_factory.mktemp("dataset"))
    restore = M.use_cpu_standins()
    try:
        M.make_synthetic_dataset(out, VIEWS, W, H, alpha=True, device="cpu")
    finally:
        restore()
    return out


def _standins(monkeypatch, targets: str):
    import cpu_standins as SI
    import gs_fused.target as T
    import harness.pipeline as HP
    import harness.train as HT

    monkeypatch.setattr(HP, "project_gaussians", SI.project_gaussians)
    monkeypatch.setattr(HP, "spherical_harmonics", SI.spherical_harmonics)
    monkeypatch.setattr(HP, "rasterize_gaussians", SI.rasterize_gaussians)
    calls = {"target": 0, "plane": 0}

    def put(value, out):
        value = value.contiguous()
        return value if out is None else out.copy_(value)

    if targets == "restatement":
        def target_from_u8(image_u8, background, out_hw, out=None):
            calls["target"] += 1
            bg = None if background is None else background.numpy()
            return put(torch.from_numpy(R.target_from_u8(image_u8.numpy(), bg, tuple(out_hw))), out)

        def plane_from_int(plane, unit, out_hw, out=None):
            calls["plane"] += 1
            return put(torch.from_numpy(R.plane_from_int(plane.numpy(), unit, tuple(out_hw))), out)
    else:
        def factor(shape, out_hw):
            d = shape[0] // out_hw[0]
            assert (shape[0] // d, shape[1] // d) == tuple(out_hw)
            return d

        def target_from_u8(image_u8, background, out_hw, out=None):
            calls["target"] += 1
            small = HT.downscale_image(image_u8.float() / 255.0, factor(image_u8.shape, out_hw))
            return put(HT.composite_with_background(small, background), out)

        def plane_from_int(plane, unit, out_hw, out=None):
            calls["plane"] += 1
            v = plane.to(torch.float32) * torch.tensor(unit, dtype=torch.float32)
            return put(HT.downscale_depth(v, factor(plane.shape, out_hw)), out)

    monkeypatch.setattr(T, "target_from_u8", target_from_u8)
    monkeypatch.setattr(T, "plane_from_int", plane_from_int)
    return calls


def _run(directory, monkeypatch, targets, **kw):
    import harness.train as HT

    calls = _standins(monkeypatch, targets)
    cfg = HT.TrainConfig(dataset=directory, model="co-gs", iters=1, num_downscales=1, resolution_schedule=20,
                         background_color="random", sh_degree=1, log_every=1, depth_loss_start_iteration=-1,
                         eval_views=2, **kw)
    return HT.train(cfg, torch.device("cpu")), calls


def test_dataset_step_matches_the_torch_path_within_the_target_tolerance(directory, monkeypatch):
    pytest.importorskip("sklearn")  # (the CPU start's neighbour search, as `seed_model(knn="sklearn")`)
    from gs_io.dataset import load_dataset

    a, calls = _run(directory, monkeypatch, "restatement")
    b, _ = _run(directory, monkeypatch, "torch")
    assert calls["target"] > 0 and calls["plane"] > 0  # targets, masks and depth all came through the cache
    ds = load_dataset(directory, "train")
    zmax = max(float(ds.depth(i).max()) for i in range(len(ds))) * 1e-3
    tol = 2.0 ** -21 + max(H, W) * 2.0 ** -22
    assert zmax < ZFAR
    bound = (1 - 0.2) * 2 * tol + tol * zmax + tol * ZFAR
    diff = abs(a["losses"][0] - b["losses"][0])
    print(f"first loss {a['losses'][0]!r} / {b['losses'][0]!r}: difference {diff:.3e}, bound {bound:.3e}")
    assert len(a["losses"]) == 1 and diff <= bound
    mse = 10.0 ** (-max(a["psnr_start"], b["psnr_start"]) / 10.0)
    assert abs(a["psnr_start"] - b["psnr_start"]) <= 10.0 / math.log(10.0) * 2 * tol / mse
    d = a["dataset"]
    assert d["num_train_views"] == 11 and d["cache_bytes"] == 11 * H * W * 7 and d["heldout"] is None
    assert a["num_gaussians_start"] == 200 and a["model"] == "co-gs"


def test_dataset_refusals_before_anything_is_read(directory):
    import harness.train as HT

    with pytest.raises(ValueError, match="dataset"):
        HT.train(HT.TrainConfig(dataset=directory), torch.device("cpu"), rank=0, world=2)
    with pytest.raises(ValueError, match="orientation_method"):
        HT.train(HT.TrainConfig(dataset=directory, dataset_orientation_method="pca"), torch.device("cpu"))
