"""GPU: training and evaluating from a dataset directory (`TrainConfig.dataset`).  The
directory is written once by tools/make_synthetic_dataset.py: 12 views of 64x48, RGBA, 16-bit depth, masks, a seed
cloud; the default split trains on 11 views and holds one out.

60 iterations with num_downscales = 1 (half size for 20 steps, then full size) of `gaussian-splatting` through the
separate ops, the one-node view and its HIP graph, and of `co-gs` through the separate ops (its depth loss joins after
step 30; the one-node view renders no depth and is refused for it, as without a dataset).  The loss is compared within
a stretch of one resolution and one set of terms: steps 0-7 against 12-19, and 31-38 (gaussian-splatting: 20-27)
against 52-59."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import target_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEV = torch.device("cuda", 0)
VIEWS, W, H = 12, 64, 48
COMMON = dict(iters=60, num_downscales=1, resolution_schedule=20, background_color="random", sh_degree=1,
              sh_degree_interval=20, log_every=1, depth_loss_start_iteration=30)
BODIES = {
    ("gaussian-splatting", "separate"): {},
    ("gaussian-splatting", "fused_render"): dict(fused_render=True),
    ("gaussian-splatting", "use_graph"): dict(fused_render=True, use_graph=True),
    ("co-gs", "separate"): dict(model="co-gs"),
}
RENDER = {"separate": "separate ops", "fused_render": "one fused op", "use_graph": "hip graph per view"}
_runs = {}


def _bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32).view(np.int32)


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    import make_synthetic_dataset as M

    out = str(tmp_path_factory.mktemp("dataset"))
    M.make_synthetic_dataset(out, VIEWS, W, H, alpha=True, device="cuda:0")
    return out


def _train(directory, key):
    """One 60-step run under set_deterministic(True), shared by the tests that look at it."""
    from harness.train import TrainConfig, train
    from rasterizer import rasterize as RZ

    if key not in _runs:
        RZ.set_deterministic(True)
        try:
            _runs[key] = train(TrainConfig(dataset=directory, **COMMON, **BODIES[key]), DEV)
        finally:
            RZ.set_deterministic(False)
    return _runs[key]


@pytest.mark.parametrize("key", list(BODIES), ids=["-".join(k) for k in BODIES])
def test_training_from_a_directory(directory, key):
    res = _train(directory, key)
    losses = res["losses"]
    assert res["render"] == RENDER[key[1]] and res["model"] == key[0] and len(losses) == 60
    assert all(np.isfinite(losses))
    late = 31 if key[0] == "co-gs" else 20
    stretches = [np.mean(losses[0:8]), np.mean(losses[12:20]), np.mean(losses[late:late + 8]), np.mean(losses[52:60])]
    print(key, "mean loss over steps 0-7, 12-19, %d-%d, 52-59:" % (late, late + 7), stretches,
          "psnr", res["psnr_start"], res["psnr_end"])
    assert stretches[1] < stretches[0] and stretches[3] < stretches[2]
    d = res["dataset"]
    assert d["num_train_views"] == 11 and (d["width"], d["height"], d["channels"]) == (W, H, 4)
    assert d["masks"] and d["depth"] and d["seed_points"] == 200
    # the cache holds the files' pixels in the files' integer widths: RGBA uint8, mask uint8, depth uint16
    assert d["cache_bytes"] == 11 * H * W * (4 * 1 + 1 + 2)
    assert res["num_gaussians_start"] == 200
    held = d["heldout"]
    assert held["num_images"] == 1 and held["split"] == "val" and np.isfinite(held["psnr"])
    assert res["psnr_masked_end"] is not None  # the dataset's masks reach the trainer's evaluation too


def test_cogs_through_the_one_node_view_is_refused_by_name(directory):
    from harness.train import TrainConfig, train

    with pytest.raises(ValueError, match="co-gs"):
        train(TrainConfig(dataset=directory, model="co-gs", fused_render=True, **COMMON), DEV)
    with pytest.raises(ValueError, match="dataset"):
        train(TrainConfig(dataset=directory, **COMMON), DEV, rank=0, world=2)


def test_graph_trains_the_same_steps_as_the_one_node_view(directory):
    a = _train(directory, ("gaussian-splatting", "fused_render"))
    b = _train(directory, ("gaussian-splatting", "use_graph"))
    worst = max(abs(x - y) for x, y in zip(a["losses"], b["losses"]))
    print("fused_render against use_graph: worst loss difference", worst)
    assert a["losses"] == b["losses"]
    assert a["param_checksum"] == b["param_checksum"]


def test_step_inputs_come_from_the_cache(directory):
    """The first step's target is `target_from_u8` of that view -- and the float32 restatement of the file's bytes --
    at the step's resolution over the step's background; mask and depth likewise; under use_graph the target is a
    DeferredTarget that writes the tensor it is given."""
    import harness.train as HT
    from gs_fused import DeferredTarget, target_from_u8
    from gs_io.dataset import load_dataset
    from harness.parallel import view_for_rank

    cfg = HT.TrainConfig(dataset=directory, **COMMON)
    data = HT.make_dataset_data(cfg, DEV)
    ds = load_dataset(directory, "train")
    assert data.cache.nbytes == 11 * H * W * 7 and len(data.cache) == len(ds) == 11
    inputs = HT.StepInputs(cfg, data, DEV)
    v, d = view_for_rank(0, 0, 1, len(ds)), HT.downscale_factor(0, cfg.num_downscales, cfg.resolution_schedule)
    assert d == 2
    bg, target, mask = inputs(v, d)
    assert bg.is_cuda and target.shape == (H // 2, W // 2, 3) and mask.shape == (H // 2, W // 2, 1)
    assert torch.equal(target, target_from_u8(data.cache.images[v], bg, (H // 2, W // 2)))
    assert np.array_equal(_bits(target), R.target_from_u8(ds.image(v), bg.cpu().numpy(), (H // 2, W // 2)).view(np.int32))
    assert np.array_equal(_bits(mask[..., 0]), R.plane_from_int(ds.mask(v), 1.0, (H // 2, W // 2)).view(np.int32))
    z = data.cache.depth(v, 2)
    assert np.array_equal(_bits(z), R.plane_from_int(ds.depth(v), 1e-3, (H // 2, W // 2)).view(np.int32))
    assert np.array_equal(_bits(data.gt_depth[v]), (ds.depth(v).astype(np.float32) * np.float32(1e-3)).view(np.int32))
    # evaluation's ground truth: full size over the fixed background
    assert np.array_equal(_bits(data.gt[v]), R.target_from_u8(ds.image(v), data.bg.cpu().numpy(), (H, W)).view(np.int32))
    # the graph's static target is written by the kernel itself
    ginputs = HT.StepInputs(HT.TrainConfig(dataset=directory, use_graph=True, fused_render=True, **COMMON), data, DEV)
    gbg, deferred, _ = ginputs(v, 1)
    assert isinstance(deferred, DeferredTarget) and tuple(deferred.shape) == (H, W, 3) and gbg is ginputs.bg_static
    static = torch.full((H, W, 3), -7.0, device=DEV)
    deferred.write(static)
    assert torch.equal(static, target_from_u8(data.cache.images[v], gbg, (H, W)))


def test_initial_model_is_the_seed_cloud(directory):
    import harness.train as HT
    from gs_fused import initial_log_scales
    from gs_io.dataset import load_dataset

    cfg = HT.TrainConfig(dataset=directory, sh_degree=2)
    ds = load_dataset(directory, "train")
    m = HT.dataset_initial_model(cfg, ds, DEV)
    g = m.gauss
    assert np.array_equal(g["means"].detach().cpu().numpy(), ds.points3D_xyz)
    rgb = ds.points3D_rgb.astype(np.float32) / np.float32(255)
    assert np.allclose(g["features_dc"].detach().cpu().numpy() * HT.SH_C0 + 0.5, rgb, atol=1e-6)  # RGB2SH
    assert g["features_rest"].shape == (200, 8, 3) and not bool(g["features_rest"].any())
    assert torch.equal(g["scales"], initial_log_scales(g["means"].detach(), 3, floor=1e-7))
    assert np.allclose(g["quats"].detach().norm(dim=-1).cpu().numpy(), 1.0, atol=1e-6)
    assert np.allclose(g["opacities"].detach().cpu().numpy(), np.log(0.1 / 0.9), atol=1e-7)
    r = HT.dataset_initial_model(HT.TrainConfig(dataset=directory, dataset_random_init=True, dataset_num_random=300,
                                                dataset_random_scale=4.0), ds, DEV)
    means = r.gauss["means"].detach()
    assert means.shape == (300, 3) and float(means.abs().max()) <= 2.0 and float(means.abs().max()) > 1.5
    dc = r.gauss["features_dc"].detach()
    assert float(dc.min()) >= 0.0 and float(dc.max()) <= 1.0


def test_pose_optimiser_runs_on_a_dataset(directory):
    from harness.train import TrainConfig, train

    res = train(TrainConfig(dataset=directory, camera_optimizer="SO3xR3", dataset_eval_split=None,
                            **dict(COMMON, iters=12)), DEV)
    assert len(res["losses"]) == 12 and all(np.isfinite(res["losses"]))
    adj = np.array(res["pose_adjustment"])
    assert adj.shape == (11, 6) and np.abs(adj).max() > 0  # the seventh group moved
    assert res["dataset"]["heldout"] is None


def test_evaluate_dataset_and_the_eval_tool(directory, tmp_path):
    import eval_dataset as E

    import harness.train as HT
    from gs_io.dataset import load_dataset
    from harness.checkpoint import latest_checkpoint
    from harness.pipeline import CameraTensors

    ckpt = str(tmp_path / "ckpt")
    HT.train(HT.TrainConfig(dataset=directory, checkpoint_dir=ckpt, save_every=9, dataset_eval_split=None,
                            **dict(COMMON, iters=10)), DEV)
    assert os.path.basename(latest_checkpoint(ckpt)).startswith("step-")
    out = str(tmp_path / "eval" / "output.json")
    info = E.main([directory, ckpt, "--output", out])
    with open(out) as f:
        written = json.load(f)
    assert list(written) == ["experiment_name", "method_name", "checkpoint", "results"] and written == info
    r = written["results"]
    for k in ("psnr", "psnr_std", "ssim", "ssim_std", "fps", "fps_std", "num_rays_per_sec", "num_rays_per_sec_std",
              "psnr_per_image", "ssim_per_image"):
        assert k in r, k
    assert r["num_images"] == 1 and r["ssim_std"] == 0.0 and r["psnr_std"] == 0.0 and r["lpips"] is None
    assert 0.0 < r["ssim"] <= 1.0 and r["fps"] > 0
    # the same numbers from the pieces: the model of that checkpoint, the held-out view, harness.train.psnr
    from export_gaussians import checkpoint_parameters

    model = HT.GaussianParams({k: v.numpy() for k, v in checkpoint_parameters(latest_checkpoint(ckpt)).items()}, DEV)
    cfg = HT.TrainConfig(dataset=directory, sh_degree=1)
    val = load_dataset(directory, "val")
    cache = HT.upload_dataset(val, DEV)
    direct = HT.evaluate_dataset(model, (val, cache), cfg, "val")
    bg = torch.tensor(HT.S.BACKGROUND, device=DEV)
    with torch.no_grad():
        rgb = model.render(CameraTensors.from_numpy(val.cameras[0], DEV), bg, 1)["rgb"]
    want = HT.psnr(rgb, cache.target(0, 1, bg))
    print("psnr: tool", r["psnr"], "evaluate_dataset", direct["psnr"], "harness.train.psnr", want)
    # 10 log10(1 / mse) against -10 log10(mse), both float32: a rounding of the quotient and of the logarithm,
    # 2 * 2^-24 relative on ~20 dB, and the render's forward is the same kernel sequence on the same inputs
    assert abs(direct["psnr"] - want) <= 1e-4 and abs(r["psnr"] - want) <= 1e-4
    many = HT.evaluate_dataset(model, directory, HT.TrainConfig(dataset=directory, sh_degree=1, dataset_eval_mode="interval",
                                                                dataset_eval_interval=4), "val")
    assert many["num_images"] == 3 and len(many["psnr_per_image"]) == 3
    t = torch.tensor(many["psnr_per_image"], dtype=torch.float64)
    std, mean = torch.std_mean(t)
    assert many["psnr"] == pytest.approx(float(mean)) and many["psnr_std"] == pytest.approx(float(std))
