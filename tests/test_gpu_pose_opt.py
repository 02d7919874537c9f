"""GPU: pose refinement end to end -- the projection's camera gradients driving `harness.camera_opt` through
`pipeline.render_view` (a known pose error is reduced), and the trainer with `camera_optimizer` on (it runs, records
the pose errors, checkpoints the seventh group; the settings it cannot serve are refused; "off" changes nothing)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def recover(mode, render_depth, steps=150, lr=2e-3, device=DEV, report=None):
    """One camera, 300 fixed Gaussians, a 64x48 image rendered from the true pose; the camera starts off by a small
    rigid error (a few pixels of image motion) and Adam runs on its six numbers.  -> (photometric loss, rotation
    error in degrees, translation error) at the start and at the end."""
    from harness import camera_opt as CO
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view

    true = S.make_camera(64, 48, yaw=0.1, pitch=-0.05, trans=(0.05, -0.02, 0.1))
    sc = S.make_scene(300, true, sh_degree=0, seed=11, scale_lo=0.08, scale_hi=0.35, z_lo=2.0, z_hi=7.0)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    means, scales, quats, opac, sh = (t(sc[k]) for k in ("means3d", "scales", "quats", "opacities", "sh_coeffs"))
    bg = t(np.array(S.BACKGROUND, np.float32))
    # the error: 0.03 rad (1.7 px at fx = 55 px) about a skew axis and 0.06 scene units (0.5 .. 1.6 px at z = 2 .. 7)
    ang, axis = 0.03, np.array([0.5, 0.8, 0.33]) / np.linalg.norm([0.5, 0.8, 0.33])
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    dR = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    V = true.viewmat.astype(np.float64).copy()
    V[:3, :3] = dR @ V[:3, :3]
    V[:3, 3] = dR @ V[:3, 3] + np.array([0.04, -0.03, 0.03])
    V = V.astype(np.float32)
    fovy = 2.0 * math.atan(true.height / (2.0 * true.fy))
    start = S.Camera(64, 48, true.fx, true.fy, true.cx, true.cy, V,
                     (S.projection_matrix(0.001, 1000.0, math.radians(60.0), fovy) @ V).astype(np.float32))

    def render(cam):
        return render_view(means, scales, quats, opac, sh, cam, bg, 0, render_depth=render_depth)

    with torch.no_grad():
        target = render(CameraTensors.from_numpy(true, device))
    posed = CO.PosedCameras([start], device, true_cams_np=[true])
    opt = CO.CameraOptimizer(mode, 1, device)
    adam = torch.optim.Adam([opt.pose_adjustment], lr=lr, eps=1e-15)
    like = CameraTensors.from_numpy(start, device)

    def losses():
        out = render(posed.camera(opt, 0, like))
        photo = (out["rgb"] - target["rgb"]).abs().mean()
        total = photo + (out["depth"] - target["depth"]).abs().mean() if render_depth else photo
        return photo, total

    first = (float(losses()[0].detach()),) + posed.pose_errors(opt)
    for _ in range(steps):
        adam.zero_grad(set_to_none=True)
        losses()[1].backward()
        adam.step()
    assert torch.isfinite(opt.pose_adjustment).all()
    last = (float(losses()[0].detach()),) + posed.pose_errors(opt)
    if report is not None:
        report(first, last)
    return first, last


@pytest.mark.parametrize("render_depth", [False, True])
@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_a_known_pose_error_is_reduced(mode, render_depth):
    first, last = recover(mode, render_depth)
    print(f"{mode} depth={render_depth}: photometric {first[0]:.5f} -> {last[0]:.5f}, rotation {first[1]:.4f} -> "
          f"{last[1]:.4f} deg, translation {first[2]:.5f} -> {last[2]:.5f}")
    assert first[1] > 1.0 and first[2] > 0.03  # the error that was put in: 0.03 rad = 1.72 degrees, |t| = 0.058
    assert last[0] < first[0] and last[1] < first[1] and last[2] < first[2]


SMALL = dict(num_gaussians=20_000, width=320, height=180, num_views=8, iters=60, sh_degree=3, sh_degree_interval=30)


def test_trainer_with_the_camera_optimizer(tmp_path):
    from harness import checkpoint as CK
    from harness.camera_opt import CameraOptimizer
    from harness.train import GaussianParams, TrainConfig, blob_scene, make_optimisers, train

    dev = torch.device("cuda", 0)
    cfg = TrainConfig(camera_optimizer="SO3xR3", pose_noise=(0.02, 0.005), checkpoint_dir=str(tmp_path), save_every=59,
                      **SMALL)
    res = train(cfg, dev)
    assert res["render"] == "separate ops" and np.isfinite(res["param_checksum"])
    adj = np.array(res["pose_adjustment"])
    assert adj.shape == (8, 6) and np.isfinite(adj).all() and np.abs(adj).max() > 0
    for k in ("pose_err_rot_deg_start", "pose_err_rot_deg_end", "pose_err_trans_start", "pose_err_trans_end",
              "camera_opt_translation", "camera_opt_rotation"):
        assert np.isfinite(res[k]), k
    assert 0.05 < res["pose_err_rot_deg_start"] < 1.5 and 0.005 < res["pose_err_trans_start"] < 0.1  # the noise
    assert res["camera_opt_translation"] > 0 and res["camera_opt_rotation"] > 0
    assert res["psnr_end"] > res["psnr_start"]

    # the checkpoint carries the parameter under the toolkit's key and its Adam state, and both come back
    path = CK.checkpoint_path(str(tmp_path), 59)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    key = "_model.camera_optimizer.pose_adjustment"
    assert saved["pipeline"][key].shape == (8, 6) and bool(saved["pipeline"][key].any())
    st = saved["optimizers"]["camera_opt"]["state"][0]
    assert float(st["step"]) == 60 and bool(st["exp_avg"].any()) and bool(st["exp_avg_sq"].any())
    # (the run went on for no step after saving: the record's adjustment is the saved one)
    assert np.array_equal(saved["pipeline"][key].numpy(), adj.astype(np.float32))
    model = GaussianParams(blob_scene(100, 0), dev)
    optims, _ = make_optimisers(cfg, model, dev, False)
    opt = CameraOptimizer("SO3xR3", 8, dev)
    adam = torch.optim.Adam([opt.pose_adjustment], lr=cfg.camera_lr, eps=1e-15)
    assert CK.load_checkpoint(path, model, optims, camera=(opt, adam)) == 60
    assert torch.equal(opt.pose_adjustment.detach().cpu(), saved["pipeline"][key])
    got = adam.state[opt.pose_adjustment]
    assert float(got["step"]) == 60 and got["exp_avg"].device.type == "cuda"
    assert torch.equal(got["exp_avg"].cpu(), st["exp_avg"]) and torch.equal(got["exp_avg_sq"].cpu(), st["exp_avg_sq"])
    # ... and the trainer resumes from it
    more = train(TrainConfig(camera_optimizer="SO3xR3", pose_noise=(0.02, 0.005), resume_from=path,
                             **{**SMALL, "iters": 70}), dev)
    assert more["start_step"] == 60 and more["iters"] == 10
    assert more["pose_err_trans_start"] == pytest.approx(res["pose_err_trans_end"], rel=1e-5)


def test_settings_the_camera_optimizer_cannot_serve_are_refused():
    from harness.train import TrainConfig, train

    dev = torch.device("cuda", 0)
    for kw, why in ((dict(fused_render=True), "fused_render"), (dict(use_graph=True), "use_graph")):
        with pytest.raises(ValueError, match=why):
            train(TrainConfig(camera_optimizer="SE3", **kw, **SMALL), dev)
    with pytest.raises(ValueError, match="one GPU"):
        train(TrainConfig(camera_optimizer="SE3", **SMALL), dev, rank=0, world=2)
    with pytest.raises(ValueError, match="CUDA"):
        train(TrainConfig(camera_optimizer="SE3", **SMALL), torch.device("cpu"))
    with pytest.raises(ValueError, match="camera_optimizer"):
        train(TrainConfig(camera_optimizer="so3", **SMALL), dev)


def test_off_changes_nothing():
    """With the compositing backward summing in a fixed order two runs are bit-identical
    (tests/test_gpu_train.py::test_deterministic_mode_makes_training_bitwise_reproducible): the default, and "off"
    spelled out with every camera setting moved off its default."""
    from harness.train import TrainConfig, train
    from rasterizer import rasterize as R

    dev = torch.device("cuda", 0)
    R.set_deterministic(True)
    try:
        a = train(TrainConfig(**SMALL), dev)
        b = train(TrainConfig(camera_optimizer="off", camera_lr=0.5, camera_trans_l2_penalty=3.0, **SMALL), dev)
    finally:
        R.set_deterministic(False)
    assert a["param_checksum"] == b["param_checksum"] and a["psnr_end"] == b["psnr_end"]
    assert "pose_err_rot_deg_start" not in a and "pose_adjustment" not in b
