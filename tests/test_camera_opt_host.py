"""CPU: harness/camera_opt.py -- the two exponential maps, the regulariser and the metrics against values the
reference's own lie_groups.py / camera_optimizers.py produced on the CPU (tests/golden/camera_opt_maps.npz, made by
tests/golden/make_golden_camera_opt.py); the chain c2w @ adj -> viewmat -> projmat against a float64 restatement;
the zero adjustment reproducing the uncorrected camera bit for bit.

The maps are the same float32 operations in another order: `torch.allclose` at rtol 1e-6 / atol 1e-7."""
import math
import os

import numpy as np
import pytest
import torch

from harness import camera_opt as CO
from harness import scene as S
from harness.pipeline import CameraTensors
from harness.train import orbit_cameras

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_opt_maps.npz")
RTOL, ATOL = 1e-6, 1e-7


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_the_inputs_cover_both_thresholds(golden):
    x = golden["tangent"]
    theta = np.linalg.norm(x[:, 3:].astype(np.float64), axis=1)
    assert not x[0].any()
    assert ((theta > 0) & (theta < 1e-2)).sum() >= 3 and (theta > 1e-2).sum() >= 3
    assert np.abs(theta - 1e-2).min() < 2e-7 and (theta > math.pi - 0.01).any() and len(x) >= 16


@pytest.mark.parametrize("mode,key", [("SO3xR3", "so3xr3"), ("SE3", "se3")])
def test_exponential_maps_match_the_reference(golden, mode, key):
    fn = CO.exp_map_SO3xR3 if mode == "SO3xR3" else CO.exp_map_SE3
    x = torch.from_numpy(golden["tangent"])
    want = torch.from_numpy(golden[key])
    got = fn(x)
    assert got.shape == want.shape == (len(x), 3, 4) and got.dtype == torch.float32
    print(f"{mode}: max |mine - reference| {float((got - want).abs().max()):.3e}")
    assert torch.allclose(got, want, rtol=RTOL, atol=ATOL)
    single = torch.cat([fn(x[i:i + 1]) for i in range(len(x))])
    assert torch.allclose(single, torch.from_numpy(golden[key + "_single"]), rtol=RTOL, atol=ATOL)
    # the zero tangent is the identity exactly, and the rotations are rotations
    assert torch.equal(got[0], torch.eye(4)[:3])
    R = got[:, :, :3].double()
    big = x[:, 3:].norm(dim=1) >= 1e-2  # (below its clamp SO3xR3 is the reference's approximation, not a rotation)
    assert (R[big] @ R[big].transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max() < 5e-6


def test_regulariser_and_metrics_match_the_reference(golden):
    for k in range(len(golden["regulariser"])):
        opt = CO.CameraOptimizer("SO3xR3", len(golden[f"reg_input_{k}"]), "cpu")
        with torch.no_grad():
            opt.pose_adjustment.copy_(torch.from_numpy(golden[f"reg_input_{k}"]))
        m = opt.metrics()
        for got, key in ((opt.regulariser(), "regulariser"), (m["camera_opt_translation"], "metric_translation"),
                         (m["camera_opt_rotation"], "metric_rotation")):
            assert torch.allclose(got.detach(), torch.tensor(golden[key][k]), rtol=RTOL, atol=ATOL), (k, key)
    opt = CO.CameraOptimizer("SE3", 3, "cpu")  # zero adjustment: zero loss, finite (zero) gradient
    opt.regulariser().backward()
    assert float(opt.regulariser().detach()) == 0.0 and torch.isfinite(opt.pose_adjustment.grad).all()
    assert CO.CameraOptimizer("off", 3, "cpu").metrics() == {} and not list(CO.CameraOptimizer("off", 3, "cpu").parameters())
    with pytest.raises(ValueError, match="camera_optimizer"):
        CO.CameraOptimizer("so3", 3, "cpu")


def _fp64_chain(c2w, tangent, mode, proj):
    """c2w @ exp(tangent), the y/z flip, the analytic inverse and proj @ viewmat, in float64 from the closed forms
    (Rodrigues; SE(3)'s left Jacobian for its translation) -- no clamp, no series."""
    c2w, x = np.asarray(c2w, np.float64), np.asarray(tangent, np.float64)
    v, w = x[:3], x[3:]
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if t > 0:
        R = np.eye(3) + math.sin(t) / t * K + (1 - math.cos(t)) / t ** 2 * (K @ K)
        Vl = np.eye(3) + (1 - math.cos(t)) / t ** 2 * K + (t - math.sin(t)) / t ** 3 * (K @ K)
    else:
        R, Vl = np.eye(3), np.eye(3)
    adj = np.eye(4)
    adj[:3, :3] = R
    adj[:3, 3] = v if mode == "SO3xR3" else Vl @ v
    c = np.concatenate([c2w, [[0, 0, 0, 1]]]) @ adj
    Rg = c[:3, :3] @ np.diag([1.0, -1.0, -1.0])
    V = np.eye(4)
    V[:3, :3] = Rg.T
    V[:3, 3] = -Rg.T @ c[:3, 3]
    return V, np.asarray(proj, np.float64) @ V, c[:3, 3]


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_corrected_camera_against_float64(mode):
    cams = orbit_cameras(5, 64, 48)
    posed = CO.PosedCameras(cams, "cpu")
    opt = CO.CameraOptimizer(mode, 5, "cpu")
    rng = np.random.default_rng(3)
    with torch.no_grad():  # angles well above both thresholds: the closed forms are what both compute there
        opt.pose_adjustment.copy_(torch.from_numpy(
            np.concatenate([rng.uniform(-0.3, 0.3, (5, 3)), rng.uniform(0.05, 0.2, (5, 3))], 1).astype(np.float32)))
    for v in range(5):
        like = CameraTensors.from_numpy(cams[v], "cpu")
        cam = posed.camera(opt, v, like)
        V, P, pos = _fp64_chain(posed.c2w[v].numpy(), opt.pose_adjustment[v].detach().numpy(), mode, posed.proj(like).numpy())
        # float32 round-off of a chain of three 3- or 4-term products of O(1) factors with entries up to |t| ~ 6.5
        for got, want in ((cam.viewmat, V), (cam.projmat, P), (cam.campos, pos)):
            assert got.dtype == torch.float32
            assert np.abs(got.detach().numpy() - want).max() <= 32 * 2.0 ** -24 * max(1.0, np.abs(want).max())
        assert cam.viewmat.requires_grad and cam.projmat.requires_grad and not cam.campos.requires_grad
        assert (cam.width, cam.height, cam.fx, cam.cy) == (like.width, like.height, like.fx, like.cy)
    # autograd reaches the six numbers of the one view that was used
    cam = posed.camera(opt, 2, CameraTensors.from_numpy(cams[2], "cpu"))
    (cam.viewmat.sum() + cam.projmat.sum()).backward()
    g = opt.pose_adjustment.grad
    assert g[2].abs().min() > 0 and not g[[0, 1, 3, 4]].any()


@pytest.mark.parametrize("mode", ["SO3xR3", "SE3"])
def test_zero_adjustment_reproduces_the_uncorrected_camera(mode):
    cams = orbit_cameras(7, 64, 48)
    posed = CO.PosedCameras(cams, "cpu")
    zero, off = CO.CameraOptimizer(mode, 7, "cpu"), CO.CameraOptimizer("off", 7, "cpu")
    for v in range(7):
        like = CameraTensors.from_numpy(cams[v], "cpu")
        a, b = posed.camera(zero, v, like), posed.camera(off, v, like)
        for x, y in ((a.viewmat, b.viewmat), (a.projmat, b.projmat), (a.campos, b.campos)):
            assert torch.equal(x.detach(), y)
        # ... which is the camera the trainer was given, to the round-off of going through its camera-to-world
        assert np.abs(b.viewmat.numpy() - cams[v].viewmat).max() <= 8 * 2.0 ** -24 * 6.5
        assert np.abs(b.projmat.numpy() - cams[v].projmat).max() <= 8 * 2.0 ** -24 * 6.5 * 2
    rot, trans = posed.pose_errors(zero)
    assert rot < 1e-4 and trans == 0.0  # (degrees: float32 round-off of R^T R)


def test_pose_noise_is_what_the_errors_measure():
    cams = orbit_cameras(6, 64, 48)
    noisy = CO.perturb_cameras(cams, 0.05, 0.02, seed=11)
    assert CO.perturb_cameras(cams, 0.0, 0.0, seed=11)[0] is cams[0]
    again = CO.perturb_cameras(cams, 0.05, 0.02, seed=11)
    assert all(np.array_equal(a.viewmat, b.viewmat) for a, b in zip(noisy, again))
    for c, n in zip(cams, noisy):
        R = n.viewmat[:3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and (n.fx, n.width) == (c.fx, c.width)
        fovy = 2.0 * math.atan(c.height / (2.0 * c.fy))
        want = S.projection_matrix(0.001, 1000.0, math.radians(60.0), fovy) @ n.viewmat
        assert np.abs(n.projmat - want).max() <= 1e-5 * np.abs(want).max()
    rot, trans = CO.PosedCameras(noisy, "cpu", true_cams_np=cams).pose_errors(None)
    assert 0.2 < rot < 3.0 and 0.02 < trans < 0.2  # sigma 0.02 rad = 1.1 degrees; 0.05 per axis
