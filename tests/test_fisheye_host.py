"""CPU: the float64 restatement of the equidistant fisheye projection (tests/fisheye_reference.py) against itself --
its VJP against central differences of its forward, its Jacobian against autograd of the centre rule, its on-axis rows
against the pinhole reference -- and everything of the feature that needs no GPU: the dataset loader's flag, the
refusals of the trainer, `render_view` and `fuse_views`, and the op's refusal of CPU tensors."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gs_fused import project_gaussians_fisheye  # noqa: E402,F401  (the feature: without it nothing here has a subject)
from rasterizer.cuda._prototypes import PROTOTYPES  # noqa: E402

assert "gsr_project_forward_fisheye" in PROTOTYPES and "gsr_project_backward_fisheye" in PROTOTYPES

import fisheye_cases as FC  # noqa: E402
import fisheye_reference as FR  # noqa: E402
import projection_cases as PC  # noqa: E402
import projection_reference as PR  # noqa: E402


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_the_cases_meet_the_forward_tests_conditions():
    """What tests/test_gpu_fisheye.py asserts of the reference alone: at most 1 % of the rows flagged (the tz == clip
    rows of `exact` apart: flagged by construction), at least 30 % visible, no NaN anywhere, in float64 and float32."""
    for name in FC.names():
        c, groups = FC.case(name)
        kw = {"cov3d": c.cov3d} if c.precomputed else {}
        for dtype in (np.float64, np.float32):
            r = FR.project_forward_fisheye_fp64(*FC.reference_args(c), dtype=dtype, **kw)
            for k in FR.OUTPUTS:
                assert r[k].dtype == dtype and np.isfinite(r[k]).all(), (name, k)
        r = FR.project_forward_fisheye_fp64(*FC.reference_args(c), **kw)
        flagged = r["ambiguous"].copy()
        if "tz_is_clip" in groups:
            assert not r["visible"][groups["tz_is_clip"]].any()
            flagged[groups["tz_is_clip"]] = False
        assert flagged.mean() <= 0.01 and r["visible"].mean() >= 0.30, (name, flagged.mean(), r["visible"].mean())
        for g in ("on_axis", "near_axis_1e-20", "edge", "needles"):
            if g in groups:
                assert r["visible"][groups[g]].mean() >= 0.9, (name, g)
        if "behind" in groups:
            assert not r["visible"][groups["behind"]].any()
        if "near_plane" in groups:
            assert 0.2 <= r["visible"][groups["near_plane"]].mean() <= 0.8


def test_jacobian_equals_autograd_of_the_centre_rule():
    c, _ = FC.case("main")
    r = FR.project_forward_fisheye_fp64(*FC.reference_args(c))
    vm = c.viewmat[:3].astype(np.float64)
    t = c.means3d.astype(np.float64) @ vm[:, :3].T + vm[:, 3]
    rows = (t[:, 2] > c.clip) & (np.hypot(t[:, 0], t[:, 1]) / t[:, 2] > 1e-3)
    assert rows.sum() > 800
    Ja = FR.centre_jacobian_autograd_fp64(t[rows], PR._f32(c.fx), PR._f32(c.fy))
    e = np.abs(Ja - r["jacobian"][rows]).max(axis=(1, 2)) / np.abs(Ja).max(axis=(1, 2))
    assert e.max() < 1e-12, e.max()


def test_vjp_against_central_differences():
    c, groups = FC.case("main")
    sel = np.arange(c.n)[groups["generic"]][:200]
    means, scales, quats = (a[sel].astype(np.float64) for a in (c.means3d, c.scales, c.quats))
    quats /= np.linalg.norm(quats, axis=1, keepdims=True)
    cam = (c.viewmat[:3], c.projmat, c.fx, c.fy, c.cx, c.cy, c.H, c.W)
    rng = np.random.default_rng(9)
    cot = [rng.standard_normal(s) for s in ((200, 2), (200,), (200, 3), (200,))]

    def outputs(m, s, q):
        r = FR.project_forward_fisheye_fp64(m, s, c.glob_scale, q, *cam, c.bw, c.clip)
        return r, [r["xys"], r["depths"], r["conics"], r["compensation"]]

    r0, _ = outputs(means, scales, quats)
    vis = r0["visible"]
    assert vis.sum() >= 150

    def loss_rows(m, s, q):  # per row: rows are independent, one evaluation perturbs all of them at once
        _, outs = outputs(m, s, q)
        return sum((o * v).reshape(200, -1).sum(axis=1) for o, v in zip(outs, cot))

    g = FR.project_vjp_fisheye_fp64(means, scales, c.glob_scale, quats, *cam, r0["compensation"], *cot,
                                    clip_thresh=c.clip)
    # the VJP scales the compensation's cotangent by 0.5 / (compensation + 1e-6): d(comp) but for the 1e-6
    g_q = g[2] - quats * (g[2] * quats).sum(axis=1, keepdims=True)  # central differences see the normalisation
    for nm, x, gx in (("means", means, g[0]), ("scales", scales, g[1]), ("quats", quats, g_q)):
        fd = np.zeros_like(x)
        for k in range(x.shape[1]):
            h = 1e-6 * np.maximum(np.abs(x[:, k]), 1e-2)
            hi, lo = x.copy(), x.copy()
            hi[:, k] += h
            lo[:, k] -= h
            a = [means, scales, quats]
            i = ("means", "scales", "quats").index(nm)
            fd[:, k] = (loss_rows(*(a[:i] + [hi] + a[i + 1:])) - loss_rows(*(a[:i] + [lo] + a[i + 1:]))) / (2 * h)
        e = np.abs(fd - gx).max(axis=1) / np.maximum(np.abs(fd).max(axis=1), 1e-6 * np.abs(fd[vis]).max())
        print(f"{nm}: worst per-row difference from central differences {e[vis].max():.3e}")
        assert e[vis].max() < 1e-4, (nm, e[vis].max())


def test_on_axis_rows_equal_the_pinhole_reference():
    c, groups = FC.case("exact")
    s = groups["on_axis"]
    a = FR.project_forward_fisheye_fp64(*FC.reference_args(c))
    b = PR.project_forward_fp64(*FC.reference_args(c))
    vm = c.viewmat[:3].astype(np.float64)
    t = c.means3d.astype(np.float64) @ vm[:, :3].T + vm[:, 3]
    assert not t[s, :2].any() and a["visible"][s].all()
    for k in FR.OUTPUTS + ("radius",):
        assert np.allclose(a[k][s], b[k][s], rtol=1e-13, atol=1e-13), k
    for k in ("radii", "num_tiles_hit", "tile_min", "tile_max", "visible"):
        assert np.array_equal(a[k][s], b[k][s]), k
    # ... and off the axis the two cameras part: the outermost rows of the main case
    c, groups = FC.case("main")
    a = FR.project_forward_fisheye_fp64(*FC.reference_args(c))
    b = PR.project_forward_fp64(*FC.reference_args(c))
    g = groups["near_axis_0.1785"]
    assert (np.abs(a["xys"][g] - b["xys"][g]).max(axis=1) > 1e-2).all()


def test_prototypes_hold_the_new_entries():
    assert PROTOTYPES["gsr_project_forward_fisheye"] == PROTOTYPES["gsr_project_forward_aa"]  # the _aa entries' parameters
    assert PROTOTYPES["gsr_project_backward_fisheye"] == PROTOTYPES["gsr_project_backward_aa"]


# ---- the loader ---------------------------------------------------------------------------------------------------------
def _fisheye_standin(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
                     block_width, opacities=None, clip_thresh=0.01):
    """gs_fused.project_gaussians_fisheye for CPU tensors without gradients: the float64 reference, rounded."""
    npy = lambda t: t.detach().cpu().numpy()  # noqa: E731
    r = FR.project_forward_fisheye_fp64(npy(means3d), npy(scales), glob_scale, npy(quats), npy(viewmat), None, fx, fy,
                                        cx, cy, img_height, img_width, block_width, clip_thresh)
    f = lambda k: torch.from_numpy(r[k].astype(np.float32))  # noqa: E731
    i = lambda k: torch.from_numpy(r[k].astype(np.int32))  # noqa: E731
    out = (f("xys"), f("depths"), i("radii"), f("conics"), f("compensation"), i("num_tiles_hit"), f("cov3d"))
    return out if opacities is None else out + (opacities * out[4].reshape(-1, *([1] * (opacities.dim() - 1))),)


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    import make_synthetic_dataset as M

    import gs_fused.fisheye as GF

    out = str(tmp_path_factory.mktemp("fisheye_dataset"))
    restore = M.use_cpu_standins()
    saved = GF.project_gaussians_fisheye
    GF.project_gaussians_fisheye = _fisheye_standin
    try:
        meta = M.make_synthetic_dataset(out, 6, 48, 32, alpha=True, device="cpu", camera_model="OPENCV_FISHEYE")
    finally:
        GF.project_gaussians_fisheye = saved
        restore()
    return out, meta


def _variant(made, name, edit):
    out, meta = made
    meta = copy.deepcopy(meta)
    edit(meta)
    path = os.path.join(out, f"{name}.json")
    with open(path, "w") as f:
        json.dump(meta, f)
    return path


def test_loader_reads_a_fisheye_dataset_only_with_the_flag(made):
    from PIL import Image

    import harness.train as HT
    from gs_io.dataset import load_dataset

    out, meta = made
    assert meta["camera_model"] == "OPENCV_FISHEYE" and all(meta[k] == 0.0 for k in ("k1", "k2", "k3", "k4"))
    with pytest.raises(ValueError, match="camera_model"):
        load_dataset(out, "train")
    with pytest.raises(ValueError, match="allow_fisheye"):
        load_dataset(out, "train")
    ds = load_dataset(out, "train", allow_fisheye=True)
    assert ds.camera_model == "fisheye" and len(ds) == 6 and all(cam.model == "fisheye" for cam in ds.cameras)
    want = HT.orbit_cameras(6, 48, 32, fov_x_deg=HT.FISHEYE_FOV_X_DEG, model="fisheye")[0]
    assert abs(ds.cameras[0].fx - want.fx) < 1e-5 and abs(want.fx * np.radians(HT.FISHEYE_FOV_X_DEG) - 48) < 1e-9
    # the images are fisheye images: the object is drawn, and smaller than the pinhole camera of 60 degrees draws it
    alpha = np.array(Image.open(ds.image_filenames[0]))[..., 3]
    assert 0 < (alpha > 127).mean() < 0.5
    # a pinhole dataset stays a pinhole dataset under the flag
    pin = _variant(made, "pinhole", lambda m: m.update(camera_model="PINHOLE"))
    assert load_dataset(pin, "train", allow_fisheye=True).camera_model == "pinhole"
    assert load_dataset(pin, "train").camera_model == "pinhole"
    # the ideal lens only
    k1 = _variant(made, "k1", lambda m: m.update(k1=0.01))
    with pytest.raises(ValueError, match="k1"):
        load_dataset(k1, "train", allow_fisheye=True)
    crop = _variant(made, "crop_radius", lambda m: m.update(fisheye_crop_radius=20.0))
    for kw in ({}, {"allow_fisheye": True}):
        with pytest.raises(ValueError, match="fisheye_crop_radius" if kw else "camera_model|fisheye_crop_radius"):
            load_dataset(crop, "train", **kw)
    with pytest.raises(ValueError, match="camera_model"):
        load_dataset(_variant(made, "equirect", lambda m: m.update(camera_model="EQUIRECTANGULAR")), "train",
                     allow_fisheye=True)


def test_trainer_takes_the_model_from_the_dataset_config():
    import harness.train as HT

    assert HT.dataset_config(HT.TrainConfig()).get("allow_fisheye") is None  # the default call is the parent's
    assert HT.dataset_config(HT.TrainConfig(dataset_allow_fisheye=True))["allow_fisheye"] is True
    cam = HT.orbit_cameras(2, 64, 48, model="fisheye", fov_x_deg=150.0)[1]
    half = HT.rescale_camera(cam, 2)
    assert half.model == "fisheye" and half.fx == cam.fx / 2 and (half.width, half.height) == (32, 24)
    assert HT.rescale_camera(HT.orbit_cameras(2, 64, 48)[0], 2).model == "pinhole"


def test_every_camera_the_trainer_builds_keeps_the_model(monkeypatch):
    """`make_data`'s cameras -- the true ones, the ones a `pose_noise` perturbs, every factor of the resolution
    schedule -- are fisheye cameras when the configuration says so: none falls back to the pinhole projection."""
    import make_synthetic_dataset as M

    import gs_fused.fisheye as GF
    import harness.train as HT
    from harness.camera_opt import perturb_cameras

    cams = HT.orbit_cameras(3, 48, 32, fov_x_deg=HT.FISHEYE_FOV_X_DEG, model="fisheye")
    moved = perturb_cameras(cams, 0.02, 0.05, 7)
    assert [c.model for c in moved] == ["fisheye"] * 3 and not np.array_equal(moved[0].viewmat, cams[0].viewmat)
    assert [c.model for c in perturb_cameras(HT.orbit_cameras(2, 48, 32), 0.02, 0.05, 7)] == ["pinhole"] * 2
    restore = M.use_cpu_standins()
    monkeypatch.setattr(GF, "project_gaussians_fisheye", _fisheye_standin)
    try:
        for noise in ((0.0, 0.0), (0.02, 0.05)):
            cfg = HT.TrainConfig(camera_model="fisheye", num_gaussians=300, width=48, height=32, num_views=3, sh_degree=1,
                                 iters=20, num_downscales=1, resolution_schedule=10, pose_noise=noise,
                                 scene_scale=(0.03, 0.15))
            data = HT.make_data(cfg, torch.device("cpu"))
            assert sorted(data.cams_by_d) == [1, 2]
            for d, views in data.cams_by_d.items():
                assert [c.model for c in views] == ["fisheye"] * 3, (noise, d)
            assert all(c.model == "fisheye" for c in data.cams_np + data.true_cams_np)
    finally:
        restore()


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option, kw, world", [
    ("fused_render", dict(fused_render=True), 1),
    ("use_graph", dict(use_graph=True), 1),
    ("camera_optimizer", dict(camera_optimizer="SO3xR3"), 1),
    ("normal_consistency", dict(normal_consistency=True), 1),
    ("filter_3d", dict(filter_3d=True), 1),
    ("prune_at", dict(prune_at=(10,)), 1),
    ("world size", dict(), 2),
])
def test_trainer_refusals_name_the_option(option, kw, world):
    import harness.train as HT

    with pytest.raises(ValueError, match=option) as e:
        HT.train(HT.TrainConfig(camera_model="fisheye", iters=1, **kw), torch.device("cpu"), 0, world)
    assert "fisheye" in str(e.value)
    with pytest.raises(ValueError, match="camera_model"):
        HT.train(HT.TrainConfig(camera_model="equirectangular", iters=1), torch.device("cpu"))


def test_render_view_and_fuse_views_refusals_name_the_option():
    from gs_fused import CropBox
    from gs_fusion import fuse_views
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view

    cam_np = S.make_camera(32, 24, fov_x_deg=150.0, model="fisheye")
    assert cam_np.model == "fisheye" and S.make_camera(32, 24).model == "pinhole"
    cam = CameraTensors.from_numpy(cam_np, "cpu")
    assert cam.model == "fisheye" and CameraTensors.from_numpy(S.make_camera(32, 24), "cpu").model == "pinhole"
    n = 4
    args = (torch.zeros(n, 3), torch.ones(n, 3), torch.ones(n, 4), torch.ones(n, 1), torch.zeros(n, 1, 3), cam,
            torch.zeros(3), 0)
    with pytest.raises(ValueError, match="crop"):
        render_view(*args, crop=CropBox(np.eye(3), np.zeros(3), np.ones(3)))
    with pytest.raises(ValueError, match="render_normals"):
        render_view(*args, render_depth=True, render_normals=True)
    with pytest.raises(ValueError, match="camera model"):
        render_view(*args[:5], CameraTensors.from_numpy(S.make_camera(32, 24), "cpu").__class__(
            32, 24, 1.0, 1.0, 1.0, 1.0, torch.eye(4), torch.eye(4), torch.zeros(3), None, "orthographic"), *args[6:])
    with pytest.raises(ValueError, match="fisheye"):
        fuse_views(None, {}, [S.make_camera(32, 24), cam_np], torch.zeros(3), 0)


def test_contribution_stats_and_the_poses_file_refuse_a_fisheye_camera(tmp_path):
    import types

    import harness.train as HT
    from gs_fusion import read_poses_json
    from harness import scene as S
    from harness.pipeline import CameraTensors, contribution_stats

    cam = CameraTensors.from_numpy(S.make_camera(32, 24, fov_x_deg=150.0, model="fisheye"), "cpu")
    model = types.SimpleNamespace(gauss={"means": torch.zeros(4, 3)})
    with pytest.raises(ValueError, match="fisheye"):
        contribution_stats(model, [CameraTensors.from_numpy(S.make_camera(32, 24), "cpu"), cam], HT.TrainConfig())
    entry = {"pose": np.eye(4).tolist(), "camera": {"width": 32, "height": 24, "fx": 20.0, "fy": 20.0, "cx": 16.0, "cy": 12.0}}
    plain, fish = str(tmp_path / "poses.json"), str(tmp_path / "fisheye_poses.json")
    with open(plain, "w") as f:
        json.dump([entry], f)
    with open(fish, "w") as f:
        json.dump([entry, dict(entry, camera=dict(entry["camera"], camera_model="OPENCV_FISHEYE"))], f)
    assert [c.model for c in read_poses_json(plain)] == ["pinhole"]
    with pytest.raises(ValueError, match="OPENCV_FISHEYE"):
        read_poses_json(fish)


def test_the_op_refuses_cpu_tensors():
    from gs_fused import project_gaussians_fisheye

    n = 4
    with pytest.raises(ValueError, match="GPU"):
        project_gaussians_fisheye(torch.zeros(n, 3), torch.ones(n, 3), 1.0, torch.ones(n, 4), torch.eye(4)[:3],
                                  torch.eye(4), 10.0, 10.0, 8.0, 8.0, 16, 16, 16)
