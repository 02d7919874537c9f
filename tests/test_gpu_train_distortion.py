"""GPU: the depth-distortion term in the trainer (TrainConfig.depth_distortion), the render
call's new keys, and the median depth in the TSDF export.

The trainer runs three hundred iterations of the size the trainer tests use, same seed: with the term, and with the
term at `distortion_lambda = 0` -- the run without the term's influence on which the same quantity can be read (the
record carries it; a weight of zero adds exact zeros to every gradient)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "trajectory_gpu.json")

# the size the trainer tests use (tests/test_gpu_train_normals.py), three hundred iterations
SMALL = dict(num_gaussians=20_000, width=320, height=180, num_views=8, iters=300, sh_degree=3, sh_degree_interval=100,
             log_every=50)


@pytest.fixture(scope="module")
def runs():
    from harness.train import TrainConfig, train

    dev = torch.device("cuda", 0)
    on = dict(depth_distortion=True, distortion_start_iteration=0)
    return {"on": train(TrainConfig(**on, **SMALL), dev),
            "zero": train(TrainConfig(**on, distortion_lambda=0.0, **SMALL), dev)}


def test_the_term_falls_and_ends_below_the_run_without_it(runs):
    on, zero = runs["on"], runs["zero"]
    assert on["render"] == "separate ops"
    assert all(math.isfinite(v) for v in on["losses"]) and math.isfinite(on["param_checksum"])
    rec, rec0 = on["depth_distortion"], zero["depth_distortion"]
    print(f"term with lambda {rec['lambda']}: {rec['term_first']:.6e} -> {rec['term_last']:.6e}; with lambda 0: "
          f"{rec0['term_first']:.6e} -> {rec0['term_last']:.6e}; PSNR {on['psnr_end']:.2f} against {zero['psnr_end']:.2f}")
    assert rec["lambda"] == 100.0 and rec["start_iteration"] == 0 and (rec["near"], rec["far"]) == (0.2, 100.0)
    assert rec0["lambda"] == 0.0
    assert rec["term_first"] > 0.0 and math.isfinite(rec["term_last"])
    assert rec["term_last"] < rec["term_first"]
    assert rec["term_last"] < rec0["term_last"]


def test_the_default_run_is_the_parents_run():
    """tools/train_trajectory.py's "gpu" case (deterministic mode, densification included) against the record the
    commit before this option printed for it on an MI355X (tests/golden/trajectory_gpu.json: that tool's JSON line,
    floats as hex), and a run that names the option but leaves it off."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_trajectory as TT

    import harness.train as HT
    from gs_fused import RefineConfig
    from rasterizer import rasterize as R

    kw = dict(TT.BASE, **TT.CASES["gpu"])
    was = R.is_deterministic()
    R.set_deterministic(True)
    try:
        def record(**more):
            res = HT.train(HT.TrainConfig(refine=RefineConfig(**TT.GPU_REFINE), sharded_adam=False, **kw, **more),
                           torch.device("cuda", 0))
            return {k: TT._hex(v) for k, v in res.items() if k not in TT.TIMING and not k.startswith("phase_")}

        plain = record()
        off = record(depth_distortion=False, distortion_lambda=3.0, distortion_start_iteration=0)
    finally:
        R.set_deterministic(was)
    assert "depth_distortion" not in plain
    assert json.dumps(off, sort_keys=True) == json.dumps(plain, sort_keys=True)
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(plain))  # (tuples as lists, as the file has them)
    for k in ("case", "world", "sharded", "rank"):
        want.pop(k)
    differing = sorted(k for k in set(want) | set(got) if want.get(k) != got.get(k))
    print(f"keys: {len(got)}; differing from the parent's record: {differing}")
    assert not differing


def test_render_view_returns_the_new_keys():
    from harness import scene as S
    from harness.pipeline import CameraTensors, render_view

    cam = S.make_camera(96, 64, yaw=0.1, pitch=-0.05)
    sc = S.make_scene(1500, cam, sh_degree=1, seed=3, scale_lo=0.02, scale_hi=0.1)
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    args = (t(sc["means3d"]).requires_grad_(True), t(sc["scales"]), t(sc["quats"]), t(sc["opacities"]).requires_grad_(True),
            t(sc["sh_coeffs"]), CameraTensors.from_numpy(cam, DEV), t(np.array(S.BACKGROUND, np.float32)), 1)
    plain = render_view(*args, render_depth=True)
    out = render_view(*args, render_depth=True, render_distortion=True)
    assert set(out) == set(plain) | {"distortion", "median_depth"}
    assert out["distortion"].shape == (64, 96, 1) and out["median_depth"].shape == (64, 96, 1)
    assert torch.equal(out["rgb"], plain["rgb"]) and torch.equal(out["depth"], plain["depth"])
    assert set(render_view(*args, render_distortion=True)) == set(render_view(*args))  # (needs render_depth)
    d, m = out["distortion"], out["median_depth"]
    assert bool((d >= -1e-6).all()) and float(d.max()) > 0 and not m.requires_grad  # (depth-sorted lists: |.| >= 0)
    seen = out["alpha"] > 0
    depths = out["depths"].detach()
    assert bool((m[seen] >= depths[out["radii"] > 0].min()).all()) and bool((m[seen] <= depths.max()).all())
    # the mapped values and the gradient's way to the means
    mapped = render_view(*args, render_depth=True, render_distortion=True,
                         distortion_values=lambda z: 100.0 / 99.8 * (1.0 - 0.2 / z))
    mapped["distortion"].mean().backward()
    assert float(args[0].grad.abs().max()) > 0 and float(args[3].grad.abs().max()) > 0
    assert bool(torch.isfinite(args[0].grad).all())
    assert float(mapped["median_depth"].max()) < 100.0 / 99.8


def _two_planes():
    """A near square (z = 1, 0.8 wide) in front of a far wall (z = 2.5, 3 wide): opaque flat discs facing -z."""
    from harness.scene import SH_C0

    def grid(half, step, z, colour):
        u = np.arange(-half, half + 1e-9, step)
        x, y = (a.reshape(-1) for a in np.meshgrid(u, u))
        n = x.size
        f32 = np.float32
        return {"means": np.stack([x, y, np.full(n, z)], 1).astype(f32),
                "scales": np.log(np.tile([0.8 * step, 0.8 * step, 0.002], (n, 1))).astype(f32),
                "quats": np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)).astype(f32), "opacities": np.full((n, 1), 6.0, f32),
                "features_dc": np.tile((np.asarray(colour) - 0.5) / SH_C0, (n, 1)).astype(f32),
                "features_rest": np.zeros((n, 0, 3), f32)}

    near, far = grid(0.4, 0.04, 1.0, (0.9, 0.2, 0.2)), grid(1.5, 0.08, 2.5, (0.2, 0.3, 0.9))
    return {k: np.concatenate([near[k], far[k]]) for k in near}


def test_median_depth_leaves_no_skirt_between_two_planes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from export_tsdf import activated

    import tsdf_reference as TR
    from gs_fusion import TSDFVolume, fuse_views
    from harness.scene import Camera, projection_matrix

    W = H = 128
    fx = fy = 100.0
    V = TR.look_at((0.0, 0.0, -1.0), (0.0, 0.0, 1.0))
    P = projection_matrix(0.001, 1000.0, 2 * math.atan(W / (2 * fx)), 2 * math.atan(H / (2 * fy)))
    cams = [Camera(W, H, fx, fy, W / 2, H / 2, V, (P @ V).astype(np.float32))]
    params = activated(_two_planes(), torch.device(DEV))
    bg = torch.zeros(3, device=DEV)

    # (the planes lie between the voxels' sample points: a depth map that is exactly flat puts no exact zero on them)
    LO, HI = [-1.6, -1.6, 0.613], [1.6, 1.6, 2.913]

    def gap_points(mode):
        vol = TSDFVolume.from_bounds(LO, HI, 0.04, 0.12, None, DEV)
        fuse_views(vol, params, cams, bg, 0, **({} if mode is None else {"depth_mode": mode}))
        p = vol.extract_point_cloud()[0].cpu().numpy()
        # the open gap: further than the truncation distance (and a voxel) behind the square and in front of the wall
        gap = (p[:, 2] > 1.0 + 0.2) & (p[:, 2] < 2.5 - 0.2)
        on_planes = (np.abs(p[:, 2] - 1.0) < 0.1) | (np.abs(p[:, 2] - 2.5) < 0.1)
        print(f"depth_mode {mode}: {len(p)} surface points, {int(on_planes.sum())} on the planes, {int(gap.sum())} in "
              f"the gap")
        return len(p), int(on_planes.sum()), int(gap.sum())

    n_e, planes_e, gap_e = gap_points("expected")
    n_m, planes_m, gap_m = gap_points("median")
    assert gap_points(None) == (n_e, planes_e, gap_e)  # the default is "expected"
    assert planes_e > 1000 and planes_m > 1000
    assert gap_e > 0   # the blend of square and wall along the silhouette: the skirt
    assert gap_m == 0  # one Gaussian's depth or the other's
    vol = TSDFVolume.from_bounds(LO, HI, 0.04, 0.12, None, DEV)
    with pytest.raises(ValueError, match="depth_mode"):
        fuse_views(vol, params, cams, bg, 0, depth_mode="bogus")


@pytest.mark.parametrize("what, kw, world, device", [
    ("fused_render", dict(fused_render=True), 1, "cuda"),
    ("use_graph", dict(use_graph=True), 1, "cuda"),
    ("world size", dict(), 2, "cuda"),
    ("CUDA", dict(), 1, "cpu"),
    ("deterministic", dict(), 1, "cuda"),
])
def test_the_trainer_refuses_by_name(what, kw, world, device):
    import harness.train as HT
    from rasterizer import rasterize as R

    cfg = HT.TrainConfig(depth_distortion=True, **kw)
    was = R.is_deterministic()
    R.set_deterministic(what == "deterministic")
    try:
        with pytest.raises(ValueError, match="depth_distortion.*" + what):
            HT._check_depth_distortion(cfg, torch.device(device), world)
        if what == "deterministic":
            R.set_deterministic(False)
            HT._check_depth_distortion(cfg, torch.device(device), world)  # everything else is in order
        HT._check_depth_distortion(HT.TrainConfig(**kw), torch.device(device), world)  # off: nothing to refuse
    finally:
        R.set_deterministic(was)
