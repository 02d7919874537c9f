#!/usr/bin/env python3
"""Render one of the harness's hidden scenes into a dataset directory the toolkit's dataparser (and
gs_io.dataset.load_dataset) reads: `images/frame_00000.png ...` (RGBA with --alpha, straight colour; RGB over
scene.BACKGROUND otherwise), `depths/*.png` (16 bit, millimetres, 0 = no measurement), `masks/*.png` (the object's
silhouette, 0 / 255), `sparse_pc.ply` (a seed cloud: surface points with 8-bit colours) and `transforms.json`
(camera-to-world matrices in the dataset convention -- x right, y up, z backwards -- and pinhole (or, --camera-model OPENCV_FISHEYE, equidistant) intrinsics, global or
with --per-frame per frame).  The images are the ones `harness.train.make_data` renders for the same settings.

    python tools/make_synthetic_dataset.py OUT [--views 12 --width 64 --height 48 --alpha] [--device cpu]

On the CPU the native ops are the oracle-backed stand-ins of tests/cpu_standins.py, as in tools/train_trajectory.py.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "gaussian-splatting-toolkit_amd"), os.path.join(ROOT, "tests"))
                if p not in sys.path]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def use_cpu_standins():
    """Wire the oracle-backed stand-ins into harness.pipeline (idempotent); returns a function that undoes it."""
    import cpu_standins as SI
    import harness.pipeline as HP

    saved = (HP.project_gaussians, HP.spherical_harmonics, HP.rasterize_gaussians)
    HP.project_gaussians, HP.spherical_harmonics, HP.rasterize_gaussians = (
        SI.project_gaussians, SI.spherical_harmonics, SI.rasterize_gaussians)

    def restore():
        HP.project_gaussians, HP.spherical_harmonics, HP.rasterize_gaussians = saved

    return restore


def camera_to_world_gl(viewmat: np.ndarray) -> np.ndarray:
    """world->camera of the rasterizer (x right, y down, z forward) -> camera-to-world [4,4] of a transforms.json
    (x right, y up, z backwards): the inverse, with the camera's y and z axes flipped."""
    V = np.asarray(viewmat, np.float64)
    R, t = V[:3, :3], V[:3, 3]
    c2w = np.eye(4)
    c2w[:3, :3] = R.T @ np.diag([1.0, -1.0, -1.0])
    c2w[:3, 3] = -R.T @ t
    return c2w.astype(np.float32)


def to_u8(x: torch.Tensor) -> np.ndarray:
    return torch.round(x.clamp(0.0, 1.0) * 255.0).to(torch.uint8).cpu().numpy()


def make_synthetic_dataset(out: str, views: int = 12, width: int = 64, height: int = 48, alpha: bool = True,
                           depth: bool = True, mask: bool = True, device="cpu", scene: str = "ball",
                           num_gaussians: int = 600, seed_points: int = 200, seed: int = 0, per_frame: bool = False,
                           scene_scale=(0.03, 0.15), extra_meta=None, view_exposure=(0.0, 0.0),
                           view_exposure_seed: int = 20241020, camera_model: str = "PINHOLE") -> dict:
    """Writes the directory and returns the transforms.json dict.  `device` "cpu" needs the stand-ins wired
    (`use_cpu_standins`), as every CPU run of the harness does.  `view_exposure` (sigma of the log-gain, sigma of the
    bias): every image's colour is disturbed per view and channel before it is quantised, as
    `TrainConfig.view_exposure` disturbs the trainer's targets (`harness.train.disturb_exposure`); the gains and biases
    go into transforms.json under "view_exposure".  `camera_model` "OPENCV_FISHEYE": the cameras are the trainer's
    equidistant ones (`TrainConfig.camera_model="fisheye"`), the images are rendered through them, and transforms.json
    states the model with `k1..k4 = 0` (gs_io.dataset.load_dataset reads it with `allow_fisheye=True`)."""
    from PIL import Image

    import harness.train as HT
    from gs_io.ply import write_point_cloud_ply
    from harness import scene as S

    if camera_model not in ("PINHOLE", "OPENCV_FISHEYE"):
        raise ValueError(f"camera_model must be PINHOLE or OPENCV_FISHEYE, got {camera_model!r}")
    device = torch.device(device)
    cfg = HT.TrainConfig(**({"camera_model": "fisheye"} if camera_model == "OPENCV_FISHEYE" else {}),
                         num_gaussians=num_gaussians, width=width, height=height, num_views=views, seed=seed,
                         scene=scene, scene_scale=tuple(scene_scale), sh_degree=1,
                         background_color="random" if alpha else "fixed", model="co-gs" if depth else "gaussian-splatting",
                         mask="alpha" if mask else "none")
    data = HT.make_data(cfg, device)
    colour = [g[..., :3] for g in (data.gt_rgba if alpha else data.gt)]
    exposure = None
    if tuple(view_exposure) != (0.0, 0.0):
        colour, exposure = HT.disturb_exposure(colour, view_exposure[0], view_exposure[1], view_exposure_seed)
    for sub in ("images", "depths", "masks"):
        os.makedirs(os.path.join(out, sub), exist_ok=True)
    cam0 = data.true_cams_np[0]
    meta = {"camera_model": camera_model}
    if camera_model == "OPENCV_FISHEYE":
        meta.update(k1=0.0, k2=0.0, k3=0.0, k4=0.0)
    intr = {"fl_x": float(cam0.fx), "fl_y": float(cam0.fy), "cx": float(cam0.cx), "cy": float(cam0.cy),
            "w": int(width), "h": int(height)}
    if not per_frame:
        meta.update(intr)
    frames = []
    for v, cam in enumerate(data.true_cams_np):
        name = f"frame_{v:05d}.png"
        img = to_u8(torch.cat((colour[v], data.gt_rgba[v][..., 3:]), dim=-1) if alpha else colour[v])
        Image.fromarray(img, "RGBA" if alpha else "RGB").save(os.path.join(out, "images", name))
        fr = {"file_path": f"images/{name}", "transform_matrix": camera_to_world_gl(cam.viewmat).astype(float).tolist()}
        if per_frame:
            fr.update(intr)
        if depth:
            mm = torch.round(data.gt_depth[v] * 1000.0).clamp(0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)
            Image.fromarray(mm).save(os.path.join(out, "depths", name))
            fr["depth_path"] = f"depths/{name}"
        if mask:
            m = (data.masks[v][..., 0] > 0.5).to(torch.uint8).cpu().numpy() * np.uint8(255)
            Image.fromarray(m, "L").save(os.path.join(out, "masks", name))
            fr["mask_path"] = f"masks/{name}"
        frames.append(fr)
    # the seed cloud: surface points of the hidden scene with their view-independent colour in 8 bits, as
    # harness.train.seed_model's "sfm" start draws them (without its triangulation noise)
    truth = HT._hidden_scene(cfg)
    rng = np.random.default_rng(seed + 1)
    pick = np.sort(rng.choice(truth["means"].shape[0], min(seed_points, truth["means"].shape[0]), replace=False))
    rgb = np.clip(truth["features_dc"][pick] * S.SH_C0 + 0.5, 0.0, 1.0)
    write_point_cloud_ply(os.path.join(out, "sparse_pc.ply"), truth["means"][pick], rgb)
    meta["ply_file_path"] = "sparse_pc.ply"
    meta["frames"] = frames
    if exposure is not None:
        meta["view_exposure"] = exposure
    meta.update(extra_meta or {})
    with open(os.path.join(out, "transforms.json"), "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1)
    return meta


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("out")
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--alpha", action="store_true", help="RGBA images with straight colour")
    ap.add_argument("--no-depth", action="store_true")
    ap.add_argument("--no-mask", action="store_true")
    ap.add_argument("--per-frame", action="store_true", help="intrinsics and size in every frame, not globally")
    ap.add_argument("--scene", default="ball", choices=["ball", "shell", "objects"])
    ap.add_argument("--gaussians", type=int, default=600)
    ap.add_argument("--seed-points", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--view-exposure", type=float, nargs=2, default=[0.0, 0.0], metavar=("G", "B"),
                    help="per-view, per-channel gain exp(N(0, G)) and bias N(0, B) on every image")
    ap.add_argument("--camera-model", default="PINHOLE", choices=["PINHOLE", "OPENCV_FISHEYE"],
                    help="OPENCV_FISHEYE: equidistant cameras (every distortion coefficient zero), rendered as such")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu", choices=["cpu", "cuda"])
    args = ap.parse_args()
    if args.device == "cpu":
        use_cpu_standins()
    meta = make_synthetic_dataset(args.out, args.views, args.width, args.height, args.alpha, not args.no_depth,
                                  not args.no_mask, args.device, args.scene, args.gaussians, args.seed_points,
                                  args.seed, args.per_frame, view_exposure=tuple(args.view_exposure),
                                  camera_model=args.camera_model)
    print(json.dumps({"out": args.out, "frames": len(meta["frames"]), "width": args.width, "height": args.height}))


if __name__ == "__main__":
    main()
