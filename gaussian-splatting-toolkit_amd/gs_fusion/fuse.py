"""Render every camera of a trajectory and fuse it: the loop of the toolkit's `ExportTSDF`
(gs_toolkit/scripts/exporter.py:151-308), without its files."""
import json
import math
from typing import Dict, List, Sequence

import numpy as np
import torch
from torch import Tensor

from harness.pipeline import CameraTensors, render_view
from harness.scene import Camera, projection_matrix

from .volume import TSDFVolume


def view_depth(depth_acc: Tensor, alpha: Tensor, alpha_min: float = 0.5):
    """Accumulated depth and alpha of a compositing pass -> (z-depth [H,W], valid [H,W] uint8):
    depth = depth_acc / alpha and valid where alpha >= alpha_min, depth 0 elsewhere."""
    a = alpha.reshape(alpha.shape[0], alpha.shape[1])
    d = depth_acc.reshape(a.shape)
    valid = a >= alpha_min
    depth = torch.where(valid, d / a, torch.zeros_like(d))
    return depth.contiguous(), valid.to(torch.uint8)


def fuse_views(volume: TSDFVolume, params: Dict[str, Tensor], cameras: Sequence[Camera], background: Tensor,
               sh_degree: int, alpha_min: float = 0.5, depth_trunc: float = 10.0) -> None:
    """Render RGB + depth from every camera (`render_view(render_depth=True, fused_depth=True)`: one compositing
    pass) and integrate it into `volume`.  `params`: activated `means3d`, `scales`, `quats`, `opacities`,
    `sh_coeffs` on the volume's device; `cameras`: `harness.scene.Camera` (host arrays).

    Everything stays on the device as float32: there is NO round trip through 8-bit colour PNG and 16-bit millimetre
    depth PNG files as in the toolkit's file-based route, hence none of their quantisation -- a deliberate difference;
    and the host is not synchronised between views."""
    dev = volume.device
    with torch.no_grad():
        for cam in cameras:
            out = render_view(params["means3d"], params["scales"], params["quats"], params["opacities"],
                              params["sh_coeffs"], CameraTensors.from_numpy(cam, dev), background, sh_degree,
                              render_depth=True, fused_depth=True, normalise_depth=False)
            depth, valid = view_depth(out["depth_acc"], out["alpha"], alpha_min)
            volume.integrate(depth, out["rgb"].contiguous(), cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat, valid=valid,
                             depth_trunc=depth_trunc)


def read_poses_json(path: str) -> List[Camera]:
    """The trajectory file `TSDFFusion.read_trajectory` reads: a list of {"pose": 4x4 camera-to-world,
    "camera": {width, height, fx, fy, cx, cy}}.  `viewmat` is the fp64 inverse of `pose`, rounded to fp32."""
    with open(path) as f:
        entries = json.load(f)
    cams = []
    for e in entries:
        pose = np.asarray(e["pose"], np.float64).reshape(4, 4)
        c = e["camera"]
        W, H = int(c["width"]), int(c["height"])
        fx, fy = float(c["fx"]), float(c["fy"])
        V = np.linalg.inv(pose).astype(np.float32)
        P = projection_matrix(0.001, 1000.0, 2 * math.atan(W / (2 * fx)), 2 * math.atan(H / (2 * fy)))
        cams.append(Camera(W, H, fx, fy, float(c["cx"]), float(c["cy"]), V, (P @ V).astype(np.float32)))
    return cams
