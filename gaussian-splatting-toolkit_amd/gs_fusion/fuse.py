"""Render every camera of a trajectory and fuse it: the loop of the toolkit's `ExportTSDF`
(gs_toolkit/scripts/exporter.py:151-308), without its files."""
import json
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from gs_fused.crop import CropBox
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


def export_mask(mask, bounding_box: bool = False, margin: int = 5) -> Tensor:
    """An object mask as `TSDFFusion.integrate` applies it to a view's depth (exporter/tsdf_fusion.py:105-130,
    `create_bounding_box_mask` :234-262) -> bool [H,W], True where depth is kept.  Torch ops on the mask's device
    (NumPy arrays are taken as CPU tensors).

    `mask` [H,W,3] or [H,W,4] uint8 (an annotation image; a fourth channel is not read, as there):
    ``gray = 0.21 * R + 0.72 * G + 0.07 * B`` in float64, added left to right, truncated to uint8; kept where
    ``gray != 0`` -- so pure red counts from 5, pure green from 2, pure blue from 15.  `mask` [H,W] (any dtype) is
    taken as gray already: kept where non-zero.  That is an extension; the reference indexes three channels.

    `bounding_box`: instead of the mask itself, the inclusive rectangle around its kept pixels, grown by `margin`
    pixels on every side and clipped to the image.  An empty mask then raises ValueError (the reference's `np.min` of
    an empty array does).  This reads four numbers back: the host waits for the device."""
    m = torch.as_tensor(mask)
    if m.dim() == 3 and m.shape[-1] in (3, 4):
        if m.dtype != torch.uint8:
            raise ValueError(f"a colour mask must be uint8, got {m.dtype}")
        c = m.to(torch.float64)
        gray = (0.21 * c[..., 0] + 0.72 * c[..., 1]) + 0.07 * c[..., 2]
        keep = gray.to(torch.uint8) != 0
    elif m.dim() == 2:
        keep = m != 0
    else:
        raise ValueError(f"expected a mask [H,W], [H,W,3] or [H,W,4], got {tuple(m.shape)}")
    if not bounding_box:
        return keep
    if margin < 0:
        raise ValueError("margin must not be negative")
    nz = torch.nonzero(keep)
    if nz.shape[0] == 0:
        raise ValueError("export_mask: the bounding box of an empty mask")
    (y0, x0), (y1, x1) = nz.min(dim=0).values.tolist(), nz.max(dim=0).values.tolist()
    H, W = keep.shape
    y0, y1 = max(y0 - margin, 0), min(y1 + margin, H - 1)
    x0, x1 = max(x0 - margin, 0), min(x1 + margin, W - 1)
    box = torch.zeros_like(keep)
    box[y0:y1 + 1, x0:x1 + 1] = True
    return box


def fuse_views(volume: TSDFVolume, params: Dict[str, Tensor], cameras: Sequence[Camera], background: Tensor,
               sh_degree: int, alpha_min: float = 0.5, depth_trunc: float = 10.0, masks: Optional[Sequence] = None,
               bounding_box: bool = False, mask_margin: int = 5, rasterize_mode: str = "classic",
               crop_box=None, depth_mode: str = "expected") -> None:
    """Render RGB + depth from every camera (`render_view(render_depth=True, fused_depth=True)`: one compositing
    pass) and integrate it into `volume`.  `params`: activated `means3d`, `scales`, `quats`, `opacities`,
    `sh_coeffs` on the volume's device; `cameras`: `harness.scene.Camera` (host arrays).

    `masks`: one object mask per camera (`export_mask`'s input; `ExportTSDF`'s `using_mask` / `mask_path`): a view's
    depth is integrated only where `export_mask(mask, bounding_box, mask_margin)` keeps it.  A mask that is not its
    camera's height x width raises ValueError.  All masks are converted before the first view is rendered.

    `rasterize_mode`: the mode the model was trained in (`render_view`'s; "antialiased" composites opacities *
    compensation) -- depth and alpha of a model trained antialiased are wrong in classic mode, and so is its mesh.

    `crop_box`: a `gs_fused.CropBox` (or its float32[16]): every view is rendered with the Gaussians whose centre the
    box keeps (`render_view(crop=...)`: a test inside the projection kernel, nothing is gathered) -- the cut in 3-D
    that separates an object from what stands behind it, which 2-D masks cannot.  A box that keeps nothing fuses
    nothing.

    `depth_mode`: which depth of a view is fused.  "expected" (the default, what the toolkit fuses): the alpha-blended
    depth, `depth_acc / alpha`.  At a silhouette that is a blend of foreground and background, which the fusion turns
    into a skirt of false surface between the two.  "median": the depth of the Gaussian at which the transmittance
    crosses 0.5 (`render_view(render_distortion=True)`'s "median_depth", gs_fused.depth_distortion) -- one Gaussian's
    depth or the other's, never a blend; what 2DGS, GOF, RaDe-GS and PGSR fuse.  It is valid where `alpha >= alpha_min`
    like the expected depth: with the default 0.5 these are exactly the pixels at which the crossing happened
    (alpha >= 0.5 is final T <= 0.5); with a smaller `alpha_min` the remaining pixels carry the depth of their last
    contributing Gaussian.  Masks, crop box and `rasterize_mode` apply as before.  Anything else raises ValueError.

    Everything stays on the device as float32: there is NO round trip through 8-bit colour PNG and 16-bit millimetre
    depth PNG files as in the toolkit's file-based route, hence none of their quantisation -- a deliberate difference;
    and the host is not synchronised between views."""
    for i, cam in enumerate(cameras):
        if getattr(cam, "model", "pinhole") != "pinhole":
            raise ValueError(f"fuse_views: camera {i} is a {cam.model} camera; TSDF integration projects voxels with "
                             "pinhole intrinsics (fisheye fusion is not built)")
    dev = volume.device
    if rasterize_mode not in ("classic", "antialiased"):
        raise ValueError("Unknown rasterize_mode: %s" % rasterize_mode)
    if depth_mode not in ("expected", "median"):
        raise ValueError("Unknown depth_mode: %s (expected or median)" % (depth_mode,))
    median_kw = {"render_distortion": True} if depth_mode == "median" else {}
    # (a CropBox goes to the device once, not once per view; anything else is `render_view`'s to check)
    crop = crop_box.tensor(dev) if isinstance(crop_box, CropBox) else crop_box
    keeps = None
    if masks is not None:
        if len(masks) != len(cameras):
            raise ValueError(f"{len(masks)} masks for {len(cameras)} cameras")
        keeps = []
        for i, (cam, mask) in enumerate(zip(cameras, masks)):
            m = torch.as_tensor(mask)
            if m.dim() < 2 or (int(m.shape[0]), int(m.shape[1])) != (int(cam.height), int(cam.width)):
                raise ValueError(f"mask {i} is {tuple(m.shape)}, its camera is {cam.height} x {cam.width}")
            keeps.append(export_mask(m.to(dev), bounding_box, mask_margin).to(torch.uint8))
    with torch.no_grad():
        for i, cam in enumerate(cameras):
            out = render_view(params["means3d"], params["scales"], params["quats"], params["opacities"],
                              params["sh_coeffs"], CameraTensors.from_numpy(cam, dev), background, sh_degree,
                              rasterize_mode=rasterize_mode, render_depth=True, fused_depth=True,
                              normalise_depth=False, crop=crop, **median_kw)
            depth, valid = view_depth(out["depth_acc"], out["alpha"], alpha_min)
            if median_kw:
                H, W = valid.shape
                depth = torch.where(valid.bool(), out["median_depth"].reshape(H, W), torch.zeros_like(depth)).contiguous()
            if keeps is not None:
                valid = valid & keeps[i]
            volume.integrate(depth, out["rgb"].contiguous(), cam.fx, cam.fy, cam.cx, cam.cy, cam.viewmat, valid=valid,
                             depth_trunc=depth_trunc)


def read_poses_json(path: str) -> List[Camera]:
    """The trajectory file `TSDFFusion.read_trajectory` reads: a list of {"pose": 4x4 camera-to-world,
    "camera": {width, height, fx, fy, cx, cy}}.  `viewmat` is the fp64 inverse of `pose`, rounded to fp32.  The format
    has no field for the camera model and every entry is read as a pinhole camera; an optional "camera_model" key in
    "camera" (absent from the toolkit's files) is honoured: anything but "pinhole" / "perspective" raises ValueError,
    since TSDF integration projects voxels with pinhole intrinsics."""
    with open(path) as f:
        entries = json.load(f)
    cams = []
    for e in entries:
        pose = np.asarray(e["pose"], np.float64).reshape(4, 4)
        c = e["camera"]
        model = str(c.get("camera_model", c.get("model", "pinhole")))
        if model.lower() not in ("pinhole", "perspective"):
            raise ValueError(f"{path}: a {model} camera (fisheye?) cannot be fused; TSDF integration projects voxels with "
                             "pinhole intrinsics")
        W, H = int(c["width"]), int(c["height"])
        fx, fy = float(c["fx"]), float(c["fy"])
        V = np.linalg.inv(pose).astype(np.float32)
        P = projection_matrix(0.001, 1000.0, 2 * math.atan(W / (2 * fx)), 2 * math.atan(H / (2 * fy)))
        cams.append(Camera(W, H, fx, fy, float(c["cx"]), float(c["cy"]), V, (P @ V).astype(np.float32)))
    return cams
