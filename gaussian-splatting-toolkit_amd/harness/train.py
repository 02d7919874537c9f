"""A minimal trainer with the toolkit's call pattern, for
BASELINE configs 3/4: `gs-train gaussian-splatting` on a synthetic scene, one
GPU or per-view data parallel.

What is reproduced from the reference (so that the rasterizer sees exactly the
calls the real models make):
  * parameters and activations of `GaussianSplattingModel`
    (gs_toolkit/models/vanilla_gs.py:128-174, 765-820): means, log-scales,
    unnormalised quats, logit opacities, features_dc [N,3], features_rest
    [N,15,3]; `exp`, normalise, `sigmoid`, SH degree warm-up
    `min(step // sh_degree_interval, sh_degree)`, `clamp(SH + 0.5, min=0)`;
  * the loss `(1 - lambda) L1 + lambda (1 - SSIM)` with lambda = 0.2
    (vanilla_gs.py:900-947; SSIM restated in plain torch, 11x11 Gaussian window);
  * one Adam optimiser per parameter group with the learning rates of
    gs_toolkit/configs/method_configs.py:98-132;
  * `xys.retain_grad()` and the densification statistics of `after_train`
    (vanilla_gs.py:344-372), and -- with `TrainConfig.densify` -- the refinement
    schedule of `refinement_after` (:381-497) every `refine_every` iterations:
    split / duplicate / cull / opacity reset with the Adam state carried along
    (`gs_fused.refine_gaussians`, one compaction launch).  Under data parallelism
    the statistics are all-reduced first and the split samples come from a
    counter-based generator keyed on (seed, step, Gaussian index), so every replica
    takes the same decisions and stays bit-identical.
The data side (cameras on a sphere, ground truth rendered by this rasterizer
from a hidden "true" scene) replaces the toolkit's datamanager.
"""
import gc
import math
import os
import time
from dataclasses import dataclass, replace
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import cogs_losses
from . import scene as S
from .parallel import GradientExchange, allreduce_densify_stats, view_for_rank
from .pipeline import CameraTensors, render_view

PARAM_NAMES = ("means", "scales", "quats", "features_dc", "features_rest", "opacities")

LRS = {"means": 1.6e-4, "features_dc": 0.0025, "features_rest": 0.0025 / 20, "opacities": 0.05,
       "scales": 0.005, "quats": 0.001}
SH_C0 = 0.28209479177387814


FISHEYE_FOV_X_DEG = 150.0  # the synthetic fisheye cameras' horizontal field of view


def orbit_cameras(n_views: int, width: int, height: int, radius: float = 6.0, fov_x_deg: float = 60.0,
                  model: str = "pinhole"):
    """Cameras on a circle around the origin, all looking at it (rasterizer
    convention: x right, y down, z forward)."""
    cams = []
    for i in range(n_views):
        th = 2 * math.pi * i / n_views
        eye = np.array([radius * math.sin(th), 0.6 * math.sin(2 * th), -radius * math.cos(th)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(np.array([0.0, -1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])  # world -> camera rows
        cam = S.make_camera(width, height, fov_x_deg, model=model)
        V = np.eye(4, dtype=np.float32)
        V[:3, :3] = R.astype(np.float32)
        V[:3, 3] = (-R @ eye).astype(np.float32)
        fovx = math.radians(fov_x_deg) if model == "pinhole" else 2.0 * math.atan(width / (2.0 * cam.fx))
        fovy = 2.0 * math.atan(height / (2.0 * cam.fy))
        P = S.projection_matrix(0.001, 1000.0, fovx, fovy) @ V
        cams.append(S.Camera(width, height, cam.fx, cam.fy, cam.cx, cam.cy, V, P.astype(np.float32), model))
    return cams


def rescale_camera(cam, d: int):
    """`camera.rescale_output_resolution(1 / d)` (gs_toolkit/cameras/cameras.py:1176-1213: fx, fy, cx, cy scaled,
    width and height scaled and truncated to integers) followed by what `get_outputs` derives from the rescaled
    camera (vanilla_gs.py:736-742: the fields of view from the NEW width / fx, the projection matrix from those)."""
    if d == 1:
        return cam
    f = 1.0 / d
    fx, fy, cx, cy = cam.fx * f, cam.fy * f, cam.cx * f, cam.cy * f
    W, H = int(cam.width * f), int(cam.height * f)
    fovx, fovy = 2.0 * math.atan(W / (2.0 * fx)), 2.0 * math.atan(H / (2.0 * fy))
    P = S.projection_matrix(0.001, 1000.0, fovx, fovy) @ cam.viewmat
    return S.Camera(W, H, fx, fy, cx, cy, cam.viewmat, P.astype(np.float32), cam.model)


def downscale_factor(step: int, num_downscales: int, resolution_schedule: int) -> int:
    """`_get_downscale_factor` while training (vanilla_gs.py:646-657): 2^max(num_downscales - step // schedule, 0)."""
    return 2 ** max(num_downscales - step // max(resolution_schedule, 1), 0)


def downscale_image(image: torch.Tensor, d: int) -> torch.Tensor:
    """`_downscale_if_required` (vanilla_gs.py:659-670): `TF.resize(image.permute(2, 0, 1), [H // d, W // d],
    antialias=None)` -- for tensors that is bilinear interpolation without antialiasing."""
    if d <= 1:
        return image
    newsize = [image.shape[0] // d, image.shape[1] // d]
    return F.interpolate(image.permute(2, 0, 1)[None], size=newsize, mode="bilinear", align_corners=False,
                         antialias=False)[0].permute(1, 2, 0)


def downscale_depth(depth: torch.Tensor, d: int) -> torch.Tensor:
    """`DepthGSModel._downscale_if_required` for a 2-D image (depth_gs.py:161-176): resized as [1,H,W]."""
    if d <= 1:
        return depth
    return F.interpolate(depth[None, None], size=[depth.shape[0] // d, depth.shape[1] // d], mode="bilinear",
                         align_corners=False, antialias=False)[0, 0]


def downscale_mask(mask: torch.Tensor, d: int) -> torch.Tensor:
    """`self._downscale_if_required(batch["mask"])` (vanilla_gs.py:919, surface_gs.py:921, depth_gs.py:429): the
    [H,W,1] mask goes through the resize the image goes through -- bilinear, no antialiasing -- so under the resolution
    schedule a 0/1 mask comes out with fractional values along its edges."""
    return downscale_image(mask, d)


def view_masks(kind: str, height: int, width: int, alphas, device) -> List[torch.Tensor]:
    """`TrainConfig.mask` -> one float [H,W,1] mask per view.  "alpha": the object's silhouette, where the accumulated
    opacity of the hidden scene's render (`alphas[v]`, [H,W,1]) is above 0.5.  "box": rows H//4 .. 3H//4 - 1 and columns
    W//4 .. 3W//4 - 1 are 1, everything else 0, the same for every view."""
    if kind == "alpha":
        return [(a > 0.5).to(torch.float32).contiguous() for a in alphas]
    if kind == "box":
        m = torch.zeros((height, width, 1), device=device)
        m[height // 4:3 * height // 4, width // 4:3 * width // 4] = 1.0
        return [m for _ in alphas]
    raise ValueError(f"unknown mask {kind!r}")


def composite_with_background(image: torch.Tensor, background: torch.Tensor) -> torch.Tensor:
    """What the models do with a ground-truth image that carries an alpha channel (vanilla_gs.py:870-881): straight
    colour over the step's background, `a * rgb + (1 - a) * background`; an RGB image is returned as it is."""
    if image.shape[-1] != 4:
        return image
    rgb, a = image[..., :3], image[..., 3:4]
    return a * rgb + (1.0 - a) * background


def blob_scene(n: int, seed: int, sh_degree: int = 3, extent: float = 1.5, scale_lo=0.01, scale_hi=0.06,
               kind: str = "ball", tex_cell: float = 0.04, objects=(48, 0.18, 0.45)):
    """Raw (pre-activation) Gaussians around the origin.  kind="ball": semi-transparent
    Gaussians filling a ball (a smooth volume).  kind="shell": opaque, small, flat-ish
    Gaussians on three nested textured spheres -- surfaces with detail at the pixel scale,
    the kind of scene densification exists for."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 3))
    p /= np.linalg.norm(p, axis=-1, keepdims=True)
    K = S.num_sh_bases(sh_degree)
    f32 = np.float32
    if kind == "objects":
        # a nerfstudio-style object scene: `n_obj` opaque spheres of different sizes scattered in a
        # ball (silhouettes against the background, mutual occlusion), each tiled by small FLAT
        # Gaussians aligned with the surface and textured with a high-contrast checker whose cells
        # are a few Gaussians wide -- detail a sparse start cannot represent without densifying
        n_obj, r_lo, r_hi = int(objects[0]), float(objects[1]), float(objects[2])
        centres = rng.standard_normal((n_obj, 3))
        centres *= (extent * rng.uniform(0.15, 1.0, (n_obj, 1)) ** (1 / 3)) / np.linalg.norm(centres, axis=-1, keepdims=True)
        radii = rng.uniform(r_lo, r_hi, n_obj)
        which = rng.choice(n_obj, n, p=radii ** 2 / np.sum(radii ** 2))  # by area
        r = radii[which][:, None]
        means = centres[which] + p * (r + 0.002 * rng.standard_normal((n, 1)))
        base = rng.uniform(0.15, 0.85, (n_obj, 3))[which]
        other = rng.uniform(0.0, 1.0, (n_obj, 3))[which]
        cell = tex_cell / r[:, 0]  # checker cell size in radians: `tex_cell` scene units on every sphere
        u = np.arctan2(p[:, 0], p[:, 2]) * np.maximum(np.sqrt(1 - p[:, 1] ** 2), 0.2)
        v = np.arcsin(np.clip(p[:, 1], -1, 1))
        chk = ((np.floor(u / cell) + np.floor(v / cell)) % 2)[:, None]
        colour = np.where(chk > 0, base, other) * (0.85 + 0.15 * rng.uniform(0, 1, (n, 1)))
        dc = (np.clip(colour, 0, 1) - 0.5) / SH_C0
        s_t = rng.uniform(math.log(scale_lo), math.log(scale_hi), (n, 2))
        scales = np.concatenate([s_t, s_t.min(axis=1, keepdims=True) + math.log(0.15)], axis=1)  # thin along the normal
        # quaternion (w, x, y, z) turning the local z axis into the outward normal p
        quats = np.stack([1.0 + p[:, 2], -p[:, 1], p[:, 0], np.zeros(n)], axis=-1)
        quats[np.linalg.norm(quats, axis=-1) < 1e-6] = (0.0, 1.0, 0.0, 0.0)
        quats /= np.linalg.norm(quats, axis=-1, keepdims=True)
        return {
            "means": means.astype(f32), "scales": scales.astype(f32), "quats": quats.astype(f32),
            "opacities": rng.uniform(2.0, 5.0, (n, 1)).astype(f32), "features_dc": dc.astype(f32),
            "features_rest": (rng.standard_normal((n, K - 1, 3)) * 0.02).astype(f32),
        }
    if kind == "shell":
        radius = np.array([0.7, 1.1, 1.5])[rng.integers(0, 3, n)][:, None]
        means = p * (radius + 0.004 * rng.standard_normal((n, 1)))
        # texture: colour varies smoothly over the sphere plus per-Gaussian contrast
        tex = 0.5 + 0.5 * np.sin(9.0 * p @ rng.standard_normal((3, 3)) + 5.0 * radius)
        dc = (0.7 * tex + 0.3 * rng.uniform(0, 1, (n, 3)) - 0.5) / SH_C0
        scales = rng.uniform(math.log(scale_lo), math.log(scale_hi), (n, 3))
        opac = rng.uniform(1.0, 4.0, (n, 1))
    else:
        means = p * (extent * rng.uniform(0, 1, (n, 1)) ** (1 / 3))
        dc = (rng.uniform(0, 1, (n, 3)) - 0.5) / SH_C0
        scales = np.log(np.exp(rng.uniform(math.log(scale_lo), math.log(scale_hi), (n, 3))))
        opac = rng.uniform(-1.0, 2.0, (n, 1))  # logits
    return {
        "means": means.astype(f32),
        "scales": scales.astype(f32),
        "quats": rng.standard_normal((n, 4)).astype(f32),
        "opacities": opac.astype(f32),
        "features_dc": dc.astype(f32),
        "features_rest": (rng.standard_normal((n, K - 1, 3)) * 0.05).astype(f32),
    }


def knn_mean_distance(points: np.ndarray, k: int = 3) -> np.ndarray:
    """Mean distance to the k nearest neighbours, the reference's initial scale
    (`k_nearest_sklearn`, vanilla_gs.py:136-140, 260-280: k + 1 neighbours, self dropped)."""
    from sklearn.neighbors import NearestNeighbors

    d, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="auto", metric="euclidean").fit(points).kneighbors(points)
    return d[:, 1:].astype(np.float32).mean(axis=-1)


def random_quats(n: int, rng) -> np.ndarray:
    """`random_quat_tensor` (gs_toolkit/utils/comms.py:69-84): uniform on the unit 3-sphere."""
    u, v, w = rng.uniform(size=n), rng.uniform(size=n), rng.uniform(size=n)
    return np.stack([np.sqrt(1 - u) * np.sin(2 * math.pi * v), np.sqrt(1 - u) * np.cos(2 * math.pi * v),
                     np.sqrt(u) * np.sin(2 * math.pi * w), np.sqrt(u) * np.cos(2 * math.pi * w)], -1).astype(np.float32)


def seed_model(truth: Dict[str, np.ndarray], n_seed: int, kind: str, seed: int, sh_degree: int = 3,
               sfm_noise: float = 0.01, random_scale: float = 3.4, knn: str = "sklearn", device=None):
    """The model's start as `GaussianSplattingModel.populate_modules` builds it
    (vanilla_gs.py:128-174) -- NOT a copy of the truth:
      kind="sfm":    a sparse point cloud with 8-bit colours, standing in for the COLMAP points
                     a nerfstudio-style dataset ships: `n_seed` surface points of the hidden scene
                     with `sfm_noise` of triangulation error; colour = the point's view-independent
                     colour.  means = the points, features_dc = RGB2SH(colour);
      kind="random": `random_init=True`: means uniform in a cube of edge `random_scale`
                     (the reference's 10 is for its unit-normalised real scenes; 3.4 encloses
                     this scene's radius-1.5 shells), features_dc = rand.
    Both: log-scales = log(mean distance to the 3 nearest seeds) on all three axes, random unit
    quaternions, opacity logit(0.1), higher SH bands zero.
    `knn`: who finds the neighbours -- "sklearn" (the reference's way, on the host) or "gpu"
    (`gs_fused.knn_mean_distance` on `device`, default the current CUDA device); same floor."""
    rng = np.random.default_rng(seed)
    K = S.num_sh_bases(sh_degree)
    f32 = np.float32
    if kind == "sfm":
        pick = np.sort(rng.choice(truth["means"].shape[0], n_seed, replace=False))
        means = truth["means"][pick] + rng.standard_normal((n_seed, 3)).astype(f32) * f32(sfm_noise)
        rgb8 = np.round(np.clip(truth["features_dc"][pick] * SH_C0 + 0.5, 0, 1) * 255.0)
        dc = ((rgb8 / 255.0) - 0.5) / SH_C0
    elif kind == "random":
        means = (rng.uniform(size=(n_seed, 3)) - 0.5) * random_scale
        dc = rng.uniform(size=(n_seed, 3))
    else:
        raise ValueError(f"unknown seed kind {kind!r}")
    means = means.astype(f32)
    if knn == "sklearn":
        avg = knn_mean_distance(means, 3)
    elif knn == "gpu":
        from gs_fused import knn_mean_distance as gpu_knn_mean_distance

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        avg = gpu_knn_mean_distance(torch.from_numpy(means).to(dev), 3).cpu().numpy()
    else:
        raise ValueError(f"unknown knn {knn!r}")
    avg = np.maximum(avg, 1e-7)
    return {
        "means": means,
        "scales": np.repeat(np.log(avg)[:, None], 3, axis=1).astype(f32),
        "quats": random_quats(n_seed, rng),
        "opacities": np.full((n_seed, 1), math.log(0.1 / 0.9), f32),
        "features_dc": dc.astype(f32),
        "features_rest": np.zeros((n_seed, K - 1, 3), f32),
    }


def means_lr(step: int, lr_init: float = 1.6e-4, lr_final: float = 1.6e-6, max_steps: int = 30000) -> float:
    """`ExponentialDecayScheduler` without warm-up, the schedule of the "means" group
    (configs/method_configs.py:98-104, engine/schedulers.py:94-135)."""
    t = min(max(step / max_steps, 0.0), 1.0)
    return math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


class GaussianParams(torch.nn.Module):
    split_sh = True  # evaluate SH from (features_dc, features_rest) without torch.cat
    fused_activations = True  # exp / normalise / sigmoid / view directions in one launch (gs_fused)
    filter_3d = None  # Mip-Splatting's 3D smoothing filter, float32 [N] (gs_fused.sampling_filter_3d); not a parameter

    def __init__(self, raw: Dict[str, np.ndarray], device):
        super().__init__()
        self.gauss = torch.nn.ParameterDict(
            {k: torch.nn.Parameter(torch.from_numpy(v).to(device)) for k, v in raw.items()})

    @property
    def num_points(self):
        return self.gauss["means"].shape[0]

    def param_list(self) -> List[torch.nn.Parameter]:
        return [self.gauss[k] for k in PARAM_NAMES]

    def replace(self, new: Dict[str, torch.Tensor]) -> None:
        """Install refined tensors as the model's parameters (vanilla_gs.py:440-447, 532)."""
        for k in PARAM_NAMES:
            if new[k] is not self.gauss[k]:
                self.gauss[k] = torch.nn.Parameter(new[k])

    def render(self, cam: CameraTensors, background, sh_degree_to_use: int, render_depth=False,
               retain_xys_grad=False, clamp_rgb=True, sh_exchange=None, caller_syncs=False, fused_depth=False,
               normalise_depth=True, rasterize_mode="classic", absgrad=False, render_normals=False,
               render_distortion=False, distortion_values=None):
        g = self.gauss
        if self.split_sh and g["features_dc"].is_cuda and g["features_rest"].shape[1] in (3, 8, 15):
            coeffs = (g["features_dc"], g["features_rest"])  # gs_fused.spherical_harmonics_split
        else:
            coeffs = torch.cat((g["features_dc"][:, None, :], g["features_rest"]), dim=1)
        if self.fused_activations and g["means"].is_cuda:
            from gs_fused import activate_gaussians

            scales, quats, opac, dirs = activate_gaussians(g["means"], g["scales"], g["quats"], g["opacities"],
                                                           cam.campos, filter_3d=self.filter_3d)
        elif self.filter_3d is not None:
            raise ValueError("filter_3d needs fused_activations on CUDA tensors: the filter is folded into the "
                             "activation kernels (gs_fused.apply_filter_3d is the torch form)")
        else:
            scales = torch.exp(g["scales"])
            quats = g["quats"] / g["quats"].norm(dim=-1, keepdim=True)
            opac, dirs = torch.sigmoid(g["opacities"]), None
        return render_view(g["means"], scales, quats, opac, coeffs, cam, background, sh_degree_to_use,
                           render_depth=render_depth, retain_xys_grad=retain_xys_grad, viewdirs=dirs,
                           clamp_rgb=clamp_rgb, caller_syncs=caller_syncs, fused_depth=fused_depth,
                           normalise_depth=normalise_depth, rasterize_mode=rasterize_mode, absgrad=absgrad,
                           **({"render_normals": True} if render_normals else {}),
                           **({"render_distortion": True, "distortion_values": distortion_values}
                              if render_distortion else {}),
                           sh_exchange=None if sh_exchange is None else (
                               sh_exchange, ("features_dc", "features_rest"), (g["features_dc"], g["features_rest"])))


def _gauss_window(size=11, sigma=1.5, device="cpu"):
    x = torch.arange(size, dtype=torch.float32, device=device) - size // 2
    g = torch.exp(-(x * x) / (2 * sigma * sigma))
    return g / g.sum()


def ssim(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """Mean SSIM of two [H,W,3] images in [0,1] (11x11 Gaussian window, sigma 1.5)."""
    a = img1.permute(2, 0, 1)[None]
    b = img2.permute(2, 0, 1)[None]
    w = _gauss_window(device=a.device)
    C = a.shape[1]
    kx = w.view(1, 1, 1, -1).repeat(C, 1, 1, 1)
    ky = w.view(1, 1, -1, 1).repeat(C, 1, 1, 1)
    blur = lambda t: F.conv2d(F.conv2d(t, kx, groups=C), ky, groups=C)
    mu1, mu2 = blur(a), blur(b)
    s11 = blur(a * a) - mu1 * mu1
    s22 = blur(b * b) - mu2 * mu2
    s12 = blur(a * b) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
    return m.mean()


def cogs_main_loss(pred: torch.Tensor, target: torch.Tensor, ssim_lambda: float) -> torch.Tensor:
    """`DepthGSModel.get_loss_dict`'s photometric terms op by op (depth_gs.py:441-462), quirk included: the SSIM is
    computed and then DROPPED -- `+self.config.ssim_lambda * simloss` stands on a line of its own (:447-448) -- so
    `main_loss` = (1 - ssim_lambda) * L1; `scale_reg` is tensor(0.) with the default config and the trainer adds
    the dict's values up (engine/trainer.py:497)."""
    Ll1 = torch.abs(target - pred).mean()
    simloss = 1 - ssim(target, pred)
    main_loss = (1 - ssim_lambda) * Ll1
    +ssim_lambda * simloss  # noqa: B018  (an expression statement, as in the source)
    scale_reg = torch.tensor(0.0).to(pred.device)
    return main_loss + scale_reg


def cogs_depth_l1(pred_depth: torch.Tensor, gt_depth: torch.Tensor) -> torch.Tensor:
    """`depth_l1` of depth_gs.py:531-538: |gt * (gt > 0) - pred * (gt > 0)|.mean() over ALL pixels, pred [H,W,1]
    squeezed; added to the loss with weight 1 (`depth_lambda` is declared twice in the config, :85 and :115, and
    read nowhere)."""
    depth_nonzero = gt_depth > 0
    pred = pred_depth.squeeze(-1)
    return torch.abs(gt_depth * depth_nonzero - pred * depth_nonzero).mean()


def psnr(a: torch.Tensor, b: torch.Tensor) -> float:
    return float(-10.0 * torch.log10(((a - b) ** 2).mean().clamp_min(1e-12)))


@dataclass
class TrainConfig:
    num_gaussians: int = 100_000
    width: int = 640
    height: int = 360
    num_views: int = 24
    iters: int = 300
    sh_degree: int = 3
    sh_degree_interval: int = 1000
    ssim_lambda: float = 0.2
    seed: int = 0
    log_every: int = 0
    eval_views: int = 4
    fused_loss: bool = True   # gs_fused.l1_ssim_loss (2 HIP kernels) instead of the torch-op SSIM
    fused_adam: bool = True   # gs_fused.FusedAdam: all six parameter groups in one HIP launch
    torch_fused_adam: bool = False  # (A/B) torch's own fused multi-tensor Adam instead
    split_sh: bool = True     # gs_fused.spherical_harmonics_split instead of torch.cat + spherical_harmonics
    fused_activations: bool = True  # gs_fused.activate_gaussians instead of exp / normalise / sigmoid / viewdirs
    # refinement (vanilla_gs.py:381-497).  Off: N stays fixed and iterations are comparable.
    densify: bool = False
    init_gaussians: Optional[int] = None  # the model starts from this many (coarser) Gaussians; default: all
    refine: Optional[object] = None       # gs_fused.RefineConfig; default: the reference's values
    refine_seed: int = 20240807           # broadcast by construction: the same on every rank
    # the densification strategy: "default" = the schedule above (with `densify`); "mcmc" = relocation of dead
    # Gaussians, growth by 5 % per refinement up to `mcmc.cap_max`, position noise after every optimiser step and the
    # opacity / scale regularisers in the loss (gs_fused.mcmc) -- no gradient statistics, no
    # opacity reset, no culling by size; `densify` and `refine` do not apply.  One GPU, CUDA only.
    strategy: str = "default"
    mcmc: Optional[object] = None         # gs_fused.MCMCConfig; default: gsplat's values
    # gs_fused.render_gaussians: the whole view as ONE autograd node (activations, projection, SH,
    # binning, compositing; densification statistics from its backward) instead of the op-by-op
    # call sequence of the models; use_graph: render -> loss -> backward replayed as one HIP graph
    fused_render: bool = False
    use_graph: bool = False
    # `rasterize_mode` of the toolkit's models (vanilla_gs.py:96-104): "classic", or "antialiased" -- the view
    # composites sigmoid(opacities) * compensation (:815-816).  Training views and `evaluate` alike, on all three step
    # bodies: the separate ops through pipeline.render_view, the one-node view and its graph through
    # `ViewSpec.rasterize_mode` (the product inside the projection kernels).  A model trained in one mode renders
    # wrongly in the other.
    rasterize_mode: str = "classic"
    # the camera model of every view: "pinhole", or "fisheye" -- the equidistant camera, pixel = f * theta, inside the
    # projection kernels (gs_fused.project_gaussians_fisheye).  The synthetic cameras then
    # span FISHEYE_FOV_X_DEG and the targets are rendered through the same model; with a `dataset` the model is the
    # dataset's.  Everything behind the projection is camera-blind.  The separate ops on one GPU: `fused_render`,
    # `use_graph`, `camera_optimizer`, `normal_consistency`, `filter_3d`, `prune_at` and a world size above 1 are
    # refused.
    camera_model: str = "pinhole"
    # absgrad (AbsGS; `absgrad` of gsplat / splatfacto): densification thresholds the accumulated norm of the per-pixel
    # |dL/dxy| sums instead of the signed screen-space gradient's, which cancels under a large Gaussian over texture.
    # Both step bodies: `ViewSpec.absgrad` on the one-node view and its graph, `rasterize_gaussians(absgrad=True)`
    # (`_rgbd` for co-gs' fused depth) on the separate ops.  The sums are larger than the signed norms, so
    # `densify_grad_thresh` wants raising with it; its default stays.  CUDA only.
    absgrad: bool = False
    # checkpoints in the toolkit's layout (harness/checkpoint.py; trainer.py:404-476)
    checkpoint_dir: Optional[str] = None
    save_every: int = 0                   # steps_per_save; 0 = never
    resume_from: Optional[str] = None     # a .ckpt file or a directory (latest step)
    scene: str = "ball"                   # blob_scene kind
    # where the model starts: "perturbed" = the hidden scene with noise on the means and washed-out
    # colour (optionally a subset, init_gaussians); "sfm" / "random" = the reference's own
    # initialisations from a sparse point cloud / uniformly random points (seed_model)
    init: str = "perturbed"
    seed_knn: str = "sklearn"             # seed_model's neighbour search: "sklearn" (host) or "gpu" (gs_fused.knn)
    means_lr_schedule: bool = False       # exponential decay of the "means" learning rate (method_configs.py:98-104)
    # data parallel only: reduce-scatter -> Adam on this rank's rows -> all-gather (parallel.ShardedAdam)
    # instead of all-reduce + Adam over every row on every rank
    sharded_adam: bool = False
    # data parallel only: "views" = the SH gradient is formed on every rank from the ranks' gathered 12-byte colour
    # cotangents (GradientExchange `sh_views`: 413 -> 161 B per Gaussian on the wire at 8 ranks), "dense" = every
    # gradient is all-reduced.  "views" needs the hook-driven exchange and the separate-ops render path.
    sh_exchange: str = "views"
    phase_every: int = 0                  # HIP events around render / loss / backward / optimizer on every k-th iteration
    phase_series: bool = False            # also return every sample (`phase_ms_series`: step, resolution divisor, 4 phases)
    scene_scale: tuple = (0.01, 0.06)     # range of the truth's Gaussian scales
    tex_cell: float = 0.04                # scene "objects": checker cell size in scene units
    scene_objects: tuple = (48, 0.18, 0.45)  # scene "objects": number of spheres, radius range
    cam_radius: float = 6.0               # radius of the camera orbit
    scene_extent: float = 1.5             # radius of the ball the scene fills
    # the reference's coarse-to-fine schedule (vanilla_gs.py:48-53, 646-669): the first `resolution_schedule`
    # iterations render at 1 / 2^num_downscales of the resolution, the next at half of that factor, ... (reference
    # defaults: 2 and 2000, i.e. 480x270 -> 960x540 -> 1920x1080 at steps 2000 and 4000; 0 here = full size from step 0)
    num_downscales: int = 0
    resolution_schedule: int = 2000
    # "random": a fresh `torch.rand(3)` background every training step (vanilla_gs.py:50, 688-690 -- the reference's
    # default), the ground truth then carries an alpha channel and is composited over it (:870-881, a
    # nerfstudio-synthetic / blender-style RGBA dataset); "fixed": scene.BACKGROUND, RGB ground truth
    background_color: str = "fixed"
    # block the host where the unchanged models do (pipeline.render_view `caller_syncs`): False, True (the two
    # read-backs of get_outputs, vanilla_gs.py:784,811) or "camera" (plus the intrinsics' .item() calls)
    caller_syncs: object = False
    # run the data-parallel machinery (gradient exchange, sharded Adam, statistics all-reduce) on a process group of
    # ONE rank too: every collective then goes through the backend as an identity -- how the RCCL code path is
    # exercised on a single-GPU box (tests/test_gpu_nccl.py)
    force_exchange: bool = False
    export_ply: Optional[str] = None      # write the trained model as `gs-export gaussian-splat` does (gs_io/ply.py)
    # random background only: the step's target as ONE kernel.  The reference downscales the RGBA ground truth and
    # composites it over the step's background every step (vanilla_gs.py:659-670, 870-881: a resize + four
    # elementwise kernels over the image).  The resized image does not depend on the step: alpha_ds * rgb_ds and
    # 1 - alpha_ds (both formed from the RESIZED RGBA, in the reference's order -- resizing does not commute with
    # the product) are cached per view and resolution and the step runs one `addcmul` with its background.
    # False: the reference's per-step sequence.
    fused_target: bool = True
    # "gaussian-splatting": GaussianSplattingModel (vanilla_gs.py).  "co-gs": DepthGSModel (depth_gs.py) -- BASELINE
    # config 5: the depth image is rasterised on the TRAINING path (`output_depth_during_training = True`, :99,
    # :345-363), the photometric loss is (1 - ssim_lambda) * L1 ONLY (:445-448: the `+ ssim_lambda * simloss` line is
    # an expression statement -- the SSIM is computed and dropped; followed as written), and from
    # `step > depth_loss_start_iteration` (:119-120, :472-476) the L1 between the rendered depth and the ground
    # truth's on the pixels with gt > 0 is ADDED UNWEIGHTED (:532-538; the trainer sums the dict,
    # engine/trainer.py:497 -- `depth_lambda` is never read).  Refinement, optimisers and schedules are the base
    # model's.  Set num_downscales = 0 and background_color = "random" for the reference's co-gs defaults (:51, :49).
    model: str = "gaussian-splatting"
    depth_loss_start_iteration: int = 6000
    use_depth_loss: bool = True
    # co-gs: RGB and depth from ONE compositing pass each way (gs_fused.rasterize_gaussians_rgbd) and the depth
    # normalisation + masked L1 in gs_fused.depth_l1_loss; False: the models' two `rasterize_gaussians` calls and
    # their torch ops (depth_gs.py:330-363, 531-538)
    fused_depth: bool = True
    # co-gs: the OPTIONAL loss terms of `DepthGSModelConfig` (depth_gs.py:93-139), every one off by default as in the
    # reference; restated in harness/cogs_losses.py (plain torch ops, outside the rasterizer's hot path).  With
    # `use_est_depth` the depth branch is the monocular-depth one (:477-531: local Pearson / scaled log-depth / TV
    # instead of `depth_l1`); `use_depth_regularization` adds the Canny-masked neighbour-mean term (:521-528) with the
    # mask and the term computed on the GPU (gs_fused.image2canny, gs_fused.depth_reg_loss) -- on the CPU it raises.
    use_scale_regularization: bool = False
    max_gauss_ratio: float = 10.0
    use_sparse_loss: bool = False
    sparse_lambda: float = 0.1
    use_est_depth: bool = False
    use_pearson_depth: bool = False
    local_patch_size: int = 128
    depth_loss_stop_iteration: int = 25_000
    use_scaled_est_depth: bool = False
    use_depth_regularization: bool = False
    using_tv_loss: bool = False
    # the three monocular-depth terms (local Pearson, scaled log-depth, TV) from gs_fused's heads on csrc/mono_depth.hip
    # instead of harness/cogs_losses.py's torch ops, the per-view mask multiplied in inside the kernels (DESIGN.md
    # section 4.11).  GPU only.  Off until its device time has been measured against the torch path.
    fused_mono_depth: bool = False
    # a per-view mask, as a dataset with object masks delivers one in `batch["mask"]`: "none"; "alpha" = the object's
    # silhouette (the hidden scene's accumulated opacity > 0.5); "box" = the central half of the image in both
    # directions (`view_masks`).  Both images -- and, for co-gs, both depth images -- are MULTIPLIED by it in front of
    # the loss (vanilla_gs.py:915-924, surface_gs.py:917-925, depth_gs.py:424-437): nothing is selected and the means
    # stay over all pixels.  vanilla_gs.py:919 and depth_gs.py:429 `.unsqueeze(-1)` the [H,W,1] mask and then
    # `repeat(1, 1, 3)` it, which cannot run on a four-dimensional tensor; surface_gs.py:921 multiplies the [H,W,1] mask
    # in directly and states what is meant -- that is what is followed, for all three models (and `gt_depth [H,W]`
    # takes the mask's one channel).  With the fused heads the multiplies happen inside the loss kernels
    # (gs_fused.*_loss(mask=...)); otherwise they are the reference's torch ops.
    mask: str = "none"
    # camera pose refinement (harness/camera_opt.py; gs_toolkit/cameras/camera_optimizers.py): "off", "SO3xR3" or "SE3".
    # A seventh parameter group -- `pose_adjustment` [num_views,6] under a plain torch.optim.Adam (eps 1e-15, the
    # `camera_opt` group of configs/method_configs.py:75-80: lr 1e-3 decaying exponentially to 5e-5 over 30 000 steps),
    # outside FusedAdam and refinement (it has no per-Gaussian rows) -- fed by the projection's camera gradients
    # (rasterizer.cuda.project_gaussians_backward_pose).  Runs the separate-ops path on one GPU: `fused_render`,
    # `use_graph`, a world size above 1 and CPU tensors are refused.  "off": nothing in the step changes.
    camera_optimizer: str = "off"
    camera_trans_l2_penalty: float = 1e-2
    camera_rot_l2_penalty: float = 1e-3
    camera_lr: float = 1e-3
    camera_lr_final: float = 5e-5
    camera_lr_max_steps: int = 30000
    # (translation sigma in scene units, rotation sigma in radians): the training cameras the trainer is given are
    # moved once by a rigid error drawn from `pose_noise_seed` (camera_opt.perturb_cameras), standing in for COLMAP's;
    # the ground truth stays rendered from the true poses, so a synthetic run has something to recover
    pose_noise: tuple = (0.0, 0.0)
    pose_noise_seed: int = 20241019
    # per-view bilateral grids (gs_fused.BilateralGrids; `use_bilateral_grid` of gsplat /
    # splatfacto, whose values the defaults are): an eighth parameter group -- one (grid_w, grid_h, grid_l) grid of 3x4
    # affine colour maps per training view under its own gs_fused.FusedAdam (eps 1e-15, `bilagrid_lr` warmed up from
    # 1 % over 1000 steps and decayed to 1 % over `iters`) -- through which the loss heads see the rendered image
    # (`grids.slice(out["rgb"], v)`; `out["rgb"]` stays the raw render), plus `bilagrid_tv_weight` times the grids'
    # total variation in the loss.  Absorbs what differs photometrically from view to view (exposure, white balance,
    # vignetting) instead of leaving it to floaters.  Evaluation renders without grids.  The separate ops and the
    # one-node view on one GPU: `use_graph`, a world size above 1 and CPU tensors are refused.  Off: nothing changes.
    bilateral_grid: bool = False
    bilagrid_shape: tuple = (16, 16, 8)
    bilagrid_lr: float = 2e-3
    bilagrid_tv_weight: float = 10.0
    # depth-normal consistency (gs_fused.normal_consistency_loss; what 2DGS, GOF, RaDe-GS, PGSR
    # and gsplat's `normal_lambda` add to colour-only training): every Gaussian's normal -- the axis of its smallest
    # scale, turned towards the camera (gs_fused.gaussian_normals) -- is composited into a normal image by a third
    # compositing pass, a second normal image is derived from the rendered depth inside the loss kernels, and
    # `normal_lambda` times the mean of 1 - alpha <normals, depth normals> joins the loss from
    # `step > normal_start_iteration`, with the view's mask.  The two defaults are gsplat's simple_trainer_2dgs.py
    # (`normal_lambda`, `normal_start_iter`) as recalled -- gsplat was not at hand to check them against; they are the
    # defaults of an opt-in, not claims.  A step that has the term renders the depth image as well (gaussian-splatting:
    # from the one RGB + depth compositing pass; co-gs renders it anyway and keeps the pass and the depth head it would
    # take without the option); a step before the start is the step it always was.  The separate ops on one GPU:
    # `fused_render`, `use_graph`, a world size above 1 and CPU tensors are refused.  Off: nothing changes.
    normal_consistency: bool = False
    normal_lambda: float = 0.05
    normal_start_iteration: int = 7000
    # depth distortion (gs_fused.depth_distortion; 2DGS's `lambda_dist`, gsplat's `distloss`):
    # `distortion_lambda` times the mean over all pixels of sum_i sum_j w_i w_j |z_i - z_j| joins the loss from
    # `step > distortion_start_iteration`, with the view's mask; it pulls the Gaussians along a ray onto one surface.
    # z is 2DGS's map of the depth, far / (far - near) (1 - near / depth), formed by torch ops on [N] so that its
    # gradient reaches the depths (and the means) by autograd; `distortion_near = distortion_far = None` passes the raw
    # depths.  The four defaults are 2DGS's (`lambda_dist` 100 as its README advises for bounded scenes, the term from
    # iteration 3000, near 0.2 and far 100 of its rasterizer) as recalled -- 2DGS was not at hand to check them against;
    # they are the defaults of an opt-in, not claims.  A step that has the term renders the depth image as well, as
    # with `normal_consistency`; a step before the start is the step it always was.  The separate ops on one GPU:
    # `fused_render`, `use_graph`, a world size above 1, CPU tensors and deterministic mode are refused.  Off: nothing
    # changes.
    depth_distortion: bool = False
    distortion_lambda: float = 100.0
    distortion_start_iteration: int = 3000
    distortion_near: Optional[float] = 0.2
    distortion_far: Optional[float] = 100.0
    # contribution-based pruning (gs_fused.ContributionStats / prune_mask; RadSplat,
    # LightGaussian, Mini-Splatting): after the optimiser step and any refinement of every step listed in `prune_at`,
    # the blend-weight statistics of the model over ALL training views (full resolution) are formed, the Gaussians the
    # rule scores lowest are removed -- `prune_keep`: the fraction that stays; `prune_threshold`: scores below it go;
    # neither: the rule's default threshold -- and the parameters, their Adam moments and the densification statistics
    # are swapped as after a refinement that changed N.  Rules: "max_weight" (default threshold 0.01), "weight_sum"
    # (needs one of the two), "dominant" (default threshold 1).  Steps after `stop_split_at` keep what was pruned: an
    # earlier one is densified again.  The separate ops, `fused_render` and `use_graph` on one GPU; a world size above
    # 1, `strategy="mcmc"`, `sharded_adam` and CPU tensors are refused.  `()`: nothing changes.
    prune_at: tuple = ()
    prune_rule: str = "max_weight"
    prune_threshold: Optional[float] = None
    prune_keep: Optional[float] = None
    # Mip-Splatting's 3D smoothing filter (gs_fused.filter3d): the model holds one float32 [N]
    # buffer `filter_3d` -- sqrt(0.2) over the largest fx / z of any training camera that sees the Gaussian, at the
    # resolution being fitted -- and every render folds it into the scales and the opacity (training, evaluation and
    # the contribution walk alike).  Recomputed before the first step, every `filter_3d_every` steps, right after
    # anything that changes the model's rows (a refinement, a `prune_at` step) and when the resolution schedule changes
    # factor; cameras as given (not the camera optimizer's).  Refinement, opacity reset and pruning work on the raw
    # parameters.  Saved in checkpoints; `export_ply` writes the baked model (gs_fused.bake_filter_3d).  The separate
    # ops on one GPU; `fused_render`, `use_graph`, `strategy="mcmc"`, a world size above 1, `fused_activations=False`
    # and CPU tensors are refused.  Off: nothing changes.
    filter_3d: bool = False
    filter_3d_every: int = 100
    # (sigma of the log-gain, sigma of the bias): every synthetic training target is multiplied once by a per-view,
    # per-channel gain exp(N(0, sigma_gain)) and shifted by N(0, sigma_bias), drawn from `view_exposure_seed`, standing
    # in for auto-exposure and white balance (a random background: the RGBA ground truth's colour is disturbed, its
    # alpha is not); evaluation keeps the true images.  Not with `dataset`.
    view_exposure: tuple = (0.0, 0.0)
    view_exposure_seed: int = 20241020
    # a dataset directory (or its transforms.json) instead of the hidden synthetic scene: read by
    # gs_io.dataset.load_dataset with the `dataset_*` fields below (the dataparser's config,
    # gs_toolkit_dataparser.py:36-67), uploaded as integers into a gs_fused.ImageCache (uint8 images, uint8 masks,
    # uint16 / uint8 depth: DESIGN.md section 4.15) and turned into each step's target by ONE kernel
    # (gs_fused.target_from_u8).  `num_views`, `width` and `height` then come from the dataset; the model starts from
    # the seed cloud as `populate_modules` does (vanilla_gs.py:126-174), or -- no cloud, or `dataset_random_init` --
    # from `dataset_num_random` uniform points in a cube of edge `dataset_random_scale`; `scene`, `init`, `mask`,
    # `pose_noise` and `fused_target` do not apply (masks and depth are used when the dataset has them).  One GPU.
    # After training the `dataset_eval_split` views are rendered and measured (`evaluate_dataset`; None: skipped).
    dataset: Optional[str] = None
    dataset_scale_factor: float = 1.0
    dataset_downscale_factor: Optional[int] = None
    dataset_orientation_method: str = "up"
    dataset_center_method: str = "poses"
    dataset_auto_scale_poses: bool = False
    dataset_eval_mode: str = "fraction"
    dataset_train_split_fraction: float = 0.9
    dataset_eval_interval: int = 8
    dataset_depth_unit_scale_factor: float = 1e-3
    dataset_random_init: bool = False
    dataset_num_random: int = 50000
    dataset_random_scale: float = 10.0
    dataset_eval_split: Optional[str] = "val"
    dataset_allow_fisheye: bool = False  # gs_io.dataset.load_dataset(allow_fisheye=...): read OPENCV_FISHEYE datasets


def quantise_depth_mm(depth: torch.Tensor) -> torch.Tensor:
    """A ground-truth depth image as the toolkit's dataset delivers it: a 16-bit PNG in millimetres read as
    `astype("float32") / 1000.0` (data/datasets/base_dataset.py:123-125); 0 = no measurement."""
    return torch.round(depth.clamp(0.0, 65.535) * 1000.0) / 1000.0


def _depth_segments_record(device):
    """What the compositing kernels do on tile grids too small to fill the chip (rasterizer.cuda.depth_segments)."""
    if device.type != "cuda":
        return None
    import rasterizer.cuda as _C

    segs, grid, least, fwd = _C._segment_knobs()[:4]
    return {"runs": segs, "runs_forward": min(segs, fwd) if fwd > 0 else segs, "tile_grids_up_to": grid,
            "lists_longer_than": least,
            "what": "on such grids the list of every split tile is cut into runs composited by their own waves "
                    "(gsr_rasterize_forward_seg / _backward_seg): results equal the single walk's to rounding"}


def _sh_views_backward_autograd():
    """CPU stand-in of gs_fused.sh_backward_views: the same sum over views through the autograd of whatever
    `harness.pipeline.spherical_harmonics` is (SH is linear in the coefficients)."""
    import harness.pipeline as HP

    def fn(degree, deg_use, means, campos_all, v_all, scale, split):
        n, K = means.shape[0], (degree + 1) ** 2
        coeffs = torch.zeros((n, K, 3), dtype=means.dtype, device=means.device, requires_grad=True)
        total = torch.zeros((n, K, 3), dtype=means.dtype, device=means.device)
        for r in range(campos_all.shape[0]):
            d = means - campos_all[r]
            d = d / d.norm(dim=-1, keepdim=True)
            (g,) = torch.autograd.grad(HP.spherical_harmonics(deg_use, d, coeffs), coeffs, v_all[r].reshape(n, 3))
            total += g
        total *= scale
        return (total[:, 0, :].contiguous(), total[:, 1:, :].contiguous()) if split else total

    return fn


def _check_config(cfg: TrainConfig) -> None:
    """The settings `train` refuses, before anything is rendered."""
    if cfg.background_color not in ("random", "fixed"):
        raise ValueError(f"unknown background_color {cfg.background_color!r}")
    if cfg.model not in ("gaussian-splatting", "co-gs"):
        raise ValueError(f"unknown model {cfg.model!r}")
    if cfg.model == "co-gs" and (cfg.fused_render or cfg.use_graph):
        raise ValueError("co-gs runs through the separate ops (fused_depth = one RGB + depth compositing pass)")
    if cfg.mask not in ("none", "alpha", "box"):
        raise ValueError(f"unknown mask {cfg.mask!r}")
    if cfg.rasterize_mode not in ("classic", "antialiased"):
        raise ValueError("Unknown rasterize_mode: %s" % cfg.rasterize_mode)
    if cfg.strategy not in ("default", "mcmc"):
        raise ValueError(f"unknown strategy {cfg.strategy!r}")
    if cfg.strategy == "mcmc":
        if cfg.refine is not None:
            raise ValueError("strategy='mcmc' takes its schedule from `mcmc` (gs_fused.MCMCConfig): `refine` "
                             "belongs to the default strategy and must stay None")
        if cfg.sharded_adam:
            raise ValueError("strategy='mcmc' does not run with `sharded_adam`: relocation rewrites whole rows of "
                             "both Adam moments in place")
    if cfg.camera_optimizer not in ("off", "SO3xR3", "SE3"):
        raise ValueError(f"unknown camera_optimizer {cfg.camera_optimizer!r}")
    if cfg.camera_optimizer != "off":
        if cfg.fused_render:
            raise ValueError("camera_optimizer needs the separate-ops path: the one-node view (fused_render, "
                             "gsr_view_backward) returns no camera gradient")
        if cfg.use_graph:
            raise ValueError("camera_optimizer needs the separate-ops path: a replayed HIP graph (use_graph) holds the "
                             "camera's matrices as constants of the capture")


def _check_camera_model(cfg: TrainConfig, world: int) -> None:
    """What `camera_model="fisheye"` refuses: everything that projects on its own."""
    if cfg.camera_model not in ("pinhole", "fisheye"):
        raise ValueError(f"unknown camera_model {cfg.camera_model!r}")
    if cfg.camera_model == "pinhole":
        return
    if cfg.fused_render:
        raise ValueError("camera_model='fisheye' does not run with fused_render: gsr_view_forward holds the pinhole projection")
    if cfg.use_graph:
        raise ValueError("camera_model='fisheye' does not run with use_graph: the captured view holds the pinhole projection")
    if cfg.camera_optimizer != "off":
        raise ValueError("camera_model='fisheye' does not run with camera_optimizer: the pose gradients differentiate the pinhole chain")
    if cfg.normal_consistency:
        raise ValueError("camera_model='fisheye' does not run with normal_consistency: depth_to_normal unprojects with pinhole intrinsics")
    if cfg.filter_3d:
        raise ValueError("camera_model='fisheye' does not run with filter_3d: its sampling rate is the pinhole's fx / z")
    if tuple(cfg.prune_at):
        raise ValueError("camera_model='fisheye' does not run with prune_at: contribution_stats projects on its own, through the pinhole")
    if world > 1:
        raise ValueError("camera_model='fisheye' runs on one GPU (world size 1): the data-parallel step was not taught the camera model")


def _check_absgrad(cfg: TrainConfig, device) -> None:
    if cfg.absgrad and device.type != "cuda":
        raise ValueError("absgrad needs CUDA tensors: the per-pixel sums come from the HIP compositing backward")


def _check_mcmc(cfg: TrainConfig, device, world: int) -> None:
    """What else `strategy="mcmc"` refuses, once the device and the world size are known."""
    if cfg.strategy != "mcmc":
        return
    if world > 1:
        raise ValueError("strategy='mcmc' runs on one GPU (world size 1): the draws and the position noise of a "
                         "data-parallel run are not coordinated")
    if device.type != "cuda":
        raise ValueError("strategy='mcmc' needs CUDA tensors: relocation, noise and regularisers are HIP kernels")


def _check_camera_optimizer(cfg: TrainConfig, device, world: int) -> None:
    """What else `camera_optimizer` refuses, once the device and the world size are known."""
    if cfg.camera_optimizer == "off":
        return
    if world > 1:
        raise ValueError("camera_optimizer runs on one GPU: the pose gradients of a data-parallel run are not exchanged")
    if device.type != "cuda":
        raise ValueError("camera_optimizer needs CUDA tensors: the camera gradients come from the HIP projection")


def _check_bilateral_grid(cfg: TrainConfig, device, world: int) -> None:
    """What `bilateral_grid` and `view_exposure` refuse, once the device and the world size are known."""
    if tuple(cfg.view_exposure) != (0.0, 0.0):
        if len(tuple(cfg.view_exposure)) != 2 or min(cfg.view_exposure) < 0:
            raise ValueError(f"view_exposure must be two non-negative sigmas (gain, bias), got {cfg.view_exposure!r}")
        if cfg.dataset is not None:
            raise ValueError("view_exposure disturbs the synthetic targets: it does not apply to `dataset`")
    if not cfg.bilateral_grid:
        return
    if cfg.use_graph:
        raise ValueError("bilateral_grid does not run under use_graph: the view index is a constant of a capture, and "
                         "the grids' gradient is written for one view")
    if world > 1:
        raise ValueError("bilateral_grid runs on one GPU (world size 1): the grids' gradients of a data-parallel run "
                         "are not exchanged")
    if device.type != "cuda":
        raise ValueError("bilateral_grid needs CUDA tensors: the slice and its backward are HIP kernels")
    from gs_fused.bilagrid import check_grid_shape

    if len(tuple(cfg.bilagrid_shape)) != 3:
        raise ValueError(f"bilagrid_shape must be (grid_w, grid_h, grid_l), got {cfg.bilagrid_shape!r}")
    check_grid_shape(*(int(s) for s in cfg.bilagrid_shape))


def _check_normal_consistency(cfg: TrainConfig, device, world: int) -> None:
    """What `normal_consistency` refuses, once the device and the world size are known."""
    if not cfg.normal_consistency:
        return
    if cfg.fused_render:
        raise ValueError("normal_consistency needs the separate-ops path: the one-node view (fused_render) composites "
                         "no normal image")
    if cfg.use_graph:
        raise ValueError("normal_consistency does not run under use_graph: the captured view holds no normal pass, and "
                         "the term joins at a step of the schedule")
    if world > 1:
        raise ValueError("normal_consistency runs on one GPU (world size 1): the normal pass's gradients of a "
                         "data-parallel run are not exchanged")
    if device.type != "cuda":
        raise ValueError("normal_consistency needs CUDA tensors: the normals and the loss head are HIP kernels")


def _check_depth_distortion(cfg: TrainConfig, device, world: int) -> None:
    """What `depth_distortion` refuses, once the device and the world size are known."""
    if not cfg.depth_distortion:
        return
    if cfg.fused_render:
        raise ValueError("depth_distortion needs the separate-ops path: the one-node view (fused_render) holds no "
                         "distortion walk")
    if cfg.use_graph:
        raise ValueError("depth_distortion does not run under use_graph: the captured view holds no distortion walk, "
                         "and the term joins at a step of the schedule")
    if world > 1:
        raise ValueError("depth_distortion runs on one GPU (world size 1): the walk's gradients of a data-parallel run "
                         "are not exchanged")
    if device.type != "cuda":
        raise ValueError("depth_distortion needs CUDA tensors: the walk is a pair of HIP kernels")
    if (cfg.distortion_near is None) != (cfg.distortion_far is None):
        raise ValueError("depth_distortion: distortion_near and distortion_far are both numbers or both None")
    if cfg.distortion_near is not None and not (0.0 < cfg.distortion_near < cfg.distortion_far):
        raise ValueError(f"depth_distortion: need 0 < distortion_near < distortion_far, got {cfg.distortion_near} and "
                         f"{cfg.distortion_far}")
    import sys

    mod = sys.modules.get("rasterizer.rasterize")  # (absent: CPU stand-ins, refused above)
    if mod is not None and mod.is_deterministic():
        raise ValueError("depth_distortion does not run in deterministic mode: the walk's backward sums with float "
                         "atomics")


def _check_prune(cfg: TrainConfig, device, world: int) -> None:
    """What `prune_at` refuses, once the device and the world size are known."""
    if not tuple(cfg.prune_at):
        return
    if world > 1:
        raise ValueError("prune_at runs on one GPU (world size 1): the ranks of a data-parallel run do not form the "
                         "statistics over all views together")
    if cfg.strategy == "mcmc":
        raise ValueError("prune_at does not run with strategy='mcmc': that strategy holds the model at its cap and "
                         "relocates what pruning would remove")
    if cfg.sharded_adam:
        raise ValueError("prune_at does not run with sharded_adam: pruning moves whole rows of both Adam moments")
    if device.type != "cuda":
        raise ValueError("prune_at needs CUDA tensors: the contribution walk is a HIP kernel")
    if cfg.prune_keep is not None and cfg.prune_threshold is not None:
        raise ValueError("prune_at: give prune_keep or prune_threshold, not both")
    from gs_fused.contribution import RULES

    if cfg.prune_rule not in RULES:
        raise ValueError(f"prune_at: unknown prune_rule {cfg.prune_rule!r}; known: {sorted(RULES)}")
    if cfg.prune_keep is None and cfg.prune_threshold is None and RULES[cfg.prune_rule] is None:
        raise ValueError(f"prune_at: prune_rule {cfg.prune_rule!r} has no default threshold; give prune_keep or "
                         f"prune_threshold")
    if cfg.prune_keep is not None and not (0.0 < cfg.prune_keep <= 1.0):
        raise ValueError(f"prune_at: prune_keep must be a fraction in (0, 1], got {cfg.prune_keep}")


def _check_filter_3d(cfg: TrainConfig, device, world: int) -> None:
    """What `filter_3d` refuses, once the device and the world size are known."""
    if not cfg.filter_3d:
        return
    if cfg.fused_render:
        raise ValueError("filter_3d needs the separate-ops path: the one-node view (fused_render) runs the unfiltered "
                         "activations inside its single call")
    if cfg.use_graph:
        raise ValueError("filter_3d does not run under use_graph: the captured view holds the unfiltered activations")
    if cfg.strategy == "mcmc":
        raise ValueError("filter_3d does not run with strategy='mcmc': relocation and the opacity regulariser read the "
                         "raw opacities, not the filtered ones")
    if world > 1:
        raise ValueError("filter_3d runs on one GPU (world size 1): the ranks of a data-parallel run do not agree on "
                         "when the buffer is recomputed")
    if not cfg.fused_activations:
        raise ValueError("filter_3d needs fused_activations: the filter is folded into the activation kernels")
    if device.type != "cuda":
        raise ValueError("filter_3d needs CUDA tensors: the sampling pass and the filtered activations are HIP kernels")
    if int(cfg.filter_3d_every) < 1:
        raise ValueError(f"filter_3d: filter_3d_every must be a positive number of steps, got {cfg.filter_3d_every}")


class Filter3DState:
    """`TrainConfig.filter_3d`: the camera tables of the sampling pass, one per factor of the resolution schedule (the
    training cameras as given), and when the model's buffer was last recomputed."""

    def __init__(self, cfg: TrainConfig, data, device):
        from gs_fused import filter_cameras

        self.tables = {d: filter_cameras(cams, device) for d, cams in data.cams_by_d.items()}
        self.every = int(cfg.filter_3d_every)
        self.d, self.at, self.updates = None, None, 0

    def update(self, model, d: int, step: int) -> None:
        from gs_fused import sampling_filter_3d

        model.filter_3d = sampling_filter_3d(model.gauss["means"].detach(), self.tables[d])
        self.d, self.at = d, step
        self.updates += 1

    def start(self, cfg: TrainConfig, model, start_step: int) -> None:
        """Before the first step (and the evaluation in front of it): a buffer restored from a checkpoint stays -- it
        is what the interrupted run held at this step -- anything else is computed at this step's factor."""
        f = model.filter_3d
        if f is not None and f.shape[0] == model.num_points and start_step > 0:
            self.d = downscale_factor(start_step - 1, cfg.num_downscales, cfg.resolution_schedule)
        else:
            self.update(model, downscale_factor(start_step, cfg.num_downscales, cfg.resolution_schedule), start_step)

    def due(self, step: int, d: int) -> bool:
        return d != self.d or (step % self.every == 0 and step != self.at)


def export_parameters(model: GaussianParams, bake_filter: bool = True) -> Dict[str, np.ndarray]:
    """The six raw parameter arrays `gs_io.write_gaussian_ply` takes; with a 3D filter on the model (and `bake_filter`)
    the log-scales and opacity logits are the baked ones: the file rendered without a filter is the filtered model."""
    out = {k: model.gauss[k].detach() for k in PARAM_NAMES}
    if bake_filter and model.filter_3d is not None:
        from gs_fused import bake_filter_3d

        out["scales"], out["opacities"] = bake_filter_3d(out["scales"], out["opacities"], model.filter_3d)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _params(model: GaussianParams) -> Dict[str, torch.nn.Parameter]:
    return {k: model.gauss[k] for k in PARAM_NAMES}


def _zero_grads(model: GaussianParams) -> None:
    for p in model.param_list():
        p.grad = None


def _hidden_scene(cfg: TrainConfig) -> Dict[str, np.ndarray]:
    return blob_scene(cfg.num_gaussians, seed=cfg.seed, sh_degree=cfg.sh_degree, kind=cfg.scene,
                      scale_lo=cfg.scene_scale[0], scale_hi=cfg.scene_scale[1], tex_cell=cfg.tex_cell,
                      objects=cfg.scene_objects, extent=cfg.scene_extent)


@dataclass
class TrainData:
    """What the toolkit's datamanager would deliver, rendered from the hidden scene."""
    factors: List[int]                        # the downscale factors of the coarse-to-fine schedule, 1 included
    cams_by_d: Dict[int, list]                # factor -> one CameraTensors per view
    bg: torch.Tensor                          # scene.BACKGROUND: evaluation, and training unless the background is random
    gt: List[torch.Tensor]                    # [H,W,3] per view, over `bg`
    gt_rgba: Optional[List[torch.Tensor]]     # random background: [H,W,4] per view, straight colour
    gt_depth: Optional[List[torch.Tensor]]    # co-gs: [H,W] per view, millimetre steps, 0 = no measurement
    masks: Optional[List[torch.Tensor]]       # TrainConfig.mask: [H,W,1] per view
    cams_np: Optional[list] = None            # the training cameras as given (scene.Camera; `pose_noise` applied)
    true_cams_np: Optional[list] = None       # the cameras the ground truth was rendered from
    cache: Optional[object] = None            # `TrainConfig.dataset`: the gs_fused.ImageCache `gt` / `gt_depth` / `masks` read
    dataset: Optional[object] = None          # ... and the gs_io.dataset.Dataset it was filled from (the training split)
    gt_train: Optional[List[torch.Tensor]] = None  # `view_exposure`: the disturbed targets the steps fit (`gt` stays true)
    gt_rgba_train: Optional[List[torch.Tensor]] = None  # ... and, random background, the disturbed [H,W,4] images
    exposure: Optional[Dict] = None           # ... and the per-view gains and biases that made them ([V,3] lists)


def disturb_exposure(gt: List[torch.Tensor], sigma_gain: float, sigma_bias: float, seed: int):
    """-> (targets, {"gain", "bias"}): every view times a per-channel gain exp(N(0, sigma_gain)) plus a per-channel
    bias N(0, sigma_bias), drawn on the host from `seed` (the same on every device)."""
    rng = np.random.default_rng(seed)
    gain = np.exp(rng.standard_normal((len(gt), 3)) * sigma_gain).astype(np.float32)
    bias = (rng.standard_normal((len(gt), 3)) * sigma_bias).astype(np.float32)
    out = [(g * torch.from_numpy(gain[v]).to(g.device) + torch.from_numpy(bias[v]).to(g.device)).contiguous()
           for v, g in enumerate(gt)]
    return out, {"gain": gain.tolist(), "bias": bias.tolist()}


class _CacheViews:
    """`TrainData.gt` / `gt_depth` / `masks` of a dataset: indexed like the lists of tensors `make_data` renders, formed
    from the integer cache when asked for (full size)."""

    def __init__(self, n: int, get):
        self.n, self.get = n, get

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, v: int) -> torch.Tensor:
        return self.get(int(v))


def dataset_config(cfg: TrainConfig) -> Dict:
    """The keyword arguments of gs_io.dataset.load_dataset from the `dataset_*` fields."""
    return dict(scale_factor=cfg.dataset_scale_factor, downscale_factor=cfg.dataset_downscale_factor,
                orientation_method=cfg.dataset_orientation_method, center_method=cfg.dataset_center_method,
                auto_scale_poses=cfg.dataset_auto_scale_poses, eval_mode=cfg.dataset_eval_mode,
                train_split_fraction=cfg.dataset_train_split_fraction, eval_interval=cfg.dataset_eval_interval,
                depth_unit_scale_factor=cfg.dataset_depth_unit_scale_factor,
                **({"allow_fisheye": True} if cfg.dataset_allow_fisheye else {}))


def upload_dataset(ds, device):
    """A split's files -> gs_fused.ImageCache: every file read into its integer dtype and copied to the device once
    (pinned memory, one `copy_` per file, no float copy on either side)."""
    from gs_fused import ImageCache

    n = len(ds)
    return ImageCache([ds.image(i) for i in range(n)],
                      None if ds.mask_filenames is None else [ds.mask(i) for i in range(n)],
                      None if ds.depth_filenames is None else [ds.depth(i) for i in range(n)],
                      depth_unit=ds.depth_unit, device=device)


def _schedule_factors(cfg: TrainConfig) -> List[int]:
    return sorted({downscale_factor(s_, cfg.num_downscales, cfg.resolution_schedule)
                   for s_ in range(0, max(cfg.iters, 1), max(min(cfg.resolution_schedule, cfg.iters), 1))} | {1})


def make_dataset_data(cfg: TrainConfig, device) -> TrainData:
    """`make_data` for `TrainConfig.dataset`: the training split's cameras, and its images, masks and depth as an
    integer cache on the device."""
    from gs_io.dataset import load_dataset

    ds = load_dataset(cfg.dataset, "train", **dataset_config(cfg))
    if len(ds) == 0:
        raise ValueError(f"dataset {cfg.dataset!r}: the training split is empty")
    if cfg.model == "co-gs" and ds.depth_filenames is None:
        raise ValueError(f"dataset {cfg.dataset!r}: model 'co-gs' needs depth_path in every frame")
    cache = upload_dataset(ds, device)
    cams_np = ds.cameras
    factors = _schedule_factors(cfg)
    cams_by_d = {d: [CameraTensors.from_numpy(rescale_camera(c, d), device) for c in cams_np] for d in factors}
    bg = torch.tensor(S.BACKGROUND, device=device)
    n = len(ds)
    return TrainData(factors, cams_by_d, bg, _CacheViews(n, lambda v: cache.target(v, 1, bg)), None,
                     None if cache.depths is None else _CacheViews(n, lambda v: cache.depth(v, 1)),
                     None if cache.masks is None else _CacheViews(n, lambda v: cache.mask(v, 1)),
                     cams_np, None, cache, ds)


def make_data(cfg: TrainConfig, device) -> TrainData:
    fov = {} if cfg.camera_model == "pinhole" else {"fov_x_deg": FISHEYE_FOV_X_DEG}
    true_np = cams_np = orbit_cameras(cfg.num_views, cfg.width, cfg.height, radius=cfg.cam_radius,
                                      model=cfg.camera_model, **fov)
    true_cams = cams = [CameraTensors.from_numpy(c, device) for c in cams_np]
    if tuple(cfg.pose_noise) != (0.0, 0.0):  # the trainer's cameras carry a pose error; the images do not
        from .camera_opt import perturb_cameras

        cams_np = perturb_cameras(true_np, cfg.pose_noise[0], cfg.pose_noise[1], cfg.pose_noise_seed)
        cams = [CameraTensors.from_numpy(c, device) for c in cams_np]
    # the coarse-to-fine schedule's cameras, one set per downscale factor
    factors = _schedule_factors(cfg)
    cams_by_d = {d: (cams if d == 1 else [CameraTensors.from_numpy(rescale_camera(c, d), device) for c in cams_np])
                 for d in factors}
    bg = torch.tensor(S.BACKGROUND, device=device)
    truth = GaussianParams(_hidden_scene(cfg), device)
    with torch.no_grad():
        if cfg.background_color == "random":
            # RGBA ground truth with straight (un-premultiplied) colour, as a blender-style dataset stores it:
            # rendered over black, C = sum c_i a_i T_i and A = 1 - T, colour = C / A
            zero = torch.zeros(3, device=device)
            gt_rgba, gt = [], []
            for c in true_cams:
                o = truth.render(c, zero, cfg.sh_degree, clamp_rgb=False)
                a = o["alpha"]
                gt_rgba.append(torch.cat((torch.where(a > 0, o["rgb"] / a.clamp_min(1e-12), torch.zeros_like(o["rgb"]))
                                          .clamp(0, 1), a), dim=-1))
                gt.append(composite_with_background(gt_rgba[-1], bg))  # evaluation: over the fixed background
        else:
            gt_rgba = None
            gt = [truth.render(c, bg, cfg.sh_degree)["rgb"] for c in true_cams]
        gt_depth = None
        if cfg.model == "co-gs":
            # the sensor's depth image: z-depth of the hidden scene where it covers the pixel, 0 (= no measurement,
            # masked out by `gt_depth > 0`) elsewhere, in millimetre steps like the dataset's 16-bit PNGs
            gt_depth = []
            for c in true_cams:
                o = truth.render(c, torch.zeros(3, device=device), cfg.sh_degree, render_depth=True,
                                 fused_depth=device.type == "cuda")
                gt_depth.append(quantise_depth_mm(torch.where(o["alpha"] > 0.5, o["depth"], torch.zeros_like(o["depth"]))
                                                  [..., 0]).contiguous())
        masks = None
        if cfg.mask != "none":
            masks = view_masks(cfg.mask, cfg.height, cfg.width,
                               [truth.render(c, bg, cfg.sh_degree)["alpha"] if cfg.mask == "alpha" else None
                                for c in true_cams], device)
    data = TrainData(factors, cams_by_d, bg, gt, gt_rgba, gt_depth, masks, cams_np, true_np)
    if tuple(cfg.view_exposure) != (0.0, 0.0):  # the trainer's targets carry a photometric error; evaluation's do not
        sg, sb = cfg.view_exposure
        data.gt_train, data.exposure = disturb_exposure(gt, sg, sb, cfg.view_exposure_seed)
        if gt_rgba is not None:  # random background: the straight colour is disturbed, the alpha is not (same draws)
            colour, _ = disturb_exposure([g[..., :3] for g in gt_rgba], sg, sb, cfg.view_exposure_seed)
            data.gt_rgba_train = [torch.cat((c, g[..., 3:]), dim=-1) for c, g in zip(colour, gt_rgba)]
    return data


def evaluate(model: GaussianParams, data: TrainData, cfg: TrainConfig, cams=None) -> Dict[str, Optional[float]]:
    """Means over `eval_views` full-size views: "psnr"; "psnr_masked" over the pixels with mask > 0.5 (with a mask);
    "depth_err", mean |rendered depth - gt depth| over the measured pixels (co-gs).  `cams`: the full-size cameras to
    render from (default: the ones the trainer was given; with a camera optimizer, the corrected ones)."""
    cogs, masked = cfg.model == "co-gs", data.masks is not None
    cams, bg, gt = data.cams_by_d[1] if cams is None else cams, data.bg, data.gt
    ps, pm, de = [], [], []
    with torch.no_grad():
        for i in np.linspace(0, cfg.num_views - 1, cfg.eval_views).astype(int):
            if cogs:
                o = model.render(cams[i], bg, cfg.sh_degree, render_depth=True, fused_depth=bg.is_cuda,
                                 rasterize_mode=cfg.rasterize_mode)
            else:
                o = model.render(cams[i], bg, cfg.sh_degree, rasterize_mode=cfg.rasterize_mode)
            ps.append(psnr(o["rgb"], gt[i]))
            if masked:
                sel = data.masks[i][..., 0] > 0.5
                pm.append(psnr(o["rgb"][sel], gt[i][sel]))
            if cogs:
                m = data.gt_depth[i] > 0
                de.append(float((o["depth"][..., 0] - data.gt_depth[i]).abs()[m].mean()) if bool(m.any()) else 0.0)
    return {"psnr": float(np.mean(ps)), "psnr_masked": float(np.mean(pm)) if masked else None,
            "depth_err": float(np.mean(de)) if cogs else None}


def evaluate_dataset(model: GaussianParams, dataset_or_cache, cfg: TrainConfig, split: str = "val", device=None) -> Dict:
    """Held-out evaluation as the toolkit's `get_average_eval_image_metrics(get_std=True)` reports it
    (pipelines/base_pipeline.py): every view of `split` rendered at full size over the fixed background, the ground
    truth formed by gs_fused.target_from_u8 (d = 1, same background).  Per image: PSNR = 10 log10(1 / mse) over all
    elements, SSIM from the fused head (`l1_ssim_loss(..., return_terms=True)`), the view's rays per second and frames
    per second (wall clock around the render, synchronised).  -> means and, as `torch.std_mean` gives it (unbiased; 0
    for one image), `*_std`, plus the per-image lists.  LPIPS is left out: no network weights ship with this package.
    `dataset_or_cache`: a path, a gs_io.dataset.Dataset of that split, or a (Dataset, ImageCache) pair."""
    from gs_fused import l1_ssim_loss
    from gs_io.dataset import Dataset, load_dataset

    device = model.gauss["means"].device if device is None else device
    if isinstance(dataset_or_cache, (tuple, list)):
        ds, cache = dataset_or_cache
    else:
        ds = dataset_or_cache if isinstance(dataset_or_cache, Dataset) else \
            load_dataset(dataset_or_cache, split, **dataset_config(cfg))
        cache = upload_dataset(ds, device) if len(ds) else None
    if len(ds) == 0:
        raise ValueError(f"the {split!r} split holds no views")
    bg = torch.tensor(S.BACKGROUND, device=device)
    cogs = cfg.model == "co-gs"
    per = {"psnr": [], "ssim": [], "num_rays_per_sec": [], "fps": []}
    with torch.no_grad():
        for v, cam_np in enumerate(ds.cameras):
            cam = CameraTensors.from_numpy(cam_np, device)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            if cogs:
                o = model.render(cam, bg, cfg.sh_degree, render_depth=True, fused_depth=True,
                                 rasterize_mode=cfg.rasterize_mode)
            else:
                o = model.render(cam, bg, cfg.sh_degree, rasterize_mode=cfg.rasterize_mode)
            torch.cuda.synchronize(device)
            dt = time.perf_counter() - t0
            rgb, gt = o["rgb"].contiguous(), cache.target(v, 1, bg)
            mse = ((rgb - gt) ** 2).mean()
            per["psnr"].append(float(10.0 * torch.log10(1.0 / mse)))
            per["ssim"].append(float(l1_ssim_loss(rgb, gt, cfg.ssim_lambda, return_terms=True)[2]))
            per["num_rays_per_sec"].append(cam.height * cam.width / dt)
            per["fps"].append(1.0 / dt)
    out = {}
    for k, vals in per.items():
        t = torch.tensor(vals, dtype=torch.float64)
        std, mean = torch.std_mean(t) if len(vals) > 1 else (torch.tensor(0.0), t.mean())
        out[k], out[f"{k}_std"] = float(mean), float(std)
    out.update({f"{k}_per_image": v for k, v in per.items()})
    out.update({"num_images": len(ds), "split": split, "lpips": None,
                "lpips_note": "not computed: no network weights ship with this package"})
    return out


def dataset_initial_model(cfg: TrainConfig, ds, device) -> GaussianParams:
    """`populate_modules` (vanilla_gs.py:126-174) on the dataset's seed cloud: means = the points, DC colour =
    RGB2SH(rgb / 255), higher bands zero, log-scales = log(mean distance to the 3 nearest seeds) on all axes
    (gs_fused.initial_log_scales on the GPU), random unit quaternions, opacity logit(0.1).  Without a cloud, or with
    `dataset_random_init`: `dataset_num_random` points uniform in a cube of edge `dataset_random_scale`, DC = rand."""
    rng = np.random.default_rng(cfg.seed + 1)
    f32 = np.float32
    if ds.points3D_xyz is not None and len(ds.points3D_xyz) > 0 and not cfg.dataset_random_init:
        means = np.ascontiguousarray(ds.points3D_xyz, f32)
        dc = ((ds.points3D_rgb.astype(f32) / f32(255.0)) - f32(0.5)) / f32(SH_C0)
    else:
        means = ((rng.uniform(size=(cfg.dataset_num_random, 3)) - 0.5) * cfg.dataset_random_scale).astype(f32)
        dc = rng.uniform(size=(cfg.dataset_num_random, 3)).astype(f32)
    n = means.shape[0]
    if device.type == "cuda":
        from gs_fused import initial_log_scales

        scales = initial_log_scales(torch.from_numpy(means).to(device), 3, floor=1e-7).cpu().numpy()
    else:
        scales = np.repeat(np.log(np.maximum(knn_mean_distance(means, 3), 1e-7))[:, None], 3, axis=1).astype(f32)
    raw = {"means": means, "scales": scales.astype(f32), "quats": random_quats(n, rng),
           "opacities": np.full((n, 1), math.log(0.1 / 0.9), f32), "features_dc": dc.astype(f32),
           "features_rest": np.zeros((n, S.num_sh_bases(cfg.sh_degree) - 1, 3), f32)}
    model = GaussianParams(raw, device)
    model.split_sh, model.fused_activations = cfg.split_sh, cfg.fused_activations
    return model


def initial_model(cfg: TrainConfig, device) -> GaussianParams:
    raw = _hidden_scene(cfg)
    rng = np.random.default_rng(cfg.seed + 1)
    if cfg.init in ("sfm", "random"):
        raw = seed_model(raw, cfg.init_gaussians or 50_000, cfg.init, cfg.seed + 1, cfg.sh_degree,
                         knn=cfg.seed_knn, device=device if cfg.seed_knn == "gpu" else None)
    else:
        # the model starts from the truth with perturbed geometry / washed-out colour
        raw["means"] += rng.standard_normal(raw["means"].shape).astype(np.float32) * 0.01
        raw["features_dc"] *= 0.3
        raw["features_rest"] *= 0.0
        raw["opacities"] -= 0.5
    if cfg.init == "perturbed" and cfg.init_gaussians is not None and cfg.init_gaussians < cfg.num_gaussians:
        # a coarser start for densification to refine: a subset, each Gaussian standing in for
        # num/init of the truth's (scales grown by the cube root of that ratio)
        keep = np.sort(rng.choice(cfg.num_gaussians, cfg.init_gaussians, replace=False))
        raw = {k: np.ascontiguousarray(v[keep]) for k, v in raw.items()}
        raw["scales"] += np.float32(math.log(cfg.num_gaussians / cfg.init_gaussians) / 3.0)
    model = GaussianParams(raw, device)
    model.split_sh, model.fused_activations = cfg.split_sh, cfg.fused_activations
    return model


def make_optimisers(cfg: TrainConfig, model: GaussianParams, device, dp: bool):
    """-> (optims, sharded): Adam per parameter group with the reference's learning rates -- one optimiser over six
    groups with `fused_adam` on the GPU, six optimisers otherwise -- or, data parallel with `sharded_adam`, no
    optimiser here and a `parallel.ShardedAdam` that runs one over this rank's rows."""
    fused = cfg.fused_adam and device.type == "cuda"

    def adam(groups):
        if fused:
            from gs_fused import FusedAdam

            return FusedAdam(groups, eps=1e-15)
        return torch.optim.Adam(groups, eps=1e-15)

    if cfg.sharded_adam and dp:
        from .parallel import ShardedAdam

        return {}, ShardedAdam(_params(model), LRS, adam, force=cfg.force_exchange)
    if not fused:
        return {k: torch.optim.Adam([model.gauss[k]], lr=lr, eps=1e-15) for k, lr in LRS.items()}, None
    groups = [{"params": [model.gauss[k]], "lr": lr} for k, lr in LRS.items()]
    return {"all": torch.optim.Adam(groups, eps=1e-15, fused=True) if cfg.torch_fused_adam else adam(groups)}, None


def make_exchange(cfg: TrainConfig, model: GaussianParams, sharded: bool, dp: bool):
    """-> (exchange, sh_views): the gradient exchange, attached -- started per parameter from autograd hooks (overlaps
    the rest of the backward), SH bands above the warm-up degree left out -- and whether the SH gradient travels as
    the ranks' gathered colour cotangents (`TrainConfig.sh_exchange`)."""
    exchange = GradientExchange(_params(model), average=True, force=cfg.force_exchange)
    # a replayed HIP graph fires no hooks, and a hook during capture would put a collective INTO the
    # graph (and reduce every gradient twice): under use_graph the exchange is started after the replay
    exchange.use_hooks = not cfg.use_graph
    if sharded:
        exchange.enabled = False  # the gradients travel by reduce-scatter inside ShardedAdam.step()
    exchange.attach()
    # (through the one native call per view as well, but not under graph replay: no hooks there)
    sh_views = dp and cfg.sh_exchange == "views" and exchange.enabled and exchange.use_hooks
    if sh_views and not model.gauss["means"].is_cuda:
        exchange.sh_views_backward = _sh_views_backward_autograd()  # no native kernel here: autograd of the SH op
    return exchange, sh_views


def loss_heads(cfg: TrainConfig, device):
    """-> (photo, depth, fused_clamp).  `photo(pred, target, mask=None)`: (1 - lambda) L1 + lambda (1 - SSIM), for co-gs
    (1 - lambda) L1 (`cogs_main_loss`).  `depth(out, gt_depth, mask=None)`: co-gs' depth L1 on the render's outputs,
    None for the base model.  A mask is multiplied into both images (vanilla_gs.py:915-924, depth_gs.py:424-437).  With
    `fused_loss` on the GPU the heads are gs_fused's kernels, the mask goes into them, and so does the clamp of the
    rendered image at 1 (vanilla_gs.py:857): `fused_clamp`, the render then leaves it out."""
    cogs, lam = cfg.model == "co-gs", cfg.ssim_lambda
    fused = bool(cfg.fused_loss and device.type == "cuda")
    if fused:
        from gs_fused import depth_l1_loss, l1_loss, l1_ssim_loss

        if cogs:
            def photo(pred, target, mask=None):
                return l1_loss(pred, target, 1.0 - lam, clamp_pred=True, mask=mask)
        else:
            def photo(pred, target, mask=None):
                return l1_ssim_loss(pred, target, lam, clamp_pred=True, mask=mask)
    else:
        def photo(pred, target, mask=None):
            if mask is not None:  # the reference's two multiplies
                pred, target = pred * mask, target * mask
            if cogs:
                return cogs_main_loss(pred, target, lam)
            return (1 - lam) * (pred - target).abs().mean() + lam * (1 - ssim(pred, target))

    if not cogs:
        depth = None
    elif fused and cfg.fused_depth:
        def depth(out, gt_depth, mask=None):
            return depth_l1_loss(out["depth_acc"], out["alpha"], gt_depth, mask=mask)
    else:
        def depth(out, gt_depth, mask=None):
            if mask is None:
                return cogs_depth_l1(out["depth"], gt_depth)
            return cogs_depth_l1(out["depth"] * mask, gt_depth * mask[..., 0])
    return photo, depth, fused


class StepInputs:
    """A step's background (vanilla_gs.py:688-690), ground truth (:859-868 downscaled, :870-881 composited over the
    step's background) and mask for a view and a downscale factor.  What does not depend on the step is cached per
    (view, factor): the resized mask, and with `fused_target` the two planes the target is one `addcmul` of."""

    def __init__(self, cfg: TrainConfig, data: TrainData, device, rank: int = 0):
        self.data, self.device, self.fused_target = data, device, cfg.fused_target
        self.cache, self.graph_targets = data.cache, bool(cfg.use_graph)
        random_bg = cfg.background_color == "random"
        # (the reference seeds every rank differently, scripts/train.py:54: the backgrounds differ per rank, as there)
        self.bg_gen = torch.Generator(device=device).manual_seed(cfg.seed + 977 * (rank + 1)) if random_bg else None
        self.bg_static = data.bg.clone() if (random_bg and cfg.use_graph) else None  # a replayed graph reads it here
        self.target_cache = {}  # (view, factor) -> (resized alpha * rgb [h,w,3], resized 1 - alpha [h,w,1])
        self.mask_cache = {}  # (view, factor) -> resized mask [h,w,1]

    def __call__(self, v: int, d: int):
        """-> (background [3], target [h,w,3], mask [h,w,1] or None); draws the step's background."""
        data = self.data
        if self.cache is not None:
            return self._from_cache(v, d)
        if self.bg_gen is None:
            bg, target = data.bg, downscale_image((data.gt if data.gt_train is None else data.gt_train)[v], d)
        else:
            bg = torch.rand(3, device=self.device, generator=self.bg_gen)
            rgba = data.gt_rgba if data.gt_rgba_train is None else data.gt_rgba_train
            if self.fused_target:
                planes = self.target_cache.get((v, d))
                if planes is None:
                    small = downscale_image(rgba[v], d)
                    a = small[..., 3:4]
                    planes = self.target_cache[(v, d)] = ((a * small[..., :3]).contiguous(), (1 - a).contiguous())
                target = torch.addcmul(planes[0], planes[1], bg)
            else:
                target = composite_with_background(downscale_image(rgba[v], d), bg)
            if self.bg_static is not None:
                self.bg_static.copy_(bg)
                bg = self.bg_static
        mask = None
        if data.masks is not None:
            mask = self.mask_cache.get((v, d))
            if mask is None:
                mask = self.mask_cache[(v, d)] = downscale_mask(data.masks[v], d).contiguous()
        return bg, target, mask


    def _from_cache(self, v: int, d: int):
        """The same three from the integer cache: the background stays the device tensor it is (never read back), the
        target is one kernel over the uint8 image, and under `use_graph` that kernel writes the graph's static target
        itself (a gs_fused.DeferredTarget: nothing is allocated or copied)."""
        cache = self.cache
        if self.bg_gen is None:
            bg = self.data.bg
        else:
            bg = torch.rand(3, device=self.device, generator=self.bg_gen)
            if self.bg_static is not None:
                self.bg_static.copy_(bg)
                bg = self.bg_static
        target = cache.deferred_target(v, d, bg) if self.graph_targets else cache.target(v, d, bg)
        return bg, target, cache.mask(v, d)


class DensifyState:
    """`xys_grad_norm`, `vis_counts` and `max_2dsize` of after_train (vanilla_gs.py:344-372) and their restart after
    every refinement (:491-493).  Who updates them: `update` in torch ops, or through `kernel`
    (gs_fused.densify_stats_), or -- `native` -- the backward of gs_fused.render_gaussians itself, into a
    `gs_fused.DensifyStats` whose tensors these then are.  `densify_until`: refinement's `stop_split_at`, from which
    step on nothing is updated (:347); None without refinement.  `first_vis`: on the ranks above 0 of a refining
    data-parallel run, which Gaussians the first view after a restart really saw (parallel.allreduce_densify_stats)."""

    def __init__(self, n: int, device, max_dim: int, densify_until: Optional[int] = None, rank: int = 0,
                 world: int = 1, kernel=None, native: bool = False, absgrad: bool = False):
        self.device, self.max_dim, self.kernel, self.native = device, max_dim, kernel, native
        self.absgrad = absgrad  # `update` reads out["xys"].absgrad (TrainConfig.absgrad, the separate ops)
        self.stop_at = math.inf if densify_until is None else densify_until
        self.watch_first_view = world > 1 and rank > 0 and densify_until is not None
        self.reset(n)

    def reset(self, n: int) -> None:
        if self.native:
            from gs_fused import DensifyStats

            self.native = DensifyStats(n, self.device, self.max_dim)
            self.xys_grad_norm, self.vis_counts, self.max_2dsize = self.native.as_tuple()
        else:
            self.xys_grad_norm = torch.zeros(n, device=self.device)
            self.vis_counts = torch.zeros(n, device=self.device, dtype=torch.int32)
            self.max_2dsize = torch.zeros(n, device=self.device)
        self.restart()

    def restart(self) -> None:
        self.first = True  # the reference's `xys_grad_norm is None` (vanilla_gs.py:354)
        self.first_vis = None
        if self.native:
            self.native.restart()

    def as_tuple(self):
        return self.xys_grad_norm, self.vis_counts, self.max_2dsize

    def update(self, out, max_dim: int, step: int) -> None:
        """After the backward of a view rendered to `out` (its "radii", and "xys" with the gradient retained)."""
        if step < self.stop_at:
            if self.native:
                pass  # done by the backward
            elif self.kernel is not None:
                # (absgrad: the per-pixel |dL/dxy| sums the compositing backward left on the tensor, in place of .grad)
                g = getattr(out["xys"], "absgrad", None) if self.absgrad else out["xys"].grad
                self.kernel(g, out["radii"], max_dim, self.xys_grad_norm, self.vis_counts,
                            self.max_2dsize, first=self.first)
            else:
                with torch.no_grad():
                    visible = out["radii"] > 0
                    g = getattr(out["xys"], "absgrad", None) if self.absgrad else out["xys"].grad
                    gnorm = torch.zeros_like(self.xys_grad_norm) if g is None else g.norm(dim=-1)
                    size = out["radii"].float() / max_dim
                    if self.first:
                        self.xys_grad_norm, self.vis_counts = gnorm.clone(), torch.ones_like(self.vis_counts)
                        self.max_2dsize = torch.where(visible, size, torch.zeros_like(size))
                    else:
                        self.xys_grad_norm += torch.where(visible, gnorm, torch.zeros_like(gnorm))
                        self.vis_counts += visible.to(torch.int32)
                        self.max_2dsize = torch.where(visible, torch.maximum(self.max_2dsize, size), self.max_2dsize)
            if self.first and self.watch_first_view:
                self.first_vis = (out["radii"] > 0).to(torch.int32)
        self.first = False


def _round_capacity(need: int, fits: bool) -> int:
    """Tile-list entries for a view that needed `need`: half as many again, rounded to 2^20.  `fits` (the lists it was
    rendered with were large enough): 2^16 of slack, rounded up; otherwise the next step is taken."""
    return ((int(1.5 * need) + 65536 + (1 << 20) - 1) >> 20) << 20 if fits else ((int(1.5 * need) + (1 << 20)) >> 20) << 20


class FusedStep:
    """An iteration with the view as ONE autograd node (gs_fused.render_gaussians: activations, projection, SH,
    binning, compositing; the densification statistics from its backward), and with `use_graph` render -> loss ->
    backward replayed as one HIP graph per view (gs_fused.render.ViewGraph).  Owns the tile lists' capacity."""
    ph = None   # no phase events on this path
    marks = ()

    def __init__(self, cfg: TrainConfig, model, data: TrainData, stats: DensifyState, photo, exchange, sh_views: bool,
                 dp: bool, history: list, mcfg=None):
        from gs_fused import ListCapacity, ViewSpec, render_gaussians
        from gs_fused.render import ViewGraph

        self.ViewSpec, self.render_gaussians, self.ViewGraph = ViewSpec, render_gaussians, ViewGraph
        self.cfg, self.model, self.stats, self.photo, self.exchange = cfg, model, stats, photo, exchange
        self.sh_views, self.dp, self.history, self.mcfg = sh_views, dp, history, mcfg

        def graph_loss(out, targets):  # (with a mask: the second static target of the graph, [h,w,1])
            loss = photo(out["rgb"], targets[0], targets[1] if len(targets) > 1 else None)
            return loss if mcfg is None else _add_mcmc_regulariser(loss, model, mcfg)

        self.graph_loss = graph_loss  # (a closure over the head alone: a ViewGraph holds it, and must not hold this)
        self.caps = ListCapacity()
        self.bilagrid = None  # a BilagridGroup: the head sees the view through its grid (not under use_graph)
        self.vgraph = self.vkey = None
        self.overflow_views = 0
        cam, g_ = data.cams_by_d[1][0], model.gauss
        with torch.no_grad():  # size the lists once, synchronously (vanilla: every view, utils.py:124)
            while True:
                probe = render_gaussians(g_["means"], g_["scales"], g_["quats"], g_["opacities"], g_["features_dc"],
                                         g_["features_rest"], cam.viewmat, cam.projmat, cam.campos, data.bg,
                                         ViewSpec(cfg.height, cfg.width, cam.fx, cam.fy, cam.cx, cam.cy, cfg.sh_degree,
                                                  rasterize_mode=cfg.rasterize_mode),  # (no backward: no absgrad)
                                         self.caps.capacity)
                need = int(probe["count"].item())
                if need <= self.caps.capacity:
                    self.caps.capacity = max(self.caps.capacity, _round_capacity(need, fits=True))
                    break
                self.caps.capacity = _round_capacity(need, fits=False)

    def __call__(self, step, v, d, cam, deg, bg, target, mask):
        cfg, caps, fstats, g_ = self.cfg, self.caps, self.stats.native, self.model.gauss
        spec = self.ViewSpec(cam.height, cam.width, cam.fx, cam.fy, cam.cx, cam.cy, deg,
                             rasterize_mode=cfg.rasterize_mode, absgrad=cfg.absgrad)
        fstats.enabled = step < self.stats.stop_at
        fstats.max_dim = max(cam.width, cam.height)  # `max(self.last_size)` of after_train
        if not cfg.use_graph:
            _zero_grads(self.model)
            slot = caps.slot(bg.device)
            used = caps.capacity
            collector = self.exchange.begin_sh_views(
                ("features_dc", "features_rest"), (g_["features_dc"], g_["features_rest"]), g_["means"], cam.campos,
                cfg.sh_degree, deg) if self.sh_views else None
            out = self.render_gaussians(g_["means"], g_["scales"], g_["quats"], g_["opacities"], g_["features_dc"],
                                        g_["features_rest"], cam.viewmat, cam.projmat, cam.campos, bg, spec, used,
                                        count_out=slot, stats=fstats, sh_collector=collector)
            if self.bilagrid is None:
                loss = self.photo(out["rgb"], target, mask)
            else:  # the heads see the view through its grid; out["rgb"] stays the raw render
                loss = self.bilagrid.add_regulariser(self.photo(self.bilagrid.apply(out["rgb"], v), target, mask))
            if self.mcfg is not None:
                loss = _add_mcmc_regulariser(loss, self.model, self.mcfg)
            loss.backward()
            caps.submitted(slot, used, bg.device)
            if caps.overflowed():
                self.overflow_views += 1
            return loss, out
        targets = (target,) if mask is None else (target, mask)
        # len(history) counts the refinements that swapped parameter tensors: N can come out unchanged (k culled,
        # k duplicated) while every tensor the graph points at is gone
        key = (spec, self.model.num_points, caps.capacity, fstats.enabled, len(self.history))
        if self.vkey != key:  # new SH degree, N changed by refinement, or larger lists: capture again
            self.vgraph = self.ViewGraph(_params(self.model), spec, caps.capacity, self.graph_loss, bg,
                                         [t.shape for t in targets], stats=fstats)
            self.vgraph.capture(cam.viewmat, cam.projmat, cam.campos, targets)
            self.vkey = key
        elif not self.vgraph.fits():  # the count of the previous replay is in pinned memory by now
            self.overflow_views += 1
            caps.capacity = _round_capacity(int(self.vgraph.count_host[0]), fits=False)
        loss, out = self.vgraph.replay(cam.viewmat, cam.projmat, cam.campos, targets)
        if self.dp:
            self.exchange.start_all()  # a replayed graph fires no hooks
        return loss, out


def _est_depth_terms(cfg: TrainConfig, step: int, pred_depth, gt_depth, target, mask):
    """co-gs' monocular-depth branch (depth_gs.py:477-531); the synthetic ground truth is metric: scale 1, shift 0.
    With a mask the terms see the masked images (:424-437): plain torch multiplies here, except that
    `fused_mono_depth`'s heads take the unmasked depths and multiply inside."""
    if mask is not None:
        target = target * mask
        if not cfg.fused_mono_depth:
            pred_depth, gt_depth, mask = pred_depth * mask, gt_depth * mask[..., 0], None
    return cogs_losses.optional_depth_terms(cfg, step, pred_depth, gt_depth, target, mono_scale_shift=(1.0, 0.0),
                                            fused=cfg.fused_mono_depth, mask=mask)


def _cogs_terms(cfg: TrainConfig, step: int, model, out, target, mask, gt_depth, d: int, depth_head, depth_on: bool):
    """What `DepthGSModel.get_loss_dict` adds to the photometric loss, in the order the trainer sums it."""
    terms = []
    if cfg.use_scale_regularization and step % 10 == 0:  # depth_gs.py:450-460
        terms.append(cogs_losses.scale_regularisation(model.gauss["scales"], cfg.max_gauss_ratio))
    if cfg.use_sparse_loss and step % 100 == 0:  # :462-467 (the raw opacity parameter, as written)
        terms.append(cogs_losses.sparse_loss(model.gauss["opacities"], cfg.sparse_lambda))
    if depth_on:
        # `gt_depth = self.get_gt_img(batch["depth"])` (downscaled like the image under a resolution schedule)
        gt_depth = downscale_depth(gt_depth, d)
        if cfg.use_est_depth:
            terms.extend(_est_depth_terms(cfg, step, out["depth"], gt_depth, target, mask).values())
        else:
            terms.append(depth_head(out, gt_depth, mask))
    return terms


class SeparateStep:
    """An iteration through the models' own call sequence: `model.render` (activations, projection, SH, rasterise as
    separate ops), the loss assembled in torch, `backward`.  On every `phase_every`-th step HIP events are recorded
    around the phases; `end_phases` closes such a step after the optimiser."""
    overflow_views = 0  # (the tile lists are rasterizer.rasterize's here: `_list_rebuilds`)

    def __init__(self, cfg: TrainConfig, model, data: TrainData, heads, exchange, sh_views: bool, device):
        self.cfg, self.model, self.gt_depth, self.cache = cfg, model, data.gt_depth, data.cache
        self.photo, self.depth_head, fused_clamp = heads
        cuda = device.type == "cuda"
        cogs = self.cogs = cfg.model == "co-gs"
        self.render_kw = dict(
            retain_xys_grad=True, clamp_rgb=not fused_clamp, sh_exchange=exchange if sh_views else None,
            caller_syncs=cfg.caller_syncs, render_depth=cogs, fused_depth=cogs and cfg.fused_depth and cuda,
            rasterize_mode=cfg.rasterize_mode, absgrad=cfg.absgrad,
            normalise_depth=not (cogs and cfg.fused_depth and cfg.fused_loss and cuda and not cfg.use_est_depth))
        self.depth_after = cfg.depth_loss_start_iteration if cogs and cfg.use_depth_loss else math.inf
        self.phase_every = cfg.phase_every if cuda else 0
        self.ph, self.depth_on = None, False
        self.marks = []  # (downscale factor, 5 events, depth loss on) per sampled step
        self.camera_opt = None  # a camera_opt.CameraOptimizer: its regulariser joins the loss (get_loss_dict)
        self.mcfg = None  # a gs_fused.MCMCConfig: the opacity / scale regularisers join the loss
        self.bilagrid = None  # a BilagridGroup: the heads see the view through its grid, its TV term joins the loss
        self.normal_terms = []  # normal_consistency: the term's value (a device scalar) at its first and latest step
        # ... and what a step that has the term adds to the render call: the normal pass, and for gaussian-splatting
        # the depth image it needs, from the one RGB + depth compositing pass (co-gs renders depth anyway and keeps its
        # own choice of the pass and of `normalise_depth`).  A step without the term renders what it always did
        self.normal_kw = dict(render_normals=True, **({} if cogs else dict(render_depth=True, fused_depth=cuda)))
        self.distortion_terms = []  # depth_distortion: likewise
        self.distortion_kw = dict(render_distortion=True, distortion_values=self._distortion_values,
                                  **({} if cogs else dict(render_depth=True, fused_depth=cuda)))

    def _distortion_values(self, depths):
        """2DGS's map of the depths onto [0, far / (far - near)), differentiable; the raw depths without a range."""
        near, far = self.cfg.distortion_near, self.cfg.distortion_far
        if near is None:
            return depths
        return (far / (far - near)) * (1.0 - near / depths)

    def _distortion_term(self, out, mask):
        from gs_fused import distortion_loss

        term = distortion_loss(out["distortion"], mask=mask)
        self.distortion_terms = self.distortion_terms[:1] + [term.detach()]
        return self.cfg.distortion_lambda * term

    def _normal_term(self, out, cam, mask):
        """`normal_lambda` times the depth-normal consistency of the view (gs_fused.normal_consistency_loss).  Where the
        render left "depth" out (co-gs with the fused depth head, which normalises inside its own kernels) the
        normalised depth is formed here from the accumulated depth and the alpha, by the render's own rule."""
        from gs_fused import normal_consistency_loss

        depth, alpha = out["depth"], out["alpha"]
        if depth is None:
            acc = out["depth_acc"]
            depth = torch.where(alpha > 0, acc / alpha, acc.detach().max())
        term = normal_consistency_loss(out["normals"], depth, alpha, cam.fx, cam.fy, cam.cx, cam.cy, mask=mask)
        self.normal_terms = self.normal_terms[:1] + [term.detach()]
        return self.cfg.normal_lambda * term

    def __call__(self, step, v, d, cam, deg, bg, target, mask):
        _zero_grads(self.model)
        ph = self.ph = _phase_marks(5) if (self.phase_every and step % self.phase_every == 0) else None
        if ph:
            ph[0].record()
        normals_on = self.cfg.normal_consistency and step > self.cfg.normal_start_iteration
        distortion_on = self.cfg.depth_distortion and step > self.cfg.distortion_start_iteration
        kw = self.render_kw
        if normals_on:
            kw = {**kw, **self.normal_kw}
        if distortion_on:
            kw = {**kw, **self.distortion_kw}
        out = self.model.render(cam, bg, deg, **kw)
        if ph:
            ph[1].record()
        if self.bilagrid is None:
            loss = self.photo(out["rgb"], target, mask)
        else:  # the heads see the view through its grid; out["rgb"] stays the raw render
            loss = self.bilagrid.add_regulariser(self.photo(self.bilagrid.apply(out["rgb"], v), target, mask))
        if self.cogs:
            self.depth_on = step > self.depth_after
            # (a dataset: the integer depth resized by the cache's kernel, so nothing is left to downscale)
            gt_depth, d_depth = (self.gt_depth[v], d) if self.cache is None else (self.cache.depth(v, d), 1)
            for term in _cogs_terms(self.cfg, step, self.model, out, target, mask, gt_depth, d_depth,
                                    self.depth_head, self.depth_on):
                loss = loss + term
        if self.camera_opt is not None:
            loss = loss + self.camera_opt.regulariser()
        if self.mcfg is not None:
            loss = _add_mcmc_regulariser(loss, self.model, self.mcfg)
        if normals_on:
            loss = loss + self._normal_term(out, cam, mask)
        if distortion_on:
            loss = loss + self._distortion_term(out, mask)
        if ph:
            ph[2].record()
        loss.backward()
        if ph:
            ph[3].record()
        return loss, out

    def end_phases(self, d: int) -> None:
        self.ph[4].record()
        self.marks.append((d, self.ph, self.depth_on))


class CameraGroup:
    """The seventh parameter group: `camera_opt.CameraOptimizer` over the training views, its Adam with the
    `camera_opt` schedule, and the cameras it corrects."""

    def __init__(self, cfg: TrainConfig, data: TrainData, device):
        from .camera_opt import CameraOptimizer, PosedCameras

        self.cfg = cfg
        self.opt = CameraOptimizer(cfg.camera_optimizer, cfg.num_views, device, cfg.camera_trans_l2_penalty,
                                   cfg.camera_rot_l2_penalty)
        self.posed = PosedCameras(data.cams_np, device, true_cams_np=data.true_cams_np)
        self.adam = torch.optim.Adam([self.opt.pose_adjustment], lr=cfg.camera_lr, eps=1e-15)

    def step_camera(self, step: int, v: int, like: CameraTensors) -> CameraTensors:
        """Zero the group's gradient, set this step's learning rate, and return view `v` corrected."""
        self.adam.zero_grad(set_to_none=True)
        self.adam.param_groups[0]["lr"] = means_lr(step, self.cfg.camera_lr, self.cfg.camera_lr_final,
                                                   self.cfg.camera_lr_max_steps)
        return self.posed.camera(self.opt, v, like)

    def eval_cameras(self, data: TrainData):
        with torch.no_grad():
            return [self.posed.camera(self.opt, v, c) for v, c in enumerate(data.cams_by_d[1])]


def make_camera_optimiser(cfg: TrainConfig, data: TrainData, device) -> Optional[CameraGroup]:
    return None if cfg.camera_optimizer == "off" else CameraGroup(cfg, data, device)


class BilagridGroup:
    """The eighth parameter group: `gs_fused.BilateralGrids` over the training views and its own gs_fused.FusedAdam
    with gsplat's schedule (`gs_fused.bilagrid.lr_schedule` over `cfg.iters`)."""

    def __init__(self, cfg: TrainConfig, device):
        from gs_fused import BilateralGrids, FusedAdam

        self.cfg = cfg
        gw, gh, gl = (int(s) for s in cfg.bilagrid_shape)
        self.grids = BilateralGrids(cfg.num_views, gw, gh, gl, device=device)
        self.adam = FusedAdam([self.grids.grids], lr=self.lr(0), eps=1e-15)

    def lr(self, step: int) -> float:
        from gs_fused.bilagrid import lr_schedule

        return lr_schedule(step, self.cfg.bilagrid_lr, self.cfg.iters)

    def begin_step(self, step: int) -> None:
        """Zero the group's gradient and set this step's learning rate."""
        self.adam.zero_grad(set_to_none=True)
        self.adam.param_groups[0]["lr"] = self.lr(step)

    def apply(self, rgb: torch.Tensor, v: int) -> torch.Tensor:
        """What the loss heads see of view `v`'s render."""
        return self.grids.slice(rgb, int(v))

    def add_regulariser(self, loss: torch.Tensor) -> torch.Tensor:
        return loss + self.cfg.bilagrid_tv_weight * self.grids.tv_loss()

    def record(self) -> Dict:
        from gs_fused.bilagrid import IDENTITY

        with torch.no_grad():
            g = self.grids.grids
            eye = torch.tensor(IDENTITY, dtype=g.dtype, device=g.device)
            away = (g - eye).abs().amax(dim=(1, 2, 3, 4))
            return {"bilateral_grid": {"shape": list(self.grids.shape), "tv_weight": self.cfg.bilagrid_tv_weight,
                                       "lr": self.cfg.bilagrid_lr, "tv_end": float(self.grids.tv_loss()),
                                       "max_abs_from_identity": [float(a) for a in away.cpu()],
                                       "checksum": float(g.double().sum())}}


def _normal_record(cfg: TrainConfig, run_step) -> Dict:
    """The record's "normal_consistency" entry: the term (before `normal_lambda`) at the first and the last step that
    had it; None where the run ended before `normal_start_iteration`."""
    terms = [float(t) for t in run_step.normal_terms]
    return {"normal_consistency": {"lambda": cfg.normal_lambda, "start_iteration": cfg.normal_start_iteration,
                                   "term_first": terms[0] if terms else None,
                                   "term_last": terms[-1] if terms else None}}


def _distortion_record(cfg: TrainConfig, run_step) -> Dict:
    """The record's "depth_distortion" entry: the term (before `distortion_lambda`) at the first and the last step that
    had it; None where the run ended before `distortion_start_iteration`."""
    terms = [float(t) for t in run_step.distortion_terms]
    return {"depth_distortion": {"lambda": cfg.distortion_lambda, "start_iteration": cfg.distortion_start_iteration,
                                 "near": cfg.distortion_near, "far": cfg.distortion_far,
                                 "term_first": terms[0] if terms else None,
                                 "term_last": terms[-1] if terms else None}}


def make_bilagrid(cfg: TrainConfig, device) -> Optional[BilagridGroup]:
    return BilagridGroup(cfg, device) if cfg.bilateral_grid else None


def pose_errors(cfg: TrainConfig, data: TrainData, camera: Optional[CameraGroup], device):
    """-> (degrees, scene units): means over the training views of the angle and the distance between the (corrected)
    camera and the true one; None where the run has neither a camera optimizer nor pose noise."""
    if camera is not None:
        return camera.posed.pose_errors(camera.opt)
    if tuple(cfg.pose_noise) == (0.0, 0.0):
        return None
    from .camera_opt import PosedCameras

    return PosedCameras(data.cams_np, device, true_cams_np=data.true_cams_np).pose_errors(None)


def pose_record(camera: Optional[CameraGroup], start, end) -> Dict:
    if start is None:
        return {}
    rec = {"pose_err_rot_deg_start": start[0], "pose_err_rot_deg_end": end[0],
           "pose_err_trans_start": start[1], "pose_err_trans_end": end[1]}
    if camera is not None:
        rec.update({k: float(v.detach()) for k, v in camera.opt.metrics().items()})
        rec["pose_adjustment"] = camera.opt.pose_adjustment.detach().cpu().tolist()
    return rec


def refine_model(cfg: TrainConfig, rcfg, step: int, model, optims, sharded, exchange, stats: DensifyState,
                 max_dim: int, dp: bool, history: list) -> None:
    """`refinement_after` (vanilla_gs.py:381-497): the statistics all-reduced under data parallelism, split /
    duplicate / cull / opacity reset (`_refine`), the new tensors and their Adam moments installed in the model, the
    optimisers, the gradient exchange and the sharded update, and the statistics restarted.  `history` gets (step, N)
    when the model's tensors changed."""
    branch, reset = _refinement_branch(rcfg, step, cfg.num_views)
    if branch != "none" or reset:
        if dp and branch == "densify":
            allreduce_densify_stats(*stats.as_tuple(), first_visible=stats.first_vis, force=cfg.force_exchange)
        old = _params(model)
        moments = {}
        for o in optims.values():
            moments.update(_adam_moments(o, old))
        if sharded is not None:
            moments = sharded.full_moments()  # refinement moves whole rows of both moments
        new, new_moments, info = _refine(old, moments, stats.as_tuple(), rcfg, step, cfg.num_views, max_dim,
                                         seed=cfg.refine_seed + step)
        if any(new[k] is not old[k] for k in PARAM_NAMES):
            model.replace(new)
            cur = _params(model)
            for o in optims.values():
                _swap_parameters(o, old, cur, new_moments)
            if info["n_out"] != info["n_in"]:
                stats.reset(info["n_out"])
            history.append((step, model.num_points))
            exchange.rebind(_params(model))
        if sharded is not None:
            # new tensors, or the same ones with an opacity reset (which zeroed moments in the
            # gathered copies): cut this rank's rows again
            sharded.bind(_params(model), new_moments)
    # the statistics restart after every refinement_after past the warm-up (:491-493)
    stats.restart()


def refine_model_mcmc(cfg: TrainConfig, mcfg, step: int, model, optims, exchange, stats: DensifyState,
                      history: list) -> None:
    """A refinement of `strategy="mcmc"` (gs_fused.mcmc_refine): dead Gaussians relocated in place, then the model
    grown towards `cap_max`.  Nothing is read back; only a refinement that added rows installs new tensors in the model
    and the optimisers -- a relocation leaves every tensor (and a captured view graph) where it is."""
    old = _params(model)
    moments = {}
    for o in optims.values():
        moments.update(_adam_moments(o, old))
    new, new_moments, info = _mcmc_refine(old, moments, mcfg, step, seed=cfg.refine_seed)
    if info["n_out"] != info["n_in"]:
        model.replace(new)
        cur = _params(model)
        for o in optims.values():
            _swap_parameters(o, old, cur, new_moments)
        stats.reset(info["n_out"])
        history.append((step, model.num_points))
        exchange.rebind(_params(model))


def prune_model(cfg: TrainConfig, step: int, model, optims, exchange, stats: DensifyState, cams, history: list,
                log: list) -> None:
    """A step of `prune_at`: the contribution statistics over the views `cams`, the keep mask of `prune_rule`, and the
    surviving rows of the parameters and their Adam moments installed as `refine_model` installs a refinement that
    changed N.  `log` gets {step, n_in, n_out, ms} (ms: host time around the whole, the device drained at both ends)."""
    from gs_fused import prune_gaussians, prune_mask

    from .pipeline import contribution_stats

    torch.cuda.synchronize(model.gauss["means"].device)
    t0 = time.perf_counter()
    n_in = model.num_points
    with torch.no_grad():
        cs = contribution_stats(model, cams, cfg)
        keep = prune_mask(cs, cfg.prune_rule, threshold=cfg.prune_threshold, keep=cfg.prune_keep,
                          scales=torch.exp(model.gauss["scales"]) if cfg.prune_rule == "weight_sum" else None)
    if not bool(keep.all()):
        old = _params(model)
        moments = {}
        for o in optims.values():
            moments.update(_adam_moments(o, old))
        new, new_moments = prune_gaussians(old, moments, keep)
        model.replace(new)
        cur = _params(model)
        for o in optims.values():
            _swap_parameters(o, old, cur, new_moments)
        stats.reset(model.num_points)
        history.append((step, model.num_points))
        exchange.rebind(_params(model))
    torch.cuda.synchronize(model.gauss["means"].device)
    log.append({"step": step, "n_in": n_in, "n_out": model.num_points, "ms": 1e3 * (time.perf_counter() - t0)})


def phase_record(marks, cfg: TrainConfig, factors) -> Dict:
    """The four `phase_ms_*` entries of the result from the steps' events: medians over all sampled steps, per
    resolution under a coarse-to-fine schedule, before / after co-gs' depth loss joins, and every sample."""
    rec = dict.fromkeys(("phase_ms_median", "phase_ms_median_by_resolution", "phase_ms_median_by_depth_loss",
                         "phase_ms_series"))
    if not marks:
        return rec
    names = ("render", "loss", "backward", "stats_exchange_optimizer")

    def med(marks):
        ms = np.array([[m[i].elapsed_time(m[i + 1]) for i in range(4)] for m in marks])
        out = {k: round(float(np.median(ms[:, i])), 4) for i, k in enumerate(names)}
        out["samples"] = len(marks)
        return out

    rec["phase_ms_median"] = med([m for _, m, _ in marks])
    if len(factors) > 1:  # the coarse-to-fine schedule: one set of medians per resolution
        rec["phase_ms_median_by_resolution"] = {
            f"{cfg.width // d_}x{cfg.height // d_}": med([m for dd, m, _ in marks if dd == d_])
            for d_ in sorted({dd for dd, _, _ in marks}, reverse=True)}
    if cfg.model == "co-gs":  # before / after the depth loss joins (the depth pass then has a backward as well)
        rec["phase_ms_median_by_depth_loss"] = {
            ("depth_loss_on" if on else "depth_loss_off"): med([m for _, m, o in marks if o == on])
            for on in sorted({o for _, _, o in marks})}
    if cfg.phase_series:
        rec["phase_ms_series"] = [[dd] + [round(m[i].elapsed_time(m[i + 1]), 4) for i in range(4)] for dd, m, _ in marks]
    return rec


def result_record(cfg: TrainConfig, device, world: int, model, run: Dict, eval0: Dict, eval1: Dict, phases: Dict) -> Dict:
    """What `train` returns.  `run`: what the driver counted (see there)."""
    steps, elapsed = cfg.iters - run["start_step"], run["elapsed"]
    cogs, masked = cfg.model == "co-gs", cfg.mask != "none" or bool((run.get("dataset") or {}).get("masks"))
    checksum = float(sum(p.detach().double().sum() for p in model.param_list()))
    return {"iters": steps, "start_step": run["start_step"], "seconds": elapsed,
            "iters_per_s": steps / elapsed, "psnr_start": eval0["psnr"],
            "psnr_end": eval1["psnr"], "losses": run["losses"], "param_checksum": checksum,
            "views_per_s": world * steps / elapsed, "num_gaussians_start": run["n0"],
            "num_gaussians_end": model.num_points, "refinements": run["history"],
            # (step, bytes) whenever the per-step exchange volume changed: SH warm-up, refinement
            "allreduce_bytes": run["exchanged_bytes"],
            "render": run["render"], "list_overflow_views": run["overflow_views"], **phases,
            "depth_segments": _depth_segments_record(device),
            "schedule": {"num_downscales": cfg.num_downscales, "resolution_schedule": cfg.resolution_schedule,
                         "background_color": cfg.background_color, "caller_syncs": cfg.caller_syncs},
            "update": run["update"], "init": cfg.init, "model": cfg.model, "mask": cfg.mask,
            **({"psnr_masked_start": eval0["psnr_masked"], "psnr_masked_end": eval1["psnr_masked"]} if masked else {}),
            # (only where it was asked for: a classic run's record stays what it was, to the byte)
            **({"rasterize_mode": cfg.rasterize_mode} if cfg.rasterize_mode != "classic" else {}),
            **({"absgrad": True} if cfg.absgrad else {}),
            **({"strategy": cfg.strategy} if cfg.strategy != "default" else {}),
            **({"camera_model": cfg.camera_model} if cfg.camera_model != "pinhole" else {}),
            "depth": ({"loss_from_step": cfg.depth_loss_start_iteration + 1 if cfg.use_depth_loss else None,
                       "one_compositing_pass": bool(cfg.fused_depth and device.type == "cuda"),
                       "mean_abs_error_start_end": [eval0["depth_err"], eval1["depth_err"]]} if cogs else None),
            "peak_memory_bytes": (int(torch.cuda.max_memory_allocated(device)) if device.type == "cuda" else None),
            "densify_grad_thresh": (run["rcfg"].densify_grad_thresh if cfg.densify else None),
            # (only where it was asked for, as above)
            **({"dataset": run["dataset"]} if run.get("dataset") is not None else {}),
            **({"prune": run["prune"]} if run.get("prune") is not None else {}),
            **({"filter_3d": run["filter_3d"]} if run.get("filter_3d") is not None else {}),
            **run.get("pose", {}), **run.get("appearance", {})}


def _note_bytes(log: list, step: int, nbytes: int) -> None:
    if not log or log[-1][1] != nbytes:
        log.append((step, nbytes))


def train(cfg: TrainConfig, device, rank: int = 0, world: int = 1) -> Dict:
    """Fit a perturbed copy of a hidden scene to its own renders.  Returns timing
    and quality numbers; every rank ends with identical parameters."""
    _check_config(cfg)
    _check_camera_model(cfg, world)
    _check_camera_optimizer(cfg, device, world)
    _check_absgrad(cfg, device)
    _check_mcmc(cfg, device, world)
    _check_bilateral_grid(cfg, device, world)
    _check_normal_consistency(cfg, device, world)
    _check_depth_distortion(cfg, device, world)
    _check_prune(cfg, device, world)
    _check_filter_3d(cfg, device, world)
    cuda = device.type == "cuda"
    mcfg = None
    if cfg.strategy == "mcmc":
        mcfg = cfg.mcmc
        if mcfg is None:
            from gs_fused import MCMCConfig

            mcfg = MCMCConfig()
        cfg = replace(cfg, densify=False)  # (a copy: the default strategy's schedule does not run)
    dp = world > 1 or (cfg.force_exchange and dist.is_available() and dist.is_initialized())
    if cfg.dataset is not None:
        if world > 1 or dp:
            raise ValueError("dataset: a dataset directory trains on one GPU (world size 1): the per-rank view "
                             "sampling of a real dataset is not implemented")
        data = make_dataset_data(cfg, device)
        ds = data.dataset
        cfg = replace(cfg, num_views=len(ds), width=ds.width, height=ds.height)  # (a copy: the caller's is left alone)
        if ds.camera_model != cfg.camera_model:  # the dataset's cameras decide
            cfg = replace(cfg, camera_model=ds.camera_model)
            _check_camera_model(cfg, world)
        model = dataset_initial_model(cfg, ds, device)
    else:
        data = make_data(cfg, device)
        model = initial_model(cfg, device)
    optims, sharded = make_optimisers(cfg, model, device, dp)
    heads = loss_heads(cfg, device)
    rcfg = cfg.refine
    if cfg.densify and rcfg is None:
        from gs_fused import RefineConfig

        rcfg = RefineConfig()
    n0 = model.num_points
    start_step = 0
    camera = make_camera_optimiser(cfg, data, device)
    bilagrid = make_bilagrid(cfg, device)
    if cfg.resume_from:
        from .checkpoint import load_checkpoint

        start_step = load_checkpoint(cfg.resume_from, model, optims, sharded=sharded,  # resizes the model to the saved N
                                     camera=None if camera is None else (camera.opt, camera.adam),
                                     **({} if bilagrid is None else {"bilagrid": (bilagrid.grids, bilagrid.adam)}))
    f3d = None
    if cfg.filter_3d:
        f3d = Filter3DState(cfg, data, device)
        f3d.start(cfg, model, start_step)
    else:
        model.filter_3d = None  # (a checkpoint written with a filter resumes as the raw model)
    use_fused = (cfg.fused_render or cfg.use_graph) and cuda and cfg.split_sh and cfg.fused_loss \
        and cfg.sh_degree in (0, 1, 2, 3)
    kernel = None
    if cfg.fused_activations and cuda and not use_fused:
        from gs_fused import densify_stats_ as kernel
    stats = DensifyState(model.num_points, device, max(cfg.width, cfg.height),
                         densify_until=0 if mcfg is not None else (rcfg.stop_split_at if cfg.densify else None),
                         rank=rank, world=world,
                         kernel=kernel, native=use_fused, absgrad=cfg.absgrad and not use_fused)
    eval0 = evaluate(model, data, cfg, None if camera is None else camera.eval_cameras(data))
    pose0 = pose_errors(cfg, data, camera, device)
    exchange, sh_views = make_exchange(cfg, model, sharded is not None, dp)
    inputs = StepInputs(cfg, data, device, rank)
    means_group = None  # the scheduled learning rate's param group (after load_checkpoint, which replaces the groups)
    if cfg.means_lr_schedule and sharded is None:
        means_group = (optims["all"] if "all" in optims else optims["means"]).param_groups[0]
    losses, history, exchanged_bytes = [], [], []  # history: (step, N) after every refinement that changed the model
    prune_steps, prune_log = frozenset(int(s) for s in cfg.prune_at), []
    cams_by_d = data.cams_by_d
    if cuda:
        torch.cuda.synchronize(device)
    if dp:
        dist.barrier()
    # the ~170 k objects that torch and the setup above leave tracked never die during training: taken out of the
    # cyclic collector's generations for the duration of the loop, so that its full passes (~30 ms each over those
    # objects) do not recur -- the loop's own garbage is still collected
    gc.collect()
    gc.freeze()
    if cuda:
        torch.cuda.reset_peak_memory_stats(device)
    t0 = time.perf_counter()
    try:  # (an exception in the loop must not leave the collector frozen for the rest of the process)
        if use_fused:  # (sizes its tile lists with a probe render: inside the timed region, as the first view is)
            run_step = FusedStep(cfg, model, data, stats, heads[0], exchange, sh_views, dp, history, mcfg=mcfg)
        else:
            run_step = SeparateStep(cfg, model, data, heads, exchange, sh_views, device)
            run_step.camera_opt = None if camera is None else camera.opt
            run_step.mcfg = mcfg
        run_step.bilagrid = bilagrid
        rebuilds0 = _list_rebuilds()
        for step in range(start_step, cfg.iters):
            v = view_for_rank(step, rank, world, cfg.num_views)
            deg = min(step // cfg.sh_degree_interval, cfg.sh_degree)
            exchange.active_rows["features_rest"] = (deg + 1) ** 2 - 1
            # this step's resolution (vanilla_gs.py:646-657, 719-720), background, ground truth and mask
            d = downscale_factor(step, cfg.num_downscales, cfg.resolution_schedule)
            cam = cams_by_d[d][v]
            if f3d is not None and f3d.due(step, d):
                f3d.update(model, d, step)
            rows_changed = len(history)
            max_dim = max(cam.width, cam.height)  # `max(self.last_size)` of after_train / refinement_after
            bg_step, target, m_step = inputs(v, d)
            if camera is not None:  # this step's camera, a function of the view's six numbers
                cam = camera.step_camera(step, v, cam)
            if bilagrid is not None:
                bilagrid.begin_step(step)
            loss, out = run_step(step, v, d, cam, deg, bg_step, target, m_step)
            stats.update(out, max_dim, step)
            if dp and sharded is None:
                _note_bytes(exchanged_bytes, step, exchange.finish())
            if cfg.means_lr_schedule:
                # the scheduler steps after the optimizer (trainer.py:479-525): iteration `step` runs at lr(step)
                if sharded is not None:
                    sharded.set_lr("means", means_lr(step, LRS["means"]))
                else:
                    means_group["lr"] = means_lr(step, LRS["means"])
            for o in optims.values():
                o.step()
            if camera is not None:
                camera.adam.step()
            if bilagrid is not None:
                bilagrid.adam.step()
            if sharded is not None:
                _note_bytes(exchanged_bytes, step, sharded.step())
            if run_step.ph:
                run_step.end_phases(d)
            # refinement_after: every refine_every iterations, after the optimizer step
            # (TrainingCallback(update_every_num_iters=refine_every), vanilla_gs.py:610-616)
            if cfg.densify and step % rcfg.refine_every == 0 and step > rcfg.warmup_length:
                refine_model(cfg, rcfg, step, model, optims, sharded, exchange, stats, max_dim, dp, history)
            if mcfg is not None:
                # gsplat's step_post_backward: the refinement when one is due, then the position noise -- every step,
                # at the step's means learning rate, outside the captured graph
                if _mcmc_branch(mcfg, step):
                    refine_model_mcmc(cfg, mcfg, step, model, optims, exchange, stats, history)
                lr = means_lr(step, LRS["means"]) if cfg.means_lr_schedule else LRS["means"]
                _mcmc_noise(model, lr * mcfg.noise_lr, cfg.refine_seed ^ 0x5DEECE66D, step)
            if prune_steps and step in prune_steps:
                prune_model(cfg, step, model, optims, exchange, stats,
                            cams_by_d[1] if camera is None else camera.eval_cameras(data), history, prune_log)
            if f3d is not None and len(history) != rows_changed:
                f3d.update(model, d, step)  # new rows: the buffer follows before anything renders them
            if cfg.save_every and cfg.checkpoint_dir and step > 0 and step % cfg.save_every == 0 and \
                    (rank == 0 or sharded is not None):
                from .checkpoint import save_checkpoint

                # (sharded moments are gathered by a collective: every rank calls, rank 0 writes)
                save_checkpoint(cfg.checkpoint_dir, step, model, optims, sharded=sharded, write=rank == 0,
                                camera=None if camera is None else (camera.opt, camera.adam),
                                **({} if bilagrid is None else {"bilagrid": (bilagrid.grids, bilagrid.adam)}))
            if cfg.log_every and step % cfg.log_every == 0:
                losses.append(float(loss.detach()))
        if dp:
            dist.barrier()
        if cuda:
            torch.cuda.synchronize(device)
        elapsed = time.perf_counter() - t0
    finally:
        gc.unfreeze()
    eval1 = evaluate(model, data, cfg, None if camera is None else camera.eval_cameras(data))
    pose1 = pose_errors(cfg, data, camera, device)
    if cfg.export_ply and rank == 0:
        from gs_io.ply import write_gaussian_ply

        write_gaussian_ply(cfg.export_ply, export_parameters(model))
    heldout = None
    if data.cache is not None and cfg.dataset_eval_split and cuda:
        from gs_io.dataset import load_dataset

        held = load_dataset(cfg.dataset, cfg.dataset_eval_split, **dataset_config(cfg))
        heldout = evaluate_dataset(model, held, cfg, cfg.dataset_eval_split, device) if len(held) else None
    run = {"start_step": start_step, "elapsed": elapsed, "n0": n0, "losses": losses, "history": history,
           "dataset": None if data.cache is None else {
               "path": cfg.dataset, "num_train_views": cfg.num_views, "width": cfg.width, "height": cfg.height,
               "channels": data.cache.channels, "masks": data.cache.masks is not None,
               "depth": data.cache.depths is not None, "cache_bytes": data.cache.nbytes,
               "seed_points": None if data.dataset.points3D_xyz is None else int(len(data.dataset.points3D_xyz)),
               "dataparser_scale": data.dataset.scale, "heldout": heldout},
           "exchanged_bytes": exchanged_bytes, "rcfg": rcfg,
           "render": ("hip graph per view" if cfg.use_graph else "one fused op") if use_fused else "separate ops",
           "overflow_views": run_step.overflow_views + (_list_rebuilds() - rebuilds0),
           "pose": pose_record(camera, pose0, pose1),
           "appearance": {**({} if bilagrid is None else bilagrid.record()),
                          **({} if data.exposure is None else {"view_exposure": data.exposure}),
                          **(_normal_record(cfg, run_step) if cfg.normal_consistency else {}),
                          **(_distortion_record(cfg, run_step) if cfg.depth_distortion else {})},
           "prune": prune_log if prune_steps else None,
           "filter_3d": None if f3d is None else {"every": f3d.every, "updates": f3d.updates},
           "update": "reduce-scatter + sharded Adam + all-gather" if sharded is not None else
           ("all-reduce (geometry) + all-gathered colour cotangents (SH) + Adam" if sh_views else "all-reduce + Adam")}
    return result_record(cfg, device, world, model, run, eval0, eval1, phase_record(run_step.marks, cfg, data.factors))


def _phase_marks(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def _list_rebuilds() -> int:
    """Views whose device-sized tile lists came out too small and were built again (rasterizer.rasterize counts
    them; 0 where that module's native library is not loaded: CPU stand-ins)."""
    import sys

    mod = sys.modules.get("rasterizer.rasterize")
    return int(mod.counters["list_rebuilds"]) if mod is not None and hasattr(mod, "counters") else 0


# the refinement backend (module-level so that CPU tests can substitute stand-ins)
def _refinement_branch(rcfg, step, num_train_data):
    from gs_fused import refinement_branch

    return refinement_branch(rcfg, step, num_train_data)


def _adam_moments(optimizer, params):
    from gs_fused import adam_moments

    return adam_moments(optimizer, params)


def _swap_parameters(optimizer, old, new, new_moments):
    from gs_fused import swap_parameters

    return swap_parameters(optimizer, old, new, new_moments)


def _refine(params, moments, stats, rcfg, step, num_train_data, max_dim, seed):
    from gs_fused import refine_gaussians

    return refine_gaussians(params, moments, stats, rcfg, step, num_train_data, max_dim, seed=seed)


# the MCMC strategy's backend (module-level for the same reason)
def _mcmc_branch(mcfg, step):
    from gs_fused import mcmc_branch

    return mcmc_branch(mcfg, step)


def _mcmc_refine(params, moments, mcfg, step, seed):
    from gs_fused import mcmc_refine

    return mcmc_refine(params, moments, mcfg, step, seed=seed)


def _mcmc_noise(model, scaler, seed, step):
    from gs_fused import mcmc_inject_noise_

    g = model.gauss
    mcmc_inject_noise_(g["means"], g["scales"], g["quats"], g["opacities"], scaler, seed, step)


def _add_mcmc_regulariser(loss, model, mcfg):
    """loss + opacity_reg * mean(opacity) + scale_reg * mean(scale) (gs_fused.mcmc_regularizer: a float64 scalar)."""
    from gs_fused import mcmc_regularizer

    g = model.gauss
    return loss + mcmc_regularizer(g["opacities"], g["scales"], mcfg.opacity_reg, mcfg.scale_reg).to(loss.dtype)
