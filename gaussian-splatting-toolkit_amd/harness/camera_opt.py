"""Camera pose refinement: the toolkit's `CameraOptimizer` (gs_toolkit/cameras/camera_optimizers.py:38-152) with its
two exponential maps (cameras/lie_groups.py), and the way a corrected camera reaches the rasterizer.

`pose_adjustment` is [num_views, 6], zero at the start: three translations, then three so(3) components.  The
correction multiplies the camera-to-world matrix on the right (camera_optimizers.py:119-123, `c2w @ adj`); after it
come the model's y/z flip and analytic inverse (vanilla_gs.py:722-734) and `projmat = projection_matrix(...) @
viewmat`, all torch ops, so autograd carries the projection's `v_viewmat` / `v_projmat`
(rasterizer.cuda.project_gaussians_backward_pose) back to the six numbers.  The colour's view dependence gives the
pose no gradient: the SH op has none with respect to the view directions, in the reference or here.

The maps are written from their formulas and keep the reference's numerics:
  SO3xR3   R = I + (sin t / t) K + ((1 - cos t) / t^2) K^2, K the cross-product matrix of w, t = sqrt(max(|w|^2,
           1e-4)) -- the squared angle clamped BEFORE the root -- and the translation taken as it is;
  SE3      R = cos t I + ((1 - cos t) / t^2) w w^T + (sin t / t) K and
           p = (sin t / t) v + ((1 - cos t) / t^2) w x v + ((t - sin t) / t^3) w (w . v), t = |w|; below t = 1e-2 the
           series: cos t = 8 / (4 + t^2) - 1, sin t / t = (cos t + 1) / 2 and (1 - cos t) / t^2 = (sin t / t) / 2 in
           the rotation, 1 - t^2 / 6, 1 / 2 - t^2 / 24 and 1 / 6 - t^2 / 120 in the translation.
"""
import math
from typing import Dict, Optional

import numpy as np
import torch

from .pipeline import CameraTensors

MODES = ("off", "SO3xR3", "SE3")


def _cross_matrix(w: torch.Tensor) -> torch.Tensor:
    """[b,3] -> [b,3,3], K with K u = w x u."""
    x, y, z = w.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([torch.stack([o, -z, y], -1), torch.stack([z, o, -x], -1), torch.stack([-y, x, o], -1)], -2)


def exp_map_SO3xR3(tangent: torch.Tensor) -> torch.Tensor:
    """[b,6] (translation, then so(3)) -> [b,3,4] = [R | t] of the direct product SO(3) x R^3."""
    trans, w = tangent[:, :3], tangent[:, 3:]
    angle = torch.clamp((w * w).sum(1), 1e-4).sqrt()
    inv = 1.0 / angle
    a = (inv * angle.sin())[:, None, None]
    b = (inv * inv * (1.0 - angle.cos()))[:, None, None]
    K = _cross_matrix(w)
    R = a * K + b * torch.bmm(K, K) + torch.eye(3, dtype=w.dtype, device=w.device)[None]
    return torch.cat([R, trans[:, :, None]], dim=-1)


def exp_map_SE3(tangent: torch.Tensor) -> torch.Tensor:
    """[b,6] (v, w) of se(3) -> [b,3,4] = [R | p] of SE(3)."""
    v, w = tangent[:, :3, None], tangent[:, 3:, None]  # [b,3,1]
    t = torch.linalg.norm(w, dim=1)[:, None]  # [b,1,1]
    t2, t3 = t ** 2, t ** 3
    small = t < 1e-2
    one = torch.ones(1, dtype=tangent.dtype, device=tangent.device)
    t_safe, t2_safe, t3_safe = torch.where(small, one, t), torch.where(small, one, t2), torch.where(small, one, t3)
    sin = t.sin()
    cos = torch.where(small, 8 / (4 + t2) - 1, t.cos())
    sin_t = torch.where(small, 0.5 * cos + 0.5, sin / t_safe)           # sin t / t
    cos_t2 = torch.where(small, 0.5 * sin_t, (1 - cos) / t2_safe)       # (1 - cos t) / t^2
    eye = torch.eye(3, dtype=tangent.dtype, device=tangent.device)[None]
    R = cos_t2 * w @ w.transpose(1, 2) + cos * eye + _cross_matrix((sin_t * w)[:, :, 0])
    sin_t = torch.where(small, 1 - t2 / 6, sin_t)
    cos_t2 = torch.where(small, 0.5 - t2 / 24, cos_t2)
    rest = torch.where(small, 1.0 / 6 - t2 / 120, (t - sin) / t3_safe)  # (t - sin t) / t^3
    p = sin_t * v + cos_t2 * torch.cross(w, v, dim=1) + rest * (w @ (w.transpose(1, 2) @ v))
    return torch.cat([R, p], dim=-1)


def to4x4(pose: torch.Tensor) -> torch.Tensor:
    """[..., 3, 4] -> [..., 4, 4] with the row (0, 0, 0, 1)."""
    last = torch.zeros_like(pose[..., :1, :])
    last[..., 0, 3] = 1
    return torch.cat([pose, last], dim=-2)


def c2w_from_viewmat(viewmat: np.ndarray) -> np.ndarray:
    """The toolkit's camera-to-world [3,4] (x right, y up, z back) of a rasterizer view matrix (world -> camera, x
    right, y down, z forward): the inverse, formed in float64, with the y and z axes flipped back."""
    V = np.asarray(viewmat, np.float64)
    R = V[:3, :3].T
    return np.concatenate([R * np.array([1.0, -1.0, -1.0]), (-R @ V[:3, 3])[:, None]], axis=1).astype(np.float32)


def projection_matrix(znear: float, zfar: float, fovx: float, fovy: float, device=None) -> torch.Tensor:
    """gs_toolkit/utils/comms.py:103-123 (harness.scene.projection_matrix), as a tensor."""
    from .scene import projection_matrix as _pm

    return torch.from_numpy(_pm(znear, zfar, fovx, fovy)).to(device)


def view_matrices(c2w: torch.Tensor, proj: torch.Tensor):
    """`get_outputs`' camera (vanilla_gs.py:722-734, :771): c2w [3,4] or [4,4] -> (viewmat [4,4], projmat [4,4] =
    proj @ viewmat, campos [3])."""
    R = c2w[:3, :3] @ torch.diag(torch.tensor([1, -1, -1], device=c2w.device, dtype=c2w.dtype))
    T = c2w[:3, 3:4]
    R_inv = R.T
    T_inv = -R_inv @ T
    bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=c2w.device, dtype=c2w.dtype)
    viewmat = torch.cat([torch.cat([R_inv, T_inv], dim=1), bottom], dim=0)
    return viewmat, proj @ viewmat, T[:, 0]


class CameraOptimizer(torch.nn.Module):
    """`pose_adjustment` [num_views,6] and what the toolkit's module does with it."""

    def __init__(self, mode: str, num_views: int, device, trans_l2_penalty: float = 1e-2,
                 rot_l2_penalty: float = 1e-3):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"unknown camera_optimizer {mode!r}: one of {MODES}")
        self.mode, self.num_views = mode, num_views
        self.trans_l2_penalty, self.rot_l2_penalty = trans_l2_penalty, rot_l2_penalty
        if mode != "off":
            self.pose_adjustment = torch.nn.Parameter(torch.zeros((num_views, 6), device=device))

    def forward(self, indices) -> torch.Tensor:
        """-> [k,3,4]: from the corrected camera's coordinates to the given camera's."""
        if self.mode == "off":
            return torch.eye(4)[None, :3, :4].tile(len(indices), 1, 1)
        tangent = self.pose_adjustment[indices, :]
        return exp_map_SO3xR3(tangent) if self.mode == "SO3xR3" else exp_map_SE3(tangent)

    def apply_to_camera(self, c2w: torch.Tensor, index: int) -> torch.Tensor:
        """c2w [3,4] of view `index` -> the corrected [4,4] (`camera.camera_to_worlds @ adj`)."""
        c2w = to4x4(c2w)
        if self.mode == "off":
            return c2w
        return c2w @ to4x4(self([index]))[0]

    def regulariser(self) -> torch.Tensor:
        """`camera_opt_regularizer` of get_loss_dict (:125-133)."""
        p = self.pose_adjustment
        return p[:, :3].norm(dim=-1).mean() * self.trans_l2_penalty + p[:, 3:].norm(dim=-1).mean() * self.rot_l2_penalty

    def metrics(self) -> Dict[str, torch.Tensor]:
        """get_metrics_dict (:139-143)."""
        if self.mode == "off":
            return {}
        p = self.pose_adjustment
        return {"camera_opt_translation": p[:, :3].norm(), "camera_opt_rotation": p[:, 3:].norm()}


class PosedCameras:
    """The training cameras as camera-to-world matrices plus intrinsics, and the per-step `CameraTensors` of a view
    with the optimizer's correction applied (differentiable with respect to `pose_adjustment`)."""

    def __init__(self, cams_np, device, true_cams_np=None):
        self.device = device
        self.c2w = torch.from_numpy(np.stack([c2w_from_viewmat(c.viewmat) for c in cams_np])).to(device)
        true = cams_np if true_cams_np is None else true_cams_np
        self.c2w_true = torch.from_numpy(np.stack([c2w_from_viewmat(c.viewmat) for c in true])).to(device)
        self._proj = {}

    def proj(self, cam: CameraTensors) -> torch.Tensor:
        key = (cam.width, cam.height, cam.fx, cam.fy)
        if key not in self._proj:
            fovx, fovy = 2.0 * math.atan(cam.width / (2.0 * cam.fx)), 2.0 * math.atan(cam.height / (2.0 * cam.fy))
            self._proj[key] = projection_matrix(0.001, 1000.0, fovx, fovy, self.device)
        return self._proj[key]

    def camera(self, opt: CameraOptimizer, v: int, like: CameraTensors) -> CameraTensors:
        """View `v` at `like`'s resolution and intrinsics, its pose corrected by `opt`."""
        viewmat, projmat, campos = view_matrices(opt.apply_to_camera(self.c2w[v], v), self.proj(like))
        return CameraTensors(like.width, like.height, like.fx, like.fy, like.cx, like.cy, viewmat, projmat,
                             campos.detach(), like.scalars, like.model)

    @torch.no_grad()
    def pose_errors(self, opt: Optional[CameraOptimizer]):
        """-> (rotation error in degrees, translation error in scene units): means over the views of the angle and
        the distance between the corrected and the true camera-to-world."""
        rot, trans = [], []
        for v in range(self.c2w.shape[0]):
            c = to4x4(self.c2w[v]) if opt is None else opt.apply_to_camera(self.c2w[v], v)
            Rd = c[:3, :3].double().T @ self.c2w_true[v, :3, :3].double()
            skew = torch.stack([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]]).norm() / 2.0  # sin
            rot.append(math.degrees(math.atan2(float(skew), float((Rd.trace() - 1.0) / 2.0))))
            trans.append(float((c[:3, 3] - self.c2w_true[v, :3, 3]).norm()))
        return float(np.mean(rot)), float(np.mean(trans))


def perturb_cameras(cams_np, sigma_trans: float, sigma_rot: float, seed: int):
    """`TrainConfig.pose_noise`: every camera's pose moved once by a rigid error -- a translation ~ N(0, sigma_trans^2)
    per axis in scene units and a rotation about a random axis by an angle ~ N(0, sigma_rot^2) radians, both in the
    camera's own frame -- standing in for COLMAP's.  Returns new `scene.Camera`s; intrinsics unchanged."""
    from .scene import Camera
    from .scene import projection_matrix as _scene_projection

    if sigma_trans == 0.0 and sigma_rot == 0.0:
        return list(cams_np)
    rng = np.random.default_rng(seed)
    out = []
    for c in cams_np:
        axis = rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        ang = rng.standard_normal() * sigma_rot
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        dR = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
        V = np.asarray(c.viewmat, np.float64).copy()
        V[:3, :3] = dR @ V[:3, :3]
        V[:3, 3] = dR @ V[:3, 3] + rng.standard_normal(3) * sigma_trans
        V = V.astype(np.float32)
        fovx, fovy = 2.0 * math.atan(c.width / (2.0 * c.fx)), 2.0 * math.atan(c.height / (2.0 * c.fy))
        P = _scene_projection(0.001, 1000.0, fovx, fovy) @ V
        out.append(Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, V, P.astype(np.float32), c.model))  # (the pose moves, the camera model stays)
    return out
