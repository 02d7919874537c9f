"""The oriented crop box of the toolkit's models, without their gathers.

``GaussianSplattingModel.get_outputs`` (gs_toolkit/models/vanilla_gs.py:703-757) computes ``crop_ids =
self.crop_box.within(self.means)`` outside training and gathers all six parameter tensors before it projects.  Here a
Gaussian outside the box is a CULLED Gaussian: the projection kernel tests the centre and lets it leave through the
exit of a clipped one (``radii == 0``), so N never changes and nothing is copied.

The rule (one device function, ``gsr_crop_inside`` in csrc/gsr_common.h; restated for the host in `CropBox.within`):
``crop`` is float32[16] = the world->box matrix ``A`` (3x4, row-major) | the half extents ``h = S / 2`` | 0;
``q_k = ((A_k0 x + A_k1 y) + A_k2 z) + A_k3`` with every product and sum rounded to float32 on its own; inside <=>
``-h_k < q_k < h_k`` for k = 0, 1, 2, strictly, as ``OrientedBox.within`` (gs_toolkit/data/scene_box.py:83-96).  A NaN
coordinate is outside; a zero extent keeps nothing.
"""
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch import Tensor
from torch.autograd import Function

import rasterizer.cuda as _C
from rasterizer.project_gaussians import backward_chain


def _host64(a, shape, name) -> np.ndarray:
    if isinstance(a, Tensor):
        a = a.detach().cpu().numpy()
    try:
        a = np.asarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"CropBox: {name} must be numbers") from None
    if a.shape != shape:
        raise ValueError(f"CropBox: {name} must have shape {shape}, got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"CropBox: {name} must be finite")
    return a.copy()


class CropBox:
    """``OrientedBox(R, T, S)`` of the toolkit (scene_box.py:74-108): a box of extents ``S`` whose frame is
    ``H = [[R, T], [0, 1]]`` in the world.  ``R`` need not be orthonormal: ``H`` is inverted as a general matrix, as the
    reference's ``torch.inverse`` does -- here in float64, the inverse then rounded to float32 once.  A singular ``H``
    raises ValueError."""

    def __init__(self, R, T, S):
        self.R = _host64(R, (3, 3), "R")
        self.T = _host64(T, (3,), "T")
        self.S = _host64(S, (3,), "S")
        H = np.eye(4, dtype=np.float64)
        H[:3, :3] = self.R
        H[:3, 3] = self.T
        try:
            inv = np.linalg.inv(H)
        except np.linalg.LinAlgError:
            raise ValueError("CropBox: [[R, T], [0, 1]] is singular") from None
        if not np.isfinite(inv).all():
            raise ValueError("CropBox: [[R, T], [0, 1]] is singular")
        v = np.zeros(16, dtype=np.float32)
        v[:12] = inv[:3, :].astype(np.float32).reshape(12)
        v[12:15] = (self.S / 2.0).astype(np.float32)
        self._values = v

    @staticmethod
    def from_params(pos: Sequence[float], rpy: Sequence[float], scale: Sequence[float]) -> "CropBox":
        """``OrientedBox.from_params`` (scene_box.py:98-108): ``R = Rz(yaw) Ry(pitch) Rx(roll)``, what viser's
        ``SO3.from_rpy_radians(roll, pitch, yaw)`` composes, in float64."""
        for v, nm in ((pos, "pos"), (rpy, "rpy"), (scale, "scale")):
            if len(tuple(v)) != 3:
                raise ValueError(f"CropBox.from_params: {nm} must hold three numbers")
        r, p, y = (float(a) for a in rpy)
        cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
        Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], np.float64)
        Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], np.float64)
        Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], np.float64)
        return CropBox((Rz @ Ry) @ Rx, pos, scale)

    def values(self) -> np.ndarray:
        """The sixteen float32 words the kernels read (a copy)."""
        return self._values.copy()

    def tensor(self, device) -> Tensor:
        """float32[16] on ``device``: what ``crop=`` takes everywhere."""
        return torch.from_numpy(self._values.copy()).to(device)

    def within(self, means: Tensor) -> Tensor:
        """bool [N]: which centres the box keeps.  On the GPU this is ``gsr_crop_mask`` -- the projection's own
        device function; on the host the same float32 operations in the same order (NumPy), bit for bit."""
        if means.dim() != 2 or means.shape[1] != 3:
            raise ValueError(f"means [N,3] expected, got {tuple(means.shape)}")
        if means.is_cuda:
            mask, _ = _C.crop_mask(means.detach().to(torch.float32).contiguous(), self.tensor(means.device),
                                   want_count=False)
            return mask.bool()
        p = means.detach().to(torch.float32).numpy()
        v = self._values
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        keep = np.ones(p.shape[0], dtype=bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(3):
                a = v[4 * k:4 * k + 4]
                q = ((a[0] * x + a[1] * y) + a[2] * z) + a[3]  # float32 throughout, each operation rounded
                h = v[12 + k]
                keep &= (q > -h) & (q < h)
        return torch.from_numpy(keep)


def _crop_tensor(crop, device) -> Tensor:
    """A `CropBox` or its float32[16] -> the tensor on ``device``."""
    if isinstance(crop, CropBox):
        return crop.tensor(device)
    if not isinstance(crop, Tensor) or crop.dtype != torch.float32 or crop.numel() != 16:
        raise ValueError("crop must be a gs_fused.CropBox or its float32[16] tensor")
    return crop.to(device).contiguous()


class _ProjectGaussiansCropped(Function):
    """forward(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, H, W, block_width, crop,
    opacities, clip_thresh) -> (xys, depths, radii, conics, compensation, num_tiles_hit, cov3d[, opacities_aa])"""

    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
                block_width, crop, opacities, clip_thresh):
        n = means3d.shape[-2]
        if n < 1 or means3d.shape[-1] != 3:
            raise ValueError(f"Invalid shape for means3d: {means3d.shape}")
        camera = (viewmat, projmat, fx, fy, cx, cy, img_height, img_width)
        cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa = \
            _C.project_gaussians_forward_crop(n, means3d, scales, glob_scale, quats, *camera, block_width, clip_thresh,
                                              crop, opacities)
        # (no lists are queued ahead of time here: rasterizer/ahead.py does not know this projection)
        ctx.static = (n, glob_scale) + camera[2:]
        ctx.aa = opacities is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii, num_tiles_hit)
        saved = (means3d, scales, quats, viewmat, projmat, cov3d, radii, conics, compensation)
        ctx.save_for_backward(*(saved + ((opacities,) if ctx.aa else ())))
        out = (xys, depths, radii, conics, compensation, num_tiles_hit, cov3d)
        return out + ((opacities_aa,) if ctx.aa else ())

    @staticmethod
    def backward(ctx, g_xys, g_depths, _g_radii, g_conics, g_compensation, _g_tiles, _g_cov3d, g_opacities_aa=None):
        # the uncropped backward entries (the chain every projection node of the package shares): they return zeros
        # wherever radii <= 0, which is where a cropped Gaussian is
        g_means, g_scales, g_quats, g_viewmat, g_projmat, g_opacities = backward_chain(
            ctx.static, ctx.saved_tensors[:9], ctx.needs_input_grad[4], ctx.needs_input_grad[5], g_xys, g_depths,
            g_conics, g_compensation, opacities=ctx.saved_tensors[9] if ctx.aa else None,
            g_opacities_aa=g_opacities_aa)
        # slots: means3d, scales, glob_scale, quats, viewmat, projmat, seven scalars, crop, opacities, clip_thresh
        return (g_means, g_scales, None, g_quats, g_viewmat, g_projmat) + (None,) * 8 + (g_opacities, None)


def project_gaussians_cropped(means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor, viewmat: Tensor,
                              projmat: Tensor, fx: float, fy: float, cx: float, cy: float, img_height: int,
                              img_width: int, block_width: int, crop, opacities: Optional[Tensor] = None,
                              clip_thresh: float = 0.01):
    """`rasterizer.project_gaussians` restricted to the oriented crop box ``crop`` (a `CropBox` or its float32[16] on
    the device): the model's ``crop_ids = self.crop_box.within(self.means)`` and six gathers (vanilla_gs.py:703-757)
    as a test inside the projection kernel.  Returns `project_gaussians`' seven outputs ``(xys, depths, radii, conics,
    compensation, num_tiles_hit, cov3d)`` with a Gaussian outside the box culled (``radii == 0``, zeros elsewhere,
    zero gradients); inside Gaussians get the uncropped op's bits.  With ``opacities`` ([N] or [N,1], sigmoid()'d) an
    eighth output ``opacities_aa = opacities * compensation`` follows: the antialiased mode's opacity, as
    `project_gaussians_antialiased` forms it.  Tile lists are not built ahead of time behind this op."""
    assert block_width > 1 and block_width <= 16, "block_width must be between 2 and 16"
    if opacities is not None and (opacities.dim() not in (1, 2) or opacities.numel() != means3d.shape[-2]):
        raise ValueError(f"opacities [N] or [N,1] expected, got {tuple(opacities.shape)}")
    crop = _crop_tensor(crop, means3d.device)
    t = [x.contiguous() for x in (means3d, scales, quats, viewmat, projmat)]
    return _ProjectGaussiansCropped.apply(t[0], t[1], glob_scale, t[2], t[3], t[4], fx, fy, cx, cy, img_height,
                                          img_width, block_width, crop,
                                          None if opacities is None else opacities.contiguous(), clip_thresh)


def crop_gaussians(params: Dict[str, Tensor], box, return_mask: bool = False):
    """The rows of every tensor of ``params`` whose centre (``params["means"]``, or ``"means3d"``) ``box`` keeps, in
    order -- what the model's six gathers return.  Mask and count come from ``gsr_crop_mask``; torch boolean indexing
    does the gather (one read-back for the sizes: export is not a hot path).  CPU tensors take `CropBox.within`."""
    key = "means" if "means" in params else "means3d"
    if key not in params:
        raise ValueError("crop_gaussians: params must hold 'means' (or 'means3d')")
    means = params[key]
    n = means.shape[0]
    for k, v in params.items():
        if not isinstance(v, Tensor) or v.dim() < 1 or v.shape[0] != n:
            raise ValueError(f"crop_gaussians: '{k}' must be a tensor of {n} rows")
    if means.is_cuda:
        mask8, count = _C.crop_mask(means.detach().to(torch.float32).contiguous(), _crop_tensor(box, means.device))
        mask = mask8.bool()
        kept = int(count.item())
    else:
        if not isinstance(box, CropBox):
            raise ValueError("crop_gaussians: host tensors take a gs_fused.CropBox")
        mask = box.within(means)
        kept = int(mask.sum())
    out = {k: v[mask.to(v.device)] for k, v in params.items()}
    if out[key].shape[0] != kept:
        raise RuntimeError(f"crop_gaussians: the mask keeps {out[key].shape[0]} rows, the count says {kept}")
    return (out, mask) if return_mask else out
