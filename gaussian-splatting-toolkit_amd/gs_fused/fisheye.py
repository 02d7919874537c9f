"""The equidistant fisheye camera inside the projection.

gsplat's ``camera_model="fisheye"`` with an ideal lens (every distortion coefficient of ``OPENCV_FISHEYE`` zero): a
point at polar angle ``theta`` from the optical axis lands ``f * theta`` pixels from the principal point.  Only the
projection knows the camera -- the pixel centre and the EWA Jacobian (csrc/project.hip's header states the rule); the
tile boxes, the sort, both compositing directions and the loss heads see ``xys``, ``conics``, ``radii``, ``depths`` and
``num_tiles_hit`` and nothing else.
"""
from typing import Optional

from torch import Tensor
from torch.autograd import Function

import rasterizer.cuda as _C

CAMERA_MODELS = ("pinhole", "fisheye")


def check_camera_model(model: str) -> str:
    if model not in CAMERA_MODELS:
        raise ValueError(f"camera model must be one of {CAMERA_MODELS}, got {model!r}")
    return model


class _ProjectGaussiansFisheye(Function):
    """forward(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, H, W, block_width, opacities,
    clip_thresh) -> (xys, depths, radii, conics, compensation, num_tiles_hit, cov3d[, opacities_aa])"""

    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
                block_width, opacities, clip_thresh):
        n = means3d.shape[-2]
        if n < 1 or means3d.shape[-1] != 3:
            raise ValueError(f"Invalid shape for means3d: {means3d.shape}")
        camera = (viewmat, projmat, fx, fy, cx, cy, img_height, img_width)
        cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa = \
            _C.project_gaussians_forward_fisheye(n, means3d, scales, glob_scale, quats, *camera, block_width,
                                                 clip_thresh, opacities)
        ctx.aa = opacities is not None
        if ctx.aa:  # the opacity the coming rasterize_gaussians receives, as project_gaussians_antialiased announces it
            from rasterizer.ahead import announce_opacity

            announce_opacity(opacities_aa)
        # (no lists are queued ahead of time here: rasterizer/ahead.py does not know this projection)
        ctx.static = (n, glob_scale) + camera[2:]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii, num_tiles_hit)
        saved = (means3d, scales, quats, viewmat, projmat, cov3d, radii, conics, compensation)
        ctx.save_for_backward(*(saved + ((opacities,) if ctx.aa else ())))
        out = (xys, depths, radii, conics, compensation, num_tiles_hit, cov3d)
        return out + ((opacities_aa,) if ctx.aa else ())

    @staticmethod
    def backward(ctx, g_xys, g_depths, _g_radii, g_conics, g_compensation, _g_tiles, _g_cov3d, g_opacities_aa=None):
        means3d, scales, quats, viewmat, projmat, cov3d, radii, conics, compensation = ctx.saved_tensors[:9]
        n, glob_scale, fx, fy, cx, cy, img_height, img_width = ctx.static
        grads = _C.project_gaussians_backward_fisheye(
            n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width, cov3d,
            radii, conics, compensation, ctx.saved_tensors[9] if ctx.aa else None, g_xys, g_depths, g_conics,
            g_compensation, g_opacities_aa if ctx.aa else None, trusted=True)
        g_means, g_scales, g_quats, g_opacities = grads[2:]  # (v_cov2d, v_cov3d) come first and stay internal
        # slots: means3d, scales, glob_scale, quats, viewmat, projmat, seven scalars, opacities, clip_thresh
        return (g_means, g_scales, None, g_quats, None, None) + (None,) * 7 + (g_opacities, None)


def project_gaussians_fisheye(means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor, viewmat: Tensor,
                              projmat: Tensor, fx: float, fy: float, cx: float, cy: float, img_height: int,
                              img_width: int, block_width: int, opacities: Optional[Tensor] = None,
                              clip_thresh: float = 0.01):
    """`rasterizer.project_gaussians` through an equidistant fisheye camera: ``xy = f * theta * (tx, ty) / r + c - 0.5``
    with ``theta = atan2(r, tz)``, the EWA Jacobian of that map, no clamp of the centre; Gaussians with camera
    ``z <= clip_thresh`` are culled, so the polar angle stays below 90 degrees; ``depths`` is the camera ``z``.
    One autograd node.  Returns `project_gaussians`' seven outputs ``(xys, depths, radii, conics, compensation,
    num_tiles_hit, cov3d)``; with ``opacities`` ([N] or [N,1], sigmoid()'d) an eighth output ``opacities_aa = opacities
    * compensation`` follows -- the antialiased mode's opacity, announced to ``rasterize_gaussians`` as
    `project_gaussians_antialiased` announces it.  Differentiable w.r.t. ``means3d``, ``scales``, ``quats`` and
    ``opacities``.  ``projmat`` is accepted for the sake of the common signature and not read.  There are no camera
    gradients: a ``viewmat`` or ``projmat`` that requires one raises ValueError, as do CPU tensors.  Tile lists are not
    built ahead of time behind this op."""
    assert block_width > 1 and block_width <= 16, "block_width must be between 2 and 16"
    for t, nm in ((means3d, "means3d"), (scales, "scales"), (quats, "quats"), (viewmat, "viewmat"),
                  (projmat, "projmat")) + (() if opacities is None else ((opacities, "opacities"),)):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise ValueError(f"project_gaussians_fisheye: {nm} must be a tensor on the GPU (there is no CPU path)")
    for t, nm in ((viewmat, "viewmat"), (projmat, "projmat")):
        if t.requires_grad:
            raise ValueError(f"project_gaussians_fisheye: {nm} requires a gradient, and the fisheye projection has no "
                             "camera gradients (pose refinement is pinhole only)")
    if opacities is not None and (opacities.dim() not in (1, 2) or opacities.numel() != means3d.shape[-2]):
        raise ValueError(f"opacities [N] or [N,1] expected, got {tuple(opacities.shape)}")
    t = [x.contiguous() for x in (means3d, scales, quats, viewmat, projmat)]
    return _ProjectGaussiansFisheye.apply(t[0], t[1], glob_scale, t[2], t[3], t[4], fx, fy, cx, cy, img_height,
                                          img_width, block_width,
                                          None if opacities is None else opacities.contiguous(), clip_thresh)
