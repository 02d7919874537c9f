"""EWA projection of 3-D Gaussians to screen space (differentiable).

Same call surface as the reference's ``rasterizer/project_gaussians.py``
(``project_gaussians`` :12-76, autograd node :79-232): argument order, the 7-tuple
that comes back, and which inputs receive gradients.  The arithmetic is in
``csrc/project.hip``.
"""
from typing import Tuple

from torch import Tensor
from torch.autograd import Function

import rasterizer.cuda as _C


def _ahead(*args):
    from rasterizer.ahead import speculate_lists  # (imported late: the package is still being imported)

    speculate_lists(*args)


_Out = Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]


def backward_chain(static, saved, needs_viewmat, needs_projmat, g_xys, g_depths, g_conics, g_compensation,
                    opacities=None, g_opacities_aa=None):
    """The backward of every projection node of the package (this module's two, gs_fused.project_gaussians_cropped):
    -> (g_means, g_scales, g_quats, g_viewmat, g_projmat, g_opacities).  `saved`: (means3d, scales, quats, viewmat,
    projmat, cov3d, radii, conics, compensation) of the forward; `static`: (n, glob_scale, fx, fy, cx, cy, H, W).
    With `opacities` the node also returned ``opacities * compensation``: its cotangent `g_opacities_aa` joins the
    chain (gsr_project_backward_aa) and `g_opacities` comes back; else `g_opacities` is None.  The camera gradients
    are a pass of their own (two more launches), run only where one of the matrices requires a gradient, on the
    compensation's cotangent the chain took."""
    means3d, scales, quats, viewmat, projmat, cov3d, radii, conics, compensation = saved
    n, glob_scale, fx, fy, cx, cy, img_height, img_width = static
    pose = needs_viewmat or needs_projmat
    g_opacities = None
    if opacities is None:
        grads = _C.project_gaussians_backward(
            n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
            cov3d, radii, conics, compensation, g_xys, g_depths, g_conics, g_compensation, trusted=True)
        g_means, g_scales, g_quats = grads[2:]  # (v_cov2d, v_cov3d) come first and stay internal
    else:
        grads = _C.project_gaussians_backward_aa(
            n, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, img_height, img_width,
            cov3d, radii, conics, compensation, opacities, g_xys, g_depths, g_conics, g_compensation, g_opacities_aa,
            want_v_compensation=pose, trusted=True)
        g_means, g_scales, g_quats, g_opacities, g_compensation = grads[2:]
    g_viewmat = g_projmat = None
    if pose:
        v_viewmat, g_projmat = _C.project_gaussians_backward_pose(
            n, means3d, viewmat, projmat, fx, fy, img_height, img_width, cov3d, radii, conics, compensation,
            g_xys, g_depths, g_conics, g_compensation, trusted=True)
        if needs_viewmat:  # in the shape that was passed: [3,4], or [4,4] with a zero last row
            g_viewmat = viewmat.new_zeros(viewmat.shape)
            g_viewmat.view(-1)[:12] = v_viewmat.view(-1)
        if not needs_projmat:
            g_projmat = None
    return g_means, g_scales, g_quats, g_viewmat, g_projmat, g_opacities


class _ProjectGaussians(Function):
    """forward(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, H, W,
    block_width, clip_thresh) -> (xys, depths, radii, conics, compensation, num_tiles_hit, cov3d)"""

    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
                img_height, img_width, block_width, clip_thresh=0.01):
        n = means3d.shape[-2]
        if n < 1 or means3d.shape[-1] != 3:
            raise ValueError(f"Invalid shape for means3d: {means3d.shape}")
        camera = (viewmat, projmat, fx, fy, cx, cy, img_height, img_width)
        # the native tuple starts with cov3d, the public one ends with it
        cov3d, xys, depths, radii, conics, compensation, num_tiles_hit = _C.project_gaussians_forward(
            n, means3d, scales, glob_scale, quats, *camera, block_width, clip_thresh)
        # everything this view's tile lists depend on exists now: start building them on the side stream, next to
        # whatever the caller does before it calls rasterize_gaussians (rasterize.py, "lists built ahead of time")
        # (the compensation and this node go along: the antialiased mode's opacity is a product with it, ahead.py)
        ctx.gsr_compensation_output = 4
        _ahead(xys, depths, radii, conics, num_tiles_hit, img_height, img_width, block_width, compensation, ctx)
        ctx.static = (n, glob_scale) + camera[2:]
        # Outputs nobody differentiates through (depths, compensation, cov3d in an RGB
        # pass) reach backward() as None rather than as N-sized zero tensors; the
        # kernel treats a missing cotangent as zero.
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii, num_tiles_hit)
        ctx.save_for_backward(means3d, scales, quats, viewmat, projmat, cov3d, radii, conics, compensation)
        return xys, depths, radii, conics, compensation, num_tiles_hit, cov3d

    @staticmethod
    def backward(ctx, g_xys, g_depths, _g_radii, g_conics, g_compensation, _g_tiles, _g_cov3d):
        g_means, g_scales, g_quats, g_viewmat, g_projmat, _ = backward_chain(
            ctx.static, ctx.saved_tensors, ctx.needs_input_grad[4], ctx.needs_input_grad[5], g_xys, g_depths, g_conics,
            g_compensation)
        # slots: means3d, scales, glob_scale, quats, viewmat, projmat, then the eight scalar arguments
        return (g_means, g_scales, None, g_quats, g_viewmat, g_projmat) + (None,) * 8


def project_gaussians(means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor, viewmat: Tensor,
                      projmat: Tensor, fx: float, fy: float, cx: float, cy: float, img_height: int,
                      img_width: int, block_width: int, clip_thresh: float = 0.01) -> _Out:
    """Project N Gaussians; differentiable w.r.t. ``means3d``, ``scales`` and ``quats``, and -- beyond the
    reference, whose backward returns None for them -- w.r.t. ``viewmat`` and ``projmat`` where they require a
    gradient (``rasterizer.cuda.project_gaussians_backward_pose``: the derivative of the projection alone; the SH
    op has no gradient with respect to the view directions, so the colour's view dependence moves no camera).

    means3d [N,3]; scales [N,3] (already exponentiated) times ``glob_scale``; quats
    [N,4] as (w,x,y,z); viewmat world->camera (row-major, top 3x4 used); projmat the
    full 4x4 ``P @ V``; fx, fy, cx, cy in pixels; tiles of ``block_width`` (2..16)
    pixels; Gaussians with camera ``z <= clip_thresh`` are culled.

    Returns ``(xys [N,2], depths [N], radii [N] i32, conics [N,3], compensation [N],
    num_tiles_hit [N] i32, cov3d [N,6])``; culled Gaussians have ``radii == 0`` and
    ``num_tiles_hit == 0`` and zeros elsewhere."""
    assert block_width > 1 and block_width <= 16, "block_width must be between 2 and 16"
    tensors = [t.contiguous() for t in (means3d, scales, quats, viewmat, projmat)]
    return _ProjectGaussians.apply(tensors[0], tensors[1], glob_scale, tensors[2], tensors[3], tensors[4],
                                   fx, fy, cx, cy, img_height, img_width, block_width, clip_thresh)


class _ProjectGaussiansAntialiased(Function):
    """forward(means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy, H, W, block_width, opacities,
    clip_thresh) -> (xys, depths, radii, conics, opacities_aa, num_tiles_hit, cov3d)"""

    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, viewmat, projmat, fx, fy, cx, cy,
                img_height, img_width, block_width, opacities, clip_thresh=0.01):
        n = means3d.shape[-2]
        if n < 1 or means3d.shape[-1] != 3:
            raise ValueError(f"Invalid shape for means3d: {means3d.shape}")
        camera = (viewmat, projmat, fx, fy, cx, cy, img_height, img_width)
        cov3d, xys, depths, radii, conics, compensation, num_tiles_hit, opacities_aa = _C.project_gaussians_forward_aa(
            n, means3d, scales, glob_scale, quats, *camera, block_width, clip_thresh, opacities)
        # the opacity the coming rasterize_gaussians receives exists already: the lists built ahead of time are built
        # for it (autograd provenance cannot show it -- it is this node's output)
        from rasterizer.ahead import announce_opacity

        announce_opacity(opacities_aa)
        _ahead(xys, depths, radii, conics, num_tiles_hit, img_height, img_width, block_width)
        ctx.static = (n, glob_scale) + camera[2:]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(radii, num_tiles_hit)
        ctx.save_for_backward(means3d, scales, quats, viewmat, projmat, cov3d, radii, conics, compensation, opacities)
        return xys, depths, radii, conics, opacities_aa, num_tiles_hit, cov3d

    @staticmethod
    def backward(ctx, g_xys, g_depths, _g_radii, g_conics, g_opacities_aa, _g_tiles, _g_cov3d):
        g_means, g_scales, g_quats, g_viewmat, g_projmat, g_opacities = backward_chain(
            ctx.static, ctx.saved_tensors[:9], ctx.needs_input_grad[4], ctx.needs_input_grad[5], g_xys, g_depths,
            g_conics, None, opacities=ctx.saved_tensors[9], g_opacities_aa=g_opacities_aa)
        # slots: means3d, scales, glob_scale, quats, viewmat, projmat, seven scalars, opacities, clip_thresh
        return (g_means, g_scales, None, g_quats, g_viewmat, g_projmat) + (None,) * 7 + (g_opacities, None)


def project_gaussians_antialiased(means3d: Tensor, scales: Tensor, glob_scale: float, quats: Tensor, viewmat: Tensor,
                                  projmat: Tensor, fx: float, fy: float, cx: float, cy: float, img_height: int,
                                  img_width: int, block_width: int, opacities: Tensor,
                                  clip_thresh: float = 0.01) -> _Out:
    """`project_gaussians` for the antialiased rasterize mode: one autograd node in place of the model's projection
    call plus its ``opacities * comp[:, None]`` line (vanilla_gs.py:815-816).

    Arguments as `project_gaussians`, plus ``opacities`` [N] or [N,1] (already sigmoid()'d).  Returns ``(xys, depths,
    radii, conics, opacities_aa, num_tiles_hit, cov3d)``: where `project_gaussians` returns the compensation, this
    returns ``opacities * compensation`` in the shape of ``opacities`` -- the product and both of its cotangents are
    formed inside the projection kernels.  Differentiable w.r.t. ``means3d``, ``scales``, ``quats``, ``opacities``
    and, where they require a gradient, ``viewmat`` and ``projmat``.  The output is announced to
    ``rasterize_gaussians`` (`rasterizer.rasterize.announce_opacity`): tile lists built ahead of time are built for it."""
    assert block_width > 1 and block_width <= 16, "block_width must be between 2 and 16"
    if opacities.dim() not in (1, 2) or opacities.numel() != means3d.shape[-2]:
        raise ValueError(f"opacities [N] or [N,1] expected, got {tuple(opacities.shape)}")
    tensors = [t.contiguous() for t in (means3d, scales, quats, viewmat, projmat, opacities)]
    return _ProjectGaussiansAntialiased.apply(tensors[0], tensors[1], glob_scale, tensors[2], tensors[3], tensors[4],
                                              fx, fy, cx, cy, img_height, img_width, block_width, tensors[5],
                                              clip_thresh)
