"""Depth distortion and median depth of a view, on csrc/distortion.hip (the rule is stated in
include/gsraster.h).  What 2DGS, GOF, RaDe-GS, PGSR and gsplat (`distloss`, `render_mode="...+median"`) share:

    depth_distortion(xys, depths, radii, conics, num_tiles_hit, values, opacities, H, W)
                                               -> (distortion [H,W], median [H,W]); gradients to xys, conics,
                                                  values and opacities through the distortion
    distortion_loss(distortion, mask=None)     scalar: the mean over ALL pixels

``distortion`` is the Mip-NeRF-360 term ``sum_i sum_j w_i w_j |z_i - z_j|`` per pixel in its O(n) form, ``median`` the
value of the last contributing Gaussian whose incoming transmittance exceeds 0.5.  One walk of its own over the tile
lists the rasterizer's cache holds for the view (the term is quadratic in the blending weights: no further channel of
the compositing passes), forward and backward.  The backward sums with float atomics: not bit-reproducible, refused
in deterministic mode.  CUDA tensors and 16 x 16 tiles only; no CPU fallback."""
import torch
from torch import Tensor
from torch.autograd import Function

import rasterizer.cuda as _C
from rasterizer import rasterize as _R

_f32 = torch.float32


class _DepthDistortion(Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, values, opacities, img_height, img_width):
        H, W = int(img_height), int(img_width)
        tile_bounds = ((W + 15) // 16, (H + 15) // 16, 1)
        xy, co, va, op = (t.detach().contiguous() for t in (xys, conics, values, opacities))

        def composite(ids, bins):
            return _C.distortion_forward(tile_bounds, (W, H, 1), ids, bins, xy, co, op, va)

        # single-segment lists: a cache hit behind the view's RGB pass (two-segment lists are built again as one)
        lists, outputs = _R.composite_lists(xys, depths, radii, conics, num_tiles_hit, opacities, H, W, 16, composite,
                                            round1=None)
        ctx.size = (H, W)
        ctx.shapes = (values.shape, opacities.shape)
        if outputs is None:  # nothing on screen: no launch
            ctx.empty = True
            distortion, median = (torch.zeros((H, W), dtype=_f32, device=xys.device) for _ in range(2))
            ctx.mark_non_differentiable(median)
            return distortion, median
        distortion, median, vsum, final_Ts, final_idx = outputs
        ctx.empty = False
        ctx.save_for_backward(lists.ids, lists.bins, xy, co, op, va, vsum, final_Ts, final_idx)
        ctx.mark_non_differentiable(median)
        return distortion, median

    @staticmethod
    def backward(ctx, v_distortion, _v_median):
        H, W = ctx.size
        if ctx.empty or v_distortion is None:
            return (None,) * 9
        ids, bins, xy, co, op, va, vsum, final_Ts, final_idx = ctx.saved_tensors
        v_xy, v_conic, v_opacity, v_values = _C.distortion_backward(
            H, W, ids, bins, xy, co, op, va, vsum, final_Ts, final_idx, v_distortion.to(_f32))
        return (v_xy, None, None, v_conic, None, v_values.view(ctx.shapes[0]), v_opacity.view(ctx.shapes[1]), None,
                None)


def depth_distortion(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, num_tiles_hit: Tensor,
                     values: Tensor, opacities: Tensor, img_height: int, img_width: int, block_width: int = 16):
    """-> ``(distortion [H,W], median [H,W])`` of the view whose projection outputs these are.

    ``values`` ([N] or [N,1]) is one scalar per Gaussian: the projection's ``depths``, or a monotone map of them (the
    trainer's ``far / (far - near) (1 - near / depth)``); the lists are ordered by ``depths`` either way.
    ``opacities`` is what the view's RGB pass composited with (for ``rasterize_mode="antialiased"``: the compensated
    ones).  With ``T_i`` the transmittance in front of contributing entry i, ``w_i = alpha_i T_i``:

        distortion = 2 sum_i w_i (z_i A_{i-1} - B_{i-1}),  A_i = sum_{j<=i} w_j,  B_i = sum_{j<=i} w_j z_j
        median     = z_i of the last contributing entry with T_i > 0.5 (0 where nothing contributes)

    under the forward compositing's skip, clamp (0.999) and stop rule.  The distortion is differentiable w.r.t. ``xys``,
    ``conics``, ``values`` and ``opacities`` (the gradient of exactly this forward); the median is marked
    non-differentiable.  Called after ``rasterize_gaussians`` for the same view, the tile lists are that call's (a cache
    hit).  A view with nothing on screen launches nothing and returns zeros.

    ValueError, naming the option: ``block_width`` other than 16; CPU tensors; deterministic mode
    (``rasterizer.rasterize.set_deterministic``) -- the backward's sums are atomic."""
    if int(block_width) != 16:
        raise ValueError(f"depth_distortion: block_width must be 16 (the walk is written for 16 x 16 tiles), got "
                         f"{block_width}")
    for name, t in (("xys", xys), ("depths", depths), ("radii", radii), ("conics", conics),
                    ("num_tiles_hit", num_tiles_hit), ("values", values), ("opacities", opacities)):
        if not isinstance(t, Tensor):
            raise RuntimeError(f"depth_distortion: {name} must be a tensor")
        if not t.is_cuda:
            raise ValueError(f"depth_distortion: {name} is a CPU tensor; the op runs on CUDA tensors only (no CPU "
                             f"fallback)")
    if _R.is_deterministic():
        raise ValueError("depth_distortion: not available in deterministic mode (rasterizer.rasterize.set_deterministic): "
                         "its backward sums with float atomics and is not bit-reproducible")
    n = xys.shape[0]
    if values.numel() != n or opacities.numel() != n:
        raise ValueError(f"depth_distortion: values and opacities must hold one scalar per Gaussian ({n}), got "
                         f"{tuple(values.shape)} and {tuple(opacities.shape)}")
    if int(img_height) < 1 or int(img_width) < 1:
        raise ValueError("depth_distortion: empty image")
    return _DepthDistortion.apply(xys, depths, radii, conics, num_tiles_hit, values, opacities, img_height, img_width)


def distortion_loss(distortion: Tensor, mask=None) -> Tensor:
    """The mean of the distortion map over ALL its pixels.  ``mask`` ([H,W] or [H,W,1]; float32, bool or uint8) is
    multiplied in and the mean stays over all pixels, as in the project's other masked heads."""
    if distortion.dim() == 3 and distortion.shape[-1] == 1:
        distortion = distortion[..., 0]
    if distortion.dim() != 2:
        raise ValueError(f"expected distortion [H,W] (or [H,W,1]), got {tuple(distortion.shape)}")
    if mask is not None:
        from .loss import _mask_arg

        distortion = distortion * _mask_arg(mask, int(distortion.shape[0]), int(distortion.shape[1]), distortion)
    return distortion.mean()
