"""RGB and a depth image from ONE compositing pass.

When a depth image is wanted the models composite twice per view
(gs_toolkit/models/vanilla_gs.py:822-855, depth_gs.py:330-363):

    rgb, alpha = rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, rgbs, opacities, H, W, B,
                                     background=background, return_alpha=True)
    depth_im = rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, depths[:, None].repeat(1, 3),
                                   opacities, H, W, B, background=torch.zeros(3))[..., 0:1]

i.e. two full forward and two full backward passes over the same sorted lists (the
list building is shared through the rasterizer's cache, the compositing is not).
`rasterize_gaussians_rgbd` composites a fourth channel in the same pass:

    rgb, alpha, depth_im = rasterize_gaussians_rgbd(xys, depths, radii, conics, num_tiles_hit, rgbs, depths,
                                                    opacities, H, W, background=background)

Same values (the RGB image is bit-identical, the extra image equals channel 0 of the
second pass) and the same gradients; block width 16 only.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor
from torch.autograd import Function

import rasterizer.cuda as _C
from rasterizer.rasterize import AbsgradOf, _is_two, backward_16px, composite_lists, is_deterministic

_f32 = torch.float32
BLOCK = 16


class _RasterizeRGBD(Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, num_tiles_hit, colors, extra, opacity, img_height, img_width,
                background, extra_background, absgrad_of=None):
        n = xys.size(0)
        tile_bounds = ((img_width + BLOCK - 1) // BLOCK, (img_height + BLOCK - 1) // BLOCK, 1)
        img_size = (img_width, img_height, 1)
        dev = xys.device

        # alpha = 1 - T and the backward's cleared accumulators come out of the compositing launch
        acc = None
        if any(ctx.needs_input_grad[i] for i in (0, 3, 5, 6, 7)) and not is_deterministic():
            acc = _C.backward_accumulators(n, 4, dev)

        def composite(ids, bins):  # -> (img, extra image, final_Ts, final_idx, alpha), as both rounds together
            return _C.rasterize_forward_rgbd(tile_bounds, img_size, ids, bins, xys, conics, colors, extra, opacity,
                                             background, extra_background, want_alpha=True, zero=acc)

        # deep scenes: lists in two segments, compositing in two rounds (rasterizer/rasterize.py, "two-round lists")
        state = []

        def round1(ids, bins1, flags):
            with torch.cuda.device(dev):
                state[:] = [torch.empty((img_height, img_width, 3), dtype=_f32, device=dev),
                            torch.empty((img_height, img_width), dtype=_f32, device=dev),
                            torch.empty((img_height, img_width), dtype=_f32, device=dev),
                            torch.empty((img_height, img_width), dtype=torch.int32, device=dev),
                            torch.empty((img_height, img_width), dtype=_f32, device=dev), flags]
            _C.rasterize_forward_round(1, tile_bounds, img_size, ids, bins1, 0, xys, conics, colors, extra, opacity,
                                       background, extra_background, state[0], state[1], state[2], state[3], flags,
                                       out_alpha=state[4], zero=acc)

        def round2(ids, aux):
            _C.rasterize_forward_round(2, tile_bounds, img_size, ids, aux[1], aux[2], xys, conics, colors, extra,
                                       opacity, background, extra_background, state[0], state[1], state[2], state[3],
                                       state[5], out_alpha=state[4])
            return tuple(state[:5])

        lists, outputs = composite_lists(xys, depths, radii, conics, num_tiles_hit, opacity, img_height, img_width,
                                         BLOCK, composite, round1, round2)
        num_intersects, ids, bins, aux = lists
        if outputs is None:
            img = torch.ones(img_height, img_width, 3, device=dev) * background
            ext = torch.full((img_height, img_width), float(extra_background), device=dev)
            # final_Ts = 0, i.e. alpha = 1, for a view with nothing on screen: the quirk of
            # `rasterize_gaussians(return_alpha=True)` (rasterize.py:119-127), kept so that the
            # fused and the two-pass route agree (tests/test_gpu_api.py::test_empty_view_*)
            Ts = torch.zeros(img_height, img_width, device=dev)
            idx = torch.zeros(img_height, img_width, dtype=torch.int32, device=dev)
            ids = torch.zeros(0, dtype=torch.int32, device=dev)
            bins = torch.zeros(0, 2, dtype=torch.int32, device=dev)
            acc = aux = None
            alpha = 1 - Ts
        else:
            img, ext, Ts, idx, alpha = outputs
        ctx.accumulators = acc
        ctx.absgrad_of = absgrad_of  # (rasterizer.rasterize.AbsgradOf: the caller's `xys`, or None)
        ctx.det = aux if (is_deterministic() and aux is not None) else None
        ctx.two = (aux[1], aux[2]) if _is_two(aux) else None
        ctx.set_materialize_grads(False)
        ctx.meta = (img_height, img_width, num_intersects, float(extra_background))
        ctx.save_for_backward(ids, bins, xys, conics, colors, extra, opacity, background, Ts, idx)
        return img, alpha, ext

    @staticmethod
    def backward(ctx, v_img, v_alpha, v_ext):
        ids, bins, xys, conics, colors, extra, opacity, background, Ts, idx = ctx.saved_tensors
        H, W, num_intersects, ebg = ctx.meta
        v_xy, v_conic, v_colors, v_extra, v_opacity = backward_16px(
            ctx, num_intersects, H, W, ids, bins, xys, conics, colors, extra, opacity, background, ebg, Ts, idx,
            v_img, v_ext, v_alpha)
        return (v_xy, None, None, v_conic, None, v_colors, v_extra, v_opacity) + (None,) * 5


def rasterize_gaussians_rgbd(xys: Tensor, depths: Tensor, radii: Tensor, conics: Tensor, num_tiles_hit: Tensor,
                             colors: Tensor, extra: Tensor, opacity: Tensor, img_height: int, img_width: int,
                             background: Optional[Tensor] = None, extra_background: float = 0.0,
                             absgrad: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (rgb [H,W,3], alpha [H,W], extra image [H,W,1]): `rasterize_gaussians(..., colors,
    return_alpha=True)` and the channel-0 image of `rasterize_gaussians(..., extra repeated
    as 3 colours, background=extra_background)` from one pass.  ``extra``: [N] or [N,1]
    (typically ``depths``).  Differentiable w.r.t. xys, conics, colors, extra, opacity.
    ``absgrad``: as in :func:`rasterizer.rasterize_gaussians` -- every backward leaves ``xys.absgrad`` [N,2]."""
    if colors.dim() != 2 or colors.shape[1] != 3:
        raise ValueError("colors must have dimensions (N, 3)")
    if extra.numel() != xys.shape[0]:
        raise ValueError("extra must hold one scalar per Gaussian")
    if background is None:
        background = torch.ones(3, dtype=_f32, device=colors.device)
    for t, nm in ((xys, "xys"), (conics, "conics"), (colors, "colors"), (extra, "extra"), (opacity, "opacity"),
                  (background, "background")):
        if not t.is_cuda:
            raise RuntimeError(f"{nm} must be a CUDA tensor")
    img, alpha, ext = _RasterizeRGBD.apply(
        xys.contiguous(), depths.contiguous(), radii.contiguous(), conics.contiguous(), num_tiles_hit.contiguous(),
        colors.contiguous().float(), extra.contiguous().float(), opacity.contiguous(), int(img_height),
        int(img_width), background.contiguous().float(), float(extra_background),
        AbsgradOf(xys) if absgrad else None)
    return img, alpha, ext[..., None]
