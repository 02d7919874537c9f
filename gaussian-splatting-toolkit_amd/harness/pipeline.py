"""The render call the toolkit's models make, reproduced outside the toolkit.

``render_view`` follows ``GaussianSplattingModel.get_outputs``
(gs_toolkit/models/vanilla_gs.py:765-855) / ``DepthGSModel.get_outputs``
(gs_toolkit/models/depth_gs.py:225-363) step by step, using only the public
``rasterizer`` API: project -> (retain xys grad) -> SH -> clamp(+0.5) ->
rasterize(return_alpha) -> optional second rasterisation of depths.
gs_toolkit itself cannot be imported in this image (tyro, jaxtyping, viser,
open3d ... are absent), so the contract is restated here for tests and bench.
"""
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from rasterizer.project_gaussians import project_gaussians
from rasterizer.rasterize import rasterize_gaussians
from rasterizer.sh import spherical_harmonics

BLOCK_WIDTH = 16  # vanilla_gs.py:762-764


@dataclass
class CameraTensors:
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    viewmat: torch.Tensor  # [4,4]
    projmat: torch.Tensor  # [4,4] = P @ V
    campos: torch.Tensor  # [3]

    # [fx, fy, cx, cy, width, height] on the device: the toolkit's `Cameras` keeps its intrinsics there and
    # `get_outputs` reads them back one `.item()` at a time (vanilla_gs.py:736-740,772-773) -- `caller_syncs="camera"`
    scalars: Optional[torch.Tensor] = None
    # "pinhole", or "fisheye": the equidistant camera (gs_fused.project_gaussians_fisheye; `projmat` is then not read)
    model: str = "pinhole"

    @staticmethod
    def from_numpy(cam, device) -> "CameraTensors":
        t = lambda a: torch.from_numpy(a).to(device)
        return CameraTensors(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                             t(cam.viewmat), t(cam.projmat), t(cam.campos),
                             torch.tensor([cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height], dtype=torch.float32,
                                          device=device), getattr(cam, "model", "pinhole"))


def render_view(
    means3d: torch.Tensor,      # [N,3]
    scales: torch.Tensor,       # [N,3] already exp()'d
    quats: torch.Tensor,        # [N,4] already normalised
    opacities: torch.Tensor,    # [N,1] already sigmoid()'d
    sh_coeffs,                  # [N,K,3] (features_dc ++ features_rest), or the pair
                                # (features_dc [N,3], features_rest [N,K-1,3]): no torch.cat (gs_fused)
    cam: CameraTensors,
    background: torch.Tensor,   # [3]
    sh_degree_to_use: int,
    rasterize_mode: str = "classic",
    render_depth: bool = False,
    retain_xys_grad: bool = False,
    clamp_rgb: bool = True,
    viewdirs: Optional[torch.Tensor] = None,  # normalised means3d - campos, if the caller already has them
    fused_depth: bool = False,  # RGB and depth image from one compositing pass (gs_fused.rasterize_gaussians_rgbd)
    sh_exchange=None,  # (parallel.GradientExchange, names, leaves) with names / leaves = ("features_dc",
                       # "features_rest") / those parameters, or ("sh_coeffs",) / ([N,K,3],): data parallel, the SH
                       # gradient is formed from the ranks' gathered colour cotangents (GradientExchange, `sh_views`)
    normalise_depth: bool = True,  # False: "depth" stays None and the caller takes the accumulated depth ("depth_acc")
                                   # and the alpha to gs_fused.depth_l1_loss, which normalises inside its kernels
    caller_syncs=False,  # True: block the host where the UNCHANGED models do -- `if (self.radii).sum() == 0`
                         # (vanilla_gs.py:784) and `assert (num_tiles_hit > 0).any()` (:811); "camera": also the
                         # intrinsics read back from the device ahead of the projection (:736-740, :772-773).
                         # False: the same ops with no read-back -- what a caller that WAS changed could do
    crop=None,  # a gs_fused.CropBox or its float32[16]: the model's crop box (vanilla_gs.py:703-757) as a test inside
                # the projection (gs_fused.project_gaussians_cropped) instead of six gathers.  A box that keeps nothing:
                # with `caller_syncs` the branch below returns what the reference returns for `crop_ids.sum() == 0`
                # (:750-757: background, depth 10, accumulation 0); without a read-back nobody can know, and the image
                # is what compositing nothing gives -- the background with alpha 0, depth 0
    absgrad: bool = False,  # the compositing backward also leaves `out["xys"].absgrad` [N,2] (rasterize_gaussians /
                            # rasterize_gaussians_rgbd, `absgrad=True`); with two passes (depth not fused) it is the
                            # RGB pass's: the colour image's share of the per-pixel gradient
    render_normals: bool = False,  # together with `render_depth`: `out["normals"]` [H,W,3], the alpha-blended,
                                   # un-normalised camera-space normals (gs_fused.gaussian_normals composited over a
                                   # zero background) -- a third compositing pass over the tile lists the rasterizer's
                                   # cache holds for this view.  Its gradient reaches `quats`, the opacities, the
                                   # conics and -- like every loss in 2DGS -- `xys`: it JOINS `xys.grad`, so the
                                   # densification statistics see the normal term as well.  CUDA tensors only
    render_distortion: bool = False,  # together with `render_depth`: `out["distortion"]` and `out["median_depth"]`
                                      # [H,W,1] (gs_fused.depth_distortion: the Mip-NeRF-360 distortion term per pixel
                                      # and the value at which the transmittance crosses 0.5) -- one more walk over
                                      # the cached tile lists.  The distortion's gradient reaches the opacities, the
                                      # conics, `distortion_values` and `xys` (it JOINS `xys.grad`); the median has
                                      # none.  CUDA tensors only, not in deterministic mode
    distortion_values=None,  # the scalar per Gaussian the two are formed from: None, the projection's `depths`; a tensor
                             # [N]; or a function `depths -> [N]` (a monotone map, whose gradient reaches the depths)
) -> Dict[str, Optional[torch.Tensor]]:
    H, W = cam.height, cam.width
    if caller_syncs == "camera" and cam.scalars is not None:
        # cx.item(), cy.item(), math.atan(width / (2 fx)), math.atan(height / (2 fy)), width.item(), height.item(),
        # fx.item(), fy.item(): eight read-backs, the first of which drains the stream (the previous iteration's
        # optimizer step included)
        sc = cam.scalars
        _ = (sc[2].item(), sc[3].item(), float(sc[4] / (2 * sc[0])), float(sc[5] / (2 * sc[1])), sc[4].item(),
             sc[5].item(), sc[0].item(), sc[1].item())
    opac_aa = None
    if crop is None and cam.model == "pinhole":
        xys, depths, radii, conics, comp, num_tiles_hit, cov3d = project_gaussians(
            means3d, scales, 1, quats, cam.viewmat[:3, :], cam.projmat, cam.fx, cam.fy, cam.cx, cam.cy,
            H, W, BLOCK_WIDTH,
        )
    elif cam.model != "pinhole":
        from gs_fused.fisheye import check_camera_model, project_gaussians_fisheye

        check_camera_model(cam.model)
        if crop is not None:
            raise ValueError("render_view: crop is not built for the fisheye camera (there is no cropped fisheye "
                             "projection)")
        if render_normals:
            raise ValueError("render_view: render_normals is pinhole only (depth_to_normal and the normal loss "
                             "unproject with pinhole intrinsics)")
        if rasterize_mode not in ("classic", "antialiased"):
            raise ValueError("Unknown rasterize_mode: %s" % rasterize_mode)
        res = project_gaussians_fisheye(
            means3d, scales, 1, quats, cam.viewmat[:3, :], cam.projmat, cam.fx, cam.fy, cam.cx, cam.cy,
            H, W, BLOCK_WIDTH, opacities=opacities if rasterize_mode == "antialiased" else None,
        )
        xys, depths, radii, conics, comp, num_tiles_hit, cov3d = res[:7]
        opac_aa = res[7] if len(res) == 8 else None
    else:
        from gs_fused import project_gaussians_cropped

        if rasterize_mode not in ("classic", "antialiased"):
            raise ValueError("Unknown rasterize_mode: %s" % rasterize_mode)
        res = project_gaussians_cropped(
            means3d, scales, 1, quats, cam.viewmat[:3, :], cam.projmat, cam.fx, cam.fy, cam.cx, cam.cy,
            H, W, BLOCK_WIDTH, crop, opacities=opacities if rasterize_mode == "antialiased" else None,
        )
        xys, depths, radii, conics, comp, num_tiles_hit, cov3d = res[:7]
        opac_aa = res[7] if len(res) == 8 else None
    if caller_syncs and (radii).sum() == 0:  # vanilla_gs.py:784-794: nothing on screen, the background
        rgb = background.repeat(H, W, 1)
        # (`depth_acc`: the accumulated, un-normalised depth the fused depth loss takes together with the alpha -- zeros
        #  over a zero alpha, so that loss trains on the reference's constant image for this view instead of meeting a
        #  None)
        return {"rgb": rgb, "alpha": background.new_zeros(H, W, 1), "depth": background.new_ones(H, W, 1) * 10,
                "depth_acc": background.new_zeros(H, W, 1), "xys": xys, "radii": radii, "depths": depths, "conics": conics,
                "num_tiles_hit": num_tiles_hit, "rgbs": None,
                **({"normals": background.new_zeros(H, W, 3)} if render_normals and render_depth else {}),
                **({"distortion": background.new_zeros(H, W, 1), "median_depth": background.new_zeros(H, W, 1)}
                   if render_distortion and render_depth else {})}
    if retain_xys_grad and xys.requires_grad:
        xys.retain_grad()  # densification reads xys.grad (vanilla_gs.py:352-353,797-798)

    if viewdirs is None:
        viewdirs = means3d.detach() - cam.campos
        viewdirs = viewdirs / viewdirs.norm(dim=-1, keepdim=True)
    split = isinstance(sh_coeffs, (tuple, list))
    if split:
        from gs_fused import spherical_harmonics_split

        # `torch.clamp(rgbs + 0.5, min=0.0)` inside the SH kernels
        sh_fn = lambda: spherical_harmonics_split(sh_degree_to_use, viewdirs, sh_coeffs[0], sh_coeffs[1], shift=0.5,  # noqa: E731
                                                  clamp_zero=True)
    else:
        sh_fn = lambda: spherical_harmonics(sh_degree_to_use, viewdirs, sh_coeffs)  # noqa: E731
    rgbs = None
    if sh_exchange is not None:
        exchange, names, leaves = sh_exchange
        K = leaves[-1].shape[1] + (1 if len(leaves) == 2 else 0)
        rgbs = exchange.deferred_sh_colors(sh_fn, names, leaves, means3d, cam.campos, {1: 0, 4: 1, 9: 2, 16: 3}[K],
                                           sh_degree_to_use, clamped=split)
    if rgbs is None:
        rgbs = sh_fn()
    if not split:
        rgbs = torch.clamp(rgbs + 0.5, min=0.0)

    if caller_syncs:
        assert (num_tiles_hit > 0).any()  # vanilla_gs.py:811 (a second blocking read-back)

    if rasterize_mode == "antialiased":
        opac = opacities * comp[:, None] if opac_aa is None else opac_aa  # (cropped, fisheye: the product left the kernel)
    elif rasterize_mode == "classic":
        opac = opacities
    else:
        raise ValueError("Unknown rasterize_mode: %s" % rasterize_mode)

    depth_im = depth_acc = None
    abs_kw = {"absgrad": True} if absgrad else {}  # (only where asked for: the default call is what it was)
    if render_depth and fused_depth:
        from gs_fused import rasterize_gaussians_rgbd

        rgb, alpha, depth_im = rasterize_gaussians_rgbd(xys, depths, radii, conics, num_tiles_hit, rgbs, depths, opac,
                                                        H, W, background=background, **abs_kw)
    else:
        rgb, alpha = rasterize_gaussians(
            xys, depths, radii, conics, num_tiles_hit, rgbs, opac, H, W, BLOCK_WIDTH,
            background=background, return_alpha=True, **abs_kw,
        )
    alpha = alpha[..., None]
    if crop is not None:
        # `rasterize_gaussians(return_alpha=True)` answers a view with nothing on screen with alpha = 1 (the quirk of
        # the reference's op, rasterize.py:119-127, which its models never meet: they return before it).  With a crop
        # the rule here is "anything on screen": alpha times 1.0 or 0.0, formed on the device (no read-back; times 1.0
        # changes no bit).  That covers the box that keeps nothing -- accumulation 0, as the reference's models give
        # -- and equally a box whose Gaussians are all off screen, where the route without a crop keeps the quirk
        alpha = alpha * (num_tiles_hit > 0).any().to(alpha.dtype)
    if clamp_rgb:
        rgb = torch.clamp(rgb, max=1.0)
    if render_depth:
        if depth_im is None:
            depth_im = rasterize_gaussians(
                xys, depths, radii, conics, num_tiles_hit, depths[:, None].repeat(1, 3), opac, H, W,
                BLOCK_WIDTH, background=torch.zeros(3, device=means3d.device),
            )[..., 0:1]
        depth_acc = depth_im
        depth_im = torch.where(alpha > 0, depth_im / alpha, depth_im.detach().max()) if normalise_depth else None
    normals_kw = {}  # (only where asked for: the default call returns the dictionary it always did)
    if render_normals and render_depth:
        from gs_fused import gaussian_normals

        normals_kw["normals"] = rasterize_gaussians(
            xys, depths, radii, conics, num_tiles_hit, gaussian_normals(quats, scales, means3d, cam.viewmat[:3, :]), opac,
            H, W, BLOCK_WIDTH, background=torch.zeros(3, device=means3d.device))
    if render_distortion and render_depth:
        from gs_fused import depth_distortion

        dist, median = depth_distortion(xys, depths, radii, conics, num_tiles_hit,
                                        depths if distortion_values is None else
                                        distortion_values(depths) if callable(distortion_values) else distortion_values,
                                        opac, H, W)
        normals_kw["distortion"], normals_kw["median_depth"] = dist[..., None], median[..., None]
    return {"rgb": rgb, "alpha": alpha, "depth": depth_im, "depth_acc": depth_acc, "xys": xys, "radii": radii,
            "depths": depths, "conics": conics, "num_tiles_hit": num_tiles_hit, "rgbs": rgbs, **normals_kw}


@torch.no_grad()
def contribution_stats(model, cams, cfg):
    """-> `gs_fused.ContributionStats` of `model` (a `harness.train.GaussianParams`) over the views `cams`
    (`CameraTensors`, at the resolution they state): per Gaussian the largest blend weight, the weight sum, the number
    of (pixel, Gaussian) pairs and the number of pixels it dominates.  Every view is projected
    by the separate ops and walked once by gs_fused's contribution walk, which builds the view's tile lists; with
    `cfg.rasterize_mode == "antialiased"` the opacities are the compensated ones the RGB pass composites with.  The
    statistics depend on no colour, so no image is composited and no SH degree enters.  No crop box; pinhole cameras only (a fisheye camera raises ValueError).  CUDA only."""
    from gs_fused import ContributionStats

    g = model.gauss
    if cfg.rasterize_mode not in ("classic", "antialiased"):
        raise ValueError("Unknown rasterize_mode: %s" % cfg.rasterize_mode)
    for cam in cams:
        if cam.model != "pinhole":
            raise ValueError(f"contribution_stats: a {cam.model} camera; the walk's views are projected by the pinhole "
                             "op (the fisheye camera is not built here)")
    if not cams:
        return ContributionStats(g["means"].shape[0], g["means"].device)
    if getattr(model, "fused_activations", False) and g["means"].is_cuda:
        from gs_fused import activate_gaussians

        # (the walk sees the filtered model, as every render does)
        scales, quats, opac, _ = activate_gaussians(g["means"], g["scales"], g["quats"], g["opacities"],
                                                    cams[0].campos, filter_3d=getattr(model, "filter_3d", None))
    elif getattr(model, "filter_3d", None) is not None:
        raise ValueError("filter_3d needs fused_activations on CUDA tensors: the filter is folded into the "
                         "activation kernels (gs_fused.apply_filter_3d is the torch form)")
    else:
        scales = torch.exp(g["scales"])
        quats = g["quats"] / g["quats"].norm(dim=-1, keepdim=True)
        opac = torch.sigmoid(g["opacities"])
    stats = ContributionStats(g["means"].shape[0], g["means"].device)
    for cam in cams:
        xys, depths, radii, conics, comp, num_tiles_hit, _ = project_gaussians(
            g["means"], scales, 1, quats, cam.viewmat[:3, :], cam.projmat, cam.fx, cam.fy, cam.cx, cam.cy,
            cam.height, cam.width, BLOCK_WIDTH)
        view_opac = opac * comp[:, None] if cfg.rasterize_mode == "antialiased" else opac
        stats.accumulate(xys, depths, radii, conics, num_tiles_hit, view_opac, cam.height, cam.width, BLOCK_WIDTH)
    return stats
