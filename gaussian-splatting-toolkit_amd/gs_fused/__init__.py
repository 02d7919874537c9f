"""Fused caller-side ops next to the rasterizer (SURVEY.md 8f "next" rows): the
photometric loss head (f2), the one-launch Adam step (f1) and SH colours from
split coefficients and the per-Gaussian activations (f4).  Same native library and C ABI (`include/gsraster.h`)
as `rasterizer`; no CPU fallback."""
from .loss import L1SSIMLoss, depth_l1_loss, depth_reg_loss, l1_loss, l1_ssim_loss  # noqa: F401
from .mono_depth import local_pearson_loss, log_depth_loss, tv_loss  # noqa: F401
from .canny import canny, canny_workspace_bytes, image2canny  # noqa: F401
from .adam import FusedAdam  # noqa: F401
from .sh import sh_backward_views, spherical_harmonics_split  # noqa: F401
from .activations import activate_gaussians, densify_stats_  # noqa: F401
from .rgbd import rasterize_gaussians_rgbd  # noqa: F401
from .refine import RefineConfig, adam_moments, refine_gaussians, refinement_branch, swap_parameters  # noqa: F401
from .mcmc import (MCMCConfig, MCMCInfo, mcmc_add, mcmc_branch, mcmc_inject_noise_, mcmc_num_new,  # noqa: F401
                   mcmc_refine, mcmc_regularizer, mcmc_relocate, relocation)
from .render import DensifyStats, ListCapacity, ViewSpec, render_gaussians  # noqa: F401
from rasterizer.project_gaussians import project_gaussians_antialiased  # noqa: F401
from .crop import CropBox, crop_gaussians, project_gaussians_cropped  # noqa: F401
from .fisheye import project_gaussians_fisheye  # noqa: F401
from .knn import KNN, initial_log_scales, k_nearest, knn, knn_mean_distance  # noqa: F401
from .target import DeferredTarget, ImageCache, plane_from_int, target_from_u8  # noqa: F401
from .bilagrid import BilateralGrids, bilagrid_slice, bilagrid_tv_loss  # noqa: F401
from .normals import depth_to_normal, gaussian_normals, normal_consistency_loss  # noqa: F401
from .distortion import depth_distortion, distortion_loss  # noqa: F401
from .contribution import ContributionStats, prune_gaussians, prune_mask, view_contributions  # noqa: F401
from .filter3d import apply_filter_3d, bake_filter_3d, filter_cameras, sampling_filter_3d  # noqa: F401
from .kmeans import KMeansResult, kmeans, kmeans_assign, kmeans_inertia, kmeans_update  # noqa: F401
