"""Loader of the native library behind ``rasterizer.cuda``.

Counterpart of the reference's ``rasterizer/cuda/_backend.py`` (prebuilt
extension first, nvcc JIT otherwise).  Here there is exactly one backend: the
HIP library ``libgsraster.so`` (C ABI in ``include/gsraster.h``) built in-tree
for gfx950 by ``csrc/Makefile``.  There is no CPU or eager-PyTorch fallback: if
the library is missing the first native call raises.
"""
import ctypes as C
import os
import subprocess

PATH = os.path.dirname(os.path.abspath(__file__))
# (GSR_LIBRARY: another build of the same library, for A/B measurements of compile-time variants -- tools/r05/)
LIB_PATH = os.environ.get("GSR_LIBRARY") or os.path.join(PATH, "libgsraster.so")
CSRC = os.path.normpath(os.path.join(PATH, "..", "..", "csrc"))

# every symbol include/gsraster.h declares
SYMBOLS = (
    "gsr_version",
    "gsr_last_error",
    "gsr_project_forward",
    "gsr_project_backward",
    "gsr_project_forward_aa",
    "gsr_project_backward_aa",
    "gsr_project_forward_crop",
    "gsr_crop_mask",
    "gsr_project_backward_pose_workspace",
    "gsr_project_backward_pose",
    "gsr_sh_forward",
    "gsr_sh_backward",
    "gsr_cumsum_workspace_bytes",
    "gsr_cumsum_tiles",
    "gsr_map_intersects",
    "gsr_sort_workspace_bytes",
    "gsr_sort_intersects",
    "gsr_tile_bin_edges",
    "gsr_reach_record_bytes",
    "gsr_tile_bands",
    "gsr_count_reach",
    "gsr_depth_order_workspace_bytes",
    "gsr_depth_order",
    "gsr_reach_records_depth_order",
    "gsr_bin_sorted_workspace_bytes",
    "gsr_bin_sorted_needs_counts",
    "gsr_bin_sorted",
    "gsr_bin_sorted_dev",
    "gsr_bin_sorted_dev_jobs",
    "gsr_publish_int32",
    "gsr_rasterize_forward",
    "gsr_rasterize_backward",
    "gsr_rasterize_forward_ex",
    "gsr_rasterize_backward_ex",
    "gsr_rasterize_forward_seg",
    "gsr_rasterize_forward_seg_workspace_bytes",
    "gsr_rasterize_backward_seg",
    "gsr_rasterize_backward_seg_workspace_bytes",
    "gsr_rasterize_backward_abs",
    "gsr_rasterize_backward_two_abs",
    "gsr_rasterize_backward_det_abs",
    "gsr_rasterize_forward_nd",
    "gsr_rasterize_backward_nd",
    "gsr_cov2d_bounds",
    "gsr_l1_ssim_forward",
    "gsr_l1_ssim_backward",
    "gsr_l1_forward",
    "gsr_l1_backward",
    "gsr_depth_l1_forward",
    "gsr_depth_l1_backward",
    "gsr_l1_ssim_masked_forward",
    "gsr_l1_ssim_masked_backward",
    "gsr_l1_masked_forward",
    "gsr_l1_masked_backward",
    "gsr_depth_l1_masked_forward",
    "gsr_depth_l1_masked_backward",
    "gsr_sh_forward_split",
    "gsr_sh_backward_split",
    "gsr_sh_backward_views",
    "gsr_rasterize_forward_rgbd",
    "gsr_rasterize_forward_scan",
    "gsr_tile_lists_subrange_workspace_bytes",
    "gsr_tile_lists_subrange",
    "gsr_saturation_filter_workspace_bytes",
    "gsr_saturation_filter",
    "gsr_rasterize_forward_round",
    "gsr_rasterize_backward_two",
    "gsr_view_forward",
    "gsr_view_forward_crop",
    "gsr_rasterize_gaussians_forward",
    "gsr_view_backward",
    "gsr_rasterize_backward_rgbd",
    "gsr_activate_forward",
    "gsr_activate_backward",
    "gsr_densify_stats",
    "gsr_densify_stats_dev",
    "gsr_refine_workspace_bytes",
    "gsr_refine_plan",
    "gsr_refine_apply",
    "gsr_mcmc_relocation",
    "gsr_mcmc_workspace_bytes",
    "gsr_mcmc_plan",
    "gsr_mcmc_apply",
    "gsr_mcmc_noise",
    "gsr_mcmc_reg_workspace_bytes",
    "gsr_mcmc_reg_forward",
    "gsr_mcmc_reg_backward",
    "gsr_adam_step",
    "gsr_rasterize_backward_det_workspace_bytes",
    "gsr_rasterize_backward_det",
    "gsr_tile_jobs_ints",
    "gsr_tile_jobs_build",
    "gsr_tsdf_touch",
    "gsr_tsdf_allocate_workspace_bytes",
    "gsr_tsdf_allocate",
    "gsr_tsdf_integrate",
    "gsr_tsdf_extract_points_workspace_bytes",
    "gsr_tsdf_extract_points_count",
    "gsr_tsdf_extract_points_emit",
    "gsr_tsdf_extract_mesh_workspace_bytes",
    "gsr_tsdf_extract_mesh_count",
    "gsr_tsdf_extract_mesh_emit",
    "gsr_mesh_clean_workspace_bytes",
    "gsr_mesh_label",
    "gsr_mesh_emit",
    "gsr_mesh_distance_workspace_bytes",
    "gsr_mesh_bvh_build",
    "gsr_mesh_distance_query",
    "gsr_mesh_distance_stats",
    "gsr_canny_workspace_bytes",
    "gsr_canny",
    "gsr_depth_reg_forward",
    "gsr_depth_reg_backward",
    "gsr_local_pearson_forward",
    "gsr_local_pearson_backward",
    "gsr_log_depth_forward",
    "gsr_log_depth_backward",
    "gsr_tv_forward",
    "gsr_tv_backward",
    "gsr_bilagrid_slice_forward",
    "gsr_bilagrid_slice_backward",
    "gsr_bilagrid_tv_forward",
    "gsr_bilagrid_tv_backward",
    "gsr_knn_workspace_bytes",
    "gsr_knn_build",
    "gsr_knn_query",
    "gsr_target_from_u8",
    "gsr_plane_from_int",
    "gsr_debug_count_staged",
    "gsr_debug_wave_trace",
    "gsr_calibrate_valu",
    "gsr_calibrate_copy",
)


def build(verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j8"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"rasterizer: native library {LIB_PATH} not found. Build it with "
            f"`make -C {CSRC}` (needs hipcc); there is no fallback implementation."
        )
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"rasterizer: {LIB_PATH} lacks symbols {missing}")
    lib.gsr_last_error.restype = C.c_char_p
    lib.gsr_version.restype = C.c_int
    lib.gsr_calibrate_valu.restype = C.c_longlong
    lib.gsr_tile_jobs_ints.restype = C.c_size_t
    lib.gsr_project_backward_pose_workspace.restype = C.c_size_t
    lib.gsr_cumsum_workspace_bytes.restype = C.c_size_t
    lib.gsr_sort_workspace_bytes.restype = C.c_size_t
    lib.gsr_reach_record_bytes.restype = C.c_size_t
    lib.gsr_depth_order_workspace_bytes.restype = C.c_size_t
    lib.gsr_bin_sorted_workspace_bytes.restype = C.c_size_t
    lib.gsr_refine_workspace_bytes.restype = C.c_size_t
    lib.gsr_mcmc_workspace_bytes.restype = C.c_size_t
    lib.gsr_mcmc_reg_workspace_bytes.restype = C.c_size_t
    lib.gsr_tile_lists_subrange_workspace_bytes.restype = C.c_size_t
    lib.gsr_saturation_filter_workspace_bytes.restype = C.c_size_t
    lib.gsr_rasterize_forward_seg_workspace_bytes.restype = C.c_size_t
    lib.gsr_rasterize_backward_seg_workspace_bytes.restype = C.c_size_t
    lib.gsr_rasterize_backward_det_workspace_bytes.restype = C.c_size_t
    lib.gsr_tsdf_allocate_workspace_bytes.restype = C.c_size_t
    lib.gsr_tsdf_extract_points_workspace_bytes.restype = C.c_size_t
    lib.gsr_tsdf_extract_mesh_workspace_bytes.restype = C.c_size_t
    lib.gsr_mesh_clean_workspace_bytes.restype = C.c_size_t
    lib.gsr_mesh_distance_workspace_bytes.restype = C.c_size_t
    lib.gsr_canny_workspace_bytes.restype = C.c_size_t
    lib.gsr_knn_workspace_bytes.restype = C.c_size_t
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


__all__ = ["lib", "build", "LIB_PATH", "SYMBOLS"]
