/*
 * gsraster.h -- C ABI of the MI355X-native Gaussian-splatting rasterizer.
 *
 * This is the drop-in boundary for the reference's native module
 * `rasterizer.cuda` (pybind module `rasterizer_cuda` / `rasterizer.csrc`,
 * gs_toolkit/gs_components/rasterizer/cuda/csrc/ext.cpp:4-18, prototypes in
 * cuda/csrc/bindings.h:19-115).  The reference has no C ABI -- its boundary is
 * pybind11 + torch::Tensor; every entry point below names the `*_tensor`
 * wrapper it replaces.  The Python mirror of the reference's package
 * (`gaussian-splatting-toolkit_amd/rasterizer`) binds these with ctypes.
 *
 * Conventions
 *   - all pointers are DEVICE pointers (hipMalloc'd, fp32 / int32 / int64 as
 *     named), contiguous, row-major, owned by the caller; inputs are never
 *     written; nothing is allocated or freed inside the library;
 *   - every output element is written by the call (the reference relies on
 *     torch::zeros pre-fill + early returns; here the kernels write the zeros
 *     themselves), EXCEPT the four gradient accumulators of
 *     gsr_rasterize_backward* which the call zero-fills itself before
 *     accumulating;
 *   - `stream` is a hipStream_t (NULL = the default stream); calls are
 *     asynchronous on that stream and never synchronise the device;
 *   - return value: 0 on success, a negative GSR_E* code otherwise, with a
 *     human-readable message available from gsr_last_error() (thread-local).
 *   - matrices are row-major; quaternions are (w,x,y,z); conics are the upper
 *     triangle (a,b,c) of the inverse 2-D covariance; tile id = ty*tiles_x+tx.
 */
#ifndef GSRASTER_H_
#define GSRASTER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_VERSION 200 /* 0.2.0 */

#define GSR_OK 0
#define GSR_EINVAL -1   /* bad argument (shape / range / null pointer) */
#define GSR_ELAUNCH -2  /* HIP reported a launch / runtime error */
#define GSR_ENOMEM -3   /* workspace too small */
#define GSR_ERANGE -4   /* index data on the device outside its range (gsr_mesh_label, gsr_mesh_bvh_build) */

typedef void *gsr_stream_t; /* hipStream_t */

int gsr_version(void);
/* message of the most recent failing call on this thread ("" if none) */
const char *gsr_last_error(void);

/* ---- projection -------------------------------------------------------
 * replaces project_gaussians_forward_tensor (bindings.cu:107-160), kernel
 * forward.cu:13-90.  viewmat: >= 12 floats (top 3x4), projmat: 16 floats.
 * outputs: cov3d[n,6] xys[n,2] depths[n] radii[n](i32) conics[n,3]
 *          compensation[n] num_tiles_hit[n](i32)
 * Precomputed covariances (the `cov3D_precomp` of Inria-style callers): with
 * scales == NULL and quats == NULL, cov3d[n,6] (upper triangle xx xy xz yy yz zz,
 * world space) is an INPUT and is not written; gsr_project_backward with the same
 * two NULLs then stops at v_cov3d (v_scale / v_quat are not touched, may be NULL). */
int gsr_project_forward(int num_points, const float *means3d,
                        const float *scales, float glob_scale,
                        const float *quats, const float *viewmat,
                        const float *projmat, float fx, float fy, float cx,
                        float cy, unsigned img_height, unsigned img_width,
                        unsigned block_width, float clip_thresh, float *cov3d,
                        float *xys, float *depths, int32_t *radii,
                        float *conics, float *compensation,
                        int32_t *num_tiles_hit, gsr_stream_t stream);

/* replaces project_gaussians_backward_tensor (bindings.cu:164-216), kernel
 * backward.cu:305-347.  outputs: v_cov2d[n,3] v_cov3d[n,6] v_mean3d[n,3]
 * v_scale[n,3] v_quat[n,4].  Each of the cotangents v_xy, v_depth, v_conic,
 * v_compensation may be NULL (= all zeros). */
int gsr_project_backward(int num_points, const float *means3d,
                         const float *scales, float glob_scale,
                         const float *quats, const float *viewmat,
                         const float *projmat, float fx, float fy, float cx,
                         float cy, unsigned img_height, unsigned img_width,
                         const float *cov3d, const int32_t *radii,
                         const float *conics, const float *compensation,
                         const float *v_xy, const float *v_depth,
                         const float *v_conic, const float *v_compensation,
                         float *v_cov2d, float *v_cov3d, float *v_mean3d,
                         float *v_scale, float *v_quat, gsr_stream_t stream);

/* The antialiased rasterize mode (`rasterize_mode="antialiased"`, vanilla_gs.py:96-104,815-816: the model composites
 * opacities * compensation) inside the projection: the same kernels behind a template flag, one more 4-byte stream
 * per Gaussian each way.
 * gsr_project_forward_aa = gsr_project_forward (same seven outputs, bit for bit) plus
 *   opacities_aa[i] = opacities[i] * compensation[i]   one float32 multiply; a culled Gaussian gets x * 0.
 * gsr_project_backward_aa = gsr_project_backward plus the product's two cotangents:
 *   v_opacities[i] = v_opacities_aa[i] * compensation[i]          (may be v_opacities_aa itself: written after the read)
 *   the compensation's cotangent inside the chain is v_compensation[i] + v_opacities_aa[i] * opacities[i] (float32;
 *   the second term alone when v_compensation == NULL), in front of the 0.5 / (compensation + 1e-6) scaling;
 *   v_compensation_out [n], nullable, receives that cotangent: what gsr_project_backward_pose takes as its
 *   v_compensation when a camera requires a gradient.  It must not be v_compensation itself. */
int gsr_project_forward_aa(int num_points, const float *means3d,
                           const float *scales, float glob_scale,
                           const float *quats, const float *viewmat,
                           const float *projmat, float fx, float fy, float cx,
                           float cy, unsigned img_height, unsigned img_width,
                           unsigned block_width, float clip_thresh,
                           const float *opacities, float *cov3d, float *xys,
                           float *depths, int32_t *radii, float *conics,
                           float *compensation, int32_t *num_tiles_hit,
                           float *opacities_aa, gsr_stream_t stream);
int gsr_project_backward_aa(int num_points, const float *means3d,
                            const float *scales, float glob_scale,
                            const float *quats, const float *viewmat,
                            const float *projmat, float fx, float fy, float cx,
                            float cy, unsigned img_height, unsigned img_width,
                            const float *cov3d, const int32_t *radii,
                            const float *conics, const float *compensation,
                            const float *opacities, const float *v_xy,
                            const float *v_depth, const float *v_conic,
                            const float *v_compensation,
                            const float *v_opacities_aa, float *v_cov2d,
                            float *v_cov3d, float *v_mean3d, float *v_scale,
                            float *v_quat, float *v_opacities,
                            float *v_compensation_out, gsr_stream_t stream);

/* The oriented crop box (`OrientedBox`, gs_toolkit/data/scene_box.py:74-108; `get_outputs` gathers the Gaussians
 * inside it before it projects, vanilla_gs.py:703-757) inside the projection: a Gaussian whose centre is outside the
 * box is a culled Gaussian -- radii = num_tiles_hit = 0 and zeros in every other output, opacities_aa included -- so
 * the count never changes, nothing is gathered, and gsr_project_backward(_aa) returns zeros for it as for any
 * radii <= 0.  `crop` is float32[16] on the device:
 *   crop[0:12]   A, the world->box matrix (the inverse of [[R, T], [0, 1]]), top 3x4, row-major
 *   crop[12:15]  h = S / 2, the half extents;  crop[15] is not read
 *   q_k = ((A_k0 x + A_k1 y) + A_k2 z) + A_k3, every product and sum rounded to float32 on its own;
 *   inside <=> -h_k < q_k < h_k for k = 0, 1, 2 (strict).  A NaN coordinate is outside; h_k = 0 keeps nothing.
 * gsr_project_forward_crop = gsr_project_forward with that test; opacities / opacities_aa both NULL, or both given:
 *   then it is gsr_project_forward_aa with that test.  Inside Gaussians get the uncropped entry's bits.
 * gsr_crop_mask: mask[i] = 1 / 0 by the same device function; count (nullable, int32[1] on the device) receives the
 *   number of ones (zeroed and summed on `stream`: one integer atomic per workgroup). */
int gsr_project_forward_crop(int num_points, const float *means3d,
                             const float *scales, float glob_scale,
                             const float *quats, const float *viewmat,
                             const float *projmat, float fx, float fy, float cx,
                             float cy, unsigned img_height, unsigned img_width,
                             unsigned block_width, float clip_thresh,
                             const float *crop, const float *opacities,
                             float *cov3d, float *xys, float *depths,
                             int32_t *radii, float *conics, float *compensation,
                             int32_t *num_tiles_hit, float *opacities_aa,
                             gsr_stream_t stream);
int gsr_crop_mask(int num_points, const float *means3d, const float *crop,
                  uint8_t *mask, int32_t *count, gsr_stream_t stream);

/* The equidistant fisheye camera (gsplat's camera_model="fisheye" with an ideal lens: every distortion coefficient
 * of OPENCV_FISHEYE zero) inside the projection: the same kernels behind one more template flag.  For the view-space
 * centre t = V p~: culled when tz <= clip_thresh (which keeps the polar angle below 90 degrees);
 *   r = sqrt(tx^2 + ty^2), theta = atan2(r, tz), s = theta / r (1 / tz at r = 0),
 *   xy = (fx s tx + cx - 0.5, fy s ty + cy - 0.5)   -- `projmat` is not read (may be NULL),
 *   J = d(xy)/dt, finite and accurate from r = 0 upward (a power series below r^2 / tz^2 = 1/32), no clamp of the
 *   centre in either direction; cov2d, conics, radii and the tile box follow from J as in gsr_project_forward;
 *   the compensation is the same quantity, its determinants formed without cancellation where scales and quats are
 *   given (accurate on needles; the pinhole expression where cov3d is handed in); depths = tz.  Every output of a
 *   culled Gaussian is zero, cov3d and conics included.
 * One entry each way for both rasterize modes: opacities / opacities_aa (forward) and opacities / v_opacities_aa /
 * v_opacities (backward) are all NULL -- then the arguments and outputs are those of gsr_project_forward /
 * gsr_project_backward -- or all given: those of the _aa entries (v_compensation_out stays nullable).
 * No crop box and no camera gradients (gsr_project_backward_pose differentiates the pinhole chain). */
int gsr_project_forward_fisheye(int num_points, const float *means3d,
                                const float *scales, float glob_scale,
                                const float *quats, const float *viewmat,
                                const float *projmat, float fx, float fy,
                                float cx, float cy, unsigned img_height,
                                unsigned img_width, unsigned block_width,
                                float clip_thresh, const float *opacities,
                                float *cov3d, float *xys, float *depths,
                                int32_t *radii, float *conics,
                                float *compensation, int32_t *num_tiles_hit,
                                float *opacities_aa, gsr_stream_t stream);
int gsr_project_backward_fisheye(int num_points, const float *means3d,
                                 const float *scales, float glob_scale,
                                 const float *quats, const float *viewmat,
                                 const float *projmat, float fx, float fy,
                                 float cx, float cy, unsigned img_height,
                                 unsigned img_width, const float *cov3d,
                                 const int32_t *radii, const float *conics,
                                 const float *compensation,
                                 const float *opacities, const float *v_xy,
                                 const float *v_depth, const float *v_conic,
                                 const float *v_compensation,
                                 const float *v_opacities_aa, float *v_cov2d,
                                 float *v_cov3d, float *v_mean3d,
                                 float *v_scale, float *v_quat,
                                 float *v_opacities, float *v_compensation_out,
                                 gsr_stream_t stream);

/* Camera gradients of the projection (the reference has none: project_gaussians.py:156-232 returns None for both
 * matrices): v_viewmat[12] (top 3x4) and v_projmat[16], the sums over the Gaussians with radii > 0 of the terms
 * gsr_project_backward forms per Gaussian, under its conventions (no fov clamp; the compensation's cotangent scaled by
 * 0.5 / (compensation + 1e-6); a NULL cotangent = all zeros).  Row 2 of v_projmat is exactly zero (the forward never
 * reads that row).  Reads cov3d, never scales or quats: precomputed covariances need nothing else.  A pass of its
 * own -- two launches, gsr_project_backward is not involved; float64 sums in a fixed order through `workspace`
 * (8-byte aligned, gsr_project_backward_pose_workspace(num_points) bytes; GSR_ENOMEM when shorter), no atomics:
 * the same inputs give the same bits.  num_points == 0 writes zeros to both outputs. */
size_t gsr_project_backward_pose_workspace(int num_points);
int gsr_project_backward_pose(int num_points, const float *means3d,
                              const float *viewmat, const float *projmat,
                              float fx, float fy, unsigned img_height,
                              unsigned img_width, const float *cov3d,
                              const int32_t *radii, const float *conics,
                              const float *compensation, const float *v_xy,
                              const float *v_depth, const float *v_conic,
                              const float *v_compensation, void *workspace,
                              size_t workspace_bytes, float *v_viewmat,
                              float *v_projmat, gsr_stream_t stream);

/* ---- spherical harmonics ----------------------------------------------
 * replaces compute_sh_forward_tensor / compute_sh_backward_tensor
 * (bindings.cu:58-103), kernels sh.cuh:188-224.  degree in 0..4 fixes the
 * coefficient layout [n, (degree+1)^2, 3]; degrees_to_use <= degree.
 * Contract for what is not in use (all SH entries below too): the bands
 * k >= (degrees_to_use+1)^2 of coeffs, and at degrees_to_use == 0 the view
 * direction, are NOT OBSERVED: they may hold anything (NaN, Inf) without
 * reaching colors.  The backward entries write exact zeros into those bands of
 * v_coeffs whatever the direction holds (a zero or non-finite direction gives
 * NaN only in the bands 1 .. in use, like the reference's x / norm). */
int gsr_sh_forward(unsigned num_points, unsigned degree,
                   unsigned degrees_to_use, const float *viewdirs,
                   const float *coeffs, float *colors, gsr_stream_t stream);
/* gsr_sh_forward with a flags word (0: gsr_sh_forward itself), for a caller
 * with other kernels of its own in flight on another stream (tile lists
 * built ahead).  Degree 3 with 16-byte aligned coeffs only; no effect
 * elsewhere.  The same colours, bit for bit.
 * GSR_SH_SHARE_CU: a quarter of the LDS per wave, so that kernels that need
 * LDS fit on a compute unit beside this one.
 * GSR_SH_NARROW (with GSR_SH_SHARE_CU): two waves per compute unit -- the
 * kernel takes 2.5 x as long and leaves the memory system to the others;
 * for a caller whose critical path is the other stream. */
#define GSR_SH_SHARE_CU 1u
#define GSR_SH_NARROW 2u
int gsr_sh_forward_flags(unsigned num_points, unsigned degree,
                         unsigned degrees_to_use, const float *viewdirs,
                         const float *coeffs, float *colors, unsigned flags,
                         gsr_stream_t stream);
int gsr_sh_backward(unsigned num_points, unsigned degree,
                    unsigned degrees_to_use, const float *viewdirs,
                    const float *v_colors, float *v_coeffs,
                    gsr_stream_t stream);

/* ---- binning ------------------------------------------------------------
 * inclusive int32 scan of num_tiles_hit; replaces the torch.cumsum of
 * compute_cumulative_intersects (utils.py:106-125).  The total is cum[n-1]
 * (device memory; the caller decides when to read it back). */
size_t gsr_cumsum_workspace_bytes(int num_points);
int gsr_cumsum_tiles(int num_points, const int32_t *num_tiles_hit,
                     int32_t *cum_tiles_hit, void *workspace,
                     size_t workspace_bytes, gsr_stream_t stream);

/* replaces map_gaussian_to_intersects_tensor (bindings.cu:218-251), kernel
 * forward.cu:94-127.  isect_ids[I] (i64) gaussian_ids[I] (i32). */
int gsr_map_intersects(int num_points, int num_intersects, const float *xys,
                       const float *depths, const int32_t *radii,
                       const int32_t *cum_tiles_hit, int tiles_x, int tiles_y,
                       unsigned block_width, int64_t *isect_ids,
                       int32_t *gaussian_ids, gsr_stream_t stream);

/* replaces torch.sort + torch.gather in bin_and_sort_gaussians
 * (utils.py:179-180): stable ascending radix sort of the (tile|depth) keys
 * over the significant bits only (32 depth bits + ceil(log2(num_tiles))). */
size_t gsr_sort_workspace_bytes(int num_intersects);
int gsr_sort_intersects(int num_intersects, int num_tiles,
                        const int64_t *isect_ids, const int32_t *gaussian_ids,
                        int64_t *isect_ids_sorted,
                        int32_t *gaussian_ids_sorted, void *workspace,
                        size_t workspace_bytes, gsr_stream_t stream);

/* replaces get_tile_bin_edges_tensor (bindings.cu:253-267), kernel
 * forward.cu:132-154.  tile_bins[num_tiles,2] (i32), (0,0) for empty tiles. */
int gsr_tile_bin_edges(int num_intersects, const int64_t *isect_ids_sorted,
                       int num_tiles, int32_t *tile_bins, gsr_stream_t stream);

/* ---- binning, fused pipeline ---------------------------------------------
 * What `_RasterizeGaussians.forward` needs from bin_and_sort_gaussians
 * (utils.py:128-182) is only `gaussian_ids_sorted` and `tile_bins`.  These two
 * calls produce exactly those (bit-identical to map + 64-bit sort + bin edges)
 * with ~4x less HBM traffic: Gaussians are ordered by depth once, intersections
 * are emitted in that order and then stably sorted by tile id only.
 *   gsr_depth_order : order[n] = Gaussian indices by (depth, index), culled
 *                     first; cum_sorted[n] = inclusive scan of num_tiles_hit in
 *                     that order (cum_sorted[n-1] = number of intersections).
 *   gsr_bin_sorted  : gaussian_ids_sorted[I], tile_bins[T,2].
 * All counts and list offsets are int32, as in the reference (`cum_tiles_hit`): a view with
 * 2^31 or more (Gaussian, tile) intersections is out of range -- sum num_tiles_hit in 64 bits
 * before sizing the lists if that can happen (the Python package does and raises).
 *
 * Exact lists (optional, block_width 16 only).  The reference lists every tile
 * of a splat's 3-sigma SQUARE (forward.cu:73-82); about half of those (splat,
 * tile) pairs cannot reach alpha >= 1/255 at any pixel of the tile, and the
 * compositing rule skips them pixel by pixel (forward.cu:349).  gsr_count_reach
 * counts, per Gaussian, the tiles that can, and fills one opaque record of
 * gsr_reach_record_bytes() bytes per Gaussian (16-byte aligned buffer).  Passing
 * the counts to gsr_depth_order (in place of num_tiles_hit) and the records to
 * gsr_bin_sorted builds the lists without the dead pairs: images and gradients
 * are unchanged, `gaussian_ids_sorted` is a subsequence of the reference's.
 * slot_of_entry (nullable, int32 as long as the lists): for the e-th list entry in
 * (band, depth position, tile) order -- the entries of the Gaussian at depth position
 * i in band b are e in [cum_sorted[b n + i - 1], cum_sorted[b n + i]) -- the index it got
 * in gaussian_ids_sorted: the inverse map gsr_rasterize_backward_det reduces along.
 * With reach_records == NULL gsr_bin_sorted reproduces the reference's lists
 * bit for bit.
 *
 * Large tile grids (above 16384 tiles; 4K at 16 px: 240 x 135) need the reach
 * records and are built in one of two ways, chosen by `num_bands` of
 * gsr_count_reach / gsr_depth_order / gsr_bin_sorted(_dev):
 *   num_bands = 1 (default of the Python package): TWO-LEVEL PARTITION -- the entries
 *     are emitted straight into per-tile-row segments and each row is then split by
 *     tile column, every store coalesced (csrc/tile_partition2.hip);
 *   num_bands = gsr_tile_bands(tiles_x, tiles_y) (4 at 4K): TILE-ROW BANDS -- the
 *     single-pass scatter band by band: gsr_count_reach writes counts[bands, n]
 *     (band-major), gsr_depth_order scans them in (band, depth) order into
 *     cum_sorted[bands * n]; slower on large lists, but hands out slot_of_entry
 *     (deterministic backward).
 * Grids up to 16384 tiles: num_bands = 1; the two-level partition from 1 M list
 * entries on, the single-pass scatter below (and whenever slot_of_entry is wanted).
 *
 * Lists without counts.  The two-level partition counts its entries itself (per tile
 * row, in depth order): where gsr_bin_sorted_needs_counts() returns 0 for the call
 * about to be made (same num_points / num_intersects-or-capacity / grid; reach records
 * and num_bands == 1 assumed), the caller may pass counts = NULL to gsr_count_reach
 * (records only, no walk over the tile rows), num_tiles_hit = cum_sorted = NULL to
 * gsr_depth_order (the order only: no gather, no scan) and cum_sorted = NULL to
 * gsr_bin_sorted(_dev); the number of entries then arrives through count_out of
 * gsr_bin_sorted_dev.  Same lists, two kernels and a scan less.
 * gsr_reach_records_depth_order is those two calls -- gsr_count_reach(counts = NULL) and
 * gsr_depth_order(num_tiles_hit = cum_sorted = NULL, num_bands = 1) -- as one: the same records and the same
 * order; where the depth order is built by the bucket sort (csrc/sort_bucket.hip: 64 k < num_points <= 4 M) the
 * records are written by its first launch.  workspace: gsr_depth_order_workspace_bytes(num_points, 1).
 *
 * How the depth sort is built (64 k < num_points <= 4 M, with or without counts) may depend on earlier calls on the same
 * device -- a hint in pinned memory sends calls to the radix passes after a view whose depths overflowed the
 * bucket sort's buckets -- the RESULT never does: both are the stable sort by (depth bits, index).
 * GSR_DEPTH_SORT=radix | bucket in the environment pins the choice. */
size_t gsr_reach_record_bytes(void);
int gsr_tile_bands(int tiles_x, int tiles_y);
int gsr_count_reach(int num_points, const float *xys, const int32_t *radii,
                    const float *conics, const float *opacities, int tiles_x,
                    int tiles_y, int num_bands, int32_t *counts,
                    void *reach_records, gsr_stream_t stream);
size_t gsr_depth_order_workspace_bytes(int num_points, int num_bands);
int gsr_depth_order(int num_points, const float *depths, const int32_t *radii,
                    const int32_t *num_tiles_hit, int num_bands,
                    int32_t *order, int32_t *cum_sorted, void *workspace,
                    size_t workspace_bytes, gsr_stream_t stream);
int gsr_reach_records_depth_order(int num_points, const float *xys, const int32_t *radii,
                                  const float *conics, const float *opacities, const float *depths,
                                  int tiles_x, int tiles_y, void *reach_records, int32_t *order,
                                  void *workspace, size_t workspace_bytes, gsr_stream_t stream);
size_t gsr_bin_sorted_workspace_bytes(int num_points, int num_intersects,
                                      int tiles_x, int tiles_y);
int gsr_bin_sorted_needs_counts(int num_points, int num_intersects, int tiles_x,
                                int tiles_y, int device_sized, int want_slots);
int gsr_bin_sorted(int num_points, int num_intersects, const int32_t *order,
                   const int32_t *cum_sorted, const float *xys,
                   const int32_t *radii, const void *reach_records, int tiles_x,
                   int tiles_y, unsigned block_width, int num_bands,
                   int32_t *gaussian_ids_sorted, int32_t *tile_bins,
                   int32_t *slot_of_entry, void *workspace,
                   size_t workspace_bytes, gsr_stream_t stream);

/* One int32 from device memory to any device-accessible address, e.g. pinned
 * host memory mapped into the device's address space: a one-thread kernel in
 * stream order instead of a copy operation.  Used to hand cum_sorted[n-1] to the
 * host as early as possible (right after gsr_depth_order). */
int gsr_publish_int32(const int32_t *src, int32_t *dst, gsr_stream_t stream);

/* gsr_bin_sorted without the host knowing the number of intersections: the
 * length of the lists is read on the device (the last element of cum_sorted, as
 * written by gsr_depth_order) and `capacity` is what gaussian_ids_sorted and the
 * workspace (gsr_bin_sorted_workspace_bytes(capacity, ...)) were sized for.  If the
 * length exceeds the capacity the lists are cut there (memory-safe, results
 * incomplete): the caller compares the two once the value has reached the host
 * and repeats the call with a larger capacity.  This removes the host round
 * trip of rasterizer/utils.py:124 (`cum_tiles_hit[-1].item()`) from the critical
 * path.  count_out (nullable) receives the uncut length; it only has to be
 * device-accessible, e.g. pinned host memory mapped into the device's address
 * space, which spares the copy as well.  Tile grids above 16384 tiles need the
 * reach records (bands, above); without them: GSR_EINVAL, use gsr_bin_sorted. */
int gsr_bin_sorted_dev(int num_points, int capacity, const int32_t *order,
                       const int32_t *cum_sorted, const float *xys,
                       const int32_t *radii, const void *reach_records,
                       int tiles_x, int tiles_y, unsigned block_width,
                       int num_bands, int32_t *gaussian_ids_sorted,
                       int32_t *tile_bins, int32_t *count_out,
                       int32_t *slot_of_entry,
                       void *workspace, size_t workspace_bytes,
                       gsr_stream_t stream);

/* ---- compositing ----------------------------------------------------------
 * replaces rasterize_forward_tensor (bindings.cu:269-328), kernel
 * forward.cu:278-395 (3 channels, fp32).  out_img[H,W,3] final_Ts[H,W]
 * final_idx[H,W](i32).
 * deep_tile_threshold (block_width 16 only; here, in gsr_rasterize_backward and in
 * the _rgbd variants): 0 = one wave per tile.  > 0: a tile whose list holds more
 * entries than this is composited by four waves, one per 8x8 sub-tile, so that a few
 * very deep tiles (clustered scenes) do not hold a kernel up after the rest of the
 * chip has drained.  Never changes a result (same per-pixel instruction sequence);
 * costs three idle workgroups per tile at launch.  A good value: 1.5x the mean list
 * length, not below 256 (a split tile costs ~2x the instructions per list entry).
 * deep_tile_threshold | GSR_DEEP_ORDERED (16x16 tiles; every entry that takes a
 * deep_tile_threshold except the two-round and the deterministic ones, which ignore
 * the flags): LONGEST JOB FIRST.  tile_bins must then be followed by
 * gsr_tile_jobs_ints(tiles_x, tiles_y) writable int32 (one allocation of
 * 2 * tiles + that many ints: room for TWO job arrays -- a launch uses the first
 * unless GSR_DEEP_SECOND is set -- and the address of the library's statistics); the compositing workgroups take their jobs from the array in
 * block order -- per XCD, its tiles' jobs (a whole tile, or the four sub-tile jobs of a
 * tile above the threshold) by decreasing half-octave of the list length ( a split
 * tile's jobs keyed by an eighth of it), stable inside a bucket -- so that the walks
 * that last longest start first and the launch does not end on a few long walks over an
 * emptying chip.  Never changes a result.
 * Who writes the array: the entry itself, with one small kernel in front of the
 * compositing launch -- or, with GSR_DEEP_PREBUILT also set, nobody: the caller has
 * called gsr_tile_jobs_build, which writes up to both arrays (say the forward's and,
 * with other parameters, the backward's) in ONE launch.  The buffer belongs to one
 * stream at a time.
 * With GSR_DEEP_SECOND (the backward's order) a launch whose lists are ALL ALIKE --
 * the longest within 1.5x the mean of the non-empty ones -- splits no tile, whatever
 * the threshold, and either order then keeps the static map's sequence: there is
 * nothing to balance and a split tile costs the backward 1.7x the instructions.
 * GSR_DEEP_TAIL_64THS(k), k = 0..63: the last k / 64 of the launch's whole-tile jobs
 * -- the shortest -- run as four sub-tile jobs each behind everything else, whatever
 * their length: quarter-length jobs to fill the launch's drain.
 * Bits: 0-21 threshold, 22-27 tail, 28 SECOND, 29 PREBUILT, 30 ORDERED. */
#define GSR_DEEP_ORDERED (1 << 30)
#define GSR_DEEP_PREBUILT (1 << 29)
#define GSR_DEEP_SECOND (1 << 28)
#define GSR_DEEP_TAIL_64THS(k) (((k) & 63) << 22)
size_t gsr_tile_jobs_ints(int tiles_x, int tiles_y);
int gsr_tile_jobs_build(int tiles_x, int tiles_y, int32_t *tile_bins, int deep_arg_first,
                        int deep_arg_second, gsr_stream_t stream);
/* gsr_bin_sorted_dev that also does gsr_tile_jobs_build's work: where the lists are built by
 * the two-level partition, its last launch writes both job orders behind tile_bins beside
 * the lists' last pass (tile_bins is complete by then), and no launch of its own is needed.
 * deep_arg_first / deep_arg_second: as gsr_tile_jobs_build takes them (0 / without
 * GSR_DEEP_ORDERED in the first: no order, plain gsr_bin_sorted_dev).  *jobs_built (host,
 * required) = 1: the arrays are as gsr_tile_jobs_build would have left them, the compositing
 * entries take GSR_DEEP_PREBUILT; 0 (another list builder, a grid whose tables do not fit
 * that launch, a grid beyond the order's tables): nothing was written, call
 * gsr_tile_jobs_build as before. */
int gsr_bin_sorted_dev_jobs(int num_points, int capacity, const int32_t *order,
                            const int32_t *cum_sorted, const float *xys,
                            const int32_t *radii, const void *reach_records,
                            int tiles_x, int tiles_y, unsigned block_width,
                            int num_bands, int32_t *gaussian_ids_sorted,
                            int32_t *tile_bins, int32_t *count_out,
                            int32_t *slot_of_entry,
                            void *workspace, size_t workspace_bytes,
                            int deep_arg_first, int deep_arg_second, int *jobs_built,
                            gsr_stream_t stream);
/* The other mapping of the same compositing rule (measurement variant, 16x16 tiles, 3 channels):
 * lanes over the 64 staged splats, a wave-wide multiplicative prefix scan for the per-pixel
 * transmittance, ballot termination (forward.cu:349-385 is the serial loop it re-maps).  Same
 * outputs as gsr_rasterize_forward up to the rounding of T (a tree-ordered product). */
int gsr_rasterize_forward_scan(int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                               const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                               const float *xys, const float *conics, const float *colors,
                               const float *opacities, const float *background, float *out_img,
                               float *final_Ts, int32_t *final_idx, gsr_stream_t stream);

int gsr_rasterize_forward(int tiles_x, int tiles_y, unsigned block_width,
                          unsigned img_width, unsigned img_height,
                          const int32_t *gaussian_ids_sorted,
                          const int32_t *tile_bins, const float *xys,
                          const float *conics, const float *colors,
                          const float *opacities, const float *background,
                          float *out_img, float *final_Ts, int32_t *final_idx,
                          int deep_tile_threshold, gsr_stream_t stream);

/* replaces rasterize_backward_tensor (bindings.cu:476-528), kernel
 * backward.cu:133-303.  v_xy[n,2] v_conic[n,3] v_colors[n,3] v_opacity[n]
 * are zero-filled by the call, then accumulated with fp32 atomics.
 * v_output_alpha may be NULL (= all zeros), here and in the _nd variant. */
int gsr_rasterize_backward(unsigned img_height, unsigned img_width,
                           unsigned block_width, int num_points,
                           const int32_t *gaussian_ids_sorted,
                           const int32_t *tile_bins, const float *xys,
                           const float *conics, const float *colors,
                           const float *opacities, const float *background,
                           const float *final_Ts, const int32_t *final_idx,
                           const float *v_output, const float *v_output_alpha,
                           float *v_xy, float *v_conic, float *v_colors,
                           float *v_opacity, int deep_tile_threshold,
                           gsr_stream_t stream);

/* The same two calls with what `_RasterizeGaussians.forward` does around them folded in
 * (rasterize.py:145-176: `out_alpha = 1 - final_Ts`; the backward's zero-filled
 * accumulators).  block_width 16 only when the extras are used.
 *   out_alpha (nullable) [H,W]: 1 - final_Ts, written by the compositing kernel;
 *   zero_ptr / zero_bytes (nullable; multiples of 4): cleared by the forward launch --
 *     pass the backward's accumulators (v_xy .. v_opacity as one allocation), keep them
 *     untouched, and call gsr_rasterize_backward_ex with accumulators_zeroed = 1: the
 *     36 MB of stores at 1 M Gaussians disappear inside the VALU-bound forward kernel
 *     instead of taking a bandwidth-bound launch of their own. */
int gsr_rasterize_forward_ex(int tiles_x, int tiles_y, unsigned block_width,
                             unsigned img_width, unsigned img_height,
                             const int32_t *gaussian_ids_sorted,
                             const int32_t *tile_bins, const float *xys,
                             const float *conics, const float *colors,
                             const float *opacities, const float *background,
                             float *out_img, float *final_Ts, int32_t *final_idx,
                             int deep_tile_threshold, float *out_alpha,
                             void *zero_ptr, size_t zero_bytes, gsr_stream_t stream);
int gsr_rasterize_backward_ex(unsigned img_height, unsigned img_width,
                              unsigned block_width, int num_points,
                              const int32_t *gaussian_ids_sorted,
                              const int32_t *tile_bins, const float *xys,
                              const float *conics, const float *colors,
                              const float *opacities, const float *background,
                              const float *final_Ts, const int32_t *final_idx,
                              const float *v_output, const float *v_output_alpha,
                              float *v_xy, float *v_conic, float *v_colors,
                              float *v_opacity, int deep_tile_threshold,
                              int accumulators_zeroed, gsr_stream_t stream);

/* gsr_rasterize_forward_ex / _rgbd (16x16 tiles, 3 channels [+ one]) with DEPTH SEGMENTS: the list of every tile that is split over
 * four waves (deep_tile_threshold) and holds more than max(deep_tile_threshold, segment_min_entries) entries is cut
 * into `segments` (2..16) runs of whole 64-entry chunks.  Compositing is associative in (C, T): every run is walked
 * ONCE from T = 1 by its own waves, a resolve pass scales the runs' colour sums by the products of the runs in front and
 * finds the run in which each pixel crosses the stop rule's 1e-4, and only those (sub-tile, run) pairs are walked again
 * from the true incoming T -- the exact stop rule and final_idx of forward.cu:278-395 (round 6; rounds 4-5 walked every
 * list twice).  For tile grids too small to fill the chip (the
 * 480 x 270 phase of the reference's coarse-to-fine schedule, vanilla_gs.py:48-53, is 510 tiles).  Results equal
 * gsr_rasterize_forward_ex's to rounding.  workspace: gsr_rasterize_forward_seg_workspace_bytes(...) bytes, 16-byte
 * aligned.  segments < 2 or deep_tile_threshold <= 0: the walk of gsr_rasterize_forward_ex (with `extra`: _rgbd). */
size_t gsr_rasterize_forward_seg_workspace_bytes(unsigned img_height, unsigned img_width, int segments);
/* extra / out_extra: NULL, or the fourth channel of gsr_rasterize_forward_rgbd ([n] / [P], over extra_background) */
int gsr_rasterize_forward_seg(int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                              const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                              const float *xys, const float *conics, const float *colors,
                              const float *extra, const float *opacities, const float *background,
                              float extra_background, float *out_img, float *out_extra,
                              float *final_Ts, int32_t *final_idx, int deep_tile_threshold,
                              float *out_alpha, void *zero_ptr, size_t zero_bytes, int segments,
                              int segment_min_entries, void *workspace, size_t workspace_bytes,
                              gsr_stream_t stream);

/* gsr_rasterize_backward_ex / _rgbd (16x16 tiles) with DEPTH SEGMENTS: the list of every tile that is split over four waves
 * (deep_tile_threshold) and holds more than max(deep_tile_threshold, segment_min_entries) entries is cut into
 * `segments` (2..16) runs, each walked by its own waves; a pre-pass computes what every run does to the backward's
 * per-pixel state (backward.cu:133-303: T and the colour buffer -- an affine map per run), so the runs are
 * independent.  For tile grids too small to fill the chip and for scenes whose deepest tiles set the kernel's
 * duration.  Results equal gsr_rasterize_backward_ex's to rounding (T reaches a run as a product of run products).
 * workspace: gsr_rasterize_backward_seg_workspace_bytes(img_height, img_width, segments) bytes, 8-byte aligned.
 * segments < 2 or deep_tile_threshold <= 0: the walk of gsr_rasterize_backward_ex (with `extra`: _rgbd). */
size_t gsr_rasterize_backward_seg_workspace_bytes(unsigned img_height, unsigned img_width, int segments);
/* extra / v_output_extra / v_extra: NULL, or the fourth channel as in gsr_rasterize_backward_rgbd */
int gsr_rasterize_backward_seg(unsigned img_height, unsigned img_width, int num_points,
                               const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                               const float *xys, const float *conics, const float *colors,
                               const float *extra, const float *opacities, const float *background,
                               float extra_background, const float *final_Ts, const int32_t *final_idx,
                               const float *v_output, const float *v_output_extra,
                               const float *v_output_alpha, float *v_xy, float *v_conic,
                               float *v_colors, float *v_extra, float *v_opacity,
                               int deep_tile_threshold, int accumulators_zeroed, int segments,
                               int segment_min_entries, void *workspace, size_t workspace_bytes,
                               gsr_stream_t stream);

/* ---- absgrad: per-pixel |dL/dxy| sums (AbsGS; `absgrad` of gsplat) ---------------------------------------------
 * v_xy is a SIGNED sum over the pixels a Gaussian covers: where the pixels of a large Gaussian pull its centre in
 * opposite directions the sum cancels, and densification -- which thresholds its norm -- never splits it.  The three
 * entries below are gsr_rasterize_backward_seg / _two / _det with one more output, v_xy_abs [N,2] float32:
 *   v_xy_abs[g] = sum over every pixel p that composites g of |v_xy(p, g)|,
 *   v_xy(p, g)  = v_sigma (a dx + b dy, b dx + c dy),  v_sigma = -opac vis v_alpha,  (dx, dy) = xy_g - pixel centre,
 * the absolute value taken per component and per pixel, before any sum; same units as v_xy.  A pixel composites g
 * under the backward's unchanged rule: g is in the tile's list at or before final_idx[p], sigma >= 0, and alpha
 * (clamped at 0.99) is at least 1/255.  The call clears v_xy_abs itself (the forward's zero_ptr does not cover it,
 * whatever accumulators_zeroed says); _det writes every element and its sums are bit-reproducible.
 * v_xy_abs == NULL: the entry each one extends, launch for launch.  16 x 16 tiles, 3 colour channels (+ extra). */
int gsr_rasterize_backward_abs(unsigned img_height, unsigned img_width, int num_points,
                               const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                               const float *xys, const float *conics, const float *colors,
                               const float *extra, const float *opacities, const float *background,
                               float extra_background, const float *final_Ts, const int32_t *final_idx,
                               const float *v_output, const float *v_output_extra,
                               const float *v_output_alpha, float *v_xy, float *v_conic,
                               float *v_colors, float *v_extra, float *v_opacity,
                               int deep_tile_threshold, int accumulators_zeroed, int segments,
                               int segment_min_entries, void *workspace, size_t workspace_bytes,
                               float *v_xy_abs, gsr_stream_t stream);
int gsr_rasterize_backward_two_abs(unsigned img_height, unsigned img_width, int num_points,
                                   const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                   const int32_t *tile_bins2, int idx_base2, const float *xys,
                                   const float *conics, const float *colors, const float *extra,
                                   const float *opacities, const float *background, float extra_background,
                                   const float *final_Ts, const int32_t *final_idx, const float *v_output,
                                   const float *v_output_extra, const float *v_output_alpha, float *v_xy,
                                   float *v_conic, float *v_colors, float *v_extra, float *v_opacity,
                                   int deep_tile_threshold, int accumulators_zeroed, float *v_xy_abs,
                                   gsr_stream_t stream);
int gsr_rasterize_backward_det_abs(
    unsigned img_height, unsigned img_width, int num_points, int list_capacity,
    const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *extra, const float *opacities, const float *background,
    float extra_background, const float *final_Ts, const int32_t *final_idx,
    const float *v_output, const float *v_output_extra,
    const float *v_output_alpha, const int32_t *order,
    const int32_t *cum_sorted, int num_bands, const int32_t *slot_of_entry,
    void *workspace, size_t workspace_bytes, float *v_xy, float *v_conic,
    float *v_colors, float *v_extra, float *v_opacity, float *v_xy_abs, gsr_stream_t stream);

/* generic channel count; replace nd_rasterize_forward_tensor /
 * nd_rasterize_backward_tensor (bindings.cu:330-469), kernels
 * forward.cu:159-276 / backward.cu:23-131.  Accumulation is fp32 here (the
 * reference accumulates in __half). 1 <= channels <= GSR_MAX_CHANNELS; above 32
 * channels the lists are walked once per 32 channels (the reference keeps all
 * channels of a tile's 256 pixels in 48 KB of shared memory: ~90 at most). */
#define GSR_MAX_CHANNELS 1024
int gsr_rasterize_forward_nd(int tiles_x, int tiles_y, unsigned block_width,
                             unsigned img_width, unsigned img_height,
                             unsigned channels,
                             const int32_t *gaussian_ids_sorted,
                             const int32_t *tile_bins, const float *xys,
                             const float *conics, const float *colors,
                             const float *opacities, const float *background,
                             float *out_img, float *final_Ts,
                             int32_t *final_idx, gsr_stream_t stream);
int gsr_rasterize_backward_nd(unsigned img_height, unsigned img_width,
                              unsigned block_width, unsigned channels,
                              int num_points,
                              const int32_t *gaussian_ids_sorted,
                              const int32_t *tile_bins, const float *xys,
                              const float *conics, const float *colors,
                              const float *opacities, const float *background,
                              const float *final_Ts, const int32_t *final_idx,
                              const float *v_output,
                              const float *v_output_alpha, float *v_xy,
                              float *v_conic, float *v_colors,
                              float *v_opacity, gsr_stream_t stream);

/* replaces compute_cov2d_bounds_tensor (bindings.cu:39-56).
 * conics[n,3] radii[n] (fp32) */
int gsr_cov2d_bounds(int num_pts, const float *cov2d, float *conics,
                     float *radii, gsr_stream_t stream);

/* ======================= "next" rows =======================
 * f2 -- fused photometric loss head.  Replaces, for the caller
 * GaussianSplattingModel.get_loss_dict (gs_toolkit/models/vanilla_gs.py:926-944),
 * `torch.abs(gt - pred).mean()` + `1 - pytorch_msssim.SSIM(data_range=1,
 * size_average=True, channel=3)(gt, pred)` and their autograd backward.
 * pred, gt: [H,W,3] fp32.  maps: scratch [9, H-10, W-10] fp32 written by the
 * forward and consumed by the backward.  sums: workspace of
 * GSR_LOSS_WORKSPACE_DOUBLES doubles (partial sums in GSR_LOSS_SUM_SLOTS slots each,
 * so that the atomics do not serialise on one address),
 * zeroed by the call.  *loss_out = (1-l)*L1 + l*(1 - SSIM) and terms_out[2] =
 * {L1 = mean |pred-gt|, SSIM mean} (terms_out may be NULL), written by a
 * one-wave kernel behind the main one.  clamp_pred != 0: the prediction is min(pred, 1), as after the models'
 * `torch.clamp(rgb, max=1.0)`, and the gradient is zero where pred > 1.
 * backward: v_pred[H,W,3] = upstream[0] * d loss / d pred (upstream on device). */
#define GSR_LOSS_SUM_SLOTS 64
#define GSR_LOSS_WORKSPACE_DOUBLES (2 * GSR_LOSS_SUM_SLOTS)
int gsr_l1_ssim_forward(unsigned img_height, unsigned img_width,
                        float ssim_lambda, int clamp_pred, const float *pred,
                        const float *gt, float *maps, double *sums,
                        float *loss_out, float *terms_out, gsr_stream_t stream);
int gsr_l1_ssim_backward(unsigned img_height, unsigned img_width,
                         float ssim_lambda, int clamp_pred,
                         const float *upstream, const float *pred,
                         const float *gt, const float *maps, float *v_pred,
                         gsr_stream_t stream);

/* f2, the photometric head of the co-gs model as its source computes it
 * (gs_toolkit/models/depth_gs.py:445-448: the `+ ssim_lambda * simloss` line is a
 * stand-alone expression statement, so `main_loss` = (1 - ssim_lambda) * L1 only):
 *   *loss_out = weight * mean |min(pred, 1) - gt|   (clamp_pred != 0; pred as is otherwise)
 * pred, gt: num_values fp32 each (an [H,W,3] image: 3 H W), 16-byte aligned.  sums:
 * workspace of GSR_LOSS_SUM_SLOTS doubles, zeroed by the call.  backward:
 * v_pred = upstream[0] * weight * sign(pred - gt) / num_values, 0 where pred > 1
 * under clamp_pred (upstream on the device). */
int gsr_l1_forward(long long num_values, float weight, int clamp_pred,
                   const float *pred, const float *gt, double *sums,
                   float *loss_out, gsr_stream_t stream);
int gsr_l1_backward(long long num_values, float weight, int clamp_pred,
                    const float *upstream, const float *pred, const float *gt,
                    float *v_pred, gsr_stream_t stream);

/* f2, depth head of the co-gs model (gs_toolkit/models/depth_gs.py:356-363, 531-538):
 *   pred = alpha > 0 ? depth / alpha : *depth_max      (depth_max: device float, the
 *                                                       detached maximum of `depth`)
 *   loss = mean over all pixels of |gt - pred| where gt > 0 (0 elsewhere)
 * depth = the depth pass of the compositing (depths as colours), alpha = 1 - T of the
 * RGB pass, gt = sensor / estimated depth; all [num_pixels] fp32.  sums: workspace of
 * GSR_LOSS_SUM_SLOTS doubles.  backward: cotangents of `depth` and `alpha`
 * (upstream[0] = d L / d loss, on the device). */
int gsr_depth_l1_forward(long long num_pixels, const float *depth,
                         const float *alpha, const float *gt,
                         const float *depth_max, double *sums, float *loss_out,
                         gsr_stream_t stream);
int gsr_depth_l1_backward(long long num_pixels, const float *upstream,
                          const float *depth, const float *alpha,
                          const float *gt, const float *depth_max,
                          float *v_depth, float *v_alpha, gsr_stream_t stream);

/* f2 with a per-view mask, as the models apply one in front of their losses
 * (vanilla_gs.py:915-924, surface_gs.py:917-925, depth_gs.py:424-437, 533-538): both images
 * are MULTIPLIED by the mask -- nothing is selected and no mean is renormalised by the
 * mask's area.  mask: [H,W] fp32, one value per pixel shared by its channels, any real
 * number (a mask resized under the resolution schedule is fractional).  With
 *   x = (clamp_pred ? min(pred, 1) : pred) * m,   y = gt * m      (both rounded to fp32)
 * the three heads compute from x and y exactly what the unmasked entry points compute
 * from pred and gt, same workspaces, same divisors (3 H W, 3 (H-10) (W-10), num_values,
 * num_pixels); their backward is v_pred = m * (d loss / d x), 0 where pred > 1 under
 * clamp_pred.  gsr_l1_masked_*: num_values = 3 H W and element e takes mask[e / 3].
 * Depth head: g' = gt * m, p' = pred * m, loss = mean over all pixels of |g' - p'| where
 * g' > 0; the cotangents of `depth` and `alpha` are the unmasked chain scaled by m.
 * The mask is a constant: it has no cotangent. */
int gsr_l1_ssim_masked_forward(unsigned img_height, unsigned img_width,
                               float ssim_lambda, int clamp_pred,
                               const float *pred, const float *gt,
                               const float *mask, float *maps, double *sums,
                               float *loss_out, float *terms_out,
                               gsr_stream_t stream);
int gsr_l1_ssim_masked_backward(unsigned img_height, unsigned img_width,
                                float ssim_lambda, int clamp_pred,
                                const float *upstream, const float *pred,
                                const float *gt, const float *mask,
                                const float *maps, float *v_pred,
                                gsr_stream_t stream);
int gsr_l1_masked_forward(long long num_values, float weight, int clamp_pred,
                          const float *pred, const float *gt,
                          const float *mask, double *sums, float *loss_out,
                          gsr_stream_t stream);
int gsr_l1_masked_backward(long long num_values, float weight, int clamp_pred,
                           const float *upstream, const float *pred,
                           const float *gt, const float *mask, float *v_pred,
                           gsr_stream_t stream);
int gsr_depth_l1_masked_forward(long long num_pixels, const float *depth,
                                const float *alpha, const float *gt,
                                const float *mask, const float *depth_max,
                                double *sums, float *loss_out,
                                gsr_stream_t stream);
int gsr_depth_l1_masked_backward(long long num_pixels, const float *upstream,
                                 const float *depth, const float *alpha,
                                 const float *gt, const float *mask,
                                 const float *depth_max, float *v_depth,
                                 float *v_alpha, gsr_stream_t stream);

/* ---- SH colours from split coefficients (caller-side glue) --
 * gsr_sh_forward / gsr_sh_backward for models that keep the DC band and the
 * higher bands as two parameters (features_dc [n,3], features_rest [n,K-1,3])
 * and torch.cat them before every render (gs_toolkit/models/vanilla_gs.py:809,
 * `colors_crop = torch.cat(...)`): no concatenated copy is made, the gradients
 * are written straight into v_dc [n,3] and v_rest [n,K-1,3].  degree in [0,3]
 * (K = (degree+1)^2; degree 0: the DC band only, viewdirs / rest / v_rest may be NULL).  Optional epilogue of the models (vanilla_gs.py:826,
 * `torch.clamp(rgbs + 0.5, min=0.0)`): colors = sh + shift, cut at 0 when
 * clamp_zero != 0 -- a channel that was cut is stored as -0.0, so that the backward,
 * which takes those colours (clamped_colors, NULL if not clamped), blocks the gradient
 * exactly where sh + shift < 0 and passes it where it is >= 0, like torch.clamp.
 * The bands of `rest` above degrees_to_use and, at degrees_to_use == 0, viewdirs are not observed (see
 * gsr_sh_forward); those bands of v_rest are written as exact zeros. */
int gsr_sh_forward_split(unsigned num_points, unsigned degree,
                         unsigned degrees_to_use, const float *viewdirs,
                         const float *dc, const float *rest, float *colors,
                         float shift, int clamp_zero, gsr_stream_t stream);
int gsr_sh_backward_split(unsigned num_points, unsigned degree,
                          unsigned degrees_to_use, const float *viewdirs,
                          const float *v_colors, const float *clamped_colors,
                          float *v_dc, float *v_rest, gsr_stream_t stream);

/* SH backward over SEVERAL views at once: what per-view data parallelism exchanges instead of the SH
 * gradient itself.  One view's gradient is rank one per Gaussian, v_coeffs[g,k,:] = B_k(dir_g) v_colors[g,:], so
 * ranks all-gather their v_colors (12 B per Gaussian; already masked by the clamp epilogue, if any) and camera
 * positions instead of all-reducing 12 K bytes per Gaussian, and each forms
 *   scale * sum_r B_k(normalize(means3d[g] - camera_positions[r])) * v_colors[r][g]      (views in order r)
 * itself -- the same sum on every rank.  v_colors: view r at v_colors + r * v_colors_stride floats, [n,3] each;
 * camera_positions: view r at camera_positions + r * camera_stride floats.  Output: v_coeffs [n,K,3], or
 * (v_coeffs NULL) v_dc [n,3] and v_rest [n,K-1,3]; K = (degree+1)^2, degree in [0,3]; bands above degrees_to_use
 * are written as exact zeros, also for a Gaussian that sits exactly at a camera position (a zero direction: NaN in the
 * bands 1 .. in use only; at degrees_to_use == 0 the positions are not observed).  The direction is formed as
 * gsr_activate_forward forms it. */
int gsr_sh_backward_views(unsigned num_points, unsigned degree, unsigned degrees_to_use,
                          unsigned num_views, const float *means3d,
                          const float *camera_positions, size_t camera_stride,
                          const float *v_colors, size_t v_colors_stride, float scale,
                          float *v_dc, float *v_rest, float *v_coeffs, gsr_stream_t stream);

/* ---- RGB + one extra channel in ONE compositing pass -------
 * The models composite twice per view when they need a depth image: RGB, then
 * depths repeated as three colours over a zero background (vanilla_gs.py:840-855,
 * depth_gs.py:346-363).  These two calls composite colors [n,3] and extra [n]
 * (one scalar per Gaussian, e.g. its depth) together: out_img [H,W,3] over
 * `background`, out_extra [H,W] over `extra_background`; final_Ts / final_idx as
 * gsr_rasterize_forward.  block_width is 16.  The backward takes the cotangents of
 * both images (and of alpha, NULL = 0) and returns v_extra [n] next to the usual four.
 * out_alpha / zero_ptr / zero_bytes / accumulators_zeroed: as in gsr_rasterize_forward_ex /
 * gsr_rasterize_backward_ex (the accumulators are v_xy .. v_opacity, v_extra: 10 n floats). */
int gsr_rasterize_forward_rgbd(int tiles_x, int tiles_y, unsigned img_width,
                               unsigned img_height,
                               const int32_t *gaussian_ids_sorted,
                               const int32_t *tile_bins, const float *xys,
                               const float *conics, const float *colors,
                               const float *extra, const float *opacities,
                               const float *background, float extra_background,
                               float *out_img, float *out_extra,
                               float *final_Ts, int32_t *final_idx,
                               int deep_tile_threshold, float *out_alpha,
                               void *zero_ptr, size_t zero_bytes,
                               gsr_stream_t stream);
int gsr_rasterize_backward_rgbd(unsigned img_height, unsigned img_width,
                                int num_points,
                                const int32_t *gaussian_ids_sorted,
                                const int32_t *tile_bins, const float *xys,
                                const float *conics, const float *colors,
                                const float *extra, const float *opacities,
                                const float *background, float extra_background,
                                const float *final_Ts, const int32_t *final_idx,
                                const float *v_output,
                                const float *v_output_extra,
                                const float *v_output_alpha, float *v_xy,
                                float *v_conic, float *v_colors, float *v_extra,
                                float *v_opacity, int deep_tile_threshold,
                                int accumulators_zeroed, gsr_stream_t stream);

/* ---- two-round lists for deep scenes (block_width 16; docs/history/DESIGN_r01-r05.md section 4.11) --------------------
 * replaces, like gsr_bin_sorted + gsr_rasterize_forward / _backward, the list construction of
 * rasterizer/utils.py:106-182 and the walks of forward.cu:278-395 / backward.cu:133-303 -- with the SAME
 * results: on a scene whose tiles saturate early (3 M Gaussians at 4K: 97.7 M list entries built, 4.1 M ever
 * read) almost every entry lies behind the depth at which its tile's pixels have all finished.  The lists of
 * the NEAREST Gaussians (a prefix of the depth order) are a prefix of every tile's list:
 *   1. gsr_tile_lists_subrange over order[0 : n1]            -> lists 1 (ids at gaussian_ids_sorted + 0)
 *   2. gsr_rasterize_forward_round(1, lists 1)               -> final values where every pixel has finished, raw
 *                                                               per-pixel state + tile_flags (bit p: sub-tile p
 *                                                               holds raw state; zero them first) elsewhere
 *   3. gsr_saturation_filter over order[n1 : n]              -> order_out: the same ids, with `dummy_index` (the
 *                                                               index of a culled record, e.g. one appended row)
 *                                                               in place of every Gaussian whose tile box holds
 *                                                               no flagged tile
 *   4. gsr_tile_lists_subrange over order[n1 : n]            -> lists 2 (ids at gaussian_ids_sorted + idx_base,
 *                                                               tile_bins2 relative to idx_base)
 *   5. gsr_rasterize_forward_round(2, lists 2, idx_base)     -> resumes and finalises the flagged sub-tiles
 *   6. gsr_rasterize_backward_two(tile_bins, tile_bins2, idx_base)
 * A tile's list is its range in tile_bins followed by its range in tile_bins2; per pixel the instruction
 * sequence is that of one walk over the concatenation, so images, final_Ts and final_idx (an index into
 * gaussian_ids_sorted, as always) are bit-identical to the single walk over the full lists, gradients equal up to
 * the order of the float atomics.  extra / out_extra / v_output_extra / v_extra: the fourth channel of the
 * _rgbd calls, all NULL for three channels.  stats_out (nullable, int32[2], device-accessible): flagged tiles,
 * Gaussians kept. */
size_t gsr_tile_lists_subrange_workspace_bytes(int count, int capacity, int tiles_x, int tiles_y);
int gsr_tile_lists_subrange(int count, int capacity, const int32_t *order, const void *reach_records,
                            int tiles_x, int tiles_y, int32_t *gaussian_ids_sorted, int32_t *tile_bins,
                            int32_t *count_out, void *workspace, size_t workspace_bytes,
                            gsr_stream_t stream);
size_t gsr_saturation_filter_workspace_bytes(int tiles_x, int tiles_y);
int gsr_saturation_filter(int count, const int32_t *order, const void *reach_records, int dummy_index,
                          const int32_t *tile_flags, int tiles_x, int tiles_y, int32_t *order_out,
                          void *workspace, size_t workspace_bytes, int32_t *stats_out,
                          gsr_stream_t stream);
int gsr_rasterize_forward_round(int round, int tiles_x, int tiles_y, unsigned img_width,
                                unsigned img_height, const int32_t *gaussian_ids_sorted,
                                const int32_t *tile_bins, int idx_base, const float *xys,
                                const float *conics, const float *colors, const float *extra,
                                const float *opacities, const float *background, float extra_background,
                                float *out_img, float *out_extra, float *final_Ts, int32_t *final_idx,
                                int32_t *tile_flags, int deep_tile_threshold, float *out_alpha,
                                void *zero_ptr, size_t zero_bytes, gsr_stream_t stream);
int gsr_rasterize_backward_two(unsigned img_height, unsigned img_width, int num_points,
                               const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                               const int32_t *tile_bins2, int idx_base2, const float *xys,
                               const float *conics, const float *colors, const float *extra,
                               const float *opacities, const float *background, float extra_background,
                               const float *final_Ts, const int32_t *final_idx, const float *v_output,
                               const float *v_output_extra, const float *v_output_alpha, float *v_xy,
                               float *v_conic, float *v_colors, float *v_extra, float *v_opacity,
                               int deep_tile_threshold, int accumulators_zeroed, gsr_stream_t stream);

/* ---- a whole view as ONE call (host-bound scenes and viewer frames) -----
 * The body of GaussianSplattingModel.get_outputs between the raw parameters and the images
 * (gs_toolkit/models/vanilla_gs.py:765-857: activations, project_gaussians, SH + 0.5 clamped,
 * tile lists, compositing -- with the depth image from the same pass when render_depth) and its
 * autograd backward, as two calls instead of ~18: the same exported functions in the same order,
 * run from C.  Nothing is allocated in here: every pointer is a caller-owned DEVICE buffer of the
 * size the per-stage function documents (n = num_points, P = H x W, T = tiles, 16 x 16 tiles).
 *   counts / cum      both NULL: lists without counts (gsr_bin_sorted_needs_counts() == 0 for
 *                     (n, capacity, grid, device_sized = 1)); else i32[n] each
 *   sort_ws / bin_ws  gsr_depth_order_workspace_bytes(n, 1) / gsr_bin_sorted_workspace_bytes(n, capacity, ..)
 *   count_out         i32[1], device or pinned host memory: entries the view needs (> capacity: cut)
 *   out_depth         [P], required iff render_depth;  out_alpha [P] nullable
 *   zero_ptr/bytes    the backward's accumulators (6 + 3 + render_depth floats per Gaussian), cleared
 *                     by the compositing launch; NULL: none */
typedef struct gsr_view_desc {
  int num_points, sh_degree, sh_degree_to_use, render_depth;
  int img_height, img_width;
  float fx, fy, cx, cy, glob_scale, clip_thresh;
  int capacity, deep_tile_threshold;
  const float *means, *log_scales, *raw_quats, *logits, *features_dc, *features_rest;
  const float *viewmat, *projmat, *campos, *background;
  float *scales, *quats, *opac, *dirs, *cov3d, *xys, *depths;
  int32_t *radii;
  float *conics, *comp;
  int32_t *tiles;
  float *colors;
  void *reach_records;
  int32_t *counts, *order, *cum, *ids, *tile_bins, *count_out;
  void *sort_ws;
  size_t sort_ws_bytes;
  void *bin_ws;
  size_t bin_ws_bytes;
  float *out_img, *out_depth, *final_Ts;
  int32_t *final_idx;
  float *out_alpha;
  void *zero_ptr;
  size_t zero_bytes;
  /* depth segments of the compositing, forward and backward (gsr_rasterize_forward_seg / _backward_seg):
   * segments < 2 = off; seg_ws: gsr_rasterize_forward_seg_workspace_bytes(...) bytes for gsr_view_forward,
   * gsr_rasterize_backward_seg_workspace_bytes(...) for gsr_view_backward (each call with its own `segments`) */
  int segments, segment_min_entries;
  void *seg_ws;
  size_t seg_ws_bytes;
  /* antialiased != 0: the view composites opac_aa [n] = opac * comp (gsr_project_forward_aa writes it; the lists,
   * the compositing and its backward read it where they read opac, gsr_project_backward_aa turns the accumulated
   * cotangent into opac's in place).  0: every call is the classic sequence and opac_aa may be NULL. */
  int antialiased;
  float *opac_aa;
} gsr_view_desc;

/* cotangents in, parameter gradients out.  accumulators: (9 + render_depth) n floats laid out
 * v_xy | v_conic | v_colors | v_opacity [| v_depths]; accumulators_zeroed != 0 when the forward's
 * launch cleared them (zero_ptr).  stats_first != NULL: also after_train's statistics
 * (gsr_densify_stats_dev).  tmp_*: scratch of [n,3] [n,6] [n,3] [n,4] floats.  v_dc == NULL: no SH backward --
 * the colour cotangents stay in the accumulators (before the clamp of the colours is applied to them) for a caller
 * that forms the SH gradient over several views (gsr_sh_backward_views). */
typedef struct gsr_view_grads {
  const float *v_img, *v_alpha, *v_depth; /* v_alpha / v_depth nullable (v_depth required iff render_depth) */
  float *accumulators;
  int accumulators_zeroed;
  const int32_t *stats_first;
  float stats_inv_size;
  float *xys_grad_norm;
  int32_t *vis_counts;
  float *max_2dsize;
  float *tmp_v_cov2d, *tmp_v_cov3d, *tmp_v_scales, *tmp_v_quats;
  float *v_means, *v_log_scales, *v_raw_quats, *v_logits, *v_dc, *v_rest;
  /* != 0: `accumulators` already hold the compositing backward's sums -- a caller that ran
   * gsr_rasterize_backward_det on the view's lists for a fixed summation order: that launch is skipped here
   * (v_img may then be NULL) and everything behind it runs as usual */
  int accumulators_final;
  /* NULL, or [n,2]: the absgrad of gsr_rasterize_backward_abs.  The compositing backward of this call overwrites it
   * (with accumulators_final the caller's gsr_rasterize_backward_det_abs has), and the statistics accumulate ITS
   * norm into xys_grad_norm in place of v_xy's. */
  float *v_xy_abs;
} gsr_view_grads;

int gsr_view_forward(const gsr_view_desc *view, gsr_stream_t stream);
/* gsr_view_forward with the oriented crop box of gsr_project_forward_crop: `crop` != NULL is float32[16] on the
 * device, the projection is that entry and a Gaussian outside the box is culled (gsr_view_backward, unchanged, then
 * returns zero gradients for it in every group).  crop == NULL: gsr_view_forward, call for call.  The pointer rides
 * next to the descriptor, not in it: gsr_view_desc keeps its layout and its size. */
int gsr_view_forward_crop(const gsr_view_desc *view, const float *crop, gsr_stream_t stream);

/* ---- the forward of rasterize_gaussians as ONE call ------------------------------------------
 * What `_RasterizeGaussians.forward` runs on the device (gs_toolkit/gs_components/rasterizer/rasterize.py:89-170:
 * bin_and_sort_gaussians, utils.py:128-182, then rasterize_forward) for 16 x 16 tiles and 3 colour channels: reach
 * records + depth order, device-sized tile lists, compositing (with alpha = 1 - T, the backward's cleared
 * accumulators, and optionally one extra channel, as gsr_rasterize_forward_ex / _rgbd).  The same exported functions
 * in the same order as the Python package would call them one by one; nothing is allocated in here.  The unchanged
 * models read `(num_tiles_hit > 0).any()` back right in front of this op (vanilla_gs.py:811): the GPU idles from
 * that read-back until the first launch below, so the host time in between is kept to one call.
 *   counts / cum   both NULL: lists without counts (gsr_bin_sorted_needs_counts() == 0); else i32[n] each
 *   order_ready    NULL, or the depth order already built for these depths / radii (gsr_depth_order(depths, radii,
 *                  NULL...), e.g. on another stream while the caller was busy): the sort is skipped and only the
 *                  records are written (needs counts == NULL); `order` / sort_ws may then be NULL
 *   reach_records  [n x gsr_reach_record_bytes()], 16-byte aligned;  order i32[n]
 *   sort_ws/bin_ws gsr_depth_order_workspace_bytes(n, 1) / gsr_bin_sorted_workspace_bytes(n, capacity, ..)
 *   ids i32[capacity], tile_bins i32[T,2], count_out i32[1] (device or pinned): entries needed (> capacity: cut)
 *   extra / out_extra  NULL, or [n] / [P]: one more channel composited with the same weights (the depths)
 *   out_img == NULL    the lists only: no compositing (colors / background / final_* / out_alpha / zero_ptr unused);
 *                      the caller composites later with gsr_rasterize_forward_ex -- how the Python package builds
 *                      a view's lists on a side stream while the models wait for their read-backs */
typedef struct gsr_raster_desc {
  int num_points, img_height, img_width, capacity, deep_tile_threshold;
  float extra_background;
  const float *xys, *depths;
  const int32_t *radii;
  const float *conics, *colors, *extra, *opac, *background;
  const int32_t *order_ready;
  void *reach_records;
  int32_t *counts, *order, *cum, *ids, *tile_bins, *count_out;
  void *sort_ws;
  size_t sort_ws_bytes;
  void *bin_ws;
  size_t bin_ws_bytes;
  float *out_img, *out_extra, *final_Ts;
  int32_t *final_idx;
  float *out_alpha;
  void *zero_ptr;
  size_t zero_bytes;
  /* depth segments of the compositing (gsr_rasterize_forward_seg): segments < 2 = off */
  int segments, segment_min_entries;
  void *seg_ws;
  size_t seg_ws_bytes;
  int deep_tile_threshold_backward; /* > 0 with GSR_DEEP_ORDERED | GSR_DEEP_SECOND: the coming backward's argument --
                                       its job order is written by the same launch as the forward's (the backward
                                       then passes it with GSR_DEEP_PREBUILT); 0: not built */
} gsr_raster_desc;
int gsr_rasterize_gaussians_forward(const gsr_raster_desc *desc, gsr_stream_t stream);
int gsr_view_backward(const gsr_view_desc *view, const gsr_view_grads *grads, gsr_stream_t stream);

/* ---- per-Gaussian activations (caller-side glue) ----------
 * exp(scales), quats / |quats|, sigmoid(opacities) and the normalised view
 * directions means - camera_position of GaussianSplattingModel.get_outputs
 * (gs_toolkit/models/vanilla_gs.py:765-826) in one launch, and their VJP in one
 * launch.  camera_position: 3 floats on the device (may be NULL together with
 * viewdirs).  Backward: v_scales / v_quats / v_opacities may each be NULL (= 0);
 * no gradient flows to the view directions (the reference detaches the means). */
int gsr_activate_forward(int num_points, const float *means,
                         const float *log_scales, const float *raw_quats,
                         const float *opacity_logits,
                         const float *camera_position, float *scales,
                         float *quats, float *opacities, float *viewdirs,
                         gsr_stream_t stream);
int gsr_activate_backward(int num_points, const float *raw_quats,
                          const float *scales, const float *quats,
                          const float *opacities, const float *v_scales,
                          const float *v_quats, const float *v_opacities,
                          float *v_log_scales, float *v_raw_quats,
                          float *v_logits, gsr_stream_t stream);

/* ---- 3D smoothing filter (csrc/filter3d.hip) -------------------------
 * Mip-Splatting's 3D filter (Yu et al., CVPR 2024, section 4.1): every Gaussian is convolved with
 * an isotropic Gaussian of the size its best-sampling training camera resolves.
 *
 * gsr_filter3d_sampling: means float [N,3]; cameras float [V,20] ON THE DEVICE, 16-byte aligned,
 * per row [0,12) the top 3x4 of the world->camera matrix (row-major), [12,18) fx, fy, cx, cy,
 * width, height, [18,20) unread.  Per Gaussian (X, Y, Z) and camera, in float32, every operation
 * rounded on its own in the order written (tests/filter3d_reference.py restates it in NumPy):
 *   x = ((r00 X + r01 Y) + r02 Z) + t0     (y with row 1, z with row 2)
 *   u = (x / z) fx + cx,   w = (y / z) fy + cy
 *   seen = z > near && u >= -(margin W) && u <= W + margin W
 *                   && w >= -(margin H) && w <= H + margin H      (a NaN compares false: unseen)
 *   nu = the largest fx / z over the cameras that see it, visited in index order; 0 when none does
 *   filter = k / nu for the seen, k / min{nu : nu > 0} for the unseen (the largest filter of any
 *            seen Gaussian), 0 for all when no camera sees any Gaussian.
 * k = sqrt(variance) as the caller rounded it.  Three launches on `stream`: `workspace`
 * (GSR_FILTER3D_WORKSPACE_BYTES on the device, 4-byte aligned, any content) is cleared, the rates
 * go to filter_out and their smallest positive one into the workspace by an integer atomic on the
 * bit patterns (no float atomics: bit-reproducible), and a second pass over filter_out applies
 * the fallback.  No read-back, no synchronisation, nothing allocated: capturable.  num_points = 0
 * launches nothing; num_cameras <= 0, a null pointer and a misaligned `cameras` are GSR_EINVAL
 * before any launch.
 *
 * gsr_activate_filtered_forward / _backward: gsr_activate_forward / _backward with the filter
 * folded into the scales and the opacity, filter_3d float [N], no gradient to it.  With
 * s_k = exp(l_k), o = sigmoid(a), f = filter_3d[i]:
 *   s'_k = sqrt(s_k^2 + f^2),   c = prod_k s_k / s'_k,   o' = o c        (scales, opacities)
 *   v_a = v_o' c o (1 - o),   v_l_k = v_s'_k s_k^2 / s'_k + v_o' o c f^2 / s'_k^2
 * Quaternions and view directions as in gsr_activate_forward.  A row with f == 0 takes the
 * unfiltered expressions and carries the bits gsr_activate_forward / _backward produce.
 * The backward reads the RAW log_scales and opacity_logits (5 words per Gaussian with the filter)
 * rather than the forward's outputs (4 words): s_k cannot be recovered from s'_k and f where
 * f >> s_k (s'^2 - f^2 cancels), and the raw parameters are alive anyway, so nothing extra is
 * kept for the backward.  One launch each; v_scales / v_quats / v_opacities may each be NULL. */
#define GSR_FILTER3D_WORKSPACE_BYTES 16
int gsr_filter3d_sampling(int num_points, const float *means, int num_cameras,
                          const float *cameras, float k, float near, float margin,
                          float *filter_out, void *workspace, gsr_stream_t stream);
int gsr_activate_filtered_forward(int num_points, const float *means, const float *log_scales,
                                  const float *raw_quats, const float *opacity_logits,
                                  const float *camera_position, const float *filter_3d,
                                  float *scales, float *quats, float *opacities, float *viewdirs,
                                  gsr_stream_t stream);
int gsr_activate_filtered_backward(int num_points, const float *raw_quats,
                                   const float *log_scales, const float *quats,
                                   const float *opacity_logits, const float *filter_3d,
                                   const float *v_scales, const float *v_quats,
                                   const float *v_opacities, float *v_log_scales,
                                   float *v_raw_quats, float *v_logits, gsr_stream_t stream);

/* ---- k-means (csrc/kmeans.hip) -----------------------------------------
 * Lloyd's k-means over N rows of D floats with K centres, 1 <= D <= GSR_KMEANS_MAX_DIM,
 * 1 <= K <= GSR_KMEANS_MAX_CLUSTERS: what builds the codebook of the spherical-harmonics rows of a
 * compressed export (gs_io.compressed).  points float [N,D], centroids float [K,D], row-major.
 *
 * gsr_kmeans_assign: labels int32 [N], dist float [N].  The rule, in float32
 * (tests/kmeans_reference.py restates it in NumPy; the kernel is held to it bit for bit):
 *   d(i,k) = sum_{j = 0..D-1} (x_ij - c_kj)^2, accumulated in the order j = 0, 1, ... from 0.0f;
 *            the subtraction, the product and the addition each rounded on its own (no contraction)
 *   best = +inf, label = 0;  for k = 0..K-1 in order:  if (d(i,k) < best) { best = d; label = k; }
 * Ties go to the lowest index.  A row whose distances are all NaN or +inf keeps label 0, and dist
 * takes the `best` that was left (+inf).  A NaN centroid never wins.  One launch; centroids pass
 * through LDS in tiles of GSR_KMEANS_TILE rows.
 *
 * gsr_kmeans_update: order int32 [N] is the STABLE sort of 0..N-1 by label and offsets int32 [K+1]
 * the segment starts (cluster k owns order[offsets[k] .. offsets[k+1])); weights float [N], >= 0,
 * or NULL (every weight 1).  Per cluster and component, S_j = sum w_i x_ij and W = sum w_i in
 * float64 (each product is exact); new_kj = float32(S_j / W).  The order of the additions depends
 * on the segment's length and the launch constants only -- thread t of 256 adds the members
 * t, t + 256, ... in order, a butterfly adds a wave's lanes, the four waves are added in index
 * order -- and there are no atomics: bit-reproducible.  A cluster without a member, or with W == 0,
 * copies old_centroids' bits; counts int32 [K] takes the segments' lengths.  A member whose label is
 * not the segment's cluster or whose index is outside [0, N) is skipped, and offsets are clamped
 * to [0, N].  new_centroids must not alias old_centroids.  One launch, K workgroups.
 *
 * gsr_kmeans_inertia: out double [1] on the device = sum_i w_i sum_j (x_ij - c_{l_i j})^2 with
 * every operation in float64, j in index order, summed lane -> wave -> workgroup -> grid in a
 * fixed order, no atomics (workspace: GSR_KMEANS_INERTIA_WORKSPACE_DOUBLES(N) doubles on the
 * device, 8-byte aligned, any content).  A label outside [0, K) adds nothing.  This, not the
 * float32 dist, is the quantity Lloyd's iteration decreases.  Two launches; N = 0 writes 0.
 *
 * All three: nothing allocated, no read-back, no synchronisation (capturable); sizes out of range
 * and null pointers are GSR_EINVAL before any launch; N = 0 is allowed (assign launches nothing,
 * update copies the old centroids and writes zero counts). */
#define GSR_KMEANS_MAX_DIM 48
#define GSR_KMEANS_MAX_CLUSTERS 65536
#define GSR_KMEANS_TILE 128
#define GSR_KMEANS_INERTIA_SHARE 1024 /* points per workgroup */
#define GSR_KMEANS_INERTIA_WORKSPACE_DOUBLES(n) \
  (((n) + GSR_KMEANS_INERTIA_SHARE - 1) / GSR_KMEANS_INERTIA_SHARE)
int gsr_kmeans_assign(int num_points, int dim, int num_clusters, const float *points,
                      const float *centroids, int32_t *labels, float *dist, gsr_stream_t stream);
int gsr_kmeans_update(int num_points, int dim, int num_clusters, const float *points,
                      const int32_t *labels, const int32_t *order, const int32_t *offsets,
                      const float *weights, const float *old_centroids, float *new_centroids,
                      int32_t *counts, gsr_stream_t stream);
int gsr_kmeans_inertia(int num_points, int dim, int num_clusters, const float *points,
                       const float *centroids, const int32_t *labels, const float *weights,
                       double *out, void *workspace, gsr_stream_t stream);

/* ---- densification statistics -----------------------------
 * GaussianSplattingModel.after_train (gs_toolkit/models/vanilla_gs.py:344-372) in
 * one launch: for every Gaussian with radii > 0,
 *   xys_grad_norm += |v_xys| (skipped if v_xys is NULL), vis_counts += 1,
 *   max_2dsize = max(max_2dsize, radii * inv_size),   inv_size = 1 / max(W, H).
 * first != 0 is the reference's first call after a refinement (:354-356,
 * `xys_grad_norm = grads; vis_counts = ones`): EVERY Gaussian gets count 1 and its
 * gradient norm (zero for the invisible ones), max_2dsize starts from 0; the three
 * arrays need not be initialised. */
int gsr_densify_stats(int num_points, const float *v_xys, const int32_t *radii,
                      float inv_size, int first, float *xys_grad_norm,
                      int32_t *vis_counts, float *max_2dsize,
                      gsr_stream_t stream);
/* the same with `first` read from device memory (one int32): the call can then sit in
 * a captured HIP graph that is replayed across refinement boundaries */
int gsr_densify_stats_dev(int num_points, const float *v_xys,
                          const int32_t *radii, float inv_size,
                          const int32_t *first, float *xys_grad_norm,
                          int32_t *vis_counts, float *max_2dsize,
                          gsr_stream_t stream);

/* ---- refinement: densify / split / duplicate / cull --------
 * GaussianSplattingModel.refinement_after (gs_toolkit/models/vanilla_gs.py:381-497)
 * with split_gaussians :540-592, dup_gaussians :594-603, cull_gaussians :499-538 and
 * the optimizer surgery dup_in_optim :303-337 / remove_from_optim :282-301, as a
 * plan (decisions + final positions) and ONE compaction launch over all tensors.
 * The host decides the branch from the step counter and fills the config:
 *   densify              step < stop_split_at and step % (reset_alpha_every *
 *                        refine_every) > num_train_data + refine_every  (:390-395);
 *                        0 = cull only (:459-463)
 *   split_by_screen_size step < stop_screen_size_at (:421)
 *   cull_big             step > refine_every * reset_alpha_every (:512)
 *   cull_by_screen_size  step < stop_screen_size_at (:518)
 *   half_max_dim         0.5 * max(W, H) of the last rendered view (:404-408)
 * gsr_refine_plan writes flags[n] (bit 0: the original survives, 1: its split
 * children survive, 2: its duplicate survives, 3: it was split), offsets[n,4] (i32,
 * 16-byte aligned: exclusive prefix counts of those four bits) and counts[4] =
 * {kept originals K0, kept split sources Ks, kept duplicates Kd, split sources}.
 * The output has K0 + n_split_samples * Ks + Kd rows: the caller reads counts back,
 * allocates, and calls gsr_refine_apply, which moves/creates the rows of up to
 * GSR_REFINE_MAX_TENSORS tensors ([n, width] fp32 each) in one launch:
 * originals in order, then split children sample by sample, then duplicates -- the
 * order of the reference's cat + cull.  kind says what new rows hold:
 *   COPY        the parent's row (quats, features_dc, features_rest, opacities)
 *   LOG_SCALES  log(exp(s) / 1.6) for children (and duplicates) of a split Gaussian
 *   MEANS       split children: mean + R(q/|q|) (exp(s) * z), z ~ N(0,1)
 *   MOMENT      zeros (exp_avg / exp_avg_sq of the new rows)
 * z comes from samples [n_split_samples * split sources, 3] (row j * sources +
 * rank, the reference's torch.randn layout) or, if samples is NULL, from
 * Philox4x32-10 with key = seed and counter = (Gaussian index, j, 0, 0) + Box-Muller.
 * vis_counts is int32 (gsr_densify_stats); max_2dsize may be NULL when no
 * screen-size rule is on. */
typedef struct {
  float densify_grad_thresh;
  float densify_size_thresh;
  float split_screen_size;
  float cull_alpha_thresh;
  float cull_scale_thresh;
  float cull_screen_size;
  float half_max_dim;
  int n_split_samples;
  int densify;
  int split_by_screen_size;
  int cull_big;
  int cull_by_screen_size;
} gsr_refine_config;
#define GSR_REFINE_COPY 0
#define GSR_REFINE_LOG_SCALES 1
#define GSR_REFINE_MEANS 2
#define GSR_REFINE_MOMENT 3
#define GSR_REFINE_MAX_TENSORS 24
typedef struct {
  const float *in; /* [n, width] */
  float *out;      /* [K0 + n_split_samples * Ks + Kd, width] */
  int width;
  int kind;
} gsr_refine_tensor;
size_t gsr_refine_workspace_bytes(int num_points);
int gsr_refine_plan(int num_points, const float *log_scales,
                    const float *opacity_logits, const float *xys_grad_norm,
                    const int32_t *vis_counts, const float *max_2dsize,
                    const gsr_refine_config *cfg, uint8_t *flags,
                    int32_t *offsets, int32_t *counts, void *workspace,
                    size_t workspace_bytes, gsr_stream_t stream);
int gsr_refine_apply(int num_points, int n_split_samples, const uint8_t *flags,
                     const int32_t *offsets, const int32_t *counts,
                     const float *log_scales, const float *raw_quats,
                     const float *samples, unsigned long long seed,
                     int num_tensors, const gsr_refine_tensor *tensors,
                     gsr_stream_t stream);

/* ---- MCMC densification ---------------------------
 * "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024;
 * gsplat's MCMCStrategy): dead Gaussians (sigmoid(logit) <= min_opacity) are
 * relocated onto live ones sampled by opacity, the model grows to a cap, and a
 * source drawn `count` times gets, with ratio n = min(count + 1, 51),
 *   o' = 1 - (1 - o)^(1/n)
 *   D  = sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1)
 *   s' = (o / D) s
 * evaluated in float64 on the device and rounded once to float32.
 * gsr_mcmc_relocation is that rule on its own: opacities [n] in (0,1), scales
 * [n,3], ratios [n] (clamped to [1, 51]).  raw_outputs = 0: o' clamped to
 * [min_opacity, 1 - 2^-23] and s' (ratio 1: the inputs unchanged);
 * raw_outputs != 0: logit of the clamped o' and log(s) + log(o / D).
 * gsr_mcmc_plan, one phase (GSR_MCMC_RELOCATE or GSR_MCMC_ADD) of a refinement:
 *   opac[n]        sigmoid(logit), float32
 *   weight         (uint32) floor(opac * 2^24); relocate: 0 for dead rows
 *   prefix[n]      inclusive uint64 prefix sum of the weights
 *   dead_index[n]  the dead rows in ascending order (the first totals[1] entries)
 *   totals[2]      {sum of the weights, number of dead rows}
 *   draws          relocate: one per dead row; add: num_draws.  Draw j takes the
 *                  Philox4x32-10 block of counter (j, phase, step, 0) and key
 *                  seed; r = c0 * 2^32 + c1; target = (r * total) >> 64; source =
 *                  the first index whose prefix is > target; draw_source[j] =
 *                  source; counts[source] += 1; relocate: row_source[dead_index[j]]
 *                  = source.  row_source[n] is -1 and counts[n] 0 elsewhere.
 *                  total == 0: relocation draws nothing (draw_source -1); a new
 *                  row copies row j mod n, which stays as it is.
 * gsr_mcmc_apply moves up to GSR_REFINE_MAX_TENSORS tensors in one launch (all
 * tensors of a refinement in ONE call): rows < n_in with counts > 0 take their new
 * opacity logit (kind GSR_MCMC_OPACITIES, width 1) and log-scales
 * (GSR_REFINE_LOG_SCALES), rows with row_source >= 0 and rows n_in + j (source
 * draw_source[j]) become copies of their source after that update, and
 * GSR_REFINE_MOMENT tensors are zeroed on all of those rows.  in == out: in place
 * (n_out == n_in); otherwise every other row is copied.  scratch: 4 n_in floats.
 * gsr_mcmc_noise: mean += Sigma (eps * gate * scaler) in place, Sigma = R diag(
 * exp(log_scale)^2) R^T, gate = 1 / (1 + exp(-100 ((1 - sigmoid(logit)) - 0.995))),
 * eps = noise[n,3] or, if NULL, the three normals of the Philox block of counter
 * (i, step, 0, 0) (the construction of gsr_refine_apply's split samples).
 * gsr_mcmc_reg_forward: out[3] (float64) = {opacity_reg * mean(sigmoid(logit)) +
 * scale_reg * mean(exp(log_scale)), the two means}; float64 terms, fixed summation
 * order, no atomics.  _backward: the gradients scaled by the cotangent v_out[0]
 * (a device pointer). */
#define GSR_MCMC_MAX_RATIO 51
#define GSR_MCMC_RELOCATE 0
#define GSR_MCMC_ADD 1
#define GSR_MCMC_OPACITIES 4
int gsr_mcmc_relocation(int n, const float *opacities, const float *scales,
                        const int32_t *ratios, float min_opacity,
                        int raw_outputs, float *new_opacities,
                        float *new_scales, gsr_stream_t stream);
size_t gsr_mcmc_workspace_bytes(int num_points);
int gsr_mcmc_plan(int num_points, int num_draws, int phase,
                  const float *opacity_logits, float min_opacity,
                  unsigned int step, unsigned long long seed, float *opac,
                  uint64_t *prefix, int32_t *dead_index, int32_t *draw_source,
                  int32_t *row_source, int32_t *counts, uint64_t *totals,
                  void *workspace, size_t workspace_bytes,
                  gsr_stream_t stream);
int gsr_mcmc_apply(int n_in, int n_out, const float *opac,
                   const float *log_scales, float min_opacity,
                   const int32_t *row_source, const int32_t *draw_source,
                   const int32_t *counts, float *scratch, int num_tensors,
                   const gsr_refine_tensor *tensors, gsr_stream_t stream);
int gsr_mcmc_noise(int num_points, float *means, const float *log_scales,
                   const float *raw_quats, const float *opacity_logits,
                   float scaler, unsigned int step, unsigned long long seed,
                   const float *noise, gsr_stream_t stream);
size_t gsr_mcmc_reg_workspace_bytes(void);
int gsr_mcmc_reg_forward(int num_points, const float *opacity_logits,
                         const float *log_scales, double opacity_reg,
                         double scale_reg, double *out, void *workspace,
                         size_t workspace_bytes, gsr_stream_t stream);
int gsr_mcmc_reg_backward(int num_points, const float *opacity_logits,
                          const float *log_scales, double opacity_reg,
                          double scale_reg, const double *v_out,
                          float *v_logits, float *v_log_scales,
                          gsr_stream_t stream);

/* ---- optimiser step ------------------------------------
 * Adam over up to GSR_ADAM_MAX_TENSORS tensors in one launch; replaces the
 * per-group torch.optim.Adam objects the toolkit builds
 * (gs_toolkit/engine/optimizers.py:59-196, learning rates and eps = 1e-15 of
 * configs/method_configs.py:47-80).  Rule of torch.optim.Adam with
 * amsgrad = False, weight_decay = 0:  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 * p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps).
 * `tensors` is a HOST array; its pointers are device pointers (fp32, n elements
 * each, updated in place: param, exp_avg, exp_avg_sq).  `step` counts from 1.
 * The betas are doubles because torch forms 1 - beta in double before rounding
 * to fp32 (1.f - 0.999f is 1.3e-5 off). */
#define GSR_ADAM_MAX_TENSORS 8
typedef struct {
  float *param;
  const float *grad;
  float *exp_avg;
  float *exp_avg_sq;
  long long n;
  float lr;
} gsr_adam_tensor;
int gsr_adam_step(int num_tensors, const gsr_adam_tensor *tensors,
                  double beta1, double beta2, double eps, long long step,
                  gsr_stream_t stream);

/* ---- deterministic compositing backward ------------------------------------------
 * gsr_rasterize_backward(_rgbd) sum the per-tile contributions to a Gaussian's gradient
 * with float atomics: the result depends on the order in which the tiles' waves retire
 * (differences of a few ulp from run to run).  This variant (16x16 tiles) writes each
 * (tile, list entry) contribution to its own row of a workspace and then sums the rows of
 * every Gaussian in a fixed order, so two runs on the same inputs give bit-identical
 * gradients ("deterministic backward").  It needs what the binning knew:
 * order / cum_sorted of gsr_depth_order (num_bands = gsr_tile_bands) and slot_of_entry of
 * gsr_bin_sorted(_dev); list_capacity = the length gaussian_ids_sorted / slot_of_entry were
 * sized for.  extra / v_output_extra / v_extra NULL: three channels; otherwise the RGB +
 * extra-channel pass of gsr_rasterize_backward_rgbd.  Every output element is written.
 * About 1.4x the time of the atomic version and 48 B of workspace per list entry. */
size_t gsr_rasterize_backward_det_workspace_bytes(int list_capacity);
int gsr_rasterize_backward_det(
    unsigned img_height, unsigned img_width, int num_points, int list_capacity,
    const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
    const float *xys, const float *conics, const float *colors,
    const float *extra, const float *opacities, const float *background,
    float extra_background, const float *final_Ts, const int32_t *final_idx,
    const float *v_output, const float *v_output_extra,
    const float *v_output_alpha, const int32_t *order,
    const int32_t *cum_sorted, int num_bands, const int32_t *slot_of_entry,
    void *workspace, size_t workspace_bytes, float *v_xy, float *v_conic,
    float *v_colors, float *v_extra, float *v_opacity, gsr_stream_t stream);

/* ---- TSDF fusion: point cloud and mesh from rendered depth ------
 * A bounded, block-sparse truncated-signed-distance volume.  Geometry: `origin[3]`, voxel
 * length, `sdf_trunc`, blocks (Bx, By, Bz) of 8x8x8 voxels, a pool of `capacity` blocks.
 * All buffers are the caller's (nothing is allocated here):
 *   table  int32 [Bz,By,Bx]      pool slot of a block, -1 = not allocated
 *   tsdf   float [capacity,512]  voxel (lx,ly,lz) of a block at (lz*8 + ly)*8 + lx
 *   weight float [capacity,512]
 *   color  float [capacity,512,3]
 *   flags  uint8 [Bz*By*Bx]      blocks touched by the view in flight; zero between views
 *   list   int32 [Bz*By*Bx]      this view's touched, allocated blocks, ascending; bit 30
 *                                set: the slot was handed out by this view (pool rows unset)
 *   state  int32 [8]             0 allocated blocks, 1 length of `list`, 2 overflow flag,
 *                                3 largest would-be block count, 4 scratch, 5 points of the
 *                                last count, 6 vertices, 7 triangles of the last count
 * Voxel (ix,iy,iz) has its centre at origin[a] + ((float)i_a + 0.5f) * voxel_length.  The
 * camera: world->camera `viewmat` and its inverse `cam2world` (row-major, 12 floats each,
 * passed by value in the kernel arguments), pixel (i,j) looks along ((j + 0.5 - cx) / fx,
 * (i + 0.5 - cy) / fy, 1).  A pixel is usable when 0 < depth <= depth_trunc and `valid`
 * (uint8 [H,W] or NULL) is non-zero.  Per view: touch, allocate, integrate, in this order on
 * one stream; nothing is read back. */
typedef struct gsr_tsdf_volume {
  float origin[3];
  float voxel_length;
  float sdf_trunc;
  int blocks[3]; /* Bx, By, Bz */
  int capacity;
  int32_t *table;
  float *tsdf;
  float *weight;
  float *color;
  int32_t *state;
} gsr_tsdf_volume;

typedef struct gsr_tsdf_view {
  unsigned height, width;
  float fx, fy, cx, cy;
  float depth_trunc;
  float viewmat[12];   /* rows 0..2 of world->camera */
  float cam2world[12]; /* rows 0..2 of its inverse */
  const float *depth;  /* [H,W] z-depth */
  const float *color;  /* [H,W,3] */
  const uint8_t *valid; /* [H,W] or NULL */
} gsr_tsdf_view;

/* flags every block within sdf_trunc (per axis) of a usable pixel's world point */
int gsr_tsdf_touch(const gsr_tsdf_volume *vol, const gsr_tsdf_view *view,
                   uint8_t *flags, gsr_stream_t stream);
/* hands pool slots to the flagged blocks without one in ascending block index (a scan, so
 * the numbering is reproducible), writes `list` and state[0..3], and clears `flags`.
 * Blocks beyond `capacity` stay -1, set state[2] and are left out of `list`. */
size_t gsr_tsdf_allocate_workspace_bytes(int num_blocks);
int gsr_tsdf_allocate(const gsr_tsdf_volume *vol, uint8_t *flags, int32_t *list,
                      void *workspace, size_t workspace_bytes, gsr_stream_t stream);
/* running weighted mean of the truncated signed distance and the colour over every voxel
 * of the blocks in `list` (their number is read on the device from state[1]) */
int gsr_tsdf_integrate(const gsr_tsdf_volume *vol, const gsr_tsdf_view *view,
                       const int32_t *list, gsr_stream_t stream);
/* Point cloud: one point per sign change between a voxel and its +x / +y / +z neighbour,
 * both observed and |tsdf| < 0.98; rows ordered by (block, voxel, axis).  _count leaves the
 * number of points in state[5] and per-block offsets in the workspace; _emit (same
 * workspace, untouched in between) writes `num_points` rows (what the caller read back). */
size_t gsr_tsdf_extract_points_workspace_bytes(int num_blocks);
int gsr_tsdf_extract_points_count(const gsr_tsdf_volume *vol, void *workspace,
                                  size_t workspace_bytes, gsr_stream_t stream);
int gsr_tsdf_extract_points_emit(const gsr_tsdf_volume *vol, const void *workspace,
                                 size_t workspace_bytes, int num_points, float *points,
                                 float *colors, float *normals, int32_t *axis,
                                 gsr_stream_t stream);
/* Surface-nets mesh: one vertex per cell whose eight corners are observed with
 * |tsdf| < 0.98 and mixed signs, one quad (two triangles, normals towards positive tsdf)
 * per sign-changing grid edge whose four cells are active.  _count leaves the numbers of
 * vertices and triangles in state[6], state[7]. */
size_t gsr_tsdf_extract_mesh_workspace_bytes(int num_blocks, int capacity);
int gsr_tsdf_extract_mesh_count(const gsr_tsdf_volume *vol, void *workspace,
                                size_t workspace_bytes, gsr_stream_t stream);
int gsr_tsdf_extract_mesh_emit(const gsr_tsdf_volume *vol, void *workspace,
                               size_t workspace_bytes, int num_vertices, int num_triangles,
                               float *vertices, float *vertex_colors, int32_t *triangles,
                               gsr_stream_t stream);

/* ---- mesh cleaning: what `ExportTSDF(clean=True)` does to mesh.ply -----
 * Input: vertices float [V,3], optional per-vertex attributes float [V,C], triangles int32
 * [F,3], min_component_faces >= 0.  The rules, applied in this order:
 *  1. Index check.  An index outside [0, V) is an error (GSR_ERANGE), found by a kernel
 *     that reads `triangles` only; its verdict is read back before any kernel that
 *     dereferences with an index is launched, and none is.
 *  2. Null faces are removed: two equal indices, or (v1 - v0) x (v2 - v0) with all three
 *     components exactly 0 in float32, every operation rounded on its own (a NaN coordinate
 *     makes the product non-zero: not null; coinciding vertices under different indices:
 *     null).  With vertices == NULL only the repeated-index part applies.
 *  3. Duplicate faces are removed: faces with the same SET of three indices, whatever the
 *     order or winding; of each set the lowest face index stays.
 *  4. Components.  Two surviving faces are adjacent when they share an edge (the same
 *     unordered pair of indices; three or more faces on one edge are all adjacent; faces
 *     that meet in a vertex only are not).  A component is the transitive closure; it is
 *     removed when it has < min_component_faces surviving faces (exactly min: kept).
 *  5. Compaction.  Surviving faces keep their relative order; vertices no surviving face
 *     references are dropped, the others keep their relative order and their rows are
 *     copied bit for bit; indices are remapped.
 * Every output is a pure function of the input: label[f] = the lowest face index of f's
 * component (-1 for a null or duplicate face), size[f] = that component's number of faces
 * (0 for a null or duplicate face), whatever `min_component_faces`.
 *   state  int32 [8]  0 scratch of the index check, 1 null faces, 2 duplicate faces,
 *                     3 components, 4 components kept, 5 faces kept, 6 vertices kept,
 *                     7 non-zero: two faces on one edge ended with different labels (an
 *                     internal error; the result must not be used)
 * gsr_mesh_label leaves the counts in `state` and the keep flags and offsets in the workspace
 * (labels / sizes [F] are copied out when not NULL); it synchronises `stream` once, for the
 * index check.  gsr_mesh_emit (same workspace, untouched in between; counts = state[6],
 * state[5] as the caller read them back) writes the compacted mesh.  The workspace query
 * returns 0 when num_faces <= 0, when the sizes do not fit (F <= 2^28) or when a size query of
 * rocPRIM fails (no device); F = 0 needs none. */
size_t gsr_mesh_clean_workspace_bytes(int num_vertices, int num_faces);
int gsr_mesh_label(int num_vertices, int num_faces, const float *vertices,
                   const int32_t *triangles, int min_component_faces, int32_t *state,
                   void *workspace, size_t workspace_bytes, int32_t *labels,
                   int32_t *sizes, gsr_stream_t stream);
int gsr_mesh_emit(int num_vertices, int num_faces, int num_attributes,
                  const float *vertices, const float *attributes,
                  const int32_t *triangles, const void *workspace,
                  size_t workspace_bytes, int out_vertices, int out_faces,
                  float *vertices_out, float *attributes_out, int32_t *triangles_out,
                  gsr_stream_t stream);

/* ---- surface distance: points against a triangle mesh -----------------
 * What gs_toolkit/evaluation/surface_distance computes for every vertex of a generated mesh.
 * Mesh: vertices float [V,3], triangles int32 [F,3] (a soup is allowed: no welding, no
 * watertightness, no normals).  Points float [n,3].  The rule:
 *  1. d(p) = min over the usable triangles f of |p - q_f(p)|, q_f(p) the closest point of
 *     triangle f to p by the Voronoi-region rule (Ericson / Eberly: three vertex regions, three
 *     edge regions, the face).  Outputs: d float [n], the index f of a minimising triangle
 *     int32 [n] (ties: any minimiser), optionally q float [n,3].  Unsigned: there is no sign.
 *  2. Degenerate triangles.  A triangle with |n|^2 <= 2^-40 |ab|^2 |ac|^2 (n = ab x ac; exactly
 *     zero area included) counts as its three edges as segments; so does one on which the
 *     rounded region tests contradict one another.  A zero-length segment counts as a point.
 *     Every quotient is guarded: finite input never gives NaN.
 *  3. Non-finite input.  A triangle with a non-finite vertex (or centroid) is left out of the
 *     tree and counted in state[1].  A non-finite point gets d = NaN, f = -1, q = NaN and is
 *     counted as invalid by the statistics, which leave it out.
 *  4. Index check.  An index outside [0, V) is GSR_ERANGE, as in gsr_mesh_label: a face that
 *     fails the check is not read through, and the verdict is read back before any later
 *     kernel runs.  A mesh with no usable triangle builds a tree on which every query answers
 *     NaN / -1 (state[1] == F tells the caller).
 *  5. Arithmetic: float32.  The triangle is translated first (a - p, b - p, c - p), q is the
 *     clamped closest point of the translated triangle and d = |q|, every operation rounded on
 *     its own (no contraction), dot(x, y) = (x0 y0 + x1 y1) + x2 y2; `closest` = p + q.
 *     tests/surface_distance_reference.py restates the sequence in NumPy.
 * Nothing is allocated here.  gsr_mesh_distance_workspace_bytes(what, F, n): bytes of the tree
 * (what = 0; kept as long as the mesh is queried), of the build's workspace (1), of a tree
 * query's workspace for n points (2; the exhaustive query needs none), of the statistics'
 * workspace (3); 0 when the sizes do not fit (F in [1, 2^28], n in [1, 2^30]) or a size query
 * of rocPRIM fails (no device).  All buffers 256-byte aligned; none needs to be zeroed.
 *   state  int32 [4]   0 scratch of the index check, 1 triangles left out, 2-3 unused
 * gsr_mesh_bvh_build synchronises `stream` once (the index check).  gsr_mesh_distance_query
 * with GSR_MESH_DISTANCE_EXHAUSTIVE tests every point against every usable triangle instead of
 * walking the tree (the on-device cross-check, never chosen by the library itself); both paths
 * evaluate a triangle with the same device function.
 * gsr_mesh_distance_stats over float32 distances, accumulated in float64 in a fixed order
 * (bit-reproducible):  stats double [8]  0 finite distances, 1 non-finite ones, 2 mean, 3 root
 * mean square, 4 max, 5 distances <= threshold (a negative threshold counts none), 6 sum,
 * 7 sum of squares; mean, rms and max are 0 when nothing is finite. */
#define GSR_MESH_DISTANCE_EXHAUSTIVE 1
#define GSR_MESH_DISTANCE_BYTES_TREE 0
#define GSR_MESH_DISTANCE_BYTES_BUILD 1
#define GSR_MESH_DISTANCE_BYTES_QUERY 2
#define GSR_MESH_DISTANCE_BYTES_STATS 3
size_t gsr_mesh_distance_workspace_bytes(int what, int num_faces, int num_points);
int gsr_mesh_bvh_build(int num_vertices, int num_faces, const float *vertices,
                       const int32_t *triangles, void *tree, size_t tree_bytes,
                       void *workspace, size_t workspace_bytes, int32_t *state,
                       gsr_stream_t stream);
int gsr_mesh_distance_query(int num_faces, const void *tree, size_t tree_bytes,
                            int num_points, const float *points, int flags, void *workspace,
                            size_t workspace_bytes, float *distance, int32_t *face,
                            float *closest, gsr_stream_t stream);
int gsr_mesh_distance_stats(int num_points, const float *distance, float threshold,
                            void *workspace, size_t workspace_bytes, double *stats,
                            gsr_stream_t stream);

/* ---- Canny edge mask: what `image2canny` hands the co-gs model ---------
 * OpenCV's cv::Canny(img8, thres1, thres2) with its defaults (aperture 3, L2gradient = false),
 * restated; this text is the specification.  All arithmetic is integer: results are exact.
 * Input: image float [H,W,3] (values expected in [0,1]).  Output: edges uint8 [H,W], 255 / 0.
 *  1. uint8.  Every channel is u8 = (uint8)trunc(x * 255.0f), the product formed in float32 (what
 *     NumPy does for `(image * 255.0).astype(np.uint8)`).  Stated difference: a product outside
 *     [0, 255] saturates and NaN gives 0 (NumPy's cast is platform-dependent there).
 *  2. Sobel.  3x3, unscaled, replicate border, per channel: dx = right column - left column, dy =
 *     row below - row above, weights 1 2 1.  norm = |dx| + |dy|; the pixel takes (mag, dx, dy)
 *     from the channel with the largest norm, the lowest channel index on ties.  mag outside
 *     the image is 0 (the zero padding applies to the magnitude only, not to the image).
 *  3. Non-maximum suppression.  low = floor(thres1), high = floor(thres2), swapped if low > high.
 *     A pixel with mag <= low is no candidate.  Otherwise, with x = |dx|, y = |dy| << 15,
 *     t22 = x * 13573, t67 = t22 + (x << 16):
 *       y < t22:  candidate iff mag > mag[left] && mag >= mag[right];
 *       y > t67:  candidate iff mag > mag[above] && mag >= mag[below];
 *       else, s = ((dx ^ dy) < 0) ? -1 : 1:
 *                 candidate iff mag > mag[row-1][col-s] && mag > mag[row+1][col+s].
 *     A candidate with mag > high is strong, any other candidate weak.
 *  4. Hysteresis.  A candidate is an edge iff its 8-connected component of candidates holds a
 *     strong pixel.
 * H or W of 1 is legal; H * W = 0 launches nothing; H * W < 2^31, H <= 16 * 65535.
 * Nothing is allocated here: gsr_canny_workspace_bytes(H, W) bytes of scratch (6 per pixel: an
 * int32 parent, a map byte, a flag byte; 256-byte aligned, no part needs to be zeroed; 0 when the
 * sizes do not fit).  Nothing is read back, no host loop depends on the data, and the output
 * is a pure function of the input (the root of a component is its smallest pixel index whatever
 * the order of the atomics). */
size_t gsr_canny_workspace_bytes(int img_height, int img_width);
int gsr_canny(int img_height, int img_width, const float *image, float thres1, float thres2,
              void *workspace, size_t workspace_bytes, uint8_t *edges, gsr_stream_t stream);

/* ---- depth regularisation of the co-gs model (depth_gs.py:521-528) ------
 * pred, mask float [H,W] (mask: any values; the model passes the non-edge mask).
 *   m    = mask * [pred > 0]
 *   num  = plus-shaped five-tap sum (centre, up, down, left, right; zero padding) of pred * m
 *   cnt  = the same sum of m;   near = num / (cnt + 1e-8)
 *   loss = mean over all H W pixels of (near - pred [pred > 0])^2
 * differentiable w.r.t. pred only (mask and [pred > 0] are constants, as in the source):
 *   g = 2 (near - pred [pred > 0]) / (H W)
 *   v_pred[q] = upstream * ( m[q] * sum_{p in plus(q)} g[p] / (cnt[p] + 1e-8) - g[q] [pred[q] > 0] )
 * NaN propagates as in the source.  The forward sums float64 partials per workgroup in a fixed
 * order and adds them in one workgroup: the scalar is bit-reproducible.
 *   scratch  float [2,H,W] (may be NULL for a forward without a backward): the pixel's own share
 *            g (m / (cnt + 1e-8) - [pred > 0]) and what its neighbours gather, g / (cnt + 1e-8)
 *   partial  double [GSR_DEPTH_REG_WORKSPACE_DOUBLES]; needs no zeroing
 * H * W in [1, 2^31). */
#define GSR_DEPTH_REG_WORKSPACE_DOUBLES 1024
int gsr_depth_reg_forward(unsigned img_height, unsigned img_width, const float *pred,
                          const float *mask, float *scratch, double *partial, float *loss_out,
                          gsr_stream_t stream);
int gsr_depth_reg_backward(unsigned img_height, unsigned img_width, const float *upstream,
                           const float *pred, const float *mask, const float *scratch,
                           float *v_pred, gsr_stream_t stream);

/* ---- monocular-depth terms of the co-gs model (depth_gs.py:477-531) ----
 * pred, gt float [H,W]; mask float [H,W] or NULL.  With a mask every term is that of the float32
 * products s = pred * mask and t = gt * mask (the model multiplies the per-view mask in before
 * this branch, depth_gs.py:424-437; nothing is selected, the means stay over all pixels) and
 * v_pred is scaled by the mask; without one s = pred, t = gt.  Everything else is float64 in
 * registers; the scalars are float64 sums in a fixed order without atomics (bit-reproducible);
 * the loss and v_pred are rounded to float32.  Differentiable w.r.t. pred only.  Every backward
 * writes every element of v_pred (no zeroing needed) and reads `upstream` (float [1]) on the
 * device.  NaN and inf propagate as in the source.  H * W in [1, 2^31).
 *
 * Local Pearson (utils/losses.py:26-45).  Patch p has its top-left corner at (rows[p], cols[p])
 * -- int64 [n_corr] when index64 != 0, else int32 [n_corr], read on the device -- and n = box_p^2
 * pixels.  With the means m_s, m_t and the centred sums S_ss, S_tt, S_st over the patch (two
 * passes: means first):
 *   loss_p = 1 - (n - 1) / n * S_st / sqrt(S_ss S_tt)     (biased covariance over unbiased
 *                                                           deviations, as the source writes it)
 *   loss   = (sum_p loss_p) / n_corr
 *   v_pred[q] = upstream * mask[q] * (1 / n_corr) * sum over the patches p that cover q, in
 *               ascending p, of A_p (B_p (s[q] - m_s) - (t[q] - m_t)),
 *               A_p = (n - 1) / (n sqrt(S_ss S_tt)),  B_p = S_st / S_ss;   0 where none covers q
 * A patch with S_ss = 0 or S_tt = 0, or box_p = 1, is 0 / 0: the loss is NaN and v_pred is NaN on
 * that patch's pixels only.  A corner outside [0, H - box_p] x [0, W - box_p] is never
 * dereferenced: its loss_p is NaN and it adds nothing to v_pred.  n_corr = 0: the loss and v_pred
 * are NaN (0 / 0, as the source).  box_p in [1, min(H, W)], else GSR_EINVAL.
 *   stats  double [n_corr, 5]: m_s, m_t, A, B, loss_p per patch, written by the forward, read by
 *          the backward; needs no zeroing
 *
 * Scaled log-depth (depth_gs.py:492-519).  image float [H,W,3], scale_shift float [2] on the
 * device.  With e = scale * s + shift - t, l = log(1 + |e|),
 * lx[y,x] = exp(-mean_c |image[y,x,c] - image[y,x+1,c]|), ly the same towards row y + 1:
 *   loss = sum_{x < W-1} lx l / (H (W - 1)) + sum_{y < H-1} ly l / ((H - 1) W)
 *   v_pred = upstream * mask * scale * sign(e) / (1 + |e|)
 *            * (lx / (H (W - 1)) [x < W-1] + ly / ((H - 1) W) [y < H-1]),        sign(0) = 0
 * H = 1 or W = 1: the loss is NaN (the mean of an empty tensor).
 *
 * Total variation (utils/losses.py:197-207):
 *   loss = sum_{x < W-1} |s[y,x] - s[y,x+1]| / (H (W - 1)) + sum_{y < H-1} |s[y,x] - s[y+1,x]| / ((H - 1) W)
 *   v_pred = upstream * mask * the four-neighbour gather of the signs of those differences over
 *            the same counts, sign(0) = 0.  H = 1 or W = 1: the loss is NaN.
 *   partial  double [GSR_MONO_DEPTH_WORKSPACE_DOUBLES] (log-depth and TV); needs no zeroing */
#define GSR_MONO_DEPTH_WORKSPACE_DOUBLES 2048
int gsr_local_pearson_forward(unsigned img_height, unsigned img_width, int box_p, int n_corr,
                              const float *pred, const float *gt, const float *mask,
                              const void *rows, const void *cols, int index64, double *stats,
                              float *loss_out, gsr_stream_t stream);
int gsr_local_pearson_backward(unsigned img_height, unsigned img_width, int box_p, int n_corr,
                               const float *upstream, const float *pred, const float *gt,
                               const float *mask, const void *rows, const void *cols, int index64,
                               const double *stats, float *v_pred, gsr_stream_t stream);
int gsr_log_depth_forward(unsigned img_height, unsigned img_width, const float *pred,
                          const float *gt, const float *image, const float *scale_shift,
                          const float *mask, double *partial, float *loss_out,
                          gsr_stream_t stream);
int gsr_log_depth_backward(unsigned img_height, unsigned img_width, const float *upstream,
                           const float *pred, const float *gt, const float *image,
                           const float *scale_shift, const float *mask, float *v_pred,
                           gsr_stream_t stream);
int gsr_tv_forward(unsigned img_height, unsigned img_width, const float *pred, const float *mask,
                   double *partial, float *loss_out, gsr_stream_t stream);
int gsr_tv_backward(unsigned img_height, unsigned img_width, const float *upstream,
                    const float *pred, const float *mask, float *v_pred, gsr_stream_t stream);

/* ---- per-view bilateral grids (csrc/bilagrid.hip) ----------------------
 * Appearance compensation between the render and the loss heads: every training view owns a
 * small 3-D grid of 3x4 affine colour maps, and a rendered pixel is mapped by the grid's value
 * at (its position, its brightness) -- what gsplat's `lib_bilagrid.slice` does, i.e.
 * F.grid_sample(grid[v:v+1], 2 (xyz - 0.5), "bilinear", align_corners=True,
 * padding_mode="border") followed by the affine map.
 *   grids  float [V][L][Gh][Gw][12], channel last (a vertex is three 16-byte loads), 16-byte
 *          aligned; the 12 channels are a row-major 3x4 map; Gw, Gh in [2, GSR_BILAGRID_MAX_XY],
 *          L in [2, GSR_BILAGRID_MAX_L]; view in [0, V)
 *   rgb    float [H][W][3];  out, v_out, v_rgb the same shape;  3 H W < 2^31
 * The rule, for pixel (px, py) with colour (r, g, b):
 *   x = (px + 0.5) / W          y = (py + 0.5) / H
 *   guide = 0.299 r + 0.587 g + 0.114 b
 *   ix = x (Gw - 1)   iy = y (Gh - 1)   iz = clamp(guide, 0, 1) (L - 1)
 *   M  = trilinear interpolation of grids[view] at (iz, iy, ix)      (12 values, 8 corners)
 *   out[k] = M[4k] r + M[4k+1] g + M[4k+2] b + M[4k+3]               k = 0, 1, 2
 * Backward, from v_out:
 *   v_grids[view][corner][4k+j] = sum over the pixels of weight(pixel, corner) v_out[k] (r, g, b, 1)[j]
 *   v_grids[other views]        = exact zeros; so are vertices that no pixel reaches (an image
 *                                 smaller than the grid).  Every element of v_grids is written.
 *   v_rgb[c] = sum_k M[4k+c] v_out[k]
 *              + [0 < guide < 1] (L - 1) (0.299, 0.587, 0.114)[c] sum_k v_out[k] (dM/diz)[4k..4k+3] . (r, g, b, 1)
 *   (the path through the guide is zero where the guide is clamped: grid_sample's border rule).
 * Per-pixel arithmetic is float32; every sum over pixels is float64 in a fixed order, without
 * atomics: two runs are bit-equal.  NaN and inf in rgb propagate into out; a NaN guide reads
 * level 0.
 *   workspace  double [GSR_BILAGRID_WORKSPACE_DOUBLES(Gw, Gh, L)] (backward); needs no zeroing
 * Total variation over all views:
 *   tv = sum over the axes L, Gh, Gw of mean((A[.. i+1 ..] - A[.. i ..])^2), each mean over all
 *        difference elements of that axis across views and channels
 *   v_grids = upstream * d tv / d A (every element written), float64 arithmetic
 *   partial  double [GSR_BILAGRID_TV_WORKSPACE_DOUBLES]; needs no zeroing
 * The identity map is (1,0,0,0, 0,1,0,0, 0,0,1,0) at every vertex. */
#define GSR_BILAGRID_CHANNELS 12
#define GSR_BILAGRID_MAX_XY 64
#define GSR_BILAGRID_MAX_L 16
/* row strips a vertex's pixel rectangle is cut into (one workgroup each) */
#define GSR_BILAGRID_STRIPS(gw, gh) \
  ((gw) * (gh) >= 2048 ? 1 : ((gw) * (gh) <= 32 ? 64 : 2048 / ((gw) * (gh))))
#define GSR_BILAGRID_WORKSPACE_DOUBLES(gw, gh, gl) \
  ((size_t)GSR_BILAGRID_STRIPS(gw, gh) * (size_t)(gw) * (size_t)(gh) * (size_t)(gl) * GSR_BILAGRID_CHANNELS)
#define GSR_BILAGRID_TV_WORKSPACE_DOUBLES 3072
int gsr_bilagrid_slice_forward(unsigned img_height, unsigned img_width, int num_views, int view,
                               int grid_w, int grid_h, int grid_l, const float *grids,
                               const float *rgb, float *out, gsr_stream_t stream);
int gsr_bilagrid_slice_backward(unsigned img_height, unsigned img_width, int num_views, int view,
                                int grid_w, int grid_h, int grid_l, const float *grids,
                                const float *rgb, const float *v_out, double *workspace,
                                float *v_rgb, float *v_grids, gsr_stream_t stream);
int gsr_bilagrid_tv_forward(int num_views, int grid_w, int grid_h, int grid_l, const float *grids,
                            double *partial, float *loss_out, gsr_stream_t stream);
int gsr_bilagrid_tv_backward(int num_views, int grid_w, int grid_h, int grid_l,
                             const float *upstream, const float *grids, float *v_grids,
                             gsr_stream_t stream);

/* ---- normal maps and the depth-normal consistency loss (csrc/normals.hip) ------
 * What surface-oriented training (2DGS, GOF, RaDe-GS, PGSR, gsplat's `normal_lambda`) adds: a
 * normal per Gaussian, composited into a normal image; a second normal image derived from the
 * rendered depth; their disagreement as a loss.  Camera space is the projection's: x right,
 * y down, z forward.  The centre of pixel (row i, column j) is (j + 0.5, i + 0.5).
 *
 * Per-Gaussian normals.  quats float [N,4] as (w,x,y,z), raw (normalised inside), 16-byte
 * aligned; scales float [N,3], of which only the order is used (log-scales and their exp give
 * the same result); means float [N,3]; viewmat float [12], row-major 3x4, on the device.
 *   axis    = the index of the smallest scale; on a tie the lowest index wins
 *   n_cam   = viewmat[:, :3] . (column `axis` of R(q / |q|))
 *   p_cam   = viewmat[:, :3] . mean + viewmat[:, 3]
 *   sign    = -1 where n_cam . p_cam > 0, else +1        (the normal faces the camera)
 *   normals = sign n_cam            float [N,3];   axis int [N];   sign float [N] (+-1)
 * Backward, from v_normals: v_quats float [N,4] through the rotation column and the
 * normalisation, (v - qn (qn . v)) / |q|.  axis and sign are piecewise constant: scales, means
 * and viewmat get no gradient.  N = 0 launches nothing; 4 N < 2^31.
 *
 * Depth normals.  depth, alpha float [H,W]; fx, fy, cx, cy the intrinsics (doubles).
 *   P(i,j) = ((j + 0.5 - cx) / fx * D, (i + 0.5 - cy) / fy * D, D),  D = depth[i][j]
 *   u = P(i+1,j) - P(i-1,j)    v = P(i,j+1) - P(i,j-1)    n_d = (u x v) / |u x v|
 * which is (0,0,-1) for a fronto-parallel plane: it faces the camera like the normals above.  A
 * pixel is invalid, and its n_d an exact zero, if it is on the image's one-pixel border, or it
 * or one of its four neighbours has alpha <= 0 or a depth that is not finite (the test is on
 * alpha: the models fill alpha == 0 pixels with depth.max()), or |u x v|^2 is zero or not finite.
 *   normals  float [H,W,3]; every element written
 *
 * Consistency loss.  normals_img float [H,W,3]: the alpha-blended, un-normalised rendered
 * normals; mask float [H,W] or NULL.
 *   loss = (1 / (H W)) sum over ALL pixels p of m(p) (1 - alpha(p) <normals_img(p), n_d(p)>)
 * (2DGS / gsplat: 1 - (normals * normals_from_depth * alpha.detach()).sum(-1), as a mean; the
 * mask is multiplied in and the mean stays over all pixels; an invalid pixel adds m(p)).
 * Backward, with s = -upstream / (H W):
 *   v_normals_img(p) = s m(p) alpha(p) n_d(p)
 *   v_depth(q)       = the sum over q's four neighbours p of the term of n_d(p) that holds
 *                      depth(q): with g = s m alpha normals_img at p, c = u x v,
 *                      dc = (g - n_d (n_d . g)) / |c|, du = v x dc, dv = dc x u, r_q the ray of q:
 *                      <du(above q), r_q> - <du(below q), r_q> + <dv(left of q), r_q> - <dv(right of q), r_q>
 *                      -- a gather, no scatter; an exact zero where no neighbour is valid
 * alpha is a weight: no gradient.  `upstream` (float [1]) is read on the device.  Arithmetic is
 * float64 per pixel, rounded to float32 on the way out; the sum over pixels is float64 in a fixed
 * order (lane, wave, workgroup, then the tiles' partials in one workgroup), without atomics: two
 * runs are bit-equal.  Every element of every output is written.  3 H W < 2^31.
 *   partial  double [GSR_NORMAL_WORKSPACE_DOUBLES(H, W)]; needs no zeroing */
#define GSR_NORMAL_TILE 16
#define GSR_NORMAL_WORKSPACE_DOUBLES(h, w)                                   \
  ((size_t)(((h) + GSR_NORMAL_TILE - 1) / GSR_NORMAL_TILE) *                  \
   (size_t)(((w) + GSR_NORMAL_TILE - 1) / GSR_NORMAL_TILE))
int gsr_gaussian_normals_forward(int num_points, const float *quats, const float *scales,
                                 const float *means, const float *viewmat, float *normals,
                                 int *axis, float *sign, gsr_stream_t stream);
int gsr_gaussian_normals_backward(int num_points, const float *quats, const float *viewmat,
                                  const int *axis, const float *sign, const float *v_normals,
                                  float *v_quats, gsr_stream_t stream);
int gsr_depth_normals(unsigned img_height, unsigned img_width, double fx, double fy, double cx,
                      double cy, const float *depth, const float *alpha, float *normals,
                      gsr_stream_t stream);
int gsr_normal_consistency_forward(unsigned img_height, unsigned img_width, double fx, double fy,
                                   double cx, double cy, const float *normals_img,
                                   const float *depth, const float *alpha, const float *mask,
                                   double *partial, float *loss_out, gsr_stream_t stream);
int gsr_normal_consistency_backward(unsigned img_height, unsigned img_width, double fx, double fy,
                                    double cx, double cy, const float *upstream,
                                    const float *normals_img, const float *depth,
                                    const float *alpha, const float *mask, float *v_normals_img,
                                    float *v_depth, gsr_stream_t stream);

/* ---- depth distortion and median depth (csrc/distortion.hip) -----------
 * The Mip-NeRF-360 distortion term per pixel (2DGS, gsplat's `distloss`) and the depth at which
 * the transmittance crosses 0.5 (`render_mode="...+median"`), from one front-to-back walk of its
 * own over single-segment tile lists (ids int32 [I], bins int32 [tiles,2]; block width 16).
 * values float [N]: one scalar per Gaussian -- the depths, or a monotone map of them.
 *
 * The walk is the forward compositing's: pixel centre = the integer pixel coordinate,
 * sigma = (a dx^2 + c dy^2) / 2 + b dx dy, alpha = min(0.999, opac exp(-sigma)); an entry with
 * sigma < 0 or alpha < 1/255 is skipped; the walk stops BEFORE the entry that would make
 * T (1 - alpha) <= 1e-4.  For the contributing entries i = 1..n in list order, T_i the
 * transmittance before entry i, w_i = alpha_i T_i, A_i = 1 - T_{i+1}, B_i = sum_{j<=i} w_j z_j:
 *   out_distortion = 2 sum_i w_i (z_i A_{i-1} - B_{i-1})
 *                    (= sum_i sum_j w_i w_j |z_i - z_j| where z does not decrease along the list)
 *   out_median     = z_i of the last contributing entry with T_i > 0.5; 0 where none contributes
 *   out_vsum = B_n, final_Ts = T_{n+1}, final_idx = the list index of entry n, or -1
 * All five are float/int32 [H,W]; every element is written; a tile with an empty list gets
 * zeros, final_Ts = 1 and final_idx = -1.
 *
 * Backward, from v_distortion float [H,W] (the median carries no gradient): the gradient of what
 * the forward computes -- the same clamp 0.999.  Back to front from final_idx, T_k by division,
 * B_{k-1} = B_k - w_k z_k, S = sum_{i>k} w_i g_i:
 *   g_k        = 2 [z_k A_{k-1} - B_{k-1} + (B_n - B_k) - z_k (A_n - A_k)]
 *   dD/dz_k    = 2 w_k [A_{k-1} - (A_n - A_k)]
 *   dD/dalpha_k = T_k g_k - S / (1 - alpha_k), and 0 where opac exp(-sigma) > 0.999 (clamped)
 *   v_sigma = -opac vis dD/dalpha_k v_distortion, into v_xy / v_conic as in the compositing backward;
 *   v_opacity += vis dD/dalpha_k v_distortion;  v_values += dD/dz_k v_distortion
 * v_xy float [N,2], v_conic [N,3], v_opacity [N], v_values [N]: cleared by the entry, then summed
 * with float atomics (not bit-reproducible from run to run). */
int gsr_distortion_forward(int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                           const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                           const float *xys, const float *conics, const float *opacities,
                           const float *values, float *out_distortion, float *out_median,
                           float *out_vsum, float *final_Ts, int32_t *final_idx,
                           gsr_stream_t stream);
int gsr_distortion_backward(unsigned img_height, unsigned img_width, int num_points,
                            const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                            const float *xys, const float *conics, const float *opacities,
                            const float *values, const float *out_vsum, const float *final_Ts,
                            const int32_t *final_idx, const float *v_distortion, float *v_xy,
                            float *v_conic, float *v_opacity, float *v_values,
                            gsr_stream_t stream);

/* ---- contribution statistics (csrc/contribution.hip) -------------------
 * Per-Gaussian statistics of the blend weight over a view, what contribution-based pruning
 * (RadSplat, LightGaussian, Mini-Splatting) scores with: one forward walk of its own over
 * single-segment tile lists (ids int32 [I], bins int32 [tiles,2]; block width 16).
 *
 * The walk is the forward compositing's, as stated for gsr_distortion_forward above: pixel
 * centre = the integer pixel coordinate, sigma = (a dx^2 + c dy^2) / 2 + b dx dy,
 * alpha = min(0.999, opac exp(-sigma)); an entry with sigma < 0 or alpha < 1/255 is skipped;
 * the walk stops BEFORE the entry that would make T (1 - alpha) <= 1e-4.  T is float32, and for
 * every contributing (pixel, entry) pair w = alpha T is one float32 product.  With g the entry's
 * Gaussian, the call ADDS to four arrays [num_points] the caller owns (zeros before the first
 * view; V calls accumulate V views):
 *   max_w[g]    = max(max_w[g], w)     float32; an integer atomic max on the bits (w > 0)
 *   sum_q[g]   += (uint32)(w * 2^24)   int64; fixed point, truncated: independent of the order
 *   hits[g]    += 1                    int64
 *   dominant[g] += 1 per PIXEL whose largest w is g's entry; strictly greater replaces, so of
 *                  equal weights the front-most entry wins.  int64
 * No float atomics: every array is bit-reproducible from run to run.  A list entry whose id is
 * outside [0, num_points) is skipped.  Pixels outside the image contribute nothing. */
int gsr_contribution_accumulate(int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                                int num_points, const int32_t *gaussian_ids_sorted,
                                const int32_t *tile_bins, const float *xys, const float *conics,
                                const float *opacities, float *max_w, int64_t *sum_q,
                                int64_t *hits, int64_t *dominant, gsr_stream_t stream);

/* ---- k nearest neighbours: points against a point cloud ----------------
 * What the toolkit's models ask scikit-learn for when they turn seed points into initial scales
 * (`k_nearest_sklearn`, vanilla_gs.py:136-140, 260-280), as a general query.  Reference points P
 * float [n,3]; queries Q float [m,3], or Q = P with GSR_KNN_SELF ("self mode": pass P again,
 * m = n); k in [1, GSR_KNN_MAX_K].  Outputs: distance float [m,k] ascending, index int32 [m,k],
 * row numbers into P.  The rule:
 *  1. Arithmetic: float32, every operation rounded on its own (no contraction):
 *     dx = q.x - p.x (likewise dy, dz), d2 = (dx*dx + dy*dy) + dz*dz, distance = sqrtf(d2).
 *     tests/knn_reference.py restates the sequence in NumPy.
 *  2. Order.  The result of a query is the k smallest pairs (d2, row) in lexicographic order: a tie
 *     in d2 goes to the smaller row.  `index` is therefore a pure function of the input, and
 *     the tree walk and the exhaustive path agree bit for bit, indices included.
 *  3. Self mode.  Row i never returns i itself, by index.  The distances are those of the
 *     reference, which takes k + 1 neighbours and drops column 0 (with duplicate points the k
 *     smallest distances over j != i are the same numbers).  Stated difference for the indices:
 *     with duplicate points the reference may drop a twin and keep i; this rule always drops i.
 *  4. Non-finite input.  A reference point with a non-finite coordinate is left out of the tree
 *     and counted in state[1] of the build.  A non-finite query gets distance = NaN, index = -1
 *     in every column and is counted in state[2] of the query.
 *  5. Too few points.  gsr_knn_query returns GSR_ERANGE, before any kernel is launched, when
 *     num_usable < k (k + 1 in self mode); num_usable is state[0] of the build as the caller read
 *     it back (the build synchronises `stream` once to read it itself).  The reference raises
 *     there too (n_neighbors > n_samples).
 *  6. m = 0 launches nothing; n = 0 is GSR_EINVAL.
 * Nothing is allocated here.  gsr_knn_workspace_bytes(what, n, m, k): bytes of the tree (what = 0:
 * n; kept as long as the cloud is queried), of the build's workspace (1: n), of a tree query's
 * workspace (2: m and k; the exhaustive query needs none); 0 when the sizes do not fit (n, m in
 * [1, 2^28], k in [1, 16] for what = 2) or a size query of rocPRIM fails (no device).  All buffers
 * 256-byte aligned; none needs to be zeroed.
 *   state  int32 [4]   build: 0 usable reference points, 1 reference points left out;
 *                      query: 2 non-finite queries (0, 1 and 3 are left alone)
 * gsr_knn_query with GSR_KNN_EXHAUSTIVE tests every query against every usable reference point
 * instead of walking the tree (the on-device cross-check, never chosen by the library itself);
 * both paths evaluate a pair with the same device function. */
#define GSR_KNN_MAX_K 16
#define GSR_KNN_EXHAUSTIVE 1
#define GSR_KNN_SELF 2
#define GSR_KNN_BYTES_TREE 0
#define GSR_KNN_BYTES_BUILD 1
#define GSR_KNN_BYTES_QUERY 2
size_t gsr_knn_workspace_bytes(int what, int num_points, int num_queries, int k);
int gsr_knn_build(int num_points, const float *points, void *tree, size_t tree_bytes,
                  void *workspace, size_t workspace_bytes, int32_t *state, gsr_stream_t stream);
int gsr_knn_query(int num_points, const void *tree, size_t tree_bytes, int num_usable,
                  int num_queries, const float *queries, int k, int flags, void *workspace,
                  size_t workspace_bytes, float *distance, int32_t *index, int32_t *state,
                  gsr_stream_t stream);

/* ---- targets from an integer image cache (csrc/target.hip) ------
 * A training step's ground truth formed from images that stay uint8 on the device, in the
 * order of the models' get_gt_img (vanilla_gs.py:859-881): convert, resize, composite.
 * gsr_target_from_u8: image uint8 [height,width,channels], channels 3 or 4 (RGBA 4-byte
 *   aligned); background float32 [3] ON THE DEVICE (read for channels = 4 only); out float32
 *   [out_height,out_width,3].  Per output pixel and channel:
 *     1. v = float(u8) / 255, correctly rounded;
 *     2. bilinear resize without antialiasing, half-pixel centres (align_corners = False):
 *        per axis s = max(scale * (dst + 0.5) - 0.5, 0) with scale = float(in) / float(out),
 *        i0 = int(s), i1 = i0 + (i0 < in - 1), l1 = s - i0, l0 = 1 - l1;
 *        value = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11); alpha included;
 *     3. channels = 4: a * rgb + (1 - a) * background from the RESIZED rgba.
 *   Every operation is rounded on its own (no contraction).  out == in: no resize, the value is
 *   v00 itself, and with channels = 3 the output is exactly u8 / 255.
 * gsr_plane_from_int: plane uint8 (elem_bytes 1) or uint16 (2) [height,width]; out float32
 *   [out_height,out_width]: v = float(value) * unit, then step 2.  Masks (unit 1), 16-bit depth
 *   in millimetres (1e-3), 8-bit monocular depth (1 / 255); zeros are interpolated like any
 *   other value.
 * Both: 1 <= out_height <= height, 1 <= out_width <= width, out_height <= 262140 (GSR_EINVAL
 * otherwise, nothing launched).  One launch, nothing allocated, no workspace. */
int gsr_target_from_u8(const uint8_t *image, int height, int width, int channels,
                       const float *background, int out_height, int out_width, float *out,
                       gsr_stream_t stream);
int gsr_plane_from_int(const void *plane, int elem_bytes, int height, int width, float unit,
                       int out_height, int out_width, float *out, gsr_stream_t stream);

/* ---- measurement hook ---------------------------------------------------------
 * counters: two device uint64 (or NULL = off, the default).  While set, the 16x16
 * compositing kernels add the number of list entries they stage to counters[0]
 * (forward) / counters[1] (backward): tiles stop once every pixel is saturated, so
 * this is what a launch really reads of the lists (bench.py prices the roofline on
 * it).  Device-wide setting (synchronises the device); not for production loops. */
int gsr_debug_count_staged(unsigned long long *counters);

/* ---- measurement hook: who ran when ---------------------------------------------
 * records: device buffer of 2 * capacity_waves * 4 uint64 (or NULL = off, the
 * default).  While set, every wave of the 16x16 compositing kernels that runs its
 * tile to the end writes {100-MHz clock at entry, at exit, tile | sub-tile mask <<
 * 32, list length | hardware id << 32} to record blockIdx.x -- forward launches to
 * the first capacity_waves records, backward launches to the second half.  The
 * tail and the imbalance of a launch (tools/exp/wave_trace.py).  Device-wide
 * setting (synchronises the device); not for production loops. */
int gsr_debug_wave_trace(unsigned long long *records, unsigned capacity_waves);

/* ---- box calibration (bench.py `calibration`; not part of the path) ----------
 * Two fixed workloads, timed by the caller with events on `stream` next to the
 * bench's own steps, so that a move of the headline between two GPU leases can be
 * attributed to the box (clock state, memory) or to the code.
 * gsr_calibrate_valu: `workgroups` x 256 lanes each run `iters` rounds of 8
 *   independent non-packed fp32 fma chains; returns the number of VALU
 *   lane-operations launched (8 * iters * 256 * workgroups; -1 on error);
 *   scratch: at least `workgroups` floats (never written).
 * gsr_calibrate_copy: float4 grid-stride copy of `bytes` (multiple of 16). */
long long gsr_calibrate_valu(int iters, int workgroups, float *scratch,
                             gsr_stream_t stream);
int gsr_calibrate_copy(const void *src, void *dst, size_t bytes,
                       gsr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRASTER_H_ */
