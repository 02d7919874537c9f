// kmeans.hip -- Lloyd's k-means over rows of up to 48 floats, gfx950: the nearest-centroid assignment, the centroid
// update and the float64 inertia (include/gsraster.h, gsr_kmeans_assign / _update / _inertia).
// What builds the codebook of the spherical-harmonics rows in a compressed export (gs_io.compressed).
//
// Built with -ffp-contract=off (csrc/Makefile): a distance is the float32 sum of (x_j - c_j)^2 over j = 0, 1, ... with the
// subtraction, the product and the sum each rounded on its own -- the order tests/kmeans_reference.py restates in NumPy,
// so labels and distances are held bit for bit.  The update and the inertia sum in float64 in an order that depends on
// the sizes and the launch constants only, without atomics: bit-reproducible from run to run.
#include "gsr_common.h"

#include <math.h>

namespace {

#define GSR_KMEANS_THREADS 256

// ---- assignment -----------------------------------------------------------------------------------------------------
// One point per lane, its row in registers (DP = D rounded up to a multiple of 4; the padding is 0 on both sides and
// adds (0 - 0)^2 = +0 to a sum that is >= +0 or NaN: the bits do not move).  The centroids pass through LDS in tiles of
// GSR_KMEANS_TILE rows of DP floats; every lane reads the same address (a broadcast, no bank conflict) as 128-bit
// reads, four centroids at a time in four independent accumulators.  Rows that pad the last tile to a multiple of four
// hold NaN: a NaN distance is never below `best`, so they never win.  The comparison is strict and visits the
// centroids in index order: ties go to the lowest index, a row whose distances are all NaN or +inf keeps label 0.
template <int DP>
__global__ __launch_bounds__(GSR_KMEANS_THREADS) void kmeans_assign_kernel(
    const int n, const int d, const int k, const float *__restrict__ points, const float *__restrict__ centroids,
    int *__restrict__ labels, float *__restrict__ dist) {
  __shared__ __attribute__((aligned(16))) float tile[GSR_KMEANS_TILE * DP];
  const long long ii = (long long)blockIdx.x * GSR_KMEANS_THREADS + threadIdx.x;
  const size_t row = (size_t)(ii < n ? ii : n - 1) * (size_t)d;  // (lanes past the end keep the barriers company)
  float x[DP];
#pragma unroll
  for (int j = 0; j < DP; ++j) x[j] = j < d ? points[row + j] : 0.f;

  float best = INFINITY;
  int label = 0;
  for (int base = 0; base < k; base += GSR_KMEANS_TILE) {
    const int rows = min(GSR_KMEANS_TILE, k - base);
    const int rows4 = (rows + 3) & ~3;
    __syncthreads();  // the previous tile has been read by every wave
    for (int e = threadIdx.x; e < rows4 * DP; e += GSR_KMEANS_THREADS) {
      const int r = e / DP, j = e - r * DP;
      float v = 0.f;
      if (r >= rows)
        v = NAN;
      else if (j < d)
        v = centroids[(size_t)(base + r) * (size_t)d + j];
      tile[e] = v;
    }
    __syncthreads();
    for (int r = 0; r < rows4; r += 4) {
      const float4 *__restrict__ c0 = reinterpret_cast<const float4 *>(tile + (r + 0) * DP);
      const float4 *__restrict__ c1 = reinterpret_cast<const float4 *>(tile + (r + 1) * DP);
      const float4 *__restrict__ c2 = reinterpret_cast<const float4 *>(tile + (r + 2) * DP);
      const float4 *__restrict__ c3 = reinterpret_cast<const float4 *>(tile + (r + 3) * DP);
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) {
        const float4 u0 = c0[q], u1 = c1[q], u2 = c2[q], u3 = c3[q];
        float t;
#define GSR_KMEANS_TERM(a, u, m, j) \
  t = x[j] - u.m;                   \
  a = a + t * t;
        GSR_KMEANS_TERM(a0, u0, x, 4 * q) GSR_KMEANS_TERM(a1, u1, x, 4 * q)
        GSR_KMEANS_TERM(a2, u2, x, 4 * q) GSR_KMEANS_TERM(a3, u3, x, 4 * q)
        GSR_KMEANS_TERM(a0, u0, y, 4 * q + 1) GSR_KMEANS_TERM(a1, u1, y, 4 * q + 1)
        GSR_KMEANS_TERM(a2, u2, y, 4 * q + 1) GSR_KMEANS_TERM(a3, u3, y, 4 * q + 1)
        GSR_KMEANS_TERM(a0, u0, z, 4 * q + 2) GSR_KMEANS_TERM(a1, u1, z, 4 * q + 2)
        GSR_KMEANS_TERM(a2, u2, z, 4 * q + 2) GSR_KMEANS_TERM(a3, u3, z, 4 * q + 2)
        GSR_KMEANS_TERM(a0, u0, w, 4 * q + 3) GSR_KMEANS_TERM(a1, u1, w, 4 * q + 3)
        GSR_KMEANS_TERM(a2, u2, w, 4 * q + 3) GSR_KMEANS_TERM(a3, u3, w, 4 * q + 3)
#undef GSR_KMEANS_TERM
      }
      const int c = base + r;
      if (a0 < best) { best = a0; label = c; }
      if (a1 < best) { best = a1; label = c + 1; }
      if (a2 < best) { best = a2; label = c + 2; }
      if (a3 < best) { best = a3; label = c + 3; }
    }
  }
  if (ii < n) {
    labels[ii] = label;
    dist[ii] = best;
  }
}

// ---- float64 sums ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double kmeans_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < GSR_WAVE; m <<= 1) v += __shfl_xor(v, m, GSR_WAVE);
  return v;  // (the same bits in every lane: a + b and b + a round alike)
}

// ---- update ---------------------------------------------------------------------------------------------------------
// One workgroup per cluster.  Thread t adds the members t, t + 256, ... of the cluster's segment of `order`, in that
// order, into DP float64 sums of w x_j and one of w (a float32 times a float32 is exact in float64); a wave's 64 lanes
// are added by the butterfly, the four waves in index order through LDS.  The order of every addition is a function of
// the segment's length alone.  A wave the segment does not reach contributes +0 without the butterfly (which would
// give +0 as well).  A member whose label is not this cluster, or whose index is outside [0, n), is skipped: an
// inconsistent `order` can neither mix clusters nor read outside `points`.
template <int DP>
__global__ __launch_bounds__(GSR_KMEANS_THREADS) void kmeans_update_kernel(
    const int n, const int d, const float *__restrict__ points, const int *__restrict__ labels,
    const int *__restrict__ order, const int *__restrict__ offsets, const float *__restrict__ weights,
    const float *__restrict__ old_centroids, float *__restrict__ new_centroids, int *__restrict__ counts) {
  __shared__ double wave_sums[GSR_KMEANS_THREADS / GSR_WAVE][DP + 1];
  const int c = blockIdx.x;
  const int begin = min(max(offsets[c], 0), n), end = min(max(offsets[c + 1], begin), n);
  const int wave = threadIdx.x / GSR_WAVE, lane = threadIdx.x % GSR_WAVE;
  double acc[DP], wsum = 0.0;
#pragma unroll
  for (int j = 0; j < DP; ++j) acc[j] = 0.0;
  for (int m = begin + (int)threadIdx.x; m < end; m += GSR_KMEANS_THREADS) {
    const int i = order[m];
    if ((unsigned)i >= (unsigned)n || labels[i] != c) continue;
    const double w = weights ? (double)weights[i] : 1.0;
    const float *__restrict__ p = points + (size_t)i * (size_t)d;
#pragma unroll
    for (int j = 0; j < DP; ++j)
      if (j < d) acc[j] += w * (double)p[j];
    wsum += w;
  }
  if (end - begin > wave * GSR_WAVE) {  // wave-uniform
#pragma unroll
    for (int j = 0; j < DP; ++j) acc[j] = kmeans_wave_sum(acc[j]);
    wsum = kmeans_wave_sum(wsum);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < DP; ++j) wave_sums[wave][j] = acc[j];
    wave_sums[wave][DP] = wsum;
  }
  __syncthreads();
  if ((int)threadIdx.x < d) {
    const int j = threadIdx.x;
    const double s = ((wave_sums[0][j] + wave_sums[1][j]) + wave_sums[2][j]) + wave_sums[3][j];
    const double ws = ((wave_sums[0][DP] + wave_sums[1][DP]) + wave_sums[2][DP]) + wave_sums[3][DP];
    const size_t at = (size_t)c * (size_t)d + j;
    // (no member, or weights that sum to zero -- not below it, the weights are >= 0: the old centroid's bits)
    new_centroids[at] = (end > begin && ws > 0.0) ? (float)(s / ws) : old_centroids[at];
  }
  if (threadIdx.x == 0) counts[c] = end - begin;
}

// ---- inertia --------------------------------------------------------------------------------------------------------
// sum_i w_i sum_j (x_ij - c_{l_i j})^2 in float64, j in index order: lane (GSR_KMEANS_INERTIA_PER_LANE points, 256
// apart, in order) -> wave (butterfly) -> workgroup (the four waves in order) -> grid (kmeans_inertia_final_kernel over
// the per-workgroup partials), as the camera-gradient sums of project.hip reduce.  A label outside [0, k) adds nothing.
#define GSR_KMEANS_INERTIA_PER_LANE (GSR_KMEANS_INERTIA_SHARE / GSR_KMEANS_THREADS)

__device__ __forceinline__ double kmeans_block_sum(double v, double *wave_sums) {
  v = kmeans_wave_sum(v);
  if (threadIdx.x % GSR_WAVE == 0) wave_sums[threadIdx.x / GSR_WAVE] = v;
  __syncthreads();
  return ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
}

__global__ __launch_bounds__(GSR_KMEANS_THREADS) void kmeans_inertia_partial_kernel(
    const int n, const int d, const int k, const float *__restrict__ points, const float *__restrict__ centroids,
    const int *__restrict__ labels, const float *__restrict__ weights, double *__restrict__ partials) {
  __shared__ double wave_sums[GSR_KMEANS_THREADS / GSR_WAVE];
  double acc = 0.0;
  const long long base = (long long)blockIdx.x * GSR_KMEANS_INERTIA_SHARE + threadIdx.x;
#pragma unroll 1
  for (int s = 0; s < GSR_KMEANS_INERTIA_PER_LANE; ++s) {
    const long long i = base + (long long)s * GSR_KMEANS_THREADS;
    if (i >= n) break;
    const int l = labels[i];
    if ((unsigned)l >= (unsigned)k) continue;
    const float *__restrict__ p = points + (size_t)i * (size_t)d;
    const float *__restrict__ c = centroids + (size_t)l * (size_t)d;
    double dd = 0.0;
    for (int j = 0; j < d; ++j) {
      const double t = (double)p[j] - (double)c[j];
      dd = dd + t * t;
    }
    acc += (weights ? (double)weights[i] : 1.0) * dd;
  }
  const double total = kmeans_block_sum(acc, wave_sums);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// One workgroup: thread t adds the partials t, t + 256, ... in that order, then wave and workgroup as above.
__global__ __launch_bounds__(GSR_KMEANS_THREADS) void kmeans_inertia_final_kernel(
    const int num_partials, const double *__restrict__ partials, double *__restrict__ out) {
  __shared__ double wave_sums[GSR_KMEANS_THREADS / GSR_WAVE];
  double acc = 0.0;
  for (int b = threadIdx.x; b < num_partials; b += GSR_KMEANS_THREADS) acc += partials[b];
  const double total = kmeans_block_sum(acc, wave_sums);
  if (threadIdx.x == 0) out[0] = total;
}

bool kmeans_sizes_ok(const char *what, int n, int d, int k) {
  if (n < 0 || d < 1 || d > GSR_KMEANS_MAX_DIM || k < 1 || k > GSR_KMEANS_MAX_CLUSTERS) {
    gsr_set_error("%s: need num_points >= 0, 1 <= dim <= %d and 1 <= num_clusters <= %d, got %d, %d, %d", what,
                  GSR_KMEANS_MAX_DIM, GSR_KMEANS_MAX_CLUSTERS, n, d, k);
    return false;
  }
  return true;
}

}  // namespace

// (one instantiation per padded width: the rows stay in registers, fully unrolled)
#define GSR_KMEANS_DISPATCH(dim, LAUNCH)                                                    \
  switch (((dim) + 3) / 4) {                                                                \
    case 1: LAUNCH(4); break;                                                               \
    case 2: LAUNCH(8); break;                                                               \
    case 3: LAUNCH(12); break;                                                              \
    case 4: LAUNCH(16); break;                                                              \
    case 5: LAUNCH(20); break;                                                              \
    case 6: LAUNCH(24); break;                                                              \
    case 7: LAUNCH(28); break;                                                              \
    case 8: LAUNCH(32); break;                                                              \
    case 9: LAUNCH(36); break;                                                              \
    case 10: LAUNCH(40); break;                                                             \
    case 11: LAUNCH(44); break;                                                             \
    default: LAUNCH(48); break;                                                             \
  }

GSR_EXPORT int gsr_kmeans_assign(int num_points, int dim, int num_clusters, const float *points,
                                 const float *centroids, int32_t *labels, float *dist, gsr_stream_t stream) {
  if (!kmeans_sizes_ok("kmeans_assign", num_points, dim, num_clusters)) return GSR_EINVAL;
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(points && centroids && labels && dist, "kmeans_assign: null pointer");
  const dim3 grid(gsr_cdiv((unsigned)num_points, GSR_KMEANS_THREADS)), block(GSR_KMEANS_THREADS);
#define GSR_KMEANS_LAUNCH(DP)                                                                                  \
  hipLaunchKernelGGL(kmeans_assign_kernel<DP>, grid, block, 0, (hipStream_t)stream, num_points, dim, num_clusters, \
                     points, centroids, labels, dist)
  GSR_KMEANS_DISPATCH(dim, GSR_KMEANS_LAUNCH)
#undef GSR_KMEANS_LAUNCH
  GSR_CHECK_LAUNCH("kmeans_assign");
  return GSR_OK;
}

GSR_EXPORT int gsr_kmeans_update(int num_points, int dim, int num_clusters, const float *points,
                                 const int32_t *labels, const int32_t *order, const int32_t *offsets,
                                 const float *weights, const float *old_centroids, float *new_centroids,
                                 int32_t *counts, gsr_stream_t stream) {
  if (!kmeans_sizes_ok("kmeans_update", num_points, dim, num_clusters)) return GSR_EINVAL;
  GSR_REQUIRE(offsets && old_centroids && new_centroids && counts, "kmeans_update: null pointer");
  GSR_REQUIRE(num_points == 0 || (points && labels && order), "kmeans_update: null pointer");
  GSR_REQUIRE(old_centroids != new_centroids, "kmeans_update: new_centroids must not alias old_centroids");
  const dim3 grid(num_clusters), block(GSR_KMEANS_THREADS);
#define GSR_KMEANS_LAUNCH(DP)                                                                                   \
  hipLaunchKernelGGL(kmeans_update_kernel<DP>, grid, block, 0, (hipStream_t)stream, num_points, dim, points, labels, \
                     order, offsets, weights, old_centroids, new_centroids, counts)
  GSR_KMEANS_DISPATCH(dim, GSR_KMEANS_LAUNCH)
#undef GSR_KMEANS_LAUNCH
  GSR_CHECK_LAUNCH("kmeans_update");
  return GSR_OK;
}

GSR_EXPORT int gsr_kmeans_inertia(int num_points, int dim, int num_clusters, const float *points,
                                  const float *centroids, const int32_t *labels, const float *weights, double *out,
                                  void *workspace, gsr_stream_t stream) {
  if (!kmeans_sizes_ok("kmeans_inertia", num_points, dim, num_clusters)) return GSR_EINVAL;
  GSR_REQUIRE(out, "kmeans_inertia: null pointer");
  GSR_REQUIRE(((uintptr_t)out & 7u) == 0, "kmeans_inertia: out must be 8-byte aligned");
  if (num_points == 0) return gsr_zero_async(out, sizeof(double), (hipStream_t)stream);
  GSR_REQUIRE(points && centroids && labels && workspace, "kmeans_inertia: null pointer");
  GSR_REQUIRE(((uintptr_t)workspace & 7u) == 0, "kmeans_inertia: workspace must be 8-byte aligned");
  const unsigned blocks = GSR_KMEANS_INERTIA_WORKSPACE_DOUBLES((unsigned)num_points);
  hipLaunchKernelGGL(kmeans_inertia_partial_kernel, dim3(blocks), dim3(GSR_KMEANS_THREADS), 0, (hipStream_t)stream,
                     num_points, dim, num_clusters, points, centroids, labels, weights, (double *)workspace);
  GSR_CHECK_LAUNCH("kmeans_inertia");
  hipLaunchKernelGGL(kmeans_inertia_final_kernel, dim3(1), dim3(GSR_KMEANS_THREADS), 0, (hipStream_t)stream,
                     (int)blocks, (const double *)workspace, out);
  GSR_CHECK_LAUNCH("kmeans_inertia (final)");
  return GSR_OK;
}
