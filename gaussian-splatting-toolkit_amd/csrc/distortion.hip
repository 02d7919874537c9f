// distortion.hip -- the depth-distortion term and the median depth of a view: one front-to-back walk over the tile
// lists, and the walk's backward (include/gsraster.h, gsr_distortion_*).
//
// Per pixel, over the contributing entries i = 1..n of its tile's list (the forward compositing's rule, gsr_common.h
// thresholds, raster_fwd_generic_kernel's expressions), T_i the transmittance before entry i, w_i = alpha_i T_i,
// A_i = 1 - T_{i+1} = sum_{j<=i} w_j, B_i = sum_{j<=i} w_j z_j:
//   distortion = 2 sum_i w_i (z_i A_{i-1} - B_{i-1})      (= sum_i sum_j w_i w_j |z_i - z_j| for sorted z)
//   median     = z_i of the last contributing entry with T_i > 0.5
// The term is quadratic in the weights, so it is no further channel of the compositing passes: the forward carries
// (T, B) next to the sum, the backward rebuilds them back to front from (final_T, B_n) and carries
// S = sum_{i>k} w_i g_i, g_k = dD/dw_k.
//
// Shape: one 16 x 16 tile per workgroup, one lane per pixel, list entries staged through LDS 256 at a time.  Backward:
// all 64 lanes of a wave work on the same entry at the same time, so their seven contributions are first summed over
// each row of 16 lanes with four DPP steps, and one lane per row adds the row's sum to the batch's accumulators in LDS
// (4 instead of 64 colliding ds_add per component and wave); one global atomic per (tile, splat, component) closes
// the batch.  LDS: 8 KB staging + 7 KB accumulators per workgroup -- the four waves' registers, not LDS, bound the
// residency.  Atomic sums: not bit-reproducible.
#include "gsr_common.h"

namespace {

constexpr int BW = 16;
constexpr int BSIZE = BW * BW;
constexpr int NCOMP = 7;  // v_xy 2, v_conic 3, v_opacity 1, v_values 1

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), CTRL, 0xf, 0xf, true));
}
// the sum over a row of 16 lanes, in every lane of the row (disabled lanes read as 0)
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_move<0x141>(v);  // row_half_mirror
  v += dpp_move<0x140>(v);  // row_mirror
  return v;
}

__global__ __launch_bounds__(BSIZE) void distortion_fwd_kernel(
    const int tiles_x, const int img_w, const int img_h, const int *__restrict__ ids_sorted,
    const int2 *__restrict__ tile_bins, const float2 *__restrict__ xys, const float *__restrict__ conics,
    const float *__restrict__ opacities, const float *__restrict__ values, float *__restrict__ out_distortion,
    float *__restrict__ out_median, float *__restrict__ out_vsum, float *__restrict__ final_Ts,
    int *__restrict__ final_idx) {
  __shared__ float s_x[BSIZE], s_y[BSIZE], s_o[BSIZE], s_a[BSIZE], s_b[BSIZE], s_c[BSIZE], s_z[BSIZE];

  const int tr = threadIdx.y * BW + threadIdx.x;
  const int tile = blockIdx.y * tiles_x + blockIdx.x;
  const int col = blockIdx.x * BW + threadIdx.x;
  const int row = blockIdx.y * BW + threadIdx.y;
  const float px = (float)col, py = (float)row;
  const bool inside = col < img_w && row < img_h;
  bool done = !inside;

  float T = 1.f, median = 0.f;  // (T in float32 by the compositing's own operations: its decisions are the forward's)
  // ... and next to it the same product and the two sums in float64: the backward rebuilds T_k and B_k from final_T
  // and B_n by division and subtraction, and n float32 roundings on the way forward would not cancel on the way back
  double Td = 1.0, B = 0.0, D = 0.0;
  int last = -1;

  const int2 range = tile_bins[tile];
  for (int base = range.x; base < range.y; base += BSIZE) {
    if (__syncthreads_count(done ? 1 : 0) >= BSIZE) break;
    const int idx = base + tr;
    if (idx < range.y) {
      const int g = ids_sorted[idx];
      const float2 xy = xys[g];
      s_x[tr] = xy.x;
      s_y[tr] = xy.y;
      s_o[tr] = opacities[g];
      s_a[tr] = conics[3 * g];
      s_b[tr] = conics[3 * g + 1];
      s_c[tr] = conics[3 * g + 2];
      s_z[tr] = values[g];
    }
    __syncthreads();
    const int count = min(BSIZE, range.y - base);
    for (int t = 0; t < count && !done; ++t) {
      const float dx = s_x[t] - px, dy = s_y[t] - py;
      const float sigma = 0.5f * (s_a[t] * dx * dx + s_c[t] * dy * dy) + s_b[t] * dx * dy;
      const float alpha = fminf(GSR_ALPHA_MAX_FWD, s_o[t] * __expf(-sigma));
      if (sigma < 0.f || alpha < GSR_ALPHA_MIN) continue;
      const float next_T = T * (1.f - alpha);
      if (next_T <= GSR_T_EPS) {
        done = true;
        break;
      }
      const float z = s_z[t];
      const double w = (double)alpha * Td;
      D += w * ((double)z * (1.0 - Td) - B);
      B += w * (double)z;
      if (T > 0.5f) median = z;
      T = next_T;
      Td *= 1.0 - (double)alpha;
      last = base + t;
    }
  }

  if (inside) {
    const size_t pid = (size_t)row * img_w + col;
    out_distortion[pid] = (float)(2.0 * D);
    out_median[pid] = median;
    out_vsum[pid] = (float)B;
    final_Ts[pid] = (float)Td;
    final_idx[pid] = last;
  }
}

__global__ __launch_bounds__(BSIZE) void distortion_bwd_kernel(
    const int tiles_x, const int img_w, const int img_h, const int *__restrict__ ids_sorted,
    const int2 *__restrict__ tile_bins, const float2 *__restrict__ xys, const float *__restrict__ conics,
    const float *__restrict__ opacities, const float *__restrict__ values, const float *__restrict__ out_vsum,
    const float *__restrict__ final_Ts, const int *__restrict__ final_idx, const float *__restrict__ v_distortion,
    float *__restrict__ v_xy, float *__restrict__ v_conic, float *__restrict__ v_opacity,
    float *__restrict__ v_values) {
  __shared__ float s_acc[BSIZE * NCOMP];
  __shared__ int s_id[BSIZE];
  __shared__ float s_x[BSIZE], s_y[BSIZE], s_o[BSIZE], s_a[BSIZE], s_b[BSIZE], s_c[BSIZE], s_z[BSIZE];
  __shared__ int s_top;

  const int tr = threadIdx.y * BW + threadIdx.x;
  const int tile = blockIdx.y * tiles_x + blockIdx.x;
  const int col = blockIdx.x * BW + threadIdx.x;
  const int row = blockIdx.y * BW + threadIdx.y;
  const float px = (float)col, py = (float)row;
  const bool inside = col < img_w && row < img_h;

  const int2 range = tile_bins[tile];
  float T_final = 1.f, Bn = 0.f, vD = 0.f;
  int bin_final = -1;
  if (inside) {
    const size_t pid = (size_t)row * img_w + col;
    T_final = final_Ts[pid];
    Bn = out_vsum[pid];
    vD = v_distortion[pid];
    bin_final = final_idx[pid];
  }
  // The per-pixel state in float64: T by n divisions and B by n subtractions in float32 would each carry n roundings
  // into differences that are small against their operands (values of one surface differ by per cent)
  const double Tn = (double)T_final, Bnd = (double)Bn;
  double T = Tn;   // T_{k+1} on the way back
  double B = Bnd;  // B_k
  double S = 0.0;  // sum_{i>k} w_i g_i

  if (tr == 0) s_top = -1;
  __syncthreads();
  if (bin_final >= 0) atomicMax(&s_top, bin_final);
  __syncthreads();
  const int top = min(range.y - 1, s_top);

  for (int hi = top; hi >= range.x; hi -= BSIZE) {
    __syncthreads();  // previous batch fully flushed
    const int idx = hi - tr;
    if (idx >= range.x) {
      const int g = ids_sorted[idx];
      s_id[tr] = g;
      const float2 xy = xys[g];
      s_x[tr] = xy.x;
      s_y[tr] = xy.y;
      s_o[tr] = opacities[g];
      s_a[tr] = conics[3 * g];
      s_b[tr] = conics[3 * g + 1];
      s_c[tr] = conics[3 * g + 2];
      s_z[tr] = values[g];
    }
#pragma unroll
    for (int k = 0; k < NCOMP; ++k) s_acc[tr * NCOMP + k] = 0.f;
    __syncthreads();
    const int count = min(BSIZE, hi - range.x + 1);
    for (int t = 0; t < count; ++t) {
      const float dx = s_x[t] - px, dy = s_y[t] - py;
      const float a = s_a[t], b = s_b[t], c = s_c[t], opac = s_o[t], z = s_z[t];
      const float sigma = 0.5f * (a * dx * dx + c * dy * dy) + b * dx * dy;
      const float vis = __expf(-sigma);
      const float raw = opac * vis;
      const float alpha = fminf(GSR_ALPHA_MAX_FWD, raw);
      const bool valid = (hi - t <= bin_final) && !(sigma < 0.f || alpha < GSR_ALPHA_MIN);
      if (!__any(valid ? 1 : 0)) continue;  // wave-uniform: the row sums below run with every lane of the wave
      float v_sigma = 0.f, v_opac = 0.f, v_z = 0.f;
      if (valid) {
        const double zd = (double)z;
        // 1 / (1 - alpha): the float32 reciprocal and one Newton step in float64 (relative error ~1e-13; 1 - alpha is
        // in [0.001, 1]) instead of the dozen instructions of a float64 division
        const double rest = 1.0 - (double)alpha;
        const double r0 = (double)__builtin_amdgcn_rcpf((float)rest);
        const double ra = r0 * (2.0 - rest * r0);
        const double Tk = T * ra;      // T_k
        const double w = (double)alpha * Tk;
        const double Bp = B - w * zd;  // B_{k-1}
        const double behind = T - Tn;  // A_n - A_k
        const double Ap = 1.0 - Tk;    // A_{k-1}
        const double g = 2.0 * (zd * Ap - Bp + (Bnd - B) - zd * behind);
        v_z = (float)(2.0 * w * (Ap - behind) * (double)vD);
        if (raw <= GSR_ALPHA_MAX_FWD) {  // (clamped: alpha does not depend on the inputs)
          const float v_alpha = (float)((Tk * g - S * ra) * (double)vD);
          v_sigma = -opac * vis * v_alpha;
          v_opac = vis * v_alpha;
        }
        S += w * g;
        T = Tk;
        B = Bp;
      }
      float part[NCOMP] = {v_sigma * (a * dx + b * dy), v_sigma * (b * dx + c * dy), 0.5f * v_sigma * dx * dx,
                           v_sigma * dx * dy,           0.5f * v_sigma * dy * dy,    v_opac,
                           v_z};
      float *acc = s_acc + t * NCOMP;
#pragma unroll
      for (int k = 0; k < NCOMP; ++k) {
        const float r = row16_sum(part[k]);
        if (threadIdx.x == 0 && r != 0.f) atomicAdd(acc + k, r);
      }
    }
    __syncthreads();
    if (tr < count) {
      const size_t g = (size_t)s_id[tr];
      const float *acc = s_acc + tr * NCOMP;
      if (acc[0] != 0.f) unsafeAtomicAdd(v_xy + 2 * g, acc[0]);
      if (acc[1] != 0.f) unsafeAtomicAdd(v_xy + 2 * g + 1, acc[1]);
      if (acc[2] != 0.f) unsafeAtomicAdd(v_conic + 3 * g, acc[2]);
      if (acc[3] != 0.f) unsafeAtomicAdd(v_conic + 3 * g + 1, acc[3]);
      if (acc[4] != 0.f) unsafeAtomicAdd(v_conic + 3 * g + 2, acc[4]);
      if (acc[5] != 0.f) unsafeAtomicAdd(v_opacity + g, acc[5]);
      if (acc[6] != 0.f) unsafeAtomicAdd(v_values + g, acc[6]);
    }
  }
}

int check_image(const char *who, int tiles_x, int tiles_y, unsigned img_w, unsigned img_h) {
  GSR_REQUIRE(img_w > 0 && img_h > 0, "%s: empty image", who);
  GSR_REQUIRE((unsigned long long)img_w * img_h < (1ull << 31), "%s: the image must hold fewer than 2^31 pixels", who);
  GSR_REQUIRE(tiles_x == (int)gsr_cdiv(img_w, BW) && tiles_y == (int)gsr_cdiv(img_h, BW),
              "%s: tile bounds (%d,%d) do not match image %ux%u / block %d", who, tiles_x, tiles_y, img_w, img_h, BW);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT int gsr_distortion_forward(int tiles_x, int tiles_y, unsigned img_w, unsigned img_h, const int32_t *ids,
                                      const int32_t *bins, const float *xys, const float *conics,
                                      const float *opacities, const float *values, float *out_distortion,
                                      float *out_median, float *out_vsum, float *final_Ts, int32_t *final_idx,
                                      gsr_stream_t stream) {
  if (int rc = check_image("distortion_forward", tiles_x, tiles_y, img_w, img_h)) return rc;
  GSR_REQUIRE(ids && bins && xys && conics && opacities && values && out_distortion && out_median && out_vsum &&
                  final_Ts && final_idx,
              "distortion_forward: null pointer");
  hipLaunchKernelGGL(distortion_fwd_kernel, dim3(tiles_x, tiles_y), dim3(BW, BW), 0, (hipStream_t)stream, tiles_x,
                     (int)img_w, (int)img_h, ids, reinterpret_cast<const int2 *>(bins),
                     reinterpret_cast<const float2 *>(xys), conics, opacities, values, out_distortion, out_median,
                     out_vsum, final_Ts, final_idx);
  GSR_CHECK_LAUNCH("distortion_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_distortion_backward(unsigned img_h, unsigned img_w, int num_points, const int32_t *ids,
                                       const int32_t *bins, const float *xys, const float *conics,
                                       const float *opacities, const float *values, const float *out_vsum,
                                       const float *final_Ts, const int32_t *final_idx, const float *v_distortion,
                                       float *v_xy, float *v_conic, float *v_opacity, float *v_values,
                                       gsr_stream_t stream) {
  const int tiles_x = (int)gsr_cdiv(img_w, BW), tiles_y = (int)gsr_cdiv(img_h, BW);
  if (int rc = check_image("distortion_backward", tiles_x, tiles_y, img_w, img_h)) return rc;
  GSR_REQUIRE(num_points >= 1, "distortion_backward: num_points must be positive");
  GSR_REQUIRE(ids && bins && xys && conics && opacities && values && out_vsum && final_Ts && final_idx &&
                  v_distortion && v_xy && v_conic && v_opacity && v_values,
              "distortion_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)num_points;
  if (v_conic == v_xy + 2 * n && v_opacity == v_conic + 3 * n && v_values == v_opacity + n) {
    // (the Python binding lays the four out back to back: one fill)
    if (int rc = gsr_zero_async(v_xy, sizeof(float) * NCOMP * n, s)) return rc;
  } else {
    if (int rc = gsr_zero_async(v_xy, sizeof(float) * 2 * n, s)) return rc;
    if (int rc = gsr_zero_async(v_conic, sizeof(float) * 3 * n, s)) return rc;
    if (int rc = gsr_zero_async(v_opacity, sizeof(float) * n, s)) return rc;
    if (int rc = gsr_zero_async(v_values, sizeof(float) * n, s)) return rc;
  }
  hipLaunchKernelGGL(distortion_bwd_kernel, dim3(tiles_x, tiles_y), dim3(BW, BW), 0, s, tiles_x, (int)img_w,
                     (int)img_h, ids, reinterpret_cast<const int2 *>(bins), reinterpret_cast<const float2 *>(xys),
                     conics, opacities, values, out_vsum, final_Ts, final_idx, v_distortion, v_xy, v_conic, v_opacity,
                     v_values);
  GSR_CHECK_LAUNCH("distortion_backward");
  return GSR_OK;
}
