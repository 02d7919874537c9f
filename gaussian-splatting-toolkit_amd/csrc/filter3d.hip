// filter3d.hip -- the 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1), gfx950: the
// per-Gaussian sampling rate over the training cameras, and the activations with the filter folded in
// (include/gsraster.h, gsr_filter3d_sampling / gsr_activate_filtered_*).
//
// Built with -ffp-contract=off (csrc/Makefile): the sampling rule and the filter's own terms are written one operation
// per rounding, in the order the float32 NumPy restatement of tests/filter3d_reference.py performs them; `/` and
// sqrtf are correctly rounded.  The expressions the filtered activations share with activations.hip (quaternions, view
// directions, the quaternion VJP) sit in blocks that switch contraction back on, as that file's build has it, so that
// they -- and every row whose filter is zero -- carry the bits of gsr_activate_forward / _backward.
#include "gsr_common.h"

namespace {

// ---- sampling rate ------------------------------------------------------------------------------------------------
// One thread per Gaussian, a loop over the cameras.  `cameras` is read-only, not aliased and indexed by the loop
// counter alone: its 18 words per camera are wave-uniform and come through the scalar cache, not as per-lane gathers.
// nu (0: seen by no camera) goes to `nu_out`; the smallest positive nu of the launch is kept in *best as the LARGEST
// complement of its bit pattern (positive floats order like their bits), so that 0 means "nothing seen": one
// integer atomic per wave after a reduction across its lanes.
#define GSR_FILTER3D_STRIDE 20

__global__ __launch_bounds__(256) void filter3d_rate_kernel(const int n, const float *__restrict__ means,
                                                            const int num_cameras,
                                                            const float *__restrict__ cameras, const float near,
                                                            const float margin, float *__restrict__ nu_out,
                                                            unsigned *__restrict__ best) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned key = 0u;
  if (i < n) {
    const float X = means[3 * i], Y = means[3 * i + 1], Z = means[3 * i + 2];
    float nu = 0.f;
    for (int v = 0; v < num_cameras; ++v) {
      const float *__restrict__ c = cameras + (size_t)GSR_FILTER3D_STRIDE * v;
      const float x = ((c[0] * X + c[1] * Y) + c[2] * Z) + c[3];
      const float y = ((c[4] * X + c[5] * Y) + c[6] * Z) + c[7];
      const float z = ((c[8] * X + c[9] * Y) + c[10] * Z) + c[11];
      const float fx = c[12], fy = c[13], cx = c[14], cy = c[15], W = c[16], H = c[17];
      const float u = (x / z) * fx + cx;
      const float w = (y / z) * fy + cy;
      const float mw = margin * W, mh = margin * H;
      // (a NaN fails every comparison: unseen)
      const bool seen = z > near && u >= -mw && u <= W + mw && w >= -mh && w <= H + mh;
      const float rate = fx / z;
      if (seen && rate > nu) nu = rate;
    }
    nu_out[i] = nu;
    if (nu > 0.f) key = ~__float_as_uint(nu);
  }
  // (every lane of the block reaches this point: whole waves shuffle)
#pragma unroll
  for (int off = GSR_WAVE / 2; off > 0; off >>= 1) key = max(key, (unsigned)__shfl_xor((int)key, off, GSR_WAVE));
  if ((threadIdx.x & (GSR_WAVE - 1)) == 0 && key != 0u) atomicMax(best, key);
}

// filter = k / nu for the seen, k / (the smallest positive nu) for the unseen, 0 when nothing is seen; in place.
__global__ __launch_bounds__(256) void filter3d_finish_kernel(const int n, const float k, float *__restrict__ filter,
                                                              const unsigned *__restrict__ best) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned key = *best;
  const float nu = filter[i];
  float f = 0.f;
  if (key != 0u) f = k / (nu > 0.f ? nu : __uint_as_float(~key));
  filter[i] = f;
}

// ---- filtered activations -----------------------------------------------------------------------------------------
// (the three helpers restate activations.hip's expressions under that file's contraction)
__device__ __forceinline__ float4 unit_quat(const float4 q) {
#pragma clang fp contract(fast)
  const float inv = 1.f / sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
  return make_float4(q.x * inv, q.y * inv, q.z * inv, q.w * inv);
}

__device__ __forceinline__ void view_direction(const float *__restrict__ means, const float *__restrict__ campos,
                                               const int i, float *__restrict__ viewdirs) {
#pragma clang fp contract(fast)
  const float dx = means[3 * i] - campos[0], dy = means[3 * i + 1] - campos[1], dz = means[3 * i + 2] - campos[2];
  const float dinv = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
  viewdirs[3 * i] = dx * dinv;
  viewdirs[3 * i + 1] = dy * dinv;
  viewdirs[3 * i + 2] = dz * dinv;
}

__device__ __forceinline__ float4 unit_quat_vjp(const float4 r, const float4 q, const float4 v) {
#pragma clang fp contract(fast)
  const float inv = 1.f / sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
  const float d = q.x * v.x + q.y * v.y + q.z * v.z + q.w * v.w;
  return make_float4((v.x - q.x * d) * inv, (v.y - q.y * d) * inv, (v.z - q.z * d) * inv, (v.w - q.w * d) * inv);
}

// s'_k = sqrt(s_k^2 + f^2), c = ((s_0 / s'_0) (s_1 / s'_1)) (s_2 / s'_2), o' = o c; f == 0: s' = s, o' = o, the
// unfiltered kernel's bits.
__global__ __launch_bounds__(256) void activate_filtered_fwd_kernel(
    const int n, const float *__restrict__ means, const float *__restrict__ log_scales,
    const float *__restrict__ raw_quats, const float *__restrict__ opacity_logits,
    const float *__restrict__ campos, const float *__restrict__ filter_3d, float *__restrict__ scales,
    float *__restrict__ quats, float *__restrict__ opacities, float *__restrict__ viewdirs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float f = filter_3d[i];
  float s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = expf(log_scales[3 * i + k]);
  float o = 1.f / (1.f + expf(-opacity_logits[i]));
  if (f != 0.f) {
    const float f2 = f * f;
    float c = 1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float sp = sqrtf(s[k] * s[k] + f2);
      const float r = s[k] / sp;
      c = k == 0 ? r : c * r;
      s[k] = sp;
    }
    o = o * c;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) scales[3 * i + k] = s[k];
  reinterpret_cast<float4 *>(quats)[i] = unit_quat(reinterpret_cast<const float4 *>(raw_quats)[i]);
  opacities[i] = o;
  if (viewdirs) view_direction(means, campos, i, viewdirs);
}

// With r_k = s_k / s'_k, c their product, o = sigmoid(a):
//   v_a   = ((v_o' c) o) (1 - o)
//   v_l_k = v_s'_k (s_k r_k) + ((v_o' o) c) ((f / s'_k) (f / s'_k))
// f == 0: v_l_k = v_s_k s_k and v_a = (v_o o) (1 - o), the unfiltered kernel's expressions on the recomputed s and o
// (the same expf and division as the forward's, hence the same bits as the stored ones).
__global__ __launch_bounds__(256) void activate_filtered_bwd_kernel(
    const int n, const float *__restrict__ raw_quats, const float *__restrict__ log_scales,
    const float *__restrict__ quats, const float *__restrict__ opacity_logits, const float *__restrict__ filter_3d,
    const float *__restrict__ v_scales, const float *__restrict__ v_quats, const float *__restrict__ v_opacities,
    float *__restrict__ v_log_scales, float *__restrict__ v_raw_quats, float *__restrict__ v_logits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float f = filter_3d[i];
  float s[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = expf(log_scales[3 * i + k]);
  const float o = 1.f / (1.f + expf(-opacity_logits[i]));
  const float vo = v_opacities ? v_opacities[i] : 0.f;
  float g_l[3], g_a;
  if (f != 0.f) {
    const float f2 = f * f;
    float r[3], t[3], c = 1.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float sp = sqrtf(s[k] * s[k] + f2);
      r[k] = s[k] / sp;
      const float q = f / sp;
      t[k] = q * q;
      c = k == 0 ? r[k] : c * r[k];
    }
    const float voc = (vo * o) * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) g_l[k] = (v_scales ? v_scales[3 * i + k] * (s[k] * r[k]) : 0.f) + voc * t[k];
    g_a = ((vo * c) * o) * (1.f - o);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) g_l[k] = v_scales ? v_scales[3 * i + k] * s[k] : 0.f;
    g_a = v_opacities ? vo * o * (1.f - o) : 0.f;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) v_log_scales[3 * i + k] = g_l[k];
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (v_quats)
    g = unit_quat_vjp(reinterpret_cast<const float4 *>(raw_quats)[i], reinterpret_cast<const float4 *>(quats)[i],
                      reinterpret_cast<const float4 *>(v_quats)[i]);
  reinterpret_cast<float4 *>(v_raw_quats)[i] = g;
  v_logits[i] = g_a;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

GSR_EXPORT int gsr_filter3d_sampling(int num_points, const float *means, int num_cameras, const float *cameras,
                                     float k, float near, float margin, float *filter_out, void *workspace,
                                     gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "filter3d_sampling: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(num_cameras > 0, "filter3d_sampling: num_cameras must be positive");
  GSR_REQUIRE(means && cameras && filter_out && workspace, "filter3d_sampling: null pointer");
  GSR_REQUIRE(aligned16(cameras), "filter3d_sampling: cameras must be 16-byte aligned");
  GSR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "filter3d_sampling: workspace must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int rc = gsr_zero_async(workspace, GSR_FILTER3D_WORKSPACE_BYTES, s);
  if (rc != GSR_OK) return rc;
  const dim3 grid(gsr_cdiv(num_points, 256)), block(256);
  hipLaunchKernelGGL(filter3d_rate_kernel, grid, block, 0, s, num_points, means, num_cameras, cameras, near, margin,
                     filter_out, reinterpret_cast<unsigned *>(workspace));
  GSR_CHECK_LAUNCH("filter3d_sampling (rate)");
  hipLaunchKernelGGL(filter3d_finish_kernel, grid, block, 0, s, num_points, k, filter_out,
                     reinterpret_cast<const unsigned *>(workspace));
  GSR_CHECK_LAUNCH("filter3d_sampling (finish)");
  return GSR_OK;
}

GSR_EXPORT int gsr_activate_filtered_forward(int num_points, const float *means, const float *log_scales,
                                             const float *raw_quats, const float *opacity_logits,
                                             const float *camera_position, const float *filter_3d, float *scales,
                                             float *quats, float *opacities, float *viewdirs, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "activate_filtered_forward: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(log_scales && raw_quats && opacity_logits && filter_3d && scales && quats && opacities,
              "activate_filtered_forward: null pointer");
  GSR_REQUIRE((viewdirs == nullptr) || (means && camera_position),
              "activate_filtered_forward: viewdirs need means and the camera position");
  GSR_REQUIRE(aligned16(raw_quats) && aligned16(quats), "activate_filtered_forward: quaternions must be 16-byte aligned");
  hipLaunchKernelGGL(activate_filtered_fwd_kernel, dim3(gsr_cdiv(num_points, 256)), dim3(256), 0, (hipStream_t)stream,
                     num_points, means, log_scales, raw_quats, opacity_logits, camera_position, filter_3d, scales,
                     quats, opacities, viewdirs);
  GSR_CHECK_LAUNCH("activate_filtered_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_activate_filtered_backward(int num_points, const float *raw_quats, const float *log_scales,
                                              const float *quats, const float *opacity_logits,
                                              const float *filter_3d, const float *v_scales, const float *v_quats,
                                              const float *v_opacities, float *v_log_scales, float *v_raw_quats,
                                              float *v_logits, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "activate_filtered_backward: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(raw_quats && log_scales && quats && opacity_logits && filter_3d && v_log_scales && v_raw_quats &&
                  v_logits,
              "activate_filtered_backward: null pointer");
  GSR_REQUIRE(aligned16(raw_quats) && aligned16(quats) && aligned16(v_raw_quats) &&
                  (v_quats == nullptr || aligned16(v_quats)),
              "activate_filtered_backward: quaternions must be 16-byte aligned");
  hipLaunchKernelGGL(activate_filtered_bwd_kernel, dim3(gsr_cdiv(num_points, 256)), dim3(256), 0, (hipStream_t)stream,
                     num_points, raw_quats, log_scales, quats, opacity_logits, filter_3d, v_scales, v_quats,
                     v_opacities, v_log_scales, v_raw_quats, v_logits);
  GSR_CHECK_LAUNCH("activate_filtered_backward");
  return GSR_OK;
}
