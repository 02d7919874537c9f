// depth_reg.hip -- the depth regularisation of the co-gs model, fused (the rule is stated in
// include/gsraster.h).  What it replaces: DepthGSModel.get_loss_dict, gs_toolkit/models/depth_gs.py:521-528,
//     depth_mask = (pred_depth > 0).detach()
//     nearDepthMean_map = nearMean_map(pred_depth, canny_mask * depth_mask)
//     loss_dict["depth_reg_loss"] = l2_loss(nearDepthMean_map, pred_depth * depth_mask) * 1.0
// with `nearMean_map` two plus-shaped 3x3 convolutions (utils/losses.py:61-81) -- as torch ops two conv2d launches
// and ~10 elementwise kernels forward, as many again backward.  Here: ONE forward kernel (five-tap gathers, the squared
// residual, float64 partial sums per workgroup in a fixed order) + a one-workgroup sum, and ONE backward kernel
// (a gather of what the forward left).  No atomics: the scalar is bit-reproducible.
//
// The per-pixel arithmetic is done in float64 registers (the kernels are bound by their ~6 loads per pixel): what is
// rounded to float32 is the two scratch planes, the gradient and the loss.
#include "gsr_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_BLOCKS = GSR_DEPTH_REG_WORKSPACE_DOUBLES;

struct Tap {
  double a, m;  // pred * m,  m = mask * [pred > 0]
};
__device__ __forceinline__ Tap tap(const float *__restrict__ pred, const float *__restrict__ mask, size_t i) {
  const float p = pred[i];
  const float m = mask[i] * (p > 0.f ? 1.f : 0.f);  // (as the source: a product, so NaN and inf propagate)
  return {(double)p * (double)m, (double)m};
}

// sum of v over the workgroup in a fixed order -> red[0]
__device__ __forceinline__ void block_sum(double v, double *red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
}

// scratch: [2][H][W], with g = 2 (near - pred [pred > 0]) / (H W):
//   0: g (m / (cnt + 1e-8) - [pred > 0])   the pixel's own share of its gradient, formed in float64 BEFORE it is rounded:
//      where near ~ pred (a single pixel, a constant region) the two terms cancel to ~1e-8 of either
//   1: g / (cnt + 1e-8)                    what the four neighbours gather
__global__ __launch_bounds__(TPB) void depth_reg_fwd_kernel(const int H, const int W, const float *__restrict__ pred,
                                                            const float *__restrict__ mask,
                                                            float *__restrict__ scratch,
                                                            double *__restrict__ partial) {
  __shared__ double red[TPB];
  const size_t n = (size_t)H * W;
  const double scale = 2.0 / (double)n;
  double acc = 0.0;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const float p = pred[i];
    const float live = p > 0.f ? 1.f : 0.f;
    const float mc = mask[i] * live;
    double num = (double)p * (double)mc, cnt = (double)mc;
    if (y > 0) { const Tap t = tap(pred, mask, i - W); num += t.a, cnt += t.m; }
    if (y + 1 < H) { const Tap t = tap(pred, mask, i + W); num += t.a, cnt += t.m; }
    if (x > 0) { const Tap t = tap(pred, mask, i - 1); num += t.a, cnt += t.m; }
    if (x + 1 < W) { const Tap t = tap(pred, mask, i + 1); num += t.a, cnt += t.m; }
    const double inv = 1.0 / (cnt + 1e-8);
    const double res = num * inv - (double)p * (double)live;
    acc += res * res;
    if (scratch) {
      const double g = scale * res;
      scratch[i] = (float)(g * ((double)mc * inv - (double)live));
      scratch[n + i] = (float)(g * inv);
    }
  }
  block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(TPB) void depth_reg_final_kernel(const int blocks, const double inv_n,
                                                              const double *__restrict__ partial,
                                                              float *__restrict__ loss_out) {
  __shared__ double red[TPB];
  double v = 0.0;
  for (int b = threadIdx.x; b < blocks; b += TPB) v += partial[b];
  block_sum(v, red);
  if (threadIdx.x == 0) *loss_out = (float)(red[0] * inv_n);
}

// v_pred[q] = upstream * ( m[q] * sum_{p in plus(q)} g[p] / (cnt[p] + 1e-8)  -  g[q] [pred[q] > 0] )
__global__ __launch_bounds__(TPB) void depth_reg_bwd_kernel(const int H, const int W,
                                                            const float *__restrict__ upstream,
                                                            const float *__restrict__ pred,
                                                            const float *__restrict__ mask,
                                                            const float *__restrict__ scratch,
                                                            float *__restrict__ v_pred) {
  const size_t n = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
  const float *__restrict__ gw = scratch + n;
  double s = 0.0;
  if (y > 0) s += (double)gw[i - W];
  if (y + 1 < H) s += (double)gw[i + W];
  if (x > 0) s += (double)gw[i - 1];
  if (x + 1 < W) s += (double)gw[i + 1];
  const float p = pred[i];
  const float live = p > 0.f ? 1.f : 0.f;
  const double m = (double)(mask[i] * live);
  v_pred[i] = (float)((double)upstream[0] * (m * s + (double)scratch[i]));
}

int check_shape(unsigned H, unsigned W, const char *who) {
  GSR_REQUIRE(H > 0 && W > 0 && (unsigned long long)H * W <= 0x7fffffffull, "%s: H * W must be in [1, 2^31)", who);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT int gsr_depth_reg_forward(unsigned img_height, unsigned img_width, const float *pred, const float *mask,
                                     float *scratch, double *partial, float *loss_out, gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "depth_reg_forward")) return rc;
  GSR_REQUIRE(pred && mask && partial && loss_out, "depth_reg_forward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  const size_t want = (n + TPB - 1) / TPB;
  const int blocks = (int)(want < (size_t)MAX_BLOCKS ? want : (size_t)MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_reg_fwd_kernel, dim3(blocks), dim3(TPB), 0, s, (int)img_height, (int)img_width, pred, mask,
                     scratch, partial);
  GSR_CHECK_LAUNCH("depth_reg_forward");
  hipLaunchKernelGGL(depth_reg_final_kernel, dim3(1), dim3(TPB), 0, s, blocks, 1.0 / (double)n,
                     (const double *)partial, loss_out);
  GSR_CHECK_LAUNCH("depth_reg_final");
  return GSR_OK;
}

GSR_EXPORT int gsr_depth_reg_backward(unsigned img_height, unsigned img_width, const float *upstream, const float *pred,
                                      const float *mask, const float *scratch, float *v_pred, gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "depth_reg_backward")) return rc;
  GSR_REQUIRE(upstream && pred && mask && scratch && v_pred, "depth_reg_backward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  hipLaunchKernelGGL(depth_reg_bwd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream,
                     (int)img_height, (int)img_width, upstream, pred, mask, scratch, v_pred);
  GSR_CHECK_LAUNCH("depth_reg_backward");
  return GSR_OK;
}
