// mono_depth.hip -- the monocular-depth terms of the co-gs loss, fused (the rule is stated in
// include/gsraster.h).  What it replaces: the `use_est_depth` branch of DepthGSModel.get_loss_dict,
// gs_toolkit/models/depth_gs.py:477-531,
//     local_pearson_loss(pred_depth, gt_depth, box_p, 0.5)      utils/losses.py:26-45
//     log(1 + |gt - (scale * pred + shift)|), edge-aware        depth_gs.py:492-519
//     tv_Loss(pred_depth)                                       utils/losses.py:197-207
// as torch ops two [n_corr, box, box] int64 gathers with an atomic index_put_ backward, and a dozen image-sized
// elementwise kernels each way for each of the other two.  Here every term is ONE forward kernel + a one-workgroup sum
// and ONE backward kernel that writes every element of the gradient: no memset, no atomics, no image-sized scratch.
//
// As in depth_reg.hip the per-pixel arithmetic is done in float64 registers and the scalars are float64 sums in a fixed
// order: what is rounded to float32 is the gradient and the loss.  The one float32 operation is the per-view mask, which
// is multiplied in as the model does it (`pred * mask`, `gt * mask`: float32 products).
#include "gsr_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_BLOCKS = GSR_MONO_DEPTH_WORKSPACE_DOUBLES / 2;
constexpr int TILE_W = 64, TILE_H = TPB / TILE_W;  // the pixel tile of one workgroup of the local-Pearson backward

// sum of v over the workgroup in a fixed order, returned to every thread (red may be reused at once)
__device__ __forceinline__ double block_sum(double v, double *red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// depth * mask as the model forms it: a float32 product (NaN and inf propagate); mask == nullptr: no mask
__device__ __forceinline__ double masked(const float *__restrict__ a, const float *__restrict__ mask, size_t i) {
  return (double)(mask ? a[i] * mask[i] : a[i]);
}
__device__ __forceinline__ double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// ---- local Pearson -----------------------------------------------------------------------------------------------
// corner p of the patch list -> (r, c); false when the patch would leave the image (nothing of it is read)
__device__ __forceinline__ bool patch_corner(const void *__restrict__ rows, const void *__restrict__ cols, int idx64,
                                             int p, int H, int W, int box, int &r, int &c) {
  const long long rr = idx64 ? ((const long long *)rows)[p] : (long long)((const int *)rows)[p];
  const long long cc = idx64 ? ((const long long *)cols)[p] : (long long)((const int *)cols)[p];
  r = (int)rr, c = (int)cc;
  return rr >= 0 && rr <= (long long)(H - box) && cc >= 0 && cc <= (long long)(W - box);
}

// one workgroup per patch.  stats[p] = {m_s, m_t, A, B, loss_p}: the means, A = (n - 1) / (n sqrt(S_ss S_tt)),
// B = S_st / S_ss, and the patch's 1 - (n - 1) / n * S_st / sqrt(S_ss S_tt).  Two passes (means, then centred sums:
// E[x^2] - E[x]^2 would cancel on depths of 3 +- 0.01); the second pass reads what the first left in L2.
__global__ __launch_bounds__(TPB) void local_pearson_fwd_kernel(const int H, const int W, const int box,
                                                                const float *__restrict__ pred,
                                                                const float *__restrict__ gt,
                                                                const float *__restrict__ mask,
                                                                const void *__restrict__ rows,
                                                                const void *__restrict__ cols, const int idx64,
                                                                double *__restrict__ stats) {
  __shared__ double red[TPB];
  const int p = blockIdx.x, t = threadIdx.x;
  double *__restrict__ st = stats + 5 * (size_t)p;
  int r, c;
  if (!patch_corner(rows, cols, idx64, p, H, W, box, r, c)) {  // (uniform over the workgroup)
    if (t == 0) st[0] = st[1] = st[2] = st[3] = 0.0, st[4] = __builtin_nan("");
    return;
  }
  const int n = box * box;
  const int dy = TPB / box, dx = TPB % box;  // thread t walks elements t, t + TPB, ...: (y, x) without a division each
  const size_t base = (size_t)r * W + c;
  double ss = 0.0, tt = 0.0;
  for (int i = t, y = t / box, x = t % box; i < n; i += TPB) {
    const size_t k = base + (size_t)y * W + x;
    ss += masked(pred, mask, k), tt += masked(gt, mask, k);
    y += dy, x += dx;
    if (x >= box) x -= box, ++y;
  }
  const double ms = block_sum(ss, red) / (double)n;
  const double mt = block_sum(tt, red) / (double)n;
  double sss = 0.0, stt = 0.0, sst = 0.0;
  for (int i = t, y = t / box, x = t % box; i < n; i += TPB) {
    const size_t k = base + (size_t)y * W + x;
    const double a = masked(pred, mask, k) - ms, b = masked(gt, mask, k) - mt;
    sss += a * a, stt += b * b, sst += a * b;
    y += dy, x += dx;
    if (x >= box) x -= box, ++y;
  }
  sss = block_sum(sss, red);
  stt = block_sum(stt, red);
  sst = block_sum(sst, red);
  if (t == 0) {
    const double root = sqrt(sss * stt), f = (double)(n - 1) / (double)n;
    st[0] = ms, st[1] = mt;
    st[2] = f / root;
    st[3] = sst / sss;
    st[4] = 1.0 - f * sst / root;  // box 1: 0 * (0 / 0); a constant patch: 0 / 0
  }
}

// loss = (sum of the patches' losses in a fixed order) / n_corr; n_corr == 0: 0 / 0
__global__ __launch_bounds__(TPB) void local_pearson_final_kernel(const int n_corr, const double *__restrict__ stats,
                                                                  float *__restrict__ loss_out) {
  __shared__ double red[TPB];
  double v = 0.0;
  for (int p = threadIdx.x; p < n_corr; p += TPB) v += stats[5 * (size_t)p + 4];
  v = block_sum(v, red);
  if (threadIdx.x == 0) *loss_out = (float)(v / (double)n_corr);
}

// exclusive prefix sum of one int per thread over the workgroup (buf: 2 * TPB ints); *total = the sum
__device__ __forceinline__ int block_scan(int v, int *buf, int *total) {
  const int t = threadIdx.x;
  int src = 0;
  buf[t] = v;
  __syncthreads();
  for (int off = 1; off < TPB; off <<= 1) {
    int x = buf[src + t];
    if (t >= off) x += buf[src + t - off];
    src ^= TPB;
    buf[src + t] = x;
    __syncthreads();
  }
  const int incl = buf[src + t];
  *total = buf[src + TPB - 1];
  __syncthreads();
  return incl - v;
}

// One thread per pixel, one workgroup per TILE_W x TILE_H tile.  The patches are taken TPB at a time: each thread tests
// one against the tile, the hits are compacted IN PATCH ORDER into LDS (so the list has no limit), and every pixel walks
// that list and adds, in ascending patch index, A (B (s - m_s) - (t - m_t)) of every patch that covers it.
//   v_pred = upstream * mask * sum / n_corr        (0 where no patch covers the pixel)
__global__ __launch_bounds__(TPB) void local_pearson_bwd_kernel(const int H, const int W, const int box,
                                                                const int n_corr, const int tiles_x,
                                                                const float *__restrict__ upstream,
                                                                const float *__restrict__ pred,
                                                                const float *__restrict__ gt,
                                                                const float *__restrict__ mask,
                                                                const void *__restrict__ rows,
                                                                const void *__restrict__ cols, const int idx64,
                                                                const double *__restrict__ stats,
                                                                float *__restrict__ v_pred) {
  __shared__ int scan[2 * TPB];
  __shared__ int lr[TPB], lc[TPB];
  __shared__ double ls[TPB][4];
  const int t = threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int y0 = ty * TILE_H, x0 = tx * TILE_W;
  const int y = y0 + t / TILE_W, x = x0 + t % TILE_W;
  const bool live = y < H && x < W;
  const size_t k = (size_t)y * W + x;
  const double s = live ? masked(pred, mask, k) : 0.0, g = live ? masked(gt, mask, k) : 0.0;
  double acc = 0.0;
  for (int first = 0; first < n_corr; first += TPB) {
    const int p = first + t;
    int r = 0, c = 0;
    const bool hit = p < n_corr && patch_corner(rows, cols, idx64, p, H, W, box, r, c) && r < y0 + TILE_H &&
                     r + box > y0 && c < x0 + TILE_W && c + box > x0;
    int count;
    const int at = block_scan(hit ? 1 : 0, scan, &count);
    if (hit) {
      const double *__restrict__ st = stats + 5 * (size_t)p;
      lr[at] = r, lc[at] = c;
      ls[at][0] = st[0], ls[at][1] = st[1], ls[at][2] = st[2], ls[at][3] = st[3];
    }
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const int r_ = lr[j], c_ = lc[j];
      if (y >= r_ && y < r_ + box && x >= c_ && x < c_ + box)
        acc += ls[j][2] * (ls[j][3] * (s - ls[j][0]) - (g - ls[j][1]));
    }
    __syncthreads();  // (the list is rewritten by the next chunk)
  }
  if (live) {
    const double m = mask ? (double)mask[k] : 1.0;
    v_pred[k] = (float)((double)upstream[0] * m * (acc / (double)n_corr));
  }
}

// ---- scaled log-depth (edge-aware) ---------------------------------------------------------------------------------
// exp(-mean_c |img[y, x, c] - img[y2, x2, c]|) of two pixels of the [H,W,3] image
__device__ __forceinline__ double edge_weight(const float *__restrict__ img, size_t a, size_t b) {
  const double d = fabs((double)img[3 * a] - (double)img[3 * b]) + fabs((double)img[3 * a + 1] - (double)img[3 * b + 1]) +
                   fabs((double)img[3 * a + 2] - (double)img[3 * b + 2]);
  return exp(-d / 3.0);
}

// partial[2 b], partial[2 b + 1]: workgroup b's sums of lambda_x log(1 + |e|) over x < W - 1 and of lambda_y ... over
// y < H - 1, with e = scale * pred + shift - gt
__global__ __launch_bounds__(TPB) void log_depth_fwd_kernel(const int H, const int W, const float *__restrict__ pred,
                                                            const float *__restrict__ gt,
                                                            const float *__restrict__ img,
                                                            const float *__restrict__ scale_shift,
                                                            const float *__restrict__ mask,
                                                            double *__restrict__ partial) {
  __shared__ double red[TPB];
  const size_t n = (size_t)H * W;
  const double scale = (double)scale_shift[0], shift = (double)scale_shift[1];
  double ax = 0.0, ay = 0.0;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const double l = log(1.0 + fabs(scale * masked(pred, mask, i) + shift - masked(gt, mask, i)));
    if (x + 1 < W) ax += edge_weight(img, i, i + 1) * l;
    if (y + 1 < H) ay += edge_weight(img, i, i + W) * l;
  }
  ax = block_sum(ax, red);
  ay = block_sum(ay, red);
  if (threadIdx.x == 0) partial[2 * blockIdx.x] = ax, partial[2 * blockIdx.x + 1] = ay;
}

// loss = sum_x / count_x + sum_y / count_y, the counts H (W - 1) and (H - 1) W (0 / 0 where a count is 0: the mean of
// an empty tensor).  Shared by the log-depth and TV terms.
__global__ __launch_bounds__(TPB) void two_means_final_kernel(const int blocks, const double count_x,
                                                              const double count_y,
                                                              const double *__restrict__ partial,
                                                              float *__restrict__ loss_out) {
  __shared__ double red[TPB];
  double vx = 0.0, vy = 0.0;
  for (int b = threadIdx.x; b < blocks; b += TPB) vx += partial[2 * b], vy += partial[2 * b + 1];
  vx = block_sum(vx, red);
  vy = block_sum(vy, red);
  if (threadIdx.x == 0) *loss_out = (float)(vx / count_x + vy / count_y);
}

// v_pred = upstream * mask * scale * sgn(e) / (1 + |e|) * (lambda_x / (H (W - 1)) [x < W - 1] + lambda_y / ((H - 1) W) [y < H - 1])
__global__ __launch_bounds__(TPB) void log_depth_bwd_kernel(const int H, const int W,
                                                            const float *__restrict__ upstream,
                                                            const float *__restrict__ pred,
                                                            const float *__restrict__ gt,
                                                            const float *__restrict__ img,
                                                            const float *__restrict__ scale_shift,
                                                            const float *__restrict__ mask,
                                                            float *__restrict__ v_pred) {
  const size_t n = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
  const double scale = (double)scale_shift[0], shift = (double)scale_shift[1];
  const double e = scale * masked(pred, mask, i) + shift - masked(gt, mask, i);
  double w = 0.0;
  if (x + 1 < W) w += edge_weight(img, i, i + 1) / ((double)H * (double)(W - 1));
  if (y + 1 < H) w += edge_weight(img, i, i + W) / ((double)(H - 1) * (double)W);
  const double m = mask ? (double)mask[i] : 1.0;
  v_pred[i] = (float)((double)upstream[0] * m * (scale * sgn(e) / (1.0 + fabs(e)) * w));
}

// ---- total variation -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void tv_fwd_kernel(const int H, const int W, const float *__restrict__ pred,
                                                     const float *__restrict__ mask, double *__restrict__ partial) {
  __shared__ double red[TPB];
  const size_t n = (size_t)H * W;
  double ax = 0.0, ay = 0.0;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
    const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
    const double p = masked(pred, mask, i);
    if (x + 1 < W) ax += fabs(p - masked(pred, mask, i + 1));
    if (y + 1 < H) ay += fabs(p - masked(pred, mask, i + W));
  }
  ax = block_sum(ax, red);
  ay = block_sum(ay, red);
  if (threadIdx.x == 0) partial[2 * blockIdx.x] = ax, partial[2 * blockIdx.x + 1] = ay;
}

// v_pred = upstream * mask * ( (sgn(p - right) - sgn(left - p)) / (H (W - 1)) + (sgn(p - below) - sgn(above - p)) / ((H - 1) W) )
__global__ __launch_bounds__(TPB) void tv_bwd_kernel(const int H, const int W, const float *__restrict__ upstream,
                                                     const float *__restrict__ pred, const float *__restrict__ mask,
                                                     float *__restrict__ v_pred) {
  const size_t n = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
  const double p = masked(pred, mask, i);
  double sx = 0.0, sy = 0.0;
  if (x + 1 < W) sx += sgn(p - masked(pred, mask, i + 1));
  if (x > 0) sx -= sgn(masked(pred, mask, i - 1) - p);
  if (y + 1 < H) sy += sgn(p - masked(pred, mask, i + W));
  if (y > 0) sy -= sgn(masked(pred, mask, i - W) - p);
  double g = 0.0;
  if (W > 1) g += sx / ((double)H * (double)(W - 1));
  if (H > 1) g += sy / ((double)(H - 1) * (double)W);
  const double m = mask ? (double)mask[i] : 1.0;
  v_pred[i] = (float)((double)upstream[0] * m * g);
}

int check_shape(unsigned H, unsigned W, const char *who) {
  GSR_REQUIRE(H > 0 && W > 0 && (unsigned long long)H * W <= 0x7fffffffull, "%s: H * W must be in [1, 2^31)", who);
  return GSR_OK;
}
int check_patches(unsigned H, unsigned W, int box, int n_corr, const void *rows, const void *cols, const char *who) {
  GSR_REQUIRE(box >= 1 && (unsigned)box <= (H < W ? H : W), "%s: box_p must be in [1, min(H, W)]", who);
  GSR_REQUIRE(n_corr >= 0, "%s: n_corr must not be negative", who);
  GSR_REQUIRE(n_corr == 0 || (rows && cols), "%s: null patch corners", who);
  return GSR_OK;
}
int stream_blocks(size_t n) {
  const size_t want = (n + TPB - 1) / TPB;
  return (int)(want < (size_t)MAX_BLOCKS ? want : (size_t)MAX_BLOCKS);
}

}  // namespace

GSR_EXPORT int gsr_local_pearson_forward(unsigned img_height, unsigned img_width, int box_p, int n_corr,
                                         const float *pred, const float *gt, const float *mask, const void *rows,
                                         const void *cols, int index64, double *stats, float *loss_out,
                                         gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "local_pearson_forward")) return rc;
  if (int rc = check_patches(img_height, img_width, box_p, n_corr, rows, cols, "local_pearson_forward")) return rc;
  GSR_REQUIRE(pred && gt && loss_out && (n_corr == 0 || stats), "local_pearson_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_corr > 0) {
    hipLaunchKernelGGL(local_pearson_fwd_kernel, dim3((unsigned)n_corr), dim3(TPB), 0, s, (int)img_height,
                       (int)img_width, box_p, pred, gt, mask, rows, cols, index64, stats);
    GSR_CHECK_LAUNCH("local_pearson_forward");
  }
  hipLaunchKernelGGL(local_pearson_final_kernel, dim3(1), dim3(TPB), 0, s, n_corr, (const double *)stats, loss_out);
  GSR_CHECK_LAUNCH("local_pearson_final");
  return GSR_OK;
}

GSR_EXPORT int gsr_local_pearson_backward(unsigned img_height, unsigned img_width, int box_p, int n_corr,
                                          const float *upstream, const float *pred, const float *gt,
                                          const float *mask, const void *rows, const void *cols, int index64,
                                          const double *stats, float *v_pred, gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "local_pearson_backward")) return rc;
  if (int rc = check_patches(img_height, img_width, box_p, n_corr, rows, cols, "local_pearson_backward")) return rc;
  GSR_REQUIRE(upstream && pred && gt && v_pred && (n_corr == 0 || stats), "local_pearson_backward: null pointer");
  const unsigned tiles_x = gsr_cdiv(img_width, TILE_W), tiles_y = gsr_cdiv(img_height, TILE_H);
  hipLaunchKernelGGL(local_pearson_bwd_kernel, dim3(tiles_x * tiles_y), dim3(TPB), 0, (hipStream_t)stream,
                     (int)img_height, (int)img_width, box_p, n_corr, (int)tiles_x, upstream, pred, gt, mask, rows, cols,
                     index64, stats, v_pred);
  GSR_CHECK_LAUNCH("local_pearson_backward");
  return GSR_OK;
}

GSR_EXPORT int gsr_log_depth_forward(unsigned img_height, unsigned img_width, const float *pred, const float *gt,
                                     const float *image, const float *scale_shift, const float *mask, double *partial,
                                     float *loss_out, gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "log_depth_forward")) return rc;
  GSR_REQUIRE(pred && gt && image && scale_shift && partial && loss_out, "log_depth_forward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  const int blocks = stream_blocks(n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(log_depth_fwd_kernel, dim3(blocks), dim3(TPB), 0, s, (int)img_height, (int)img_width, pred, gt,
                     image, scale_shift, mask, partial);
  GSR_CHECK_LAUNCH("log_depth_forward");
  hipLaunchKernelGGL(two_means_final_kernel, dim3(1), dim3(TPB), 0, s, blocks,
                     (double)img_height * (double)(img_width - 1), (double)(img_height - 1) * (double)img_width,
                     (const double *)partial, loss_out);
  GSR_CHECK_LAUNCH("log_depth_final");
  return GSR_OK;
}

GSR_EXPORT int gsr_log_depth_backward(unsigned img_height, unsigned img_width, const float *upstream,
                                      const float *pred, const float *gt, const float *image,
                                      const float *scale_shift, const float *mask, float *v_pred,
                                      gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "log_depth_backward")) return rc;
  GSR_REQUIRE(upstream && pred && gt && image && scale_shift && v_pred, "log_depth_backward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  hipLaunchKernelGGL(log_depth_bwd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream,
                     (int)img_height, (int)img_width, upstream, pred, gt, image, scale_shift, mask, v_pred);
  GSR_CHECK_LAUNCH("log_depth_backward");
  return GSR_OK;
}

GSR_EXPORT int gsr_tv_forward(unsigned img_height, unsigned img_width, const float *pred, const float *mask,
                              double *partial, float *loss_out, gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "tv_forward")) return rc;
  GSR_REQUIRE(pred && partial && loss_out, "tv_forward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  const int blocks = stream_blocks(n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tv_fwd_kernel, dim3(blocks), dim3(TPB), 0, s, (int)img_height, (int)img_width, pred, mask,
                     partial);
  GSR_CHECK_LAUNCH("tv_forward");
  hipLaunchKernelGGL(two_means_final_kernel, dim3(1), dim3(TPB), 0, s, blocks,
                     (double)img_height * (double)(img_width - 1), (double)(img_height - 1) * (double)img_width,
                     (const double *)partial, loss_out);
  GSR_CHECK_LAUNCH("tv_final");
  return GSR_OK;
}

GSR_EXPORT int gsr_tv_backward(unsigned img_height, unsigned img_width, const float *upstream, const float *pred,
                               const float *mask, float *v_pred, gsr_stream_t stream) {
  if (int rc = check_shape(img_height, img_width, "tv_backward")) return rc;
  GSR_REQUIRE(upstream && pred && v_pred, "tv_backward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  hipLaunchKernelGGL(tv_bwd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream,
                     (int)img_height, (int)img_width, upstream, pred, mask, v_pred);
  GSR_CHECK_LAUNCH("tv_backward");
  return GSR_OK;
}
