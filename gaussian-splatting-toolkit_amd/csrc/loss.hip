// loss.hip -- fused photometric loss head  (1-lambda)*L1 + lambda*(1-SSIM)  and
// its gradient w.r.t. the rendered image (gfx950).   [SURVEY.md 8(f) row f2]
//
// What it replaces: GaussianSplattingModel.get_loss_dict
// (gs_toolkit/models/vanilla_gs.py:926-944): `torch.abs(gt - pred).mean()` and
// `1 - SSIM(data_range=1.0, size_average=True, channel=3)(gt, pred)` from the
// third-party package pytorch_msssim (pinned "1.0.0" in the reference's
// pyproject.toml:27; not vendored).  Its published algorithm, restated: 11-tap
// Gaussian window (sigma 1.5, normalised), separable, VALID padding (maps are
// (H-10) x (W-10)); mu1, mu2, E[x^2], E[y^2], E[xy]; sigma = E[..] - mu*mu;
// C1 = 0.01^2, C2 = 0.03^2;
//   S = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2)),
// mean over channels and positions.
//
// As torch ops this is 5 depthwise blurs (10 conv launches, MIOpen picks slow
// grouped-conv kernels: 2.3 ms forward + ~1.5 ms backward at 1080p, more than the
// whole rasterizer) plus ~20 elementwise kernels.  Here: ONE forward kernel
// (both images staged once per tile in LDS, the five blurs done separably from
// LDS, S and the three partial derivatives dS/dmu1, dS/dE[x^2], dS/dE[xy] written
// as planar maps, the two sums reduced to double atomics) and ONE backward kernel
// (transposed blur of the three maps + the L1 sign term -> d loss / d pred, which
// is exactly the `v_out_img` the compositing backward consumes).
#include <algorithm>

#include "gsr_common.h"

namespace {

constexpr int kWin = 11;
constexpr int kHalo = kWin - 1;
constexpr int kTW = 32, kTH = 16;                  // tile of outputs per workgroup
constexpr int kIW = kTW + kHalo, kIH = kTH + kHalo;  // staged inputs

// normalised 11-tap Gaussian, sigma = 1.5 (pytorch_msssim._fspecial_gauss_1d): the float32 values nearest to the
// exact weights (nine digits: their sum is 1 - 1.4e-9; a window that does not sum to 1 biases E[x^2] - mu^2 with one
// sign at every position).  The backward's transposed blur uses them.
__constant__ float kW[kWin] = {0.0010283801f, 0.007598758f, 0.036000773f, 0.10936069f, 0.21300554f,
                               0.26601171f,   0.21300554f,  0.10936069f,  0.036000773f, 0.007598758f,
                               0.0010283801f};
// The forward kernel forms the five window moments, S and its partial derivatives in double, with the exact
// normalised weights kWd: in float32, E[x^2] and E[xy] carry ~22 roundings of size eps32 mu^2, which do not shrink with
// the variance they are there to measure (flat backgrounds, ramps: variance <~ C2).  The inputs are float32, so their
// products are exact in double; the three maps are rounded to float32 once, on the store.  Measurements: DESIGN.md 4.4.
__constant__ double kWd[kWin] = {0.00102838008447911,  0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
                                 0.2130055377112537,   0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
                                 0.03600077212843083,  0.007598758135239185, 0.00102838008447911};
constexpr double kC1 = 0.01 * 0.01, kC2 = 0.03 * 0.03;

// The masked heads (kMasked) follow the models' `pred * mask`, `gt * mask` in front of the loss
// (vanilla_gs.py:915-924, surface_gs.py:917-925, depth_gs.py:424-437): the products are ROUNDED VALUES, as the
// torch multiplies leave them in memory.  Contracted into the subtraction that follows, `pred * m - gt * m` would
// be an fma on an unrounded product and sign(x - y) could differ from torch's where pred == gt.
__device__ __forceinline__ float mul_rounded(const float a, const float b) {
#pragma clang fp contract(off)
  return a * b;
}

// S and d S / d (mu1, E[x^2], E[xy]) (x = pred) at one position, from the five moments.  Every operation is rounded on
// its own and S is the oracle's expression A1 A2 / (B1 B2): with pred == gt the moments of x and y are the same bits,
// so A1 == B1 and A2 == B2 bit for bit, S is exactly 1 and the loss exactly 0, as in the reference.
__device__ __forceinline__ void ssim_point(const double mu1, const double mu2, const double e11, const double e22,
                                           const double e12, double &S, double &d_mu, double &d11, double &d12) {
#pragma clang fp contract(off)
  const double s11 = e11 - mu1 * mu1, s22 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
  const double A1 = 2.0 * mu1 * mu2 + kC1, A2 = 2.0 * s12 + kC2;
  const double B1 = mu1 * mu1 + mu2 * mu2 + kC1, B2 = s11 + s22 + kC2;
  const double den = B1 * B2;
  S = A1 * A2 / den;
  const double dA1 = A2 / den, dA2 = A1 / den, dB1 = -S / B1, dB2 = -S / B2;
  d_mu = dA1 * (2.0 * mu2) + dB1 * (2.0 * mu1) + dA2 * (-2.0 * mu2) + dB2 * (-2.0 * mu1);
  d11 = dB2;        // d S / d E[x^2]
  d12 = 2.0 * dA2;  // d S / d E[xy]
}

// img: [H,W,3] interleaved.  maps: [3 derivative kinds][3 channels][Hv][Wv] planar.
// sums[0] += sum |x-y| over the tile's own pixels, sums[1] += sum S over its valid outputs.
// clamp_pred: the prediction is min(pred, 1) (the models clamp the rendered image at 1
// before the loss, vanilla_gs.py:857 `torch.clamp(rgb, max=1.0)`; folding it in here
// saves that op and its three-kernel backward).
// kMasked: x = min(pred, 1) * m and y = gt * m with m = mask[H,W] (one value per pixel, any real number), formed
// here, in the staging loop -- one more global read per staged pixel, no LDS plane, nothing per blur tap; the
// divisors stay those of the whole image.  `mask` is not read otherwise.
template <bool kMasked>
__global__ __launch_bounds__(256) void l1_ssim_fwd_kernel(
    const int H, const int W, const float lambda, const int clamp_pred, const float *__restrict__ pred,
    const float *__restrict__ gt, const float *__restrict__ mask, float *__restrict__ maps,
    double *__restrict__ sums) {
  __shared__ float sx[kIH][kIW + 1], sy[kIH][kIW + 1];
  __shared__ double hb[5][kIH][kTW + 1];  // 34 KB (43 KB with sx, sy)
  __shared__ double red[2][4];

  const int Hv = H - kHalo, Wv = W - kHalo;
  const int c = blockIdx.z;
  const int ox = blockIdx.x * kTW, oy = blockIdx.y * kTH;
  const int tid = threadIdx.x;

  double l1 = 0.0;
  for (int i = tid; i < kIH * kIW; i += 256) {
    const int r = i / kIW, q = i % kIW;
    const int gy = oy + r, gx = ox + q;
    float x = 0.f, y = 0.f;
    if (gy < H && gx < W) {
      const size_t o = ((size_t)gy * W + gx) * 3 + c;
      x = pred[o];
      if (clamp_pred) x = fminf(x, 1.f);
      y = gt[o];
      if constexpr (kMasked) {
        const float m = mask[(size_t)gy * W + gx];
        x = mul_rounded(x, m);
        y = mul_rounded(y, m);
      }
      if (r < kTH && q < kTW) l1 += fabs((double)x - (double)y);  // every pixel belongs to exactly one tile
    }
    sx[r][q] = x;
    sy[r][q] = y;
  }
  __syncthreads();

  // horizontal pass of the five quantities
  for (int i = tid; i < kIH * kTW; i += 256) {
    const int r = i / kTW, q = i % kTW;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double x = sx[r][q + k], y = sy[r][q + k], w = kWd[k];
      a0 += w * x;
      a1 += w * y;
      a2 += w * (x * x);
      a3 += w * (y * y);
      a4 += w * (x * y);
    }
    hb[0][r][q] = a0;
    hb[1][r][q] = a1;
    hb[2][r][q] = a2;
    hb[3][r][q] = a3;
    hb[4][r][q] = a4;
  }
  __syncthreads();

  // vertical pass + SSIM and its partials: 512 outputs, 2 per lane
  double ssum = 0.0;
  const size_t plane = (size_t)Hv * Wv;
  for (int i = tid; i < kTH * kTW; i += 256) {
    const int r = i / kTW, q = i % kTW;
    const int gy = oy + r, gx = ox + q;
    if (gy >= Hv || gx >= Wv) continue;
    double mu1 = 0.0, mu2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const double w = kWd[k];
      mu1 += w * hb[0][r + k][q];
      mu2 += w * hb[1][r + k][q];
      e11 += w * hb[2][r + k][q];
      e22 += w * hb[3][r + k][q];
      e12 += w * hb[4][r + k][q];
    }
    double S, d_mu, d11, d12;
    ssim_point(mu1, mu2, e11, e22, e12, S, d_mu, d11, d12);
    ssum += S;
    const size_t o = (size_t)c * plane + (size_t)gy * Wv + gx;
    maps[o] = (float)d_mu;
    maps[3 * plane + o] = (float)d11;
    maps[6 * plane + o] = (float)d12;
  }

  // block reduction -> two double atomics
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    l1 += __shfl_xor(l1, o);
    ssum += __shfl_xor(ssum, o);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = l1;
    red[1][tid >> 6] = ssum;
  }
  __syncthreads();
  if (tid == 0) {
    // GSR_LOSS_SUM_SLOTS partial sums per quantity: 12 k workgroups adding doubles to the
    // same two addresses serialised in the L2 (that alone was ~250 us of this kernel)
    const unsigned linear = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const unsigned slot = linear % GSR_LOSS_SUM_SLOTS;
    atomicAdd(&sums[slot], red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    atomicAdd(&sums[GSR_LOSS_SUM_SLOTS + slot], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}

// The partial sums -> the three scalars.  A separate one-wave launch: doing it in the
// workgroup that finishes last needs an agent-scope release fence in every workgroup,
// and on gfx950 that fence writes the XCD's whole L2 back (measured: 80 -> 520 us).
__global__ __launch_bounds__(64) void l1_ssim_finalize_kernel(const int H, const int W, const float lambda,
                                                              const double *__restrict__ sums,
                                                              float *__restrict__ loss_out,
                                                              float *__restrict__ terms_out) {
  const int tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int k = tid; k < GSR_LOSS_SUM_SLOTS; k += 64) {
    a += sums[k];
    b += sums[GSR_LOSS_SUM_SLOTS + k];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o);
    b += __shfl_xor(b, o);
  }
  if (tid == 0) {
    const double l1m = a / (3.0 * (double)H * (double)W);
    const double ssm = b / (3.0 * (double)(H - kHalo) * (double)(W - kHalo));
    *loss_out = (float)((1.0 - (double)lambda) * l1m + (double)lambda * (1.0 - ssm));
    if (terms_out) {
      terms_out[0] = (float)l1m;
      terms_out[1] = (float)ssm;
    }
  }
}

// v_pred = up * [ (1-lambda) sign(x-y)/(3HW) - lambda/(3 Hv Wv) * ( blurT(Dmu) + 2x blurT(D11) + y blurT(D12) ) ]
// kMasked: the same expression in x = min(pred, 1) * m and y = gt * m, times m (d x / d pred) at the end.
template <bool kMasked>
__global__ __launch_bounds__(256) void l1_ssim_bwd_kernel(
    const int H, const int W, const float lambda, const int clamp_pred, const float *__restrict__ upstream,
    const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ mask,
    const float *__restrict__ maps, float *__restrict__ v_pred) {
  __shared__ float sm[3][kIH][kIW + 1];
  __shared__ float hb[3][kIH][kTW + 1];

  const int Hv = H - kHalo, Wv = W - kHalo;
  const int c = blockIdx.z;
  const int ox = blockIdx.x * kTW, oy = blockIdx.y * kTH;  // tile of image pixels
  const int tid = threadIdx.x;
  const size_t plane = (size_t)Hv * Wv;

  // map entries (i-k, j-l), k,l in [0,10]  ->  rows oy-10 .. oy+15, cols ox-10 .. ox+31
  for (int i = tid; i < kIH * kIW; i += 256) {
    const int r = i / kIW, q = i % kIW;
    const int my = oy - kHalo + r, mx = ox - kHalo + q;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (my >= 0 && my < Hv && mx >= 0 && mx < Wv) {
      const size_t o = (size_t)c * plane + (size_t)my * Wv + mx;
      d0 = maps[o];
      d1 = maps[3 * plane + o];
      d2 = maps[6 * plane + o];
    }
    sm[0][r][q] = d0;
    sm[1][r][q] = d1;
    sm[2][r][q] = d2;
  }
  __syncthreads();
  // pixel column j gathers map columns j-l with weight w[l]: staged index q + kHalo - l
  for (int i = tid; i < kIH * kTW; i += 256) {
    const int r = i / kTW, q = i % kTW;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int l = 0; l < kWin; ++l) {
      const float w = kW[l];
      a0 += w * sm[0][r][q + kHalo - l];
      a1 += w * sm[1][r][q + kHalo - l];
      a2 += w * sm[2][r][q + kHalo - l];
    }
    hb[0][r][q] = a0;
    hb[1][r][q] = a1;
    hb[2][r][q] = a2;
  }
  __syncthreads();
  const float up = upstream[0];
  const float k_l1 = up * (1.f - lambda) / (3.f * (float)H * (float)W);
  const float k_ss = -up * lambda / (3.f * (float)Hv * (float)Wv);
  for (int i = tid; i < kTH * kTW; i += 256) {
    const int r = i / kTW, q = i % kTW;
    const int gy = oy + r, gx = ox + q;
    if (gy >= H || gx >= W) continue;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f;
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
      const float w = kW[k];
      g0 += w * hb[0][r + kHalo - k][q];
      g1 += w * hb[1][r + kHalo - k][q];
      g2 += w * hb[2][r + kHalo - k][q];
    }
    const size_t o = ((size_t)gy * W + gx) * 3 + c;
    const float xr = pred[o];
    float y = gt[o];
    float x = clamp_pred ? fminf(xr, 1.f) : xr;
    float m = 1.f;
    if constexpr (kMasked) {
      m = mask[(size_t)gy * W + gx];
      x = mul_rounded(x, m);
      y = mul_rounded(y, m);
    }
    const float d = x - y;
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    float g = k_l1 * sgn + k_ss * (g0 + 2.f * x * g1 + y * g2);
    if constexpr (kMasked) g = mul_rounded(m, g);
    v_pred[o] = (clamp_pred && xr > 1.f) ? 0.f : g;  // clamp(max=1) passes the gradient where pred <= 1
  }
}

}  // namespace

namespace {

// mask == nullptr: the unmasked kernels
int l1_ssim_forward_launch(unsigned img_height, unsigned img_width, float ssim_lambda, int clamp_pred,
                           const float *pred, const float *gt, const float *mask, float *maps, double *sums,
                           float *loss_out, float *terms_out, hipStream_t s) {
  if (int zrc = gsr_zero_async(sums, GSR_LOSS_WORKSPACE_DOUBLES * sizeof(double), s)) return zrc;
  const dim3 grd(gsr_cdiv(img_width, kTW), gsr_cdiv(img_height, kTH), 3);
  if (mask)
    hipLaunchKernelGGL(l1_ssim_fwd_kernel<true>, grd, dim3(256), 0, s, (int)img_height, (int)img_width, ssim_lambda,
                       clamp_pred, pred, gt, mask, maps, sums);
  else
    hipLaunchKernelGGL(l1_ssim_fwd_kernel<false>, grd, dim3(256), 0, s, (int)img_height, (int)img_width, ssim_lambda,
                       clamp_pred, pred, gt, mask, maps, sums);
  hipLaunchKernelGGL(l1_ssim_finalize_kernel, dim3(1), dim3(64), 0, s, (int)img_height, (int)img_width,
                     ssim_lambda, (const double *)sums, loss_out, terms_out);
  return GSR_OK;
}

void l1_ssim_backward_launch(unsigned img_height, unsigned img_width, float ssim_lambda, int clamp_pred,
                             const float *upstream, const float *pred, const float *gt, const float *mask,
                             const float *maps, float *v_pred, hipStream_t s) {
  const dim3 grd(gsr_cdiv(img_width, kTW), gsr_cdiv(img_height, kTH), 3);
  if (mask)
    hipLaunchKernelGGL(l1_ssim_bwd_kernel<true>, grd, dim3(256), 0, s, (int)img_height, (int)img_width, ssim_lambda,
                       clamp_pred, upstream, pred, gt, mask, maps, v_pred);
  else
    hipLaunchKernelGGL(l1_ssim_bwd_kernel<false>, grd, dim3(256), 0, s, (int)img_height, (int)img_width, ssim_lambda,
                       clamp_pred, upstream, pred, gt, mask, maps, v_pred);
}

}  // namespace

GSR_EXPORT int gsr_l1_ssim_forward(unsigned img_height, unsigned img_width, float ssim_lambda,
                                   int clamp_pred, const float *pred, const float *gt, float *maps,
                                   double *sums, float *loss_out, float *terms_out, gsr_stream_t stream) {
  GSR_REQUIRE(img_height > kHalo && img_width > kHalo, "l1_ssim_forward: image must be larger than 10x10");
  GSR_REQUIRE(pred && gt && maps && sums && loss_out, "l1_ssim_forward: null pointer");
  if (int rc = l1_ssim_forward_launch(img_height, img_width, ssim_lambda, clamp_pred, pred, gt, nullptr, maps, sums,
                                      loss_out, terms_out, (hipStream_t)stream))
    return rc;
  GSR_CHECK_LAUNCH("l1_ssim_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_l1_ssim_masked_forward(unsigned img_height, unsigned img_width, float ssim_lambda,
                                          int clamp_pred, const float *pred, const float *gt, const float *mask,
                                          float *maps, double *sums, float *loss_out, float *terms_out,
                                          gsr_stream_t stream) {
  GSR_REQUIRE(img_height > kHalo && img_width > kHalo, "l1_ssim_masked_forward: image must be larger than 10x10");
  GSR_REQUIRE(pred && gt && mask && maps && sums && loss_out, "l1_ssim_masked_forward: null pointer");
  if (int rc = l1_ssim_forward_launch(img_height, img_width, ssim_lambda, clamp_pred, pred, gt, mask, maps, sums,
                                      loss_out, terms_out, (hipStream_t)stream))
    return rc;
  GSR_CHECK_LAUNCH("l1_ssim_masked_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_l1_ssim_backward(unsigned img_height, unsigned img_width, float ssim_lambda,
                                    int clamp_pred, const float *upstream, const float *pred, const float *gt,
                                    const float *maps, float *v_pred, gsr_stream_t stream) {
  GSR_REQUIRE(img_height > kHalo && img_width > kHalo, "l1_ssim_backward: image must be larger than 10x10");
  GSR_REQUIRE(upstream && pred && gt && maps && v_pred, "l1_ssim_backward: null pointer");
  l1_ssim_backward_launch(img_height, img_width, ssim_lambda, clamp_pred, upstream, pred, gt, nullptr, maps, v_pred,
                          (hipStream_t)stream);
  GSR_CHECK_LAUNCH("l1_ssim_backward");
  return GSR_OK;
}

GSR_EXPORT int gsr_l1_ssim_masked_backward(unsigned img_height, unsigned img_width, float ssim_lambda,
                                           int clamp_pred, const float *upstream, const float *pred,
                                           const float *gt, const float *mask, const float *maps, float *v_pred,
                                           gsr_stream_t stream) {
  GSR_REQUIRE(img_height > kHalo && img_width > kHalo, "l1_ssim_masked_backward: image must be larger than 10x10");
  GSR_REQUIRE(upstream && pred && gt && mask && maps && v_pred, "l1_ssim_masked_backward: null pointer");
  l1_ssim_backward_launch(img_height, img_width, ssim_lambda, clamp_pred, upstream, pred, gt, mask, maps, v_pred,
                          (hipStream_t)stream);
  GSR_CHECK_LAUNCH("l1_ssim_masked_backward");
  return GSR_OK;
}

// ---- L1-only photometric head: what DepthGSModel's `main_loss` really is --------
// depth_gs.py:445-448 reads
//     loss_dict["main_loss"] = (1 - self.config.ssim_lambda) * Ll1
//     +self.config.ssim_lambda * simloss
// -- the second line is a stand-alone expression statement, so the SSIM term is computed
// and thrown away: the co-gs photometric loss is  weight * mean |gt - pred|  with
// weight = 1 - ssim_lambda.  One streaming kernel each way, no maps, no blur.
namespace {

// kMasked: element e of the interleaved [H,W,3] image belongs to pixel e / 3.  The float4 at elements 4i .. 4i+3
// starts in pixel p = 4i / 3 at channel r = 4i - 3p and always ends in pixel p + 1 (r + 3 >= 3, r + 3 < 6): two
// mask reads, element k takes the second one from k >= 3 - r on.  p + 1 holds element 4i + 3 < n: in bounds.
template <bool kMasked>
__global__ __launch_bounds__(256) void l1_fwd_kernel(const long long n4, const long long n, const int clamp_pred,
                                                     const float *__restrict__ pred, const float *__restrict__ gt,
                                                     const float *__restrict__ mask, double *__restrict__ sums) {
  __shared__ float red[4];
  float acc = 0.f;
  const float4 *p4 = reinterpret_cast<const float4 *>(pred);
  const float4 *g4 = reinterpret_cast<const float4 *>(gt);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 x = p4[i];
    float4 y = g4[i];
    if (clamp_pred) {
      x.x = fminf(x.x, 1.f);
      x.y = fminf(x.y, 1.f);
      x.z = fminf(x.z, 1.f);
      x.w = fminf(x.w, 1.f);
    }
    if constexpr (kMasked) {
      const long long p = (4 * i) / 3;
      const int r = (int)(4 * i - 3 * p);
      const float m0 = mask[p], m1 = mask[p + 1];
      const float mx = m0, my = r < 2 ? m0 : m1, mz = r < 1 ? m0 : m1, mw = m1;
      x.x = mul_rounded(x.x, mx), y.x = mul_rounded(y.x, mx);
      x.y = mul_rounded(x.y, my), y.y = mul_rounded(y.y, my);
      x.z = mul_rounded(x.z, mz), y.z = mul_rounded(y.z, mz);
      x.w = mul_rounded(x.w, mw), y.w = mul_rounded(y.w, mw);
    }
    acc += (fabsf(x.x - y.x) + fabsf(x.y - y.y)) + (fabsf(x.z - y.z) + fabsf(x.w - y.w));
  }
  if (blockIdx.x == 0) {  // the (at most three) elements behind the last float4
    const long long i = 4 * n4 + threadIdx.x;
    if (i < n) {
      float x = clamp_pred ? fminf(pred[i], 1.f) : pred[i];
      float y = gt[i];
      if constexpr (kMasked) {
        const float m = mask[i / 3];
        x = mul_rounded(x, m);
        y = mul_rounded(y, m);
      }
      acc += fabsf(x - y);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(&sums[blockIdx.x % GSR_LOSS_SUM_SLOTS], (double)red[0] + red[1] + red[2] + red[3]);
}

__global__ __launch_bounds__(64) void l1_finalize_kernel(const long long n, const float weight,
                                                         const double *__restrict__ sums,
                                                         float *__restrict__ loss_out) {
  double a = 0.0;
  for (int k = threadIdx.x; k < GSR_LOSS_SUM_SLOTS; k += 64) a += sums[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if (threadIdx.x == 0) *loss_out = (float)((double)weight * (a / (double)n));
}

template <bool kMasked>
__global__ __launch_bounds__(256) void l1_bwd_kernel(const long long n, const float weight, const int clamp_pred,
                                                     const float *__restrict__ upstream,
                                                     const float *__restrict__ pred, const float *__restrict__ gt,
                                                     const float *__restrict__ mask, float *__restrict__ v_pred) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float xr = pred[i];
  float x = clamp_pred ? fminf(xr, 1.f) : xr;
  float y = gt[i];
  float m = 1.f;
  if constexpr (kMasked) {
    m = mask[i / 3];
    x = mul_rounded(x, m);
    y = mul_rounded(y, m);
  }
  const float d = x - y;
  const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  const float k = upstream[0] * weight / (float)n;
  float g = k * sgn;
  if constexpr (kMasked) g = mul_rounded(m, g);
  v_pred[i] = (clamp_pred && xr > 1.f) ? 0.f : g;
}

}  // namespace

namespace {

int l1_forward_launch(long long num_values, float weight, int clamp_pred, const float *pred, const float *gt,
                      const float *mask, double *sums, float *loss_out, hipStream_t s) {
  if (int zrc = gsr_zero_async(sums, GSR_LOSS_SUM_SLOTS * sizeof(double), s)) return zrc;
  const long long n4 = num_values / 4;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min<long long>((n4 + 1023) / 1024, 4096));
  if (mask)
    hipLaunchKernelGGL(l1_fwd_kernel<true>, dim3(blocks), dim3(256), 0, s, n4, num_values, clamp_pred, pred, gt, mask,
                       sums);
  else
    hipLaunchKernelGGL(l1_fwd_kernel<false>, dim3(blocks), dim3(256), 0, s, n4, num_values, clamp_pred, pred, gt, mask,
                       sums);
  hipLaunchKernelGGL(l1_finalize_kernel, dim3(1), dim3(64), 0, s, num_values, weight, (const double *)sums,
                     loss_out);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT int gsr_l1_forward(long long num_values, float weight, int clamp_pred, const float *pred,
                              const float *gt, double *sums, float *loss_out, gsr_stream_t stream) {
  GSR_REQUIRE(num_values > 0, "l1_forward: empty image");
  GSR_REQUIRE(pred && gt && sums && loss_out, "l1_forward: null pointer");
  GSR_REQUIRE(((uintptr_t)pred & 15) == 0 && ((uintptr_t)gt & 15) == 0, "l1_forward: images must be 16-byte aligned");
  if (int rc = l1_forward_launch(num_values, weight, clamp_pred, pred, gt, nullptr, sums, loss_out,
                                 (hipStream_t)stream))
    return rc;
  GSR_CHECK_LAUNCH("l1_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_l1_masked_forward(long long num_values, float weight, int clamp_pred, const float *pred,
                                     const float *gt, const float *mask, double *sums, float *loss_out,
                                     gsr_stream_t stream) {
  GSR_REQUIRE(num_values > 0 && num_values % 3 == 0, "l1_masked_forward: expected an [H,W,3] image");
  GSR_REQUIRE(pred && gt && mask && sums && loss_out, "l1_masked_forward: null pointer");
  GSR_REQUIRE(((uintptr_t)pred & 15) == 0 && ((uintptr_t)gt & 15) == 0,
              "l1_masked_forward: images must be 16-byte aligned");
  if (int rc = l1_forward_launch(num_values, weight, clamp_pred, pred, gt, mask, sums, loss_out, (hipStream_t)stream))
    return rc;
  GSR_CHECK_LAUNCH("l1_masked_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_l1_backward(long long num_values, float weight, int clamp_pred, const float *upstream,
                               const float *pred, const float *gt, float *v_pred, gsr_stream_t stream) {
  GSR_REQUIRE(num_values > 0, "l1_backward: empty image");
  GSR_REQUIRE(upstream && pred && gt && v_pred, "l1_backward: null pointer");
  hipLaunchKernelGGL(l1_bwd_kernel<false>, dim3((unsigned)((num_values + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, num_values, weight, clamp_pred, upstream, pred, gt, (const float *)nullptr,
                     v_pred);
  GSR_CHECK_LAUNCH("l1_backward");
  return GSR_OK;
}

GSR_EXPORT int gsr_l1_masked_backward(long long num_values, float weight, int clamp_pred, const float *upstream,
                                      const float *pred, const float *gt, const float *mask, float *v_pred,
                                      gsr_stream_t stream) {
  GSR_REQUIRE(num_values > 0 && num_values % 3 == 0, "l1_masked_backward: expected an [H,W,3] image");
  GSR_REQUIRE(upstream && pred && gt && mask && v_pred, "l1_masked_backward: null pointer");
  hipLaunchKernelGGL(l1_bwd_kernel<true>, dim3((unsigned)((num_values + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, num_values, weight, clamp_pred, upstream, pred, gt, mask, v_pred);
  GSR_CHECK_LAUNCH("l1_masked_backward");
  return GSR_OK;
}

// ---- depth head of the co-gs model (DepthGSModel, gs_toolkit/models/depth_gs.py) --
//   pred  = where(alpha > 0, depth / alpha, depth.detach().max())      (:356-363)
//   loss  = | gt * (gt > 0) - pred * (gt > 0) |.mean()                   (:531-538)
// as one kernel forward (+ the one-wave sum) and one backward that writes the
// cotangents of the two compositing passes' outputs (accumulated depth, alpha)
// directly -- ~8 elementwise / indexing launches forward and ~10 backward otherwise.
namespace {

// kMasked (depth_gs.py:424-437 in front of :531-538): g' = gt * m, p' = pred * m, the measured pixels are those
// with g' > 0 and the loss is mean |g' - p'| over them; the cotangent of pred is m * sign(p' - g') / n.
template <bool kMasked>
__global__ __launch_bounds__(256) void depth_l1_fwd_kernel(const long long n, const float *__restrict__ depth,
                                                           const float *__restrict__ alpha,
                                                           const float *__restrict__ gt,
                                                           const float *__restrict__ mask,
                                                           const float *__restrict__ depth_max,
                                                           double *__restrict__ sums) {
  __shared__ float red[4];
  const float far = *depth_max;
  float acc = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float a = alpha[i];
    float g = gt[i];
    float pred = a > 0.f ? depth[i] / a : far;
    if constexpr (kMasked) {
      const float m = mask[i];
      g = mul_rounded(g, m);
      pred = mul_rounded(pred, m);
    }
    acc += g > 0.f ? fabsf(g - pred) : 0.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(&sums[blockIdx.x % GSR_LOSS_SUM_SLOTS], (double)red[0] + red[1] + red[2] + red[3]);
}

__global__ __launch_bounds__(64) void depth_l1_finalize_kernel(const long long n, const double *__restrict__ sums,
                                                               float *__restrict__ loss_out) {
  double a = 0.0;
  for (int k = threadIdx.x; k < GSR_LOSS_SUM_SLOTS; k += 64) a += sums[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  if (threadIdx.x == 0) *loss_out = (float)(a / (double)n);
}

template <bool kMasked>
__global__ __launch_bounds__(256) void depth_l1_bwd_kernel(const long long n, const float *__restrict__ upstream,
                                                           const float *__restrict__ depth,
                                                           const float *__restrict__ alpha,
                                                           const float *__restrict__ gt,
                                                           const float *__restrict__ mask,
                                                           const float *__restrict__ depth_max,
                                                           float *__restrict__ v_depth, float *__restrict__ v_alpha) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float a = alpha[i], d = depth[i];
  float g = gt[i], m = 1.f;
  if constexpr (kMasked) {
    m = mask[i];
    g = mul_rounded(g, m);
  }
  float vd = 0.f, va = 0.f;
  if (a > 0.f && g > 0.f) {  // the far value of uncovered pixels is detached
    const float inv = 1.f / a;
    const float pred = d * inv;
    const float pm = kMasked ? mul_rounded(pred, m) : pred;
    const float s = pm > g ? 1.f : (pm < g ? -1.f : 0.f);
    float vp = upstream[0] * s / (float)n;
    if constexpr (kMasked) vp = mul_rounded(vp, m);
    vd = vp * inv;
    va = -vp * pred * inv;
  }
  v_depth[i] = vd;
  v_alpha[i] = va;
}

}  // namespace

GSR_EXPORT int gsr_depth_l1_forward(long long num_pixels, const float *depth, const float *alpha, const float *gt,
                                    const float *depth_max, double *sums, float *loss_out, gsr_stream_t stream) {
  GSR_REQUIRE(num_pixels > 0, "depth_l1_forward: empty image");
  GSR_REQUIRE(depth && alpha && gt && depth_max && sums && loss_out, "depth_l1_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = gsr_zero_async(sums, GSR_LOSS_SUM_SLOTS * sizeof(double), s)) return zrc;
  const unsigned blocks = (unsigned)std::min<long long>((num_pixels + 1023) / 1024, 4096);
  hipLaunchKernelGGL(depth_l1_fwd_kernel<false>, dim3(blocks), dim3(256), 0, s, num_pixels, depth, alpha, gt,
                     (const float *)nullptr, depth_max, sums);
  hipLaunchKernelGGL(depth_l1_finalize_kernel, dim3(1), dim3(64), 0, s, num_pixels, (const double *)sums, loss_out);
  GSR_CHECK_LAUNCH("depth_l1_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_depth_l1_masked_forward(long long num_pixels, const float *depth, const float *alpha,
                                           const float *gt, const float *mask, const float *depth_max, double *sums,
                                           float *loss_out, gsr_stream_t stream) {
  GSR_REQUIRE(num_pixels > 0, "depth_l1_masked_forward: empty image");
  GSR_REQUIRE(depth && alpha && gt && mask && depth_max && sums && loss_out, "depth_l1_masked_forward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (int zrc = gsr_zero_async(sums, GSR_LOSS_SUM_SLOTS * sizeof(double), s)) return zrc;
  const unsigned blocks = (unsigned)std::min<long long>((num_pixels + 1023) / 1024, 4096);
  hipLaunchKernelGGL(depth_l1_fwd_kernel<true>, dim3(blocks), dim3(256), 0, s, num_pixels, depth, alpha, gt, mask,
                     depth_max, sums);
  hipLaunchKernelGGL(depth_l1_finalize_kernel, dim3(1), dim3(64), 0, s, num_pixels, (const double *)sums, loss_out);
  GSR_CHECK_LAUNCH("depth_l1_masked_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_depth_l1_backward(long long num_pixels, const float *upstream, const float *depth,
                                     const float *alpha, const float *gt, const float *depth_max, float *v_depth,
                                     float *v_alpha, gsr_stream_t stream) {
  GSR_REQUIRE(num_pixels > 0, "depth_l1_backward: empty image");
  GSR_REQUIRE(upstream && depth && alpha && gt && depth_max && v_depth && v_alpha, "depth_l1_backward: null pointer");
  hipLaunchKernelGGL(depth_l1_bwd_kernel<false>, dim3((unsigned)((num_pixels + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, num_pixels, upstream, depth, alpha, gt, (const float *)nullptr, depth_max,
                     v_depth, v_alpha);
  GSR_CHECK_LAUNCH("depth_l1_backward");
  return GSR_OK;
}

GSR_EXPORT int gsr_depth_l1_masked_backward(long long num_pixels, const float *upstream, const float *depth,
                                            const float *alpha, const float *gt, const float *mask,
                                            const float *depth_max, float *v_depth, float *v_alpha,
                                            gsr_stream_t stream) {
  GSR_REQUIRE(num_pixels > 0, "depth_l1_masked_backward: empty image");
  GSR_REQUIRE(upstream && depth && alpha && gt && mask && depth_max && v_depth && v_alpha,
              "depth_l1_masked_backward: null pointer");
  hipLaunchKernelGGL(depth_l1_bwd_kernel<true>, dim3((unsigned)((num_pixels + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, num_pixels, upstream, depth, alpha, gt, mask, depth_max, v_depth, v_alpha);
  GSR_CHECK_LAUNCH("depth_l1_masked_backward");
  return GSR_OK;
}
