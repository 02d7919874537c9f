// bilagrid.hip -- per-view bilateral grids: appearance compensation between the render and the loss heads (DESIGN.md
// section 4.18; the rule is stated in include/gsraster.h).  What it replaces as torch ops: F.grid_sample over a
// [1,12,L,Gh,Gw] volume + the 3x4 affine map, whose backward (grid_sampler_3d_backward) scatters 96 values per pixel
// into the grid with float atomics.  Here:
//   forward   one thread per pixel, the 8 corners read as three 16-byte loads each (channel-last storage)
//   backward  v_rgb: one thread per pixel (the slice recomputed, plus d/dz for the path through the guide);
//             v_A:   a GATHER per grid vertex.  The xy weights of a pixel are a fixed function of its position, so the
//                    pixels that reach vertex (gx, gy) form a rectangle.  One workgroup per (vertex, strip of the
//                    rectangle's rows) stages 256 pixels at a time in LDS -- z level, the two z-weighted xy weights,
//                    the 12 products v_out[r] * (r, g, b, 1)[k] -- and thread (level, channel) walks them serially in
//                    pixel order, summing in float64.  A second launch adds the strips in ascending order and writes
//                    EVERY element of v_A (zeros for the other views and for vertices no pixel reaches).
// No atomics, no memset; two runs are bit-equal.  Per-pixel arithmetic float32, every cross-pixel sum float64.
#include "gsr_common.h"

namespace {

constexpr int TPB = 256;
constexpr int CH = GSR_BILAGRID_CHANNELS;
constexpr int TV_MAX_BLOCKS = GSR_BILAGRID_TV_WORKSPACE_DOUBLES / 3;

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

// pixel p of n along an image axis -> the lower vertex i0 in [0, G - 2] and the fraction f in [0, 1) of
// (p + 0.5) / n * (G - 1).  One function for the forward, the backward and the vertex gather: they agree on a
// pixel's cell bit for bit.
__device__ __forceinline__ void axis_coord(const int p, const int n, const int G, int &i0, float &f) {
  const float ix = __fdiv_rn((float)p + 0.5f, (float)n) * (float)(G - 1);
  i0 = min((int)ix, G - 2);
  f = ix - (float)i0;
}

// the guide -> level z0 in [0, L - 2], fraction fz in [0, 1]; false where the guide is clamped (no gradient through it)
__device__ __forceinline__ bool guide_coord(const float r, const float g, const float b, const int L, int &z0,
                                            float &fz) {
  const float gd = 0.299f * r + 0.587f * g + 0.114f * b;
  const float iz = fminf(fmaxf(gd, 0.f), 1.f) * (float)(L - 1);  // (NaN -> 0)
  z0 = min((int)iz, L - 2);
  fz = iz - (float)z0;
  return gd > 0.f && gd < 1.f;
}

__device__ __forceinline__ void load12(const float *__restrict__ p, float *a) {
  const float4 *q = reinterpret_cast<const float4 *>(p);
  const float4 u = q[0], v = q[1], w = q[2];
  a[0] = u.x, a[1] = u.y, a[2] = u.z, a[3] = u.w, a[4] = v.x, a[5] = v.y, a[6] = v.z, a[7] = v.w;
  a[8] = w.x, a[9] = w.y, a[10] = w.z, a[11] = w.w;
}

// the bilinear interpolation of one level: a + f (b - a) along x, then along y (a constant grid comes back exactly)
__device__ __forceinline__ void level_at(const float *__restrict__ level, const int Gw, const int x0, const int y0,
                                         const float fx, const float fy, float *m) {
  const float *p = level + ((size_t)y0 * Gw + (size_t)x0) * CH;
  float a[CH], b[CH], top[CH];
  load12(p, a);
  load12(p + CH, b);
#pragma unroll
  for (int c = 0; c < CH; ++c) top[c] = fmaf(fx, b[c] - a[c], a[c]);
  load12(p + (size_t)Gw * CH, a);
  load12(p + (size_t)Gw * CH + CH, b);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float bot = fmaf(fx, b[c] - a[c], a[c]);
    m[c] = fmaf(fy, bot - top[c], top[c]);
  }
}

// M = trilinear interpolation of the view's grid, and dMz = d M / d iz: the difference of the two levels' bilinear
// interpolations
__device__ __forceinline__ void slice_at(const float *__restrict__ grid, const int Gw, const int Gh, const int x0,
                                         const int y0, const int z0, const float fx, const float fy, const float fz,
                                         float *M, float *dMz) {
  float m0[CH];
  level_at(grid + (size_t)z0 * Gh * Gw * CH, Gw, x0, y0, fx, fy, m0);
  level_at(grid + (size_t)(z0 + 1) * Gh * Gw * CH, Gw, x0, y0, fx, fy, M);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    dMz[c] = M[c] - m0[c];
    M[c] = fmaf(fz, dMz[c], m0[c]);
  }
}

__global__ __launch_bounds__(TPB) void slice_fwd_kernel(const int H, const int W, const int Gw, const int Gh,
                                                        const int L, const float *__restrict__ grid,
                                                        const float *__restrict__ rgb, float *__restrict__ out) {
  const size_t n = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int py = (int)(i / W), px = (int)(i - (size_t)py * W);
  const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
  int x0, y0, z0;
  float fx, fy, fz;
  axis_coord(px, W, Gw, x0, fx);
  axis_coord(py, H, Gh, y0, fy);
  guide_coord(r, g, b, L, z0, fz);
  float M[CH], dMz[CH];
  slice_at(grid, Gw, Gh, x0, y0, z0, fx, fy, fz, M, dMz);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    out[3 * i + k] = fmaf(M[4 * k], r, fmaf(M[4 * k + 1], g, fmaf(M[4 * k + 2], b, M[4 * k + 3])));
}

// v_rgb[c] = sum_r M[r][c] v_out[r] + [0 < guide < 1] (L - 1) guide_weight[c] sum_r v_out[r] (dMz[r] . (r, g, b, 1))
__global__ __launch_bounds__(TPB) void slice_bwd_rgb_kernel(const int H, const int W, const int Gw, const int Gh,
                                                            const int L, const float *__restrict__ grid,
                                                            const float *__restrict__ rgb,
                                                            const float *__restrict__ v_out,
                                                            float *__restrict__ v_rgb) {
  const size_t n = (size_t)H * W;
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int py = (int)(i / W), px = (int)(i - (size_t)py * W);
  const float r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
  const float vo[3] = {v_out[3 * i], v_out[3 * i + 1], v_out[3 * i + 2]};
  int x0, y0, z0;
  float fx, fy, fz;
  axis_coord(px, W, Gw, x0, fx);
  axis_coord(py, H, Gh, y0, fy);
  const bool inside = guide_coord(r, g, b, L, z0, fz);
  float M[CH], dMz[CH];
  slice_at(grid, Gw, Gh, x0, y0, z0, fx, fy, fz, M, dMz);
  float t = 0.f;
  if (inside) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      t = fmaf(vo[k], fmaf(dMz[4 * k], r, fmaf(dMz[4 * k + 1], g, fmaf(dMz[4 * k + 2], b, dMz[4 * k + 3]))), t);
    t *= (float)(L - 1);
  }
  const float gw[3] = {0.299f, 0.587f, 0.114f};
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v_rgb[3 * i + c] = fmaf(gw[c], t, fmaf(M[c], vo[0], fmaf(M[4 + c], vo[1], M[8 + c] * vo[2])));
}

// the pixels p of an axis of n that can reach vertex gv of G: [lo, hi), one pixel of slack on either side (a pixel
// inside the range that does not reach the vertex gets weight 0 from its own axis_coord)
__device__ __forceinline__ void vertex_range(const int gv, const int n, const int G, int &lo, int &hi) {
  const long long a = gv > 0 ? (long long)(gv - 1) * n / (G - 1) - 1 : 0;
  const long long b = ((long long)(gv + 1) * n + (G - 2)) / (G - 1) + 1;
  lo = (int)(a > 0 ? a : 0);
  hi = (int)(b < n ? b : n);
}

// the weight pixel p gives vertex gv along one axis
__device__ __forceinline__ float vertex_weight(const int p, const int n, const int G, const int gv) {
  int i0;
  float f;
  axis_coord(p, n, G, i0, f);
  return i0 == gv ? 1.f - f : (i0 + 1 == gv ? f : 0.f);
}

// partial[strip][gy][gx][z][c]: the strip's share of v_A at the vertex; every element is written
__global__ __launch_bounds__(TPB) void slice_bwd_grid_kernel(const int H, const int W, const int Gw, const int Gh,
                                                             const int L, const int strips,
                                                             const float *__restrict__ rgb,
                                                             const float *__restrict__ v_out,
                                                             double *__restrict__ partial) {
  __shared__ int sz[TPB];
  __shared__ float sw0[TPB], sw1[TPB];
  __shared__ float sp[TPB][CH];
  const int t = threadIdx.x;
  const unsigned vert = blockIdx.x % (unsigned)(Gw * Gh);  // workgroup = strip * Gw * Gh + vertex
  const int gx = (int)(vert % (unsigned)Gw), gy = (int)(vert / (unsigned)Gw), s = (int)(blockIdx.x / (unsigned)(Gw * Gh));
  int x_lo, x_hi, y_lo, y_hi;
  vertex_range(gx, W, Gw, x_lo, x_hi);
  vertex_range(gy, H, Gh, y_lo, y_hi);
  const int per = (y_hi - y_lo + strips - 1) / strips;
  const int r0 = y_lo + s * per, r1 = min(r0 + per, y_hi);
  const int rw = x_hi - x_lo;
  const long long n = (r1 > r0 && rw > 0) ? (long long)rw * (r1 - r0) : 0;
  const int outs = L * CH;  // (<= 192)
  const int z = t / CH, c = t - z * CH;
  double acc = 0.0;
  for (long long base = 0; base < n; base += TPB) {
    const long long i = base + t;
    int z0 = 0;
    float w0 = 0.f, w1 = 0.f, P[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) P[k] = 0.f;
    if (i < n) {
      const int py = r0 + (int)(i / rw), px = x_lo + (int)(i % rw);
      const float w = vertex_weight(py, H, Gh, gy) * vertex_weight(px, W, Gw, gx);
      if (w != 0.f) {
        const size_t q = (size_t)py * W + px;
        const float h[4] = {rgb[3 * q], rgb[3 * q + 1], rgb[3 * q + 2], 1.f};
        float fz;
        guide_coord(h[0], h[1], h[2], L, z0, fz);
        w0 = w * (1.f - fz), w1 = w * fz;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float vo = v_out[3 * q + r];
#pragma unroll
          for (int k = 0; k < 4; ++k) P[4 * r + k] = vo * h[k];
        }
      }
    }
    sz[t] = z0, sw0[t] = w0, sw1[t] = w1;
#pragma unroll
    for (int k = 0; k < CH; ++k) sp[t][k] = P[k];
    __syncthreads();
    if (t < outs) {
      const int cnt = (int)(n - base < (long long)TPB ? n - base : (long long)TPB);
      for (int j = 0; j < cnt; ++j) {  // (every thread reads pixel j: LDS broadcasts)
        const int zz = sz[j];
        const float ws = z == zz ? sw0[j] : (z == zz + 1 ? sw1[j] : 0.f);
        acc += (double)(ws * sp[j][c]);
      }
    }
    __syncthreads();  // (the stage is rewritten by the next chunk)
  }
  if (t < outs) partial[(size_t)blockIdx.x * outs + t] = acc;
}

// v_A[V][L][Gh][Gw][12]: the strips of view `view` added in ascending order; exact zeros for every other view
__global__ __launch_bounds__(TPB) void slice_bwd_final_kernel(const int V, const int view, const int Gw, const int Gh,
                                                              const int L, const int strips,
                                                              const double *__restrict__ partial,
                                                              float *__restrict__ v_grids) {
  const size_t per_view = (size_t)L * Gh * Gw * CH;
  const size_t o = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (o >= per_view * V) return;
  const size_t e = o % per_view;
  float r = 0.f;
  if (o / per_view == (size_t)view) {
    const int c = (int)(e % CH);
    const size_t vert = e / CH;  // (z, gy, gx)
    const size_t plane = (size_t)Gh * Gw;
    const int z = (int)(vert / plane);
    const size_t xy = vert - (size_t)z * plane;
    double acc = 0.0;
    for (int s = 0; s < strips; ++s) acc += partial[((size_t)s * plane + xy) * ((size_t)L * CH) + (size_t)z * CH + c];
    r = (float)acc;
  }
  v_grids[o] = r;
}

// ---- total variation over all views --------------------------------------------------------------------------------
// element i of A[V][L][Gh][Gw][12] -> its vertex (z, y, x)
__device__ __forceinline__ void tv_vertex(const size_t i, const int Gw, const int Gh, const int L, int &z, int &y,
                                          int &x) {
  const size_t vert = i / CH;
  x = (int)(vert % Gw);
  y = (int)((vert / Gw) % Gh);
  z = (int)((vert / ((size_t)Gw * Gh)) % L);
}

// partial[3 b ..]: workgroup b's sums of the squared forward differences along L, Gh and Gw
__global__ __launch_bounds__(TPB) void tv_fwd_kernel(const size_t n, const int Gw, const int Gh, const int L,
                                                     const float *__restrict__ A, double *__restrict__ partial) {
  __shared__ double red[TPB];
  const size_t sx = CH, sy = (size_t)Gw * CH, sz = (size_t)Gh * Gw * CH;
  double al = 0.0, ay = 0.0, ax = 0.0;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
    int z, y, x;
    tv_vertex(i, Gw, Gh, L, z, y, x);
    const double a = (double)A[i];
    if (z + 1 < L) {
      const double d = (double)A[i + sz] - a;
      al += d * d;
    }
    if (y + 1 < Gh) {
      const double d = (double)A[i + sy] - a;
      ay += d * d;
    }
    if (x + 1 < Gw) {
      const double d = (double)A[i + sx] - a;
      ax += d * d;
    }
  }
  al = block_sum(al, red);
  ay = block_sum(ay, red);
  ax = block_sum(ax, red);
  if (threadIdx.x == 0) partial[3 * blockIdx.x] = al, partial[3 * blockIdx.x + 1] = ay, partial[3 * blockIdx.x + 2] = ax;
}

__global__ __launch_bounds__(TPB) void tv_final_kernel(const int blocks, const double count_l, const double count_y,
                                                       const double count_x, const double *__restrict__ partial,
                                                       float *__restrict__ loss_out) {
  __shared__ double red[TPB];
  double vl = 0.0, vy = 0.0, vx = 0.0;
  for (int b = threadIdx.x; b < blocks; b += TPB) vl += partial[3 * b], vy += partial[3 * b + 1], vx += partial[3 * b + 2];
  vl = block_sum(vl, red);
  vy = block_sum(vy, red);
  vx = block_sum(vx, red);
  if (threadIdx.x == 0) *loss_out = (float)(vl / count_l + vy / count_y + vx / count_x);
}

// v_A[i] = upstream * sum over the axes of 2 / count * ((A[i] - A[i - s]) [i > 0] - (A[i + s] - A[i]) [i < last])
__global__ __launch_bounds__(TPB) void tv_bwd_kernel(const size_t n, const int Gw, const int Gh, const int L,
                                                     const double inv_l, const double inv_y, const double inv_x,
                                                     const float *__restrict__ upstream, const float *__restrict__ A,
                                                     float *__restrict__ v_A) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const size_t sx = CH, sy = (size_t)Gw * CH, sz = (size_t)Gh * Gw * CH;
  int z, y, x;
  tv_vertex(i, Gw, Gh, L, z, y, x);
  const double a = (double)A[i];
  double gl = 0.0, gy = 0.0, gx = 0.0;
  if (z > 0) gl += a - (double)A[i - sz];
  if (z + 1 < L) gl -= (double)A[i + sz] - a;
  if (y > 0) gy += a - (double)A[i - sy];
  if (y + 1 < Gh) gy -= (double)A[i + sy] - a;
  if (x > 0) gx += a - (double)A[i - sx];
  if (x + 1 < Gw) gx -= (double)A[i + sx] - a;
  v_A[i] = (float)((double)upstream[0] * 2.0 * (gl * inv_l + gy * inv_y + gx * inv_x));
}

int check_grid(int V, int gw, int gh, int gl, const char *who) {
  GSR_REQUIRE(V >= 1, "%s: num_views must be positive", who);
  GSR_REQUIRE(gw >= 2 && gw <= GSR_BILAGRID_MAX_XY, "%s: grid_w must be in [2, %d]", who, GSR_BILAGRID_MAX_XY);
  GSR_REQUIRE(gh >= 2 && gh <= GSR_BILAGRID_MAX_XY, "%s: grid_h must be in [2, %d]", who, GSR_BILAGRID_MAX_XY);
  GSR_REQUIRE(gl >= 2 && gl <= GSR_BILAGRID_MAX_L, "%s: grid_l must be in [2, %d]", who, GSR_BILAGRID_MAX_L);
  GSR_REQUIRE((unsigned long long)V * gw * gh * gl * CH <= 0x7fffffffull, "%s: the grids must hold fewer than 2^31 floats",
              who);
  return GSR_OK;
}
int check_slice(unsigned H, unsigned W, int V, int view, int gw, int gh, int gl, const float *grids, const char *who) {
  GSR_REQUIRE(H > 0 && W > 0 && (unsigned long long)H * W * 3 <= 0x7fffffffull, "%s: 3 * H * W must be in [1, 2^31)", who);
  if (int rc = check_grid(V, gw, gh, gl, who)) return rc;
  GSR_REQUIRE(view >= 0 && view < V, "%s: view must be in [0, num_views)", who);
  GSR_REQUIRE(grids && ((uintptr_t)grids & 15) == 0, "%s: grids must be a 16-byte aligned pointer", who);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT int gsr_bilagrid_slice_forward(unsigned img_height, unsigned img_width, int num_views, int view, int grid_w,
                                          int grid_h, int grid_l, const float *grids, const float *rgb, float *out,
                                          gsr_stream_t stream) {
  if (int rc = check_slice(img_height, img_width, num_views, view, grid_w, grid_h, grid_l, grids,
                           "bilagrid_slice_forward"))
    return rc;
  GSR_REQUIRE(rgb && out, "bilagrid_slice_forward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  const float *grid = grids + (size_t)view * grid_l * grid_h * grid_w * CH;
  hipLaunchKernelGGL(slice_fwd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream,
                     (int)img_height, (int)img_width, grid_w, grid_h, grid_l, grid, rgb, out);
  GSR_CHECK_LAUNCH("bilagrid_slice_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_bilagrid_slice_backward(unsigned img_height, unsigned img_width, int num_views, int view, int grid_w,
                                           int grid_h, int grid_l, const float *grids, const float *rgb,
                                           const float *v_out, double *workspace, float *v_rgb, float *v_grids,
                                           gsr_stream_t stream) {
  if (int rc = check_slice(img_height, img_width, num_views, view, grid_w, grid_h, grid_l, grids,
                           "bilagrid_slice_backward"))
    return rc;
  GSR_REQUIRE(rgb && v_out && workspace && v_rgb && v_grids, "bilagrid_slice_backward: null pointer");
  const size_t n = (size_t)img_height * img_width;
  const float *grid = grids + (size_t)view * grid_l * grid_h * grid_w * CH;
  const int strips = GSR_BILAGRID_STRIPS(grid_w, grid_h);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(slice_bwd_rgb_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, s, (int)img_height,
                     (int)img_width, grid_w, grid_h, grid_l, grid, rgb, v_out, v_rgb);
  GSR_CHECK_LAUNCH("bilagrid_slice_backward (rgb)");
  hipLaunchKernelGGL(slice_bwd_grid_kernel, dim3((unsigned)(grid_w * grid_h * strips)), dim3(TPB), 0, s,
                     (int)img_height, (int)img_width, grid_w, grid_h, grid_l, strips, rgb, v_out, workspace);
  GSR_CHECK_LAUNCH("bilagrid_slice_backward (grid)");
  const size_t total = (size_t)num_views * grid_l * grid_h * grid_w * CH;
  hipLaunchKernelGGL(slice_bwd_final_kernel, dim3((unsigned)((total + TPB - 1) / TPB)), dim3(TPB), 0, s, num_views, view,
                     grid_w, grid_h, grid_l, strips, (const double *)workspace, v_grids);
  GSR_CHECK_LAUNCH("bilagrid_slice_backward (final)");
  return GSR_OK;
}

GSR_EXPORT int gsr_bilagrid_tv_forward(int num_views, int grid_w, int grid_h, int grid_l, const float *grids,
                                       double *partial, float *loss_out, gsr_stream_t stream) {
  if (int rc = check_grid(num_views, grid_w, grid_h, grid_l, "bilagrid_tv_forward")) return rc;
  GSR_REQUIRE(grids && partial && loss_out, "bilagrid_tv_forward: null pointer");
  const size_t n = (size_t)num_views * grid_l * grid_h * grid_w * CH;
  const size_t want = (n + TPB - 1) / TPB;
  const int blocks = (int)(want < (size_t)TV_MAX_BLOCKS ? want : (size_t)TV_MAX_BLOCKS);
  const double per = (double)num_views * CH;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tv_fwd_kernel, dim3(blocks), dim3(TPB), 0, s, n, grid_w, grid_h, grid_l, grids, partial);
  GSR_CHECK_LAUNCH("bilagrid_tv_forward");
  hipLaunchKernelGGL(tv_final_kernel, dim3(1), dim3(TPB), 0, s, blocks, per * (grid_l - 1) * grid_h * grid_w,
                     per * grid_l * (grid_h - 1) * grid_w, per * grid_l * grid_h * (grid_w - 1),
                     (const double *)partial, loss_out);
  GSR_CHECK_LAUNCH("bilagrid_tv_final");
  return GSR_OK;
}

GSR_EXPORT int gsr_bilagrid_tv_backward(int num_views, int grid_w, int grid_h, int grid_l, const float *upstream,
                                        const float *grids, float *v_grids, gsr_stream_t stream) {
  if (int rc = check_grid(num_views, grid_w, grid_h, grid_l, "bilagrid_tv_backward")) return rc;
  GSR_REQUIRE(upstream && grids && v_grids, "bilagrid_tv_backward: null pointer");
  const size_t n = (size_t)num_views * grid_l * grid_h * grid_w * CH;
  const double per = (double)num_views * CH;
  hipLaunchKernelGGL(tv_bwd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, n, grid_w,
                     grid_h, grid_l, 1.0 / (per * (grid_l - 1) * grid_h * grid_w),
                     1.0 / (per * grid_l * (grid_h - 1) * grid_w), 1.0 / (per * grid_l * grid_h * (grid_w - 1)),
                     upstream, grids, v_grids);
  GSR_CHECK_LAUNCH("bilagrid_tv_backward");
  return GSR_OK;
}
