// normals.hip -- normal maps and the depth-normal consistency loss (the rule is stated in
// include/gsraster.h).  What 2DGS / GOF / RaDe-GS / PGSR / gsplat's `normal_lambda` add to colour-only training: every
// Gaussian gets a normal (the axis of its smallest scale, turned towards the camera), the normals are composited into
// an image, a second normal image is derived from the rendered depth, and their disagreement is penalised.
//   gaussian normals  one thread per Gaussian, forward and backward (v_quats through the normalisation and the
//                     rotation column; argmin and the facing sign are piecewise constant)
//   depth normals     one thread per pixel, one workgroup per 16 x 16 tile; depth and validity staged in LDS with a
//                     one-pixel halo
//   consistency loss  forward: the same tile, the depth normal formed in registers and never written; one float64
//                     partial per tile, summed in a fixed order by a one-workgroup launch.
//                     backward: v_normals_img per pixel, and v_depth as a GATHER -- the tile stages depth with a
//                     two-pixel halo, forms dL/du and dL/dv (u, v the two central differences) of every pixel of the
//                     tile and its one-pixel ring in LDS, and pixel q adds the four terms of its four neighbours.
// No atomics, no memset, every output element written; two runs are bit-equal.  As in mono_depth.hip the per-element
// arithmetic is done in float64 registers (these kernels stream 20-50 bytes per element: the arithmetic is free) and
// what is rounded to float32 is what leaves the kernel.
#include "gsr_common.h"

namespace {

constexpr int TPB = 256;
constexpr int TILE = GSR_NORMAL_TILE;  // 16: TILE * TILE == TPB
constexpr int H1 = TILE + 2;           // the tile with a one-pixel halo
constexpr int H2 = TILE + 4;           // ... with a two-pixel halo

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

struct Intr {
  double fx, fy, cx, cy;
};

// the ray of pixel (row i, column j) through its centre (j + 0.5, i + 0.5): P = ray * depth, ray.z == 1
__device__ __forceinline__ double ray_x(const Intr &K, const int j) { return ((double)j + 0.5 - K.cx) / K.fx; }
__device__ __forceinline__ double ray_y(const Intr &K, const int i) { return ((double)i + 0.5 - K.cy) / K.fy; }

// The depth normal of pixel (i, j) from its four neighbours' depths, and what its pullback needs.
//   u = P(i+1, j) - P(i-1, j)    v = P(i, j+1) - P(i, j-1)    c = u x v    n = c / |c|
// (0, 0, -1) for a fronto-parallel plane.  false where |c|^2 is zero or not finite: the caller writes the zeros (n is
// then left unset, which keeps the struct in registers).  One function for the depth-normal map, the loss and its
// backward: they agree on a pixel's normal and validity bit for bit.
struct DepthNormal {
  double n[3], u[3], v[3], inv_len;
};
__device__ __forceinline__ bool depth_normal(const Intr &K, const int i, const int j, const double d_up,
                                             const double d_down, const double d_left, const double d_right,
                                             DepthNormal &o) {
  const double rx = ray_x(K, j), ry = ray_y(K, i);
  o.u[0] = rx * (d_down - d_up);
  o.u[1] = ray_y(K, i + 1) * d_down - ray_y(K, i - 1) * d_up;
  o.u[2] = d_down - d_up;
  o.v[0] = ray_x(K, j + 1) * d_right - ray_x(K, j - 1) * d_left;
  o.v[1] = ry * (d_right - d_left);
  o.v[2] = d_right - d_left;
  const double c0 = o.u[1] * o.v[2] - o.u[2] * o.v[1];
  const double c1 = o.u[2] * o.v[0] - o.u[0] * o.v[2];
  const double c2 = o.u[0] * o.v[1] - o.u[1] * o.v[0];
  const double l2 = c0 * c0 + c1 * c1 + c2 * c2;
  if (!(l2 > 0.0) || !isfinite(l2)) return false;
  o.inv_len = 1.0 / sqrt(l2);
  o.n[0] = c0 * o.inv_len, o.n[1] = c1 * o.inv_len, o.n[2] = c2 * o.inv_len;
  return true;
}

// g = dL/dn -> dL/du and dL/dv:  dL/dc = (g - n (n . g)) / |c|,  dL/du = v x dL/dc,  dL/dv = dL/dc x u
__device__ __forceinline__ void depth_normal_pullback(const DepthNormal &o, const double *g, double *du, double *dv) {
  const double ng = o.n[0] * g[0] + o.n[1] * g[1] + o.n[2] * g[2];
  const double c0 = (g[0] - o.n[0] * ng) * o.inv_len, c1 = (g[1] - o.n[1] * ng) * o.inv_len,
               c2 = (g[2] - o.n[2] * ng) * o.inv_len;
  du[0] = o.v[1] * c2 - o.v[2] * c1, du[1] = o.v[2] * c0 - o.v[0] * c2, du[2] = o.v[0] * c1 - o.v[1] * c0;
  dv[0] = c1 * o.u[2] - c2 * o.u[1], dv[1] = c2 * o.u[0] - c0 * o.u[2], dv[2] = c0 * o.u[1] - c1 * o.u[0];
}

// Stage the depth of the tile at (y0, x0) with a halo of `halo` pixels: sd the depth, sk whether the pixel can take part
// in a normal (inside the image, alpha > 0 -- the test is on alpha: the models fill alpha == 0 pixels with depth.max()
// -- and a finite depth).  A pixel outside the image is not read; that is also what makes the image's one-pixel border
// invalid.  Ends with a barrier.
template <int halo>
__device__ __forceinline__ void stage_depth(const int H, const int W, const int y0, const int x0,
                                            const float *__restrict__ depth, const float *__restrict__ alpha,
                                            float *sd, unsigned char *sk) {
  constexpr int S = TILE + 2 * halo;
  for (int k = threadIdx.x; k < S * S; k += TPB) {
    const int ly = k / S, lx = k - ly * S;
    const int y = y0 - halo + ly, x = x0 - halo + lx;
    float d = 0.f;
    bool ok = false;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t q = (size_t)y * W + x;
      d = depth[q];
      ok = !(alpha[q] <= 0.f) && isfinite(d);
    }
    sd[k] = d, sk[k] = ok ? 1 : 0;
  }
  __syncthreads();
}

// the normal of the pixel at (ly, lx) of a staged tile of row stride S, image pixel (i, j)
template <int S>
__device__ __forceinline__ bool staged_normal(const Intr &K, const float *sd, const unsigned char *sk, const int ly,
                                              const int lx, const int i, const int j, DepthNormal &o) {
  const int c = ly * S + lx;
  if (!(sk[c] && sk[c - S] && sk[c + S] && sk[c - 1] && sk[c + 1])) return false;
  return depth_normal(K, i, j, (double)sd[c - S], (double)sd[c + S], (double)sd[c - 1], (double)sd[c + 1], o);
}

__global__ __launch_bounds__(TPB) void depth_normal_kernel(const int H, const int W, const int tiles_x, const Intr K,
                                                           const float *__restrict__ depth,
                                                           const float *__restrict__ alpha,
                                                           float *__restrict__ normals) {
  __shared__ float sd[H1 * H1];
  __shared__ unsigned char sk[H1 * H1];
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int y0 = ty * TILE, x0 = tx * TILE;
  stage_depth<1>(H, W, y0, x0, depth, alpha, sd, sk);
  const int ly = threadIdx.x / TILE, lx = threadIdx.x % TILE;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= H || x >= W) return;
  DepthNormal o;
  const bool valid = staged_normal<H1>(K, sd, sk, ly + 1, lx + 1, y, x, o);
  const size_t q = (size_t)y * W + x;
  normals[3 * q] = valid ? (float)o.n[0] : 0.f;
  normals[3 * q + 1] = valid ? (float)o.n[1] : 0.f;
  normals[3 * q + 2] = valid ? (float)o.n[2] : 0.f;
}

// partial[tile] = sum over the tile's pixels of m (1 - alpha <N, n_d>); an invalid pixel adds m
__global__ __launch_bounds__(TPB) void consistency_fwd_kernel(const int H, const int W, const int tiles_x, const Intr K,
                                                              const float *__restrict__ nimg,
                                                              const float *__restrict__ depth,
                                                              const float *__restrict__ alpha,
                                                              const float *__restrict__ mask,
                                                              double *__restrict__ partial) {
  __shared__ float sd[H1 * H1];
  __shared__ unsigned char sk[H1 * H1];
  __shared__ double red[TPB];
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int y0 = ty * TILE, x0 = tx * TILE;
  stage_depth<1>(H, W, y0, x0, depth, alpha, sd, sk);
  const int ly = threadIdx.x / TILE, lx = threadIdx.x % TILE;
  const int y = y0 + ly, x = x0 + lx;
  double term = 0.0;
  if (y < H && x < W) {
    const size_t q = (size_t)y * W + x;
    const double m = mask ? (double)mask[q] : 1.0;
    DepthNormal o;
    if (staged_normal<H1>(K, sd, sk, ly + 1, lx + 1, y, x, o)) {
      const double dot = (double)nimg[3 * q] * o.n[0] + (double)nimg[3 * q + 1] * o.n[1] + (double)nimg[3 * q + 2] * o.n[2];
      term = m * (1.0 - (double)alpha[q] * dot);
    } else {
      term = m;
    }
  }
  term = block_sum(term, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = term;
}

// loss = (the tiles' sums in a fixed order) / (H W)
__global__ __launch_bounds__(TPB) void consistency_final_kernel(const int tiles, const double count,
                                                                const double *__restrict__ partial,
                                                                float *__restrict__ loss_out) {
  __shared__ double red[TPB];
  double v = 0.0;
  for (int b = threadIdx.x; b < tiles; b += TPB) v += partial[b];
  v = block_sum(v, red);
  if (threadIdx.x == 0) *loss_out = (float)(v / count);
}

// With s = -upstream / (H W):  v_nimg(p) = s m alpha n_d(p)  (zeros at an invalid pixel), and from g(p) = dL/dn_d(p) =
// s m alpha N(p) the pullback's dL/du(p), dL/dv(p) in LDS for the tile and its ring.  Then for pixel q with ray r_q
//   v_depth(q) = <du(up of q), r_q> - <du(down of q), r_q> + <dv(left of q), r_q> - <dv(right of q), r_q>
// (q is the lower neighbour of the pixel above it, and so on); an invalid or outside pixel holds zeros.
__global__ __launch_bounds__(TPB) void consistency_bwd_kernel(const int H, const int W, const int tiles_x, const Intr K,
                                                              const float *__restrict__ upstream,
                                                              const float *__restrict__ nimg,
                                                              const float *__restrict__ depth,
                                                              const float *__restrict__ alpha,
                                                              const float *__restrict__ mask,
                                                              float *__restrict__ v_nimg,
                                                              float *__restrict__ v_depth) {
  __shared__ float sd[H2 * H2];
  __shared__ unsigned char sk[H2 * H2];
  __shared__ double sg[H1 * H1][6];
  const int ty = (int)(blockIdx.x / (unsigned)tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)tiles_x);
  const int y0 = ty * TILE, x0 = tx * TILE;
  stage_depth<2>(H, W, y0, x0, depth, alpha, sd, sk);
  const double s = -(double)upstream[0] / ((double)H * (double)W);
  for (int k = threadIdx.x; k < H1 * H1; k += TPB) {
    const int ry = k / H1, rx = k - ry * H1;  // ring coordinates: the tile is [1, TILE] in both
    const int y = y0 - 1 + ry, x = x0 - 1 + rx;
    double du[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0};
    if (y >= 0 && y < H && x >= 0 && x < W) {
      const size_t q = (size_t)y * W + x;
      const bool own = ry >= 1 && ry <= TILE && rx >= 1 && rx <= TILE;  // this workgroup writes the pixel
      DepthNormal o;
      const bool valid = staged_normal<H2>(K, sd, sk, ry + 1, rx + 1, y, x, o);
      float vn[3] = {0.f, 0.f, 0.f};
      if (valid) {
        const double w = s * (mask ? (double)mask[q] : 1.0) * (double)alpha[q];
        const double g[3] = {w * (double)nimg[3 * q], w * (double)nimg[3 * q + 1], w * (double)nimg[3 * q + 2]};
        depth_normal_pullback(o, g, du, dv);
        vn[0] = (float)(w * o.n[0]), vn[1] = (float)(w * o.n[1]), vn[2] = (float)(w * o.n[2]);
      }
      if (own) v_nimg[3 * q] = vn[0], v_nimg[3 * q + 1] = vn[1], v_nimg[3 * q + 2] = vn[2];
    }
    sg[k][0] = du[0], sg[k][1] = du[1], sg[k][2] = du[2], sg[k][3] = dv[0], sg[k][4] = dv[1], sg[k][5] = dv[2];
  }
  __syncthreads();
  const int ly = threadIdx.x / TILE, lx = threadIdx.x % TILE;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= H || x >= W) return;
  const int c = (ly + 1) * H1 + lx + 1;
  const double rx = ray_x(K, x), ry = ray_y(K, y);
  const double *up = sg[c - H1], *down = sg[c + H1], *left = sg[c - 1], *right = sg[c + 1];
  double acc = up[0] * rx + up[1] * ry + up[2];
  acc -= down[0] * rx + down[1] * ry + down[2];
  acc += left[3] * rx + left[4] * ry + left[5];
  acc -= right[3] * rx + right[4] * ry + right[5];
  v_depth[(size_t)y * W + x] = (float)acc;
}

// ---- per-Gaussian normals ------------------------------------------------------------------------------------------
// column `axis` of R(q), q normalised (the projection's convention, project.hip)
__device__ __forceinline__ void rot_column(const int axis, const double w, const double x, const double y, const double z,
                                           double *c) {
  if (axis == 0)
    c[0] = 1.0 - 2.0 * (y * y + z * z), c[1] = 2.0 * (x * y + w * z), c[2] = 2.0 * (x * z - w * y);
  else if (axis == 1)
    c[0] = 2.0 * (x * y - w * z), c[1] = 1.0 - 2.0 * (x * x + z * z), c[2] = 2.0 * (y * z + w * x);
  else
    c[0] = 2.0 * (x * z + w * y), c[1] = 2.0 * (y * z - w * x), c[2] = 1.0 - 2.0 * (x * x + y * y);
}

__global__ __launch_bounds__(TPB) void gaussian_normals_fwd_kernel(const int n, const float *__restrict__ quats,
                                                                   const float *__restrict__ scales,
                                                                   const float *__restrict__ means,
                                                                   const float *__restrict__ viewmat,
                                                                   float *__restrict__ normals, int *__restrict__ axis_out,
                                                                   float *__restrict__ sign_out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const float4 qf = reinterpret_cast<const float4 *>(quats)[i];
  const float s0 = scales[3 * (size_t)i], s1 = scales[3 * (size_t)i + 1], s2 = scales[3 * (size_t)i + 2];
  int axis = 0;  // the smallest scale; a tie goes to the lowest index (a NaN scale never wins)
  float sm = s0;
  if (s1 < sm) axis = 1, sm = s1;
  if (s2 < sm) axis = 2;
  const double qw = qf.x, qx = qf.y, qy = qf.z, qz = qf.w;
  const double inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  double c[3];
  rot_column(axis, qw * inv, qx * inv, qy * inv, qz * inv, c);
  const double mx = means[3 * (size_t)i], my = means[3 * (size_t)i + 1], mz = means[3 * (size_t)i + 2];
  double nc[3], pc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = viewmat[4 * r], b = viewmat[4 * r + 1], d = viewmat[4 * r + 2];
    nc[r] = a * c[0] + b * c[1] + d * c[2];
    pc[r] = a * mx + b * my + d * mz + (double)viewmat[4 * r + 3];
  }
  const double sgn = (nc[0] * pc[0] + nc[1] * pc[1] + nc[2] * pc[2]) > 0.0 ? -1.0 : 1.0;  // faces the camera
  normals[3 * (size_t)i] = (float)(sgn * nc[0]);
  normals[3 * (size_t)i + 1] = (float)(sgn * nc[1]);
  normals[3 * (size_t)i + 2] = (float)(sgn * nc[2]);
  axis_out[i] = axis;
  sign_out[i] = (float)sgn;
}

__global__ __launch_bounds__(TPB) void gaussian_normals_bwd_kernel(const int n, const float *__restrict__ quats,
                                                                   const float *__restrict__ viewmat,
                                                                   const int *__restrict__ axis_in,
                                                                   const float *__restrict__ sign_in,
                                                                   const float *__restrict__ v_normals,
                                                                   float *__restrict__ v_quats) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const float4 qf = reinterpret_cast<const float4 *>(quats)[i];
  const double sgn = sign_in[i];
  const double h0 = sgn * (double)v_normals[3 * (size_t)i], h1 = sgn * (double)v_normals[3 * (size_t)i + 1],
               h2 = sgn * (double)v_normals[3 * (size_t)i + 2];
  // g = V^T (sign v_normals): the cotangent of the rotation column in world space
  const double g0 = viewmat[0] * h0 + viewmat[4] * h1 + viewmat[8] * h2;
  const double g1 = viewmat[1] * h0 + viewmat[5] * h1 + viewmat[9] * h2;
  const double g2 = viewmat[2] * h0 + viewmat[6] * h1 + viewmat[10] * h2;
  const double qw = qf.x, qx = qf.y, qy = qf.z, qz = qf.w;
  const double inv = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  const double w = qw * inv, x = qx * inv, y = qy * inv, z = qz * inv;
  double vw, vx, vy, vz;  // the column's pullback to the normalised quaternion
  const int axis = axis_in[i];
  if (axis == 0) {
    vw = 2.0 * (z * g1 - y * g2);
    vx = 2.0 * (y * g1 + z * g2);
    vy = 2.0 * (x * g1 - w * g2) - 4.0 * y * g0;
    vz = 2.0 * (w * g1 + x * g2) - 4.0 * z * g0;
  } else if (axis == 1) {
    vw = 2.0 * (x * g2 - z * g0);
    vx = 2.0 * (y * g0 + w * g2) - 4.0 * x * g1;
    vy = 2.0 * (x * g0 + z * g2);
    vz = 2.0 * (y * g2 - w * g0) - 4.0 * z * g1;
  } else {
    vw = 2.0 * (y * g0 - x * g1);
    vx = 2.0 * (z * g0 - w * g1) - 4.0 * x * g2;
    vy = 2.0 * (w * g0 + z * g1) - 4.0 * y * g2;
    vz = 2.0 * (x * g0 + y * g1);
  }
  // through q / |q|:  (v - qn (qn . v)) / |q|
  const double dot = w * vw + x * vx + y * vy + z * vz;
  reinterpret_cast<float4 *>(v_quats)[i] = make_float4((float)((vw - w * dot) * inv), (float)((vx - x * dot) * inv),
                                                       (float)((vy - y * dot) * inv), (float)((vz - z * dot) * inv));
}

int check_image(unsigned H, unsigned W, double fx, double fy, const char *who) {
  GSR_REQUIRE(H > 0 && W > 0 && (unsigned long long)H * W * 3 <= 0x7fffffffull, "%s: 3 * H * W must be in [1, 2^31)", who);
  GSR_REQUIRE(fx != 0.0 && fy != 0.0 && fx == fx && fy == fy, "%s: fx and fy must be non-zero numbers", who);
  return GSR_OK;
}
int check_gaussians(int n, const float *quats, const char *who) {
  GSR_REQUIRE(n >= 0 && (unsigned long long)n * 4 <= 0x7fffffffull, "%s: 4 * num_points must be in [0, 2^31)", who);
  GSR_REQUIRE(n == 0 || (quats && ((uintptr_t)quats & 15) == 0), "%s: quats must be a 16-byte aligned pointer", who);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT int gsr_gaussian_normals_forward(int num_points, const float *quats, const float *scales, const float *means,
                                            const float *viewmat, float *normals, int *axis, float *sign,
                                            gsr_stream_t stream) {
  if (int rc = check_gaussians(num_points, quats, "gaussian_normals_forward")) return rc;
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(scales && means && viewmat && normals && axis && sign, "gaussian_normals_forward: null pointer");
  hipLaunchKernelGGL(gaussian_normals_fwd_kernel, dim3(gsr_cdiv((unsigned)num_points, TPB)), dim3(TPB), 0,
                     (hipStream_t)stream, num_points, quats, scales, means, viewmat, normals, axis, sign);
  GSR_CHECK_LAUNCH("gaussian_normals_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_gaussian_normals_backward(int num_points, const float *quats, const float *viewmat, const int *axis,
                                             const float *sign, const float *v_normals, float *v_quats,
                                             gsr_stream_t stream) {
  if (int rc = check_gaussians(num_points, quats, "gaussian_normals_backward")) return rc;
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(viewmat && axis && sign && v_normals && v_quats && ((uintptr_t)v_quats & 15) == 0,
              "gaussian_normals_backward: null pointer, or v_quats not 16-byte aligned");
  hipLaunchKernelGGL(gaussian_normals_bwd_kernel, dim3(gsr_cdiv((unsigned)num_points, TPB)), dim3(TPB), 0,
                     (hipStream_t)stream, num_points, quats, viewmat, axis, sign, v_normals, v_quats);
  GSR_CHECK_LAUNCH("gaussian_normals_backward");
  return GSR_OK;
}

GSR_EXPORT int gsr_depth_normals(unsigned img_height, unsigned img_width, double fx, double fy, double cx, double cy,
                                 const float *depth, const float *alpha, float *normals, gsr_stream_t stream) {
  if (int rc = check_image(img_height, img_width, fx, fy, "depth_normals")) return rc;
  GSR_REQUIRE(depth && alpha && normals, "depth_normals: null pointer");
  const unsigned tiles_x = gsr_cdiv(img_width, TILE), tiles_y = gsr_cdiv(img_height, TILE);
  const Intr K = {fx, fy, cx, cy};
  hipLaunchKernelGGL(depth_normal_kernel, dim3(tiles_x * tiles_y), dim3(TPB), 0, (hipStream_t)stream, (int)img_height,
                     (int)img_width, (int)tiles_x, K, depth, alpha, normals);
  GSR_CHECK_LAUNCH("depth_normals");
  return GSR_OK;
}

GSR_EXPORT int gsr_normal_consistency_forward(unsigned img_height, unsigned img_width, double fx, double fy, double cx,
                                              double cy, const float *normals_img, const float *depth,
                                              const float *alpha, const float *mask, double *partial, float *loss_out,
                                              gsr_stream_t stream) {
  if (int rc = check_image(img_height, img_width, fx, fy, "normal_consistency_forward")) return rc;
  GSR_REQUIRE(normals_img && depth && alpha && partial && loss_out, "normal_consistency_forward: null pointer");
  const unsigned tiles_x = gsr_cdiv(img_width, TILE), tiles_y = gsr_cdiv(img_height, TILE);
  const Intr K = {fx, fy, cx, cy};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(consistency_fwd_kernel, dim3(tiles_x * tiles_y), dim3(TPB), 0, s, (int)img_height, (int)img_width,
                     (int)tiles_x, K, normals_img, depth, alpha, mask, partial);
  GSR_CHECK_LAUNCH("normal_consistency_forward");
  hipLaunchKernelGGL(consistency_final_kernel, dim3(1), dim3(TPB), 0, s, (int)(tiles_x * tiles_y),
                     (double)img_height * (double)img_width, (const double *)partial, loss_out);
  GSR_CHECK_LAUNCH("normal_consistency_final");
  return GSR_OK;
}

GSR_EXPORT int gsr_normal_consistency_backward(unsigned img_height, unsigned img_width, double fx, double fy, double cx,
                                               double cy, const float *upstream, const float *normals_img,
                                               const float *depth, const float *alpha, const float *mask,
                                               float *v_normals_img, float *v_depth, gsr_stream_t stream) {
  if (int rc = check_image(img_height, img_width, fx, fy, "normal_consistency_backward")) return rc;
  GSR_REQUIRE(upstream && normals_img && depth && alpha && v_normals_img && v_depth,
              "normal_consistency_backward: null pointer");
  const unsigned tiles_x = gsr_cdiv(img_width, TILE), tiles_y = gsr_cdiv(img_height, TILE);
  const Intr K = {fx, fy, cx, cy};
  hipLaunchKernelGGL(consistency_bwd_kernel, dim3(tiles_x * tiles_y), dim3(TPB), 0, (hipStream_t)stream,
                     (int)img_height, (int)img_width, (int)tiles_x, K, upstream, normals_img, depth, alpha, mask,
                     v_normals_img, v_depth);
  GSR_CHECK_LAUNCH("normal_consistency_backward");
  return GSR_OK;
}
