// project.hip -- EWA projection of 3-D Gaussians and its VJP (gfx950).
//
// One lane per Gaussian; purely streaming (100 B in+out per Gaussian forward,
// ~190 B backward), HBM-bound.  The camera matrices are wave-uniform kernel
// arguments read through the scalar cache.  All outputs are written by every
// lane (zeros for culled splats) so callers can hand in uninitialised buffers.
//
// Behaviour restated from the reference kernels (gs_toolkit/gs_components/
// rasterizer/cuda/csrc): forward.cu:13-90,398-464, backward.cu:305-453,
// helpers.cuh:7-219.  3x3 algebra is written out on row-major scalars.
//
// Parity: this file is compiled with -ffp-contract=off (Makefile), like the CPU oracle
// (oracle/Makefile), and evaluates every expression in the oracle's operation order with
// correctly rounded division and square root (hipcc's default): the forward outputs --
// including the integer radii / num_tiles_hit, which sit behind a ceil() -- are then
// bit-identical to the oracle's (tests/test_gpu_kernels.py::test_project_forward).  The
// kernels are HBM-bound, so the few un-fused multiply-adds cost nothing measurable.
//
// Equidistant fisheye (FISH; gsplat's camera_model="fisheye" with an ideal lens).  For the
// view-space centre t = V p~ of a Gaussian:
//   * near plane: culled when tz <= clip, as above -- which also keeps the polar angle below 90 degrees;
//   * pixel centre: r = sqrt(tx^2 + ty^2), theta = atan2(r, tz), s = theta / r (-> 1 / tz as r -> 0),
//     xy = (fx s tx + cx - 0.5, fy s ty + cy - 0.5): pixel i has its centre at i, as on the pinhole path.  `projmat`
//     is not read;
//   * Jacobian, with d^2 = r^2 + tz^2 and c = (tz / d^2 - s) / r^2 (= 2 ds/d(r^2)):
//       J = [ fx (s + tx^2 c)   fx tx ty c        -fx tx / d^2 ]
//           [ fy tx ty c        fy (s + ty^2 c)   -fy ty / d^2 ]
//     Below q = r^2 / tz^2 < GSR_FISHEYE_SERIES_Q, s and c (and dc/d(r^2), which the backward needs) come from their
//     power series in q -- the closed forms are 0/0 at r = 0 and cancel next to it -- so every entry is finite and
//     accurate from r = 0 upward, also where r^2 underflows;
//   * no clamp of the centre, forward or backward: |J| <= max(fx, fy) / clip for tz > clip, and both directions
//     differentiate the same function;
//   * everything after J (cov2d = J W S W^T J^T, the +0.3, gsr_cov2d_bounds, the radius, gsr_tile_bbox) is the
//     pinhole text, but for the compensation's determinant, which is formed from the minors of T M where scales and
//     rotation are given (at its place in the kernel); depths = tz (ordering by ray distance |t| is not built);
//   * backward: v_t = J^T v_xy + (dJ/dt contracted with v_J) + W's third row v_depth; the rest is the pinhole chain.
#include "gsr_common.h"

namespace {

struct M3 {
  float a00, a01, a02, a10, a11, a12, a20, a21, a22;
};

__device__ __forceinline__ M3 mul(const M3 &A, const M3 &B) {
  M3 C;
  C.a00 = A.a00 * B.a00 + A.a01 * B.a10 + A.a02 * B.a20;
  C.a01 = A.a00 * B.a01 + A.a01 * B.a11 + A.a02 * B.a21;
  C.a02 = A.a00 * B.a02 + A.a01 * B.a12 + A.a02 * B.a22;
  C.a10 = A.a10 * B.a00 + A.a11 * B.a10 + A.a12 * B.a20;
  C.a11 = A.a10 * B.a01 + A.a11 * B.a11 + A.a12 * B.a21;
  C.a12 = A.a10 * B.a02 + A.a11 * B.a12 + A.a12 * B.a22;
  C.a20 = A.a20 * B.a00 + A.a21 * B.a10 + A.a22 * B.a20;
  C.a21 = A.a20 * B.a01 + A.a21 * B.a11 + A.a22 * B.a21;
  C.a22 = A.a20 * B.a02 + A.a21 * B.a12 + A.a22 * B.a22;
  return C;
}
__device__ __forceinline__ M3 transpose(const M3 &A) {
  return M3{A.a00, A.a10, A.a20, A.a01, A.a11, A.a21, A.a02, A.a12, A.a22};
}

// (w,x,y,z) quaternion -> rotation; renormalises (helpers.cuh:144-159)
__device__ __forceinline__ M3 quat_to_rot(float qw, float qx, float qy, float qz,
                                          float &w, float &x, float &y, float &z) {
  const float s = 1.f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);  // (not rsqrtf: see the parity note)
  w = qw * s;
  x = qx * s;
  y = qy * s;
  z = qz * s;
  M3 R;
  R.a00 = 1.f - 2.f * (y * y + z * z);
  R.a01 = 2.f * (x * y - w * z);
  R.a02 = 2.f * (x * z + w * y);
  R.a10 = 2.f * (x * y + w * z);
  R.a11 = 1.f - 2.f * (x * x + z * z);
  R.a12 = 2.f * (y * z - w * x);
  R.a20 = 2.f * (x * z - w * y);
  R.a21 = 2.f * (y * z + w * x);
  R.a22 = 1.f - 2.f * (x * x + y * y);
  return R;
}

// s = theta / r, c = 2 ds/d(r^2), cu = dc/d(r^2) (GRAD only), w = 1 / d^2 of the equidistant projection (header).
// Series: s tz = sum_k (-q)^k / (2k + 1), c tz^3 = sum_{k>=1} (-1)^k 2k / (2k + 1) q^(k-1),
// cu tz^5 = sum_{k>=2} (-1)^k 2k (k - 1) / (2k + 1) q^(k-2); six terms each, first dropped term below 3e-8 relative
// at the switch.  Above it the closed form of c loses 1.5 ulp / q: below 3e-6 relative, times q in J.
#define GSR_FISHEYE_SERIES_Q 0.03125f
struct Fisheye {
  float s, c, cu, w;
};
template <bool GRAD>
__device__ __forceinline__ Fisheye fisheye_terms(const float tx, const float ty, const float tz) {
  Fisheye f;
  const float r2 = tx * tx + ty * ty;  // (may underflow to 0: the series takes it)
  const float z2 = tz * tz;
  const float q = r2 / z2;
  f.w = 1.f / (r2 + z2);
  f.cu = 0.f;
  if (q < GSR_FISHEYE_SERIES_Q) {
    const float rz = 1.f / tz, rz3 = rz * rz * rz;
    f.s = rz * (1.f + q * (-1.f / 3.f + q * (1.f / 5.f + q * (-1.f / 7.f + q * (1.f / 9.f + q * (-1.f / 11.f))))));
    f.c = rz3 * (-2.f / 3.f + q * (4.f / 5.f + q * (-6.f / 7.f + q * (8.f / 9.f + q * (-10.f / 11.f + q * (12.f / 13.f))))));
    if constexpr (GRAD)
      f.cu = rz3 * rz * rz *
             (4.f / 5.f + q * (-12.f / 7.f + q * (24.f / 9.f + q * (-40.f / 11.f + q * (60.f / 13.f + q * (-84.f / 15.f))))));
  } else {
    const float r = sqrtf(r2);
    f.s = atan2f(r, tz) / r;
    f.c = (tz * f.w - f.s) / r2;
    if constexpr (GRAD) f.cu = (-tz * f.w * f.w - 1.5f * f.c) / r2;
  }
  return f;
}

struct Cam {
  float v[12];  // view matrix, top 3x4, row-major
  float p[16];  // full projection (P*V), row-major
};

// AA: also opacities_aa = opacities * compensation (the antialiased rasterize mode's opacity, vanilla_gs.py:815-816),
// one float32 multiply on the compensation this lane holds anyway; everything else is the same text for both flags.
// CROP: a Gaussian whose centre is outside the oriented crop box (gsr_crop_inside, gsr_common.h) leaves through the
// exit of a clipped one -- radii = num_tiles_hit = 0, zeros elsewhere -- before anything but its centre was read.
struct FwdAA {
  const float *opacities;
  float *opacities_aa;
};
struct FwdCrop {
  const float *crop;  // float32[16], gsr_common.h
};
template <typename T, typename... R>
__device__ __forceinline__ const T &fwd_first(const T &t, const R &...) {
  return t;
}
// FISH: the equidistant fisheye's Jacobian and pixel centre (header) in place of the pinhole's; no clamp, no projmat.
// X: nothing, FwdAA, FwdCrop, or FwdAA then FwdCrop (an empty pack leaves the classic kernel's signature as it was)
template <bool AA, bool CROP, bool FISH, typename... X>
__global__ __launch_bounds__(256) void project_fwd_kernel(
    const int n, const float *__restrict__ means3d,
    const float *__restrict__ scales, const float glob_scale,
    const float *__restrict__ quats, const float *__restrict__ viewmat,
    const float *__restrict__ projmat, const float fx, const float fy,
    const float cx, const float cy, const int img_w, const int img_h,
    const int tiles_x, const int tiles_y, const int bw, const float clip,
    float *__restrict__ cov3d, float *__restrict__ xys,
    float *__restrict__ depths, int *__restrict__ radii,
    float *__restrict__ conics, float *__restrict__ compensation,
    int *__restrict__ num_tiles_hit, const X... aa) {
  static_assert(sizeof...(X) == (AA ? 1 : 0) + (CROP ? 1 : 0),
                "project_fwd_kernel<AA, CROP, FISH, [FwdAA,] [FwdCrop]>: one argument per flag, in that order");
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;

  float o_cov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float o_x = 0.f, o_y = 0.f, o_depth = 0.f, o_comp = 0.f;
  float o_k0 = 0.f, o_k1 = 0.f, o_k2 = 0.f;
  int o_radius = 0, o_tiles = 0;

  const float px = means3d[3 * i], py = means3d[3 * i + 1], pz = means3d[3 * i + 2];
  const float *V = viewmat;
  const float tx = V[0] * px + V[1] * py + V[2] * pz + V[3];
  const float ty = V[4] * px + V[5] * py + V[6] * pz + V[7];
  const float tz = V[8] * px + V[9] * py + V[10] * pz + V[11];

  bool keep = true;
  if constexpr (CROP) {
    const FwdCrop &c = (aa, ...);  // (the last argument)
    keep = gsr_crop_inside(c.crop, px, py, pz);
  }

  if (keep && tz > clip) {  // near-plane cull is `z <= clip` (helpers.cuh:212-219)
    const M3 W{V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]};
    // FISH: T = J W is formed first, so that the minors of T M (the compensation, below) can be taken while M exists
    [[maybe_unused]] M3 Tf;
    [[maybe_unused]] float fish_s = 0.f, fish_det = 0.f;
    if constexpr (FISH) {
      const Fisheye f = fisheye_terms<false>(tx, ty, tz);
      const float xyc = tx * ty * f.c;
      const M3 J{fx * (f.s + tx * tx * f.c), fx * xyc, -fx * tx * f.w, fy * xyc, fy * (f.s + ty * ty * f.c), -fy * ty * f.w,
                 0.f, 0.f, 0.f};
      Tf = mul(J, W);
      fish_s = f.s;
    }
    M3 S;
    if (scales) {
      float w, x, y, z;
      const M3 R = quat_to_rot(quats[4 * i], quats[4 * i + 1], quats[4 * i + 2],
                               quats[4 * i + 3], w, x, y, z);
      const float s0 = glob_scale * scales[3 * i], s1 = glob_scale * scales[3 * i + 1],
                  s2 = glob_scale * scales[3 * i + 2];
      const M3 M{R.a00 * s0, R.a01 * s1, R.a02 * s2, R.a10 * s0, R.a11 * s1,
                 R.a12 * s2, R.a20 * s0, R.a21 * s1, R.a22 * s2};
      S = mul(M, transpose(M));
      if constexpr (FISH) {
        // det C for the compensation.  C00 C11 - C01^2 loses every digit on an elongated footprint (a needle of
        // 1 : 1000 has a determinant of 1e-6 of its terms).  C = A A^T with A = T M (2 x 3), and by Cauchy-Binet det C
        // is the sum of the squares of A's three 2 x 2 minors -- each a product of two scales times a minor of T R,
        // no cancellation between them.  Covariances handed in have no factor M: they keep the pinhole expression
        const M3 A = mul(Tf, M);
        const float m01 = A.a00 * A.a11 - A.a01 * A.a10;
        const float m02 = A.a00 * A.a12 - A.a02 * A.a10;
        const float m12 = A.a01 * A.a12 - A.a02 * A.a11;
        fish_det = m01 * m01 + m02 * m02 + m12 * m12;
      }
    } else {  // precomputed covariances: cov3d is an INPUT (upper triangle xx xy xz yy yz zz)
      const float *c = cov3d + 6 * i;
      S = M3{c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]};
    }
    o_cov[0] = S.a00;
    o_cov[1] = S.a01;
    o_cov[2] = S.a02;
    o_cov[3] = S.a11;
    o_cov[4] = S.a12;
    o_cov[5] = S.a22;

    M3 T;
    if constexpr (FISH) {
      T = Tf;
    } else {
      // EWA: clamp the centre to 1.3x the frustum, J = d(pix)/d(t)
      const float limx = 1.3f * (0.5f * (float)img_w / fx);
      const float limy = 1.3f * (0.5f * (float)img_h / fy);
      const float ex = tz * fminf(limx, fmaxf(-limx, tx / tz));
      const float ey = tz * fminf(limy, fmaxf(-limy, ty / tz));
      const float rz = 1.f / tz, rz2 = rz * rz;
      const M3 J{fx * rz, 0.f, -fx * ex * rz2, 0.f, fy * rz, -fy * ey * rz2, 0.f, 0.f, 0.f};
      T = mul(J, W);
    }
    const M3 Vs{S.a00, S.a01, S.a02, S.a01, S.a11, S.a12, S.a02, S.a12, S.a22};
    const M3 C = mul(mul(T, Vs), transpose(T));
    const float det_orig = C.a00 * C.a11 - C.a01 * C.a01;
    const float c0 = C.a00 + 0.3f, c1 = C.a01, c2 = C.a11 + 0.3f;
    const float det_blur = c0 * c2 - c1 * c1;
    float comp = sqrtf(fmaxf(0.f, det_orig / det_blur));
    if constexpr (FISH) {  // det (C + 0.3 I) = det C + 0.3 tr C + 0.09: positive terms only
      if (scales) comp = sqrtf(fish_det / (fish_det + 0.3f * (C.a00 + C.a11) + 0.09f));
    }

    float k0, k1, k2, radius;
    if (gsr_cov2d_bounds(c0, c1, c2, k0, k1, k2, radius)) {
      o_k0 = k0;
      o_k1 = k1;
      o_k2 = k2;
      float u, v;
      if constexpr (FISH) {
        u = fx * fish_s * tx + cx - 0.5f;
        v = fy * fish_s * ty + cy - 0.5f;
      } else {
        const float *P = projmat;
        const float hx = P[0] * px + P[1] * py + P[2] * pz + P[3];
        const float hy = P[4] * px + P[5] * py + P[6] * pz + P[7];
        const float hw = P[12] * px + P[13] * py + P[14] * pz + P[15];
        const float rw = 1.f / (hw + 1e-6f);
        u = 0.5f * (float)img_w * (hx * rw) + cx - 0.5f;
        v = 0.5f * (float)img_h * (hy * rw) + cy - 0.5f;
      }
      int minx, miny, maxx, maxy;
      gsr_tile_bbox(u, v, radius, tiles_x, tiles_y, 0.f, bw, minx, miny, maxx, maxy);
      const int area = (maxx - minx) * (maxy - miny);
      if (area > 0) {
        o_tiles = area;
        o_depth = tz;
        o_radius = (int)radius;
        o_x = u;
        o_y = v;
        o_comp = comp;
      }
    }
  }

  if constexpr (FISH) {  // every output of a culled Gaussian is zero (the pinhole entries keep the covariance and the
    if (o_tiles == 0) {  // conic of one that passed the near plane and was culled later, as the reference's kernel does)
#pragma unroll
      for (int k = 0; k < 6; ++k) o_cov[k] = 0.f;
      o_k0 = o_k1 = o_k2 = 0.f;
    }
  }
  if (scales) {
#pragma unroll
    for (int k = 0; k < 6; ++k) gsr_store_stream(cov3d + 6 * i + k, o_cov[k]);  // (read again by the backward only)
  }
  xys[2 * i] = o_x;
  xys[2 * i + 1] = o_y;
  depths[i] = o_depth;
  radii[i] = o_radius;
  conics[3 * i] = o_k0;
  conics[3 * i + 1] = o_k1;
  conics[3 * i + 2] = o_k2;
  gsr_store_stream(compensation + i, o_comp);
  num_tiles_hit[i] = o_tiles;
  if constexpr (AA) {
    const FwdAA &a = fwd_first(aa...);
    gsr_store_stream(a.opacities_aa + i, a.opacities[i] * o_comp);  // (culled or cropped: x * 0)
  }
}

// What the chain of project_bwd_kernel holds for one VISIBLE Gaussian between the cotangents and v_mean3d: shared
// with project_pose_partial_kernel (the camera gradients are sums of these terms), so that both kernels evaluate
// every expression in the same float32 operations and order.
struct BwdChain {
  float px, py, pz;     // the centre
  float vt0, vt1, vt3;  // cotangent of rows 0, 1, 3 of P p~
  float vz;             // cotangent of depth = V[2,:] . p~
  float vtx, vty, vtz;  // cotangent of the view-space centre t = V p~ through J
  float j00, j02, j11, j12;  // the non-zero entries of J
  M3 vT;                // cotangent of T = J W
  float g2[3], g3[6], gm[3];
};

// AA: `v_comp_aa` (= v_opacities_aa * opacities, the antialiased opacity's share) is added to the compensation's
// cotangent in float32, in front of its scaling.
// FISH: the equidistant fisheye's centre and Jacobian (header); the camera-gradient fields (vt0, vt1, vt3) stay zero.
template <bool AA = false, bool FISH = false>
__device__ __forceinline__ void project_bwd_chain(
    const int i, const float *__restrict__ means3d, const float *__restrict__ viewmat,
    const float *__restrict__ projmat, const float fx, const float fy, const int img_w, const int img_h,
    const float *__restrict__ cov3d, const float *__restrict__ conics, const float *__restrict__ compensation,
    const float *__restrict__ v_xy, const float *__restrict__ v_depth, const float *__restrict__ v_conic,
    const float *__restrict__ v_compensation, BwdChain &c, const float v_comp_aa = 0.f) {
  float *const g2 = c.g2, *const g3 = c.g3, *const gm = c.gm;
  const float px = means3d[3 * i], py = means3d[3 * i + 1], pz = means3d[3 * i + 2];
  const float *P = projmat;
  const float *V = viewmat;

  float vt0 = 0.f, vt1 = 0.f, vt3 = 0.f;
  if constexpr (FISH) {
    gm[0] = gm[1] = gm[2] = 0.f;  // (the centre's share joins v_t below, through J)
  } else {
    // pixel = ndc2pix(P p / (w + eps))  ->  d/dp  (helpers.cuh:125-142)
    const float hx = P[0] * px + P[1] * py + P[2] * pz + P[3];
    const float hy = P[4] * px + P[5] * py + P[6] * pz + P[7];
    const float hw = P[12] * px + P[13] * py + P[14] * pz + P[15];
    const float rw = 1.f / (hw + 1e-6f);
    const float vnx = v_xy ? 0.5f * (float)img_w * v_xy[2 * i] : 0.f;
    const float vny = v_xy ? 0.5f * (float)img_h * v_xy[2 * i + 1] : 0.f;
    vt0 = vnx * rw;
    vt1 = vny * rw;
    vt3 = -(vnx * hx + vny * hy) * rw * rw;
    gm[0] = P[0] * vt0 + P[4] * vt1 + P[12] * vt3;
    gm[1] = P[1] * vt0 + P[5] * vt1 + P[13] * vt3;
    gm[2] = P[2] * vt0 + P[6] * vt1 + P[14] * vt3;
  }

  // depth = V[2,:] . p
  const float vz = v_depth ? v_depth[i] : 0.f;
  gm[0] += V[8] * vz;
  gm[1] += V[9] * vz;
  gm[2] += V[10] * vz;

  // conic = inv(cov2d)  ->  v_cov2d = -X G X  (helpers.cuh:62-74)
  const float X00 = conics[3 * i], X01 = conics[3 * i + 1], X11 = conics[3 * i + 2];
  const float G00 = v_conic ? v_conic[3 * i] : 0.f, G01 = v_conic ? 0.5f * v_conic[3 * i + 1] : 0.f,
              G11 = v_conic ? v_conic[3 * i + 2] : 0.f;
  const float A00 = X00 * G00 + X01 * G01, A01 = X00 * G01 + X01 * G11;
  const float A10 = X01 * G00 + X11 * G01, A11 = X01 * G01 + X11 * G11;
  g2[0] = -(A00 * X00 + A01 * X01);
  g2[1] = -(A00 * X01 + A01 * X11) - (A10 * X00 + A11 * X01);
  g2[2] = -(A10 * X01 + A11 * X11);

  // compensation = sqrt(det(cov2d - 0.3 I) / det(cov2d))  (helpers.cuh:76-90)
  {
    const float comp = compensation[i];
    const float inv_det = X00 * X11 - X01 * X01;
    const float om2 = 1.f - comp * comp;
    const float vsq = (AA ? (v_compensation ? v_compensation[i] + v_comp_aa : v_comp_aa)
                          : (v_compensation ? v_compensation[i] : 0.f)) * 0.5f / (comp + 1e-6f);
    g2[0] += vsq * (om2 * X00 - 0.3f * inv_det);
    g2[1] += 2.f * vsq * (om2 * X01);
    g2[2] += vsq * (om2 * X11 - 0.3f * inv_det);
  }

  // cov2d = T V T^T, T = J W  (backward.cu:350-423; no fov clamp here)
  const M3 W{V[0], V[1], V[2], V[4], V[5], V[6], V[8], V[9], V[10]};
  const float tx = V[0] * px + V[1] * py + V[2] * pz + V[3];
  const float ty = V[4] * px + V[5] * py + V[6] * pz + V[7];
  const float tz = V[8] * px + V[9] * py + V[10] * pz + V[11];
  [[maybe_unused]] const float rz = 1.f / tz, rz2 = rz * rz, rz3 = rz2 * rz;
  M3 J;
  [[maybe_unused]] Fisheye f;
  if constexpr (FISH) {
    f = fisheye_terms<true>(tx, ty, tz);
    const float xyc = tx * ty * f.c;
    J = M3{fx * (f.s + tx * tx * f.c), fx * xyc, -fx * tx * f.w, fy * xyc, fy * (f.s + ty * ty * f.c), -fy * ty * f.w,
           0.f, 0.f, 0.f};
  } else {
    J = M3{fx * rz, 0.f, -fx * tx * rz2, 0.f, fy * rz, -fy * ty * rz2, 0.f, 0.f, 0.f};
  }
  const float *c3 = cov3d + 6 * i;
  const M3 Vs{c3[0], c3[1], c3[2], c3[1], c3[3], c3[4], c3[2], c3[4], c3[5]};
  const M3 Gc{g2[0], 0.5f * g2[1], 0.f, 0.5f * g2[1], g2[2], 0.f, 0.f, 0.f, 0.f};
  const M3 T = mul(J, W);
  const M3 vV = mul(mul(transpose(T), Gc), T);
  g3[0] = vV.a00;
  g3[1] = vV.a01 + vV.a10;
  g3[2] = vV.a02 + vV.a20;
  g3[3] = vV.a11;
  g3[4] = vV.a12 + vV.a21;
  g3[5] = vV.a22;
  // v_T = G T V^T + G^T T V
  const M3 P1 = mul(mul(Gc, T), transpose(Vs));
  const M3 P2 = mul(mul(transpose(Gc), T), Vs);
  const M3 vT{P1.a00 + P2.a00, P1.a01 + P2.a01, P1.a02 + P2.a02,
              P1.a10 + P2.a10, P1.a11 + P2.a11, P1.a12 + P2.a12,
              P1.a20 + P2.a20, P1.a21 + P2.a21, P1.a22 + P2.a22};
  const M3 vJ = mul(vT, transpose(W));
  float vtx, vty, vtz;
  if constexpr (FISH) {
    // sum(v_J * J) = ae s + m c - ct w with ae, m, ct below; s, c, w are functions of (r^2, tz) with
    // ds/dtx = tx c, dc/dtx = 2 tx cu, dw/dtx = -2 tx w^2 (ty alike), ds/dtz = -w, dc/dtz = 2 w^2, dw/dtz = -2 tz w^2
    const float A = fx * vJ.a00, B = fx * vJ.a01 + fy * vJ.a10, E = fy * vJ.a11;
    const float Cx = fx * vJ.a02, Cy = fy * vJ.a12;
    const float ae = A + E;
    const float m = A * tx * tx + B * tx * ty + E * ty * ty;
    const float ct = Cx * tx + Cy * ty;
    const float w2 = f.w * f.w;
    const float k = ae * f.c + 2.f * m * f.cu + 2.f * ct * w2;  // the factor of tx (ty) the three radial terms share
    vtx = tx * k + (2.f * A * tx + B * ty) * f.c - Cx * f.w;
    vty = ty * k + (B * tx + 2.f * E * ty) * f.c - Cy * f.w;
    vtz = -ae * f.w + 2.f * m * w2 + 2.f * ct * tz * w2;
    // xy = (fx s tx, fy s ty) + const:  v_t += J^T v_xy
    const float vx = v_xy ? v_xy[2 * i] : 0.f, vy = v_xy ? v_xy[2 * i + 1] : 0.f;
    vtx += J.a00 * vx + J.a10 * vy;
    vty += J.a01 * vx + J.a11 * vy;
    vtz += J.a02 * vx + J.a12 * vy;
  } else {
    vtx = -fx * rz2 * vJ.a02;
    vty = -fy * rz2 * vJ.a12;
    vtz = -fx * rz2 * vJ.a00 + 2.f * fx * tx * rz3 * vJ.a02 -
          fy * rz2 * vJ.a11 + 2.f * fy * ty * rz3 * vJ.a12;
  }
  gm[0] += vtx * W.a00 + vty * W.a10 + vtz * W.a20;
  gm[1] += vtx * W.a01 + vty * W.a11 + vtz * W.a21;
  gm[2] += vtx * W.a02 + vty * W.a12 + vtz * W.a22;

  c.px = px; c.py = py; c.pz = pz;
  c.vt0 = vt0; c.vt1 = vt1; c.vt3 = vt3;
  c.vz = vz;
  c.vtx = vtx; c.vty = vty; c.vtz = vtz;
  c.j00 = J.a00; c.j02 = J.a02; c.j11 = J.a11; c.j12 = J.a12;
  c.vT = vT;
}

struct BwdAA {  // (v_opacities may be v_opacities_aa itself: read before the write)
  const float *opacities, *v_opacities_aa;
  float *v_opacities, *v_compensation_out;
};
template <bool AA, bool FISH, typename... X>  // X: nothing, or BwdAA
__global__ __launch_bounds__(256) void project_bwd_kernel(
    const int n, const float *__restrict__ means3d,
    const float *__restrict__ scales, const float glob_scale,
    const float *__restrict__ quats, const float *__restrict__ viewmat,
    const float *__restrict__ projmat, const float fx, const float fy,
    const int img_w, const int img_h, const float *__restrict__ cov3d,
    const int *__restrict__ radii, const float *__restrict__ conics,
    const float *__restrict__ compensation, const float *__restrict__ v_xy,
    const float *__restrict__ v_depth, const float *__restrict__ v_conic,
    const float *__restrict__ v_compensation, float *__restrict__ v_cov2d,
    float *__restrict__ v_cov3d, float *__restrict__ v_mean3d,
    float *__restrict__ v_scale, float *__restrict__ v_quat, const X... aa) {
  static_assert(AA == (sizeof...(X) == 1), "project_bwd_kernel<true, FISH, BwdAA> or project_bwd_kernel<false, FISH>");
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;

  float v_oaa = 0.f, v_comp_aa = 0.f;
  if constexpr (AA) {
    const BwdAA &a = (aa, ...);
    v_oaa = a.v_opacities_aa[i];
    v_comp_aa = v_oaa * a.opacities[i];
  }

  BwdChain c;
  float *const g2 = c.g2, *const g3 = c.g3, *const gm = c.gm;
  g2[0] = g2[1] = g2[2] = 0.f;
  g3[0] = g3[1] = g3[2] = g3[3] = g3[4] = g3[5] = 0.f;
  gm[0] = gm[1] = gm[2] = 0.f;
  float gs[3] = {0.f, 0.f, 0.f};
  float gq[4] = {0.f, 0.f, 0.f, 0.f};

  if (radii[i] > 0) {
    project_bwd_chain<AA, FISH>(i, means3d, viewmat, projmat, fx, fy, img_w, img_h, cov3d, conics, compensation, v_xy,
                          v_depth, v_conic, v_compensation, c, v_comp_aa);

    // cov3d = M M^T, M = R S  (backward.cu:427-453)
    const M3 vS{g3[0], 0.5f * g3[1], 0.5f * g3[2], 0.5f * g3[1], g3[3],
                0.5f * g3[4], 0.5f * g3[2], 0.5f * g3[4], g3[5]};
    if (scales) {  // (precomputed covariances: the chain ends at v_cov3d)
    float w, x, y, z;
    const M3 R = quat_to_rot(quats[4 * i], quats[4 * i + 1], quats[4 * i + 2],
                             quats[4 * i + 3], w, x, y, z);
    const float s0 = glob_scale * scales[3 * i], s1 = glob_scale * scales[3 * i + 1],
                s2 = glob_scale * scales[3 * i + 2];
    const M3 M{R.a00 * s0, R.a01 * s1, R.a02 * s2, R.a10 * s0, R.a11 * s1,
               R.a12 * s2, R.a20 * s0, R.a21 * s1, R.a22 * s2};
    M3 vM = mul(vS, M);
    vM.a00 *= 2.f; vM.a01 *= 2.f; vM.a02 *= 2.f;
    vM.a10 *= 2.f; vM.a11 *= 2.f; vM.a12 *= 2.f;
    vM.a20 *= 2.f; vM.a21 *= 2.f; vM.a22 *= 2.f;
    gs[0] = (R.a00 * vM.a00 + R.a10 * vM.a10 + R.a20 * vM.a20) * glob_scale;
    gs[1] = (R.a01 * vM.a01 + R.a11 * vM.a11 + R.a21 * vM.a21) * glob_scale;
    gs[2] = (R.a02 * vM.a02 + R.a12 * vM.a12 + R.a22 * vM.a22) * glob_scale;
    const M3 vR{vM.a00 * s0, vM.a01 * s1, vM.a02 * s2, vM.a10 * s0, vM.a11 * s1,
                vM.a12 * s2, vM.a20 * s0, vM.a21 * s1, vM.a22 * s2};
    // d(R)/d(q) with q treated as unit (helpers.cuh:161-200)
    gq[0] = 2.f * (x * (vR.a21 - vR.a12) + y * (vR.a02 - vR.a20) + z * (vR.a10 - vR.a01));
    gq[1] = 2.f * (-2.f * x * (vR.a11 + vR.a22) + y * (vR.a10 + vR.a01) +
                   z * (vR.a20 + vR.a02) + w * (vR.a21 - vR.a12));
    gq[2] = 2.f * (x * (vR.a10 + vR.a01) - 2.f * y * (vR.a00 + vR.a22) +
                   z * (vR.a21 + vR.a12) + w * (vR.a02 - vR.a20));
    gq[3] = 2.f * (x * (vR.a20 + vR.a02) + y * (vR.a21 + vR.a12) -
                   2.f * z * (vR.a00 + vR.a11) + w * (vR.a10 - vR.a01));
    }
  }

#pragma unroll
  for (int k = 0; k < 3; ++k) gsr_store_stream(v_cov2d + 3 * i + k, g2[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) gsr_store_stream(v_cov3d + 6 * i + k, g3[k]);  // (scratch of the chain: nobody reads it)
#pragma unroll
  for (int k = 0; k < 3; ++k) gsr_store_stream(v_mean3d + 3 * i + k, gm[k]);
  if (scales) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v_scale[3 * i + k] = gs[k];  // (read next by the activation backward)
#pragma unroll
    for (int k = 0; k < 4; ++k) v_quat[4 * i + k] = gq[k];
  }
  if constexpr (AA) {
    const BwdAA &a = (aa, ...);
    a.v_opacities[i] = v_oaa * compensation[i];  // (read next by the activation backward; culled: x * 0)
    if (a.v_compensation_out)  // the cotangent the chain took, for gsr_project_backward_pose
      gsr_store_stream(a.v_compensation_out + i, v_compensation ? v_compensation[i] + v_comp_aa : v_comp_aa);
  }
}

// ---- camera gradients ------------------------------------------------------------------
// v_viewmat [3,4] and v_projmat [4,4] are sums over the visible Gaussians of terms project_bwd_chain already holds:
//   v_projmat[r,:]  = sum vt_r p~            r = 0, 1, 3 (row 2 is never read by the forward: exactly zero)
//   v_viewmat[r,:]  = sum v_t[r] p~  (+ v_depth p~ for r = 2)  +  [ (J^T vT)[r,:3], 0 ]
// The chain's factors are the float32 numbers project_bwd_kernel forms; their products (exact in float64) and the
// 24 sums are float64: per lane over the GSR_POSE_PER_LANE Gaussians of the lane, then wave (xor butterfly) ->
// workgroup (the four waves in order, through LDS) -> grid (project_pose_final_kernel over the per-workgroup
// partials), every step in a fixed order and no atomics, rounded to float32 once.
#define GSR_POSE_SUMS 24
#define GSR_POSE_PER_LANE 4
#define GSR_POSE_SHARE (256 * GSR_POSE_PER_LANE)  // Gaussians per workgroup

__device__ __forceinline__ double pose_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < GSR_WAVE; m <<= 1) v += __shfl_xor(v, m, GSR_WAVE);
  return v;  // (the same bits in every lane: a + b and b + a round alike)
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void project_pose_partial_kernel(
    const int n, const float *__restrict__ means3d, const float *__restrict__ viewmat,
    const float *__restrict__ projmat, const float fx, const float fy, const int img_w, const int img_h,
    const float *__restrict__ cov3d, const int *__restrict__ radii, const float *__restrict__ conics,
    const float *__restrict__ compensation, const float *__restrict__ v_xy, const float *__restrict__ v_depth,
    const float *__restrict__ v_conic, const float *__restrict__ v_compensation, double *__restrict__ partials) {
  __shared__ double wave_sums[4][GSR_POSE_SUMS];
  double acc[GSR_POSE_SUMS];  // [0,12): v_viewmat row-major; [12,24): rows 0, 1, 3 of v_projmat
#pragma unroll
  for (int k = 0; k < GSR_POSE_SUMS; ++k) acc[k] = 0.0;

  const long long base = (long long)blockIdx.x * GSR_POSE_SHARE + threadIdx.x;
#pragma unroll 1
  for (int j = 0; j < GSR_POSE_PER_LANE; ++j) {
    const long long ii = base + (long long)j * 256;
    if (ii >= n) break;
    const int i = (int)ii;
    if (radii[i] <= 0) continue;
    BwdChain c;
    project_bwd_chain(i, means3d, viewmat, projmat, fx, fy, img_w, img_h, cov3d, conics, compensation, v_xy, v_depth,
                      v_conic, v_compensation, c);
    const double p[4] = {(double)c.px, (double)c.py, (double)c.pz, 1.0};
    const double vt[3] = {(double)c.vtx, (double)c.vty, (double)c.vtz + (double)c.vz};
    const double vp[3] = {(double)c.vt0, (double)c.vt1, (double)c.vt3};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[4 * r + q] += vt[r] * p[q];
        acc[12 + 4 * r + q] += vp[r] * p[q];
      }
    }
    // v_W = J^T vT (rows 0 and 1 of J only)
    const double j00 = c.j00, j02 = c.j02, j11 = c.j11, j12 = c.j12;
    const double t0[3] = {(double)c.vT.a00, (double)c.vT.a01, (double)c.vT.a02};
    const double t1[3] = {(double)c.vT.a10, (double)c.vT.a11, (double)c.vT.a12};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      acc[q] += j00 * t0[q];
      acc[4 + q] += j11 * t1[q];
      acc[8 + q] += j02 * t0[q] + j12 * t1[q];
    }
  }

  const int wave = threadIdx.x / GSR_WAVE, lane = threadIdx.x % GSR_WAVE;
#pragma unroll
  for (int k = 0; k < GSR_POSE_SUMS; ++k) {
    const double s = pose_wave_sum(acc[k]);
    if (lane == 0) wave_sums[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < GSR_POSE_SUMS) {
    const int k = threadIdx.x;
    partials[(size_t)blockIdx.x * GSR_POSE_SUMS + k] =
        ((wave_sums[0][k] + wave_sums[1][k]) + wave_sums[2][k]) + wave_sums[3][k];
  }
}

// One workgroup: wave w owns the sums 6 w .. 6 w + 5; lane l adds the partials l, l + 64, l + 128, ... in that
// order, the wave's butterfly adds the lanes.
__global__ __launch_bounds__(256) void project_pose_final_kernel(
    const int num_partials, const double *__restrict__ partials, float *__restrict__ v_viewmat,
    float *__restrict__ v_projmat) {
  const int wave = threadIdx.x / GSR_WAVE, lane = threadIdx.x % GSR_WAVE;
#pragma unroll 1
  for (int s = 0; s < GSR_POSE_SUMS / 4; ++s) {
    const int k = wave * (GSR_POSE_SUMS / 4) + s;
    double a = 0.0;
    for (int b = lane; b < num_partials; b += GSR_WAVE) a += partials[(size_t)b * GSR_POSE_SUMS + k];
    a = pose_wave_sum(a);
    if (lane == 0) {
      if (k < 12) {
        v_viewmat[k] = (float)a;
      } else {
        const int r = (k - 12) / 4, q = (k - 12) % 4;
        v_projmat[4 * (r == 2 ? 3 : r) + q] = (float)a;
      }
    }
  }
  if (threadIdx.x < 4) v_projmat[8 + threadIdx.x] = 0.f;
}

__global__ __launch_bounds__(256) void cov2d_bounds_kernel(
    const int n, const float *__restrict__ cov2d, float *__restrict__ conics,
    float *__restrict__ radii) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float k0 = 0.f, k1 = 0.f, k2 = 0.f, r = 0.f;
  gsr_cov2d_bounds(cov2d[3 * i], cov2d[3 * i + 1], cov2d[3 * i + 2], k0, k1, k2, r);
  conics[3 * i] = k0;
  conics[3 * i + 1] = k1;
  conics[3 * i + 2] = k2;
  radii[i] = r;
}

// mask[i] = centre i is inside the crop box, by the projection's own rule.  count (nullable, zeroed by the entry
// point): one ballot + popcount per wave, the four waves' counts through LDS, one integer atomic per workgroup.
__global__ __launch_bounds__(256) void crop_mask_kernel(const int n, const float *__restrict__ means3d,
                                                        const float *__restrict__ crop, uint8_t *__restrict__ mask,
                                                        int *__restrict__ count) {
  __shared__ int wave_counts[256 / GSR_WAVE];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool in = false;
  if (i < n) {
    const size_t o = 3 * (size_t)i;
    in = gsr_crop_inside(crop, means3d[o], means3d[o + 1], means3d[o + 2]);
    mask[i] = in ? 1 : 0;
  }
  if (count == nullptr) return;  // (uniform over the grid)
  const unsigned long long inside = __ballot(in);
  if (threadIdx.x % GSR_WAVE == 0) wave_counts[threadIdx.x / GSR_WAVE] = __popcll(inside);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int c = (wave_counts[0] + wave_counts[1]) + (wave_counts[2] + wave_counts[3]);
    if (c > 0) atomicAdd(count, c);
  }
}

}  // namespace

GSR_EXPORT int gsr_project_forward(
    int num_points, const float *means3d, const float *scales, float glob_scale,
    const float *quats, const float *viewmat, const float *projmat, float fx,
    float fy, float cx, float cy, unsigned img_height, unsigned img_width,
    unsigned block_width, float clip_thresh, float *cov3d, float *xys,
    float *depths, int32_t *radii, float *conics, float *compensation,
    int32_t *num_tiles_hit, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "project_forward: num_points < 0");
  GSR_REQUIRE(block_width >= 2 && block_width <= 16, "project_forward: block_width must be in [2,16]");
  GSR_REQUIRE(img_height > 0 && img_width > 0, "project_forward: empty image");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && viewmat && projmat && cov3d && xys && depths &&
                  radii && conics && compensation && num_tiles_hit,
              "project_forward: null pointer");
  GSR_REQUIRE((scales == nullptr) == (quats == nullptr),
              "project_forward: pass both scales and quats, or neither (cov3d is then an input)");
  const int tiles_x = (int)gsr_cdiv(img_width, block_width);
  const int tiles_y = (int)gsr_cdiv(img_height, block_width);
  hipLaunchKernelGGL((project_fwd_kernel<false, false, false>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                     (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                     viewmat, projmat, fx, fy, cx, cy, (int)img_width, (int)img_height,
                     tiles_x, tiles_y, (int)block_width, clip_thresh, cov3d, xys, depths,
                     radii, conics, compensation, num_tiles_hit);
  GSR_CHECK_LAUNCH("project_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_project_forward_aa(
    int num_points, const float *means3d, const float *scales, float glob_scale,
    const float *quats, const float *viewmat, const float *projmat, float fx,
    float fy, float cx, float cy, unsigned img_height, unsigned img_width,
    unsigned block_width, float clip_thresh, const float *opacities, float *cov3d, float *xys,
    float *depths, int32_t *radii, float *conics, float *compensation,
    int32_t *num_tiles_hit, float *opacities_aa, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "project_forward_aa: num_points < 0");
  GSR_REQUIRE(block_width >= 2 && block_width <= 16, "project_forward_aa: block_width must be in [2,16]");
  GSR_REQUIRE(img_height > 0 && img_width > 0, "project_forward_aa: empty image");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && viewmat && projmat && cov3d && xys && depths &&
                  radii && conics && compensation && num_tiles_hit && opacities && opacities_aa,
              "project_forward_aa: null pointer");
  GSR_REQUIRE((scales == nullptr) == (quats == nullptr),
              "project_forward_aa: pass both scales and quats, or neither (cov3d is then an input)");
  const int tiles_x = (int)gsr_cdiv(img_width, block_width);
  const int tiles_y = (int)gsr_cdiv(img_height, block_width);
  hipLaunchKernelGGL((project_fwd_kernel<true, false, false, FwdAA>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                     (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                     viewmat, projmat, fx, fy, cx, cy, (int)img_width, (int)img_height,
                     tiles_x, tiles_y, (int)block_width, clip_thresh, cov3d, xys, depths,
                     radii, conics, compensation, num_tiles_hit, FwdAA{opacities, opacities_aa});
  GSR_CHECK_LAUNCH("project_forward_aa");
  return GSR_OK;
}

GSR_EXPORT int gsr_project_forward_crop(
    int num_points, const float *means3d, const float *scales, float glob_scale,
    const float *quats, const float *viewmat, const float *projmat, float fx,
    float fy, float cx, float cy, unsigned img_height, unsigned img_width,
    unsigned block_width, float clip_thresh, const float *crop, const float *opacities, float *cov3d,
    float *xys, float *depths, int32_t *radii, float *conics, float *compensation,
    int32_t *num_tiles_hit, float *opacities_aa, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "project_forward_crop: num_points < 0");
  GSR_REQUIRE(block_width >= 2 && block_width <= 16, "project_forward_crop: block_width must be in [2,16]");
  GSR_REQUIRE(img_height > 0 && img_width > 0, "project_forward_crop: empty image");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && viewmat && projmat && cov3d && xys && depths &&
                  radii && conics && compensation && num_tiles_hit && crop,
              "project_forward_crop: null pointer");
  GSR_REQUIRE((opacities == nullptr) == (opacities_aa == nullptr),
              "project_forward_crop: pass both opacities and opacities_aa, or neither");
  GSR_REQUIRE((scales == nullptr) == (quats == nullptr),
              "project_forward_crop: pass both scales and quats, or neither (cov3d is then an input)");
  const int tiles_x = (int)gsr_cdiv(img_width, block_width);
  const int tiles_y = (int)gsr_cdiv(img_height, block_width);
  if (opacities) {
    hipLaunchKernelGGL((project_fwd_kernel<true, true, false, FwdAA, FwdCrop>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                       (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                       viewmat, projmat, fx, fy, cx, cy, (int)img_width, (int)img_height,
                       tiles_x, tiles_y, (int)block_width, clip_thresh, cov3d, xys, depths,
                       radii, conics, compensation, num_tiles_hit, FwdAA{opacities, opacities_aa}, FwdCrop{crop});
  } else {
    hipLaunchKernelGGL((project_fwd_kernel<false, true, false, FwdCrop>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                       (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                       viewmat, projmat, fx, fy, cx, cy, (int)img_width, (int)img_height,
                       tiles_x, tiles_y, (int)block_width, clip_thresh, cov3d, xys, depths,
                       radii, conics, compensation, num_tiles_hit, FwdCrop{crop});
  }
  GSR_CHECK_LAUNCH("project_forward_crop");
  return GSR_OK;
}

GSR_EXPORT int gsr_crop_mask(int num_points, const float *means3d, const float *crop, uint8_t *mask,
                             int32_t *count, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "crop_mask: num_points < 0");
  if (count != nullptr)
    if (int rc = gsr_zero_async(count, sizeof(int32_t), (hipStream_t)stream)) return rc;
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && crop && mask, "crop_mask: null pointer");
  hipLaunchKernelGGL(crop_mask_kernel, dim3(gsr_cdiv(num_points, 256)), dim3(256), 0, (hipStream_t)stream,
                     num_points, means3d, crop, mask, count);
  GSR_CHECK_LAUNCH("crop_mask");
  return GSR_OK;
}

GSR_EXPORT int gsr_project_backward(
    int num_points, const float *means3d, const float *scales, float glob_scale,
    const float *quats, const float *viewmat, const float *projmat, float fx,
    float fy, float cx, float cy, unsigned img_height, unsigned img_width,
    const float *cov3d, const int32_t *radii, const float *conics,
    const float *compensation, const float *v_xy, const float *v_depth,
    const float *v_conic, const float *v_compensation, float *v_cov2d,
    float *v_cov3d, float *v_mean3d, float *v_scale, float *v_quat,
    gsr_stream_t stream) {
  (void)cx;
  (void)cy;
  GSR_REQUIRE(num_points >= 0, "project_backward: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && viewmat && projmat && cov3d && radii && conics && compensation && v_cov2d &&
                  v_cov3d && v_mean3d,
              "project_backward: null pointer");
  GSR_REQUIRE((scales == nullptr) == (quats == nullptr), "project_backward: pass both scales and quats, or neither");
  GSR_REQUIRE(scales == nullptr || (v_scale && v_quat), "project_backward: null pointer");
  hipLaunchKernelGGL((project_bwd_kernel<false, false>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                     (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                     viewmat, projmat, fx, fy, (int)img_width, (int)img_height, cov3d, radii,
                     conics, compensation, v_xy, v_depth, v_conic, v_compensation, v_cov2d,
                     v_cov3d, v_mean3d, v_scale, v_quat);
  GSR_CHECK_LAUNCH("project_backward");
  return GSR_OK;
}

GSR_EXPORT int gsr_project_backward_aa(
    int num_points, const float *means3d, const float *scales, float glob_scale,
    const float *quats, const float *viewmat, const float *projmat, float fx,
    float fy, float cx, float cy, unsigned img_height, unsigned img_width,
    const float *cov3d, const int32_t *radii, const float *conics,
    const float *compensation, const float *opacities, const float *v_xy, const float *v_depth,
    const float *v_conic, const float *v_compensation, const float *v_opacities_aa, float *v_cov2d,
    float *v_cov3d, float *v_mean3d, float *v_scale, float *v_quat, float *v_opacities,
    float *v_compensation_out, gsr_stream_t stream) {
  (void)cx;
  (void)cy;
  GSR_REQUIRE(num_points >= 0, "project_backward_aa: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && viewmat && projmat && cov3d && radii && conics && compensation && opacities &&
                  v_opacities_aa && v_cov2d && v_cov3d && v_mean3d && v_opacities,
              "project_backward_aa: null pointer");
  GSR_REQUIRE((scales == nullptr) == (quats == nullptr), "project_backward_aa: pass both scales and quats, or neither");
  GSR_REQUIRE(scales == nullptr || (v_scale && v_quat), "project_backward_aa: null pointer");
  // (v_opacities may be v_opacities_aa itself; nothing else may overlap what the kernel still reads)
  GSR_REQUIRE(v_compensation_out == nullptr || v_compensation_out != v_compensation,
              "project_backward_aa: v_compensation_out must not alias v_compensation");
  hipLaunchKernelGGL((project_bwd_kernel<true, false, BwdAA>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                     (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                     viewmat, projmat, fx, fy, (int)img_width, (int)img_height, cov3d, radii,
                     conics, compensation, v_xy, v_depth, v_conic, v_compensation, v_cov2d,
                     v_cov3d, v_mean3d, v_scale, v_quat,
                     BwdAA{opacities, v_opacities_aa, v_opacities, v_compensation_out});
  GSR_CHECK_LAUNCH("project_backward_aa");
  return GSR_OK;
}

// The fisheye entries: one each way for both rasterize modes (opacities / opacities_aa, and the backward's
// opacities / v_opacities_aa / v_opacities, all NULL: the classic mode).
GSR_EXPORT int gsr_project_forward_fisheye(
    int num_points, const float *means3d, const float *scales, float glob_scale,
    const float *quats, const float *viewmat, const float *projmat, float fx,
    float fy, float cx, float cy, unsigned img_height, unsigned img_width,
    unsigned block_width, float clip_thresh, const float *opacities, float *cov3d, float *xys,
    float *depths, int32_t *radii, float *conics, float *compensation,
    int32_t *num_tiles_hit, float *opacities_aa, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "project_forward_fisheye: num_points < 0");
  GSR_REQUIRE(block_width >= 2 && block_width <= 16, "project_forward_fisheye: block_width must be in [2,16]");
  GSR_REQUIRE(img_height > 0 && img_width > 0, "project_forward_fisheye: empty image");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && viewmat && cov3d && xys && depths && radii && conics && compensation && num_tiles_hit,
              "project_forward_fisheye: null pointer");  // (projmat is not read)
  GSR_REQUIRE((opacities == nullptr) == (opacities_aa == nullptr),
              "project_forward_fisheye: pass both opacities and opacities_aa, or neither");
  GSR_REQUIRE((scales == nullptr) == (quats == nullptr),
              "project_forward_fisheye: pass both scales and quats, or neither (cov3d is then an input)");
  const int tiles_x = (int)gsr_cdiv(img_width, block_width);
  const int tiles_y = (int)gsr_cdiv(img_height, block_width);
  if (opacities) {
    hipLaunchKernelGGL((project_fwd_kernel<true, false, true, FwdAA>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                       (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                       viewmat, projmat, fx, fy, cx, cy, (int)img_width, (int)img_height,
                       tiles_x, tiles_y, (int)block_width, clip_thresh, cov3d, xys, depths,
                       radii, conics, compensation, num_tiles_hit, FwdAA{opacities, opacities_aa});
  } else {
    hipLaunchKernelGGL((project_fwd_kernel<false, false, true>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                       (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                       viewmat, projmat, fx, fy, cx, cy, (int)img_width, (int)img_height,
                       tiles_x, tiles_y, (int)block_width, clip_thresh, cov3d, xys, depths,
                       radii, conics, compensation, num_tiles_hit);
  }
  GSR_CHECK_LAUNCH("project_forward_fisheye");
  return GSR_OK;
}

GSR_EXPORT int gsr_project_backward_fisheye(
    int num_points, const float *means3d, const float *scales, float glob_scale,
    const float *quats, const float *viewmat, const float *projmat, float fx,
    float fy, float cx, float cy, unsigned img_height, unsigned img_width,
    const float *cov3d, const int32_t *radii, const float *conics,
    const float *compensation, const float *opacities, const float *v_xy, const float *v_depth,
    const float *v_conic, const float *v_compensation, const float *v_opacities_aa, float *v_cov2d,
    float *v_cov3d, float *v_mean3d, float *v_scale, float *v_quat, float *v_opacities,
    float *v_compensation_out, gsr_stream_t stream) {
  (void)cx;
  (void)cy;
  GSR_REQUIRE(num_points >= 0, "project_backward_fisheye: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means3d && viewmat && cov3d && radii && conics && compensation && v_cov2d && v_cov3d && v_mean3d,
              "project_backward_fisheye: null pointer");
  GSR_REQUIRE((opacities == nullptr) == (v_opacities_aa == nullptr) && (opacities == nullptr) == (v_opacities == nullptr),
              "project_backward_fisheye: pass opacities, v_opacities_aa and v_opacities, or none of them");
  GSR_REQUIRE(opacities != nullptr || v_compensation_out == nullptr,
              "project_backward_fisheye: v_compensation_out goes with opacities");
  GSR_REQUIRE((scales == nullptr) == (quats == nullptr), "project_backward_fisheye: pass both scales and quats, or neither");
  GSR_REQUIRE(scales == nullptr || (v_scale && v_quat), "project_backward_fisheye: null pointer");
  GSR_REQUIRE(v_compensation_out == nullptr || v_compensation_out != v_compensation,
              "project_backward_fisheye: v_compensation_out must not alias v_compensation");
  if (opacities) {
    hipLaunchKernelGGL((project_bwd_kernel<true, true, BwdAA>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                       (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                       viewmat, projmat, fx, fy, (int)img_width, (int)img_height, cov3d, radii,
                       conics, compensation, v_xy, v_depth, v_conic, v_compensation, v_cov2d,
                       v_cov3d, v_mean3d, v_scale, v_quat,
                       BwdAA{opacities, v_opacities_aa, v_opacities, v_compensation_out});
  } else {
    hipLaunchKernelGGL((project_bwd_kernel<false, true>), dim3(gsr_cdiv(num_points, 256)), dim3(256), 0,
                       (hipStream_t)stream, num_points, means3d, scales, glob_scale, quats,
                       viewmat, projmat, fx, fy, (int)img_width, (int)img_height, cov3d, radii,
                       conics, compensation, v_xy, v_depth, v_conic, v_compensation, v_cov2d,
                       v_cov3d, v_mean3d, v_scale, v_quat);
  }
  GSR_CHECK_LAUNCH("project_backward_fisheye");
  return GSR_OK;
}

GSR_EXPORT size_t gsr_project_backward_pose_workspace(int num_points) {
  return num_points > 0 ? (size_t)gsr_cdiv((unsigned)num_points, GSR_POSE_SHARE) * GSR_POSE_SUMS * sizeof(double) : 0;
}

GSR_EXPORT int gsr_project_backward_pose(
    int num_points, const float *means3d, const float *viewmat, const float *projmat, float fx, float fy,
    unsigned img_height, unsigned img_width, const float *cov3d, const int32_t *radii, const float *conics,
    const float *compensation, const float *v_xy, const float *v_depth, const float *v_conic,
    const float *v_compensation, void *workspace, size_t workspace_bytes, float *v_viewmat, float *v_projmat,
    gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "project_backward_pose: num_points < 0");
  GSR_REQUIRE(v_viewmat && v_projmat, "project_backward_pose: null pointer");
  if (num_points == 0) {  // no Gaussian, no term: zeros
    if (int rc = gsr_zero_async(v_viewmat, 12 * sizeof(float), (hipStream_t)stream)) return rc;
    return gsr_zero_async(v_projmat, 16 * sizeof(float), (hipStream_t)stream);
  }
  GSR_REQUIRE(means3d && viewmat && projmat && cov3d && radii && conics && compensation && workspace,
              "project_backward_pose: null pointer");
  GSR_REQUIRE(((uintptr_t)workspace & 7u) == 0, "project_backward_pose: workspace must be 8-byte aligned");
  if (workspace_bytes < gsr_project_backward_pose_workspace(num_points)) {
    gsr_set_error("project_backward_pose: workspace of %zu bytes, %zu needed", workspace_bytes,
                  gsr_project_backward_pose_workspace(num_points));
    return GSR_ENOMEM;
  }
  const unsigned blocks = gsr_cdiv((unsigned)num_points, GSR_POSE_SHARE);
  hipLaunchKernelGGL(project_pose_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, num_points,
                     means3d, viewmat, projmat, fx, fy, (int)img_width, (int)img_height, cov3d, radii, conics,
                     compensation, v_xy, v_depth, v_conic, v_compensation, (double *)workspace);
  GSR_CHECK_LAUNCH("project_backward_pose");
  hipLaunchKernelGGL(project_pose_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int)blocks,
                     (const double *)workspace, v_viewmat, v_projmat);
  GSR_CHECK_LAUNCH("project_backward_pose (final)");
  return GSR_OK;
}

GSR_EXPORT int gsr_cov2d_bounds(int num_pts, const float *cov2d, float *conics,
                                float *radii, gsr_stream_t stream) {
  GSR_REQUIRE(num_pts >= 0, "cov2d_bounds: num_pts < 0");
  if (num_pts == 0) return GSR_OK;
  GSR_REQUIRE(cov2d && conics && radii, "cov2d_bounds: null pointer");
  hipLaunchKernelGGL(cov2d_bounds_kernel, dim3(gsr_cdiv(num_pts, 256)), dim3(256), 0,
                     (hipStream_t)stream, num_pts, cov2d, conics, radii);
  GSR_CHECK_LAUNCH("cov2d_bounds");
  return GSR_OK;
}
