// target.hip -- a training step's ground truth from an INTEGER image cache (include/gsraster.h).
// The toolkit keeps every image as float32 and forms a step's target in three passes (get_gt_img, vanilla_gs.py:859-881:
// `image.float() / 255`, bilinear resize, composite over the step's background).  Here the images stay uint8 on the
// device and ONE kernel forms the target: a thread per output pixel converts its four taps, resizes all channels and
// composites -- 4 B read and 12 B written per output pixel at full size.  Integer planes (masks, 16-bit sensor depth,
// 8-bit monocular depth) go through the same kernel with one channel and `value * unit` as the conversion.
//
// Compiled with -ffp-contract=off (Makefile): every product, sum and difference below is rounded on its own and the
// division by 255 is correctly rounded (hipcc's default), so the float32 NumPy restatement of the tests
// (tests/target_reference.py) performs the same operations in the same order and gives the same bits.
//
//   per axis:  s = max(scale * (dst + 0.5) - 0.5, 0)   scale = float(in) / float(out)
//              i0 = int(s)   i1 = i0 + (i0 < in - 1)   l1 = s - i0   l0 = 1 - l1
//   value   :  ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
//   C = 4   :  a * rgb + (1 - a) * background, from the RESIZED rgba
// With out == in the scale is 1, s = dst exactly and l1 = 0: the taps collapse and the value is v00 itself; that case
// takes one tap instead of four (the same bits).  No LDS, no atomics; nothing is differentiated.
#include "gsr_common.h"

namespace {

constexpr int TGT_BX = 64, TGT_BY = 4;  // a wave per output row segment: coalesced taps and stores

struct Axis {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Axis axis_taps(const int dst, const float scale, const int in) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  Axis a;
  a.i0 = min((int)s, in - 1);  // (s <= in - 1 for dst < out <= in up to rounding: the min never changes the tap)
  a.i1 = a.i0 + (a.i0 < in - 1 ? 1 : 0);
  a.l1 = s - (float)a.i0;
  a.l0 = 1.f - a.l1;
  return a;
}

__device__ __forceinline__ float lerp2(const Axis &ax, const Axis &ay, const float v00, const float v01,
                                       const float v10, const float v11) {
  const float top = ax.l0 * v00 + ax.l1 * v01;
  const float bot = ax.l0 * v10 + ax.l1 * v11;
  return ay.l0 * top + ay.l1 * bot;
}

// one tap of C uint8 channels as floats in [0,1]
template <int C>
__device__ __forceinline__ void load_tap(const uint8_t *__restrict__ img, const size_t pixel, float (&v)[C]) {
  if constexpr (C == 4) {
    const uchar4 p = reinterpret_cast<const uchar4 *>(img)[pixel];
    v[0] = (float)p.x / 255.f;
    v[1] = (float)p.y / 255.f;
    v[2] = (float)p.z / 255.f;
    v[3] = (float)p.w / 255.f;
  } else {
    const uint8_t *p = img + pixel * C;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (float)p[c] / 255.f;
  }
}

// C = 3 / 4: uint8 image -> float32 [h,w,3] target.  C = 1: integer plane (T) * unit -> float32 [h,w].
template <int C, typename T>
__global__ __launch_bounds__(TGT_BX *TGT_BY) void target_kernel(const T *__restrict__ src, const int H, const int W,
                                                                const float *__restrict__ background, const float unit,
                                                                const int h, const int w, const float scale_y,
                                                                const float scale_x, float *__restrict__ out) {
  const int x = blockIdx.x * TGT_BX + threadIdx.x, y = blockIdx.y * TGT_BY + threadIdx.y;
  if (x >= w || y >= h) return;
  const bool same = (h == H) && (w == W);  // kernel-uniform
  const size_t o = (size_t)y * w + x;
  if constexpr (C == 1) {
    float val;
    if (same) {
      val = (float)src[o] * unit;
    } else {
      const Axis ax = axis_taps(x, scale_x, W), ay = axis_taps(y, scale_y, H);
      const T *r0 = src + (size_t)ay.i0 * W, *r1 = src + (size_t)ay.i1 * W;
      val = lerp2(ax, ay, (float)r0[ax.i0] * unit, (float)r0[ax.i1] * unit, (float)r1[ax.i0] * unit,
                  (float)r1[ax.i1] * unit);
    }
    out[o] = val;
  } else {
    float v[C];
    const uint8_t *img = reinterpret_cast<const uint8_t *>(src);
    if (same) {
      load_tap<C>(img, o, v);
    } else {
      const Axis ax = axis_taps(x, scale_x, W), ay = axis_taps(y, scale_y, H);
      float v00[C], v01[C], v10[C], v11[C];
      load_tap<C>(img, (size_t)ay.i0 * W + ax.i0, v00);
      load_tap<C>(img, (size_t)ay.i0 * W + ax.i1, v01);
      load_tap<C>(img, (size_t)ay.i1 * W + ax.i0, v10);
      load_tap<C>(img, (size_t)ay.i1 * W + ax.i1, v11);
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = lerp2(ax, ay, v00[c], v01[c], v10[c], v11[c]);
    }
    if constexpr (C == 4) {
      const float a = v[3], na = 1.f - a;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = a * v[c] + na * background[c];
    }
    float *p = out + o * 3;
    p[0] = v[0];
    p[1] = v[1];
    p[2] = v[2];
  }
}

// the sizes every entry accepts: 1 <= out <= in on both axes, the grid within the launch limits
int check_sizes(const char *who, const int H, const int W, const int h, const int w) {
  GSR_REQUIRE(H >= 1 && W >= 1, "%s: the source is %d x %d", who, H, W);
  GSR_REQUIRE(h >= 1 && h <= H && w >= 1 && w <= W, "%s: out_hw (%d, %d) must be within [1, source] = (%d, %d)", who, h,
              w, H, W);
  GSR_REQUIRE(gsr_cdiv((unsigned)h, TGT_BY) <= 65535u, "%s: more than %d output rows", who, 65535 * TGT_BY);
  return GSR_OK;
}

template <int C, typename T>
int launch(const char *who, const T *src, const int H, const int W, const float *background, const float unit,
           const int h, const int w, float *out, hipStream_t s) {
  const dim3 grid(gsr_cdiv((unsigned)w, TGT_BX), gsr_cdiv((unsigned)h, TGT_BY)), block(TGT_BX, TGT_BY);
  hipLaunchKernelGGL((target_kernel<C, T>), grid, block, 0, s, src, H, W, background, unit, h, w,
                     (float)H / (float)h, (float)W / (float)w, out);
  GSR_CHECK_LAUNCH(who);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT int gsr_target_from_u8(const uint8_t *image, int height, int width, int channels, const float *background,
                                  int out_height, int out_width, float *out, gsr_stream_t stream) {
  GSR_REQUIRE(image && out, "target_from_u8: null pointer");
  GSR_REQUIRE(channels == 3 || channels == 4, "target_from_u8: channels must be 3 or 4, got %d", channels);
  GSR_REQUIRE(channels == 3 || background, "target_from_u8: an RGBA image needs a background");
  GSR_REQUIRE(channels == 3 || (reinterpret_cast<uintptr_t>(image) & 3) == 0,
              "target_from_u8: an RGBA image must be 4-byte aligned");
  if (const int rc = check_sizes("target_from_u8", height, width, out_height, out_width)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (channels == 4)
    return launch<4, uint8_t>("target_from_u8", image, height, width, background, 0.f, out_height, out_width, out, s);
  return launch<3, uint8_t>("target_from_u8", image, height, width, background, 0.f, out_height, out_width, out, s);
}

GSR_EXPORT int gsr_plane_from_int(const void *plane, int elem_bytes, int height, int width, float unit, int out_height,
                                  int out_width, float *out, gsr_stream_t stream) {
  GSR_REQUIRE(plane && out, "plane_from_int: null pointer");
  GSR_REQUIRE(elem_bytes == 1 || elem_bytes == 2, "plane_from_int: elements of 1 or 2 bytes, got %d", elem_bytes);
  GSR_REQUIRE(elem_bytes == 1 || (reinterpret_cast<uintptr_t>(plane) & 1) == 0,
              "plane_from_int: a 16-bit plane must be 2-byte aligned");
  if (const int rc = check_sizes("plane_from_int", height, width, out_height, out_width)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (elem_bytes == 2)
    return launch<1, uint16_t>("plane_from_int", static_cast<const uint16_t *>(plane), height, width, nullptr, unit,
                               out_height, out_width, out, s);
  return launch<1, uint8_t>("plane_from_int", static_cast<const uint8_t *>(plane), height, width, nullptr, unit,
                            out_height, out_width, out, s);
}
