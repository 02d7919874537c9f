// contribution.hip -- per-Gaussian statistics of the blend weight w = alpha T over a view: one front-to-back walk over
// the tile lists, forward only (include/gsraster.h, gsr_contribution_accumulate).
//
// Per pixel the walk is the forward compositing's (gsr_common.h thresholds, distortion_fwd_kernel's expressions); for
// every contributing (pixel, entry) pair, w = alpha T in float32 goes into four [N] arrays the caller owns:
//   max_w    = max w                       atomicMax on the float's bits (w > 0: the order of bits is that of values)
//   sum_q    = sum (uint32)(w 2^24)        fixed point, truncated: an integer sum, independent of the order
//   hits     = number of pairs
//   dominant = number of pixels whose largest w is this Gaussian's (strictly greater replaces: front-most wins a tie)
// The launch ADDS to what the arrays hold.  No float atomics: every result is bit-reproducible.
//
// Shape: one 16 x 16 tile per workgroup, one lane per pixel, list entries staged through LDS 256 at a time.  All 64
// lanes of a wave sit on the same entry (as in distortion_bwd_kernel); an entry no lane of the wave contributes to is
// skipped on a ballot.  Per entry, max / quantised sum / count are reduced over each row of 16 lanes with four DPP
// steps, one lane per row updates the batch's accumulators in LDS, and one global atomic per (tile, entry, statistic)
// with a non-zero count closes the batch.  256 * 0.999 * 2^24 < 2^32: a tile's quantised sum fits a uint32 LDS word.
// `dominant`: each lane carries (best w, best list index); after the walk the wave adds once per distinct Gaussian.
// LDS: 7 KB staging + 3 KB accumulators per workgroup.
#include "gsr_common.h"

namespace {

constexpr int BW = 16;
constexpr int BSIZE = BW * BW;
constexpr float Q_SCALE = 16777216.f;  // 2^24

template <int CTRL>
__device__ __forceinline__ unsigned dpp_move(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// sum / max over a row of 16 lanes, in every lane of the row (every lane of the wave is active at the call)
__device__ __forceinline__ unsigned row16_sum(unsigned v) {
  v += dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_move<0x141>(v);  // row_half_mirror
  v += dpp_move<0x140>(v);  // row_mirror
  return v;
}
__device__ __forceinline__ unsigned row16_max(unsigned v) {
  v = max(v, dpp_move<0xB1>(v));
  v = max(v, dpp_move<0x4E>(v));
  v = max(v, dpp_move<0x141>(v));
  v = max(v, dpp_move<0x140>(v));
  return v;
}

__global__ __launch_bounds__(BSIZE) void contribution_kernel(
    const int tiles_x, const int img_w, const int img_h, const int num_points, const int *__restrict__ ids_sorted,
    const int2 *__restrict__ tile_bins, const float2 *__restrict__ xys, const float *__restrict__ conics,
    const float *__restrict__ opacities, unsigned *__restrict__ max_w, unsigned long long *__restrict__ sum_q,
    unsigned long long *__restrict__ hits, unsigned long long *__restrict__ dominant) {
  __shared__ float s_x[BSIZE], s_y[BSIZE], s_o[BSIZE], s_a[BSIZE], s_b[BSIZE], s_c[BSIZE];
  __shared__ int s_id[BSIZE];
  __shared__ unsigned s_max[BSIZE], s_sum[BSIZE], s_hits[BSIZE];

  const int tr = threadIdx.y * BW + threadIdx.x;
  const int lane = tr & 63;
  const int tile = blockIdx.y * tiles_x + blockIdx.x;
  const int col = blockIdx.x * BW + threadIdx.x;
  const int row = blockIdx.y * BW + threadIdx.y;
  const float px = (float)col, py = (float)row;
  bool done = !(col < img_w && row < img_h);  // a lane outside the image contributes nothing

  float T = 1.f, best_w = 0.f;
  int best = -1;  // list index of the pixel's largest w

  const int2 range = tile_bins[tile];
  for (int base = range.x; base < range.y; base += BSIZE) {
    if (__syncthreads_count(done ? 1 : 0) >= BSIZE) break;
    const int idx = base + tr;
    if (idx < range.y) {
      const int g = ids_sorted[idx];
      const bool known = (unsigned)g < (unsigned)num_points;  // (an id outside the arrays: an entry nobody sees)
      const int gs = known ? g : 0;
      const float2 xy = xys[gs];
      s_id[tr] = gs;
      s_x[tr] = xy.x;
      s_y[tr] = xy.y;
      s_o[tr] = known ? opacities[gs] : 0.f;
      s_a[tr] = conics[3 * gs];
      s_b[tr] = conics[3 * gs + 1];
      s_c[tr] = conics[3 * gs + 2];
    }
    s_max[tr] = 0u;
    s_sum[tr] = 0u;
    s_hits[tr] = 0u;
    __syncthreads();
    const int count = min(BSIZE, range.y - base);
    for (int t = 0; t < count; ++t) {
      if (!__any(done ? 0 : 1)) break;  // wave-uniform: every pixel of the wave has stopped
      const float dx = s_x[t] - px, dy = s_y[t] - py;
      const float sigma = 0.5f * (s_a[t] * dx * dx + s_c[t] * dy * dy) + s_b[t] * dx * dy;
      const float alpha = fminf(GSR_ALPHA_MAX_FWD, s_o[t] * __expf(-sigma));
      bool valid = !done && !(sigma < 0.f || alpha < GSR_ALPHA_MIN);
      const float next_T = T * (1.f - alpha);
      if (valid && next_T <= GSR_T_EPS) {
        done = true;
        valid = false;
      }
      if (!__any(valid ? 1 : 0)) continue;  // wave-uniform: the row reductions below run with every lane of the wave
      float w = 0.f;
      if (valid) {
        w = alpha * T;
        T = next_T;
        if (w > best_w) {
          best_w = w;
          best = base + t;
        }
      }
      const unsigned rh = row16_sum(valid ? 1u : 0u);
      const unsigned rq = row16_sum((unsigned)(w * Q_SCALE));
      const unsigned rm = row16_max(__float_as_uint(w));
      if (threadIdx.x == 0 && rh != 0u) {
        atomicMax(&s_max[t], rm);
        atomicAdd(&s_sum[t], rq);
        atomicAdd(&s_hits[t], rh);
      }
    }
    __syncthreads();
    if (tr < count && s_hits[tr] != 0u) {
      const size_t g = (size_t)s_id[tr];
      atomicMax(max_w + g, s_max[tr]);
      atomicAdd(sum_q + g, (unsigned long long)s_sum[tr]);
      atomicAdd(hits + g, (unsigned long long)s_hits[tr]);
    }
  }

  // one add per distinct (wave, Gaussian): the first pending lane's id, the ballot of its equals, their count
  int g = -1;
  if (best >= 0) g = ids_sorted[best];  // (a contributing entry: its id is inside the arrays)
  bool pending = g >= 0;
  unsigned long long left = __ballot(pending ? 1 : 0);
  while (left != 0ull) {
    const int leader = __ffsll((long long)left) - 1;
    const int gl = __shfl(g, leader);
    const bool same = pending && g == gl;
    const unsigned long long eq = __ballot(same ? 1 : 0);
    if (lane == leader) atomicAdd(dominant + (size_t)gl, (unsigned long long)__popcll(eq));
    if (same) pending = false;
    left &= ~eq;
  }
}

}  // namespace

GSR_EXPORT int gsr_contribution_accumulate(int tiles_x, int tiles_y, unsigned img_w, unsigned img_h, int num_points,
                                           const int32_t *ids, const int32_t *bins, const float *xys,
                                           const float *conics, const float *opacities, float *max_w, int64_t *sum_q,
                                           int64_t *hits, int64_t *dominant, gsr_stream_t stream) {
  GSR_REQUIRE(img_w > 0 && img_h > 0, "contribution_accumulate: empty image");
  GSR_REQUIRE((unsigned long long)img_w * img_h < (1ull << 31),
              "contribution_accumulate: the image must hold fewer than 2^31 pixels");
  GSR_REQUIRE(tiles_x == (int)gsr_cdiv(img_w, BW) && tiles_y == (int)gsr_cdiv(img_h, BW),
              "contribution_accumulate: tile bounds (%d,%d) do not match image %ux%u / block %d", tiles_x, tiles_y,
              img_w, img_h, BW);
  GSR_REQUIRE(num_points >= 1, "contribution_accumulate: num_points must be positive");
  GSR_REQUIRE(ids && bins && xys && conics && opacities && max_w && sum_q && hits && dominant,
              "contribution_accumulate: null pointer");
  hipLaunchKernelGGL(contribution_kernel, dim3(tiles_x, tiles_y), dim3(BW, BW), 0, (hipStream_t)stream, tiles_x,
                     (int)img_w, (int)img_h, num_points, ids, reinterpret_cast<const int2 *>(bins),
                     reinterpret_cast<const float2 *>(xys), conics, opacities, reinterpret_cast<unsigned *>(max_w),
                     reinterpret_cast<unsigned long long *>(sum_q), reinterpret_cast<unsigned long long *>(hits),
                     reinterpret_cast<unsigned long long *>(dominant));
  GSR_CHECK_LAUNCH("contribution_accumulate");
  return GSR_OK;
}
