// canny.hip -- the Canny edge mask of an [H,W,3] float image on the GPU (the rule is stated in
// include/gsraster.h, the NumPy + SciPy oracle is tests/canny_reference.py).  What the co-gs model's depth
// regularisation asks `image2canny` for (gs_toolkit/utils/losses.py:48-58) on every training step.
//
// All arithmetic is integer: the result is exact, and a pure function of the input.
//
//   canny_nms_kernel   one workgroup per 32 x 16 tile: the image as uint8 in LDS with a 2-pixel halo, Sobel + channel
//                      pick at a 1-pixel halo (mag, dx, dy as int16 in LDS), non-maximum suppression -> one map byte
//                      per pixel (none / weak / strong); parent[p] = p, flag[p] = 0.  No dx / dy / mag reaches HBM.
//   canny_link_kernel  one thread per candidate: unite with the candidate neighbours at E, SW, S, SE (every
//                      8-adjacency once).  The union-find of mesh_clean.hip: parent[x] only ever falls (atomicMin),
//                      so the root of a component is its smallest pixel index whatever the order of the atomics.
//   canny_mark_kernel  every strong pixel stores 1 into flag[root] (byte stores of one value, no atomics).
//   canny_emit_kernel  edges[p] = candidate && flag[root(p)] ? 255 : 0.
//
// Grids: the tile kernel is a 2-D grid of tiles; the other three are one thread per pixel.  The only data-dependent
// loops are the root chases.  Nothing is read back; nothing is allocated.
#include <climits>

#include "gsr_common.h"

namespace {

constexpr int TPB = 256;
constexpr int TW = 32, TH = 16;          // pixels per workgroup
constexpr int IW = TW + 4, IH = TH + 4;  // staged image: 2-pixel halo
constexpr int MW = TW + 2, MH = TH + 2;  // gradient: 1-pixel halo
enum : uint8_t { MAP_NONE = 0, MAP_WEAK = 1, MAP_STRONG = 2 };

// (uint8)trunc(x * 255.0f), the product in float32; saturating, NaN -> 0
__device__ __forceinline__ uint8_t to_u8(float x) {
  const float t = x * 255.0f;
  if (!(t > 0.f)) return 0;
  return t >= 255.f ? 255 : (uint8_t)(int)t;
}

__global__ __launch_bounds__(TPB) void canny_nms_kernel(const int H, const int W, const int low, const int high,
                                                        const float *__restrict__ image, uint8_t *__restrict__ map,
                                                        int32_t *__restrict__ parent, uint8_t *__restrict__ flag) {
  __shared__ uint8_t s_img[IH][IW * 3];
  __shared__ short s_mag[MH][MW], s_dx[MH][MW], s_dy[MH][MW];
  const int ox = blockIdx.x * TW, oy = blockIdx.y * TH;
  const int tid = threadIdx.x;

  // replicate border: coordinates are clamped, so every load is inside the image
  for (int i = tid; i < IH * IW * 3; i += TPB) {
    const int r = i / (IW * 3), e = i - r * (IW * 3);
    const int px = e / 3, c = e - 3 * px;
    const int gy = gsr_clampi(oy - 2 + r, 0, H - 1), gx = gsr_clampi(ox - 2 + px, 0, W - 1);
    s_img[r][e] = to_u8(image[((size_t)gy * W + gx) * 3 + c]);
  }
  __syncthreads();

  // gradient entry (r, q) is pixel (oy - 1 + r, ox - 1 + q) = staged (r + 1, q + 1); outside the image mag is 0
  for (int i = tid; i < MH * MW; i += TPB) {
    const int r = i / MW, q = i - r * MW;
    const int gy = oy - 1 + r, gx = ox - 1 + q;
    int mag = 0, bdx = 0, bdy = 0;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      mag = -1;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int a00 = s_img[r][3 * q + c], a01 = s_img[r][3 * (q + 1) + c], a02 = s_img[r][3 * (q + 2) + c];
        const int a10 = s_img[r + 1][3 * q + c], a12 = s_img[r + 1][3 * (q + 2) + c];
        const int a20 = s_img[r + 2][3 * q + c], a21 = s_img[r + 2][3 * (q + 1) + c], a22 = s_img[r + 2][3 * (q + 2) + c];
        const int dx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
        const int dy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
        const int norm = abs(dx) + abs(dy);
        if (norm > mag) mag = norm, bdx = dx, bdy = dy;  // ties: the lowest channel
      }
    }
    s_mag[r][q] = (short)mag;  // (<= 2040)
    s_dx[r][q] = (short)bdx;
    s_dy[r][q] = (short)bdy;
  }
  __syncthreads();

  for (int i = tid; i < TH * TW; i += TPB) {
    const int r = i / TW, q = i - r * TW;
    const int gy = oy + r, gx = ox + q;
    if (gy >= H || gx >= W) continue;
    const int mr = r + 1, mq = q + 1;
    const int m = s_mag[mr][mq];
    uint8_t out = MAP_NONE;
    if (m > low) {
      const int dx = s_dx[mr][mq], dy = s_dy[mr][mq];
      const int x = abs(dx), y = abs(dy) << 15;
      const int t22 = x * 13573, t67 = t22 + (x << 16);
      bool cand;
      if (y < t22) {
        cand = m > s_mag[mr][mq - 1] && m >= s_mag[mr][mq + 1];
      } else if (y > t67) {
        cand = m > s_mag[mr - 1][mq] && m >= s_mag[mr + 1][mq];
      } else {
        const int s = (dx ^ dy) < 0 ? -1 : 1;
        cand = m > s_mag[mr - 1][mq - s] && m > s_mag[mr + 1][mq + s];
      }
      if (cand) out = m > high ? MAP_STRONG : MAP_WEAK;
    }
    const size_t p = (size_t)gy * W + gx;
    map[p] = out;
    parent[p] = (int32_t)p;
    flag[p] = 0;
  }
}

// ---- union-find over pixels (the pattern of mesh_clean.hip) ----------------------------------------------------------
// parent[] is read and written by other threads of the same launch: loads are device-scope atomic loads, stores are
// atomicMin only, so parent[x] never rises and parent[x] <= x always holds (no cycles).
__device__ __forceinline__ int load_parent(const int32_t *parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// root of x, halving the path on the way (a lowered pointer still points to an ancestor)
__device__ __forceinline__ int find_root(int32_t *parent, int x) {
  for (;;) {
    const int p = load_parent(parent, x);
    if (p == x) return x;
    const int gp = load_parent(parent, p);
    if (gp == p) return p;
    atomicMin(parent + x, gp);
    x = gp;
  }
}
// Hooks the larger root under the smaller.  atomicMin returns what parent[hi] held: hi itself -> hi was a root and
// is hooked now; anything else -> another thread had hooked hi under `old` meanwhile, parent[hi] is now
// min(old, lo), and the other of the two still has to be joined: go on with (old, lo).  Both are below hi, so the
// loop ends.
__device__ __forceinline__ void unite(int32_t *parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(parent + hi, lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}
// (in a later launch: parent[] is final and only read)
__device__ __forceinline__ int final_root(const int32_t *__restrict__ parent, int x) {
  for (int p = parent[x]; p != x; p = parent[x]) x = p;
  return x;
}

__global__ __launch_bounds__(TPB) void canny_link_kernel(const int H, const int W, const uint8_t *__restrict__ map,
                                                         int32_t *__restrict__ parent) {
  const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
  if (p >= (long long)H * W || map[p] == MAP_NONE) return;
  const int y = (int)(p / W), x = (int)(p - (long long)y * W);
  const bool right = x + 1 < W, below = y + 1 < H;
  if (right && map[p + 1] != MAP_NONE) unite(parent, (int)p, (int)p + 1);
  if (below) {
    const long long d = p + W;
    if (x > 0 && map[d - 1] != MAP_NONE) unite(parent, (int)p, (int)(d - 1));
    if (map[d] != MAP_NONE) unite(parent, (int)p, (int)d);
    if (right && map[d + 1] != MAP_NONE) unite(parent, (int)p, (int)(d + 1));
  }
}

__global__ __launch_bounds__(TPB) void canny_mark_kernel(const long long n, const uint8_t *__restrict__ map,
                                                         const int32_t *__restrict__ parent,
                                                         uint8_t *__restrict__ flag) {
  const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
  if (p >= n || map[p] != MAP_STRONG) return;
  flag[final_root(parent, (int)p)] = 1;  // every writer stores the same value
}

__global__ __launch_bounds__(TPB) void canny_emit_kernel(const long long n, const uint8_t *__restrict__ map,
                                                         const int32_t *__restrict__ parent,
                                                         const uint8_t *__restrict__ flag,
                                                         uint8_t *__restrict__ edges) {
  const long long p = (long long)blockIdx.x * TPB + threadIdx.x;
  if (p >= n) return;
  edges[p] = (map[p] != MAP_NONE && flag[final_root(parent, (int)p)]) ? 255 : 0;
}

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

GSR_EXPORT size_t gsr_canny_workspace_bytes(int img_height, int img_width) {
  if (img_height <= 0 || img_width <= 0 || (long long)img_height * img_width > INT_MAX) return 0;
  const size_t n = (size_t)img_height * img_width;
  return align_up(4 * n) + 2 * align_up(n);  // parent, map, flag
}

GSR_EXPORT int gsr_canny(int img_height, int img_width, const float *image, float thres1, float thres2,
                         void *workspace, size_t workspace_bytes, uint8_t *edges, gsr_stream_t stream) {
  const int H = img_height, W = img_width;
  GSR_REQUIRE(H >= 0 && W >= 0 && (long long)H * W <= INT_MAX, "canny: H * W must be in [0, %d]", INT_MAX);
  if (H == 0 || W == 0) return GSR_OK;
  GSR_REQUIRE(image && edges, "canny: null pointer");
  GSR_REQUIRE(thres1 == thres1 && thres2 == thres2 && fabsf(thres1) < 1e9f && fabsf(thres2) < 1e9f,
              "canny: thresholds must be finite and below 1e9 in magnitude");
  const size_t need = gsr_canny_workspace_bytes(H, W);
  if (!workspace || workspace_bytes < need) {
    gsr_set_error("canny: workspace %zu < %zu bytes", workspace_bytes, need);
    return GSR_ENOMEM;
  }
  GSR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "canny: workspace must be 256-byte aligned");
  int low = (int)floorf(thres1), high = (int)floorf(thres2);
  if (low > high) {
    const int t = low;
    low = high, high = t;
  }
  const size_t n = (size_t)H * W;
  char *base = static_cast<char *>(workspace);
  int32_t *parent = reinterpret_cast<int32_t *>(base);
  uint8_t *map = reinterpret_cast<uint8_t *>(base + align_up(4 * n));
  uint8_t *flag = map + align_up(n);
  hipStream_t s = (hipStream_t)stream;
  const dim3 tiles(gsr_cdiv(W, TW), gsr_cdiv(H, TH)), px((unsigned)((n + TPB - 1) / TPB)), tpb(TPB);
  GSR_REQUIRE(tiles.y <= 65535u, "canny: image height above %d", 65535 * TH);
  hipLaunchKernelGGL(canny_nms_kernel, tiles, tpb, 0, s, H, W, low, high, image, map, parent, flag);
  GSR_CHECK_LAUNCH("canny_nms");
  hipLaunchKernelGGL(canny_link_kernel, px, tpb, 0, s, H, W, (const uint8_t *)map, parent);
  GSR_CHECK_LAUNCH("canny_link");
  hipLaunchKernelGGL(canny_mark_kernel, px, tpb, 0, s, (long long)n, (const uint8_t *)map, (const int32_t *)parent, flag);
  GSR_CHECK_LAUNCH("canny_mark");
  hipLaunchKernelGGL(canny_emit_kernel, px, tpb, 0, s, (long long)n, (const uint8_t *)map, (const int32_t *)parent,
                     (const uint8_t *)flag, edges);
  GSR_CHECK_LAUNCH("canny_emit");
  return GSR_OK;
}
