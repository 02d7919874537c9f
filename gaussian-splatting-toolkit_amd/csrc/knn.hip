// knn.hip -- k nearest neighbours among 3-D points on the GPU: what the toolkit's models ask scikit-learn for when
// they turn a seed cloud into initial Gaussian scales (`k_nearest_sklearn`, vanilla_gs.py:136-140, 260-280), as a
// general query (the rule is stated in include/gsraster.h, the NumPy restatement is
// tests/knn_reference.py).
//
// Compiled with -ffp-contract=off (Makefile): a pair's d2 = (dx*dx + dy*dy) + dz*dz with dx = q.x - p.x, every
// operation rounded on its own; the square root is correctly rounded.
//
// gsr_knn_build:  prepare (finiteness, per-workgroup bounds) -> bounds -> [host reads two words] -> keys (30-bit Morton
//   code << 32 | row: unique; left-out rows all ones) -> rocPRIM radix sort -> gather (sorted 16-byte rows: xyz, row)
//   -> leaf boxes -> one launch per level of the tree, bottom-up.
// gsr_knn_query:  Morton codes of the queries on the same grid -> radix sort with their row numbers -> one lane per
//   query, stackless walk; or (GSR_KNN_EXHAUSTIVE) every query against every usable point, points tiled through LDS.
//   Both call `consider` and nothing else for a pair.
//
// The tree is implicit.  Leaf l holds the sorted points [LEAF l, LEAF (l + 1)); L = ceil(usable / LEAF) leaves are
// padded to Lp, the next power of two, with empty boxes (lo = +inf, hi = -inf).  Nodes are a heap: node 1 the root,
// children 2 i and 2 i + 1, leaves Lp .. 2 Lp - 1; a node is two rows of 16 bytes (box lo, box hi).  A level is built
// from the finished level below by its own launch: no counters, no fences.  The escape of a node -- where the walk
// goes when the node's subtree is finished or skipped -- is index arithmetic: strip the trailing one bits (climb
// while the node is a right child), stop at 0 (the root was a right end), else add one (the right sibling).  No
// ropes, no stack, no runtime-indexed private array, no scratch.
//
// The best list: K pairs (d2, row) in registers, K a template parameter (1, 2, 3, 4, 8, 16; k is rounded up), kept
// ascending in the lexicographic order of the pair by a fully unrolled insertion.  The result is the set of the K
// smallest pairs whatever the order of the insertions, so tree and exhaustive path agree bit for bit, rows included.
// The list is seeded from the leaf whose code is nearest the query's and SEED_WING(K) leaves either side; the walk
// leaves those leaves out.
//
// The prune rule: a subtree is skipped iff  b > d2[K-1]  (strictly; no slack), b = (gx*gx + gy*gy) + gz*gz with
// g = max(lo - q, q - hi, 0) per axis.  Why no slack is needed: a point p of the subtree has lo <= p <= hi.  Rounding
// to nearest is monotone and odd, so for q > hi >= p: fl(q - hi) <= fl(q - p) = |dx|; for q < lo <= p: fl(lo - q) <=
// fl(p - q) = |dx|; else g = 0.  Hence 0 <= g <= |dx| per axis; fl of a product of non-negative operands and fl of a sum
// are monotone in each operand, so b <= d2 AS COMPUTED for every point of the subtree.  A skipped subtree therefore
// holds only pairs with d2 > d2[K-1]: none of them belongs to the K smallest, ties included (a pair that ties
// d2[K-1] has b <= d2[K-1] and is visited).  An overflow gives d2 = +inf on both sides of the comparison and prunes
// nothing.
//
// Determinism: keys are unique, so the sort, the leaves and the boxes are pure functions of the input; a query's
// result is a set defined by a total order.
//
// The key and bounds kernels are copies of mesh_distance.hip's (there they work on triangles and their centroids and
// carry the index check): a shared header would have changed that file.
#include <climits>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gsr_common.h"

namespace {

constexpr int MAX_POINTS = 1 << 28;
constexpr int TPB = 256;
constexpr int LEAF = 8;  // points per leaf: a choice, not a fitted constant
constexpr int SELF = INT_MIN;

enum { ST_USABLE = 0, ST_SKIPPED = 1, ST_BAD_QUERIES = 2 };

struct Header {  // first 256 bytes of the tree
  float lo[3];     // scene bounds: the grid of the Morton codes
  float scale[3];  // 1024 / extent (0 for a flat axis)
};

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ V3 load3(const float *p, size_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

__device__ __forceinline__ uint32_t spread10(uint32_t v) {
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
__device__ __forceinline__ uint32_t morton30(V3 p, const Header *h) {
  const float fx = fminf(fmaxf((p.x - h->lo[0]) * h->scale[0], 0.f), 1023.f);
  const float fy = fminf(fmaxf((p.y - h->lo[1]) * h->scale[1], 0.f), 1023.f);
  const float fz = fminf(fmaxf((p.z - h->lo[2]) * h->scale[2], 0.f), 1023.f);
  return (spread10((uint32_t)fx) << 2) | (spread10((uint32_t)fy) << 1) | spread10((uint32_t)fz);
}

// ---- build -----------------------------------------------------------------------------------------------------------
__global__ void knn_state_init_kernel(int32_t *state, int first, int count) {
  if ((int)threadIdx.x < count) state[first + threadIdx.x] = 0;
}

// finiteness, bounds of the workgroup
__global__ __launch_bounds__(TPB) void knn_prepare_kernel(const int n, const float *__restrict__ pts,
                                                          float *__restrict__ partial, int32_t *__restrict__ state) {
  __shared__ float red[6][TPB];
  __shared__ int skipped;
  const int i = blockIdx.x * TPB + threadIdx.x, t = threadIdx.x;
  if (t == 0) skipped = 0;
  __syncthreads();
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n) {
    const V3 p = load3(pts, i);
    if (finite3(p)) {
      lo[0] = hi[0] = p.x, lo[1] = hi[1] = p.y, lo[2] = hi[2] = p.z;
    } else {
      atomicAdd(&skipped, 1);
    }
  }
  for (int k = 0; k < 3; ++k) red[k][t] = lo[k], red[3 + k][t] = hi[k];
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < 3; ++k) {
        red[k][t] = fminf(red[k][t], red[k][t + s]);
        red[3 + k][t] = fmaxf(red[3 + k][t], red[3 + k][t + s]);
      }
    __syncthreads();
  }
  if (t < 6) partial[6 * (size_t)blockIdx.x + t] = red[t][0];
  if (t == 0 && skipped) atomicAdd(&state[ST_SKIPPED], skipped);
}

__global__ __launch_bounds__(TPB) void knn_bounds_kernel(const int blocks, const int n, const float *__restrict__ partial,
                                                         int32_t *__restrict__ state, Header *__restrict__ h) {
  __shared__ float red[6][TPB];
  const int t = threadIdx.x;
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int b = t; b < blocks; b += TPB)
    for (int k = 0; k < 3; ++k) {
      v[k] = fminf(v[k], partial[6 * (size_t)b + k]);
      v[3 + k] = fmaxf(v[3 + k], partial[6 * (size_t)b + 3 + k]);
    }
  for (int k = 0; k < 6; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < 3; ++k) {
        red[k][t] = fminf(red[k][t], red[k][t + s]);
        red[3 + k][t] = fmaxf(red[3 + k][t], red[3 + k][t + s]);
      }
    __syncthreads();
  }
  if (t < 3) {
    const float ext = red[3 + t][0] - red[t][0];
    h->lo[t] = isfinite(red[t][0]) ? red[t][0] : 0.f;
    h->scale[t] = (ext > 0.f && isfinite(ext)) ? 1024.f / ext : 0.f;
  }
  if (t == 0) state[ST_USABLE] = n - state[ST_SKIPPED];
}

__global__ __launch_bounds__(TPB) void knn_keys_kernel(const int n, const float *__restrict__ pts,
                                                       const Header *__restrict__ h, uint64_t *__restrict__ key) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const V3 p = load3(pts, i);
  key[i] = finite3(p) ? ((uint64_t)morton30(p, h) << 32) | (uint32_t)i : ~0ull;
}

// sorted rows: (xyz | row number); the row's code next to it, for the seed search
__global__ __launch_bounds__(TPB) void knn_gather_kernel(const int nu, const int n, const float *__restrict__ pts,
                                                         const uint64_t *__restrict__ key, float4 *__restrict__ sorted,
                                                         uint32_t *__restrict__ code) {
  const int l = blockIdx.x * TPB + threadIdx.x;
  if (l >= nu) return;
  const uint64_t kk = key[l];
  const int row = (int)(uint32_t)kk;
  if ((unsigned)row >= (unsigned)n) return;  // (never: the first nu keys carry the rows of finite points)
  const V3 p = load3(pts, row);
  sorted[l] = make_float4(p.x, p.y, p.z, __int_as_float(row));
  code[l] = (uint32_t)(kk >> 32);
}

// box of leaf l -> node Lp + l; empty for the padding leaves
__global__ __launch_bounds__(TPB) void knn_leaf_box_kernel(const int nu, const int Lp, const float4 *__restrict__ sorted,
                                                           float4 *__restrict__ nodes) {
  const int l = blockIdx.x * TPB + threadIdx.x;
  if (l >= Lp) return;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int j = 0; j < LEAF; ++j) {
    const int at = l * LEAF + j;
    if (at < nu) {
      const float4 p = sorted[at];
      lo[0] = fminf(lo[0], p.x), lo[1] = fminf(lo[1], p.y), lo[2] = fminf(lo[2], p.z);
      hi[0] = fmaxf(hi[0], p.x), hi[1] = fmaxf(hi[1], p.y), hi[2] = fmaxf(hi[2], p.z);
    }
  }
  nodes[2 * (size_t)(Lp + l)] = make_float4(lo[0], lo[1], lo[2], 0.f);
  nodes[2 * (size_t)(Lp + l) + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

// level of `count` nodes (count .. 2 count - 1) from the finished level below
__global__ __launch_bounds__(TPB) void knn_level_kernel(const int count, float4 *__restrict__ nodes) {
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= count) return;
  const size_t i = (size_t)count + t;
  const float4 a0 = nodes[4 * i], a1 = nodes[4 * i + 1], b0 = nodes[4 * i + 2], b1 = nodes[4 * i + 3];
  nodes[2 * i] = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), 0.f);
  nodes[2 * i + 1] = make_float4(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z), 0.f);
}

// ---- query -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void knn_query_keys_kernel(const int m, const float *__restrict__ q,
                                                             const Header *__restrict__ h, uint32_t *__restrict__ key,
                                                             int32_t *__restrict__ val) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= m) return;
  const V3 p = load3(q, i);
  key[i] = finite3(p) ? morton30(p, h) : 0xffffffffu;
  val[i] = i;
}

template <int K>
struct Best {
  float d2[K];
  int row[K];
};
__device__ __forceinline__ bool before(float da, int ra, float db, int rb) {
  return da < db || (da == db && ra < rb);
}
template <int K>
__device__ __forceinline__ void clear(Best<K> &b) {
#pragma unroll
  for (int j = 0; j < K; ++j) b.d2[j] = INFINITY, b.row[j] = INT_MAX;
}
// the one place a pair is evaluated: reference row r (xyz | row number) against query p, `skip` the row left out
template <int K>
__device__ __forceinline__ void consider(const float4 r, const V3 p, const int skip, Best<K> &b) {
  const int row = __float_as_int(r.w);
  const float dx = p.x - r.x, dy = p.y - r.y, dz = p.z - r.z;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  if (row == skip || !before(d2, row, b.d2[K - 1], b.row[K - 1])) return;
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {  // (b[j - 1] is still the old one when b[j] takes it)
    const bool here = before(d2, row, b.d2[j], b.row[j]);
    bool shift = false;
    if (j > 0) shift = before(d2, row, b.d2[j - 1], b.row[j - 1]);
    const float nd = shift ? b.d2[j > 0 ? j - 1 : 0] : d2;
    const int nr = shift ? b.row[j > 0 ? j - 1 : 0] : row;
    b.d2[j] = here ? nd : b.d2[j];
    b.row[j] = here ? nr : b.row[j];
  }
}
template <int K>
__device__ __forceinline__ void write_result(const size_t row, const int k, const Best<K> &b, float *dist, int32_t *idx) {
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < k) dist[row * k + j] = sqrtf(b.d2[j]), idx[row * k + j] = b.row[j];
}
__device__ __forceinline__ void write_invalid(const size_t row, const int k, float *dist, int32_t *idx) {
  for (int j = 0; j < k; ++j) dist[row * k + j] = NAN, idx[row * k + j] = -1;
}
template <int K>
__device__ __forceinline__ void leaf_test(const float4 *__restrict__ sorted, const int l, const int nu, const V3 p,
                                          const int skip, Best<K> &b) {
#pragma unroll
  for (int j = 0; j < LEAF; ++j) {
    const int at = l * LEAF + j;
    if (at < nu) consider<K>(sorted[at], p, skip, b);
  }
}
// leaves either side of the seed leaf: 2 wing + 1 leaves hold more than K + 1 points away from the ends
__host__ __device__ constexpr int seed_wing(int K) { return K / LEAF + 1; }

template <int K>
__global__ __launch_bounds__(TPB) void knn_query_kernel(const int m, const int k, const int self,
                                                        const int32_t *__restrict__ order,
                                                        const float *__restrict__ q, const Header *__restrict__ h,
                                                        const float4 *__restrict__ sorted,
                                                        const uint32_t *__restrict__ code,
                                                        const float4 *__restrict__ nodes, const int nu, const int L,
                                                        const int Lp, float *__restrict__ dist,
                                                        int32_t *__restrict__ idx, int32_t *__restrict__ state) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= m) return;
  const int row = order[i];
  if ((unsigned)row >= (unsigned)m) return;  // (never: `order` is a permutation written by this call)
  const V3 p = load3(q, row);
  if (!finite3(p)) {
    write_invalid(row, k, dist, idx);
    atomicAdd(&state[ST_BAD_QUERIES], 1);
    return;
  }
  const int skip = self ? row : SELF;
  Best<K> best;
  clear(best);
  // seed: the leaf of the point whose code is nearest the query's, and its neighbours
  const uint32_t c = morton30(p, h);
  int lo = 0, hi = nu;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (code[mid] < c) lo = mid + 1; else hi = mid;
  }
  int at = min(lo, nu - 1);
  if (lo > 0 && lo < nu && c - code[lo - 1] < code[lo] - c) at = lo - 1;
  const int s0 = max(at / LEAF - seed_wing(K), 0), s1 = min(at / LEAF + seed_wing(K), L - 1);
  for (int l = s0; l <= s1; ++l) leaf_test<K>(sorted, l, nu, p, skip, best);
  int node = 1;
  while (node != 0) {
    const float4 r0 = nodes[2 * (size_t)node], r1 = nodes[2 * (size_t)node + 1];
    const float gx = fmaxf(fmaxf(r0.x - p.x, p.x - r1.x), 0.f);
    const float gy = fmaxf(fmaxf(r0.y - p.y, p.y - r1.y), 0.f);
    const float gz = fmaxf(fmaxf(r0.z - p.z, p.z - r1.z), 0.f);
    const float b = (gx * gx + gy * gy) + gz * gz;
    const bool enter = !(b > best.d2[K - 1]);
    if (enter && node < Lp) {
      node = 2 * node;
      continue;
    }
    if (enter) {
      const int l = node - Lp;
      if (l < s0 || l > s1) leaf_test<K>(sorted, l, nu, p, skip, best);
    }
    node >>= __builtin_ctz(~(unsigned)node);  // (node < 2^27: ~node has a one bit)
    node = node ? node + 1 : 0;
  }
  write_result<K>(row, k, best, dist, idx);
}

// every query against every usable point, TPB points at a time through LDS (every lane reads the same row: a broadcast)
template <int K>
__global__ __launch_bounds__(TPB) void knn_exhaustive_kernel(const int m, const int k, const int self,
                                                             const float *__restrict__ q,
                                                             const float4 *__restrict__ sorted, const int nu,
                                                             float *__restrict__ dist, int32_t *__restrict__ idx,
                                                             int32_t *__restrict__ state) {
  __shared__ float4 tile[TPB];
  const int i = blockIdx.x * TPB + threadIdx.x;
  V3 p = {0.f, 0.f, 0.f};
  if (i < m) p = load3(q, i);
  const bool live = i < m && finite3(p);
  const int skip = self ? i : SELF;
  Best<K> best;
  clear(best);
  for (int base = 0; base < nu; base += TPB) {  // (nu is uniform: every thread reaches the barriers)
    const int count = min(TPB, nu - base);
    __syncthreads();
    if ((int)threadIdx.x < count) tile[threadIdx.x] = sorted[base + threadIdx.x];
    __syncthreads();
    if (live)
      for (int j = 0; j < count; ++j) consider<K>(tile[j], p, skip, best);
  }
  if (i >= m) return;
  if (live) {
    write_result<K>(i, k, best, dist, idx);
  } else {
    write_invalid(i, k, dist, idx);
    atomicAdd(&state[ST_BAD_QUERIES], 1);
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline int leaves_of(int points) { return (points + LEAF - 1) / LEAF; }
inline int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct Tree {
  Header *header;
  float4 *sorted;  // [n]
  uint32_t *code;  // [n]
  float4 *nodes;   // [4 Lp(n)]: node i is rows 2 i and 2 i + 1, node 0 unused
};
size_t carve_tree(int n, void *mem, Tree *t) {
  const size_t head = 256, sp = align_up((size_t)n * 16), cd = align_up((size_t)n * 4);
  const size_t nd = align_up((size_t)4 * pow2_ceil(leaves_of(n)) * 16);
  if (t) {
    char *p = static_cast<char *>(mem);
    t->header = reinterpret_cast<Header *>(p);
    t->sorted = reinterpret_cast<float4 *>(p + head);
    t->code = reinterpret_cast<uint32_t *>(p + head + sp);
    t->nodes = reinterpret_cast<float4 *>(p + head + sp + cd);
  }
  return head + sp + cd + nd;
}

struct BuildSpace {
  uint64_t *key_in, *key_out;  // [n]
  float *partial;              // [6 blocks]
  char *temp;
  size_t temp_bytes;
};
size_t carve_build(int n, void *mem, size_t bytes, BuildSpace *w) {
  const size_t n8 = align_up((size_t)n * 8), pb = align_up((size_t)gsr_cdiv(n, TPB) * 6 * 4);
  const size_t head = 2 * n8 + pb;
  if (w) {
    char *p = static_cast<char *>(mem);
    w->key_in = reinterpret_cast<uint64_t *>(p);
    w->key_out = reinterpret_cast<uint64_t *>(p + n8);
    w->partial = reinterpret_cast<float *>(p + 2 * n8);
    w->temp = p + head;
    w->temp_bytes = bytes - head;
  }
  return head;
}

struct QuerySpace {
  uint32_t *key_in, *key_out;  // [m]
  int32_t *val_in, *val_out;   // [m]
  char *temp;
  size_t temp_bytes;
};
size_t carve_query(int m, void *mem, size_t bytes, QuerySpace *w) {
  const size_t m4 = align_up((size_t)m * 4);
  if (w) {
    char *p = static_cast<char *>(mem);
    w->key_in = reinterpret_cast<uint32_t *>(p);
    w->key_out = reinterpret_cast<uint32_t *>(p + m4);
    w->val_in = reinterpret_cast<int32_t *>(p + 2 * m4);
    w->val_out = reinterpret_cast<int32_t *>(p + 3 * m4);
    w->temp = p + 4 * m4;
    w->temp_bytes = bytes - 4 * m4;
  }
  return 4 * m4;
}

bool build_temp_bytes(int n, size_t *out) {
  return rocprim::radix_sort_keys(nullptr, *out, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)n, 0, 64) ==
         hipSuccess;
}
bool query_temp_bytes(int m, size_t *out) {
  return rocprim::radix_sort_pairs(nullptr, *out, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                   (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)m, 0, 32) == hipSuccess;
}

int check_space(const void *ws, size_t have, size_t need, const char *who, const char *what) {
  GSR_REQUIRE(need != 0, "%s: the %s size query failed", who, what);
  if (have < need || !ws) {
    gsr_set_error("%s: %s %zu < %zu bytes", who, what, have, need);
    return GSR_ENOMEM;
  }
  GSR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: %s must be 256-byte aligned", who, what);
  return GSR_OK;
}

struct QueryArgs {
  int m, k, self, nu, L, Lp;
  const int32_t *order;
  const float *q;
  Tree t;
  float *dist;
  int32_t *idx, *state;
};
template <int K>
void launch_query(const QueryArgs &a, bool exhaustive, hipStream_t s) {
  const dim3 g(gsr_cdiv(a.m, TPB)), tpb(TPB);
  if (exhaustive)
    hipLaunchKernelGGL(knn_exhaustive_kernel<K>, g, tpb, 0, s, a.m, a.k, a.self, a.q, (const float4 *)a.t.sorted, a.nu,
                       a.dist, a.idx, a.state);
  else
    hipLaunchKernelGGL(knn_query_kernel<K>, g, tpb, 0, s, a.m, a.k, a.self, a.order, a.q, (const Header *)a.t.header,
                       (const float4 *)a.t.sorted, (const uint32_t *)a.t.code, (const float4 *)a.t.nodes, a.nu, a.L,
                       a.Lp, a.dist, a.idx, a.state);
}

}  // namespace

GSR_EXPORT size_t gsr_knn_workspace_bytes(int what, int num_points, int num_queries, int k) {
  const int n = num_points, m = num_queries;
  size_t temp = 0;
  switch (what) {
    case GSR_KNN_BYTES_TREE:
      return n <= 0 || n > MAX_POINTS ? 0 : carve_tree(n, nullptr, nullptr);
    case GSR_KNN_BYTES_BUILD:
      if (n <= 0 || n > MAX_POINTS || !build_temp_bytes(n, &temp)) return 0;
      return carve_build(n, nullptr, 0, nullptr) + align_up(temp);
    case GSR_KNN_BYTES_QUERY:
      if (m <= 0 || m > MAX_POINTS || k < 1 || k > GSR_KNN_MAX_K || !query_temp_bytes(m, &temp)) return 0;
      return carve_query(m, nullptr, 0, nullptr) + align_up(temp);
    default:
      return 0;
  }
}

GSR_EXPORT int gsr_knn_build(int num_points, const float *points, void *tree, size_t tree_bytes, void *workspace,
                             size_t workspace_bytes, int32_t *state, gsr_stream_t stream) {
  const int n = num_points;
  GSR_REQUIRE(n >= 1 && n <= MAX_POINTS, "knn_build: num_points must be in [1, %d]", MAX_POINTS);
  GSR_REQUIRE(points != nullptr && state != nullptr, "knn_build: null pointer");
  if (int rc = check_space(tree, tree_bytes, gsr_knn_workspace_bytes(GSR_KNN_BYTES_TREE, n, 0, 0), "knn_build", "tree"))
    return rc;
  if (int rc = check_space(workspace, workspace_bytes, gsr_knn_workspace_bytes(GSR_KNN_BYTES_BUILD, n, 0, 0),
                           "knn_build", "workspace"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Tree t;
  BuildSpace w;
  carve_tree(n, tree, &t);
  carve_build(n, workspace, workspace_bytes, &w);
  const unsigned blocks = gsr_cdiv(n, TPB);
  const dim3 gn(blocks), tpb(TPB);
  hipLaunchKernelGGL(knn_state_init_kernel, dim3(1), dim3(4), 0, s, state, 0, 4);
  GSR_CHECK_LAUNCH("knn_state_init");
  hipLaunchKernelGGL(knn_prepare_kernel, gn, tpb, 0, s, n, points, w.partial, state);
  GSR_CHECK_LAUNCH("knn_prepare");
  hipLaunchKernelGGL(knn_bounds_kernel, dim3(1), tpb, 0, s, (int)blocks, n, (const float *)w.partial, state, t.header);
  GSR_CHECK_LAUNCH("knn_bounds");
  int st[2] = {0, 0};
  GSR_CHECK_HIP(hipMemcpyAsync(st, state, sizeof(st), hipMemcpyDeviceToHost, s));
  GSR_CHECK_HIP(hipStreamSynchronize(s));
  const int nu = st[ST_USABLE];
  GSR_REQUIRE(nu >= 0 && nu <= n && nu + st[ST_SKIPPED] == n, "knn_build: inconsistent counts %d + %d != %d", nu,
              st[ST_SKIPPED], n);
  if (nu == 0) return GSR_OK;  // (state says so: every query fails with GSR_ERANGE)
  hipLaunchKernelGGL(knn_keys_kernel, gn, tpb, 0, s, n, points, (const Header *)t.header, w.key_in);
  GSR_CHECK_LAUNCH("knn_keys");
  size_t tb = w.temp_bytes;
  GSR_CHECK_HIP(rocprim::radix_sort_keys(w.temp, tb, (const uint64_t *)w.key_in, w.key_out, (size_t)n, 0, 64, s));
  hipLaunchKernelGGL(knn_gather_kernel, dim3(gsr_cdiv(nu, TPB)), tpb, 0, s, nu, n, points, (const uint64_t *)w.key_out,
                     t.sorted, t.code);
  GSR_CHECK_LAUNCH("knn_gather");
  const int Lp = pow2_ceil(leaves_of(nu));
  hipLaunchKernelGGL(knn_leaf_box_kernel, dim3(gsr_cdiv(Lp, TPB)), tpb, 0, s, nu, Lp, (const float4 *)t.sorted, t.nodes);
  GSR_CHECK_LAUNCH("knn_leaf_box");
  for (int count = Lp / 2; count >= 1; count >>= 1) {
    hipLaunchKernelGGL(knn_level_kernel, dim3(gsr_cdiv(count, TPB)), tpb, 0, s, count, t.nodes);
    GSR_CHECK_LAUNCH("knn_level");
  }
  return GSR_OK;
}

GSR_EXPORT int gsr_knn_query(int num_points, const void *tree, size_t tree_bytes, int num_usable, int num_queries,
                             const float *queries, int k, int flags, void *workspace, size_t workspace_bytes,
                             float *distance, int32_t *index, int32_t *state, gsr_stream_t stream) {
  const int n = num_points, m = num_queries, nu = num_usable;
  const int self = (flags & GSR_KNN_SELF) ? 1 : 0;
  GSR_REQUIRE(n >= 1 && n <= MAX_POINTS, "knn_query: num_points must be in [1, %d]", MAX_POINTS);
  GSR_REQUIRE(m >= 0 && m <= MAX_POINTS, "knn_query: num_queries must be in [0, %d]", MAX_POINTS);
  GSR_REQUIRE(k >= 1 && k <= GSR_KNN_MAX_K, "knn_query: k must be in [1, %d], got %d", GSR_KNN_MAX_K, k);
  GSR_REQUIRE((flags & ~(GSR_KNN_EXHAUSTIVE | GSR_KNN_SELF)) == 0, "knn_query: unknown flags %d", flags);
  GSR_REQUIRE(nu >= 0 && nu <= n, "knn_query: num_usable must be in [0, num_points]");
  GSR_REQUIRE(!self || m == n, "knn_query: self mode needs the reference points as queries (%d != %d)", m, n);
  if (nu < k + self) {
    gsr_set_error("knn_query: %d usable reference points, k = %d%s needs %d", nu, k, self ? " in self mode" : "",
                  k + self);
    return GSR_ERANGE;
  }
  if (m == 0) return GSR_OK;
  GSR_REQUIRE(queries && distance && index && state, "knn_query: null pointer");
  if (int rc = check_space(tree, tree_bytes, gsr_knn_workspace_bytes(GSR_KNN_BYTES_TREE, n, 0, 0), "knn_query", "tree"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  QueryArgs a;
  carve_tree(n, const_cast<void *>(tree), &a.t);
  a.m = m, a.k = k, a.self = self, a.nu = nu, a.L = leaves_of(nu), a.Lp = pow2_ceil(a.L);
  a.order = nullptr, a.q = queries, a.dist = distance, a.idx = index, a.state = state;
  const bool exhaustive = (flags & GSR_KNN_EXHAUSTIVE) != 0;
  hipLaunchKernelGGL(knn_state_init_kernel, dim3(1), dim3(4), 0, s, state, (int)ST_BAD_QUERIES, 1);
  GSR_CHECK_LAUNCH("knn_state_init");
  if (!exhaustive) {
    if (int rc = check_space(workspace, workspace_bytes, gsr_knn_workspace_bytes(GSR_KNN_BYTES_QUERY, 0, m, k),
                             "knn_query", "workspace"))
      return rc;
    QuerySpace w;
    carve_query(m, workspace, workspace_bytes, &w);
    hipLaunchKernelGGL(knn_query_keys_kernel, dim3(gsr_cdiv(m, TPB)), dim3(TPB), 0, s, m, queries,
                       (const Header *)a.t.header, w.key_in, w.val_in);
    GSR_CHECK_LAUNCH("knn_query_keys");
    size_t tb = w.temp_bytes;
    GSR_CHECK_HIP(rocprim::radix_sort_pairs(w.temp, tb, (const uint32_t *)w.key_in, w.key_out,
                                            (const int32_t *)w.val_in, w.val_out, (size_t)m, 0, 32, s));
    a.order = w.val_out;
  }
  if (k == 1) launch_query<1>(a, exhaustive, s);
  else if (k == 2) launch_query<2>(a, exhaustive, s);
  else if (k == 3) launch_query<3>(a, exhaustive, s);
  else if (k == 4) launch_query<4>(a, exhaustive, s);
  else if (k <= 8) launch_query<8>(a, exhaustive, s);
  else launch_query<16>(a, exhaustive, s);
  GSR_CHECK_LAUNCH(exhaustive ? "knn_exhaustive" : "knn_query");
  return GSR_OK;
}
