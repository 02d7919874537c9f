// mesh_distance.hip -- unsigned distance from points to a triangle mesh on the GPU: what the toolkit's
// gs_toolkit/evaluation/surface_distance tool computes per vertex of a generated mesh (the rule
// is stated in include/gsraster.h, the NumPy restatement is tests/surface_distance_reference.py).
//
// Compiled with -ffp-contract=off (Makefile): `tri_closest` is evaluated with every operation rounded on its own, in
// the order the float32 NumPy restatement uses; division and square root are correctly rounded.
//
// gsr_mesh_bvh_build:  prepare (index check, finiteness, centroid, per-workgroup bounds) -> [host reads two words]
//   -> bounds -> keys (30-bit Morton code of the centroid << 32 | triangle index: unique) -> rocPRIM radix sort ->
//   gather (leaf l = three padded rows of the l-th triangle's vertices) -> Karras (one thread per internal node over
//   the unique keys) -> ropes -> refit (bottom-up, one thread per leaf, an arrival counter per internal node).
// gsr_mesh_distance_query:  Morton codes of the points on the same grid -> radix sort with their row numbers -> one
//   lane per point, stackless walk; or (GSR_MESH_DISTANCE_EXHAUSTIVE) every point against every leaf, leaves tiled
//   through LDS.  Both call `tri_closest` and nothing else for a triangle.
// gsr_mesh_distance_stats:  float64 partials per workgroup in a fixed order, then one workgroup.
//
// The tree.  Internal nodes 0 .. Fu-2 (Fu = usable triangles), node 0 the root; a node reference is i >= 0 for an
// internal node, ~l < 0 for leaf l, NODE_END for "done".  An internal node is two rows of 16 bytes: (box lo, left
// child) and (box hi, escape); a leaf's escape is the .w of its second row.  The escape ("rope") of a node is where
// the walk goes when the node's subtree is finished or skipped: the right child of the one internal node whose split
// is the node's last leaf (`after[last]`; every gap between two neighbouring leaves is the split of exactly one
// internal node), NODE_END when its last leaf is Fu-1.  The walk is: internal node -> box test -> left child or
// escape; leaf -> triangle -> escape.  No stack, so no runtime-indexed private array and no scratch.
//
// The prune slack.  A subtree is skipped when  db2 > (best + 2^-18 R)^2,  db2 the squared distance from the point to
// the node's box as computed, R = the largest |component| of (lo - p, hi - p).  Derivation, u = 2^-24: every triangle
// of the subtree lies in the box, so its translated vertices have |components| <= R.  (1) translation rounds each
// component by <= uR: the rounded triangle is within sqrt3 uR of the true one.  (2) the closest point as computed,
// a' + v e0 + w e1: e = b' - a' (|e| <= 2R: error 2uR), v e (2uR, plus e's 2uR), twice; the two sums (3uR, 5uR); v + w
// may exceed 1 by u (2uR): <= 18uR per component, 18 sqrt3 uR < 32uR in norm, from a point OF the rounded triangle --
// whichever region the rounded tests chose, the point is on the triangle, so its norm is no less than the true
// distance minus these.  (3) the norm (three squares, two sums, a root): 2.5u relative of <= sqrt3 R: 4.4uR.  (4) the
// box side: (1 + u) per difference, 5u relative on db2, 2.5u on db <= sqrt3 R: 4.4uR.  (5) squaring best + slack: 1.5u
// relative, 2.6uR.  Sum < 46uR; the slack is 64uR = 2^-18 R.  With it, no skipped triangle's COMPUTED distance is
// below the best at that moment, so the walk returns the exhaustive kernel's minimum bit for bit.
//
// Determinism: keys are unique, so the sort, the tree and the boxes (min / max) are pure functions of the input; a
// point's distance is a minimum of values that do not depend on the order; the statistics are summed in a fixed order.
#include <climits>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gsr_common.h"

namespace {

constexpr int MAX_FACES = 1 << 28;
constexpr int MAX_POINTS = 1 << 30;
constexpr int TPB = 256;
constexpr int NODE_END = INT_MIN;
constexpr int STATS_BLOCKS = 1024;
constexpr float SLACK = 1.f / 262144.f;            // 2^-18
constexpr float FLAT = 1.f / 1099511627776.f;      // 2^-40: |n|^2 <= FLAT |ab|^2 |ac|^2 counts as zero area

struct Header {  // first 256 bytes of the tree
  int32_t usable;   // Fu
  int32_t root;     // 0, or ~0 when Fu == 1
  float lo[3];      // scene bounds: the grid of the Morton codes
  float scale[3];   // 1024 / extent (0 for a flat axis)
};

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 along(V3 a, float t, V3 e) { return {a.x + t * e.x, a.y + t * e.y, a.z + t * e.z}; }
__device__ __forceinline__ bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }

// closest point of segment (a, a + e) to the origin; a zero-length segment is the point a
__device__ __forceinline__ V3 seg_closest(V3 a, V3 e) {
  const float ee = dot(e, e);
  float t = ee > 0.f ? -dot(a, e) / ee : 0.f;
  t = fminf(fmaxf(t, 0.f), 1.f);
  return along(a, t, e);
}

// Closest point of triangle (a, b, c) to the ORIGIN (the caller has translated by -p): the seven Voronoi regions
// (Ericson, Real-Time Collision Detection 5.1.5), every quotient guarded, and the three edges as segments when the
// triangle has no area to speak of or the rounded region tests contradict one another.
__device__ __forceinline__ V3 tri_closest(V3 a, V3 b, V3 c) {
  const V3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b);
  const V3 n = {ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x};
  const float d1 = -dot(ab, a), d2 = -dot(ac, a);
  const float d3 = -dot(ab, b), d4 = -dot(ac, b);
  const float d5 = -dot(ab, c), d6 = -dot(ac, c);
  const float va = d3 * d6 - d5 * d4, vb = d5 * d2 - d1 * d6, vc = d1 * d4 - d3 * d2;
  const bool flat = !(dot(n, n) > FLAT * (dot(ab, ab) * dot(ac, ac)));
  if (!flat) {
    if (d1 <= 0.f && d2 <= 0.f) return a;
    if (d3 >= 0.f && d4 <= d3) return b;
    if (d6 >= 0.f && d5 <= d6) return c;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
      const float den = d1 - d3;
      return along(a, den > 0.f ? d1 / den : 0.f, ab);
    }
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
      const float den = d2 - d6;
      return along(a, den > 0.f ? d2 / den : 0.f, ac);
    }
    const float e0 = d4 - d3, e1 = d5 - d6;
    if (va <= 0.f && e0 >= 0.f && e1 >= 0.f) {
      const float den = e0 + e1;
      return along(b, den > 0.f ? e0 / den : 0.f, bc);
    }
    if (va > 0.f && vb > 0.f && vc > 0.f) {
      const float sum = (va + vb) + vc;
      const float v = vb / sum, w = vc / sum;
      return along(along(a, v, ab), w, ac);
    }
  }
  const V3 q0 = seg_closest(a, ab), q1 = seg_closest(b, bc), q2 = seg_closest(a, ac);
  const float s0 = dot(q0, q0), s1 = dot(q1, q1), s2 = dot(q2, q2);
  V3 q = q0;
  float s = s0;
  if (s1 < s) q = q1, s = s1;
  if (s2 < s) q = q2;
  return q;
}

__device__ __forceinline__ float norm3(V3 q) { return sqrtf(dot(q, q)); }

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
enum { ST_BAD = 0, ST_SKIPPED = 1 };

__global__ void md_state_init_kernel(int32_t *state) {
  state[threadIdx.x] = threadIdx.x == ST_BAD ? INT_MAX : 0;
}

// index check (reads `triangles` only for a face that fails it), finiteness, centroid, bounds of the workgroup
__global__ __launch_bounds__(TPB) void md_prepare_kernel(const int F, const int V, const float *__restrict__ vtx,
                                                         const int32_t *__restrict__ tri, float4 *__restrict__ cent,
                                                         float *__restrict__ partial, int32_t *__restrict__ state) {
  __shared__ float red[6][TPB];
  __shared__ int skipped;
  const int f = blockIdx.x * TPB + threadIdx.x, t = threadIdx.x;
  if (t == 0) skipped = 0;
  __syncthreads();
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (f < F) {
    const int ia = tri[3 * (size_t)f], ib = tri[3 * (size_t)f + 1], ic = tri[3 * (size_t)f + 2];
    bool ok = false;
    V3 g = {0.f, 0.f, 0.f};
    if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) {
      atomicMin(&state[ST_BAD], f);  // (the lowest offender; nothing is read through these indices)
    } else {
      const float *pa = vtx + 3 * (size_t)ia, *pb = vtx + 3 * (size_t)ib, *pc = vtx + 3 * (size_t)ic;
      const V3 a = {pa[0], pa[1], pa[2]}, b = {pb[0], pb[1], pb[2]}, c = {pc[0], pc[1], pc[2]};
      ok = finite3(a) && finite3(b) && finite3(c);
      if (ok) {
        lo[0] = fminf(fminf(a.x, b.x), c.x), hi[0] = fmaxf(fmaxf(a.x, b.x), c.x);
        lo[1] = fminf(fminf(a.y, b.y), c.y), hi[1] = fmaxf(fmaxf(a.y, b.y), c.y);
        lo[2] = fminf(fminf(a.z, b.z), c.z), hi[2] = fmaxf(fmaxf(a.z, b.z), c.z);
        g = {((a.x + b.x) + c.x) * (1.f / 3.f), ((a.y + b.y) + c.y) * (1.f / 3.f), ((a.z + b.z) + c.z) * (1.f / 3.f)};
        ok = finite3(g);  // (a sum that overflows: left out like a non-finite vertex)
        if (!ok) lo[0] = lo[1] = lo[2] = INFINITY, hi[0] = hi[1] = hi[2] = -INFINITY;
      }
      if (!ok) atomicAdd(&skipped, 1);
    }
    cent[f] = make_float4(g.x, g.y, g.z, ok ? 1.f : 0.f);
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

__global__ __launch_bounds__(TPB) void md_bounds_kernel(const int blocks, const int F, const float *__restrict__ partial,
                                                        const int32_t *__restrict__ state, Header *__restrict__ h) {
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
    h->lo[t] = red[t][0];
    h->scale[t] = (ext > 0.f && isfinite(ext)) ? 1024.f / ext : 0.f;
  }
  if (t == 0) {
    const int usable = state[ST_BAD] != INT_MAX ? 0 : F - state[ST_SKIPPED];
    h->usable = usable;
    h->root = usable == 1 ? ~0 : 0;
  }
}

__global__ __launch_bounds__(TPB) void md_keys_kernel(const int F, const float4 *__restrict__ cent,
                                                      const Header *__restrict__ h, uint64_t *__restrict__ key,
                                                      int32_t *__restrict__ val) {
  const int f = blockIdx.x * TPB + threadIdx.x;
  if (f >= F) return;
  const float4 g = cent[f];
  key[f] = g.w != 0.f ? ((uint64_t)morton30({g.x, g.y, g.z}, h) << 32) | (uint32_t)f : ~0ull;
  val[f] = f;
}

// leaf l = the l-th triangle of the sorted order: (a | face), (b | escape, written by ropes), (c | 0)
__global__ __launch_bounds__(TPB) void md_gather_kernel(const int Fu, const float *__restrict__ vtx,
                                                        const int32_t *__restrict__ tri,
                                                        const uint64_t *__restrict__ key,
                                                        const int32_t *__restrict__ order, float4 *__restrict__ leaves,
                                                        uint32_t *__restrict__ leaf_code) {
  const int l = blockIdx.x * TPB + threadIdx.x;
  if (l >= Fu) return;
  const int f = order[l];
  const float *pa = vtx + 3 * (size_t)tri[3 * (size_t)f], *pb = vtx + 3 * (size_t)tri[3 * (size_t)f + 1],
              *pc = vtx + 3 * (size_t)tri[3 * (size_t)f + 2];
  leaves[3 * (size_t)l + 0] = make_float4(pa[0], pa[1], pa[2], __int_as_float(f));
  leaves[3 * (size_t)l + 1] = make_float4(pb[0], pb[1], pb[2], __int_as_float(NODE_END));
  leaves[3 * (size_t)l + 2] = make_float4(pc[0], pc[1], pc[2], 0.f);
  leaf_code[l] = (uint32_t)(key[l] >> 32);
}

// length of the common prefix of keys i and j, -1 outside [0, Fu) (Karras 2012; the keys are unique)
__device__ __forceinline__ int delta(const uint64_t *key, int Fu, int i, int j) {
  if (j < 0 || j >= Fu) return -1;
  return __clzll((long long)(key[i] ^ key[j]));
}

__global__ __launch_bounds__(TPB) void md_karras_kernel(const int Fu, const uint64_t *__restrict__ key,
                                                        float4 *__restrict__ nodes, int32_t *__restrict__ right,
                                                        int32_t *__restrict__ last, int32_t *__restrict__ after,
                                                        int32_t *__restrict__ parent_node,
                                                        int32_t *__restrict__ parent_leaf,
                                                        int32_t *__restrict__ counter) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= Fu - 1) return;
  const int d = delta(key, Fu, i, i + 1) > delta(key, Fu, i, i - 1) ? 1 : -1;
  const int dmin = delta(key, Fu, i, i - d);
  int lmax = 2;
  while (delta(key, Fu, i, i + lmax * d) > dmin) lmax <<= 1;  // (at most 2 Fu: the index leaves [0, Fu))
  int len = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(key, Fu, i, i + (len + t) * d) > dmin) len += t;
  const int j = i + len * d;
  const int dnode = delta(key, Fu, i, j);
  int s = 0;
  for (int t = (len + 1) >> 1;; t = (t + 1) >> 1) {
    if (delta(key, Fu, i, i + (s + t) * d) > dnode) s += t;
    if (t == 1) break;
  }
  const int split = i + s * d + min(d, 0);
  const int first = min(i, j), lst = max(i, j);
  const int L = first == split ? ~split : split;
  const int R = lst == split + 1 ? ~(split + 1) : split + 1;
  reinterpret_cast<int32_t *>(nodes + 2 * (size_t)i)[3] = L;
  right[i] = R;
  last[i] = lst;
  after[split] = R;
  counter[i] = 0;
  if (L < 0) parent_leaf[~L] = i; else parent_node[L] = i;
  if (R < 0) parent_leaf[~R] = i; else parent_node[R] = i;
  if (i == 0) parent_node[0] = -1;
}

__global__ __launch_bounds__(TPB) void md_ropes_kernel(const int Fu, const int32_t *__restrict__ last,
                                                       const int32_t *__restrict__ after, float4 *__restrict__ nodes,
                                                       float4 *__restrict__ leaves) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= Fu) return;
  if (i < Fu - 1) {
    const int e = last[i];
    reinterpret_cast<int32_t *>(nodes + 2 * (size_t)i + 1)[3] = e == Fu - 1 ? NODE_END : after[e];
  }
  reinterpret_cast<int32_t *>(leaves + 3 * (size_t)i + 1)[3] = i == Fu - 1 ? NODE_END : after[i];
}

struct Box {
  float lo[3], hi[3];
};
__device__ __forceinline__ Box leaf_box(const float4 *leaves, int l) {
  const float4 a = leaves[3 * (size_t)l], b = leaves[3 * (size_t)l + 1], c = leaves[3 * (size_t)l + 2];
  Box x;
  x.lo[0] = fminf(fminf(a.x, b.x), c.x), x.hi[0] = fmaxf(fmaxf(a.x, b.x), c.x);
  x.lo[1] = fminf(fminf(a.y, b.y), c.y), x.hi[1] = fmaxf(fmaxf(a.y, b.y), c.y);
  x.lo[2] = fminf(fminf(a.z, b.z), c.z), x.hi[2] = fmaxf(fmaxf(a.z, b.z), c.z);
  return x;
}
// A node's box is handed from the thread that finished it to the thread that arrives second at its parent, within
// one launch and possibly across XCDs: every word of it is stored and loaded with device-scope atomics, with a fence
// between the stores and the arrival counter and another between the counter and the loads.
__device__ __forceinline__ void store_box(float4 *nodes, int i, const Box &x) {
  uint32_t *r0 = reinterpret_cast<uint32_t *>(nodes + 2 * (size_t)i), *r1 = r0 + 4;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    __hip_atomic_store(r0 + k, __float_as_uint(x.lo[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(r1 + k, __float_as_uint(x.hi[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__device__ __forceinline__ Box load_box(float4 *nodes, int i) {
  uint32_t *r0 = reinterpret_cast<uint32_t *>(nodes + 2 * (size_t)i), *r1 = r0 + 4;
  Box x;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x.lo[k] = __uint_as_float(__hip_atomic_load(r0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    x.hi[k] = __uint_as_float(__hip_atomic_load(r1 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  return x;
}

// one thread per leaf climbs; at every internal node the first arrival stops, the second merges and goes on
// (at most Fu - 1 merges in all, at most the tree's depth <= 64 per thread)
__global__ __launch_bounds__(TPB) void md_refit_kernel(const int Fu, const float4 *__restrict__ leaves,
                                                       float4 *nodes, const int32_t *__restrict__ right,
                                                       const int32_t *__restrict__ parent_node,
                                                       const int32_t *__restrict__ parent_leaf, int32_t *counter) {
  const int l = blockIdx.x * TPB + threadIdx.x;
  if (l >= Fu || Fu < 2) return;
  Box box = leaf_box(leaves, l);
  int child = ~l, p = parent_leaf[l];
  while (p >= 0) {
    __threadfence();  // (the box of `child`, stored below on the way up, before the arrival)
    if (atomicAdd(counter + p, 1) == 0) return;
    __threadfence();
    const int L = reinterpret_cast<const int32_t *>(nodes + 2 * (size_t)p)[3], R = right[p];
    const int sib = child == L ? R : L;
    const Box o = sib < 0 ? leaf_box(leaves, ~sib) : load_box(nodes, sib);
#pragma unroll
    for (int k = 0; k < 3; ++k) box.lo[k] = fminf(box.lo[k], o.lo[k]), box.hi[k] = fmaxf(box.hi[k], o.hi[k]);
    store_box(nodes, p, box);
    child = p;
    p = parent_node[p];
  }
}

// ---- query -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void md_point_keys_kernel(const int n, const float *__restrict__ pts,
                                                            const Header *__restrict__ h, uint32_t *__restrict__ key,
                                                            int32_t *__restrict__ val) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const V3 p = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
  key[i] = finite3(p) ? morton30(p, h) : 0xffffffffu;
  val[i] = i;
}

struct Best {
  float d;
  int face;
  V3 q;
};
__device__ __forceinline__ void leaf_test(const float4 ra, const float4 rb, const float4 rc, const V3 p, Best &best) {
  const V3 q = tri_closest({ra.x - p.x, ra.y - p.y, ra.z - p.z}, {rb.x - p.x, rb.y - p.y, rb.z - p.z},
                           {rc.x - p.x, rc.y - p.y, rc.z - p.z});
  const float d = norm3(q);
  if (d < best.d) best.d = d, best.face = __float_as_int(ra.w), best.q = q;
}
__device__ __forceinline__ void write_result(const int row, const V3 p, const Best &best, float *dist, int32_t *face,
                                             float *closest) {
  dist[row] = best.d;
  face[row] = best.face;
  if (closest) {
    closest[3 * (size_t)row + 0] = p.x + best.q.x;
    closest[3 * (size_t)row + 1] = p.y + best.q.y;
    closest[3 * (size_t)row + 2] = p.z + best.q.z;
  }
}
__device__ __forceinline__ void write_invalid(const int row, float *dist, int32_t *face, float *closest) {
  dist[row] = NAN;
  face[row] = -1;
  if (closest) closest[3 * (size_t)row] = closest[3 * (size_t)row + 1] = closest[3 * (size_t)row + 2] = NAN;
}

__global__ __launch_bounds__(TPB) void md_query_kernel(const int n, const int32_t *__restrict__ order,
                                                       const float *__restrict__ pts, const Header *__restrict__ h,
                                                       const float4 *__restrict__ leaves,
                                                       const float4 *__restrict__ nodes,
                                                       const uint32_t *__restrict__ leaf_code,
                                                       float *__restrict__ dist, int32_t *__restrict__ face,
                                                       float *__restrict__ closest) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int row = order[i];
  if ((unsigned)row >= (unsigned)n) return;  // (never: `order` is a permutation written by this call)
  const V3 p = {pts[3 * (size_t)row], pts[3 * (size_t)row + 1], pts[3 * (size_t)row + 2]};
  const int Fu = h->usable;
  if (!finite3(p) || Fu <= 0) {
    write_invalid(row, dist, face, closest);
    return;
  }
  // seed: the leaf whose code is nearest the point's
  const uint32_t code = morton30(p, h);
  int lo = 0, hi = Fu;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (leaf_code[mid] < code) lo = mid + 1; else hi = mid;
  }
  int seed = min(lo, Fu - 1);
  if (lo > 0 && lo < Fu && code - leaf_code[lo - 1] < leaf_code[lo] - code) seed = lo - 1;
  Best best = {INFINITY, -1, {0.f, 0.f, 0.f}};
  leaf_test(leaves[3 * (size_t)seed], leaves[3 * (size_t)seed + 1], leaves[3 * (size_t)seed + 2], p, best);
  int node = h->root;
  while (node != NODE_END) {
    if (node >= 0) {
      const float4 r0 = nodes[2 * (size_t)node], r1 = nodes[2 * (size_t)node + 1];
      const float ax = r0.x - p.x, ay = r0.y - p.y, az = r0.z - p.z;
      const float bx = p.x - r1.x, by = p.y - r1.y, bz = p.z - r1.z;
      const float dx = fmaxf(fmaxf(ax, bx), 0.f), dy = fmaxf(fmaxf(ay, by), 0.f), dz = fmaxf(fmaxf(az, bz), 0.f);
      const float db2 = (dx * dx + dy * dy) + dz * dz;
      const float R = fmaxf(fmaxf(fmaxf(fabsf(ax), fabsf(bx)), fmaxf(fabsf(ay), fabsf(by))), fmaxf(fabsf(az), fabsf(bz)));
      const float reach = best.d + SLACK * R;
      node = db2 > reach * reach ? __float_as_int(r1.w) : __float_as_int(r0.w);
    } else {
      const int l = ~node;
      const float4 ra = leaves[3 * (size_t)l], rb = leaves[3 * (size_t)l + 1], rc = leaves[3 * (size_t)l + 2];
      leaf_test(ra, rb, rc, p, best);
      node = __float_as_int(rb.w);
    }
  }
  write_result(row, p, best, dist, face, closest);
}

// every point against every leaf, TPB leaves at a time through LDS (every lane reads the same row: a broadcast)
__global__ __launch_bounds__(TPB) void md_exhaustive_kernel(const int n, const float *__restrict__ pts,
                                                            const Header *__restrict__ h,
                                                            const float4 *__restrict__ leaves,
                                                            float *__restrict__ dist, int32_t *__restrict__ face,
                                                            float *__restrict__ closest) {
  __shared__ float4 tile[3 * TPB];
  const int i = blockIdx.x * TPB + threadIdx.x;
  const int Fu = h->usable;
  V3 p = {0.f, 0.f, 0.f};
  if (i < n) p = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
  const bool live = i < n && finite3(p) && Fu > 0;
  Best best = {INFINITY, -1, {0.f, 0.f, 0.f}};
  for (int base = 0; base < Fu; base += TPB) {  // (Fu is uniform: every thread reaches the barriers)
    const int count = min(TPB, Fu - base);
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * count; k += TPB) tile[k] = leaves[3 * (size_t)base + k];
    __syncthreads();
    if (live)
      for (int k = 0; k < count; ++k) leaf_test(tile[3 * k], tile[3 * k + 1], tile[3 * k + 2], p, best);
  }
  if (i >= n) return;
  if (live) write_result(i, p, best, dist, face, closest); else write_invalid(i, dist, face, closest);
}

// ---- statistics ------------------------------------------------------------------------------------------------------
// partial / result rows: 0 valid count, 1 invalid count, 2 sum, 3 sum of squares, 4 max, 5 count of d <= threshold
__device__ __forceinline__ void stats_merge(double *a, const double *b) {
  a[0] += b[0], a[1] += b[1], a[2] += b[2], a[3] += b[3], a[4] = fmax(a[4], b[4]), a[5] += b[5];
}
__device__ __forceinline__ void stats_block_reduce(double *v, double (*red)[TPB]) {
  const int t = threadIdx.x;
  for (int k = 0; k < 6; ++k) red[k][t] = v[k];
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s) {
      double a[6], b[6];
      for (int k = 0; k < 6; ++k) a[k] = red[k][t], b[k] = red[k][t + s];
      stats_merge(a, b);
      for (int k = 0; k < 6; ++k) red[k][t] = a[k];
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(TPB) void md_stats_partial_kernel(const int n, const float *__restrict__ dist,
                                                               const float tau, double *__restrict__ partial) {
  __shared__ double red[6][TPB];
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * TPB) {
    const float d = dist[i];
    if (isfinite(d)) {
      const double x = (double)d;
      v[0] += 1, v[2] += x, v[3] += x * x, v[4] = fmax(v[4], x), v[5] += d <= tau ? 1 : 0;
    } else {
      v[1] += 1;
    }
  }
  stats_block_reduce(v, red);
  if (threadIdx.x < 6) partial[6 * (size_t)blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}
// stats: 0 count, 1 invalid, 2 mean, 3 rms, 4 max, 5 within, 6 sum, 7 sum of squares (mean, rms, max 0 without a count)
__global__ __launch_bounds__(TPB) void md_stats_final_kernel(const int blocks, const double *__restrict__ partial,
                                                             double *__restrict__ stats) {
  __shared__ double red[6][TPB];
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (int b = threadIdx.x; b < blocks; b += TPB) stats_merge(v, partial + 6 * (size_t)b);
  stats_block_reduce(v, red);
  if (threadIdx.x == 0) {
    const double c = red[0][0];
    stats[0] = c, stats[1] = red[1][0];
    stats[2] = c > 0 ? red[2][0] / c : 0.0;
    stats[3] = c > 0 ? sqrt(red[3][0] / c) : 0.0;
    stats[4] = red[4][0], stats[5] = red[5][0], stats[6] = red[2][0], stats[7] = red[3][0];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Tree {
  Header *header;
  float4 *leaves;       // [3F]
  float4 *nodes;        // [2 max(F - 1, 1)]
  uint32_t *leaf_code;  // [F]
};
size_t carve_tree(int F, void *mem, Tree *t) {
  const size_t head = 256, lv = align_up((size_t)3 * F * 16), nd = align_up((size_t)2 * (F > 1 ? F - 1 : 1) * 16);
  const size_t lc = align_up((size_t)F * 4);
  if (t) {
    char *p = static_cast<char *>(mem);
    t->header = reinterpret_cast<Header *>(p);
    t->leaves = reinterpret_cast<float4 *>(p + head);
    t->nodes = reinterpret_cast<float4 *>(p + head + lv);
    t->leaf_code = reinterpret_cast<uint32_t *>(p + head + lv + nd);
  }
  return head + lv + nd + lc;
}

struct BuildSpace {
  uint64_t *key_in, *key_out;  // [F]
  float4 *cent;                // [F]
  int32_t *val_in, *val_out, *right, *last, *after, *parent_node, *parent_leaf, *counter;  // [F]
  float *partial;              // [6 blocks]
  char *temp;
  size_t temp_bytes;
};
size_t carve_build(int F, void *mem, size_t bytes, BuildSpace *w) {
  const size_t f8 = align_up((size_t)F * 8), f16 = align_up((size_t)F * 16), f4 = align_up((size_t)F * 4);
  const size_t pb = align_up((size_t)gsr_cdiv(F, TPB) * 6 * 4);
  const size_t head = 2 * f8 + f16 + 8 * f4 + pb;
  if (w) {
    char *p = static_cast<char *>(mem);
    auto take = [&p](size_t n) { char *q = p; p += n; return q; };
    w->key_in = reinterpret_cast<uint64_t *>(take(f8));
    w->key_out = reinterpret_cast<uint64_t *>(take(f8));
    w->cent = reinterpret_cast<float4 *>(take(f16));
    int32_t **per_face[8] = {&w->val_in, &w->val_out, &w->right, &w->last, &w->after, &w->parent_node, &w->parent_leaf,
                             &w->counter};
    for (auto **q : per_face) *q = reinterpret_cast<int32_t *>(take(f4));
    w->partial = reinterpret_cast<float *>(take(pb));
    w->temp = p;
    w->temp_bytes = bytes - head;
  }
  return head;
}

struct QuerySpace {
  uint32_t *key_in, *key_out;  // [n]
  int32_t *val_in, *val_out;   // [n]
  char *temp;
  size_t temp_bytes;
};
size_t carve_query(int n, void *mem, size_t bytes, QuerySpace *w) {
  const size_t n4 = align_up((size_t)n * 4);
  if (w) {
    char *p = static_cast<char *>(mem);
    w->key_in = reinterpret_cast<uint32_t *>(p);
    w->key_out = reinterpret_cast<uint32_t *>(p + n4);
    w->val_in = reinterpret_cast<int32_t *>(p + 2 * n4);
    w->val_out = reinterpret_cast<int32_t *>(p + 3 * n4);
    w->temp = p + 4 * n4;
    w->temp_bytes = bytes - 4 * n4;
  }
  return 4 * n4;
}

bool build_temp_bytes(int F, size_t *out) {
  return rocprim::radix_sort_pairs(nullptr, *out, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                   (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)F, 0, 64) == hipSuccess;
}
bool query_temp_bytes(int n, size_t *out) {
  return rocprim::radix_sort_pairs(nullptr, *out, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                   (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)n, 0, 32) == hipSuccess;
}
int stats_blocks(int n) { return (int)(gsr_cdiv(n, TPB) < (unsigned)STATS_BLOCKS ? gsr_cdiv(n, TPB) : STATS_BLOCKS); }

int check_space(const void *ws, size_t have, size_t need, const char *who, const char *what) {
  GSR_REQUIRE(need != 0, "%s: the %s size query failed", who, what);
  if (have < need || !ws) {
    gsr_set_error("%s: %s %zu < %zu bytes", who, what, have, need);
    return GSR_ENOMEM;
  }
  GSR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: %s must be 256-byte aligned", who, what);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT size_t gsr_mesh_distance_workspace_bytes(int what, int num_faces, int num_points) {
  const int F = num_faces, n = num_points;
  size_t temp = 0;
  switch (what) {
    case GSR_MESH_DISTANCE_BYTES_TREE:
      return F <= 0 || F > MAX_FACES ? 0 : carve_tree(F, nullptr, nullptr);
    case GSR_MESH_DISTANCE_BYTES_BUILD:
      if (F <= 0 || F > MAX_FACES || !build_temp_bytes(F, &temp)) return 0;
      return carve_build(F, nullptr, 0, nullptr) + align_up(temp);
    case GSR_MESH_DISTANCE_BYTES_QUERY:
      if (n <= 0 || n > MAX_POINTS || !query_temp_bytes(n, &temp)) return 0;
      return carve_query(n, nullptr, 0, nullptr) + align_up(temp);
    case GSR_MESH_DISTANCE_BYTES_STATS:
      return n <= 0 || n > MAX_POINTS ? 0 : align_up((size_t)stats_blocks(n) * 6 * 8);
    default:
      return 0;
  }
}

GSR_EXPORT int gsr_mesh_bvh_build(int num_vertices, int num_faces, const float *vertices, const int32_t *triangles,
                                  void *tree, size_t tree_bytes, void *workspace, size_t workspace_bytes,
                                  int32_t *state, gsr_stream_t stream) {
  const int V = num_vertices, F = num_faces;
  GSR_REQUIRE(V >= 0, "mesh_bvh_build: num_vertices < 0");
  GSR_REQUIRE(F >= 1 && F <= MAX_FACES, "mesh_bvh_build: num_faces must be in [1, %d]", MAX_FACES);
  GSR_REQUIRE(triangles != nullptr && state != nullptr && (vertices != nullptr || V == 0),
              "mesh_bvh_build: null pointer");
  if (int rc = check_space(tree, tree_bytes, gsr_mesh_distance_workspace_bytes(GSR_MESH_DISTANCE_BYTES_TREE, F, 0),
                           "mesh_bvh_build", "tree"))
    return rc;
  if (int rc = check_space(workspace, workspace_bytes,
                           gsr_mesh_distance_workspace_bytes(GSR_MESH_DISTANCE_BYTES_BUILD, F, 0), "mesh_bvh_build",
                           "workspace"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Tree t;
  BuildSpace w;
  carve_tree(F, tree, &t);
  carve_build(F, workspace, workspace_bytes, &w);
  const unsigned blocks = gsr_cdiv(F, TPB);
  const dim3 gf(blocks), tpb(TPB);
  hipLaunchKernelGGL(md_state_init_kernel, dim3(1), dim3(4), 0, s, state);
  GSR_CHECK_LAUNCH("md_state_init");
  hipLaunchKernelGGL(md_prepare_kernel, gf, tpb, 0, s, F, V, vertices, triangles, w.cent, w.partial, state);
  GSR_CHECK_LAUNCH("md_prepare");
  hipLaunchKernelGGL(md_bounds_kernel, dim3(1), tpb, 0, s, (int)blocks, F, (const float *)w.partial,
                     (const int32_t *)state, t.header);
  GSR_CHECK_LAUNCH("md_bounds");
  int st[2] = {0, 0};
  GSR_CHECK_HIP(hipMemcpyAsync(st, state, sizeof(st), hipMemcpyDeviceToHost, s));
  GSR_CHECK_HIP(hipStreamSynchronize(s));
  if (st[ST_BAD] != INT_MAX) {
    gsr_set_error("mesh_bvh_build: triangle %d has a vertex index outside [0, %d)", st[ST_BAD], V);
    return GSR_ERANGE;
  }
  const int Fu = F - st[ST_SKIPPED];
  if (Fu <= 0) return GSR_OK;  // (the header says so: every query answers NaN; the caller reads state[1])
  hipLaunchKernelGGL(md_keys_kernel, gf, tpb, 0, s, F, (const float4 *)w.cent, (const Header *)t.header, w.key_in,
                     w.val_in);
  GSR_CHECK_LAUNCH("md_keys");
  size_t tb = w.temp_bytes;
  GSR_CHECK_HIP(rocprim::radix_sort_pairs(w.temp, tb, (const uint64_t *)w.key_in, w.key_out, (const int32_t *)w.val_in,
                                          w.val_out, (size_t)F, 0, 64, s));
  const dim3 gu(gsr_cdiv(Fu, TPB));
  hipLaunchKernelGGL(md_gather_kernel, gu, tpb, 0, s, Fu, vertices, triangles, (const uint64_t *)w.key_out,
                     (const int32_t *)w.val_out, t.leaves, t.leaf_code);
  GSR_CHECK_LAUNCH("md_gather");
  if (Fu >= 2) {
    hipLaunchKernelGGL(md_karras_kernel, gu, tpb, 0, s, Fu, (const uint64_t *)w.key_out, t.nodes, w.right, w.last,
                       w.after, w.parent_node, w.parent_leaf, w.counter);
    GSR_CHECK_LAUNCH("md_karras");
    hipLaunchKernelGGL(md_ropes_kernel, gu, tpb, 0, s, Fu, (const int32_t *)w.last, (const int32_t *)w.after, t.nodes,
                       t.leaves);
    GSR_CHECK_LAUNCH("md_ropes");
    hipLaunchKernelGGL(md_refit_kernel, gu, tpb, 0, s, Fu, (const float4 *)t.leaves, t.nodes, (const int32_t *)w.right,
                       (const int32_t *)w.parent_node, (const int32_t *)w.parent_leaf, w.counter);
    GSR_CHECK_LAUNCH("md_refit");
  }
  return GSR_OK;
}

GSR_EXPORT int gsr_mesh_distance_query(int num_faces, const void *tree, size_t tree_bytes, int num_points,
                                       const float *points, int flags, void *workspace, size_t workspace_bytes,
                                       float *distance, int32_t *face, float *closest, gsr_stream_t stream) {
  const int F = num_faces, n = num_points;
  GSR_REQUIRE(F >= 1 && F <= MAX_FACES, "mesh_distance_query: num_faces must be in [1, %d]", MAX_FACES);
  GSR_REQUIRE(n >= 0 && n <= MAX_POINTS, "mesh_distance_query: num_points must be in [0, %d]", MAX_POINTS);
  GSR_REQUIRE((flags & ~GSR_MESH_DISTANCE_EXHAUSTIVE) == 0, "mesh_distance_query: unknown flags %d", flags);
  if (n == 0) return GSR_OK;
  GSR_REQUIRE(points && distance && face, "mesh_distance_query: null pointer");
  if (int rc = check_space(tree, tree_bytes, gsr_mesh_distance_workspace_bytes(GSR_MESH_DISTANCE_BYTES_TREE, F, 0),
                           "mesh_distance_query", "tree"))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  Tree t;
  carve_tree(F, const_cast<void *>(tree), &t);
  const dim3 gn(gsr_cdiv(n, TPB)), tpb(TPB);
  if (flags & GSR_MESH_DISTANCE_EXHAUSTIVE) {
    hipLaunchKernelGGL(md_exhaustive_kernel, gn, tpb, 0, s, n, points, (const Header *)t.header,
                       (const float4 *)t.leaves, distance, face, closest);
    GSR_CHECK_LAUNCH("md_exhaustive");
    return GSR_OK;
  }
  if (int rc = check_space(workspace, workspace_bytes,
                           gsr_mesh_distance_workspace_bytes(GSR_MESH_DISTANCE_BYTES_QUERY, 0, n),
                           "mesh_distance_query", "workspace"))
    return rc;
  QuerySpace w;
  carve_query(n, workspace, workspace_bytes, &w);
  hipLaunchKernelGGL(md_point_keys_kernel, gn, tpb, 0, s, n, points, (const Header *)t.header, w.key_in, w.val_in);
  GSR_CHECK_LAUNCH("md_point_keys");
  size_t tb = w.temp_bytes;
  GSR_CHECK_HIP(rocprim::radix_sort_pairs(w.temp, tb, (const uint32_t *)w.key_in, w.key_out, (const int32_t *)w.val_in,
                                          w.val_out, (size_t)n, 0, 32, s));
  hipLaunchKernelGGL(md_query_kernel, gn, tpb, 0, s, n, (const int32_t *)w.val_out, points, (const Header *)t.header,
                     (const float4 *)t.leaves, (const float4 *)t.nodes, (const uint32_t *)t.leaf_code, distance, face,
                     closest);
  GSR_CHECK_LAUNCH("md_query");
  return GSR_OK;
}

GSR_EXPORT int gsr_mesh_distance_stats(int num_points, const float *distance, float threshold, void *workspace,
                                       size_t workspace_bytes, double *stats, gsr_stream_t stream) {
  const int n = num_points;
  GSR_REQUIRE(n >= 0 && n <= MAX_POINTS, "mesh_distance_stats: num_points must be in [0, %d]", MAX_POINTS);
  GSR_REQUIRE(stats != nullptr && (distance != nullptr || n == 0), "mesh_distance_stats: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const int blocks = n ? stats_blocks(n) : 0;
  if (n)
    if (int rc = check_space(workspace, workspace_bytes,
                             gsr_mesh_distance_workspace_bytes(GSR_MESH_DISTANCE_BYTES_STATS, 0, n),
                             "mesh_distance_stats", "workspace"))
      return rc;
  double *partial = static_cast<double *>(workspace);
  if (n) {
    hipLaunchKernelGGL(md_stats_partial_kernel, dim3(blocks), dim3(TPB), 0, s, n, distance, threshold, partial);
    GSR_CHECK_LAUNCH("md_stats_partial");
  }
  hipLaunchKernelGGL(md_stats_final_kernel, dim3(1), dim3(TPB), 0, s, blocks, (const double *)partial, stats);
  GSR_CHECK_LAUNCH("md_stats_final");
  return GSR_OK;
}
