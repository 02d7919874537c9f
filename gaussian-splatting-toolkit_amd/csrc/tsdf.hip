// tsdf.hip -- TSDF fusion of rendered depth / colour into a block-sparse volume, and surface extraction
// (the rules and the buffers are in include/gsraster.h).
//
// Compiled with -ffp-contract=off (Makefile): the float32 NumPy oracle of the tests performs the same operations in
// the same order, and with correctly rounded division and square root the results are the same bits.
//
// Per view: touch (one thread per pixel, byte flags, no atomics) -> allocate (one rocPRIM scan over the block
// grid gives both the slot numbers and the compacted list) -> integrate (one workgroup per listed block, one thread
// per voxel, a fixed grid looping over the device-side list: nothing is read back and no grid is sized by the pool).
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gsr_common.h"

namespace {

constexpr int VOX = 512;                // voxels of a block = threads of a workgroup
constexpr int LIST_NEW = 1 << 30;       // list entry: the slot was handed out by this view
constexpr int MAX_BLOCKS = LIST_NEW - 1;
constexpr int MAX_CAPACITY = (1 << 22) - 1;  // capacity * 512 fits an int
constexpr int GRID = 2048;              // workgroups of the kernels that loop over blocks
constexpr float QUALIFY = 0.98f;

enum { ST_ALLOCATED = 0, ST_LIST = 1, ST_OVERFLOW = 2, ST_NEEDED = 3, ST_PENDING = 4, ST_POINTS = 5, ST_VERTICES = 6,
       ST_TRIANGLES = 7 };

__device__ __forceinline__ float row3(const float *m, float x, float y, float z) {
  return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}
__device__ __forceinline__ float centre(const gsr_tsdf_volume &vol, int a, int i) {
  return vol.origin[a] + ((float)i + 0.5f) * vol.voxel_length;
}
__device__ __forceinline__ bool pixel_usable(const gsr_tsdf_view &vw, unsigned p, float d) {
  if (!(d > 0.f && d <= vw.depth_trunc)) return false;
  return vw.valid == nullptr || vw.valid[p] != 0;
}

// ---- step 1: touch ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_touch_kernel(const gsr_tsdf_volume vol, const gsr_tsdf_view vw,
                                                         uint8_t *__restrict__ flags) {
  const unsigned p = blockIdx.x * 256u + threadIdx.x;
  if (p >= vw.height * vw.width) return;
  const unsigned i = p / vw.width, j = p - i * vw.width;
  const float d = vw.depth[p];
  if (!pixel_usable(vw, p, d)) return;
  const float xn = (((float)j + 0.5f) - vw.cx) / vw.fx;
  const float yn = (((float)i + 0.5f) - vw.cy) / vw.fy;
  const float x = xn * d, y = yn * d;
  const float l8 = 8.f * vol.voxel_length;
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float pw = row3(vw.cam2world + 4 * a, x, y, d);
    float l = floorf(((pw - vol.sdf_trunc) - vol.origin[a]) / l8);
    float h = floorf(((pw + vol.sdf_trunc) - vol.origin[a]) / l8);
    l = fmaxf(l, 0.f);
    h = fminf(h, (float)(vol.blocks[a] - 1));
    if (!(l <= h)) return;  // outside the volume (or not a number)
    lo[a] = (int)l;
    hi[a] = (int)h;
  }
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y_ = lo[1]; y_ <= hi[1]; ++y_)
      for (int x_ = lo[0]; x_ <= hi[0]; ++x_) {
        uint8_t *f = flags + ((size_t)z * vol.blocks[1] + y_) * vol.blocks[0] + x_;
        if (*f == 0) *f = 1;  // every writer stores the same value: no atomics (the read only spares stores)
      }
}

// ---- step 2: allocate ------------------------------------------------------------------------------------------------
// scanned value of a block: (flagged and without a slot) << 32 | flagged
struct AllocInput {
  const uint8_t *flags;
  const int32_t *table;
  __device__ unsigned long long operator()(int b) const {
    const unsigned long long fl = flags[b] != 0;
    return ((fl && table[b] < 0) ? (1ull << 32) : 0ull) | fl;
  }
};

__global__ __launch_bounds__(256) void tsdf_alloc_apply_kernel(const gsr_tsdf_volume vol, uint8_t *__restrict__ flags,
                                                               int32_t *__restrict__ list,
                                                               const unsigned long long *__restrict__ scan,
                                                               const int nb) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  const int base = vol.state[ST_ALLOCATED];  // (written by tsdf_alloc_commit_kernel only)
  const bool fl = flags[b] != 0;
  const unsigned long long s = scan[b];
  const int before_new = (int)(s >> 32), before_flagged = (int)(s & 0xffffffffu);
  const bool is_new = fl && vol.table[b] < 0;
  if (fl) {
    flags[b] = 0;
    // slots go out in ascending block index, so what does not fit is a suffix of this view's new blocks
    const int dropped = max(0, base + before_new - vol.capacity);
    if (!is_new) {
      list[before_flagged - dropped] = b;
    } else if (base + before_new < vol.capacity) {
      vol.table[b] = base + before_new;
      list[before_flagged - dropped] = b | LIST_NEW;
    }
  }
  if (b == nb - 1) {
    const int want = base + before_new + (is_new ? 1 : 0);
    const int dropped = max(0, want - vol.capacity);
    vol.state[ST_PENDING] = min(want, vol.capacity);
    vol.state[ST_LIST] = before_flagged + (fl ? 1 : 0) - dropped;
    if (dropped > 0) vol.state[ST_OVERFLOW] = 1;
    vol.state[ST_NEEDED] = max(vol.state[ST_NEEDED], want);
  }
}

__global__ void tsdf_alloc_commit_kernel(int32_t *state) { state[ST_ALLOCATED] = state[ST_PENDING]; }

// ---- step 3: integrate -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VOX) void tsdf_integrate_kernel(const gsr_tsdf_volume vol, const gsr_tsdf_view vw,
                                                             const int32_t *__restrict__ list) {
  const int count = vol.state[ST_LIST];
  const int v = threadIdx.x;
  const int lx = v & 7, ly = (v >> 3) & 7, lz = v >> 6;
  for (int k = blockIdx.x; k < count; k += gridDim.x) {
    const int e = list[k];
    const bool fresh = (e & LIST_NEW) != 0;  // pool rows of a slot handed out by this view hold nothing yet
    const int b = e & (LIST_NEW - 1);
    const int slot = vol.table[b];
    const size_t idx = (size_t)slot * VOX + v;
    float t = 0.f, w = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (!fresh) {
      t = vol.tsdf[idx];
      w = vol.weight[idx];
      c0 = vol.color[3 * idx + 0];
      c1 = vol.color[3 * idx + 1];
      c2 = vol.color[3 * idx + 2];
    }
    const int bx = b % vol.blocks[0], by = (b / vol.blocks[0]) % vol.blocks[1], bz = b / (vol.blocks[0] * vol.blocks[1]);
    const float px = centre(vol, 0, bx * 8 + lx), py = centre(vol, 1, by * 8 + ly), pz = centre(vol, 2, bz * 8 + lz);
    const float cx_ = row3(vw.viewmat + 0, px, py, pz);
    const float cy_ = row3(vw.viewmat + 4, px, py, pz);
    const float cz_ = row3(vw.viewmat + 8, px, py, pz);
    bool upd = cz_ > 0.f;
    if (upd) {
      const float u = vw.fx * (cx_ / cz_) + vw.cx;
      const float vv = vw.fy * (cy_ / cz_) + vw.cy;
      const float ju = floorf(u), iv = floorf(vv);
      upd = ju >= 0.f && ju < (float)vw.width && iv >= 0.f && iv < (float)vw.height;
      if (upd) {
        const unsigned j = (unsigned)ju, i = (unsigned)iv;
        const unsigned p = i * vw.width + j;
        const float d = vw.depth[p];
        upd = pixel_usable(vw, p, d);
        if (upd) {
          const float xn = (((float)j + 0.5f) - vw.cx) / vw.fx;
          const float yn = (((float)i + 0.5f) - vw.cy) / vw.fy;
          const float m = sqrtf((1.f + xn * xn) + yn * yn);
          const float sdf = (d - cz_) * m;
          upd = sdf > -vol.sdf_trunc;
          if (upd) {
            const float f = fminf(1.f, sdf / vol.sdf_trunc);
            const float w1 = w + 1.f;
            t = (t * w + f) / w1;
            c0 = (c0 * w + vw.color[3 * (size_t)p + 0]) / w1;
            c1 = (c1 * w + vw.color[3 * (size_t)p + 1]) / w1;
            c2 = (c2 * w + vw.color[3 * (size_t)p + 2]) / w1;
            w = w1;
          }
        }
      }
    }
    if (upd || fresh) {
      vol.tsdf[idx] = t;
      vol.weight[idx] = w;
      vol.color[3 * idx + 0] = c0;
      vol.color[3 * idx + 1] = c1;
      vol.color[3 * idx + 2] = c2;
    }
  }
}

// ---- extraction: shared pieces -----------------------------------------------------------------------------------------
// voxel (gx,gy,gz) of the whole grid -> its pool index, or -1 outside the volume / in a block without a slot
__device__ __forceinline__ int voxel_index(const gsr_tsdf_volume &vol, int gx, int gy, int gz) {
  if ((unsigned)gx >= (unsigned)(vol.blocks[0] * 8) || (unsigned)gy >= (unsigned)(vol.blocks[1] * 8) ||
      (unsigned)gz >= (unsigned)(vol.blocks[2] * 8))
    return -1;
  const int slot = vol.table[((gz >> 3) * vol.blocks[1] + (gy >> 3)) * vol.blocks[0] + (gx >> 3)];
  if (slot < 0) return -1;
  return slot * VOX + ((((gz & 7) << 3) | (gy & 7)) << 3 | (gx & 7));
}
__device__ __forceinline__ bool qualifies(float f, float w) { return w > 0.f && fabsf(f) < QUALIFY; }
// -> observed and |f| < 0.98; f is 0 where nothing is stored
__device__ __forceinline__ bool fetch(const gsr_tsdf_volume &vol, int gx, int gy, int gz, float &f, int &idx) {
  idx = voxel_index(vol, gx, gy, gz);
  f = 0.f;
  if (idx < 0) return false;
  f = vol.tsdf[idx];
  return qualifies(f, vol.weight[idx]);
}
// central difference over observed neighbours; a missing neighbour is replaced by the centre value
__device__ __forceinline__ void gradient(const gsr_tsdf_volume &vol, const int g[3], float f, float out[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int gp[3] = {g[0], g[1], g[2]}, gm[3] = {g[0], g[1], g[2]};
    gp[a] += 1;
    gm[a] -= 1;
    const int ip = voxel_index(vol, gp[0], gp[1], gp[2]), im = voxel_index(vol, gm[0], gm[1], gm[2]);
    const float fp = (ip >= 0 && vol.weight[ip] > 0.f) ? vol.tsdf[ip] : f;
    const float fm = (im >= 0 && vol.weight[im] > 0.f) ? vol.tsdf[im] : f;
    out[a] = fp - fm;
  }
}
__device__ __forceinline__ void block_origin(const gsr_tsdf_volume &vol, int b, int v, int g[3]) {
  g[0] = (b % vol.blocks[0]) * 8 + (v & 7);
  g[1] = ((b / vol.blocks[0]) % vol.blocks[1]) * 8 + ((v >> 3) & 7);
  g[2] = (b / (vol.blocks[0] * vol.blocks[1])) * 8 + (v >> 6);
}

using BlockScan = rocprim::block_scan<int, VOX>;

__global__ void tsdf_store_total_kernel(const int32_t *incl, int nb, int32_t *dst) { *dst = incl[nb - 1]; }

// ---- points ----------------------------------------------------------------------------------------------------------
// bit a: the edge to the +a neighbour carries a point
__device__ __forceinline__ int point_mask(const gsr_tsdf_volume &vol, const int g[3], float &f0) {
  int idx;
  if (!fetch(vol, g[0], g[1], g[2], f0, idx)) return 0;
  int mask = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int h[3] = {g[0], g[1], g[2]};
    h[a] += 1;
    float f1;
    if (fetch(vol, h[0], h[1], h[2], f1, idx) && f0 * f1 < 0.f) mask |= 1 << a;
  }
  return mask;
}

template <bool EMIT>
__global__ __launch_bounds__(VOX) void tsdf_points_kernel(const gsr_tsdf_volume vol, const int nb,
                                                          int32_t *__restrict__ cnt, const int32_t *__restrict__ incl,
                                                          const int num_points, float *__restrict__ points,
                                                          float *__restrict__ colors, float *__restrict__ normals,
                                                          int32_t *__restrict__ axis) {
  __shared__ BlockScan::storage_type storage;
  const int v = threadIdx.x;
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    if (vol.table[b] < 0) {
      if (!EMIT && v == 0) cnt[b] = 0;
      continue;
    }
    if (EMIT && cnt[b] == 0) continue;
    int g[3];
    block_origin(vol, b, v, g);
    float f0;
    const int mask = point_mask(vol, g, f0);
    int off, total;
    __syncthreads();  // the storage of the previous block's scan
    BlockScan().exclusive_scan(__popc(mask), off, 0, total, storage);
    if (!EMIT) {
      if (v == 0) cnt[b] = total;
      continue;
    }
    if (mask == 0) continue;
    int row = incl[b] - cnt[b] + off;
    const int i0 = voxel_index(vol, g[0], g[1], g[2]);
    float g0[3];
    gradient(vol, g, f0, g0);
    const float r0 = fabsf(f0);
    for (int a = 0; a < 3; ++a) {
      if (!(mask >> a & 1)) continue;
      if (row >= num_points) break;  // (a count read back before the volume changed)
      int h[3] = {g[0], g[1], g[2]};
      h[a] += 1;
      const int i1 = voxel_index(vol, h[0], h[1], h[2]);
      const float f1 = vol.tsdf[i1];
      const float r1 = fabsf(f1), den = r0 + r1;
      float g1[3];
      gradient(vol, h, f1, g1);
      float p[3] = {centre(vol, 0, g[0]), centre(vol, 1, g[1]), centre(vol, 2, g[2])};
      p[a] = (centre(vol, a, g[a]) * r1 + centre(vol, a, h[a]) * r0) / den;
      float n[3];
      for (int k = 0; k < 3; ++k) {
        points[3 * (size_t)row + k] = p[k];
        colors[3 * (size_t)row + k] = (vol.color[3 * (size_t)i0 + k] * r1 + vol.color[3 * (size_t)i1 + k] * r0) / den;
        n[k] = (g0[k] * r1 + g1[k] * r0) / den;
      }
      const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
      for (int k = 0; k < 3; ++k) normals[3 * (size_t)row + k] = len > 0.f ? n[k] / len : 0.f;
      axis[row] = a;
      ++row;
    }
  }
}

// ---- mesh (surface nets) ---------------------------------------------------------------------------------------------
// corner k of the cell at g: offsets (k & 1, k >> 1 & 1, k >> 2)
__device__ __forceinline__ bool cell_corners(const gsr_tsdf_volume &vol, const int g[3], float f[8], int idx[8]) {
  bool all_q = true, any_n = false, all_n = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    all_q &= fetch(vol, g[0] + (k & 1), g[1] + (k >> 1 & 1), g[2] + (k >> 2), f[k], idx[k]);
    any_n |= f[k] < 0.f;
    all_n &= f[k] < 0.f;
  }
  return all_q && any_n && !all_n;
}

// pass 1: which cells carry a vertex (vidx = 0 / -1) and how many per block
__global__ __launch_bounds__(VOX) void tsdf_cells_kernel(const gsr_tsdf_volume vol, const int nb,
                                                         int32_t *__restrict__ vidx, int32_t *__restrict__ vcnt) {
  __shared__ BlockScan::storage_type storage;
  const int v = threadIdx.x;
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    const int slot = vol.table[b];
    if (slot < 0) {
      if (v == 0) vcnt[b] = 0;
      continue;
    }
    int g[3];
    block_origin(vol, b, v, g);
    float f[8];
    int idx[8];
    const bool active = cell_corners(vol, g, f, idx);
    vidx[(size_t)slot * VOX + v] = active ? 0 : -1;
    int off, total;
    __syncthreads();
    BlockScan().exclusive_scan(active ? 1 : 0, off, 0, total, storage);
    if (v == 0) vcnt[b] = total;
  }
}

__device__ __forceinline__ int cell_vertex(const gsr_tsdf_volume &vol, const int32_t *vidx, int gx, int gy, int gz) {
  const int i = voxel_index(vol, gx, gy, gz);
  return i < 0 ? -1 : vidx[i];
}

// the quad of the grid edge g -> g + e_a: q[0..3] = vertex numbers (or activity marks) of the cells at
// g - e_b - e_c, g - e_c, g, g - e_b with (a, b, c) cyclic; false if one of them carries no vertex
__device__ __forceinline__ bool edge_quad(const gsr_tsdf_volume &vol, const int32_t *vidx, const int g[3], int a,
                                          int q[4]) {
  const int b = (a + 1) % 3, c = (a + 2) % 3;
  if (g[b] < 1 || g[c] < 1) return false;
  int h[3] = {g[0], g[1], g[2]};
  q[2] = cell_vertex(vol, vidx, h[0], h[1], h[2]);
  h[b] -= 1;
  q[3] = cell_vertex(vol, vidx, h[0], h[1], h[2]);
  h[c] -= 1;
  q[0] = cell_vertex(vol, vidx, h[0], h[1], h[2]);
  h[b] += 1;
  q[1] = cell_vertex(vol, vidx, h[0], h[1], h[2]);
  return q[0] >= 0 && q[1] >= 0 && q[2] >= 0 && q[3] >= 0;
}

// bit a: the edge to the +a neighbour changes sign and its four cells carry vertices
__device__ __forceinline__ int face_mask(const gsr_tsdf_volume &vol, const int32_t *vidx, const int g[3], bool &neg0) {
  const int i0 = voxel_index(vol, g[0], g[1], g[2]);
  neg0 = vol.tsdf[i0] < 0.f;
  int mask = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    int q[4];
    if (!edge_quad(vol, vidx, g, a, q)) continue;
    int h[3] = {g[0], g[1], g[2]};
    h[a] += 1;
    const int i1 = voxel_index(vol, h[0], h[1], h[2]);  // a corner of an active cell: stored
    if ((vol.tsdf[i1] < 0.f) != neg0) mask |= 1 << a;
  }
  return mask;
}

// pass 2 (EMIT = false): triangles per block; pass 4 (EMIT = true): the triangles
template <bool EMIT>
__global__ __launch_bounds__(VOX) void tsdf_faces_kernel(const gsr_tsdf_volume vol, const int nb,
                                                         const int32_t *__restrict__ vidx, int32_t *__restrict__ fcnt,
                                                         const int32_t *__restrict__ fincl, const int num_triangles,
                                                         int32_t *__restrict__ triangles) {
  __shared__ BlockScan::storage_type storage;
  const int v = threadIdx.x;
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    if (vol.table[b] < 0) {
      if (!EMIT && v == 0) fcnt[b] = 0;
      continue;
    }
    if (EMIT && fcnt[b] == 0) continue;
    int g[3];
    block_origin(vol, b, v, g);
    bool neg0;
    const int mask = face_mask(vol, vidx, g, neg0);
    int off, total;
    __syncthreads();
    BlockScan().exclusive_scan(2 * __popc(mask), off, 0, total, storage);
    if (!EMIT) {
      if (v == 0) fcnt[b] = total;
      continue;
    }
    int row = fincl[b] - fcnt[b] + off;
    for (int a = 0; a < 3; ++a) {
      if (!(mask >> a & 1)) continue;
      if (row + 2 > num_triangles) break;
      int q[4];
      edge_quad(vol, vidx, g, a, q);
      int32_t *t = triangles + 3 * (size_t)row;
      // normals towards positive tsdf: +a when the lower voxel is the negative one
      t[0] = q[0], t[1] = neg0 ? q[1] : q[2], t[2] = neg0 ? q[2] : q[1];
      t[3] = q[0], t[4] = neg0 ? q[2] : q[3], t[5] = neg0 ? q[3] : q[2];
      row += 2;
    }
  }
}

// pass 3: vertex numbers (into vidx), positions and colours
__global__ __launch_bounds__(VOX) void tsdf_vertices_kernel(const gsr_tsdf_volume vol, const int nb,
                                                            int32_t *__restrict__ vidx,
                                                            const int32_t *__restrict__ vcnt,
                                                            const int32_t *__restrict__ vincl, const int num_vertices,
                                                            float *__restrict__ vertices,
                                                            float *__restrict__ vertex_colors) {
  __shared__ BlockScan::storage_type storage;
  const int v = threadIdx.x;
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    const int slot = vol.table[b];
    if (slot < 0 || vcnt[b] == 0) continue;
    const size_t own = (size_t)slot * VOX + v;
    const bool active = vidx[own] >= 0;
    int off, total;
    __syncthreads();
    BlockScan().exclusive_scan(active ? 1 : 0, off, 0, total, storage);
    if (!active) continue;
    const int row = vincl[b] - vcnt[b] + off;
    vidx[own] = row;
    if (row >= num_vertices) continue;
    int g[3];
    block_origin(vol, b, v, g);
    float f[8];
    int idx[8];
    cell_corners(vol, g, f, idx);
    float ps[3] = {0.f, 0.f, 0.f}, cs[3] = {0.f, 0.f, 0.f}, n = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int eb = (a + 1) % 3, ec = (a + 2) % 3;
#pragma unroll
      for (int dc = 0; dc < 2; ++dc)
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const int k0 = (db << eb) | (dc << ec), k1 = k0 | (1 << a);
          if ((f[k0] < 0.f) == (f[k1] < 0.f)) continue;
          const float r0 = fabsf(f[k0]), r1 = fabsf(f[k1]), den = r0 + r1;
          int h[3] = {g[0] + (k0 & 1), g[1] + (k0 >> 1 & 1), g[2] + (k0 >> 2)};
          float p[3] = {centre(vol, 0, h[0]), centre(vol, 1, h[1]), centre(vol, 2, h[2])};
          p[a] = (centre(vol, a, h[a]) * r1 + centre(vol, a, h[a] + 1) * r0) / den;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            ps[k] += p[k];
            cs[k] += (vol.color[3 * (size_t)idx[k0] + k] * r1 + vol.color[3 * (size_t)idx[k1] + k] * r0) / den;
          }
          n += 1.f;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      vertices[3 * (size_t)row + k] = ps[k] / n;
      vertex_colors[3 * (size_t)row + k] = cs[k] / n;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

int check_volume(const gsr_tsdf_volume *vol, const char *who) {
  GSR_REQUIRE(vol != nullptr, "%s: null volume", who);
  GSR_REQUIRE(vol->blocks[0] > 0 && vol->blocks[1] > 0 && vol->blocks[2] > 0, "%s: blocks must be positive", who);
  GSR_REQUIRE((long long)vol->blocks[0] * vol->blocks[1] * vol->blocks[2] <= MAX_BLOCKS &&
                  vol->blocks[0] <= MAX_BLOCKS && vol->blocks[1] <= MAX_BLOCKS && vol->blocks[2] <= MAX_BLOCKS &&
                  (long long)vol->blocks[0] * vol->blocks[1] <= MAX_BLOCKS,
              "%s: more than %d blocks", who, MAX_BLOCKS);
  GSR_REQUIRE(vol->voxel_length > 0.f, "%s: voxel length must be positive", who);
  GSR_REQUIRE(vol->sdf_trunc > 0.f, "%s: sdf_trunc must be positive", who);
  GSR_REQUIRE(vol->capacity > 0 && vol->capacity <= MAX_CAPACITY, "%s: capacity must be in [1, %d]", who, MAX_CAPACITY);
  GSR_REQUIRE(vol->table && vol->tsdf && vol->weight && vol->color && vol->state, "%s: null volume buffer", who);
  return GSR_OK;
}

int check_view(const gsr_tsdf_view *vw, const char *who) {
  GSR_REQUIRE(vw != nullptr, "%s: null view", who);
  GSR_REQUIRE(vw->height > 0 && vw->width > 0, "%s: empty image", who);
  GSR_REQUIRE((unsigned long long)vw->height * vw->width < (1ull << 31), "%s: image too large", who);
  GSR_REQUIRE(vw->fx > 0.f && vw->fy > 0.f, "%s: focal lengths must be positive", who);
  GSR_REQUIRE(vw->depth_trunc > 0.f, "%s: depth_trunc must be positive", who);
  GSR_REQUIRE(vw->depth && vw->color, "%s: null image", who);
  return GSR_OK;
}

inline int num_blocks(const gsr_tsdf_volume *vol) { return vol->blocks[0] * vol->blocks[1] * vol->blocks[2]; }

size_t int_scan_temp(int n) {
  size_t bytes = 0;
  (void)rocprim::inclusive_scan(nullptr, bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)n,
                                rocprim::plus<int32_t>());
  return bytes;
}

size_t alloc_scan_temp(int n) {
  size_t bytes = 0;
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), AllocInput{nullptr, nullptr});
  (void)rocprim::exclusive_scan(nullptr, bytes, in, (unsigned long long *)nullptr, 0ull, (size_t)n,
                                rocprim::plus<unsigned long long>());
  return bytes;
}

int check_workspace(const void *ws, size_t have, size_t need, const char *who) {
  if (have < need || !ws) {
    gsr_set_error("%s: workspace %zu < %zu bytes", who, have, need);
    return GSR_ENOMEM;
  }
  GSR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT int gsr_tsdf_touch(const gsr_tsdf_volume *vol, const gsr_tsdf_view *view, uint8_t *flags,
                              gsr_stream_t stream) {
  if (int rc = check_volume(vol, "tsdf_touch")) return rc;
  if (int rc = check_view(view, "tsdf_touch")) return rc;
  GSR_REQUIRE(flags != nullptr, "tsdf_touch: null flags");
  hipLaunchKernelGGL(tsdf_touch_kernel, dim3(gsr_cdiv(view->height * view->width, 256)), dim3(256), 0,
                     (hipStream_t)stream, *vol, *view, flags);
  GSR_CHECK_LAUNCH("tsdf_touch");
  return GSR_OK;
}

GSR_EXPORT size_t gsr_tsdf_allocate_workspace_bytes(int nb) {
  if (nb <= 0 || nb > MAX_BLOCKS) return 0;
  return align_up((size_t)nb * sizeof(unsigned long long)) + align_up(alloc_scan_temp(nb));
}

GSR_EXPORT int gsr_tsdf_allocate(const gsr_tsdf_volume *vol, uint8_t *flags, int32_t *list, void *workspace,
                                 size_t workspace_bytes, gsr_stream_t stream) {
  if (int rc = check_volume(vol, "tsdf_allocate")) return rc;
  GSR_REQUIRE(flags && list, "tsdf_allocate: null pointer");
  const int nb = num_blocks(vol);
  if (int rc = check_workspace(workspace, workspace_bytes, gsr_tsdf_allocate_workspace_bytes(nb), "tsdf_allocate"))
    return rc;
  auto *scan = static_cast<unsigned long long *>(workspace);
  const size_t head = align_up((size_t)nb * sizeof(unsigned long long));
  auto in = rocprim::make_transform_iterator(rocprim::counting_iterator<int>(0), AllocInput{flags, vol->table});
  size_t temp_bytes = workspace_bytes - head;
  GSR_CHECK_HIP(rocprim::exclusive_scan(static_cast<char *>(workspace) + head, temp_bytes, in, scan, 0ull,
                                        (size_t)nb, rocprim::plus<unsigned long long>(), (hipStream_t)stream));
  hipLaunchKernelGGL(tsdf_alloc_apply_kernel, dim3(gsr_cdiv(nb, 256)), dim3(256), 0, (hipStream_t)stream, *vol, flags,
                     list, scan, nb);
  GSR_CHECK_LAUNCH("tsdf_alloc_apply");
  hipLaunchKernelGGL(tsdf_alloc_commit_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, vol->state);
  GSR_CHECK_LAUNCH("tsdf_alloc_commit");
  return GSR_OK;
}

GSR_EXPORT int gsr_tsdf_integrate(const gsr_tsdf_volume *vol, const gsr_tsdf_view *view, const int32_t *list,
                                  gsr_stream_t stream) {
  if (int rc = check_volume(vol, "tsdf_integrate")) return rc;
  if (int rc = check_view(view, "tsdf_integrate")) return rc;
  GSR_REQUIRE(list != nullptr, "tsdf_integrate: null list");
  const int nb = num_blocks(vol);
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(nb < GRID ? nb : GRID), dim3(VOX), 0, (hipStream_t)stream, *vol, *view,
                     list);
  GSR_CHECK_LAUNCH("tsdf_integrate");
  return GSR_OK;
}

GSR_EXPORT size_t gsr_tsdf_extract_points_workspace_bytes(int nb) {
  if (nb <= 0 || nb > MAX_BLOCKS) return 0;
  return 2 * align_up((size_t)nb * 4) + align_up(int_scan_temp(nb));
}

GSR_EXPORT int gsr_tsdf_extract_points_count(const gsr_tsdf_volume *vol, void *workspace, size_t workspace_bytes,
                                             gsr_stream_t stream) {
  if (int rc = check_volume(vol, "tsdf_extract_points_count")) return rc;
  const int nb = num_blocks(vol);
  if (int rc = check_workspace(workspace, workspace_bytes, gsr_tsdf_extract_points_workspace_bytes(nb),
                               "tsdf_extract_points_count"))
    return rc;
  const size_t seg = align_up((size_t)nb * 4);
  char *ws = static_cast<char *>(workspace);
  auto *cnt = reinterpret_cast<int32_t *>(ws), *incl = reinterpret_cast<int32_t *>(ws + seg);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tsdf_points_kernel<false>, dim3(nb < GRID ? nb : GRID), dim3(VOX), 0, s, *vol, nb, cnt,
                     (const int32_t *)nullptr, 0, (float *)nullptr, (float *)nullptr, (float *)nullptr,
                     (int32_t *)nullptr);
  GSR_CHECK_LAUNCH("tsdf_points_count");
  size_t temp_bytes = workspace_bytes - 2 * seg;
  GSR_CHECK_HIP(rocprim::inclusive_scan(ws + 2 * seg, temp_bytes, cnt, incl, (size_t)nb,
                                        rocprim::plus<int32_t>(), s));
  hipLaunchKernelGGL(tsdf_store_total_kernel, dim3(1), dim3(1), 0, s, incl, nb, vol->state + ST_POINTS);
  GSR_CHECK_LAUNCH("tsdf_store_total");
  return GSR_OK;
}

GSR_EXPORT int gsr_tsdf_extract_points_emit(const gsr_tsdf_volume *vol, const void *workspace, size_t workspace_bytes,
                                            int num_points, float *points, float *colors, float *normals,
                                            int32_t *axis, gsr_stream_t stream) {
  if (int rc = check_volume(vol, "tsdf_extract_points_emit")) return rc;
  GSR_REQUIRE(num_points >= 0, "tsdf_extract_points_emit: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(points && colors && normals && axis, "tsdf_extract_points_emit: null output");
  const int nb = num_blocks(vol);
  if (int rc = check_workspace(workspace, workspace_bytes, gsr_tsdf_extract_points_workspace_bytes(nb),
                               "tsdf_extract_points_emit"))
    return rc;
  const size_t seg = align_up((size_t)nb * 4);
  char *ws = static_cast<char *>(const_cast<void *>(workspace));
  hipLaunchKernelGGL(tsdf_points_kernel<true>, dim3(nb < GRID ? nb : GRID), dim3(VOX), 0, (hipStream_t)stream, *vol, nb,
                     reinterpret_cast<int32_t *>(ws), reinterpret_cast<const int32_t *>(ws + seg), num_points, points,
                     colors, normals, axis);
  GSR_CHECK_LAUNCH("tsdf_points_emit");
  return GSR_OK;
}

namespace {
struct MeshWorkspace {
  int32_t *vidx, *vcnt, *fcnt, *vincl, *fincl;
  char *temp;
  size_t temp_bytes;
};
size_t mesh_workspace(int nb, int capacity, void *workspace, size_t workspace_bytes, MeshWorkspace *out) {
  const size_t seg = align_up((size_t)nb * 4), head = align_up((size_t)capacity * VOX * 4);
  const size_t need = head + 4 * seg + align_up(int_scan_temp(nb));
  if (out) {
    char *ws = static_cast<char *>(workspace);
    out->vidx = reinterpret_cast<int32_t *>(ws);
    out->vcnt = reinterpret_cast<int32_t *>(ws + head);
    out->fcnt = reinterpret_cast<int32_t *>(ws + head + seg);
    out->vincl = reinterpret_cast<int32_t *>(ws + head + 2 * seg);
    out->fincl = reinterpret_cast<int32_t *>(ws + head + 3 * seg);
    out->temp = ws + head + 4 * seg;
    out->temp_bytes = workspace_bytes - (head + 4 * seg);
  }
  return need;
}
}  // namespace

GSR_EXPORT size_t gsr_tsdf_extract_mesh_workspace_bytes(int nb, int capacity) {
  if (nb <= 0 || nb > MAX_BLOCKS || capacity <= 0 || capacity > MAX_CAPACITY) return 0;
  return mesh_workspace(nb, capacity, nullptr, 0, nullptr);
}

GSR_EXPORT int gsr_tsdf_extract_mesh_count(const gsr_tsdf_volume *vol, void *workspace, size_t workspace_bytes,
                                           gsr_stream_t stream) {
  if (int rc = check_volume(vol, "tsdf_extract_mesh_count")) return rc;
  const int nb = num_blocks(vol);
  if (int rc = check_workspace(workspace, workspace_bytes, gsr_tsdf_extract_mesh_workspace_bytes(nb, vol->capacity),
                               "tsdf_extract_mesh_count"))
    return rc;
  MeshWorkspace w;
  mesh_workspace(nb, vol->capacity, workspace, workspace_bytes, &w);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(nb < GRID ? nb : GRID);
  hipLaunchKernelGGL(tsdf_cells_kernel, grid, dim3(VOX), 0, s, *vol, nb, w.vidx, w.vcnt);
  GSR_CHECK_LAUNCH("tsdf_cells");
  hipLaunchKernelGGL(tsdf_faces_kernel<false>, grid, dim3(VOX), 0, s, *vol, nb, (const int32_t *)w.vidx, w.fcnt,
                     (const int32_t *)nullptr, 0, (int32_t *)nullptr);
  GSR_CHECK_LAUNCH("tsdf_faces_count");
  GSR_CHECK_HIP(rocprim::inclusive_scan(w.temp, w.temp_bytes, w.vcnt, w.vincl, (size_t)nb, rocprim::plus<int32_t>(), s));
  GSR_CHECK_HIP(rocprim::inclusive_scan(w.temp, w.temp_bytes, w.fcnt, w.fincl, (size_t)nb, rocprim::plus<int32_t>(), s));
  hipLaunchKernelGGL(tsdf_store_total_kernel, dim3(1), dim3(1), 0, s, (const int32_t *)w.vincl, nb,
                     vol->state + ST_VERTICES);
  hipLaunchKernelGGL(tsdf_store_total_kernel, dim3(1), dim3(1), 0, s, (const int32_t *)w.fincl, nb,
                     vol->state + ST_TRIANGLES);
  GSR_CHECK_LAUNCH("tsdf_store_total");
  return GSR_OK;
}

GSR_EXPORT int gsr_tsdf_extract_mesh_emit(const gsr_tsdf_volume *vol, void *workspace, size_t workspace_bytes,
                                          int num_vertices, int num_triangles, float *vertices, float *vertex_colors,
                                          int32_t *triangles, gsr_stream_t stream) {
  if (int rc = check_volume(vol, "tsdf_extract_mesh_emit")) return rc;
  GSR_REQUIRE(num_vertices >= 0 && num_triangles >= 0, "tsdf_extract_mesh_emit: negative count");
  if (num_vertices == 0) return GSR_OK;
  GSR_REQUIRE(vertices && vertex_colors && (triangles || num_triangles == 0), "tsdf_extract_mesh_emit: null output");
  const int nb = num_blocks(vol);
  if (int rc = check_workspace(workspace, workspace_bytes, gsr_tsdf_extract_mesh_workspace_bytes(nb, vol->capacity),
                               "tsdf_extract_mesh_emit"))
    return rc;
  MeshWorkspace w;
  mesh_workspace(nb, vol->capacity, workspace, workspace_bytes, &w);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(nb < GRID ? nb : GRID);
  hipLaunchKernelGGL(tsdf_vertices_kernel, grid, dim3(VOX), 0, s, *vol, nb, w.vidx, (const int32_t *)w.vcnt,
                     (const int32_t *)w.vincl, num_vertices, vertices, vertex_colors);
  GSR_CHECK_LAUNCH("tsdf_vertices");
  if (num_triangles > 0) {
    hipLaunchKernelGGL(tsdf_faces_kernel<true>, grid, dim3(VOX), 0, s, *vol, nb, (const int32_t *)w.vidx, w.fcnt,
                       (const int32_t *)w.fincl, num_triangles, triangles);
    GSR_CHECK_LAUNCH("tsdf_faces_emit");
  }
  return GSR_OK;
}
