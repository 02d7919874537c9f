// mesh_clean.hip -- cleaning of a triangle mesh on the GPU: null faces, duplicate faces, connected components of
// fewer than `min_component_faces` faces, unreferenced vertices (the rules are stated in
// include/gsraster.h, the NumPy oracle is tests/mesh_clean_reference.py).
//
// Compiled with -ffp-contract=off (Makefile): the null rule's cross product is evaluated with every operation rounded
// on its own, as the float32 NumPy oracle does.
//
// gsr_mesh_label:  validate -> [host reads one word] -> null -> sort by the largest index -> sort (stable) by the two
//   smaller ones -> duplicate flags -> half-edge records -> sort -> union-find over the runs of equal edges -> labels
//   -> sizes (histogram into the root's slot) -> verify -> keep flags, vertex marks -> two scans -> counts in `state`.
// gsr_mesh_emit:   triangles (remapped) and vertex / attribute rows (copied as 32-bit words).
//
// Grids: EVERY kernel here is one thread per element with a grid sized by its element count (F faces, 3F half-edge
// records or V vertices; at most 3 * 2^28 / 256 workgroups); none loops with a grid stride.  The only loops are the
// root chase of the union-find and the per-wave merge of the histogram.
//
// Determinism: a face's label is the smallest face index of its component -- the union-find only ever lowers
// parent[x] (atomicMin, parent[x] <= x), so whatever the order in which the atomics land, the root of a tree is its
// smallest member.  Sizes are integer sums.  Counts and compaction come from scans.  Flags that several threads set
// are stores of one value.
#include <climits>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "gsr_common.h"

namespace {

constexpr int MAX_FACES = 1 << 28;  // 3 F half-edge records index with an int
constexpr int MAX_VERTICES = INT_MAX - 1;
constexpr int TPB = 256;
constexpr uint32_t NO_KEY32 = 0xffffffffu;

enum { ST_BAD = 0, ST_NULL = 1, ST_DUP = 2, ST_COMPONENTS = 3, ST_COMPONENTS_KEPT = 4, ST_FACES_KEPT = 5,
       ST_VERTICES_KEPT = 6, ST_UNCONVERGED = 7 };
enum : uint8_t { FACE_ALIVE = 0, FACE_NULL = 1, FACE_DUP = 2 };

// bits of a vertex index; a pair of indices packs into 2 * vb bits, and 1 << 2 * vb sorts behind every pair
inline int vertex_bits(int V) {
  int b = 1;
  while (b < 31 && (1ll << b) < (long long)V) ++b;
  return b;
}

__device__ __forceinline__ void sort3(int &a, int &b, int &c) {
  int t;
  if (a > b) t = a, a = b, b = t;
  if (b > c) t = b, b = c, c = t;
  if (a > b) t = a, a = b, b = t;
}
__device__ __forceinline__ uint64_t pair_key(int lo, int hi, int vb) { return ((uint64_t)lo << vb) | (uint64_t)hi; }

// adds `n` (summed over the workgroup) to *dst with one atomic per workgroup that has anything to add
__device__ __forceinline__ void block_add(int n, int32_t *dst) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  const int wave = __popcll(__ballot(n != 0));  // (n is 0 or 1 everywhere in this file)
  if (wave && (threadIdx.x & (GSR_WAVE - 1)) == 0) atomicAdd(&total, wave);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(dst, total);
}

// ---- validate: reads `triangles` only --------------------------------------------------------------------------------
__global__ void mesh_state_init_kernel(int32_t *state) {
  state[threadIdx.x] = threadIdx.x == ST_BAD ? INT_MAX : 0;
}

__global__ __launch_bounds__(TPB) void mesh_validate_kernel(const int F, const int V, const int32_t *__restrict__ tri,
                                                            int32_t *__restrict__ state) {
  const int f = blockIdx.x * TPB + threadIdx.x;
  if (f >= F) return;
  const int a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V)
    atomicMin(&state[ST_BAD], f);  // (the lowest offender: the message does not depend on who came first)
}

// ---- null faces; keys of the first duplicate sort --------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void mesh_null_kernel(const int F, const float *__restrict__ vtx,
                                                        const int32_t *__restrict__ tri, uint8_t *__restrict__ fflag,
                                                        uint32_t *__restrict__ key, int32_t *__restrict__ val,
                                                        int32_t *__restrict__ state) {
  const int f = blockIdx.x * TPB + threadIdx.x;
  bool null = false;
  if (f < F) {
    int a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
    null = a == b || b == c || a == c;
    if (!null && vtx != nullptr) {
      const float *p0 = vtx + 3 * (size_t)a, *p1 = vtx + 3 * (size_t)b, *p2 = vtx + 3 * (size_t)c;
      const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
      const float wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
      const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
      null = nx == 0.f && ny == 0.f && nz == 0.f;  // (a NaN compares unequal: not null)
    }
    sort3(a, b, c);
    fflag[f] = null ? FACE_NULL : FACE_ALIVE;
    key[f] = null ? NO_KEY32 : (uint32_t)c;
    val[f] = f;
  }
  block_add(null ? 1 : 0, state + ST_NULL);
}

// keys of the second (stable) duplicate sort: the two smaller indices of the faces in the order of the first
__global__ __launch_bounds__(TPB) void mesh_dupkey_kernel(const int F, const int vb, const int32_t *__restrict__ tri,
                                                          const uint8_t *__restrict__ fflag,
                                                          const int32_t *__restrict__ order,
                                                          uint64_t *__restrict__ key) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= F) return;
  const int f = order[i];
  int a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
  sort3(a, b, c);
  key[i] = fflag[f] != FACE_ALIVE ? (1ull << (2 * vb)) : pair_key(a, b, vb);
}

// faces are now ordered by (sorted triple, face index): every member of a run of equal triples but its first is a
// duplicate.  Null faces (recognised by their key, which no thread writes here) lie behind all others.
__global__ __launch_bounds__(TPB) void mesh_dupflag_kernel(const int F, const int vb, const int32_t *__restrict__ tri,
                                                           const uint64_t *__restrict__ key,
                                                           const int32_t *__restrict__ order,
                                                           uint8_t *__restrict__ fflag, int32_t *__restrict__ state) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  bool dup = false;
  if (i >= 1 && i < F && key[i] != (1ull << (2 * vb)) && key[i] == key[i - 1]) {
    const int f = order[i], g = order[i - 1];
    const int cf = max(max(tri[3 * (size_t)f], tri[3 * (size_t)f + 1]), tri[3 * (size_t)f + 2]);
    const int cg = max(max(tri[3 * (size_t)g], tri[3 * (size_t)g + 1]), tri[3 * (size_t)g + 2]);
    dup = cf == cg;
    if (dup) fflag[f] = FACE_DUP;
  }
  block_add(dup ? 1 : 0, state + ST_DUP);
}

// ---- half-edge records -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void mesh_edges_kernel(const int F, const int vb, const int32_t *__restrict__ tri,
                                                         const uint8_t *__restrict__ fflag,
                                                         uint64_t *__restrict__ key, int32_t *__restrict__ val,
                                                         int32_t *__restrict__ parent, int32_t *__restrict__ count) {
  const int f = blockIdx.x * TPB + threadIdx.x;
  if (f >= F) return;
  const int a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
  const bool alive = fflag[f] == FACE_ALIVE;
  const uint64_t none = 1ull << (2 * vb);
  key[3 * (size_t)f + 0] = alive ? pair_key(min(a, b), max(a, b), vb) : none;
  key[3 * (size_t)f + 1] = alive ? pair_key(min(b, c), max(b, c), vb) : none;
  key[3 * (size_t)f + 2] = alive ? pair_key(min(c, a), max(c, a), vb) : none;
  val[3 * (size_t)f + 0] = val[3 * (size_t)f + 1] = val[3 * (size_t)f + 2] = f;
  parent[f] = f;
  count[f] = 0;
}

// ---- union-find over faces -------------------------------------------------------------------------------------------
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
// loop ends.  Only roots are written to: the traffic spreads over the roots, not one word.
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

__global__ __launch_bounds__(TPB) void mesh_union_kernel(const int E, const uint64_t none,
                                                         const uint64_t *__restrict__ key,
                                                         const int32_t *__restrict__ face,
                                                         int32_t *__restrict__ parent) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i < 1 || i >= E) return;
  const uint64_t k = key[i];
  if (k == none || k != key[i - 1]) return;
  unite(parent, face[i - 1], face[i]);  // a run of n records links its n faces in a chain
}

// (a launch of its own: parent[] is final and only read) label = root; size: histogram into the root's slot, the
// lanes of a wave that share a root merged into one atomic
__global__ __launch_bounds__(TPB) void mesh_label_kernel(const int F, const int32_t *__restrict__ parent,
                                                         const uint8_t *__restrict__ fflag,
                                                         int32_t *__restrict__ label, int32_t *__restrict__ count) {
  const int f = blockIdx.x * TPB + threadIdx.x;
  const bool alive = f < F && fflag[f] == FACE_ALIVE;
  int r = -1;
  if (alive) {
    r = f;
    for (int p = parent[r]; p != r; p = parent[r]) r = p;
  }
  if (f < F) label[f] = r;
  const int lane = threadIdx.x & (GSR_WAVE - 1);
  unsigned long long todo = __ballot(alive);
  while (todo) {  // (wave-uniform)
    const int leader = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(r, leader);
    const unsigned long long same = __ballot(alive && r == r0);
    if (lane == leader) atomicAdd(count + r0, __popcll(same));
    todo &= ~same;
  }
}

// every pair of linked faces carries one label, or state[ST_UNCONVERGED] is set (stores of one value)
__global__ __launch_bounds__(TPB) void mesh_verify_kernel(const int E, const uint64_t none,
                                                          const uint64_t *__restrict__ key,
                                                          const int32_t *__restrict__ face,
                                                          const int32_t *__restrict__ label,
                                                          int32_t *__restrict__ state) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i < 1 || i >= E) return;
  const uint64_t k = key[i];
  if (k == none || k != key[i - 1]) return;
  if (label[face[i]] != label[face[i - 1]]) state[ST_UNCONVERGED] = 1;
}

// sizes, keep flags, component counts, marks of the vertices that kept faces reference
__global__ __launch_bounds__(TPB) void mesh_keep_kernel(const int F, const int min_faces,
                                                        const int32_t *__restrict__ tri,
                                                        const int32_t *__restrict__ label,
                                                        const int32_t *__restrict__ count, int32_t *__restrict__ size,
                                                        int32_t *__restrict__ keep, uint8_t *__restrict__ vmark,
                                                        int32_t *__restrict__ state) {
  const int f = blockIdx.x * TPB + threadIdx.x;
  int root = 0, root_kept = 0;
  if (f < F) {
    const int r = label[f];
    const int n = r < 0 ? 0 : count[r];
    const bool kept = r >= 0 && n >= min_faces;
    size[f] = n;
    keep[f] = kept ? 1 : 0;
    if (kept)
      for (int k = 0; k < 3; ++k) {
        uint8_t *m = vmark + tri[3 * (size_t)f + k];
        if (*m == 0) *m = 1;  // every writer stores the same value (the read only spares stores)
      }
    root = r == f;
    root_kept = root && kept;
  }
  block_add(root, state + ST_COMPONENTS);
  block_add(root_kept, state + ST_COMPONENTS_KEPT);
}

struct MarkToInt {
  __device__ int32_t operator()(uint8_t m) const { return m != 0; }
};

__global__ void mesh_store_totals_kernel(const int32_t *fincl, int F, const int32_t *vincl, int V, int32_t *state) {
  state[ST_FACES_KEPT] = fincl[F - 1];
  state[ST_VERTICES_KEPT] = V > 0 ? vincl[V - 1] : 0;
}

__global__ __launch_bounds__(TPB) void mesh_copy_kernel(const int n, const int32_t *__restrict__ a,
                                                        int32_t *__restrict__ a_out, const int32_t *__restrict__ b,
                                                        int32_t *__restrict__ b_out) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  if (a_out) a_out[i] = a[i];
  if (b_out) b_out[i] = b[i];
}

// ---- emit ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void mesh_emit_faces_kernel(const int F, const int32_t *__restrict__ tri,
                                                              const int32_t *__restrict__ keep,
                                                              const int32_t *__restrict__ fincl,
                                                              const int32_t *__restrict__ vincl, const int out_F,
                                                              int32_t *__restrict__ out) {
  const int f = blockIdx.x * TPB + threadIdx.x;
  if (f >= F || !keep[f]) return;
  const int row = fincl[f] - 1;
  if (row >= out_F) return;  // (a count read back before the workspace changed)
  for (int k = 0; k < 3; ++k) out[3 * (size_t)row + k] = vincl[tri[3 * (size_t)f + k]] - 1;
}

__global__ __launch_bounds__(TPB) void mesh_emit_vertices_kernel(const int V, const int C,
                                                                 const uint32_t *__restrict__ vtx,
                                                                 const uint32_t *__restrict__ attr,
                                                                 const uint8_t *__restrict__ vmark,
                                                                 const int32_t *__restrict__ vincl, const int out_V,
                                                                 uint32_t *__restrict__ out_vtx,
                                                                 uint32_t *__restrict__ out_attr) {
  const int v = blockIdx.x * TPB + threadIdx.x;
  if (v >= V || !vmark[v]) return;
  const int row = vincl[v] - 1;
  if (row >= out_V) return;
  for (int k = 0; k < 3; ++k) out_vtx[3 * (size_t)row + k] = vtx[3 * (size_t)v + k];
  for (int k = 0; k < C; ++k) out_attr[(size_t)C * row + k] = attr[(size_t)C * v + k];
}

// ---- host side -------------------------------------------------------------------------------------------------------
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Workspace {
  uint64_t *key_in, *key_out;  // [3F]
  int32_t *val_in, *val_out;   // [3F]
  int32_t *parent, *label, *count, *size, *keep, *fincl;  // [F]
  int32_t *vincl;                                         // [V]
  uint8_t *fflag, *vmark;                                 // [F], [V]
  char *temp;
  size_t temp_bytes;
};

// the largest temporary storage any rocPRIM call of gsr_mesh_label asks for; false when a size query fails
bool temp_bytes_for(int V, int F, size_t *out) {
  const unsigned end_bit = 2 * vertex_bits(V) + 1;
  const uint64_t *k64 = nullptr;
  const uint32_t *k32 = nullptr;
  const int32_t *i32 = nullptr;
  auto marks = rocprim::make_transform_iterator((const uint8_t *)nullptr, MarkToInt());
  size_t b[5] = {0, 0, 0, 0, 0};
  const hipError_t e[5] = {
      rocprim::radix_sort_pairs(nullptr, b[0], k64, (uint64_t *)nullptr, i32, (int32_t *)nullptr, (size_t)3 * F, 0,
                                end_bit),
      rocprim::radix_sort_pairs(nullptr, b[1], k64, (uint64_t *)nullptr, i32, (int32_t *)nullptr, (size_t)F, 0, end_bit),
      rocprim::radix_sort_pairs(nullptr, b[2], k32, (uint32_t *)nullptr, i32, (int32_t *)nullptr, (size_t)F, 0, 32),
      rocprim::inclusive_scan(nullptr, b[3], i32, (int32_t *)nullptr, (size_t)F, rocprim::plus<int32_t>()),
      rocprim::inclusive_scan(nullptr, b[4], marks, (int32_t *)nullptr, (size_t)(V > 0 ? V : 1),
                              rocprim::plus<int32_t>())};
  size_t need = 0;
  for (int k = 0; k < 5; ++k) {
    if (e[k] != hipSuccess) return false;
    need = b[k] > need ? b[k] : need;
  }
  *out = need;
  return true;
}

// lays the arrays out in `workspace` (w != nullptr) -> the bytes they take, temporaries of rocPRIM not included
size_t carve(int V, int F, void *workspace, size_t workspace_bytes, Workspace *w) {
  const size_t e8 = align_up((size_t)3 * F * 8), e4 = align_up((size_t)3 * F * 4), f4 = align_up((size_t)F * 4);
  const size_t v4 = align_up((size_t)V * 4), f1 = align_up((size_t)F), v1 = align_up((size_t)V);
  const size_t head = 2 * e8 + 2 * e4 + 6 * f4 + v4 + f1 + v1;
  if (w) {
    char *p = static_cast<char *>(workspace);
    auto take = [&p](size_t n) { char *q = p; p += n; return q; };
    w->key_in = reinterpret_cast<uint64_t *>(take(e8));
    w->key_out = reinterpret_cast<uint64_t *>(take(e8));
    w->val_in = reinterpret_cast<int32_t *>(take(e4));
    w->val_out = reinterpret_cast<int32_t *>(take(e4));
    int32_t **per_face[6] = {&w->parent, &w->label, &w->count, &w->size, &w->keep, &w->fincl};
    for (auto **q : per_face) *q = reinterpret_cast<int32_t *>(take(f4));
    w->vincl = reinterpret_cast<int32_t *>(take(v4));
    w->fflag = reinterpret_cast<uint8_t *>(take(f1));
    w->vmark = reinterpret_cast<uint8_t *>(take(v1));
    w->temp = p;
    w->temp_bytes = workspace_bytes - head;
  }
  return head;
}

int check_sizes(int V, int F, const char *who) {
  GSR_REQUIRE(V >= 0 && V <= MAX_VERTICES, "%s: num_vertices must be in [0, %d]", who, MAX_VERTICES);
  GSR_REQUIRE(F >= 0 && F <= MAX_FACES, "%s: num_faces must be in [0, %d]", who, MAX_FACES);
  return GSR_OK;
}

int check_workspace(const void *ws, size_t have, size_t need, const char *who) {
  GSR_REQUIRE(need != 0, "%s: the workspace size query failed", who);
  if (have < need || !ws) {
    gsr_set_error("%s: workspace %zu < %zu bytes", who, have, need);
    return GSR_ENOMEM;
  }
  GSR_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "%s: workspace must be 256-byte aligned", who);
  return GSR_OK;
}

}  // namespace

GSR_EXPORT size_t gsr_mesh_clean_workspace_bytes(int num_vertices, int num_faces) {
  if (num_vertices < 0 || num_vertices > MAX_VERTICES || num_faces <= 0 || num_faces > MAX_FACES) return 0;
  size_t temp = 0;
  if (!temp_bytes_for(num_vertices, num_faces, &temp)) return 0;
  return carve(num_vertices, num_faces, nullptr, 0, nullptr) + align_up(temp);
}

GSR_EXPORT int gsr_mesh_label(int num_vertices, int num_faces, const float *vertices, const int32_t *triangles,
                              int min_component_faces, int32_t *state, void *workspace, size_t workspace_bytes,
                              int32_t *labels, int32_t *sizes, gsr_stream_t stream) {
  const int V = num_vertices, F = num_faces;
  if (int rc = check_sizes(V, F, "mesh_label")) return rc;
  GSR_REQUIRE(min_component_faces >= 0, "mesh_label: min_component_faces < 0");
  GSR_REQUIRE(state != nullptr, "mesh_label: null state");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_state_init_kernel, dim3(1), dim3(8), 0, s, state);
  GSR_CHECK_LAUNCH("mesh_state_init");
  if (F == 0) return GSR_OK;
  GSR_REQUIRE(triangles != nullptr, "mesh_label: null triangles");
  if (int rc = check_workspace(workspace, workspace_bytes, gsr_mesh_clean_workspace_bytes(V, F), "mesh_label"))
    return rc;
  // rule 1: the index check reads `triangles` only, and its verdict is read here before any kernel that
  // dereferences with an index is launched
  hipLaunchKernelGGL(mesh_validate_kernel, dim3(gsr_cdiv(F, TPB)), dim3(TPB), 0, s, F, V, triangles, state);
  GSR_CHECK_LAUNCH("mesh_validate");
  int bad = 0;
  GSR_CHECK_HIP(hipMemcpyAsync(&bad, state + ST_BAD, sizeof(int), hipMemcpyDeviceToHost, s));
  GSR_CHECK_HIP(hipStreamSynchronize(s));
  if (bad != INT_MAX) {
    gsr_set_error("mesh_label: triangle %d has a vertex index outside [0, %d)", bad, V);
    return GSR_ERANGE;
  }

  Workspace w;
  carve(V, F, workspace, workspace_bytes, &w);
  const int vb = vertex_bits(V), E = 3 * F;
  const uint64_t none = 1ull << (2 * vb);
  const dim3 gf(gsr_cdiv(F, TPB)), ge(gsr_cdiv(E, TPB)), tpb(TPB);
  size_t tb;
  // rule 2
  hipLaunchKernelGGL(mesh_null_kernel, gf, tpb, 0, s, F, vertices, triangles, w.fflag,
                     reinterpret_cast<uint32_t *>(w.key_in), w.val_in, state);
  GSR_CHECK_LAUNCH("mesh_null");
  // rule 3: order by (largest index), then stably by (smallest, middle) = by the sorted triple, ties by face index
  tb = w.temp_bytes;
  GSR_CHECK_HIP(rocprim::radix_sort_pairs(w.temp, tb, reinterpret_cast<const uint32_t *>(w.key_in),
                                          reinterpret_cast<uint32_t *>(w.key_out), (const int32_t *)w.val_in,
                                          w.val_out, (size_t)F, 0, 32, s));
  hipLaunchKernelGGL(mesh_dupkey_kernel, gf, tpb, 0, s, F, vb, triangles, (const uint8_t *)w.fflag,
                     (const int32_t *)w.val_out, w.key_in);
  GSR_CHECK_LAUNCH("mesh_dupkey");
  tb = w.temp_bytes;
  GSR_CHECK_HIP(rocprim::radix_sort_pairs(w.temp, tb, (const uint64_t *)w.key_in, w.key_out,
                                          (const int32_t *)w.val_out, w.val_in, (size_t)F, 0, 2 * vb + 1, s));
  hipLaunchKernelGGL(mesh_dupflag_kernel, gf, tpb, 0, s, F, vb, triangles, (const uint64_t *)w.key_out,
                     (const int32_t *)w.val_in, w.fflag, state);
  GSR_CHECK_LAUNCH("mesh_dupflag");
  // rule 4
  hipLaunchKernelGGL(mesh_edges_kernel, gf, tpb, 0, s, F, vb, triangles, (const uint8_t *)w.fflag, w.key_in, w.val_in,
                     w.parent, w.count);
  GSR_CHECK_LAUNCH("mesh_edges");
  tb = w.temp_bytes;
  GSR_CHECK_HIP(rocprim::radix_sort_pairs(w.temp, tb, (const uint64_t *)w.key_in, w.key_out,
                                          (const int32_t *)w.val_in, w.val_out, (size_t)E, 0, 2 * vb + 1, s));
  hipLaunchKernelGGL(mesh_union_kernel, ge, tpb, 0, s, E, none, (const uint64_t *)w.key_out,
                     (const int32_t *)w.val_out, w.parent);
  GSR_CHECK_LAUNCH("mesh_union");
  hipLaunchKernelGGL(mesh_label_kernel, gf, tpb, 0, s, F, (const int32_t *)w.parent, (const uint8_t *)w.fflag, w.label,
                     w.count);
  GSR_CHECK_LAUNCH("mesh_label");
  hipLaunchKernelGGL(mesh_verify_kernel, ge, tpb, 0, s, E, none, (const uint64_t *)w.key_out,
                     (const int32_t *)w.val_out, (const int32_t *)w.label, state);
  GSR_CHECK_LAUNCH("mesh_verify");
  // rule 5: keep flags and vertex marks, then the two scans
  if (V > 0)
    if (int rc = gsr_zero_async(w.vmark, align_up((size_t)V), s)) return rc;
  hipLaunchKernelGGL(mesh_keep_kernel, gf, tpb, 0, s, F, min_component_faces, triangles, (const int32_t *)w.label,
                     (const int32_t *)w.count, w.size, w.keep, w.vmark, state);
  GSR_CHECK_LAUNCH("mesh_keep");
  tb = w.temp_bytes;
  GSR_CHECK_HIP(rocprim::inclusive_scan(w.temp, tb, (const int32_t *)w.keep, w.fincl, (size_t)F,
                                        rocprim::plus<int32_t>(), s));
  if (V > 0) {
    tb = w.temp_bytes;
    auto marks = rocprim::make_transform_iterator((const uint8_t *)w.vmark, MarkToInt());
    GSR_CHECK_HIP(rocprim::inclusive_scan(w.temp, tb, marks, w.vincl, (size_t)V, rocprim::plus<int32_t>(), s));
  }
  hipLaunchKernelGGL(mesh_store_totals_kernel, dim3(1), dim3(1), 0, s, (const int32_t *)w.fincl, F,
                     (const int32_t *)w.vincl, V, state);
  GSR_CHECK_LAUNCH("mesh_store_totals");
  if (labels || sizes) {
    hipLaunchKernelGGL(mesh_copy_kernel, gf, tpb, 0, s, F, (const int32_t *)w.label, labels, (const int32_t *)w.size,
                       sizes);
    GSR_CHECK_LAUNCH("mesh_copy");
  }
  return GSR_OK;
}

GSR_EXPORT int gsr_mesh_emit(int num_vertices, int num_faces, int num_attributes, const float *vertices,
                             const float *attributes, const int32_t *triangles, const void *workspace,
                             size_t workspace_bytes, int out_vertices, int out_faces, float *vertices_out,
                             float *attributes_out, int32_t *triangles_out, gsr_stream_t stream) {
  const int V = num_vertices, F = num_faces, C = attributes ? num_attributes : 0;
  if (int rc = check_sizes(V, F, "mesh_emit")) return rc;
  GSR_REQUIRE(num_attributes >= 0, "mesh_emit: num_attributes < 0");
  GSR_REQUIRE(out_vertices >= 0 && out_faces >= 0 && out_vertices <= V && out_faces <= F,
              "mesh_emit: output counts outside [0, V] / [0, F]");
  if (out_faces == 0 || out_vertices == 0) return GSR_OK;
  GSR_REQUIRE(vertices && triangles && vertices_out && triangles_out && (C == 0 || attributes_out),
              "mesh_emit: null pointer");
  if (int rc = check_workspace(workspace, workspace_bytes, gsr_mesh_clean_workspace_bytes(V, F), "mesh_emit"))
    return rc;
  Workspace w;
  carve(V, F, const_cast<void *>(workspace), workspace_bytes, &w);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_emit_faces_kernel, dim3(gsr_cdiv(F, TPB)), dim3(TPB), 0, s, F, triangles,
                     (const int32_t *)w.keep, (const int32_t *)w.fincl, (const int32_t *)w.vincl, out_faces,
                     triangles_out);
  GSR_CHECK_LAUNCH("mesh_emit_faces");
  hipLaunchKernelGGL(mesh_emit_vertices_kernel, dim3(gsr_cdiv(V, TPB)), dim3(TPB), 0, s, V, C,
                     reinterpret_cast<const uint32_t *>(vertices), reinterpret_cast<const uint32_t *>(attributes),
                     (const uint8_t *)w.vmark, (const int32_t *)w.vincl, out_vertices,
                     reinterpret_cast<uint32_t *>(vertices_out), reinterpret_cast<uint32_t *>(attributes_out));
  GSR_CHECK_LAUNCH("mesh_emit_vertices");
  return GSR_OK;
}
