// mcmc.hip -- densification by relocation ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et al.
// 2024; gsplat's MCMCStrategy), gfx950: dead Gaussians are moved onto live ones sampled by opacity, the model grows by
// a fixed factor up to a cap, a relocated or cloned Gaussian gets the opacity and scale that leave the image unchanged,
// position noise scaled by the covariance follows every optimiser step, and two L1 regularisers let Gaussians die.
//
// As in refine.hip the *decisions* are separated from the *data movement*:
//   gsr_mcmc_plan    one pass over the opacity logits: opacity, dead flag, an INTEGER sampling weight
//                    floor(opacity * 2^24), the inclusive uint64 prefix sum of the weights and the ranks of the dead
//                    rows (integer scans: any scan shape gives the same table), then the draws -- one Philox block
//                    each, target = mulhi64(r, total), source by binary search in the prefix table, count[source] += 1
//                    with an integer atomic.  No floating-point sum anywhere: the plan is bit-reproducible.
//   gsr_mcmc_apply   the sources' new opacity / scale (float64, below) into scratch first, then ONE streaming launch
//                    over the tensor table: sources take their new values, destination rows become copies of their
//                    source AFTER that update, the Adam moments of both are zeroed.  A destination reads the scratch
//                    values or rows that no thread writes (a source is alive, a destination dead): nothing depends on
//                    scheduling.
// The number of new rows is host arithmetic and the number of dead rows stays on the device: no read-back.
//
// Relocation values (gsplat's compute_relocation) for opacity o, ratio n in [1, 51]:
//   o' = 1 - (1 - o)^(1/n);   D = sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1);   s' = (o / D) s
// in float64: the alternating sum loses 1.4e-4 relative in float32 (measured on the host over o in [0.005, 1 - 1e-6],
// n in [1, 51]; float64: 6.6e-13).  The binomials are a 51 x 51 Pascal table in constant memory, exact in float64
// (C(50,25) < 2^53).
#include "gsr_common.h"
#include "philox.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxRatio = GSR_MCMC_MAX_RATIO;

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }  // activations.hip's expression

struct Pascal {
  double c[kMaxRatio][kMaxRatio];
  constexpr Pascal() : c{} {
    for (int i = 0; i < kMaxRatio; ++i) {
      c[i][0] = 1.0;
      for (int k = 1; k <= i; ++k) c[i][k] = c[i - 1][k - 1] + (k < i ? c[i - 1][k] : 0.0);
    }
  }
};
__constant__ Pascal kPascal = Pascal();

// o in (0,1), n in [1, 51] -> o' and o / D
__device__ void relocation_values(const double o, const int n, double &o_new, double &ratio) {
  o_new = 1.0 - pow(1.0 - o, 1.0 / (double)n);
  double D = 0.0;
  for (int i = 1; i <= n; ++i) {
    double p = o_new, sign = 1.0;
    for (int k = 0; k < i; ++k) {
      D += kPascal.c[i - 1][k] * sign * p / sqrt((double)(k + 1));
      p *= o_new;
      sign = -sign;
    }
  }
  ratio = o / D;
}

__device__ __forceinline__ double clamp_opacity(const double o, const double min_opacity) {
  return fmin(fmax(o, min_opacity), 1.0 - 1.1920928955078125e-07);
}

// ---- (a) on its own -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mcmc_relocation_kernel(const int n, const float *__restrict__ opacities,
                                                                 const float *__restrict__ scales,
                                                                 const int *__restrict__ ratios, const float min_opacity,
                                                                 const int raw_outputs, float *__restrict__ out_o,
                                                                 float *__restrict__ out_s) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int r = min(max(ratios[i], 1), kMaxRatio);
  const float o = opacities[i];
  const float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
  double o_new = (double)o, ratio = 1.0;
  if (r > 1) relocation_values((double)o, r, o_new, ratio);
  if (raw_outputs) {
    const double oc = clamp_opacity(o_new, (double)min_opacity);
    out_o[i] = (float)log(oc / (1.0 - oc));
    const double lr = log(ratio);
    out_s[3 * i] = (float)(log((double)s0) + lr);
    out_s[3 * i + 1] = (float)(log((double)s1) + lr);
    out_s[3 * i + 2] = (float)(log((double)s2) + lr);
  } else if (r == 1) {  // the inputs, unchanged
    out_o[i] = o, out_s[3 * i] = s0, out_s[3 * i + 1] = s1, out_s[3 * i + 2] = s2;
  } else {
    out_o[i] = (float)clamp_opacity(o_new, (double)min_opacity);
    out_s[3 * i] = (float)(ratio * (double)s0);
    out_s[3 * i + 1] = (float)(ratio * (double)s1);
    out_s[3 * i + 2] = (float)(ratio * (double)s2);
  }
}

// ---- (b) plan: integer scans ------------------------------------------------------------------------------------------
struct WD {
  unsigned long long w;  // sampling weight
  int d;                 // dead flag
};
__device__ __forceinline__ WD addwd(WD a, WD b) { return WD{a.w + b.w, a.d + b.d}; }

__device__ __forceinline__ WD weight_of(const float o, const float min_opacity, const int phase) {
  const bool dead = o <= min_opacity;  // NaN compares false
  // o * 2^24 is exact in float32 (a power of two); a NaN opacity gets weight 0
  unsigned w = (o == o) ? (unsigned)floorf(o * 16777216.f) : 0u;
  if (phase == GSR_MCMC_RELOCATE && dead) w = 0u;
  return WD{(unsigned long long)w, dead ? 1 : 0};
}

__device__ __forceinline__ WD wave_inclusive(WD v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    WD o;
    o.w = __shfl_up(v.w, d, 64);
    o.d = __shfl_up(v.d, d, 64);
    if ((int)(threadIdx.x & 63) >= d) v = addwd(v, o);
  }
  return v;
}

__device__ __forceinline__ WD block_inclusive(WD v, WD &total) {
  __shared__ WD wsum[kBlock / 64];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  v = wave_inclusive(v);
  __syncthreads();  // wsum may still be read from a previous call
  if (l == 63) wsum[w] = v;
  __syncthreads();
  WD base{0ull, 0}, t{0ull, 0};
#pragma unroll
  for (int k = 0; k < kBlock / 64; ++k) {
    if (k < w) base = addwd(base, wsum[k]);
    t = addwd(t, wsum[k]);
  }
  total = t;
  return addwd(v, base);
}

// pass 1: opacity by-product + per-workgroup totals
__global__ __launch_bounds__(kBlock) void mcmc_weights_kernel(const int n, const float *__restrict__ logits,
                                                              const float min_opacity, const int phase,
                                                              float *__restrict__ opac, WD *__restrict__ block_sums) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  WD v{0ull, 0};
  if (i < n) {
    const float o = sigmoidf_(logits[i]);
    opac[i] = o;
    v = weight_of(o, min_opacity, phase);
  }
  WD total;
  block_inclusive(v, total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// pass 2: one workgroup scans the per-workgroup totals in place (exclusive); totals = {sum of weights, dead rows}
__global__ __launch_bounds__(kBlock) void mcmc_scan_blocks_kernel(const int num_blocks, WD *__restrict__ block_sums,
                                                                  unsigned long long *__restrict__ totals) {
  WD carry{0ull, 0};
  for (int base = 0; base < num_blocks; base += kBlock) {
    const int b = base + threadIdx.x;
    const WD v = b < num_blocks ? block_sums[b] : WD{0ull, 0};
    WD total;
    const WD inc = block_inclusive(v, total);
    if (b < num_blocks) block_sums[b] = WD{carry.w + inc.w - v.w, carry.d + inc.d - v.d};
    carry = addwd(carry, total);
  }
  if (threadIdx.x == 0) {
    totals[0] = carry.w;
    totals[1] = (unsigned long long)carry.d;
  }
}

// pass 3: inclusive prefix of the weights, the dead rows in ascending order, and the draws' tables cleared
__global__ __launch_bounds__(kBlock) void mcmc_prefix_kernel(const int n, const float *__restrict__ opac,
                                                             const float min_opacity, const int phase,
                                                             const WD *__restrict__ block_sums,
                                                             unsigned long long *__restrict__ prefix,
                                                             int *__restrict__ dead_index, int *__restrict__ row_source,
                                                             int *__restrict__ counts) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const WD v = i < n ? weight_of(opac[i], min_opacity, phase) : WD{0ull, 0};
  WD total;
  const WD inc = block_inclusive(v, total);
  if (i < n) {
    const WD b = block_sums[blockIdx.x];
    prefix[i] = b.w + inc.w;
    if (v.d) dead_index[b.d + inc.d - 1] = i;  // rank < number of dead rows <= n
    row_source[i] = -1;
    counts[i] = 0;
  }
}

// ---- (c) draws -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mcmc_draw_kernel(const int n, const int num_draws, const int phase,
                                                           const unsigned step, const uint64_t seed,
                                                           const unsigned long long *__restrict__ prefix,
                                                           const int *__restrict__ dead_index,
                                                           const unsigned long long *__restrict__ totals,
                                                           int *__restrict__ draw_source, int *__restrict__ row_source,
                                                           int *__restrict__ counts) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long total = totals[0];
  const int nd = phase == GSR_MCMC_RELOCATE ? min((int)totals[1], n) : num_draws;
  if (j >= nd) return;
  if (total == 0ull) {  // nothing to sample from: relocation does nothing, a new row copies row j mod n unchanged
    draw_source[j] = phase == GSR_MCMC_RELOCATE ? -1 : j % n;
    return;
  }
  uint32_t c0 = (uint32_t)j, c1 = (uint32_t)phase, c2 = step, c3 = 0;
  philox4x32_10(seed, c0, c1, c2, c3);
  const unsigned long long r = ((unsigned long long)c0 << 32) | c1;
  const unsigned long long target = __umul64hi(r, total);  // in [0, total)
  int lo = 0, hi = n - 1;  // first index whose inclusive prefix is > target; prefix[n - 1] = total > target
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (prefix[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  draw_source[j] = lo;
  atomicAdd(&counts[lo], 1);
  if (phase == GSR_MCMC_RELOCATE) row_source[dead_index[j]] = lo;
}

// ---- (d) apply -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mcmc_new_values_kernel(const int n, const float *__restrict__ opac,
                                                                 const float *__restrict__ log_scales,
                                                                 const int *__restrict__ counts, const float min_opacity,
                                                                 float *__restrict__ new_logits,
                                                                 float *__restrict__ new_log_scales) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int c = counts[i];
  if (c <= 0) return;
  double o_new, ratio;
  relocation_values((double)opac[i], min(c + 1, kMaxRatio), o_new, ratio);
  const double oc = clamp_opacity(o_new, (double)min_opacity), lr = log(ratio);
  new_logits[i] = (float)log(oc / (1.0 - oc));
#pragma unroll
  for (int k = 0; k < 3; ++k) new_log_scales[3 * i + k] = (float)((double)log_scales[3 * i + k] + lr);
}

constexpr int kMaxTensors = GSR_REFINE_MAX_TENSORS;
struct ApplyArgs {
  gsr_refine_tensor t[kMaxTensors];
  int first_block[kMaxTensors + 1];
  int num;
};
constexpr int kElemsPerBlock = kBlock * 4;

__global__ __launch_bounds__(kBlock) void mcmc_apply_kernel(const ApplyArgs a, const int n_in, const int n_out,
                                                            const int *__restrict__ row_source,
                                                            const int *__restrict__ draw_source,
                                                            const int *__restrict__ counts,
                                                            const float *__restrict__ new_logits,
                                                            const float *__restrict__ new_log_scales) {
  int ti = 0;
#pragma unroll
  for (int k = 1; k < kMaxTensors; ++k)
    if (k < a.num && (int)blockIdx.x >= a.first_block[k]) ti = k;
  const gsr_refine_tensor T = a.t[ti];
  const long long blk = (long long)blockIdx.x - a.first_block[ti];
  const int w = T.width;
  const long long total = (long long)n_out * w;
  const bool in_place = T.in == T.out;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long e = blk * kElemsPerBlock + u * kBlock + threadIdx.x;
    if (e >= total) continue;
    const int r = (int)(e / w), c = (int)(e - (long long)r * w);
    const int s = r < n_in ? row_source[r] : draw_source[r - n_in];
    const bool is_new = s >= 0;
    const int src = is_new ? s : r;  // < n_in
    const bool updated = counts[src] > 0;
    if (!is_new && !updated) {
      if (!in_place) T.out[e] = T.in[e];
      continue;
    }
    float v;
    if (T.kind == GSR_REFINE_MOMENT) v = 0.f;
    else if (T.kind == GSR_MCMC_OPACITIES && updated) v = new_logits[src];
    else if (T.kind == GSR_REFINE_LOG_SCALES && updated) v = new_log_scales[3 * src + c];
    else v = T.in[(long long)src * w + c];  // (in place: a source row of this kind is written by no thread)
    T.out[e] = v;
  }
}

// ---- (e) noise -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void mcmc_noise_kernel(const int n, float *__restrict__ means,
                                                            const float *__restrict__ log_scales,
                                                            const float *__restrict__ raw_quats,
                                                            const float *__restrict__ logits, const float scaler,
                                                            const unsigned step, const uint64_t seed,
                                                            const float *__restrict__ noise) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float z[3];
  if (noise) z[0] = noise[3 * i], z[1] = noise[3 * i + 1], z[2] = noise[3 * i + 2];
  else split_normals(seed, (uint32_t)i, step, z);
  const float o = sigmoidf_(logits[i]);
  const float gate = 1.f / (1.f + expf(-100.f * ((1.f - o) - 0.995f)));
  const float g = gate * scaler;
  if (g == 0.f) return;  // scaler 0 (or a gate that underflowed): the means stay bit-identical
  const float vx = z[0] * g, vy = z[1] * g, vz = z[2] * g;
  const float4 q4 = reinterpret_cast<const float4 *>(raw_quats)[i];
  const float inv = 1.f / fmaxf(sqrtf(q4.x * q4.x + q4.y * q4.y + q4.z * q4.z + q4.w * q4.w), 1e-12f);
  const float qw = q4.x * inv, qx = q4.y * inv, qy = q4.z * inv, qz = q4.w * inv;
  const float r00 = 1.f - 2.f * (qy * qy + qz * qz), r01 = 2.f * (qx * qy - qw * qz), r02 = 2.f * (qx * qz + qw * qy);
  const float r10 = 2.f * (qx * qy + qw * qz), r11 = 1.f - 2.f * (qx * qx + qz * qz), r12 = 2.f * (qy * qz - qw * qx);
  const float r20 = 2.f * (qx * qz - qw * qy), r21 = 2.f * (qy * qz + qw * qx), r22 = 1.f - 2.f * (qx * qx + qy * qy);
  const float e0 = expf(log_scales[3 * i]), e1 = expf(log_scales[3 * i + 1]), e2 = expf(log_scales[3 * i + 2]);
  // Sigma v = R diag(s^2) R^T v
  const float t0 = (r00 * vx + r10 * vy + r20 * vz) * (e0 * e0);
  const float t1 = (r01 * vx + r11 * vy + r21 * vz) * (e1 * e1);
  const float t2 = (r02 * vx + r12 * vy + r22 * vz) * (e2 * e2);
  means[3 * i] += r00 * t0 + r01 * t1 + r02 * t2;
  means[3 * i + 1] += r10 * t0 + r11 * t1 + r12 * t2;
  means[3 * i + 2] += r20 * t0 + r21 * t1 + r22 * t2;
}

// ---- (f) regularisers ------------------------------------------------------------------------------------------------
// L = opacity_reg * mean(sigmoid(logit)) + scale_reg * mean(exp(log_scale)); float64 terms, sums in a fixed order:
// lane (grid-stride, ascending) -> wave (shuffle tree) -> workgroup (waves in order) -> grid (second launch, same
// shape over the workgroups' partial sums).  No floating-point atomics.
constexpr int kRegBlocks = 1024;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // lane 0
}

__device__ __forceinline__ void block_sum2(double &a, double &b) {  // thread 0 gets the sums
  __shared__ double sa[kBlock / 64], sb[kBlock / 64];
  a = wave_sum(a), b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) sa[threadIdx.x >> 6] = a, sb[threadIdx.x >> 6] = b;
  __syncthreads();
  if (threadIdx.x == 0) {
    a = sa[0], b = sb[0];
    for (int k = 1; k < kBlock / 64; ++k) a += sa[k], b += sb[k];
  }
}

__global__ __launch_bounds__(kBlock) void mcmc_reg_partial_kernel(const int n, const float *__restrict__ logits,
                                                                  const float *__restrict__ log_scales,
                                                                  double *__restrict__ partials) {
  double so = 0.0, ss = 0.0;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    so += 1.0 / (1.0 + exp(-(double)logits[i]));
    ss += (exp((double)log_scales[3 * i]) + exp((double)log_scales[3 * i + 1])) + exp((double)log_scales[3 * i + 2]);
  }
  block_sum2(so, ss);
  if (threadIdx.x == 0) partials[2 * blockIdx.x] = so, partials[2 * blockIdx.x + 1] = ss;
}

__global__ __launch_bounds__(kBlock) void mcmc_reg_final_kernel(const int n, const int num_partials,
                                                                const double *__restrict__ partials,
                                                                const double opacity_reg, const double scale_reg,
                                                                double *__restrict__ out) {
  double so = 0.0, ss = 0.0;
  for (int b = threadIdx.x; b < num_partials; b += kBlock) so += partials[2 * b], ss += partials[2 * b + 1];
  block_sum2(so, ss);
  if (threadIdx.x == 0) {
    const double mo = so / (double)n, ms = ss / (3.0 * (double)n);
    out[0] = opacity_reg * mo + scale_reg * ms;
    out[1] = mo;
    out[2] = ms;
  }
}

__global__ __launch_bounds__(kBlock) void mcmc_reg_backward_kernel(const int n, const float *__restrict__ logits,
                                                                   const float *__restrict__ log_scales,
                                                                   const double opacity_reg, const double scale_reg,
                                                                   const double *__restrict__ v_out,
                                                                   float *__restrict__ v_logits,
                                                                   float *__restrict__ v_log_scales) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const double v = v_out[0];
  const double sg = 1.0 / (1.0 + exp(-(double)logits[i]));
  v_logits[i] = (float)(v * (opacity_reg / (double)n) * sg * (1.0 - sg));
  const double c = v * (scale_reg / (3.0 * (double)n));
#pragma unroll
  for (int k = 0; k < 3; ++k) v_log_scales[3 * i + k] = (float)(c * exp((double)log_scales[3 * i + k]));
}

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

GSR_EXPORT int gsr_mcmc_relocation(int n, const float *opacities, const float *scales, const int32_t *ratios,
                                   float min_opacity, int raw_outputs, float *new_opacities, float *new_scales,
                                   gsr_stream_t stream) {
  GSR_REQUIRE(n >= 0, "mcmc_relocation: n < 0");
  if (n == 0) return GSR_OK;
  GSR_REQUIRE(opacities && scales && ratios && new_opacities && new_scales, "mcmc_relocation: null pointer");
  hipLaunchKernelGGL(mcmc_relocation_kernel, dim3(gsr_cdiv((unsigned)n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                     n, opacities, scales, ratios, min_opacity, raw_outputs, new_opacities, new_scales);
  GSR_CHECK_LAUNCH("mcmc_relocation");
  return GSR_OK;
}

GSR_EXPORT size_t gsr_mcmc_workspace_bytes(int num_points) {
  const size_t blocks = gsr_cdiv((unsigned)(num_points > 0 ? num_points : 1), kBlock);
  return align256(blocks * sizeof(WD)) + 256;
}

GSR_EXPORT int gsr_mcmc_plan(int num_points, int num_draws, int phase, const float *opacity_logits, float min_opacity,
                             unsigned int step, unsigned long long seed, float *opac, uint64_t *prefix,
                             int32_t *dead_index, int32_t *draw_source, int32_t *row_source, int32_t *counts,
                             uint64_t *totals, void *workspace, size_t workspace_bytes, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 1, "mcmc_plan: num_points < 1");
  GSR_REQUIRE(phase == GSR_MCMC_RELOCATE || phase == GSR_MCMC_ADD, "mcmc_plan: unknown phase");
  GSR_REQUIRE(phase == GSR_MCMC_RELOCATE || num_draws >= 0, "mcmc_plan: num_draws < 0");
  GSR_REQUIRE(opacity_logits && opac && prefix && dead_index && draw_source && row_source && counts && totals &&
                  workspace,
              "mcmc_plan: null pointer");
  GSR_REQUIRE(workspace_bytes >= gsr_mcmc_workspace_bytes(num_points), "mcmc_plan: workspace too small");
  GSR_REQUIRE(aligned(workspace, 16) && aligned(prefix, 8) && aligned(totals, 8),
              "mcmc_plan: workspace must be 16-byte, prefix / totals 8-byte aligned");
  const unsigned blocks = gsr_cdiv((unsigned)num_points, kBlock);
  WD *block_sums = reinterpret_cast<WD *>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mcmc_weights_kernel, dim3(blocks), dim3(kBlock), 0, s, num_points, opacity_logits, min_opacity,
                     phase, opac, block_sums);
  hipLaunchKernelGGL(mcmc_scan_blocks_kernel, dim3(1), dim3(kBlock), 0, s, (int)blocks, block_sums,
                     reinterpret_cast<unsigned long long *>(totals));
  hipLaunchKernelGGL(mcmc_prefix_kernel, dim3(blocks), dim3(kBlock), 0, s, num_points, opac, min_opacity, phase,
                     block_sums, reinterpret_cast<unsigned long long *>(prefix), dead_index, row_source, counts);
  // relocate: one draw per dead row (their number stays on the device: at most num_points); add: num_draws
  const int max_draws = phase == GSR_MCMC_RELOCATE ? num_points : num_draws;
  if (max_draws > 0)
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3(gsr_cdiv((unsigned)max_draws, kBlock)), dim3(kBlock), 0, s, num_points,
                       num_draws, phase, step, (uint64_t)seed, reinterpret_cast<const unsigned long long *>(prefix),
                       dead_index, reinterpret_cast<const unsigned long long *>(totals), draw_source, row_source, counts);
  GSR_CHECK_LAUNCH("mcmc_plan");
  return GSR_OK;
}

GSR_EXPORT int gsr_mcmc_apply(int n_in, int n_out, const float *opac, const float *log_scales, float min_opacity,
                              const int32_t *row_source, const int32_t *draw_source, const int32_t *counts,
                              float *scratch, int num_tensors, const gsr_refine_tensor *tensors, gsr_stream_t stream) {
  GSR_REQUIRE(n_in >= 1 && n_out >= n_in, "mcmc_apply: need 1 <= n_in <= n_out");
  GSR_REQUIRE(num_tensors >= 0 && num_tensors <= kMaxTensors, "mcmc_apply: too many tensors for one call");
  GSR_REQUIRE(opac && log_scales && row_source && counts && scratch && (n_out == n_in || draw_source),
              "mcmc_apply: null pointer");
  hipStream_t s = (hipStream_t)stream;
  float *new_logits = scratch, *new_log_scales = scratch + n_in;  // [n_in] + [n_in, 3]
  // (one call moves every tensor of a refinement -- six parameters and twelve moments fit the table: a second call
  //  in place would form the scratch from log-scales the first has already updated)
  hipLaunchKernelGGL(mcmc_new_values_kernel, dim3(gsr_cdiv((unsigned)n_in, kBlock)), dim3(kBlock), 0, s, n_in, opac,
                     log_scales, counts, min_opacity, new_logits, new_log_scales);
  if (num_tensors > 0) {
    GSR_REQUIRE(tensors, "mcmc_apply: null pointer");
    ApplyArgs a{};
    a.num = num_tensors;
    long long blocks = 0;
    for (int k = 0; k < num_tensors; ++k) {
      const gsr_refine_tensor &t = tensors[k];
      GSR_REQUIRE(t.in && t.out && t.width >= 1, "mcmc_apply: bad tensor");
      GSR_REQUIRE(t.kind == GSR_REFINE_COPY || t.kind == GSR_REFINE_LOG_SCALES || t.kind == GSR_REFINE_MOMENT ||
                      t.kind == GSR_MCMC_OPACITIES,
                  "mcmc_apply: unknown tensor kind");
      GSR_REQUIRE(t.kind != GSR_REFINE_LOG_SCALES || t.width == 3, "mcmc_apply: log-scales have width 3");
      GSR_REQUIRE(t.kind != GSR_MCMC_OPACITIES || t.width == 1, "mcmc_apply: opacities have width 1");
      GSR_REQUIRE(n_out == n_in || t.in != t.out, "mcmc_apply: growth needs separate outputs");
      a.t[k] = t;
      a.first_block[k] = (int)blocks;
      blocks += ((long long)n_out * t.width + kElemsPerBlock - 1) / kElemsPerBlock;
      GSR_REQUIRE(blocks < (1ll << 31), "mcmc_apply: too many elements for one launch");
    }
    a.first_block[num_tensors] = (int)blocks;
    hipLaunchKernelGGL(mcmc_apply_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, a, n_in, n_out, row_source,
                       draw_source, counts, new_logits, new_log_scales);
  }
  GSR_CHECK_LAUNCH("mcmc_apply");
  return GSR_OK;
}

GSR_EXPORT int gsr_mcmc_noise(int num_points, float *means, const float *log_scales, const float *raw_quats,
                              const float *opacity_logits, float scaler, unsigned int step, unsigned long long seed,
                              const float *noise, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 0, "mcmc_noise: num_points < 0");
  if (num_points == 0) return GSR_OK;
  GSR_REQUIRE(means && log_scales && raw_quats && opacity_logits, "mcmc_noise: null pointer");
  GSR_REQUIRE(aligned(raw_quats, 16), "mcmc_noise: quaternions must be 16-byte aligned");
  hipLaunchKernelGGL(mcmc_noise_kernel, dim3(gsr_cdiv((unsigned)num_points, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, num_points, means, log_scales, raw_quats, opacity_logits, scaler, step,
                     (uint64_t)seed, noise);
  GSR_CHECK_LAUNCH("mcmc_noise");
  return GSR_OK;
}

GSR_EXPORT size_t gsr_mcmc_reg_workspace_bytes(void) { return (size_t)kRegBlocks * 2 * sizeof(double); }

GSR_EXPORT int gsr_mcmc_reg_forward(int num_points, const float *opacity_logits, const float *log_scales,
                                    double opacity_reg, double scale_reg, double *out, void *workspace,
                                    size_t workspace_bytes, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 1, "mcmc_reg_forward: num_points < 1");
  GSR_REQUIRE(opacity_logits && log_scales && out && workspace, "mcmc_reg_forward: null pointer");
  GSR_REQUIRE(workspace_bytes >= gsr_mcmc_reg_workspace_bytes() && aligned(workspace, 8) && aligned(out, 8),
              "mcmc_reg_forward: workspace too small or misaligned");
  const unsigned need = gsr_cdiv((unsigned)num_points, kBlock);
  const int blocks = (int)(need < (unsigned)kRegBlocks ? need : (unsigned)kRegBlocks);
  double *partials = reinterpret_cast<double *>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mcmc_reg_partial_kernel, dim3(blocks), dim3(kBlock), 0, s, num_points, opacity_logits, log_scales,
                     partials);
  hipLaunchKernelGGL(mcmc_reg_final_kernel, dim3(1), dim3(kBlock), 0, s, num_points, blocks, partials, opacity_reg,
                     scale_reg, out);
  GSR_CHECK_LAUNCH("mcmc_reg_forward");
  return GSR_OK;
}

GSR_EXPORT int gsr_mcmc_reg_backward(int num_points, const float *opacity_logits, const float *log_scales,
                                     double opacity_reg, double scale_reg, const double *v_out, float *v_logits,
                                     float *v_log_scales, gsr_stream_t stream) {
  GSR_REQUIRE(num_points >= 1, "mcmc_reg_backward: num_points < 1");
  GSR_REQUIRE(opacity_logits && log_scales && v_out && v_logits && v_log_scales, "mcmc_reg_backward: null pointer");
  hipLaunchKernelGGL(mcmc_reg_backward_kernel, dim3(gsr_cdiv((unsigned)num_points, kBlock)), dim3(kBlock), 0,
                     (hipStream_t)stream, num_points, opacity_logits, log_scales, opacity_reg, scale_reg, v_out,
                     v_logits, v_log_scales);
  GSR_CHECK_LAUNCH("mcmc_reg_backward");
  return GSR_OK;
}
