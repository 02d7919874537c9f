// host stand-in for the HIP names knn.hip uses: real threads per workgroup, a barrier for __syncthreads
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct float4 { float x, y, z, w; };
inline float4 make_float4(float x, float y, float z, float w) { return {x, y, z, w}; }
inline thread_local dim3 threadIdx, blockIdx, blockDim, gridDim;
inline std::barrier<> *shim_barrier = nullptr;
inline void __syncthreads() { shim_barrier->arrive_and_wait(); }
inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline int __float_as_int(float f) { int i; memcpy(&i, &f, 4); return i; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
using std::isfinite; using std::min; using std::max;
typedef void *hipStream_t;
typedef int hipError_t;
enum { hipSuccess = 0, hipMemcpyDeviceToHost = 2 };
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char *hipGetErrorString(hipError_t) { return "shim"; }
inline hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, int, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
template <class K, class... A>
void shim_launch(K kernel, dim3 grid, dim3 block, A... args) {
  for (unsigned b = 0; b < grid.x; ++b) {
    std::barrier<> bar(block.x);
    shim_barrier = &bar;
    std::barrier<> *pb = &bar;
    std::vector<std::thread> ts;
    for (unsigned t = 0; t < block.x; ++t)
      ts.emplace_back([=] { threadIdx = dim3(t); blockIdx = dim3(b); blockDim = block; gridDim = grid; kernel(args...); pb->arrive_and_drop(); });
    for (auto &t : ts) t.join();
  }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) shim_launch(kernel, grid, block, __VA_ARGS__)
