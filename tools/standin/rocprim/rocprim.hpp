#pragma once
#include <hip/hip_runtime.h>
#include <numeric>
namespace rocprim {
template <class K> hipError_t radix_sort_keys(void *temp, size_t &bytes, const K *in, K *out, size_t n, unsigned, unsigned, hipStream_t = 0) {
  if (!temp) { bytes = 512; return hipSuccess; }
  memset(temp, 0xAB, bytes < 512 ? bytes : 512);
  std::copy(in, in + n, out); std::sort(out, out + n); return hipSuccess;
}
template <class K, class V> hipError_t radix_sort_pairs(void *temp, size_t &bytes, const K *kin, K *kout, const V *vin, V *vout, size_t n, unsigned, unsigned, hipStream_t = 0) {
  if (!temp) { bytes = 512; return hipSuccess; }
  memset(temp, 0xAB, bytes < 512 ? bytes : 512);
  std::vector<size_t> o(n); std::iota(o.begin(), o.end(), 0);
  std::stable_sort(o.begin(), o.end(), [&](size_t a, size_t b) { return kin[a] < kin[b]; });
  for (size_t i = 0; i < n; ++i) kout[i] = kin[o[i]], vout[i] = vin[o[i]];
  return hipSuccess;
}
}
