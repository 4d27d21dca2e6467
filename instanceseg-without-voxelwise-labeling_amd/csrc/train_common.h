// Device helpers shared by the two training-target files (rpn_train.hip, box_head_train.hip): the sampling hash of DESIGN
// ("Sampling contract") and the fixed-order reductions of their single-workgroup kernels.
#pragma once
#include "m3d_common.h"

namespace m3dtrain {

constexpr int kOne = 1024;         // threads of the single-workgroup kernels

// key(i) = upper 32 bits of the splitmix64 finaliser of stream + i, where stream = the 64-bit finaliser of the caller's seed.
// Without that first scramble a key would depend on seed + i only, and draw j of seed s would be draw j - 1 of seed s + 1: callers
// that count their seeds up would replay shifted draws.
inline unsigned long long seed_stream(unsigned long long seed) {
  unsigned long long z = seed * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ inline unsigned int mix_key(unsigned long long seed, unsigned long long i) {
  unsigned long long z = (seed + i) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (unsigned int)(z >> 32);
}

// exclusive prefix of one value per thread over a workgroup of kOne threads; *total = the sum
__device__ inline unsigned int block_exscan(unsigned int v, unsigned int* sh, unsigned int* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < kOne; off <<= 1) {
    const unsigned int add = t >= off ? sh[t - off] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  *total = sh[kOne - 1];
  const unsigned int ex = sh[t] - v;
  __syncthreads();
  return ex;
}

template <typename T>
__device__ inline T block_sum(T v, T* sh) {   // fixed tree: the same bits every run
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = kOne / 2; off > 0; off >>= 1) {
    if (t < off) sh[t] += sh[t + off];
    __syncthreads();
  }
  const T r = sh[0];
  __syncthreads();
  return r;
}

}  // namespace m3dtrain
