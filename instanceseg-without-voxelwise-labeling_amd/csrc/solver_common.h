// What the solver's update files (sgd.hip, adam.hip) share: the chunking, the statistics tree and the pointer checks (DESIGN, "Solver").
// Work is cut into chunks of kChunk elements of one tensor (a function of the tensors' sizes and order only); one workgroup per chunk.
// Statistics: one fp64 partial and one count per chunk, summed by a finish kernel in a fixed order - no floating-point atomics.
#pragma once
#include "m3d_common.h"

namespace {

constexpr int kTPB = 256;
constexpr int kChunk = 8192;            // elements per workgroup: 8 quads per thread
constexpr int kMaxSeg = 64;             // descriptors per launch (the kernel-argument space holds 4 KB)
constexpr int kMaxBlocks = 1 << 22;     // workgroups per launch (2^35 elements)
constexpr int kMaxCount = 65536;
constexpr long long kMaxN = 1ll << 40;

__device__ __forceinline__ void stat_of(float g, double& s, double& bad) {
  const double v = (double)g;
  s += v * v;
  bad += (__float_as_uint(g) & 0x7f800000u) == 0x7f800000u ? 1.0 : 0.0;
}

// (a, b) summed over the workgroup in a fixed tree; valid in thread 0
__device__ __forceinline__ void block_sum2(double& a, double& b, double* sm) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[2 * w] = a; sm[2 * w + 1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = (sm[0] + sm[2]) + (sm[4] + sm[6]);
    b = (sm[1] + sm[3]) + (sm[5] + sm[7]);
  }
}

// thread t adds the partials t, t + kTPB, ... in ascending order, then the fixed tree: a function of the number of chunks only
__device__ __forceinline__ void finish_sum2(const double* __restrict__ part, long long chunks, double& s, double& bad, double* sm) {
  s = 0.0;
  bad = 0.0;
  for (long long i = threadIdx.x; i < chunks; i += kTPB) { s += part[2 * i]; bad += part[2 * i + 1]; }
  block_sum2(s, bad, sm);
}

inline long long chunks_of(long long n) { return (n + kChunk - 1) / kChunk; }

inline bool apart(const void* a, const void* b, long long n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * 4;
  return x < y ? y - x >= bytes : x - y >= bytes;
}

// the d_stats / d_ws / ws_bytes convention of m3d_sgd_step for a call of `chunks` chunks: M3D_OK with *query set for the size query
inline int stats_workspace(const double* d_stats, const void* d_ws, size_t* ws_bytes, long long chunks, bool* query) {
  const size_t need = d_stats ? sizeof(double) * 2 * (size_t)chunks : 0;
  *query = !d_ws && ws_bytes;
  if (*query) {
    *ws_bytes = need;
    return M3D_OK;
  }
  if (d_stats) {
    if (((uintptr_t)d_stats | (uintptr_t)d_ws) & 7) return M3D_EINVAL;
    if (need > 0 && (!d_ws || !ws_bytes)) return M3D_EINVAL;
    if (need > 0 && *ws_bytes < need) return M3D_EWORKSPACE;
  }
  return M3D_OK;
}

}  // namespace
