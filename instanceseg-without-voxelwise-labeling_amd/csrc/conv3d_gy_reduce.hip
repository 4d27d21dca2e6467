// One pass over a conv layer's output gradient gy [batch, cout, D, H, W] for everything the backward of a training step needs from it
// besides the two GEMM-shaped launches: the bias gradient gb[c] = fp32(sum of gy[:, c] in fp64) and gy's operand bound (max |gy|, the
// slot array m3d_conv3d_zw_forward and m3d_conv3d_wgrad_f16x2 take).  Before it the f16x2 weight gradient swept gy for the bound and
// m3d_conv3d_bias_grad read it again with one workgroup per channel.
//
// The reduction is bn_train.hip's: every workgroup owns a span of kSpan elements of one (image, channel) slab (boundaries: a function of
// the shape only), 16-byte loads from the first aligned element, scalar head and tail (slabs of D H W % 4 != 0 elements misalign every
// other slab), per-thread fp64 sums in a fixed order, a fixed tree inside the workgroup, and a finish kernel that adds a channel's
// partials in ascending (image, span) order and rounds once.  No floating-point atomics.  The maximum travels as conv3d_zw.hip's epilogue
// leaves it: |value| as bits, one atomic max per workgroup into slot (workgroup % slots); a maximum does not depend on the order.
#include "m3d_common.h"

namespace {

constexpr int kTPB = 256;
constexpr int kSpan = 16384;      // elements of one slab that one workgroup reduces (64 per thread)

template <bool SUM>
__global__ __launch_bounds__(kTPB) void gy_reduce_partial_kernel(const float* __restrict__ gy, double* __restrict__ part,
                                                                 unsigned* __restrict__ slots, int C, long long V, int nspan, int P,
                                                                 int nslots) {
  __shared__ double sm[4];
  __shared__ unsigned wm[4];
  const long long slab = blockIdx.x / nspan;
  const int s = (int)(blockIdx.x % nspan);
  const long long off = (long long)s * kSpan;
  const long long left = V - off;
  const int len = (int)(left < kSpan ? left : kSpan);
  const float* p = gy + slab * V + off;
  double sum = 0.0;
  unsigned m = 0;
  auto take = [&](float v) {
    if (SUM) sum += (double)v;
    const unsigned b = __float_as_uint(v) & 0x7FFFFFFFu;
    m = b > m ? b : m;
  };
  int head = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);      // scalar elements in front of the first 16-byte boundary
  head = head < len ? head : len;
  if ((int)threadIdx.x < head) take(p[threadIdx.x]);
  const int nq = (len - head) >> 2;
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  for (int i = threadIdx.x; i < nq; i += kTPB) {
    const float4 q = p4[i];
    take(q.x); take(q.y); take(q.z); take(q.w);
  }
  const int t = head + 4 * nq + (int)threadIdx.x;
  if (t < len) take(p[t]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    if (SUM) sum += __shfl_down(sum, o, 64);
    const unsigned u = (unsigned)__shfl_xor((int)m, o);
    m = u > m ? u : m;
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[w] = sum; wm[w] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (SUM) part[(long long)(slab % C) * P + (slab / C) * nspan + s] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    m = max(max(wm[0], wm[1]), max(wm[2], wm[3]));
    if (m) atomicMax(slots + (blockIdx.x % (unsigned)nslots), m);
  }
}

__global__ __launch_bounds__(64) void gy_reduce_finish_kernel(const double* __restrict__ part, int C, int P, float* __restrict__ gb) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const double* p = part + (long long)c * P;
  double s = 0.0;
  for (int i = 0; i < P; ++i) s += p[i];
  gb[c] = (float)s;
}

}  // namespace

M3D_API int m3d_conv3d_gy_reduce(const float* d_gy, int batch, int cout, int depth, int height, int width, float* d_grad_bias,
                                 float* d_gy_max, void* d_ws, size_t* ws_bytes, void* stream) {
  if (batch < 1 || cout < 1 || depth < 1 || height < 1 || width < 1) return M3D_EINVAL;
  const long long DH = (long long)depth * height;
  if (DH >= (1ll << 31) || DH * width >= (1ll << 31)) return M3D_EUNSUPPORTED;
  const long long V = DH * width;
  const int nspan = (int)((V + kSpan - 1) / kSpan);
  // one workgroup per span: the grid stays under the 2^32 threads of one launch
  if ((long long)batch * cout * nspan >= (1ll << 32) / kTPB) return M3D_EUNSUPPORTED;
  const int P = batch * nspan;
  const size_t need = sizeof(double) * (size_t)cout * P;
  if (!d_ws) {
    if (!ws_bytes) return M3D_EINVAL;
    *ws_bytes = need;
    return M3D_OK;
  }
  if (!d_gy || ((uintptr_t)d_gy & 3) || !d_gy_max || ((uintptr_t)d_gy_max & 3) || ((uintptr_t)d_grad_bias & 3) || !ws_bytes ||
      ((uintptr_t)d_ws & 7))
    return M3D_EINVAL;
  if (*ws_bytes < need) return M3D_EWORKSPACE;
  hipStream_t st = m3d::as_stream(stream);
  const int nslots = m3d_conv3d_zw_slots();
  if (hipMemsetAsync(d_gy_max, 0, nslots * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
  const dim3 grid((unsigned)((long long)batch * cout * nspan));
  if (d_grad_bias) {
    hipLaunchKernelGGL(gy_reduce_partial_kernel<true>, grid, dim3(kTPB), 0, st, d_gy, (double*)d_ws, (unsigned*)d_gy_max, cout, V, nspan, P,
                       nslots);
    hipLaunchKernelGGL(gy_reduce_finish_kernel, dim3((cout + 63) / 64), dim3(64), 0, st, (const double*)d_ws, cout, P, d_grad_bias);
  } else {
    hipLaunchKernelGGL(gy_reduce_partial_kernel<false>, grid, dim3(kTPB), 0, st, d_gy, (double*)d_ws, (unsigned*)d_gy_max, cout, V, nspan, P,
                       nslots);
  }
  return m3d::check_launch("conv3d_gy_reduce");
}
