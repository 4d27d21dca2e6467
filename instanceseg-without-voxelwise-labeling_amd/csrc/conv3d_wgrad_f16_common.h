// What conv3d_wgrad_f16.hip and conv3d_wgrad_narrow_f16.hip share: the split-K workspace partial[slot][tap][co][ci], the kernel that
// folds it, the rule that sizes the slots and the argument checks of the entry points.  The two files differ in the voxel tile, the LDS
// images and the staging only.  They stay separate translation units (an unnamed namespace here on purpose: each gets its own copy of
// the reduce kernel in its own code object).
#pragma once
#include "f16x2.h"

namespace {

using namespace m3d::f16x2;

constexpr int RG = 8;                                       // strided groups of the reduce kernel
constexpr int WG_MAX_TILES = 16;                            // tiles of a slot: caps the MFMA chain of an accumulator (f16x2.h, mfma3)
constexpr int WG_TARGET_WGS = 512;                          // two workgroups per CU

// a wave's nine (dy, dx) accumulators of tap plane dz -> the slot's partial (pp), in scaled units: acc[i = co][j = ci], col j = r =
// lane & 31, row i = acc_row(g) + 4 h.  acc_row (f16x2.h) is spelled out: summed in another association, the two kernels come out with
// other scalar registers than they have had
__device__ __forceinline__ void store_partial(float* pp, const f32x16 (&acc)[3][3], int dz, int cb, int ib, int r, int h, int cin,
                                              int cout) {
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int tap = dz * 9 + dy * 3 + dx;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int co = cb * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
        pp[((size_t)tap * cout + co) * cin + ib * 32 + r] = acc[dy][dx][g];
      }
    }
}

// dW[co][ci][tap] = (sum over the slots in a fixed order) / s_g / s_x: a block is 32 consecutive partial elements x RG strided groups
__global__ __launch_bounds__(256) void conv3d_wgrad_f16_reduce_kernel(const float* __restrict__ partial, int slots, long long n, int cin,
                                                                      int cout, const float* __restrict__ x_max,
                                                                      const float* __restrict__ g_max, float* __restrict__ dw) {
  __shared__ float sm[RG][32];
  const int e = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long long i = (long long)blockIdx.x * 32 + e;                 // n is a multiple of 32 * 32 * 27
  float s_, inv_x, inv_g;
  f16_scale_of(bound_of_slots(x_max, threadIdx.x & 63), s_, inv_x);
  f16_scale_of(bound_of_slots(g_max, threadIdx.x & 63), s_, inv_g);
  float sum = 0.f;
  for (int s = g; s < slots; s += RG) sum += partial[(size_t)s * n + i];
  sm[g][e] = sum;
  __syncthreads();
  if (g == 0) {
    float tot = sm[0][e];
#pragma unroll
    for (int k = 1; k < RG; ++k) tot += sm[k][e];
    const long long cc = (long long)cout * cin;
    const int tap = (int)(i / cc);
    const long long rem = i - tap * cc;                                // co * cin + ci
    dw[rem * 27 + tap] = tot * inv_g * inv_x;
  }
}

inline bool extents_ok(int batch, int cin, int cout, int D, int H, int W) {
  return batch > 0 && cin > 0 && cout > 0 && D > 0 && H > 0 && W > 0;
}

// the slot rule, a function of the shape only: p.NT tiles -> cbs, ibs, tps, slots, n of either file's plan struct
template <class Plan>
void slot_rule(Plan& p, int cin, int cout) {
  p.cbs = cout / 32; p.ibs = cin / 32;
  const long long tps = (long long)p.NT * p.cbs * p.ibs / WG_TARGET_WGS;
  p.tps = (int)(tps < 1 ? 1 : tps > WG_MAX_TILES ? WG_MAX_TILES : tps);
  p.slots = (p.NT + p.tps - 1) / p.tps;
  p.n = (long long)cout * cin * 27;
}

// what the *_plan entry points report
template <class Plan>
void report_plan(const Plan& p, int mfma_per_tile, int* slots, int* tiles_per_slot, int* chain, int* folds) {
  if (slots) *slots = p.slots;
  if (tiles_per_slot) *tiles_per_slot = p.tps;
  if (chain) *chain = p.tps * mfma_per_tile;
  // fp32 operations on an output behind its MFMA chain: the adds of its strided group (the first partial is added to 0), the RG - 1 adds
  // of the group sums, the two scale multiplies
  if (folds) *folds = (p.slots + RG - 1) / RG + (RG - 1) + 2;
}

// pointers and alignment of a wgrad call
inline int check_args(const float* d_in, const float* d_grad_out, const float* d_grad_weight, const float* d_in_max,
                      const float* d_gy_max, const void* d_ws) {
  if (!d_in || !d_grad_out || !d_grad_weight || !d_in_max || !d_gy_max || !d_ws) return M3D_EINVAL;
  if (((uintptr_t)d_in | (uintptr_t)d_grad_out | (uintptr_t)d_grad_weight | (uintptr_t)d_in_max | (uintptr_t)d_gy_max) & 3) return M3D_EINVAL;
  if ((uintptr_t)d_ws & 15) return M3D_EINVAL;
  return M3D_OK;
}

}  // namespace
