// The "f16x2" arithmetic, once: what every kernel file that runs fp32 GEMMs on the f16 matrix cores has to agree on (the test side's
// statement of the same contract is tests/f16x2_contract.py).
//
// fp16 carries an 11-bit significand, so an fp32 operand x, scaled by a power of two s (exact), is cut into two fp16 numbers
//     x s = h + l + e,   h = fp16(x s) (round to nearest),   l = fp16(x s - h),   |e| <= 2^-22 |x s|
// and an fp32 product is three v_mfma_f32_32x32x16_f16 accumulated in fp32:
//     x.w = xh.wh + (xh.wl + xl.wh)  +  [xl.wl and the e-terms, each <= 2^-22 |x.w|: dropped]
// Products of two 11-bit numbers are exact in fp32.
#pragma once
#include "m3d_common.h"

namespace m3d {
namespace f16x2 {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// Slots of an operand-bound array: 32 non-negative floats that a producer's epilogue fills (atomicMax per workgroup, slot = block & 31),
// the largest is the bound.  m3d_conv3d_zw_slots() returns this constant.
constexpr int kBoundSlots = 32;

// The power of two s with bound * s in [2^14, 2^15), and its inverse, from the bound's exponent field (no host read of the bound).
// Why that binade: fp16's largest finite value is just under 2^16, so an operand whose largest magnitude is `bound` fits with a binade
// of headroom; fp16 has 30 binades, so values down to 2^-18 of the largest keep all 22 bits of the cut and smaller ones an absolute
// error of 2^-40 of the largest.
__device__ __forceinline__ void f16_scale_of(float bound, float& s, float& inv) {
  int f = 268 - (int)((__float_as_uint(bound) >> 23) & 255u);
  f = f < 2 ? 2 : (f > 252 ? 252 : f);
  s = __uint_as_float((unsigned)f << 23);
  inv = __uint_as_float((unsigned)(254 - f) << 23);
}

// accumulator register g of a 32 x 32 MFMA block -> row inside the block (+ 4 * (lane >> 5))
__device__ __host__ constexpr int acc_row(int g) { return (g & 3) + 8 * (g >> 2); }

// the cut: v is already scaled
__device__ __forceinline__ void cut(float v, _Float16& h, _Float16& l) {
  h = (_Float16)v;
  l = (_Float16)(v - (float)h);
}
// v = a s (exact), then the cut
__device__ __forceinline__ void cut(float a, float s, _Float16& h, _Float16& l) { cut(a * s, h, l); }
// into element u of a pair of fp16 vectors (f16x2, f16x8: an element of a vector type binds to no reference)
template <class V>
__device__ __forceinline__ void cut(float v, V& hh, V& ll, int u) {
  const _Float16 h = (_Float16)v;
  hh[u] = h; ll[u] = (_Float16)(v - (float)h);
}
// two scaled values at once, as the packed pairs the staging code stores
__device__ __forceinline__ void cut(float v0, float v1, f16x2& hh, f16x2& ll) {
  hh = f16x2{(_Float16)v0, (_Float16)v1};
  ll = f16x2{(_Float16)(v0 - (float)hh[0]), (_Float16)(v1 - (float)hh[1])};
}

__device__ __forceinline__ unsigned pack2(_Float16 a, _Float16 b) {
  return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
}

// the largest of the kBoundSlots slots, in every lane of the wave: lane i holds slot i & 31 on entry.  conv3d_zn.hip and upconv3d_f16.hip
// keep this loop open-coded: through the helper their main kernels come out with other address arithmetic (some 20 instructions
// fewer), and a change of their instruction stream is not a thing to get from a header
__device__ __forceinline__ float max_of_slot_lanes(float m) {
#pragma unroll
  for (int o = kBoundSlots / 2; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  return m;
}
__device__ __forceinline__ float bound_of_slots(const float* __restrict__ slots, int lane) {
  return max_of_slot_lanes(slots[lane & (kBoundSlots - 1)]);
}

// One fp32 product block: hh, hl, lh.  The f16 MFMA TRUNCATES when it adds its products into the accumulator, a bias of ~3e-9 of the
// running sum per MFMA that grows with the length of the chain.  Kernels whose operands can be of one sign (gradients times post-ReLU
// activations) therefore cap the run of MFMAs into one accumulator (384 in the weight-gradient kernels) and fold the partial sums with
// round-to-nearest fp32 adds; with signed weights the forward kernels run over all of K (5e-6 at 256 input channels).
__device__ __forceinline__ void mfma3(f16x8 ah, f16x8 al, f16x8 bh, f16x8 bl, f32x16& acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
}

}  // namespace f16x2
using f16x2::f16_scale_of;      // include/m3d.h and the tests' contract speak of m3d::f16_scale_of
}  // namespace m3d
