// Forward of the mask head's ConvTranspose3d(kernel 2, stride 2, padding 0) on the f16 matrix cores at fp32 accuracy, with two epilogues:
//   plain   y[r,co,2z+a,2y+b,2x+c]   = bias[co] + sum_ci x[r,ci,z,y,x] W[ci,co,a,b,c]  [ReLU]         (what m3d_upconv3d_2x_forward writes)
//   fused   out[r,k,2z+a,2y+b,2x+c]  = act(bc[k] + sum_co wc[k,co] max(y[r,co,2z+a,2y+b,2x+c], 0))    (upconv + ReLU + Mask_Outs.classify
//           [+ sigmoid]: the tail of mask_net in one launch - the [R, Cout, 2D, 2H, 2W] tensor is never written, there is no workspace)
// Operands as PyTorch stores them: x fp32 [R,Cin,D,H,W], W [Cin,Cout,2,2,2] (cut once by the pack call), wc [K,Cout], K <= 8.
//
// GEMM view (upconv3d.hip): out[n][col] = sum_ci W[ci][n] x[ci][col], n = 8 co + 4a + 2b + c, col = (r, v) over ALL RoIs (R V columns: a
// tile may span two RoIs, every column carries its own (r, v)).  The "f16x2" cut of conv3d_zn.hip: each operand times the power of two
// f16_scale_of(bound), cut into hi + lo fp16, three v_mfma_f32_32x32x16_f16 per fp32 product (lo hi, hi lo, hi hi), fp32 accumulation,
// un-scaled by an exact power of two.  x is cut while it is staged from the raw fp32 tensor; the bound is the largest of the 32 slots of
// d_in_max (what the conv before left, or one sweep).
//
// Decomposition: a workgroup (4 waves) owns 64 columns.  Its x tile is cut ONCE into LDS - [hi / lo][k step][k half][64 columns] 16-byte
// units, 256 bytes per input channel: 64 KB at Cin = 256 - and stays there while the workgroup walks every output channel: wave (a, b)
// takes the two parities c = 0, 1 of its (a, b) and both 32-column blocks, 32 output channels at a time (four 32 x 32 accumulators).  The
// weights are the ROW operand and the pack orders them [32-channel block][k step][parity][hi / lo][lane], so a 32 x 32 result holds 32
// channels of ONE parity in its registers and a voxel on the lane: the plain epilogue pairs the c = 0 / c = 1 accumulators into one
// 8-byte store (neighbouring lanes at neighbouring x), the fused epilogue sums over the channels inside the lane.  A weight fragment is
// one 16-byte load per lane out of the L2-resident pack (2 MB at 256 -> 256), requested one k step ahead; an x fragment is one
// ds_read_b128, 16 lanes on 16 consecutive units = one 256-byte bank row: no conflicts.  More than 256 input channels: the tile is
// re-staged in chunks of 256 channels inside every channel block (correct at any Cin % 16 == 0; the shipped head has 256).  Plain
// epilogue only: a launch with fewer column tiles than the chip has CUs (R < 48 on a 7^3 grid) cuts the channel blocks into 2, 4, ..
// slices along blockIdx.y, a function of the shape only; every element is computed exactly as without the cut.
//
// The classifier is fp32 FMA on the accumulator tile, in an order that depends on the shape only: per lane half h (rows 4h + {0..3} + 8i
// of a block) the channels in ascending order, blocks in ascending order, s = fma(wc, u, s) from s = 0; then s(h = 0) + s(h = 1) (one
// cross-lane exchange), then + bc[k], then the sigmoid of m3d_common.h (the formula m3d_conv3d_forward_split_sigmoid uses).
//
// No atomics, every output element written once by one lane, no scratch, bit-identical run to run.  ReLU is `v < 0 ? 0 : v`: a NaN goes
// through (an Inf / NaN operand gives NaN on every output of its column, or of its channel for a weight).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):     VGPRs   AGPRs   SGPRs   scratch   LDS (Cin >= 256)   workgroups / CU
//   upconv_f16_kernel<false> (plain)                                   171       0      60         0   65 536 (dynamic)                 2
//   upconv_f16_kernel<true>  (fused)                                   211       0      90         0   65 536 (dynamic)                 2
//
// The two constants of the accuracy contract (tests/upconv_f16_cases.py), from this code:
//   n_acc = 3 Cin / 16: one accumulator takes every k step's three MFMAs (a re-staged chunk continues the same accumulator); the only
//       fp32 operation after them is the LAST one, fma(acc, 1 / (s_x s_w), bias) - one rounding, the bound's 2^-24 |y| term;
//       c1 = 3.01: neither operand is rounded to fp32 before the cut;
//   m = Cout + 2: Cout products / adds of the classifier sum in any order, + 1 for the bias add, + 1 for the one partial sum the fixed
//       order adds (the two lane halves).
#include <initializer_list>

#include "f16x2.h"

namespace {

using namespace m3d::f16x2;      // the cut, its vector types and the bound slots: f16x2.h

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int UF_NT = 256;
constexpr int UF_VT = 64;                         // columns of a workgroup
constexpr int UF_KC = 256;                        // input channels of one staged chunk
constexpr int UF_STEP_UNITS = 8 * 2 * 64;         // packed weights of one (channel block, k step): [parity 8][hi / lo][lane 64] 16-byte units
constexpr int UF_MAXK = 8;
constexpr unsigned UF_CUS = 256;                  // below this many column tiles the plain epilogue cuts the channel blocks into slices

// packed[channel block 32][k step = ci / 16][parity p = 4a + 2b + c][hi / lo][lane] <- weight [Cin][Cout][2][2][2] fp32: lane (row = l % 32,
// half = l / 32) holds W[ci = 16 step + 8 half + j][co = 32 block + row][p], j = 0..7; rows beyond Cout are zero
__global__ __launch_bounds__(256) void upconv_f16_pack_kernel(const float* __restrict__ w, int cin, int cout, u32x4* __restrict__ packed,
                                                              const float* __restrict__ wamax) {
  float sw, inv;
  f16_scale_of(*wamax, sw, inv);
  const int steps = cin / 16, ncb = (cout + 31) / 32;
  const long long total = (long long)ncb * steps * 8 * 64;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int lane = (int)(e & 63), p = (int)((e >> 6) & 7);
    const long long r = e >> 9;
    const int ks = (int)(r % steps), cb = (int)(r / steps);
    const int co = cb * 32 + (lane & 31), kh = lane >> 5;
    u32x4 ph, pl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f16x2 hh, ll;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float v = 0.f;
        if (co < cout) v = w[((size_t)(ks * 16 + 8 * kh + 2 * j + u) * cout + co) * 8 + p] * sw;
        cut(v, hh, ll, u);
      }
      ph[j] = __builtin_bit_cast(unsigned, hh); pl[j] = __builtin_bit_cast(unsigned, ll);
    }
    u32x4* dst = packed + ((size_t)(cb * steps + ks) * 8 + p) * 128 + lane;
    dst[0] = ph; dst[64] = pl;
  }
}

struct UfArgs {
  const float* x; const u32x4* wp; const float* bias; const float* wc; const float* bc; float* out;
  const float* in_max; const float* wamax;
  int Cin, Cout, K, H, W, V, relu, sigmoid;
  long long cols;                                  // R V
};

template <bool FUSED>
__global__ __launch_bounds__(UF_NT, 2) void upconv_f16_kernel(UfArgs a) {
  extern __shared__ u32x4 uf_lds[];                // [hi / lo][k step of the chunk][k half][64 columns]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int steps = a.Cin / 16, ncb = (a.Cout + 31) / 32;
  const bool multi = a.Cin > UF_KC;                // more channels than one staged chunk holds
  const int lo_base = (multi ? UF_KC / 16 : steps) * 2 * UF_VT;
  const size_t V = (size_t)a.V;

  // ---- operand scales (powers of two): the input's bound = the largest slot, the weights' as packed
  float xs, inv_x, inv_w;
  {
    float im = a.in_max[lane & (kBoundSlots - 1)];      // max_of_slot_lanes of f16x2.h, open-coded: see there
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) im = fmaxf(im, __shfl_xor(im, o));
    float sw_;
    f16_scale_of(im, xs, inv_x);
    f16_scale_of(*a.wamax, sw_, inv_w);
  }
  const float un = inv_x * inv_w;

  // ---- staging: thread = (column tid % 64, 8-channel groups tid / 64 + 4 q); a column beyond the end re-reads the last one (never stored)
  const long long col0 = (long long)blockIdx.x * UF_VT;
  const int sc = tid & 63, sg = tid >> 6;
  const float* sx;
  {
    long long c = col0 + sc;
    c = c < a.cols ? c : a.cols - 1;
    const long long r = c / a.V;
    sx = a.x + (size_t)r * a.Cin * V + (size_t)(c - r * a.V);
  }
  auto stage = [&](int c0, int nch) __attribute__((always_inline)) {
    const int groups = nch / 8;
#pragma unroll 2
    for (int gq = sg; gq < groups; gq += 4) {
      float raw[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[j] = sx[(size_t)(c0 + 8 * gq + j) * V];
      u32x4 ph, pl;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f16x2 hh, ll;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float v = raw[2 * j + e] * xs;
          cut(v, hh, ll, e);
        }
        ph[j] = __builtin_bit_cast(unsigned, hh); pl[j] = __builtin_bit_cast(unsigned, ll);
      }
      uf_lds[gq * UF_VT + sc] = ph;                // gq = 2 (k step) + k half
      uf_lds[lo_base + gq * UF_VT + sc] = pl;
    }
  };

  // ---- output columns of this lane: block j holds column col0 + 32 j + lane % 32
  const int fr = lane & 31, fh = lane >> 5;
  const int pa = wave >> 1, pb = wave & 1;
  const int W2 = 2 * a.W;
  bool ok[2];
  size_t orow[2];                                  // r of the column; the channel part is added per output
  int ovox[2];                                     // offset of (2z + a, 2y + b, 2x) inside one [2D,2H,2W] channel
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long c = col0 + 32 * j + fr;
    ok[j] = c < a.cols;
    const long long cc = ok[j] ? c : 0;
    const long long r = cc / a.V;
    const int v = (int)(cc - r * a.V);
    const int x = v % a.W, zy = v / a.W, y = zy % a.H, z = zy / a.H;
    orow[j] = (size_t)r;
    ovox[j] = ((2 * z + pa) * (2 * a.H) + 2 * y + pb) * W2 + 2 * x;
  }

  // ---- weight fragments: [c][hi / lo] of step t = block * steps + k step, requested one step ahead
  const u32x4* const wsrc = a.wp + (4 * pa + 2 * pb) * 128 + lane;
  const int T = ncb * steps;
  f16x8 A0[2][2], A1[2][2];
  auto fetch_a = [&](f16x8 (&A)[2][2], int t) __attribute__((always_inline)) {
    const u32x4* p = wsrc + (size_t)(t < T ? t : T - 1) * UF_STEP_UNITS;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) A[c][hl] = __builtin_bit_cast(f16x8, p[c * 128 + hl * 64]);
  };

  f32x16 acc[2][2];                                // [column block][c]
  float s[UF_MAXK][2][2];                          // fused: the classifier sums of this lane half
#pragma unroll
  for (int k = 0; k < UF_MAXK; ++k)
#pragma unroll
    for (int j = 0; j < 2; ++j) { s[k][j][0] = 0.f; s[k][j][1] = 0.f; }

  auto step = [&](f16x8 (&Ac)[2][2], f16x8 (&An)[2][2], int t, int ks) __attribute__((always_inline)) {
    if (multi && (ks & (UF_KC / 16 - 1)) == 0) {   // workgroup-uniform: every wave walks the same (block, k step) sequence
      __syncthreads();                             // every wave has read the chunk before
      const int c0 = ks * 16;
      stage(c0, a.Cin - c0 < UF_KC ? a.Cin - c0 : UF_KC);
      __syncthreads();
    }
    fetch_a(An, t + 1);
    const int kl = multi ? (ks & (UF_KC / 16 - 1)) : ks;
    f16x8 Bf[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int hl = 0; hl < 2; ++hl) Bf[j][hl] = __builtin_bit_cast(f16x8, uf_lds[hl * lo_base + (kl * 2 + fh) * UF_VT + 32 * j + fr]);
    constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};                     // small products first: (lo, hi) (hi, lo) (hi, hi)
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[j][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ac[c][PA[q]], Bf[j][PB[q]], acc[j][c], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);             // a step is one scheduling region: the weight requests stay one step ahead
  };

  // the channel blocks of this workgroup: all of them, or - plain epilogue, a launch that leaves CUs idle - the slice blockIdx.y
  const int cb_lo = (int)((long long)blockIdx.y * ncb / gridDim.y), cb_hi = (int)((long long)(blockIdx.y + 1) * ncb / gridDim.y);
  int t = cb_lo * steps;
  fetch_a(A0, t);
  if (!multi) {
    stage(0, a.Cin);
    __syncthreads();
  }

#pragma unroll 1
  for (int cb = cb_lo; cb < cb_hi; ++cb) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[j][c][g] = 0.f;
    int ks = 0;
#pragma unroll 1
    for (; ks + 1 < steps; ks += 2, t += 2) {
      step(A0, A1, t, ks);
      step(A1, A0, t + 1, ks + 1);
    }
    if (ks < steps) {                              // an odd step count: the next block's first fragments are in A1 - move them where it reads
      step(A0, A1, t, ks);
      ++t;
#pragma unroll
      for (int c = 0; c < 2; ++c) { A0[c][0] = A1[c][0]; A0[c][1] = A1[c][1]; }
    }

    // ---- epilogue of the block: register g = channel 32 cb + 4 fh + acc_row(g), lane = one column of each block
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int co = cb * 32 + 4 * fh + acc_row(g);
      if (co >= a.Cout) continue;
      const float bv = a.bias ? a.bias[co] : 0.f;
      float u[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          float v = fmaf(acc[j][c][g], un, bv);    // (un: a power of two - the one rounding is the add's)
          if (FUSED || a.relu) v = v < 0.f ? 0.f : v;
          u[j][c] = v;
        }
      if constexpr (FUSED) {
#pragma unroll
        for (int k = 0; k < UF_MAXK; ++k) {
          if (k >= a.K) break;
          const float wk = a.wc[(size_t)k * a.Cout + co];
#pragma unroll
          for (int j = 0; j < 2; ++j) { s[k][j][0] = fmaf(wk, u[j][0], s[k][j][0]); s[k][j][1] = fmaf(wk, u[j][1], s[k][j][1]); }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (ok[j]) {
            const f32x2 o = {u[j][0], u[j][1]};
            *reinterpret_cast<f32x2*>(a.out + (orow[j] * a.Cout + co) * 8 * V + ovox[j]) = o;
          }
      }
    }
  }

  if constexpr (FUSED) {
    // the two lane halves hold the two halves of every channel block: s(h = 0) + s(h = 1) (commutative: both halves get the same bits),
    // then half h stores column block h
#pragma unroll
    for (int k = 0; k < UF_MAXK; ++k) {
      if (k >= a.K) break;
      float tsum[2][2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int c = 0; c < 2; ++c) tsum[j][c] = s[k][j][c] + __shfl_xor(s[k][j][c], 32);
      const float bk = a.bc ? a.bc[k] : 0.f;
      f32x2 o = {(fh ? tsum[1][0] : tsum[0][0]) + bk, (fh ? tsum[1][1] : tsum[0][1]) + bk};
      if (a.sigmoid) { o[0] = m3d::sigmoid_f32(o[0]); o[1] = m3d::sigmoid_f32(o[1]); }
      const bool okh = fh ? ok[1] : ok[0];
      const size_t rr = fh ? orow[1] : orow[0];
      const int vv = fh ? ovox[1] : ovox[0];
      if (okh) *reinterpret_cast<f32x2*>(a.out + (rr * a.K + k) * 8 * V + vv) = o;
    }
  }
}

inline size_t uf_plane_bytes(int cin, int cout) { return (size_t)((cout + 31) / 32) * (cin / 16) * UF_STEP_UNITS * 16; }

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// product >= 2^31 (every factor is a positive int)
bool too_big(std::initializer_list<int> f) {
  long long p = 1;
  for (int v : f) {
    p *= v;
    if (p >= (1ll << 31)) return true;
  }
  return false;
}

bool bad_dims(int R, int Cin, int Cout, int D, int H, int W) { return R < 0 || Cin < 1 || Cout < 1 || D < 1 || H < 1 || W < 1; }

bool pack_ok(int Cin, int Cout) {
  return Cin >= 16 && Cin % 16 == 0 && Cout >= 1 && Cout <= (1 << 26) && !too_big({Cin, (Cout + 31) / 32 * 32, 8});
}

// every refusal of a launch, then the launch
int uf_launch(const char* what, bool fused, const float* d_x, const void* d_packed, const float* d_bias, const float* d_wc, const float* d_bc,
              float* d_out, int R, int Cin, int Cout, int K, int D, int H, int W, int relu, int sigmoid, const float* d_in_max, void* stream) {
  if (bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (R == 0) return M3D_OK;                                       // nothing to write: no pointer is looked at
  if (fused && (K < 1 || K > UF_MAXK)) return M3D_EUNSUPPORTED;
  if (!m3d_upconv3d_2x_f16x2_supported(R, Cin, Cout, D, H, W)) return M3D_EUNSUPPORTED;
  if (fused && too_big({R, K, 8, D, H, W})) return M3D_EUNSUPPORTED;
  if (!d_x || !d_packed || !d_out || !d_in_max || (fused && !d_wc)) return M3D_EINVAL;
  if (misaligned(d_x, 3) || misaligned(d_bias, 3) || misaligned(d_wc, 3) || misaligned(d_bc, 3) || misaligned(d_out, 3) ||
      misaligned(d_in_max, 3))
    return M3D_EINVAL;
  if (misaligned(d_packed, 15) || misaligned(d_out, 7)) return M3D_EUNSUPPORTED;
  UfArgs a{};
  a.x = d_x; a.wp = static_cast<const u32x4*>(d_packed); a.bias = d_bias; a.wc = d_wc; a.bc = d_bc; a.out = d_out; a.in_max = d_in_max;
  a.wamax = reinterpret_cast<const float*>(static_cast<const char*>(d_packed) + uf_plane_bytes(Cin, Cout));
  a.Cin = Cin; a.Cout = Cout; a.K = K; a.H = H; a.W = W; a.V = D * H * W; a.relu = relu ? 1 : 0; a.sigmoid = sigmoid ? 1 : 0;
  a.cols = (long long)R * a.V;
  const unsigned blocks = (unsigned)((a.cols + UF_VT - 1) / UF_VT);
  const int lds = (Cin < UF_KC ? Cin : UF_KC) * 4 * UF_VT;          // hi + lo fp16 of 64 columns per channel
  if (fused) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(upconv_f16_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(upconv_f16_kernel<true>, dim3(blocks), dim3(UF_NT), lds, m3d::as_stream(stream), a);
  } else {
    // fewer column tiles than CUs: the channel blocks are cut into 2, 4, .. slices (a function of the shape only) until the launch has
    // 256 workgroups or a slice is one block.  A slice stages the x tile again and computes its channels exactly as the whole walk does:
    // the same bits.  The fused epilogue sums over all channels inside one workgroup and never splits.
    unsigned slices = 1;
    while ((unsigned long long)blocks * slices < UF_CUS && 2 * slices <= (unsigned)((Cout + 31) / 32)) slices *= 2;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(upconv_f16_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(upconv_f16_kernel<false>, dim3(blocks, slices), dim3(UF_NT), lds, m3d::as_stream(stream), a);
  }
  return m3d::check_launch(what);
}

}  // namespace

M3D_API int m3d_upconv3d_2x_f16x2_supported(int R, int Cin, int Cout, int D, int H, int W) {
  if (bad_dims(R, Cin, Cout, D, H, W) || !pack_ok(Cin, Cout)) return 0;
  if (too_big({8, D, H, W})) return 0;
  if (R > 0 && (too_big({R, Cin, D, H, W}) || too_big({R, Cout, 8, D, H, W}))) return 0;
  return 1;
}

M3D_API size_t m3d_upconv3d_2x_f16x2_packed_bytes(int Cin, int Cout) {
  if (!pack_ok(Cin, Cout)) return 0;
  return uf_plane_bytes(Cin, Cout) + 256;            // + the weight's largest magnitude (one float) behind the fragments
}

M3D_API int m3d_upconv3d_2x_f16x2_pack(const float* d_weight, int Cin, int Cout, void* d_packed, void* stream) {
  if (Cin < 1 || Cout < 1) return M3D_EINVAL;
  if (!pack_ok(Cin, Cout)) return M3D_EUNSUPPORTED;
  if (!d_weight || !d_packed || misaligned(d_weight, 3)) return M3D_EINVAL;
  if (misaligned(d_packed, 15)) return M3D_EUNSUPPORTED;
  float* wamax = reinterpret_cast<float*>(static_cast<char*>(d_packed) + uf_plane_bytes(Cin, Cout));
  if (const int rc = m3d_absmax(d_weight, (long long)Cin * Cout * 8, wamax, stream)) return rc;
  hipLaunchKernelGGL(upconv_f16_pack_kernel, dim3(1024), dim3(256), 0, m3d::as_stream(stream), d_weight, Cin, Cout, (u32x4*)d_packed,
                     (const float*)wamax);
  return m3d::check_launch("upconv3d_2x_f16x2_pack");
}

M3D_API int m3d_upconv3d_2x_forward_f16x2(const float* d_x, const void* d_packed, const float* d_bias, float* d_y, int R, int Cin, int Cout,
                                          int D, int H, int W, int relu, const float* d_in_max, void* stream) {
  return uf_launch("upconv3d_2x_forward_f16x2", false, d_x, d_packed, d_bias, nullptr, nullptr, d_y, R, Cin, Cout, 0, D, H, W, relu, 0,
                   d_in_max, stream);
}

M3D_API int m3d_mask_tail_f16x2(const float* d_x, const void* d_packed, const float* d_up_bias, const float* d_cls_weight,
                                const float* d_cls_bias, float* d_out, int R, int Cin, int Cout, int K, int D, int H, int W, int sigmoid,
                                const float* d_in_max, void* stream) {
  return uf_launch("mask_tail_f16x2", true, d_x, d_packed, d_up_bias, d_cls_weight, d_cls_bias, d_out, R, Cin, Cout, K, D, H, W, 1, sigmoid,
                   d_in_max, stream);
}
