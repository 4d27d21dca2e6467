// Backward of the box head's fully-connected layers as fp32 MFMA GEMMs for gfx950, on the operands as PyTorch stores them:
//     dgrad   gx[M,K] = gy[M,N] . W[N,K]           (reduction over N)
//     wgrad   gw[N,K] = gy[M,N]^T . x[M,K]         (reduction over M),   gb[N] = sum_m gy[m,n] out of the same launch
//
// What it replaces: the autograd of nn.Linear at lib/modeling/fast_rcnn_heads.py:84-85,114-117 (fc1: K = C*7^3 = 87 808, N = 1024: a
// 360 MB weight; fc2) and :15-19,42-45 (cls_score, bbox_pred) - two cuBLAS SGEMMs and a column sum per layer.  No transposed copy of
// any operand is made: the 360 MB matrix is read once by dgrad, and its gradient written once by wgrad.
//
// Roofline: MFMA-bound (v_mfma_f32_32x32x2_f32, 157.3 TFLOP/s): 2*M*N*K FLOP per GEMM against (N + M) K 4 bytes moved once - at fc1,
// 23.0 GFLOP = 0.15 ms against 0.065 ms (M = 128) / 0.036 ms (M = 256) of bytes at 6.3 TB/s.
// Design (one template, one flag):
//  * the output is [rows, K] in both GEMMs (rows = M / N) and its column index k is the contiguous index of the big operand B (W / x),
//    whose row index IS the reduction index ("reduction-major").  Such an operand needs no transposition and no LDS padding: for
//    32x32x2 lane l (j = l & 31, h = l >> 5) takes B[r(h)][j] - one ds_read_b32 out of one LDS row, consecutive lanes at consecutive
//    addresses (the two half-waves are separate bank groups for ds_read_b32: conflict-free).  Global -> LDS stays 16-byte quads along k;
//  * the small operand is gy in both: reduction-contiguous in dgrad (staged as the forward stages x: rows padded to 36 floats,
//    ds_read_b128 fragments, lane half h holds the reduction indices 4h..4h+3 of an 8-deep group - the B reads use the same
//    permutation), reduction-major in wgrad (staged and read exactly like B).  gy may have any M, N >= 1 and 4-byte alignment: where a row
//    or the base is not a 16-byte multiple (cls_score N = 2, bbox_pred N = 12) it is loaded element by element;
//  * workgroup tile 128 x 128 x 32, 4 waves as 2 x 2, each 64 x 64 = 2 x 2 MFMA blocks, two workgroups per CU; double-buffered LDS,
//    one barrier per chunk, the next chunk's global loads issued before the chunk's 64 MFMAs per wave (as fc_gemm.hip);
//  * reduction rows beyond the end enter the sum, so the ragged last chunk is ZERO-FILLED in LDS (never clamped); output rows / columns
//    beyond the end are clamped at the load and masked at the store;
//  * where the output has fewer than 512 tiles (the machine's resident workgroups) the reduction is cut into `slices` (<= 64, a function
//    of the shape only); partials go to the caller's workspace and a second kernel adds them in slice order: bit-identical run to run;
//  * unit order: blockIdx % 8 is the XCD; one XCD gets a contiguous run of units, and inside a column tile the row tiles are
//    neighbours - the N/128 wgrad tiles that share an x panel (the M/128 dgrad tiles that share a W panel) meet in one L2;
//  * gb: the workgroups of the first column tile sum their staged gy tile column by column (row order, one thread per column, no
//    atomics); with a split reduction the per-slice sums travel through the workspace like the partials.
// These kernels stay on the fp32-input MFMA and stay the default.  The same two GEMMs on the f16 matrix cores (the f16x2 cut on the raw
// operands, opt-in, 1.8 x - 2.2 x faster at the fc1 shapes and slower at fc2) are fc_backward_f16.hip: DESIGN.md, "Box-head backward on
// the f16 pipe".
#include "f16x2.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BT = 128, BR = 32, LSA = BR + 4;                     // tile edge, reduction chunk, padded row stride of dgrad's gy tile
constexpr int kBFloats = BR * BT;                                  // the reduction-major tile: [32 reduction rows][128]
constexpr int kSlots = 512;                                        // resident workgroups: 256 CUs x 2
using m3d::f16x2::acc_row;      // accumulator register g -> row inside a 32x32 block (+4*(lane>>5))

struct FcbArgs {
  const float* gy; const float* b; float* out; float* part; float* gb; float* gb_part;
  int M, N, K;
  int rows, red;          // output rows and reduction length: (M, N) in dgrad, (N, M) in wgrad
  int rt, kt, slices, chunks, per_xcd;
  int gy_vec;             // gy rows and base are 16-byte multiples: quads; else element loads
};

template <bool WGRAD>
__global__ __launch_bounds__(256, 2) void fc_backward_kernel(FcbArgs a) {
  constexpr int kAFloats = WGRAD ? BR * BT : BT * LSA;
  constexpr int kStage = kAFloats + kBFloats;
  extern __shared__ float lds[];                                   // 2 x [A tile][B tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int tiles = a.rt * a.kt, u = xcd * a.per_xcd + idx;
  if (idx >= a.per_xcd || u >= tiles * a.slices) return;
  const int slice = u / tiles, tile = u - slice * tiles;
  const int tk = tile / a.rt, tr = tile - tk * a.rt;               // row tiles of one column panel are neighbours
  const int r0 = tr * BT, k0 = tk * BT;
  const int c0 = (int)((long long)slice * a.chunks / a.slices), c1 = (int)((long long)(slice + 1) * a.chunks / a.slices);
  const int full = a.red / BR;                                     // whole chunks of the reduction
  const int c1f = min(c1, full);
  const size_t N = (size_t)a.N, K = (size_t)a.K;

  // ---- staging.  Reduction-major tiles: thread -> (row = tid/32 + 8 i, quad = tid%32), i = 0..3: a half-wave moves 512 contiguous
  // bytes.  dgrad's gy tile: thread -> (row = tid/8 + 32 i, quad = tid%8) as in the forward.
  const int bq = tid & 31, brow = tid >> 5;
  const float* pb = a.b + min(k0 + 4 * bq, a.K - 4);               // column clamped: masked at the store
  const int aq = WGRAD ? bq : (tid & 7), arow = WGRAD ? brow : (tid >> 3);
  int acol[4];                                                     // wgrad: the four gy columns of this thread, clamped one by one
#pragma unroll
  for (int e = 0; e < 4; ++e) acol[e] = a.gy_vec ? min(r0 + 4 * aq, a.N - 4) + e : min(r0 + 4 * aq + e, a.N - 1);
  size_t arowoff[4];                                               // dgrad: gy row offsets of this thread (row clamped: masked at the store)
#pragma unroll
  for (int i = 0; i < 4; ++i) arowoff[i] = (size_t)min(r0 + arow + 32 * i, a.M - 1) * N + 4 * aq;

  // whole chunks only: no predicate, nothing touches the loaded registers until commit() after the MFMA loop
  f32x4 sa[4], sb[4];
  auto fetch = [&](int c) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sb[i] = *reinterpret_cast<const f32x4*>(pb + (size_t)(c * BR + brow + 8 * i) * K);
      if constexpr (WGRAD) {
        const float* p = a.gy + (size_t)(c * BR + arow + 8 * i) * N;
        if (a.gy_vec) sa[i] = *reinterpret_cast<const f32x4*>(p + acol[0]);
        else { sa[i][0] = p[acol[0]]; sa[i][1] = p[acol[1]]; sa[i][2] = p[acol[2]]; sa[i][3] = p[acol[3]]; }
      } else {
        const float* p = a.gy + arowoff[i] + c * BR;
        if (a.gy_vec) sa[i] = *reinterpret_cast<const f32x4*>(p);
        else { sa[i][0] = p[0]; sa[i][1] = p[1]; sa[i][2] = p[2]; sa[i][3] = p[3]; }
      }
    }
  };
  auto commit = [&](float* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (WGRAD) *reinterpret_cast<f32x4*>(buf + (arow + 8 * i) * BT + 4 * aq) = sa[i];
      else *reinterpret_cast<f32x4*>(buf + (arow + 32 * i) * LSA + 4 * aq) = sa[i];
      *reinterpret_cast<f32x4*>(buf + kAFloats + (brow + 8 * i) * BT + 4 * bq) = sb[i];
    }
  };
  // the ragged last chunk: every reduction index beyond the end is zero in LDS
  auto fetch_tail = [&]() __attribute__((always_inline)) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = full * BR + brow + 8 * i;
      sb[i] = z;
      if (r < a.red) sb[i] = *reinterpret_cast<const f32x4*>(pb + (size_t)r * K);
      sa[i] = z;
      if constexpr (WGRAD) {
        const int m = full * BR + arow + 8 * i;
        if (m < a.M) {
          const float* p = a.gy + (size_t)m * N;
          sa[i][0] = p[acol[0]]; sa[i][1] = p[acol[1]]; sa[i][2] = p[acol[2]]; sa[i][3] = p[acol[3]];
        }
      } else {
        const float* p = a.gy + arowoff[i] + full * BR;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (full * BR + 4 * aq + e < a.N) sa[i][e] = p[e];
      }
    }
  };

  // ---- fragments: wave (wm, wn) owns rows [wm*64, +64) x cols [wn*64, +64); in the 8-deep group g lane half h holds the reduction
  // indices 8g + 4h + kk, kk = 0..3, on both operands
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 31, fh = lane >> 5;
  const int offB = kAFloats + 4 * fh * BT + wn * 64 + fr;
  const int offA = WGRAD ? 4 * fh * BT + wm * 64 + fr : (wm * 64 + fr) * LSA + 4 * fh;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
  const bool own_gb = WGRAD && a.gb != nullptr && tk == 0 && tid < BT;   // waves 0 and 1 of the first column tile: one gy column each
  float gbsum = 0.f;

  auto compute = [&](const float* cur) __attribute__((always_inline)) {
    if constexpr (WGRAD) {
      if (own_gb) {
#pragma unroll 8
        for (int r = 0; r < BR; ++r) gbsum += cur[r * BT + tid];
      }
    }
#pragma unroll
    for (int g = 0; g < BR / 8; ++g) {
      f32x4 fa[2];
      if constexpr (!WGRAD) {
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const f32x4*>(cur + offA + i * 32 * LSA + g * 8);
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int ro = (8 * g + kk) * BT;
        float va[2], vb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if constexpr (WGRAD) va[i] = cur[offA + ro + i * 32];
          else va[i] = fa[i][kk];
          vb[i] = cur[offB + ro + i * 32];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[i], vb[j], acc[i][j], 0, 0, 0);
      }
    }
  };

  if (c0 < c1f) { fetch(c0); commit(lds); }
  __syncthreads();
  for (int c = c0; c < c1f; ++c) {
    const float* cur = lds + ((c - c0) & 1) * kStage;
    fetch(c + 1 < c1f ? c + 1 : c);                               // last chunk: harmless re-fetch instead of a branch around the loads
    __builtin_amdgcn_sched_barrier(0);                            // keep the loads in front of the MFMAs
    compute(cur);
    commit(lds + ((c + 1 - c0) & 1) * kStage);
    __syncthreads();
  }
  if (c1 > c1f) {                                                 // only the last slice, only if red % 32 != 0
    fetch_tail();
    commit(lds);                                                  // buffer 0: the loop's last barrier is behind every read of it
    __syncthreads();
    compute(lds);
  }

  // ---- epilogue: register g of block (i, j) is out[r0 + wm*64 + i*32 + acc_row(g) + 4*fh][k0 + wn*64 + j*32 + fr]: for a fixed g the
  // half-wave writes one 128-byte row segment
  const bool direct = a.slices == 1;
  float* dst = direct ? a.out : a.part + (size_t)slice * a.rows * K;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + wn * 64 + j * 32 + fr;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rb = r0 + wm * 64 + i * 32 + 4 * fh;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int r = rb + acc_row(g);
        if (r < a.rows && k < a.K) dst[(size_t)r * K + k] = acc[i][j][g];
      }
    }
  }
  if constexpr (WGRAD) {
    if (own_gb && r0 + tid < a.N) (direct ? a.gb : a.gb_part + (size_t)slice * N)[r0 + tid] = gbsum;
  }
}

// out[e] = sum_s part[s][e] and gb[n] = sum_s gb_part[s][n], slices added in index order.  One thread = four consecutive outputs
// (K % 4 == 0, 16-byte aligned), every slice's quad one 16-byte load.
__global__ __launch_bounds__(256) void fc_backward_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, long long total,
                                                                 int slices, const float* __restrict__ gb_part,
                                                                 float* __restrict__ gb, int N) {
  const long long Q = total >> 2;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < Q; q += (long long)gridDim.x * 256) {
    const long long e = q << 2;
    f32x4 v = *reinterpret_cast<const f32x4*>(part + e);
    for (int s = 1; s < slices; ++s) v += *reinterpret_cast<const f32x4*>(part + (size_t)s * total + e);
    *reinterpret_cast<f32x4*>(out + e) = v;
  }
  if (gb)
    for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
      float v = gb_part[n];
      for (int s = 1; s < slices; ++s) v += gb_part[(size_t)s * N + n];
      gb[n] = v;
    }
}

struct BPlan { int rt, kt, chunks, slices, per_xcd; };

// The split is a function of the shape only: an output with fewer tiles than the machine has workgroup slots cuts its reduction so
// that the units fill them once - never more than 64 slices, and (the forward's rule) about four chunks or more per slice, so that a
// unit's partial tile (64 KB written, read again by the reduce kernel) stays small beside its MFMA work.
BPlan make_plan(int rows, int red, int K) {
  BPlan p;
  p.rt = (rows + BT - 1) / BT; p.kt = (K + BT - 1) / BT; p.chunks = (red + BR - 1) / BR;
  const long long tiles = (long long)p.rt * p.kt;
  int s = tiles >= kSlots ? 1 : (int)(kSlots / tiles);
  s = s > 64 ? 64 : s;
  s = s > p.chunks / 4 + 1 ? p.chunks / 4 + 1 : s;
  p.slices = s < 1 ? 1 : s;
  p.per_xcd = (int)((tiles * p.slices + 7) / 8);
  return p;
}

size_t dgrad_need(int M, int N, int K) {
  const BPlan p = make_plan(M, N, K);
  return p.slices > 1 ? (size_t)p.slices * M * K * sizeof(float) : 0;
}

bool too_big(long long a, long long b) { return a * b >= (1ll << 31); }
bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

template <bool WGRAD>
int launch(const FcbArgs& a, const BPlan& p, hipStream_t st) {
  const size_t lds = sizeof(float) * 2 * ((WGRAD ? BR * BT : BT * LSA) + kBFloats);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(fc_backward_kernel<WGRAD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(fc_backward_kernel<WGRAD>, dim3(8 * p.per_xcd), dim3(256), lds, st, a);
  if (p.slices > 1) {
    const long long total = (long long)a.rows * a.K;
    long long blocks = (total / 4 + 255) / 256;
    blocks = blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(fc_backward_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)a.part, a.out, total, p.slices,
                       (const float*)a.gb_part, a.gb, a.N);
  }
  return m3d::check_launch(WGRAD ? "linear_wgrad" : "linear_dgrad");
}

}  // namespace

// Non-decreasing in M: a larger M can have more row tiles and therefore FEWER slices, so the size asked for is the largest need of any
// row count up to M (one candidate per row-tile count: its largest M).
M3D_API size_t m3d_linear_dgrad_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  size_t need = 0;
  const int rt = (M + BT - 1) / BT, kt = (K + BT - 1) / BT;
  for (int t = 1; t <= rt && (long long)t * kt < kSlots; ++t) {
    const long long mx = (long long)t * BT;
    const size_t n = dgrad_need(mx < M ? (int)mx : M, N, K);
    need = n > need ? n : need;
  }
  return m3d::align_up(need, 16);
}

M3D_API int m3d_linear_dgrad(const float* d_gy, const float* d_weight, float* d_gx, int M, int N, int K, void* d_ws, size_t ws_bytes,
                             void* stream) {
  if (M < 0 || N < 1 || K < 1) return M3D_EINVAL;
  if (M == 0) return M3D_OK;                                       // nothing to write: no pointer is looked at
  if (!d_gy || !d_weight || !d_gx) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_weight, 3) || misaligned(d_gx, 3) || misaligned(d_ws, 3)) return M3D_EINVAL;
  if (K % 4 != 0 || misaligned(d_weight, 15) || misaligned(d_gx, 15)) return M3D_EUNSUPPORTED;
  if (too_big(M, N) || too_big(N, K) || too_big(M, K)) return M3D_EUNSUPPORTED;
  const size_t asked = m3d_linear_dgrad_workspace_bytes(M, N, K);
  if (asked && (!d_ws || ws_bytes < asked)) return M3D_EINVAL;
  if (asked && misaligned(d_ws, 15)) return M3D_EUNSUPPORTED;
  const BPlan p = make_plan(M, N, K);
  FcbArgs a{d_gy, d_weight, d_gx, (float*)d_ws, nullptr, nullptr, M, N, K, M, N, p.rt, p.kt, p.slices, p.chunks, p.per_xcd,
            (N % 4 == 0 && !misaligned(d_gy, 15)) ? 1 : 0};
  return launch<false>(a, p, m3d::as_stream(stream));
}

M3D_API size_t m3d_linear_wgrad_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  const BPlan p = make_plan(N, M, K);                              // the tiles do not depend on M; the slices grow with it
  return p.slices > 1 ? m3d::align_up((size_t)p.slices * ((size_t)N * K + N) * sizeof(float), 16) : 0;
}

M3D_API int m3d_linear_wgrad(const float* d_gy, const float* d_x, float* d_gw, float* d_gb, int M, int N, int K, void* d_ws,
                             size_t ws_bytes, void* stream) {
  if (M < 0 || N < 1 || K < 1) return M3D_EINVAL;
  if (!d_gw || (M > 0 && (!d_gy || !d_x))) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_x, 3) || misaligned(d_gw, 3) || misaligned(d_gb, 3) || misaligned(d_ws, 3)) return M3D_EINVAL;
  if (K % 4 != 0 || misaligned(d_x, 15) || misaligned(d_gw, 15)) return M3D_EUNSUPPORTED;
  if (too_big(M, N) || too_big(N, K) || too_big(M, K)) return M3D_EUNSUPPORTED;
  hipStream_t st = m3d::as_stream(stream);
  if (M == 0) {                                                    // an empty batch: torch's gradients are zeros
    if (hipMemsetAsync(d_gw, 0, (size_t)N * K * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    if (d_gb && hipMemsetAsync(d_gb, 0, (size_t)N * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    return M3D_OK;
  }
  const size_t asked = m3d_linear_wgrad_workspace_bytes(M, N, K);
  if (asked && (!d_ws || ws_bytes < asked)) return M3D_EINVAL;
  if (asked && misaligned(d_ws, 15)) return M3D_EUNSUPPORTED;
  const BPlan p = make_plan(N, M, K);
  float* part = (float*)d_ws;
  FcbArgs a{d_gy, d_x, d_gw, part, d_gb, part ? part + (size_t)p.slices * N * K : nullptr, M, N, K, N, M, p.rt, p.kt, p.slices, p.chunks,
            p.per_xcd, (N % 4 == 0 && !misaligned(d_gy, 15)) ? 1 : 0};
  return launch<true>(a, p, m3d::as_stream(stream));
}
