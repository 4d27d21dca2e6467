// Backward of the box head's fully-connected layers on the f16 matrix cores at fp32 accuracy ("f16x2 split", tests/f16x2_contract.py),
// on the operands as PyTorch stores them - the two GEMMs of fc_backward.hip with v_mfma_f32_32x32x16_f16 instead of 32x32x2_f32:
//     dgrad   gx[M,K] = gy[M,N] . W[N,K]           (reduction over N)
//     wgrad   gw[N,K] = gy[M,N]^T . x[M,K]         (reduction over M),   gb[N] = sum_m gy[m,n] (uncut fp32) out of the same launch
// Every operand value is multiplied by its tensor's power of two (f16_scale_of of the tensor's bound: one scale per operand) and cut
// into hi = fp16(v), lo = fp16(v - hi) ONCE, on its way from the global-load registers to LDS; three MFMA products (hh, hl, lh) per
// fp32 product accumulate in fp32 and the scales are undone (exactly) in the epilogue.  No packed or transposed copy of W, x or gy
// exists: the 360 MB matrix is read once (fp32) and its gradient written once.
//
// Feeding the MFMA.  The output is [rows, K] in both GEMMs and the big operand B (W / x) is reduction-major: its row index is the
// reduction index, while lane (r, h) of a 32x32x16 MFMA wants 8 consecutive reduction indices of ONE column as a 16-byte fragment.
// The transposition happens in registers at staging: a thread loads the 16-byte quad of its 4 columns from 8 consecutive reduction
// rows, cuts the 32 values and writes, per column, one 16-byte hi and one 16-byte lo fragment - ds_read_b128 then delivers MFMA
// operands with no further movement.  The alternative (a reduction-major fp16 image read with ds_read_b64_tr_b16) needs two transposed
// reads per fragment: per 16-deep step a wave issues 2 A + 8 B fragments x 2 = 20 reads for its 12 MFMAs (1.7 per MFMA gap, of the 3
// that fit) against 10 ds_read_b128 here (0.8 per gap, of the 2 that fit); both fit, the cut costs the same VALU work in both, and the
// register transposition has no alignment rule to get wrong (a tr read at an address that is not 8-byte aligned returns other data)
// and stores with full-width conflict-free ds_write_b128.  32x32x16 and not 16x16x32: the same cycles per FLOP, half the fragment
// reads per FLOP, and the accumulator layout (column on the lane, rows in registers) that the quad store below needs.
//
// Design:
//  * workgroup tile 128 x 128 x 32, 4 waves; wave w owns 32 output rows and all 128 columns as four 32x32 blocks: block j of lane r is
//    column 4 r + j of the tile, so one accumulator register of the four blocks is one 16-byte store and a wave writes whole 512-byte
//    row segments; two workgroups per CU;
//  * LDS per stage: B as [k-group g = 0..3][e = 0..3][q = 0..31] x 16 bytes (column 4 q + e, reduction indices 8 g .. 8 g + 7), a hi
//    and a lo plane; a staging thread (q, g) writes its four fragments with four stores whose 8-lane groups are contiguous, and lane
//    (r, h) of k16 step s reads [2 s + h][j][r]: a half-wave reads 512 contiguous bytes (conflict-free).  wgrad's gy tile is
//    reduction-major as well and is staged and read the same way (wave w takes e = w: its MFMA row r is tile row 4 r + w);
//    dgrad's gy tile is reduction-contiguous already: a thread cuts 8 consecutive values of one row into one fragment pair,
//    [g][row] x 16 bytes with the group stride padded to 130 fragments so that the stores of 4 lanes x 2 rows fall on 8 bank quads;
//  * waves 0, 1 stage B, waves 2, 3 stage gy: 8 quads per thread and chunk, fetched before the chunk's MFMAs, cut and stored after them;
//  * reduction rows beyond the end are ZERO-FILLED in LDS (never clamped); output rows / columns beyond the end are clamped at the load
//    and masked at the store;
//  * an accumulator takes at most 384 chained MFMAs (64 chunks x 2 steps x 3 products) before it is folded into fp32 registers (the
//    rule of the f16x2 wgrad kernels); only a reduction longer than 2048 per slice reaches that, and only then the FOLD instantiation
//    (64 more registers, one workgroup per CU) runs;
//  * split of the reduction, unit order, partials and the slice-order reduce: as fc_backward.hip, except that a problem below 2^24
//    multiply-adds is never split (a second launch costs more than the few microseconds one workgroup needs for it);
//  * gb: in the workgroups of the first column tile the threads that stage gy add their raw fp32 values, each its 8 rows of every chunk
//    in row order, and the four k-group sums of a column are added in group order through LDS at the end; slices as the partials.
//    No atomics anywhere; results are bit-identical run to run.
#include "f16x2.h"

namespace {

using namespace m3d::f16x2;      // the cut, its vector types and the bound slots: f16x2.h

constexpr int BT = 128, BR = 32;                                   // tile edge, reduction chunk
constexpr int GSB = 128, GSD = 130;                                // fragments per k-group: reduction-major tiles / dgrad's gy tile
constexpr int kSlots = 512;                                        // resident workgroups: 256 CUs x 2
constexpr int kFoldChunks = 64;                                    // 64 chunks x 6 MFMAs = 384 per accumulator
constexpr long long kSplitMinWork = 1ll << 24;                     // M N K below this: one launch, no split
constexpr int kBoundBytes = 256;                                   // head of the workspace: the two swept bounds

struct FcbArgs {
  const float* gy; const float* b; float* out; float* part; float* gb; float* gb_part;
  const float* gy_bound; const float* b_bound; int gy_bound_n, b_bound_n;
  int M, N, K;
  int rows, red;          // output rows and reduction length: (M, N) in dgrad, (N, M) in wgrad
  int rt, kt, slices, chunks, per_xcd;
};

__device__ inline float bound_max(const float* __restrict__ b, int n) {
  float m = b[0];
  for (int i = 1; i < n; ++i) m = fmaxf(m, b[i]);
  return m;
}

// 8 values (already scaled) -> the hi and lo fragments
__device__ __forceinline__ void cut8(const float (&v)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f16x2 hh, ll;
    cut(v[2 * j], v[2 * j + 1], hh, ll);
    hi[j] = __builtin_bit_cast(unsigned, hh); lo[j] = __builtin_bit_cast(unsigned, ll);
  }
}

template <bool WGRAD, bool FOLD>
__global__ __launch_bounds__(256, FOLD ? 1 : 2) void fc_backward_f16_kernel(FcbArgs a) {
  constexpr int GSA = WGRAD ? GSB : GSD;
  constexpr int kAFrags = 4 * GSA, kBFrags = 4 * GSB;              // fragments (16 bytes) per plane
  constexpr int kStage = 2 * kAFrags + 2 * kBFrags;                // [A hi][A lo][B hi][B lo]
  extern __shared__ u32x4 lds[];                                   // 2 stages
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

  float sa, ia, sb, ib;                                            // the two scales and their inverses
  f16_scale_of(bound_max(a.gy_bound, a.gy_bound_n), sa, ia);
  f16_scale_of(bound_max(a.b_bound, a.b_bound_n), sb, ib);

  // ---- staging.  Waves 0, 1: B.  Waves 2, 3: gy.  Reduction-major tiles: thread -> (q = t % 32, g = t / 32), rows 8 g + j of the chunk,
  // columns 4 q .. 4 q + 3 (a half-wave load = 512 contiguous bytes of one row).  dgrad's gy tile: thread -> (g = t % 4, row = t / 4 + 32 i),
  // i = 0..3: the two quads 8 g .. 8 g + 7 of the chunk.
  const bool stage_b = wave < 2;                                   // wave-uniform
  const bool rm = stage_b || WGRAD;                                // this thread stages a reduction-major tile
  const int t = tid & 127;
  const int sq = t & 31, sg = t >> 5;
  const float* prm = stage_b ? a.b + min(k0 + 4 * sq, a.K - 4) : a.gy + min(r0 + 4 * sq, a.N - 4);   // column clamped: masked at the store
  const size_t ldrm = stage_b ? K : N;
  const float srm = stage_b ? sb : sa;
  const int dg = t & 3, drow = t >> 2;
  size_t doff[4];                                                  // dgrad: gy row offsets of this thread (row clamped: masked at the store)
#pragma unroll
  for (int i = 0; i < 4; ++i) doff[i] = (size_t)min(r0 + drow + 32 * i, a.M - 1) * N + 8 * dg;

  const bool own_gb = WGRAD && a.gb != nullptr && tk == 0;         // workgroup-uniform
  f32x4 gbsum = {0.f, 0.f, 0.f, 0.f};

  f32x4 sv[8];
  // whole chunks only: no predicate, nothing touches the loaded registers until commit() after the MFMA loop
  auto fetch = [&](int c) __attribute__((always_inline)) {
    if (rm) {
#pragma unroll
      for (int j = 0; j < 8; ++j) sv[j] = *reinterpret_cast<const f32x4*>(prm + (size_t)(c * BR + 8 * sg + j) * ldrm);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sv[2 * i] = *reinterpret_cast<const f32x4*>(a.gy + doff[i] + c * BR);
        sv[2 * i + 1] = *reinterpret_cast<const f32x4*>(a.gy + doff[i] + c * BR + 4);
      }
    }
  };
  // the ragged last chunk: every reduction index beyond the end is zero in LDS
  auto fetch_tail = [&]() __attribute__((always_inline)) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (rm) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int r = full * BR + 8 * sg + j;
        sv[j] = z;
        if (r < a.red) sv[j] = *reinterpret_cast<const f32x4*>(prm + (size_t)r * ldrm);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int hq = 0; hq < 2; ++hq) {
          const int n = full * BR + 8 * dg + 4 * hq;              // N % 4 == 0: a quad is inside or outside as a whole
          sv[2 * i + hq] = z;
          if (n + 4 <= a.N) sv[2 * i + hq] = *reinterpret_cast<const f32x4*>(a.gy + doff[i] + full * BR + 4 * hq);
        }
    }
  };
  auto commit = [&](u32x4* buf) __attribute__((always_inline)) {
    if (rm) {
      if constexpr (WGRAD) {
        if (own_gb && !stage_b) {
#pragma unroll
          for (int j = 0; j < 8; ++j) gbsum += sv[j];              // rows 8 g .. 8 g + 7 of the chunk, in row order
        }
      }
      u32x4* dst = buf + (stage_b ? 2 * kAFrags : 0) + sg * 4 * 32 + sq;
      const int lo_off = stage_b ? kBFrags : kAFrags;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = sv[j][e] * srm;
        u32x4 hi, lo;
        cut8(v, hi, lo);
        dst[e * 32] = hi; dst[e * 32 + lo_off] = lo;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = sv[2 * i + (j >> 2)][j & 3] * sa;
        u32x4 hi, lo;
        cut8(v, hi, lo);
        u32x4* dst = buf + dg * GSA + drow + 32 * i;
        dst[0] = hi; dst[kAFrags] = lo;
      }
    }
  };

  // ---- fragments: in k16 step s lane (fr, fh) holds the reduction indices 16 s + 8 fh .. + 7 of the chunk = k-group 2 s + fh
  const int fr = lane & 31, fh = lane >> 5;
  const int offA = WGRAD ? (fh * 4 + wave) * 32 + fr : fh * GSA + wave * 32 + fr;
  const int offB = 2 * kAFrags + fh * GSB + fr;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[j][g] = 0.f;
  f32x16 tot[FOLD ? 4 : 1];
  if constexpr (FOLD) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) tot[j][g] = 0.f;
  }
  int chained = 0;                                                 // chunks in the accumulators since the last fold

  auto compute = [&](const u32x4* cur) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const f16x8 ah = __builtin_bit_cast(f16x8, cur[offA + 2 * s * GSA]);
      const f16x8 al = __builtin_bit_cast(f16x8, cur[offA + 2 * s * GSA + kAFrags]);
      f16x8 bh[4], bl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bh[j] = __builtin_bit_cast(f16x8, cur[offB + 2 * s * GSB + j * 32]);
        bl[j] = __builtin_bit_cast(f16x8, cur[offB + 2 * s * GSB + j * 32 + kBFrags]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) mfma3(ah, al, bh[j], bl[j], acc[j]);
    }
    if constexpr (FOLD) {
      if (++chained == kFoldChunks) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          tot[j] += acc[j];
#pragma unroll
          for (int g = 0; g < 16; ++g) acc[j][g] = 0.f;
        }
        chained = 0;
      }
    }
  };

  if (c0 < c1f) { fetch(c0); commit(lds); }
  __syncthreads();
  for (int c = c0; c < c1f; ++c) {
    const u32x4* cur = lds + ((c - c0) & 1) * kStage;
    const bool more = c + 1 < c1f;
    if (more) fetch(c + 1);
    __builtin_amdgcn_sched_barrier(0);                            // keep the loads in front of the MFMAs
    compute(cur);
    if (more) commit(lds + ((c + 1 - c0) & 1) * kStage);
    __syncthreads();
  }
  if (c1 > c1f) {                                                 // only the last slice, only if red % 32 != 0
    fetch_tail();
    commit(lds);                                                  // stage 0: the loop's last barrier is behind every read of it
    __syncthreads();
    compute(lds);
  }
  if constexpr (FOLD) {
    if (chained) {
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[j] += acc[j];
    }
  }

  // ---- epilogue: register g of the four blocks is out[row][k0 + 4 fr .. + 3], row = r0 + wave*32 + acc_row(g) + 4 fh in dgrad and
  // r0 + 4 (acc_row(g) + 4 fh) + wave in wgrad: one 16-byte store per lane, a half-wave writes one 512-byte row segment
  const bool direct = a.slices == 1;
  float* dst = direct ? a.out : a.part + (size_t)slice * a.rows * K;
  const int k = k0 + 4 * fr;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int rl = acc_row(g) + 4 * fh;
    const int r = r0 + (WGRAD ? 4 * rl + wave : wave * 32 + rl);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((FOLD ? tot[j][g] : acc[j][g]) * ia) * ib;
    if (r < a.rows && k < a.K) *reinterpret_cast<f32x4*>(dst + (size_t)r * K + k) = v;
  }
  if constexpr (WGRAD) {
    if (own_gb) {                                                 // workgroup-uniform: every thread reaches the barriers
      float* red = reinterpret_cast<float*>(lds);
      __syncthreads();                                            // behind the last fragment reads
      if (!stage_b) *reinterpret_cast<f32x4*>(red + sg * BT + 4 * sq) = gbsum;
      __syncthreads();
      if (tid < BT) {                                             // column r0 + 4 q + e sits at [g][4 q + e] (clamped quads are masked here)
        const float v = ((red[tid] + red[BT + tid]) + red[2 * BT + tid]) + red[3 * BT + tid];
        if (r0 + tid < a.N) (direct ? a.gb : a.gb_part + (size_t)slice * N)[r0 + tid] = v;
      }
    }
  }
}

// out[e] = sum_s part[s][e] and gb[n] = sum_s gb_part[s][n], slices added in index order (fc_backward.hip's reduce, which lives in that
// file's unnamed namespace).  One thread = four consecutive outputs (K % 4 == 0, 16-byte aligned).
__global__ __launch_bounds__(256) void fc_backward_f16_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                     long long total, int slices, const float* __restrict__ gb_part,
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

struct BPlan { int rt, kt, chunks, slices, per_xcd, cps, chain, folds; };

// The split is a function of the shape only (fc_backward.hip's rule: fill the 512 workgroup slots once, at most 64 slices, about four
// chunks or more per slice), and none at all below kSplitMinWork multiply-adds.  cps = the most chunks a slice holds; an accumulator
// chains 6 MFMAs per chunk and is folded every kFoldChunks chunks where a slice is longer than that.
BPlan make_plan(int rows, int red, int K) {
  BPlan p;
  p.rt = (rows + BT - 1) / BT; p.kt = (K + BT - 1) / BT; p.chunks = (red + BR - 1) / BR;
  const long long tiles = (long long)p.rt * p.kt;
  int s = tiles >= kSlots ? 1 : (int)(kSlots / tiles);
  s = s > 64 ? 64 : s;
  s = s > p.chunks / 4 + 1 ? p.chunks / 4 + 1 : s;
  if ((long long)rows * red * K < kSplitMinWork) s = 1;
  p.slices = s < 1 ? 1 : s;
  p.per_xcd = (int)((tiles * p.slices + 7) / 8);
  p.cps = (p.chunks + p.slices - 1) / p.slices;
  p.chain = 6 * (p.cps < kFoldChunks ? p.cps : kFoldChunks);
  p.folds = p.cps > kFoldChunks ? (p.cps + kFoldChunks - 1) / kFoldChunks : 0;
  return p;
}

bool too_big(long long a, long long b) { return a * b >= (1ll << 31); }
bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }
bool supported(int M, int N, int K) {
  return M >= 1 && N >= 64 && K >= 4 && N % 4 == 0 && K % 4 == 0 && !too_big(M, N) && !too_big(N, K) && !too_big(M, K);
}

template <bool WGRAD, bool FOLD>
void launch_gemm(const FcbArgs& a, const BPlan& p, hipStream_t st) {
  const size_t lds = sizeof(u32x4) * 2 * (2 * 4 * (WGRAD ? GSB : GSD) + 2 * 4 * GSB);
  auto kern = fc_backward_f16_kernel<WGRAD, FOLD>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(8 * p.per_xcd), dim3(256), lds, st, a);
}

template <bool WGRAD>
int launch(const FcbArgs& a, const BPlan& p, hipStream_t st) {
  if (p.folds) launch_gemm<WGRAD, true>(a, p, st);
  else launch_gemm<WGRAD, false>(a, p, st);
  if (p.slices > 1) {
    const long long total = (long long)a.rows * a.K;
    long long blocks = (total / 4 + 255) / 256;
    blocks = blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(fc_backward_f16_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)a.part, a.out, total,
                       p.slices, (const float*)a.gb_part, a.gb, a.N);
  }
  return m3d::check_launch(WGRAD ? "linear_wgrad_f16x2" : "linear_dgrad_f16x2");
}

int plan_out(const BPlan& p, int* slices, int* chain, int* folds) {
  if (slices) *slices = p.slices;
  if (chain) *chain = p.chain;
  if (folds) *folds = p.folds;
  return M3D_OK;
}

bool bad_slots(const float* b, int n) { return b && (n < 1 || n > 1024); }

}  // namespace

M3D_API int m3d_linear_backward_f16x2_supported(int M, int N, int K) { return supported(M, N, K) ? 1 : 0; }

M3D_API int m3d_linear_dgrad_f16x2_plan(int M, int N, int K, int* slices, int* chain, int* folds) {
  if (M < 1 || N < 1 || K < 1) return M3D_EINVAL;
  if (!supported(M, N, K)) return M3D_EUNSUPPORTED;
  return plan_out(make_plan(M, N, K), slices, chain, folds);
}

M3D_API int m3d_linear_wgrad_f16x2_plan(int M, int N, int K, int* slices, int* chain, int* folds) {
  if (M < 1 || N < 1 || K < 1) return M3D_EINVAL;
  if (!supported(M, N, K)) return M3D_EUNSUPPORTED;
  return plan_out(make_plan(N, M, K), slices, chain, folds);
}

M3D_API size_t m3d_linear_dgrad_f16x2_workspace_bytes(int M, int N, int K) {
  if (!supported(M, N, K)) return 0;
  const BPlan p = make_plan(M, N, K);
  return kBoundBytes + (p.slices > 1 ? m3d::align_up((size_t)p.slices * M * K * sizeof(float), 16) : 0);
}

M3D_API size_t m3d_linear_wgrad_f16x2_workspace_bytes(int M, int N, int K) {
  if (!supported(M, N, K)) return 0;
  const BPlan p = make_plan(N, M, K);
  return kBoundBytes + (p.slices > 1 ? m3d::align_up((size_t)p.slices * ((size_t)N * K + N) * sizeof(float), 16) : 0);
}

M3D_API int m3d_linear_dgrad_f16x2(const float* d_gy, const float* d_weight, float* d_gx, int M, int N, int K, const float* d_gy_bound,
                                   int gy_bound_slots, const float* d_w_bound, int w_bound_slots, void* d_ws, size_t ws_bytes,
                                   void* stream) {
  if (M < 0 || N < 1 || K < 1) return M3D_EINVAL;
  if (M == 0) return M3D_OK;                                       // nothing to write: no pointer is looked at
  if (!supported(M, N, K)) return M3D_EUNSUPPORTED;                // the shape first: a refusal needs no pointer
  if (!d_gy || !d_weight || !d_gx || !d_ws) return M3D_EINVAL;
  if (bad_slots(d_gy_bound, gy_bound_slots) || bad_slots(d_w_bound, w_bound_slots)) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_weight, 3) || misaligned(d_gx, 3) || misaligned(d_ws, 3) || misaligned(d_gy_bound, 3) ||
      misaligned(d_w_bound, 3))
    return M3D_EINVAL;
  if (misaligned(d_gy, 15) || misaligned(d_weight, 15) || misaligned(d_gx, 15) || misaligned(d_ws, 15)) return M3D_EUNSUPPORTED;
  if (ws_bytes < m3d_linear_dgrad_f16x2_workspace_bytes(M, N, K)) return M3D_EINVAL;
  const BPlan p = make_plan(M, N, K);
  float* bounds = (float*)d_ws;
  if (!d_gy_bound) {
    if (const int rc = m3d_absmax(d_gy, (long long)M * N, bounds, stream)) return rc;
    d_gy_bound = bounds; gy_bound_slots = 1;
  }
  if (!d_w_bound) {
    if (const int rc = m3d_absmax(d_weight, (long long)N * K, bounds + 1, stream)) return rc;
    d_w_bound = bounds + 1; w_bound_slots = 1;
  }
  float* part = (float*)((char*)d_ws + kBoundBytes);
  FcbArgs a{d_gy, d_weight, d_gx, part, nullptr, nullptr, d_gy_bound, d_w_bound, gy_bound_slots, w_bound_slots, M, N, K, M, N,
            p.rt, p.kt, p.slices, p.chunks, p.per_xcd};
  return launch<false>(a, p, m3d::as_stream(stream));
}

M3D_API int m3d_linear_wgrad_f16x2(const float* d_gy, const float* d_x, float* d_gw, float* d_gb, int M, int N, int K,
                                   const float* d_gy_bound, int gy_bound_slots, const float* d_x_bound, int x_bound_slots, void* d_ws,
                                   size_t ws_bytes, void* stream) {
  if (M < 0 || N < 1 || K < 1) return M3D_EINVAL;
  if (!supported(M > 0 ? M : 1, N, K)) return M3D_EUNSUPPORTED;    // the shape first: a refusal needs no pointer
  if (!d_gw || (M > 0 && (!d_gy || !d_x || !d_ws))) return M3D_EINVAL;
  if (bad_slots(d_gy_bound, gy_bound_slots) || bad_slots(d_x_bound, x_bound_slots)) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_x, 3) || misaligned(d_gw, 3) || misaligned(d_gb, 3) || misaligned(d_ws, 3) ||
      misaligned(d_gy_bound, 3) || misaligned(d_x_bound, 3))
    return M3D_EINVAL;
  if (misaligned(d_gy, 15) || misaligned(d_x, 15) || misaligned(d_gw, 15) || misaligned(d_ws, 15)) return M3D_EUNSUPPORTED;
  hipStream_t st = m3d::as_stream(stream);
  if (M == 0) {                                                    // an empty batch: torch's gradients are zeros
    if (hipMemsetAsync(d_gw, 0, (size_t)N * K * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    if (d_gb && hipMemsetAsync(d_gb, 0, (size_t)N * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    return M3D_OK;
  }
  if (ws_bytes < m3d_linear_wgrad_f16x2_workspace_bytes(M, N, K)) return M3D_EINVAL;
  const BPlan p = make_plan(N, M, K);
  float* bounds = (float*)d_ws;
  if (!d_gy_bound) {
    if (const int rc = m3d_absmax(d_gy, (long long)M * N, bounds, stream)) return rc;
    d_gy_bound = bounds; gy_bound_slots = 1;
  }
  if (!d_x_bound) {
    if (const int rc = m3d_absmax(d_x, (long long)M * K, bounds + 1, stream)) return rc;
    d_x_bound = bounds + 1; x_bound_slots = 1;
  }
  float* part = (float*)((char*)d_ws + kBoundBytes);
  FcbArgs a{d_gy, d_x, d_gw, part, d_gb, part + (size_t)p.slices * N * K, d_gy_bound, d_x_bound, gy_bound_slots, x_bound_slots, M, N, K,
            N, M, p.rt, p.kt, p.slices, p.chunks, p.per_xcd};
  return launch<true>(a, p, st);
}
