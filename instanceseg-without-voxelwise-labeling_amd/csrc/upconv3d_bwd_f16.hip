// Backward of the mask head's ConvTranspose3d(kernel 2, stride 2, padding 0) (+ ReLU) on the f16 matrix cores at fp32 accuracy ("f16x2
// split", tests/f16x2_contract.py), on the operands as PyTorch stores them - the two GEMMs of upconv3d.hip's backward with
// v_mfma_f32_32x32x16_f16 instead of 32x32x2_f32.  With col = (r, z, y, x) over ALL RoIs, n = 8 co + 4 a + 2 b + c and
// g[col, n] = gy[r, co, 2z+a, 2y+b, 2x+c], set to 0 where the forward's own output y is <= 0 (a SELECT while staging, before the cut: a
// masked-out Inf / NaN contributes exactly 0):
//     dgrad   gx[col, ci] = sum_n   g[col, n] W[ci, n]          (reduction 8 Cout)
//     wgrad   gW[ci, n]   = sum_col x[col, ci] g[col, n]        (reduction R D H W);   gb[co] = sum g (uncut fp32) out of the same launch
// Every operand value is multiplied by its tensor's power of two (f16_scale_of of the tensor's bound; for g that is the bound of the
// UNMASKED gy) and cut into hi = fp16(v), lo = fp16(v - hi) ONCE, on its way from the global-load registers to LDS or to the MFMA
// operand registers; three MFMA products (hh, hl, lh) per fp32 product accumulate in fp32 and the scales are undone (exactly) in the
// epilogue.  No packed, transposed or shuffled copy of gy, y, x or W exists.
//
// Feeding the MFMA.  Lane (r, h) of a 32x32x16 MFMA wants 8 consecutive reduction indices of ONE row / column as a 16-byte fragment.
//  * dgrad: the reduction runs over n.  The 8 values n = 8 co .. 8 co + 7 of one column are the 2 x 2 x 2 output voxels of one input
//    voxel in one channel: four 8-byte loads (a, b; c = 0, 1 adjacent), neighbouring lanes at neighbouring x.  W[ci, n] is contiguous
//    along n: a lane's fragment is two 16-byte loads from the raw fp32 tensor (L2-resident, 2 MB at 256 -> 256), cut in registers - no
//    pack call, no LDS for W.  The accumulator holds the column on the lane and ci in its registers: a store writes 32 consecutive
//    voxels of one gx channel.
//  * wgrad: the reduction runs over columns.  Neither x nor g is contiguous along it in units an MFMA can use (V = 343: no row is a
//    16-byte multiple, g has stride 2), so a staging thread gathers its 8 columns with 4- / 8-byte loads and cuts them into one fragment.
//    The reduction order inside a 32-column chunk is free as long as both operands agree: fragment (k-group kg, element j) holds
//    column chunk * 32 + kg + 4 j, so the four lanes kg = 0..3 of one load instruction sit at neighbouring voxels.  A thread walks its
//    columns incrementally ((x, y, z, r) += 4 with carries): no division in the loop.
//
// Design:
//  * dgrad: a workgroup (4 waves) owns 64 columns and up to 256 input channels (blockIdx.y: the 256-channel group); wave w takes the
//    32-channel blocks w and w + 4 of the group against both 32-column blocks: four 32x32 accumulators.  The reduction is walked in
//    chunks of 32 n (4 output channels): thread (column t % 64, channel t / 64) stages one g fragment pair per chunk
//    ([hi / lo][k-group][64 columns] x 16 bytes, double-buffered: 16 KB), the W fragments of the next chunk are requested before the
//    chunk's MFMAs and cut after them.  Never split: slices = 1, no workspace beyond the swept bounds;
//  * wgrad: workgroup tile 128 (ci) x 128 (n) x 32 columns, 4 waves; wave w owns 32 rows and all 128 columns as four 32x32 blocks,
//    block j of lane r = column 4 r + j, so one accumulator register of the four blocks is one 16-byte store (fc_backward_f16.hip's
//    output layout).  LDS per stage: x as [k-group][128 rows] and g as [k-group][j][32] fragments, a hi and a lo plane each; the
//    k-group strides are padded (130 / 137 fragments, 34 per j) so that the 8 lanes of a 16-byte store phase (4 k-groups x 2 rows) fall
//    on 8 different bank quads, and a half-wave reads 512 contiguous bytes.  Split-K over column chunks into the workspace (at most 16
//    slices of about four chunks or more, a function of the shape only), partials folded in slice order by a reduce launch;
//  * columns beyond the end are ZERO in LDS (wgrad: reduction) or clamped at the load and masked at the store (dgrad: output);
//    32-channel blocks beyond Cin are skipped;
//  * an accumulator takes at most 384 chained MFMAs (64 chunks x 2 steps x 3 products) before it is folded into fp32 registers (the
//    rule of the f16x2 wgrad kernels); only then the FOLD instantiation (64 more registers, one workgroup per CU) runs: dgrad at
//    Cout > 256, wgrad where a slice holds more than 2048 columns;
//  * gb: in the workgroups of the first row tile every thread adds the raw masked fp32 values it stages (its 8 columns of every chunk
//    in order, c = 0 and c = 1 apart); the four k-group sums of an n are added in group order through LDS, then the 8 parities of a
//    channel in n order, then the slices in slice order.
//    No atomics anywhere; every output element and every workspace element the call reads is written by the call; bit-identical run
//    to run.  An Inf / NaN in an unmasked operand (or in a bound) gives NaN, never a finite number.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):     VGPRs   AGPRs   SGPRs   scratch   LDS (dynamic)   workgroups / CU
//   upconv_dgrad_f16_kernel<false>                                     176       0      48         0          16 384                 2
//   upconv_dgrad_f16_kernel<true>  (FOLD)                              222      64      47         0          16 384                 1
//   upconv_wgrad_f16_kernel<false>                                     188       0      76         0          68 352                 2
//   upconv_wgrad_f16_kernel<true>  (FOLD)                              256      92      77         0          68 352                 1
//
// The constants of the accuracy contract (tests/upconv_backward_f16_cases.py), from this code: c1 = 3.01 (neither operand is rounded
// before the cut); an output's running sum is rounded once per MFMA of its chain (at most `chain` between two folds), once per fold,
// once per slice the reduce launch adds, and by the two scale multiplies: n_acc = chain max(folds, 1) + folds + slices + 2, with
// (slices, chain, folds) from the _plan calls.  gb adds 8 R D H W fp32 terms and gb_partials = 32 + slices partial sums.
#include <initializer_list>

#include "f16x2.h"

namespace {

using namespace m3d::f16x2;      // the cut, its vector types and the bound slots: f16x2.h

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kChunk = 32;                       // reduction indices per chunk: two 16-deep MFMA steps
constexpr int kFoldChunks = 64;                  // 64 chunks x 6 MFMAs = 384 per accumulator
constexpr int kBoundBytes = 256;                 // head of the workspace: the two swept bounds
constexpr int DG_VT = 64;                        // dgrad: columns of a workgroup
constexpr int DG_CB = 8;                         // dgrad: 32-channel blocks of a workgroup (two per wave)
constexpr int WG_BT = 128;                       // wgrad: tile edge
constexpr int WG_SKA = 130;                      // wgrad: fragments per k-group of the x plane
constexpr int WG_SJ = 34, WG_SKB = 4 * WG_SJ + 1;   // wgrad: fragments per j / per k-group of the g plane
constexpr int WG_PLANE_A = 4 * WG_SKA, WG_PLANE_B = 4 * WG_SKB;
constexpr int WG_STAGE = 2 * WG_PLANE_A + 2 * WG_PLANE_B;   // [x hi][x lo][g hi][g lo]
constexpr int kSlots = 512;                      // resident workgroups: 256 CUs x 2
constexpr int kMaxSlices = 16;

struct UbArgs {
  const float* gy; const float* ym; const float* b;          // b: W (dgrad) / x (wgrad)
  float* out; float* part; float* gb; float* gb_part;
  const float* gy_bound; const float* b_bound; int gy_bound_n, b_bound_n;
  int R, Cin, Cout, D, H, W, V;
  int cols;                                                   // R V
  int rt, kt, slices, chunks, per_xcd;                        // wgrad
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

// g = gy where the forward's output is positive (a select: a masked-out Inf / NaN is 0)
__device__ __forceinline__ f32x2 masked(f32x2 g, f32x2 m, bool has_mask) {
  if (has_mask) { g[0] = m[0] > 0.f ? g[0] : 0.f; g[1] = m[1] > 0.f ? g[1] : 0.f; }
  return g;
}

// ------------------------------------------------------------------ dgrad
template <bool FOLD>
__global__ __launch_bounds__(256, FOLD ? 1 : 2) void upconv_dgrad_f16_kernel(UbArgs a) {
  constexpr int kPlane = 4 * DG_VT, kStage = 2 * kPlane;           // [hi][lo] of [k-group][64 columns]
  extern __shared__ u32x4 ub_lds[];                                // 2 stages
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NC = 8 * a.Cout, chunks = a.Cout / 4, ncb = a.Cin / 32;
  const size_t V = (size_t)a.V;
  const int H2W2 = 4 * a.H * a.W, W2 = 2 * a.W;
  const bool has_mask = a.ym != nullptr;

  float sa, ia, sb, ib;                                            // the two scales and their inverses
  f16_scale_of(bound_max(a.gy_bound, a.gy_bound_n), sa, ia);
  f16_scale_of(bound_max(a.b_bound, a.b_bound_n), sb, ib);

  // ---- staging of g: thread = (column tid % 64, output channel tid / 64 of the chunk); a column beyond the end re-reads the last one
  const int col0 = blockIdx.x * DG_VT;
  const int sc = tid & 63, skg = tid >> 6;
  size_t gbase;                                                    // offset of (r, co = skg, 2z, 2y, 2x)
  {
    const int c = min(col0 + sc, a.cols - 1);
    const int r = c / a.V, v = c - r * a.V;
    const int x = v % a.W, zy = v / a.W, y = zy % a.H, z = zy / a.H;
    gbase = ((size_t)r * a.Cout + skg) * 8 * V + (size_t)(((2 * z) * (2 * a.H) + 2 * y) * W2 + 2 * x);
  }
  // ---- W fragments: the channel blocks of this wave, lane (fr, fh) = row fr, reduction indices 16 s + 8 fh .. + 7 of the chunk
  const int fr = lane & 31, fh = lane >> 5;
  const int cb0 = blockIdx.y * DG_CB + wave;
  const int nblk = cb0 >= ncb ? 0 : (cb0 + 4 >= ncb ? 1 : 2);      // wave-uniform
  const float* wrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) wrow[i] = a.b + (size_t)(min(cb0 + 4 * i, ncb - 1) * 32 + fr) * NC + 8 * fh;

  f32x2 sg[4], sm[4];
  f32x4 wraw[2][2][2];
  auto fetch = [&](int c) __attribute__((always_inline)) {
    const size_t off = gbase + (size_t)(4 * c) * 8 * V;
#pragma unroll
    for (int ab = 0; ab < 4; ++ab) {
      const size_t o = off + (ab >> 1) * H2W2 + (ab & 1) * W2;
      sg[ab] = *reinterpret_cast<const f32x2*>(a.gy + o);
      if (has_mask) sm[ab] = *reinterpret_cast<const f32x2*>(a.ym + o);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 2; ++q) wraw[i][s][q] = *reinterpret_cast<const f32x4*>(wrow[i] + c * kChunk + 16 * s + 4 * q);
  };
  f16x8 Ah[2][2], Al[2][2];                                        // [block][step]
  auto commit = [&](u32x4* buf) __attribute__((always_inline)) {
    float v[8];
#pragma unroll
    for (int ab = 0; ab < 4; ++ab) {
      const f32x2 g = masked(sg[ab], sm[ab], has_mask);
      v[2 * ab] = g[0] * sa; v[2 * ab + 1] = g[1] * sa;
    }
    u32x4 hi, lo;
    cut8(v, hi, lo);
    buf[skg * DG_VT + sc] = hi; buf[kPlane + skg * DG_VT + sc] = lo;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = wraw[i][s][j >> 2][j & 3] * sb;
        cut8(v, hi, lo);
        Ah[i][s] = __builtin_bit_cast(f16x8, hi); Al[i][s] = __builtin_bit_cast(f16x8, lo);
      }
  };

  f32x16 acc[2][2];                                                // [channel block][column block]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
  f32x16 tot[FOLD ? 2 : 1][FOLD ? 2 : 1];
  if constexpr (FOLD) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) tot[i][j][g] = 0.f;
  }
  int chained = 0;                                                 // chunks in the accumulators since the last fold

  auto compute = [&](const u32x4* cur) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f16x8 bh[2], bl[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bh[j] = __builtin_bit_cast(f16x8, cur[(2 * s + fh) * DG_VT + 32 * j + fr]);
        bl[j] = __builtin_bit_cast(f16x8, cur[kPlane + (2 * s + fh) * DG_VT + 32 * j + fr]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (i < nblk) {
#pragma unroll
          for (int j = 0; j < 2; ++j) mfma3(Ah[i][s], Al[i][s], bh[j], bl[j], acc[i][j]);
        }
    }
    if constexpr (FOLD) {
      if (++chained == kFoldChunks) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            tot[i][j] += acc[i][j];
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
          }
        chained = 0;
      }
    }
  };

  fetch(0);
  commit(ub_lds);
  __syncthreads();
  for (int c = 0; c < chunks; ++c) {
    const u32x4* cur = ub_lds + (c & 1) * kStage;
    const bool more = c + 1 < chunks;
    if (more) fetch(c + 1);
    __builtin_amdgcn_sched_barrier(0);                             // keep the loads in front of the MFMAs
    compute(cur);
    if (more) commit(ub_lds + ((c + 1) & 1) * kStage);
    __syncthreads();
  }
  if constexpr (FOLD) {
    if (chained) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) tot[i][j] += acc[i][j];
    }
  }

  // ---- epilogue: register g of block (i, j) is channel 32 (cb0 + 4 i) + acc_row(g) + 4 fh of column col0 + 32 j + fr
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = col0 + 32 * j + fr;
    if (c >= a.cols) continue;
    const int r = c / a.V, v = c - r * a.V;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i >= nblk) continue;
      float* dst = a.out + ((size_t)r * a.Cin + (cb0 + 4 * i) * 32 + 4 * fh) * V + v;
#pragma unroll
      for (int g = 0; g < 16; ++g) dst[(size_t)acc_row(g) * V] = ((FOLD ? tot[i][j][g] : acc[i][j][g]) * ia) * ib;
    }
  }
}

// ------------------------------------------------------------------ wgrad
struct ColPos { int x, y, z, r; };

// the column n further on (n <= 4: at most five carries)
__device__ __forceinline__ void advance(ColPos& p, int n, int W, int H, int D) {
  p.x += n;
  while (p.x >= W) {
    p.x -= W;
    if (++p.y == H) {
      p.y = 0;
      if (++p.z == D) { p.z = 0; ++p.r; }
    }
  }
}

template <bool FOLD>
__global__ __launch_bounds__(256, FOLD ? 1 : 2) void upconv_wgrad_f16_kernel(UbArgs a) {
  extern __shared__ u32x4 ub_lds[];                                // 2 stages
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int tiles = a.rt * a.kt, u = xcd * a.per_xcd + idx;
  if (idx >= a.per_xcd || u >= tiles * a.slices) return;
  const int slice = u / tiles, tile = u - slice * tiles;
  const int tk = tile / a.rt, tr = tile - tk * a.rt;               // row tiles of one column panel are neighbours
  const int r0 = tr * WG_BT, k0 = tk * WG_BT;
  const int c0 = (int)((long long)slice * a.chunks / a.slices), c1 = (int)((long long)(slice + 1) * a.chunks / a.slices);
  const int NC = 8 * a.Cout;
  const size_t V = (size_t)a.V;
  const int H2W2 = 4 * a.H * a.W, W2 = 2 * a.W;
  const bool has_mask = a.ym != nullptr;

  float sa, ia, sb, ib;                                            // the two scales and their inverses
  f16_scale_of(bound_max(a.gy_bound, a.gy_bound_n), sa, ia);
  f16_scale_of(bound_max(a.b_bound, a.b_bound_n), sb, ib);

  // ---- staging.  thread = (k-group kg = t % 4, unit t / 4): its columns are chunk * 32 + kg + 4 j, j = 0..7, on both operands.
  // g: unit = the n pair p (n = k0 + 2 p, + 1: c = 0, 1 - one 8-byte load per column); x: unit = rows p and p + 64 of the tile
  const int kg = tid & 3, p = tid >> 2;
  const int n0 = k0 + 2 * p;
  const size_t gbase = (size_t)(n0 >> 3) * 8 * V + ((n0 >> 2) & 1) * H2W2 + ((n0 >> 1) & 1) * W2;
  size_t xbase[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) xbase[i] = (size_t)min(r0 + p + 64 * i, a.Cin - 1) * V;   // row clamped: its block is skipped
  ColPos pos;
  int col = c0 * kChunk + kg;                                      // the next column this thread fetches
  {
    const int r = col / a.V, v = col - r * a.V;
    pos.r = r; pos.x = v % a.W;
    const int zy = v / a.W;
    pos.y = zy % a.H; pos.z = zy / a.H;
  }
  const int rowx = a.Cin * a.V, rowg = a.Cout * 8 * a.V;           // elements of one RoI of x / of gy

  const bool own_gb = a.gb != nullptr && tr == 0;                  // workgroup-uniform
  f32x2 gbsum = {0.f, 0.f};

  f32x2 sg[8], sm[8];
  float sx[2][8];
  unsigned valid = 0;                                              // bit j: column j of the fetched chunk exists
  // columns in order, chunk after chunk: fetch(c0), fetch(c0 + 1), ..  Nothing touches the loaded registers until commit()
  auto fetch = [&]() __attribute__((always_inline)) {
    valid = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool ok = col < a.cols;
      valid |= ok ? 1u << j : 0u;
      const int xo = ok ? pos.r * rowx + (pos.z * a.H + pos.y) * a.W + pos.x : 0;
      const int go = ok ? pos.r * rowg + ((2 * pos.z) * (2 * a.H) + 2 * pos.y) * W2 + 2 * pos.x : 0;
      sg[j] = *reinterpret_cast<const f32x2*>(a.gy + gbase + go);
      if (has_mask) sm[j] = *reinterpret_cast<const f32x2*>(a.ym + gbase + go);
#pragma unroll
      for (int i = 0; i < 2; ++i) sx[i][j] = a.b[xbase[i] + xo];
      col += 4;
      advance(pos, 4, a.W, a.H, a.D);
    }
  };
  // registers -> LDS: columns beyond the end are zero on both operands, gy is masked by y > 0
  auto commit = [&](u32x4* buf) __attribute__((always_inline)) {
    float v0[8], v1[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f32x2 g = masked(sg[j], sm[j], has_mask);
      if (!(valid >> j & 1)) { g[0] = 0.f; g[1] = 0.f; }
      if (own_gb) gbsum += g;                                      // the uncut values, column order
      v0[j] = g[0] * sa; v1[j] = g[1] * sa;
    }
    u32x4 hi, lo;
    u32x4* gdst = buf + 2 * WG_PLANE_A + kg * WG_SKB + 2 * (p & 1) * WG_SJ + (p >> 1);   // n - k0 = 4 q + j: q = p / 2, j = 2 (p % 2) + c
    cut8(v0, hi, lo);
    gdst[0] = hi; gdst[WG_PLANE_B] = lo;
    cut8(v1, hi, lo);
    gdst[WG_SJ] = hi; gdst[WG_SJ + WG_PLANE_B] = lo;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v0[j] = (valid >> j & 1) ? sx[i][j] * sb : 0.f;
      cut8(v0, hi, lo);
      u32x4* xdst = buf + kg * WG_SKA + p + 64 * i;
      xdst[0] = hi; xdst[WG_PLANE_A] = lo;
    }
  };

  // ---- fragments: in k16 step s lane (fr, fh) holds k-group 2 s + fh; wave w owns rows 32 w .. 32 w + 31 of the tile
  const int fr = lane & 31, fh = lane >> 5;
  const bool live = r0 + 32 * wave < a.Cin;                        // wave-uniform: a block beyond Cin is skipped
  const int offA = fh * WG_SKA + 32 * wave + fr;
  const int offB = 2 * WG_PLANE_A + fh * WG_SKB + fr;
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
    if (live) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f16x8 ah = __builtin_bit_cast(f16x8, cur[offA + 2 * s * WG_SKA]);
        const f16x8 al = __builtin_bit_cast(f16x8, cur[offA + 2 * s * WG_SKA + WG_PLANE_A]);
        f16x8 bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bh[j] = __builtin_bit_cast(f16x8, cur[offB + 2 * s * WG_SKB + j * WG_SJ]);
          bl[j] = __builtin_bit_cast(f16x8, cur[offB + 2 * s * WG_SKB + j * WG_SJ + WG_PLANE_B]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) mfma3(ah, al, bh[j], bl[j], acc[j]);
      }
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

  fetch();                                                         // c0 < c1: every slice holds a chunk
  commit(ub_lds);
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    const u32x4* cur = ub_lds + ((c - c0) & 1) * WG_STAGE;
    const bool more = c + 1 < c1;
    if (more) fetch();
    __builtin_amdgcn_sched_barrier(0);                             // keep the loads in front of the MFMAs
    compute(cur);
    if (more) commit(ub_lds + ((c + 1 - c0) & 1) * WG_STAGE);
    __syncthreads();
  }
  if constexpr (FOLD) {
    if (chained) {
#pragma unroll
      for (int j = 0; j < 4; ++j) tot[j] += acc[j];
    }
  }

  // ---- epilogue: register g of the four blocks is gW[r0 + 32 w + acc_row(g) + 4 fh][k0 + 4 fr .. + 3]: one 16-byte store per lane
  const bool direct = a.slices == 1;
  if (live) {
    float* dst = (direct ? a.out : a.part + (size_t)slice * a.Cin * NC) + k0 + 4 * fr;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int r = r0 + 32 * wave + acc_row(g) + 4 * fh;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ((FOLD ? tot[j][g] : acc[j][g]) * ia) * ib;
      *reinterpret_cast<f32x4*>(dst + (size_t)r * NC) = v;
    }
  }
  if (own_gb) {                                                    // workgroup-uniform; the loop's last barrier is behind every read of LDS
    float* red = reinterpret_cast<float*>(ub_lds);
    *reinterpret_cast<f32x2*>(red + kg * WG_BT + 2 * p) = gbsum;   // [k-group][n - k0]
    __syncthreads();
    if (tid < WG_BT) red[4 * WG_BT + tid] = ((red[tid] + red[WG_BT + tid]) + red[2 * WG_BT + tid]) + red[3 * WG_BT + tid];
    __syncthreads();
    if (tid < WG_BT / 8) {
      const float* q = red + 4 * WG_BT + 8 * tid;
      float s = q[0];
#pragma unroll
      for (int e = 1; e < 8; ++e) s += q[e];
      (direct ? a.gb : a.gb_part + (size_t)slice * a.Cout)[(k0 >> 3) + tid] = s;
    }
  }
}

// out[e] = sum_s part[s][e] and gb[n] = sum_s gb_part[s][n], slices added in index order.  One thread = four consecutive outputs
// (the output is Cin x 8 Cout floats, 16-byte aligned).
__global__ __launch_bounds__(256) void upconv_bwd_f16_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, long long total,
                                                                    int slices, const float* __restrict__ gb_part, float* __restrict__ gb,
                                                                    int N) {
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

// chain = the most MFMAs an accumulator takes between two folds (6 per chunk), folds = the folds of the longest slice
void chain_of(BPlan& p) {
  p.cps = (p.chunks + p.slices - 1) / p.slices;
  p.chain = 6 * (p.cps < kFoldChunks ? p.cps : kFoldChunks);
  p.folds = p.cps > kFoldChunks ? (p.cps + kFoldChunks - 1) / kFoldChunks : 0;
}

// dgrad: one chunk = 4 output channels, never split
BPlan dgrad_plan(int Cout) {
  BPlan p{};
  p.chunks = Cout / 4; p.slices = 1;
  chain_of(p);
  return p;
}

// wgrad: the split is a function of the shape only - fill the 512 workgroup slots once, at most kMaxSlices slices, about four chunks or
// more per slice
BPlan wgrad_plan(int R, int Cin, int Cout, int V) {
  BPlan p{};
  p.rt = (Cin + WG_BT - 1) / WG_BT; p.kt = 8 * Cout / WG_BT;
  p.chunks = (int)(((long long)R * V + kChunk - 1) / kChunk);
  const int tiles = p.rt * p.kt;
  int s = tiles >= kSlots ? 1 : kSlots / tiles;
  s = s > kMaxSlices ? kMaxSlices : s;
  s = s > p.chunks / 4 + 1 ? p.chunks / 4 + 1 : s;
  p.slices = s < 1 ? 1 : s;
  p.per_xcd = (tiles * p.slices + 7) / 8;
  chain_of(p);
  return p;
}

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

bool supported(int R, int Cin, int Cout, int D, int H, int W) {
  if (R < 1 || bad_dims(R, Cin, Cout, D, H, W) || Cin % 32 != 0 || Cout % 32 != 0) return false;
  return !(too_big({R, Cin, D, H, W}) || too_big({R, Cout, 8, D, H, W}) || too_big({Cin, Cout, 8}));
}

int plan_out(const BPlan& p, int* slices, int* chain, int* folds) {
  if (slices) *slices = p.slices;
  if (chain) *chain = p.chain;
  if (folds) *folds = p.folds;
  return M3D_OK;
}

// the bounds a caller left out, swept into the head of the workspace: slot 0 (gy) and slot kBoundSlots (the other operand)
int sweep_bounds(UbArgs& a, long long gy_n, long long b_n, void* d_ws, void* stream) {
  float* bounds = (float*)d_ws;
  a.gy_bound_n = a.b_bound_n = kBoundSlots;
  if (!a.gy_bound) {
    if (const int rc = m3d_absmax(a.gy, gy_n, bounds, stream)) return rc;
    a.gy_bound = bounds; a.gy_bound_n = 1;
  }
  if (!a.b_bound) {
    if (const int rc = m3d_absmax(a.b, b_n, bounds + kBoundSlots, stream)) return rc;
    a.b_bound = bounds + kBoundSlots; a.b_bound_n = 1;
  }
  return M3D_OK;
}

}  // namespace

M3D_API int m3d_upconv3d_2x_backward_f16x2_supported(int R, int Cin, int Cout, int D, int H, int W) {
  return supported(R, Cin, Cout, D, H, W) ? 1 : 0;
}

M3D_API int m3d_upconv3d_2x_dgrad_f16x2_plan(int R, int Cin, int Cout, int D, int H, int W, int* slices, int* chain, int* folds) {
  if (R < 1 || bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (!supported(R, Cin, Cout, D, H, W)) return M3D_EUNSUPPORTED;
  return plan_out(dgrad_plan(Cout), slices, chain, folds);
}

M3D_API int m3d_upconv3d_2x_wgrad_f16x2_plan(int R, int Cin, int Cout, int D, int H, int W, int* slices, int* chain, int* folds,
                                             int* gb_partials) {
  if (R < 1 || bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (!supported(R, Cin, Cout, D, H, W)) return M3D_EUNSUPPORTED;
  const BPlan p = wgrad_plan(R, Cin, Cout, D * H * W);
  if (gb_partials) *gb_partials = 32 + p.slices;                   // 4 k-groups x 8 parities of a channel, then the slices
  return plan_out(p, slices, chain, folds);
}

M3D_API size_t m3d_upconv3d_2x_dgrad_f16x2_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W) {
  return supported(R, Cin, Cout, D, H, W) ? kBoundBytes : 0;
}

M3D_API size_t m3d_upconv3d_2x_wgrad_f16x2_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W) {
  if (!supported(R, Cin, Cout, D, H, W)) return 0;
  const BPlan p = wgrad_plan(R, Cin, Cout, D * H * W);
  return kBoundBytes + (p.slices > 1 ? m3d::align_up((size_t)p.slices * ((size_t)Cin * 8 * Cout + Cout) * sizeof(float), 16) : 0);
}

M3D_API int m3d_upconv3d_2x_dgrad_f16x2(const float* d_gy, const float* d_y_mask, const float* d_weight, float* d_gx, int R, int Cin,
                                        int Cout, int D, int H, int W, const float* d_gy_max, const float* d_w_max, void* d_ws,
                                        size_t ws_bytes, void* stream) {
  if (bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (R == 0) return M3D_OK;                                       // nothing to write: no pointer is looked at
  if (!supported(R, Cin, Cout, D, H, W)) return M3D_EUNSUPPORTED;  // the shape first: a refusal needs no pointer
  if (!d_gy || !d_weight || !d_gx || !d_ws) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_y_mask, 3) || misaligned(d_weight, 3) || misaligned(d_gx, 3) || misaligned(d_ws, 3) ||
      misaligned(d_gy_max, 3) || misaligned(d_w_max, 3))
    return M3D_EINVAL;
  if (misaligned(d_gy, 15) || misaligned(d_y_mask, 15) || misaligned(d_weight, 15) || misaligned(d_ws, 15)) return M3D_EUNSUPPORTED;
  if (ws_bytes < m3d_upconv3d_2x_dgrad_f16x2_workspace_bytes(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  const int V = D * H * W;
  const BPlan p = dgrad_plan(Cout);
  UbArgs a{};
  a.gy = d_gy; a.ym = d_y_mask; a.b = d_weight; a.out = d_gx; a.gy_bound = d_gy_max; a.b_bound = d_w_max;
  a.R = R; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W; a.V = V; a.cols = R * V;
  a.slices = 1; a.chunks = p.chunks;
  if (const int rc = sweep_bounds(a, (long long)R * Cout * 8 * V, (long long)Cin * Cout * 8, d_ws, stream)) return rc;
  const dim3 grid((unsigned)((a.cols + DG_VT - 1) / DG_VT), (unsigned)((Cin / 32 + DG_CB - 1) / DG_CB));
  const size_t lds = sizeof(u32x4) * 2 * 2 * 4 * DG_VT;
  auto kern = p.folds ? upconv_dgrad_f16_kernel<true> : upconv_dgrad_f16_kernel<false>;
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, m3d::as_stream(stream), a);
  return m3d::check_launch("upconv3d_2x_dgrad_f16x2");
}

M3D_API int m3d_upconv3d_2x_wgrad_f16x2(const float* d_gy, const float* d_y_mask, const float* d_x, float* d_gw, float* d_gb, int R,
                                        int Cin, int Cout, int D, int H, int W, const float* d_gy_max, const float* d_x_max, void* d_ws,
                                        size_t ws_bytes, void* stream) {
  if (bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (!supported(R > 0 ? R : 1, Cin, Cout, D, H, W)) return M3D_EUNSUPPORTED;    // the shape first: a refusal needs no pointer
  if (!d_gw || (R > 0 && (!d_gy || !d_x || !d_ws))) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_y_mask, 3) || misaligned(d_x, 3) || misaligned(d_gw, 3) || misaligned(d_gb, 3) ||
      misaligned(d_ws, 3) || misaligned(d_gy_max, 3) || misaligned(d_x_max, 3))
    return M3D_EINVAL;
  if (misaligned(d_gw, 15) || (R > 0 && (misaligned(d_gy, 15) || misaligned(d_y_mask, 15) || misaligned(d_ws, 15)))) return M3D_EUNSUPPORTED;
  hipStream_t st = m3d::as_stream(stream);
  if (R == 0) {                                                    // an empty batch: torch's gradients are zeros
    if (hipMemsetAsync(d_gw, 0, (size_t)Cin * Cout * 8 * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    if (d_gb && hipMemsetAsync(d_gb, 0, (size_t)Cout * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    return M3D_OK;
  }
  if (ws_bytes < m3d_upconv3d_2x_wgrad_f16x2_workspace_bytes(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  const int V = D * H * W;
  const BPlan p = wgrad_plan(R, Cin, Cout, V);
  float* part = (float*)((char*)d_ws + kBoundBytes);
  UbArgs a{};
  a.gy = d_gy; a.ym = d_y_mask; a.b = d_x; a.out = d_gw; a.part = part; a.gb = d_gb;
  a.gb_part = part + (size_t)p.slices * Cin * 8 * Cout;
  a.gy_bound = d_gy_max; a.b_bound = d_x_max;
  a.R = R; a.Cin = Cin; a.Cout = Cout; a.D = D; a.H = H; a.W = W; a.V = V; a.cols = R * V;
  a.rt = p.rt; a.kt = p.kt; a.slices = p.slices; a.chunks = p.chunks; a.per_xcd = p.per_xcd;
  if (const int rc = sweep_bounds(a, (long long)R * Cout * 8 * V, (long long)R * Cin * V, d_ws, stream)) return rc;
  const size_t lds = sizeof(u32x4) * 2 * WG_STAGE;
  auto kern = p.folds ? upconv_wgrad_f16_kernel<true> : upconv_wgrad_f16_kernel<false>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3(8 * p.per_xcd), dim3(256), lds, st, a);
  if (p.slices > 1) {
    const long long total = (long long)Cin * 8 * Cout;
    long long blocks = (total / 4 + 255) / 256;
    blocks = blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(upconv_bwd_f16_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)a.part, a.out, total, p.slices,
                       (const float*)a.gb_part, a.gb, Cout);
  }
  return m3d::check_launch("upconv3d_2x_wgrad_f16x2");
}
