// ConvTranspose3d(kernel 2, stride 2, padding 0) of the mask head as fp32 MFMA GEMMs for gfx950, forward and both backward directions, on
// the operands as PyTorch stores them: x [R,Cin,D,H,W], weight [Cin,Cout,2,2,2] (nn.ConvTranspose3d.weight), y / gy [R,Cout,2D,2H,2W].
//
// What it replaces: lib/modeling/mask_rcnn_heads.py:156,193 (upconv + ReLU) and their autograd.  A stride-2 kernel-2 transposed conv never
// overlaps its outputs, so with V = D H W voxels per RoI, n = (co,a,b,c) = 8 co + 4 a + 2 b + c the NC = 8 Cout columns of the weight read
// as a [Cin, NC] matrix, and G[r][n][v] = g[r, co, 2z+a, 2y+b, 2x+c] the "voxel-shuffled" view of the 2x tensor:
//     forward   y-shuffled [r][n][v] = sum_ci W[ci][n] x[r][ci][v]  (+ bias[co], ReLU)       one GEMM per RoI, reduction Cin
//     dgrad     gx[r][ci][v]         = sum_n  W[ci][n] G[r][n][v]                            one GEMM per RoI, reduction NC
//     wgrad     gw[ci][n]            = sum_{r,v} x[r][ci][v] G[r][n][v]                      one GEMM, reduction R V;  gb[co] out of it
// with g = gy [y > 0] where the forward applied ReLU (y: the forward's own output), applied while G is staged.  The shuffled tensor is
// never materialised: the forward's epilogue and the backward's staging address the 2x tensor directly, two x-adjacent floats (c = 0, 1)
// per 8-byte access, neighbouring lanes at neighbouring x - whole output rows are read and written contiguously.
//
// Roofline (soma step, R = 64, 256 channels, 7^3): 23.0 GFLOP per direction = 0.15 ms at the fp32 MFMA rate (157.3 TFLOP/s) against
// 0.035 ms of bytes (22 MB x + 2 MB W + 180 MB y at 6.3 TB/s; the masked backward reads y as well): MFMA-bound in all three directions.
//
// Design (one kernel template, three modes; the structure of fc_backward.hip):
//  * workgroup tile 128 x 128 x 32, 4 waves as 2 x 2, each 64 x 64 = 2 x 2 blocks of v_mfma_f32_32x32x2_f32; double-buffered LDS, one
//    barrier per chunk, the next chunk's global loads issued before the chunk's 64 MFMAs per wave and committed to LDS after them (the
//    zero fill and the ReLU mask are applied at the commit, so nothing waits on a load before the MFMAs);
//  * an operand whose memory rows ARE reduction rows ("reduction-major": W and x in the forward, the gathered G in dgrad) is staged as
//    [32][128] and a fragment is one ds_read_b32 per lane out of one LDS row, conflict-free without padding; an operand that is
//    contiguous along the reduction (W in dgrad, x and G in wgrad) is staged as [128][32 + 4] and read as ds_read_b128 (lane half h holds
//    the reduction indices 4h..4h+3 of an 8-deep group - both layouts use the same permutation, so they mix freely);
//  * x and the 2x tensor are loaded 4 / 8 bytes per lane with neighbouring lanes at neighbouring addresses: V = 343 makes no row of x a
//    16-byte multiple; W (rows of NC = 8 Cout floats) is loaded in 16-byte quads;
//  * reduction indices beyond the end are ZERO in LDS on both operands; output rows / columns beyond the end are clamped at the load and
//    masked at the store: any Cin, Cout, D, H, W >= 1;
//  * dgrad and wgrad: where the output has fewer tiles than the machine has workgroup slots (512) the reduction is cut into `slices`
//    (<= 64, a function of the shape only); partials go to the caller's workspace and a second kernel adds them in slice order.  The
//    forward never splits (reduction Cin, R x 8 Cout / 128 x V / 128 tiles);
//  * gb: the workgroups of the first row tile sum their staged G tile row by row (one thread per n, chunk order, reduction order), the 8
//    parities of a channel are added in n order, slices in slice order: no atomics, no separate pass over gy;
//  * unit order: blockIdx % 8 is the XCD; one XCD gets a contiguous run of units, and inside a column tile the row tiles are neighbours.
#include <initializer_list>

#include "f16x2.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

enum { FWD = 0, DGRAD = 1, WGRAD = 2 };
constexpr int BT = 128, BR = 32, LSA = BR + 4;                    // tile edge, reduction chunk, padded row stride of a reduction-contiguous tile
constexpr int kRM = BR * BT, kRC = BT * LSA;                       // floats of a reduction-major / reduction-contiguous tile
constexpr int kSlots = 512;                                        // resident workgroups: 256 CUs x 2
using m3d::f16x2::acc_row;      // accumulator register g -> row inside a 32x32 block (+4*(lane>>5))

struct UpArgs {
  const float* w; const float* x; const float* g; const float* ym; const float* bias;
  float* out; float* part; float* gb; float* gb_part;
  int R, Cin, Cout, NC, H, W, V;
  int rows, cols;          // one output matrix: (NC, V) forward, (Cin, V) dgrad, (Cin, NC) wgrad
  int batch;               // output matrices: R, R, 1
  int rt, ct, slices, chunks, cpr, per_xcd, relu;
  int tiles;               // batch * rt * ct
};

// offset of output voxel (2z, 2y, 2x) inside one [2D,2H,2W] channel for input voxel v = (z H + y) W + x
__device__ __forceinline__ int up_offset(int v, int H, int W) {
  const int x = v % W, zy = v / W, y = zy % H, z = zy / H;
  return ((2 * z) * (2 * H) + 2 * y) * (2 * W) + 2 * x;
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void upconv_kernel(UpArgs a) {
  constexpr bool A_RM = MODE == FWD, B_RM = MODE != WGRAD;
  constexpr int kAFloats = A_RM ? kRM : kRC, kBFloats = B_RM ? kRM : kRC;
  constexpr int kStage = kAFloats + kBFloats;
  extern __shared__ float lds[];                                   // 2 x [A tile][B tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int u = xcd * a.per_xcd + idx;
  if (idx >= a.per_xcd || (long long)u >= (long long)a.tiles * a.slices) return;
  const int slice = u / a.tiles, t = u - slice * a.tiles;
  const int per = a.rt * a.ct, rb = t / per, t2 = t - rb * per;     // rb: the RoI of this output matrix (0 in wgrad)
  const int tc = t2 / a.rt, tr = t2 - tc * a.rt;                   // row tiles of one column panel are neighbours
  const int r0 = tr * BT, k0 = tc * BT;
  const int c0 = (int)((long long)slice * a.chunks / a.slices), c1 = (int)((long long)(slice + 1) * a.chunks / a.slices);
  const size_t V = (size_t)a.V, NC = (size_t)a.NC;
  const bool has_mask = a.ym != nullptr;

  // ---- staging.  tl = tid % 32 is the contiguous index of every 4- and 8-byte load, th = tid / 32 the row
  const int tl = tid & 31, th = tid >> 5;
  const int aq = tid & 7, arow = tid >> 3;                         // dgrad's W tile: (row = tid/8 + 32 i, quad = tid%8)
  int vcol[4], goff[4];                                            // forward, dgrad: the four voxel columns of this thread, clamped
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    vcol[e] = min(k0 + tl + 32 * e, a.V - 1);
    goff[e] = MODE == DGRAD ? up_offset(vcol[e], a.H, a.W) : 0;
  }
  const int H2W2 = 4 * a.H * a.W, W2 = 2 * a.W;

  f32x4 sa[4];
  f32x4 sb[4];                                                     // forward: 16 floats of x
  f32x2 sg[8], sm[8];                                              // backward: 8 float2 of gy and of the mask
  // loads only, every address clamped into its operand; nothing touches the loaded registers until commit() after the MFMA loop
  auto fetch = [&](int c) __attribute__((always_inline)) {
    if constexpr (MODE == FWD) {
      const int ncol = min(r0 + 4 * tl, a.NC - 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int ci = min(c * BR + th + 8 * i, a.Cin - 1);
        sa[i] = *reinterpret_cast<const f32x4*>(a.w + (size_t)ci * NC + ncol);
        const float* px = a.x + ((size_t)rb * a.Cin + ci) * V;
#pragma unroll
        for (int e = 0; e < 4; ++e) sb[i][e] = px[vcol[e]];
      }
    } else if constexpr (MODE == DGRAD) {
      const int n4 = min(c * BR + 4 * aq, a.NC - 4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        sa[i] = *reinterpret_cast<const f32x4*>(a.w + (size_t)min(r0 + arow + 32 * i, a.Cin - 1) * NC + n4);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int n = c * BR + 2 * (th + 8 * i);
        const size_t base = ((size_t)rb * a.Cout + min(n >> 3, a.Cout - 1)) * 8 * V + ((n >> 2) & 1) * H2W2 + ((n >> 1) & 1) * W2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          sg[4 * i + e] = *reinterpret_cast<const f32x2*>(a.g + base + goff[e]);
          if (has_mask) sm[4 * i + e] = *reinterpret_cast<const f32x2*>(a.ym + base + goff[e]);
        }
      }
    } else {
      const int r = c / a.cpr, v = min((c - r * a.cpr) * BR + tl, a.V - 1);
      const int go = up_offset(v, a.H, a.W);
#pragma unroll
      for (int i = 0; i < 16; ++i) sa[i >> 2][i & 3] = a.x[((size_t)r * a.Cin + min(r0 + th + 8 * i, a.Cin - 1)) * V + v];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int n = k0 + 2 * (th + 8 * i);
        const size_t off = ((size_t)r * a.Cout + min(n >> 3, a.Cout - 1)) * 8 * V + ((n >> 2) & 1) * H2W2 + ((n >> 1) & 1) * W2 + go;
        sg[i] = *reinterpret_cast<const f32x2*>(a.g + off);
        if (has_mask) sm[i] = *reinterpret_cast<const f32x2*>(a.ym + off);
      }
    }
  };
  // registers -> LDS: reduction indices beyond the end become zero on both operands, gy is masked by y > 0
  auto masked = [&](f32x2 gv, f32x2 mv, bool valid) __attribute__((always_inline)) {
    if (has_mask) { gv[0] = mv[0] > 0.f ? gv[0] : 0.f; gv[1] = mv[1] > 0.f ? gv[1] : 0.f; }
    if (!valid) { gv[0] = 0.f; gv[1] = 0.f; }
    return gv;
  };
  auto commit = [&](float* buf, int c) __attribute__((always_inline)) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == FWD) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool valid = c * BR + th + 8 * i < a.Cin;
        *reinterpret_cast<f32x4*>(buf + (th + 8 * i) * BT + 4 * tl) = valid ? sa[i] : z;
#pragma unroll
        for (int e = 0; e < 4; ++e) buf[kAFloats + (th + 8 * i) * BT + tl + 32 * e] = valid ? sb[i][e] : 0.f;
      }
    } else if constexpr (MODE == DGRAD) {
      const bool avalid = c * BR + 4 * aq < a.NC;                   // NC % 8 == 0: a quad is inside or outside as a whole
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(buf + (arow + 32 * i) * LSA + 4 * aq) = avalid ? sa[i] : z;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int p = th + 8 * i;
        const bool valid = c * BR + 2 * p < a.NC;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const f32x2 gv = masked(sg[4 * i + e], sm[4 * i + e], valid);
          buf[kAFloats + (2 * p) * BT + tl + 32 * e] = gv[0];
          buf[kAFloats + (2 * p + 1) * BT + tl + 32 * e] = gv[1];
        }
      }
    } else {
      const int r = c / a.cpr;
      const bool valid = (c - r * a.cpr) * BR + tl < a.V;
#pragma unroll
      for (int i = 0; i < 16; ++i) buf[(th + 8 * i) * LSA + tl] = valid ? sa[i >> 2][i & 3] : 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int p = th + 8 * i;
        const f32x2 gv = masked(sg[i], sm[i], valid);
        buf[kAFloats + (2 * p) * LSA + tl] = gv[0];
        buf[kAFloats + (2 * p + 1) * LSA + tl] = gv[1];
      }
    }
  };

  // ---- fragments: wave (wm, wn) owns rows [wm*64, +64) x cols [wn*64, +64); in the 8-deep group g lane half h holds the reduction
  // indices 8g + 4h + kk, kk = 0..3, on both operands
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 31, fh = lane >> 5;
  const int offA = A_RM ? 4 * fh * BT + wm * 64 + fr : (wm * 64 + fr) * LSA + 4 * fh;
  const int offB = kAFloats + (B_RM ? 4 * fh * BT + wn * 64 + fr : (wn * 64 + fr) * LSA + 4 * fh);
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[i][j][g] = 0.f;
  const bool block_gb = MODE == WGRAD && a.gb != nullptr && tr == 0;     // the first row tile of every column panel sums its G tile
  const bool own_gb = block_gb && tid < BT;                              // waves 0 and 1: one n each
  float gbsum = 0.f;

  auto compute = [&](const float* cur) __attribute__((always_inline)) {
    if constexpr (MODE == WGRAD) {
      if (own_gb) {
#pragma unroll
        for (int q = 0; q < BR / 4; ++q) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(cur + kAFloats + tid * LSA + 4 * q);
          gbsum += v[0]; gbsum += v[1]; gbsum += v[2]; gbsum += v[3];
        }
      }
    }
#pragma unroll
    for (int g = 0; g < BR / 8; ++g) {
      f32x4 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if constexpr (!A_RM) fa[i] = *reinterpret_cast<const f32x4*>(cur + offA + i * 32 * LSA + g * 8);
        if constexpr (!B_RM) fb[i] = *reinterpret_cast<const f32x4*>(cur + offB + i * 32 * LSA + g * 8);
      }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int ro = (8 * g + kk) * BT;
        float va[2], vb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if constexpr (A_RM) va[i] = cur[offA + ro + i * 32];
          else va[i] = fa[i][kk];
          if constexpr (B_RM) vb[i] = cur[offB + ro + i * 32];
          else vb[i] = fb[i][kk];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[i], vb[j], acc[i][j], 0, 0, 0);
      }
    }
  };

  if (c0 < c1) { fetch(c0); commit(lds, c0); }
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    const float* cur = lds + ((c - c0) & 1) * kStage;
    const int cn = c + 1 < c1 ? c + 1 : c;                         // last chunk: harmless re-fetch instead of a branch around the loads
    fetch(cn);
    __builtin_amdgcn_sched_barrier(0);                             // keep the loads in front of the MFMAs
    compute(cur);
    commit(lds + ((c + 1 - c0) & 1) * kStage, cn);
    __syncthreads();
  }

  // ---- epilogue: register g of block (i, j) is row r0 + wm*64 + i*32 + acc_row(g) + 4*fh, column k0 + wn*64 + j*32 + fr
  if constexpr (MODE == FWD) {
    // rows are n = (co,a,b,c): registers g, g+1 (g even) are c = 0, 1 - one float2 of the 2x tensor; lanes are neighbouring x
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = k0 + wn * 64 + j * 32 + fr;
      if (v >= a.V) continue;
      const int vo = up_offset(v, a.H, a.W);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int nb = r0 + wm * 64 + i * 32 + 4 * fh;
#pragma unroll
        for (int g = 0; g < 16; g += 2) {
          const int n = nb + acc_row(g);
          if (n >= a.NC) continue;
          const int co = n >> 3;
          const float bv = a.bias ? a.bias[co] : 0.f;
          f32x2 o = {acc[i][j][g] + bv, acc[i][j][g + 1] + bv};
          if (a.relu) { o[0] = o[0] < 0.f ? 0.f : o[0]; o[1] = o[1] < 0.f ? 0.f : o[1]; }
          *reinterpret_cast<f32x2*>(a.out + ((size_t)rb * a.Cout + co) * 8 * V + ((n >> 2) & 1) * H2W2 + ((n >> 1) & 1) * W2 + vo) = o;
        }
      }
    }
  } else {
    const size_t cols = (size_t)a.cols;
    float* dst = (a.slices == 1 ? a.out : a.part + (size_t)slice * a.batch * a.rows * cols) + (size_t)rb * a.rows * cols;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wn * 64 + j * 32 + fr;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int rbase = r0 + wm * 64 + i * 32 + 4 * fh;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          const int r = rbase + acc_row(g);
          if (r < a.rows && k < a.cols) dst[(size_t)r * cols + k] = acc[i][j][g];
        }
      }
    }
  }
  if constexpr (MODE == WGRAD) {
    if (block_gb) {                                                // block-uniform; the loop's last barrier is behind every read of LDS
      if (own_gb) lds[tid] = gbsum;
      __syncthreads();
      const int co = (k0 >> 3) + tid;
      if (tid < BT / 8 && co < a.Cout) {
        float s = lds[8 * tid];
#pragma unroll
        for (int q = 1; q < 8; ++q) s += lds[8 * tid + q];
        (a.slices == 1 ? a.gb : a.gb_part + (size_t)slice * a.Cout)[co] = s;
      }
    }
  }
}

// out[e] = sum_s part[s][e] and gb[n] = sum_s gb_part[s][n], slices added in index order
__global__ __launch_bounds__(256) void upconv_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, long long total,
                                                            int slices, const float* __restrict__ gb_part, float* __restrict__ gb, int N) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    float v = part[e];
    for (int s = 1; s < slices; ++s) v += part[(size_t)s * total + e];
    out[e] = v;
  }
  if (gb)
    for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
      float v = gb_part[n];
      for (int s = 1; s < slices; ++s) v += gb_part[(size_t)s * N + n];
      gb[n] = v;
    }
}

struct UPlan { int rt, ct, chunks, slices, per_xcd, tiles; };

// The split is a function of the shape only: an output with fewer tiles than the machine has workgroup slots cuts its reduction so that
// the units fill them once - never more than 64 slices, and about four chunks or more per slice (fc_backward.hip's rule).
UPlan make_plan(long long batch, int rows, int cols, long long chunks, bool split) {
  UPlan p;
  p.rt = (rows + BT - 1) / BT; p.ct = (cols + BT - 1) / BT; p.chunks = (int)chunks;
  const long long tiles = batch * p.rt * p.ct;
  long long s = (!split || tiles >= kSlots) ? 1 : kSlots / tiles;
  s = s > 64 ? 64 : s;
  s = s > chunks / 4 + 1 ? chunks / 4 + 1 : s;
  p.slices = s < 1 ? 1 : (int)s;
  p.tiles = (int)tiles;
  p.per_xcd = (int)((tiles * p.slices + 7) / 8);
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

// any operand of 2^31 elements or more (R >= 1): x / gx, y / gy, weight / gw
bool operands_too_big(int R, int Cin, int Cout, int D, int H, int W) {
  return too_big({R, Cin, D, H, W}) || too_big({R, Cout, 8, D, H, W}) || too_big({Cin, Cout, 8});
}

// shapes no call accepts at any R: the workspace functions answer 0 there (and stay non-decreasing in R everywhere else)
bool no_workspace(int Cin, int Cout, int D, int H, int W) {
  return bad_dims(1, Cin, Cout, D, H, W) || too_big({8, D, H, W}) || too_big({Cin, Cout, 8});
}

size_t dgrad_need(int R, int Cin, int Cout, int V) {
  const UPlan p = make_plan(R, Cin, V, (8ll * Cout + BR - 1) / BR, true);
  return p.slices > 1 ? (size_t)p.slices * R * Cin * V * sizeof(float) : 0;
}

template <int MODE>
int launch(UpArgs& a, const UPlan& p, hipStream_t st) {
  a.rt = p.rt; a.ct = p.ct; a.slices = p.slices; a.chunks = p.chunks; a.per_xcd = p.per_xcd; a.tiles = p.tiles;
  const size_t lds = sizeof(float) * 2 * ((MODE == FWD ? kRM : kRC) + (MODE == WGRAD ? kRC : kRM));
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(upconv_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(upconv_kernel<MODE>, dim3(8 * p.per_xcd), dim3(256), lds, st, a);
  if (p.slices > 1) {
    const long long total = (long long)a.batch * a.rows * a.cols;
    long long blocks = (total + 255) / 256;
    blocks = blocks > 4096 ? 4096 : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(upconv_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)a.part, a.out, total, p.slices,
                       (const float*)a.gb_part, a.gb, a.Cout);
  }
  return m3d::check_launch(MODE == FWD ? "upconv3d_2x_forward" : MODE == DGRAD ? "upconv3d_2x_dgrad" : "upconv3d_2x_wgrad");
}

}  // namespace

// The partial sums one output element of the call is added up from (host only): 1 = nothing is split.  0 for a shape the call refuses.
M3D_API int m3d_upconv3d_2x_slices(int kind, int R, int Cin, int Cout, int D, int H, int W) {
  if (kind < FWD || kind > WGRAD || R < 1 || bad_dims(R, Cin, Cout, D, H, W) || operands_too_big(R, Cin, Cout, D, H, W)) return 0;
  const int V = D * H * W, NC = 8 * Cout;
  if (kind == FWD) return 1;
  if (kind == DGRAD) return make_plan(R, Cin, V, (NC + BR - 1) / BR, true).slices;
  return make_plan(1, Cin, NC, (long long)R * ((V + BR - 1) / BR), true).slices;
}

M3D_API int m3d_upconv3d_2x_forward(const float* d_x, const float* d_weight, const float* d_bias, float* d_y, int R, int Cin, int Cout,
                                    int D, int H, int W, int relu, void* stream) {
  if (bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (R == 0) return M3D_OK;                                       // nothing to write: no pointer is looked at
  if (!d_x || !d_weight || !d_y) return M3D_EINVAL;
  if (misaligned(d_x, 3) || misaligned(d_weight, 3) || misaligned(d_bias, 3) || misaligned(d_y, 3)) return M3D_EINVAL;
  if (misaligned(d_x, 15) || misaligned(d_weight, 15) || misaligned(d_y, 15)) return M3D_EUNSUPPORTED;
  if (operands_too_big(R, Cin, Cout, D, H, W)) return M3D_EUNSUPPORTED;
  const int V = D * H * W, NC = 8 * Cout;
  UpArgs a{d_weight, d_x, nullptr, nullptr, d_bias, d_y, nullptr, nullptr, nullptr, R, Cin, Cout, NC, H, W, V, NC, V, R};
  a.cpr = 0; a.relu = relu ? 1 : 0;
  return launch<FWD>(a, make_plan(R, NC, V, (Cin + BR - 1) / BR, false), m3d::as_stream(stream));
}

// Non-decreasing in R: a larger R has more tiles and therefore FEWER slices, so the size asked for is the largest need of any RoI count
// up to R (from 512 RoIs on nothing is split)
M3D_API size_t m3d_upconv3d_2x_dgrad_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W) {
  if (R < 1 || no_workspace(Cin, Cout, D, H, W)) return 0;
  size_t need = 0;
  for (int r = 1; r <= R && r < kSlots; ++r) {
    const size_t n = dgrad_need(r, Cin, Cout, D * H * W);
    need = n > need ? n : need;
  }
  return m3d::align_up(need, 16);
}

M3D_API int m3d_upconv3d_2x_dgrad(const float* d_gy, const float* d_y_mask, const float* d_weight, float* d_gx, int R, int Cin, int Cout,
                                  int D, int H, int W, void* d_ws, size_t ws_bytes, void* stream) {
  if (bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (R == 0) return M3D_OK;                                       // nothing to write: no pointer is looked at
  if (!d_gy || !d_weight || !d_gx) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_y_mask, 3) || misaligned(d_weight, 3) || misaligned(d_gx, 3) || misaligned(d_ws, 3))
    return M3D_EINVAL;
  if (misaligned(d_gy, 15) || misaligned(d_y_mask, 15) || misaligned(d_weight, 15) || misaligned(d_gx, 15)) return M3D_EUNSUPPORTED;
  if (operands_too_big(R, Cin, Cout, D, H, W)) return M3D_EUNSUPPORTED;
  const size_t asked = m3d_upconv3d_2x_dgrad_workspace_bytes(R, Cin, Cout, D, H, W);
  if (asked && (!d_ws || ws_bytes < asked)) return M3D_EINVAL;
  if (asked && misaligned(d_ws, 15)) return M3D_EUNSUPPORTED;
  const int V = D * H * W, NC = 8 * Cout;
  UpArgs a{d_weight, nullptr, d_gy, d_y_mask, nullptr, d_gx, (float*)d_ws, nullptr, nullptr, R, Cin, Cout, NC, H, W, V, Cin, V, R};
  a.cpr = 0; a.relu = 0;
  return launch<DGRAD>(a, make_plan(R, Cin, V, (NC + BR - 1) / BR, true), m3d::as_stream(stream));
}

// The tiles do not depend on R; the chunks, and with them the slices, grow with it
M3D_API size_t m3d_upconv3d_2x_wgrad_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W) {
  if (R < 1 || no_workspace(Cin, Cout, D, H, W)) return 0;
  const long long cpr = ((long long)D * H * W + BR - 1) / BR;
  const UPlan p = make_plan(1, Cin, 8 * Cout, R * cpr, true);
  return p.slices > 1 ? m3d::align_up((size_t)p.slices * ((size_t)Cin * 8 * Cout + Cout) * sizeof(float), 16) : 0;
}

M3D_API int m3d_upconv3d_2x_wgrad(const float* d_gy, const float* d_y_mask, const float* d_x, float* d_gw, float* d_gb, int R, int Cin,
                                  int Cout, int D, int H, int W, void* d_ws, size_t ws_bytes, void* stream) {
  if (bad_dims(R, Cin, Cout, D, H, W)) return M3D_EINVAL;
  if (!d_gw || (R > 0 && (!d_gy || !d_x))) return M3D_EINVAL;
  if (misaligned(d_gy, 3) || misaligned(d_y_mask, 3) || misaligned(d_x, 3) || misaligned(d_gw, 3) || misaligned(d_gb, 3) ||
      misaligned(d_ws, 3))
    return M3D_EINVAL;
  if (misaligned(d_gw, 15) || (R > 0 && (misaligned(d_gy, 15) || misaligned(d_y_mask, 15) || misaligned(d_x, 15)))) return M3D_EUNSUPPORTED;
  if (too_big({Cin, Cout, 8}) || (R > 0 && operands_too_big(R, Cin, Cout, D, H, W))) return M3D_EUNSUPPORTED;
  hipStream_t st = m3d::as_stream(stream);
  if (R == 0) {                                                    // an empty batch: torch's gradients are zeros
    if (hipMemsetAsync(d_gw, 0, (size_t)Cin * Cout * 8 * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    if (d_gb && hipMemsetAsync(d_gb, 0, (size_t)Cout * sizeof(float), st) != hipSuccess) return M3D_ELAUNCH;
    return M3D_OK;
  }
  const size_t asked = m3d_upconv3d_2x_wgrad_workspace_bytes(R, Cin, Cout, D, H, W);
  if (asked && (!d_ws || ws_bytes < asked)) return M3D_EINVAL;
  if (asked && misaligned(d_ws, 15)) return M3D_EUNSUPPORTED;
  const int V = D * H * W, NC = 8 * Cout, cpr = (V + BR - 1) / BR;
  const UPlan p = make_plan(1, Cin, NC, (long long)R * cpr, true);
  float* part = (float*)d_ws;
  UpArgs a{nullptr, d_x, d_gy, d_y_mask, nullptr, d_gw, part, d_gb, part ? part + (size_t)p.slices * Cin * NC : nullptr,
           R, Cin, Cout, NC, H, W, V, Cin, NC, 1};
  a.cpr = cpr; a.relu = 0;
  return launch<WGRAD>(a, p, st);
}
