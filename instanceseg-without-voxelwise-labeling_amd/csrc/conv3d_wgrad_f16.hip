// 3x3x3 convolution backward-weights (stride 1, pad 1) on the f16 matrix cores at fp32 accuracy: the "f16x2" cut of fc_gemm.hip /
// conv3d_zw.hip (both operands scaled by a power of two and cut into two fp16 numbers, 22 bits; three v_mfma_f32_32x32x16_f16 per fp32
// product, fp32 accumulation) applied to
//   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+dz-1,y+dy-1,x+dx-1]
// the gradient autograd computes for every 3^3 nn.Conv3d of lib/modeling/DSN.py:19-36 during training.  cin and cout multiples of 32.
//
// GEMM view per tap: M = cout (32 per workgroup), N = cin (32 per workgroup), K = voxels.  Voxels are the contiguous dimension of both
// operands, so a k-step of 16 is one 16-voxel x row of the tile and lane (r, h) of the MFMA takes the 8 consecutive x of its half:
// one aligned ds_read_b128 from a [channel][row][16 x] fp16 image, no transposed read.
//
// Workgroup = (split-K slot, cout block, cin block), 3 waves, wave = dz: it holds the 9 accumulators of its (dy, dx) taps.  A tile is
// 2 x 4 x 16 voxels (z, y, x); per tile the workgroup stages gy[32 co][8 rows] and the halo tile x[32 ci][4 x 6 rows][x0 - 1 .. x0 + 16],
// CUT ONCE while staging, as separate hi and lo fp16 images.  A dz / dy shift is another row of the halo image.
//
// The +-1 shift along x (dx = 0, 2) is built in registers: a row of the x image is its 16 aligned voxels (32 bytes) and, apart, one
// "edge" dword per row = (x[x0 - 1] << 16) | x[x0 + 16].  A lane reads its aligned 8 halves (ds_read_b128), the dword before them (the
// other half's last dword, or the edge) and the dword behind them, and shifts by 16 bits across the five dwords: 4 v_alignbit per shifted
// 8-half fragment, in the MFMAs' shadow.  Shifted copies of the image would have cost 3 x the 55 KB of the x image; as it is the workgroup
// holds 72 KB and two of them share a CU.  Channel pitches are odd multiples of 16 bytes: every 16-lane group of a ds_read_b128 covers
// the 64 banks once.
//
// Accumulation chain: the f16 MFMA truncates when it adds into its accumulator (conv3d_zw.hip), so no accumulator takes more than
// WF_CHAIN = 384 consecutive MFMAs: a slot is at most 16 tiles (8 rows x 3 products = 24 MFMAs per accumulator and tile), then the
// workgroup ends and writes its partial.  The second level is the split-K workspace: the reduce kernel adds the partials with fp32
// round-to-nearest adds in a fixed order (8 strided groups per output, then the 8 group sums in order) and multiplies by 1 / s_g and
// 1 / s_x once (exact).  A second register set per wave would have been 144 more registers, one wave per SIMD instead of two; the
// workspace costs 110 KB written and read per 16 tiles (2048 voxels x 64 channels x 4 bytes = 512 KB of operands, before the halo).
// No atomics: bit-identical run to run.
// The cut, the MFMA triple and the bound slots are those of f16x2.h; the partial store, the reduce kernel and the slot rule those of
// conv3d_wgrad_f16_common.h.
#include "conv3d_wgrad_f16_common.h"

namespace {

constexpr int WF_NT = 192;                                  // 3 waves: wave = dz
constexpr int TZ = 2, TY = 4, TX = 16;                      // voxel tile: 8 rows = 8 k-steps of 16
constexpr int GROWS = TZ * TY, HZ = TZ + 2, HY = TY + 2, XROWS = HZ * HY;
constexpr int MFMA_PER_TILE = GROWS * 3;                    // per accumulator: 8 k-steps x (hh + hl + lh)
constexpr int WF_CHAIN = WG_MAX_TILES * MFMA_PER_TILE;      // 384: the longest run of MFMAs into one accumulator
static_assert(WF_CHAIN <= 512, "chain");
constexpr long long WF_MAX_WGS = 0xFFFFFFFFll / WF_NT;      // a launch takes fewer than 2^32 threads
constexpr int EDGE_OFF = XROWS * 32;                        // edge dwords of a channel behind its rows
constexpr int XP = EDGE_OFF + XROWS * 4 + 16;               // 880: channel pitch of the x image
constexpr int GP = GROWS * 32 + 16;                         // 272: channel pitch of the gy image
static_assert((XP / 16) % 2 == 1 && (GP / 16) % 2 == 1 && XP % 16 == 0 && GP % 16 == 0, "odd multiples of 16 bytes");
constexpr int X_PART = 32 * XP, G_PART = 32 * GP;
constexpr int LDS_BYTES = 2 * X_PART + 2 * G_PART;          // [x hi][x lo][gy hi][gy lo] = 73,728
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
constexpr int X_ITEMS = 32 * XROWS * 6, G_ITEMS = 32 * GROWS * 4;
static_assert(X_ITEMS % WF_NT == 0, "x staging items per thread");

struct WfPlan { int tiles_x, tiles_y, tiles_z, NT, cbs, ibs, tps, slots; long long n; };

// four consecutive x of one row, zeros outside [0, W); p points at column xf of the row (never dereferenced outside the row)
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ p, int xf, int W, bool row_ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row_ok) {
    if (xf >= 0 && xf + 3 < W) {
      v = *reinterpret_cast<const f32x4u*>(p);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((unsigned)(xf + j) < (unsigned)W) v[j] = p[j];
    }
  }
  return v;
}

// partial[slot][tap][co][ci] in scaled units
__global__ __launch_bounds__(WF_NT, 2) void conv3d_wgrad_f16_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                    float* __restrict__ partial, const float* __restrict__ x_max,
                                                                    const float* __restrict__ g_max, int B, int cin, int cout, int D,
                                                                    int H, int W, WfPlan pl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* const xh = lds;
  unsigned char* const xl = lds + X_PART;
  unsigned char* const gh = lds + 2 * X_PART;
  unsigned char* const gl = gh + G_PART;
  const int tid = threadIdx.x, lane = tid & 63;
  const int dz = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = blockIdx.x;
  const int ib = bid % pl.ibs; bid /= pl.ibs;
  const int cb = bid % pl.cbs;
  const int slot = bid / pl.cbs;
  const size_t HW = (size_t)H * W, DHW = HW * D;

  float sx, sg, inv_;
  f16_scale_of(bound_of_slots(x_max, lane), sx, inv_);
  f16_scale_of(bound_of_slots(g_max, lane), sg, inv_);

  f32x16 acc[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  const int r = lane & 31, h = lane >> 5;
  const int xmain = r * XP + 16 * h;
  const int xprev = r * XP + (h ? 12 : EDGE_OFF), xprev_st = h ? 32 : 4;      // the dword before the lane's 8 halves
  const int xnext = r * XP + (h ? EDGE_OFF : 16), xnext_st = h ? 4 : 32;      // the dword behind them
  const int gmain = r * GP + 16 * h;

  const int t_end = min(pl.NT, (slot + 1) * pl.tps);
  for (int t = slot * pl.tps; t < t_end; ++t) {
    int q = t;
    const int x0 = (q % pl.tiles_x) * TX; q /= pl.tiles_x;
    const int y0 = (q % pl.tiles_y) * TY; q /= pl.tiles_y;
    const int z0 = (q % pl.tiles_z) * TZ;
    const int b = q / pl.tiles_z;
    __syncthreads();                                   // the previous tile's MFMAs have read the images
    // ---- gy[cb * 32 + c][row][x0 + 4 q ..]: one quad per item, cut, 8 bytes to each image
    {
      const float* gb = gy + ((size_t)b * cout + (size_t)cb * 32) * DHW;
      for (int e = tid; e < G_ITEMS; e += WF_NT) {
        const int qq = e & 3, row = (e >> 2) & 7, c = e >> 5;
        const int zz = z0 + (row >> 2), yy = y0 + (row & 3), xf = x0 + 4 * qq;
        const bool rok = (zz < D) & (yy < H);
        const f32x4 v = load_quad(gb + (size_t)c * DHW + (size_t)zz * HW + (size_t)yy * W + xf, xf, W, rok);
        _Float16 hh[4], ll[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cut(v[j], sg, hh[j], ll[j]);
        const int off = c * GP + row * 32 + qq * 8;
        *reinterpret_cast<u32x2*>(gh + off) = u32x2{pack2(hh[0], hh[1]), pack2(hh[2], hh[3])};
        *reinterpret_cast<u32x2*>(gl + off) = u32x2{pack2(ll[0], ll[1]), pack2(ll[2], ll[3])};
      }
    }
    // ---- x[ib * 32 + c][halo row][x0 - 4 + 4 q ..]: q = 1..4 the row's 16 aligned voxels, q = 0 / 5 the two edge voxels
    {
      const float* xb = x + ((size_t)b * cin + (size_t)ib * 32) * DHW;
#pragma unroll 4
      for (int u = 0; u < X_ITEMS / WF_NT; ++u) {
        const int e = tid + u * WF_NT;
        const int qq = e % 6, row = (e / 6) % XROWS, c = e / (6 * XROWS);
        const int zz = z0 + row / HY - 1, yy = y0 + row % HY - 1;
        const bool rok = ((unsigned)zz < (unsigned)D) & ((unsigned)yy < (unsigned)H);
        const float* rp = xb + (size_t)c * DHW + (rok ? (size_t)zz * HW + (size_t)yy * W : 0);
        if (qq >= 1 && qq <= 4) {
          const int xf = x0 - 4 + 4 * qq;
          const f32x4 v = load_quad(rp + xf, xf, W, rok);
          _Float16 hh[4], ll[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) cut(v[j], sx, hh[j], ll[j]);
          const int off = c * XP + row * 32 + (qq - 1) * 8;
          *reinterpret_cast<u32x2*>(xh + off) = u32x2{pack2(hh[0], hh[1]), pack2(hh[2], hh[3])};
          *reinterpret_cast<u32x2*>(xl + off) = u32x2{pack2(ll[0], ll[1]), pack2(ll[2], ll[3])};
        } else {
          const int xx = qq == 0 ? x0 - 1 : x0 + TX;
          const float v = (rok && (unsigned)xx < (unsigned)W) ? rp[xx] : 0.f;
          _Float16 hh, ll;
          cut(v, sx, hh, ll);
          const int off = c * XP + EDGE_OFF + row * 4 + (qq == 0 ? 2 : 0);     // edge dword = (left << 16) | right
          *reinterpret_cast<_Float16*>(xh + off) = hh;
          *reinterpret_cast<_Float16*>(xl + off) = ll;
        }
      }
    }
    __syncthreads();
    // ---- MFMA: k-step = one x row of the tile; A = gy[co = r][8 h ..], B = x[ci = r][8 h + dx - 1 ..] of halo row (tz + dz, ty + dy)
#pragma unroll 2
    for (int grow = 0; grow < GROWS; ++grow) {
      const int tz = grow >> 2, ty = grow & 3;
      const f16x8 ah = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(gh + gmain + grow * 32));
      const f16x8 al = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(gl + gmain + grow * 32));
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int hr = (tz + dz) * HY + ty + dy;
        u32x4 w[2], f0[2], f2[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const unsigned char* im = p ? xl : xh;
          w[p] = *reinterpret_cast<const u32x4*>(im + xmain + hr * 32);
          const unsigned pv = *reinterpret_cast<const unsigned*>(im + xprev + hr * xprev_st);
          const unsigned nx = *reinterpret_cast<const unsigned*>(im + xnext + hr * xnext_st);
          f0[p][0] = __builtin_amdgcn_alignbit(w[p][0], pv, 16);
          f0[p][1] = __builtin_amdgcn_alignbit(w[p][1], w[p][0], 16);
          f0[p][2] = __builtin_amdgcn_alignbit(w[p][2], w[p][1], 16);
          f0[p][3] = __builtin_amdgcn_alignbit(w[p][3], w[p][2], 16);
          f2[p][0] = __builtin_amdgcn_alignbit(w[p][1], w[p][0], 16);
          f2[p][1] = __builtin_amdgcn_alignbit(w[p][2], w[p][1], 16);
          f2[p][2] = __builtin_amdgcn_alignbit(w[p][3], w[p][2], 16);
          f2[p][3] = __builtin_amdgcn_alignbit(nx, w[p][3], 16);
        }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const f16x8 bh = __builtin_bit_cast(f16x8, dx == 0 ? f0[0] : dx == 1 ? w[0] : f2[0]);
          const f16x8 bl = __builtin_bit_cast(f16x8, dx == 0 ? f0[1] : dx == 1 ? w[1] : f2[1]);
          mfma3(ah, al, bh, bl, acc[dy][dx]);
        }
      }
    }
  }
  store_partial(partial + (size_t)slot * pl.n, acc, dz, cb, ib, r, h, cin, cout);
}

bool wf_supported(int batch, int cin, int cout, int D, int H, int W) {
  if (!extents_ok(batch, cin, cout, D, H, W)) return false;
  if (cin % 32 || cout % 32 || cin > 4096 || cout > 4096) return false;
  const long long tz = ((long long)D + TZ - 1) / TZ, ty = ((long long)H + TY - 1) / TY, tx = ((long long)W + TX - 1) / TX;
  if (tz * ty > (1ll << 30) || tz * ty * tx > (1ll << 30)) return false;       // each product below 2^61
  return (long long)batch * (tz * ty * tx) <= (1ll << 30);
}

WfPlan wf_plan(int batch, int cin, int cout, int D, int H, int W) {
  WfPlan p;
  p.tiles_x = (W + TX - 1) / TX; p.tiles_y = (H + TY - 1) / TY; p.tiles_z = (D + TZ - 1) / TZ;
  p.NT = batch * p.tiles_x * p.tiles_y * p.tiles_z;
  slot_rule(p, cin, cout);
  return p;
}

}  // namespace

M3D_API int m3d_conv3d_wgrad_f16x2_supported(int batch, int cin, int cout, int depth, int height, int width) {
  if (!wf_supported(batch, cin, cout, depth, height, width)) return 0;
  const WfPlan p = wf_plan(batch, cin, cout, depth, height, width);
  return (long long)p.slots * p.cbs * p.ibs <= WF_MAX_WGS ? 1 : 0;
}

M3D_API size_t m3d_conv3d_wgrad_f16x2_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width) {
  if (!m3d_conv3d_wgrad_f16x2_supported(batch, cin, cout, depth, height, width)) return 0;
  const WfPlan p = wf_plan(batch, cin, cout, depth, height, width);
  return (size_t)p.slots * (size_t)p.n * sizeof(float);
}

M3D_API int m3d_conv3d_wgrad_f16x2_plan(int batch, int cin, int cout, int depth, int height, int width, int* slots, int* tiles_per_slot,
                                        int* chain, int* folds) {
  if (!extents_ok(batch, cin, cout, depth, height, width)) return M3D_EINVAL;
  if (!m3d_conv3d_wgrad_f16x2_supported(batch, cin, cout, depth, height, width)) return M3D_EUNSUPPORTED;
  report_plan(wf_plan(batch, cin, cout, depth, height, width), MFMA_PER_TILE, slots, tiles_per_slot, chain, folds);
  return M3D_OK;
}

M3D_API int m3d_conv3d_wgrad_f16x2(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                   int depth, int height, int width, const float* d_in_max, const float* d_gy_max, void* d_ws,
                                   size_t ws_bytes, void* stream) {
  if (check_args(d_in, d_grad_out, d_grad_weight, d_in_max, d_gy_max, d_ws) != M3D_OK) return M3D_EINVAL;
  if (!extents_ok(batch, cin, cout, depth, height, width)) return M3D_EINVAL;
  if (!m3d_conv3d_wgrad_f16x2_supported(batch, cin, cout, depth, height, width)) return M3D_EUNSUPPORTED;
  if (ws_bytes < m3d_conv3d_wgrad_f16x2_workspace_bytes(batch, cin, cout, depth, height, width)) return M3D_EINVAL;
  const WfPlan p = wf_plan(batch, cin, cout, depth, height, width);
  hipStream_t st = m3d::as_stream(stream);
  float* partial = (float*)d_ws;
  auto kern = conv3d_wgrad_f16_kernel;
  // 72 KB of LDS are above the 64 KB a launch gets unasked.  Per launch, not once: the attribute belongs to the current device's copy
  // of the kernel (a host-side call, no device work)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  const unsigned blocks = (unsigned)((long long)p.slots * p.cbs * p.ibs);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(WF_NT), LDS_BYTES, st, d_in, d_grad_out, partial, d_in_max, d_gy_max, batch, cin, cout,
                     depth, height, width, p);
  int rc = m3d::check_launch("conv3d_wgrad_f16x2");
  if (rc != M3D_OK) return rc;
  hipLaunchKernelGGL(conv3d_wgrad_f16_reduce_kernel, dim3((unsigned)(p.n / 32)), dim3(256), 0, st, partial, p.slots, p.n, cin, cout,
                     d_in_max, d_gy_max, d_grad_weight);
  return m3d::check_launch("conv3d_wgrad_f16x2_reduce");
}
