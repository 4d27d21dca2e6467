// 3x3x3 convolution backward-weights (stride 1, pad 1) on maps at most 8 voxels wide, on the f16 matrix cores at fp32 accuracy: the
// "f16x2" cut of conv3d_wgrad_f16.hip (both operands scaled by a power of two and cut once into two fp16 numbers, three
// v_mfma_f32_32x32x16_f16 per fp32 product, fp32 accumulation) on the 2 x 8 x 8 voxel tile of conv3d_wgrad_narrow.hip:
//   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+dz-1,y+dy-1,x+dx-1]
// the gradient autograd computes for the per-RoI 3^3 convs on 7^3 grids: lib/modeling/fast_rcnn_heads.py:120-179 (roi_Xconv1fc_head)
// and the mask head's convs at MRCNN.DILATION = 1 (lib/modeling/mask_rcnn_heads.py:141-151).  conv3d_wgrad_f16.hip's 2 x 4 x 16 tile
// is a third full on such a grid (343 of 1024 slots); this one holds 343 of 512.
//
// GEMM view per tap as there: M = cout (32 per workgroup), N = cin (32 per workgroup), K = voxels.  Workgroup = (split-K slot, cout
// block, cin block), 3 waves, wave = dz, nine accumulators for its (dy, dx) taps.  A row of the tile is 8 voxels = 16 bytes of fp16,
// so a 16-deep k-step is TWO rows: lane (r, h) takes row (z, y + h), one aligned ds_read_b128 from a [channel][row][8 x] image.  A dz /
// dy shift is another row of the halo image x[32 ci][4 x 10 rows].
//
// The +-1 shift along x needs no edge data: the map is one tile along x and starts at 0, so x = -1 is padding and x = 8 is outside the
// map.  dx = 0 is the lane's eight halves shifted up by one half with a zero shifted in, dx = 2 shifted down with a zero shifted in: 4
// v_alignbit per fragment, no edge dword, no 2-byte LDS access, no halo columns.  Columns >= W are staged as zeros in both images.
//
// LDS: pitches 656 B (x: 40 rows x 16 B + 16) and 272 B (gy: 16 rows x 16 B + 16), odd multiples of 16 bytes, 32 channels x hi / lo of
// each = 59,392 bytes: two workgroups per CU, one stages while the other multiplies.
//
// Accumulation chain and fold as in conv3d_wgrad_f16.hip: a tile is 8 k-steps x 3 products = 24 MFMAs per accumulator, a slot at most
// 16 tiles (WF_CHAIN = 384), then the workgroup writes its partial; the reduce kernel adds the partials with fp32 adds in a fixed
// order (8 strided groups, then the 8 group sums in order) and un-scales by exact powers of two.  No atomics, every element of dW
// written, slots a function of the shape only: bit-identical run to run and on any stream.
// A file of its own so that the code objects of the other wgrad kernels stay what they were.  DESIGN, "Narrow-map wgrad on the f16 pipe".
//
// Dilation 2 (the mask head's convs at MRCNN.DILATION = 2, padding 2; m3d_conv3d_wgrad_narrow_dilated_f16x2) is the second instantiation
// of the same kernel:
//   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+2(dz-1),y+2(dy-1),x+2(dx-1)]
// Three things differ.  The halo: x[32 ci][6 x 12 rows], pitch 1168 B (72 rows x 16 B + 16, still an odd multiple of 16), a tap's row
// is (tz + 2 dz) 12 + ty + 2 dy; LDS 92,160 bytes, one workgroup per CU and launch bounds of its own.  The +-2 shift along x: two halves
// are one dword, so the shifted fragments are whole-dword moves with a zero dword shifted in ({0, w0, w1, w2} and {w1, w2, w3, 0}) - x =
// -2, -1 are padding and x = 8, 9 outside the map, so again no edge data.  The staging: with one workgroup per CU nobody else hides the
// loads, so a thread loads its share of the NEXT tile (12 rows of x, up to 3 of gy, whole 8-voxel rows) into registers before the MFMAs
// of this tile and cuts and writes them behind the next barrier; 356 VGPRs, which one workgroup per CU has.  Tiles, slots, chain and
// folds are those of dilation 1 for the same shape.  DESIGN, "Dilated narrow-map wgrad on the f16 pipe".
// The cut, the MFMA triple and the bound slots are those of f16x2.h; the partial store, the reduce kernel and the slot rule those of
// conv3d_wgrad_f16_common.h.
#include "conv3d_wgrad_f16_common.h"

namespace {

constexpr int WN_NT = 192;                                  // 3 waves: wave = dz
constexpr int TZ = 2, TY = 8, TX = 8;                       // voxel tile: 16 rows = 8 k-steps of two rows
constexpr int MAX_W = TX;
constexpr int GROWS = TZ * TY, KSTEPS = GROWS / 2;
constexpr int MFMA_PER_TILE = KSTEPS * 3;                   // per accumulator: 8 k-steps x (hh + hl + lh)
constexpr int WN_CHAIN = WG_MAX_TILES * MFMA_PER_TILE;      // 384: the longest run of MFMAs into one accumulator
static_assert(WN_CHAIN <= 384, "chain");
constexpr long long WN_MAX_WGS = 0xFFFFFFFFll / WN_NT;      // a launch takes fewer than 2^32 threads
constexpr int GP = GROWS * 16 + 16;                         // 272: channel pitch of the gy image
constexpr int G_PART = 32 * GP;
constexpr int G_ITEMS = 32 * GROWS * 2;                     // quads

// what depends on the dilation: the halo image of x and with it the LDS budget and the occupancy
template <int DIL>
struct Halo {
  static constexpr int HZ = TZ + 2 * DIL, HY = TY + 2 * DIL, XROWS = HZ * HY;      // 4 x 10 = 40 rows; 6 x 12 = 72 rows
  static constexpr int XP = XROWS * 16 + 16;                                       // 656 / 1168: channel pitch of the x image
  static constexpr int X_PART = 32 * XP;
  static constexpr int LDS_BYTES = 2 * X_PART + 2 * G_PART;                        // [x hi][x lo][gy hi][gy lo] = 59,392 / 92,160
  static constexpr int X_ITEMS = 32 * XROWS * 2;                                   // quads
  static constexpr int WGS_PER_CU = DIL == 1 ? 2 : 1;
  static_assert((XP / 16) % 2 == 1 && (GP / 16) % 2 == 1 && XP % 16 == 0 && GP % 16 == 0, "odd multiples of 16 bytes");
  static_assert(WGS_PER_CU * LDS_BYTES <= 160 * 1024, "workgroups per CU");
};
static_assert(Halo<1>::LDS_BYTES == 59392 && Halo<2>::LDS_BYTES == 92160 && Halo<2>::XP == 1168, "LDS budget");

struct WnPlan { int tiles_y, tiles_z, NT, cbs, ibs, tps, slots; long long n; };

// four consecutive x of one row from column xf >= 0, zeros at columns >= W; p points at column xf of the row and is not dereferenced
// outside the row (so no load starts before the image or ends behind it)
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ p, int xf, int W, bool row_ok) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row_ok) {
    if (xf + 3 < W) {
      v = *reinterpret_cast<const f32x4u*>(p);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xf + j < W) v[j] = p[j];
    }
  }
  return v;
}

__device__ __forceinline__ void stage_quad(unsigned char* __restrict__ hi, unsigned char* __restrict__ lo, int off, const f32x4 v, float s) {
  _Float16 hh[4], ll[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) cut(v[j], s, hh[j], ll[j]);
  *reinterpret_cast<u32x2*>(hi + off) = u32x2{pack2(hh[0], hh[1]), pack2(hh[2], hh[3])};
  *reinterpret_cast<u32x2*>(lo + off) = u32x2{pack2(ll[0], ll[1]), pack2(ll[2], ll[3])};
}

// partial[slot][tap][co][ci] in scaled units
template <int DIL>
__global__ __launch_bounds__(WN_NT, Halo<DIL>::WGS_PER_CU) void conv3d_wgrad_narrow_f16_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                           float* __restrict__ partial, const float* __restrict__ x_max,
                                                                           const float* __restrict__ g_max, int B, int cin, int cout,
                                                                           int D, int H, int W, WnPlan pl) {
  constexpr int HY = Halo<DIL>::HY, XROWS = Halo<DIL>::XROWS, XP = Halo<DIL>::XP, X_PART = Halo<DIL>::X_PART, X_ITEMS = Halo<DIL>::X_ITEMS;
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
  const int xmain = r * XP + 16 * h;                   // half h = 1 reads the row below: y + 1
  const int gmain = r * GP + 16 * h;

  const int t_end = min(pl.NT, (slot + 1) * pl.tps);

  // Dilation 2 stages whole 8-voxel rows from registers that were loaded a tile ahead (one workgroup per CU: nobody else hides the
  // loads).  A thread's x rows are rc = tid + 192 i of the 32 x 72, i = 3 m + k: 192 x 3 = 8 x 72, so (channel, row) = divmod(tid +
  // 192 k, 72) + (8 m, 0) - three rows per thread, each in four channels; its gy rows rc = tid + 192 i < 512, (channel, row) =
  // (rc >> 4, rc & 15).  The row decode and its 64-bit address are worked out three times per tile, not once per quad.
  constexpr bool AHEAD = DIL == 2;
  constexpr int XK = 3, XM = 4, XCS = 8, GI = 3;
  static_assert(!AHEAD || (WN_NT * XK == XCS * XROWS && XCS * XM == 32 && WN_NT * GI >= 32 * GROWS), "row map of the look-ahead");
  [[maybe_unused]] f32x4 xq[AHEAD ? XK : 1][AHEAD ? XM : 1][2], gq[AHEAD ? GI : 1][2];
  [[maybe_unused]] bool xok[XK], gok[GI];
  [[maybe_unused]] int xc[XK], xr[XK];
  if constexpr (AHEAD) {
#pragma unroll
    for (int k = 0; k < XK; ++k) {
      xc[k] = (tid + WN_NT * k) / XROWS;
      xr[k] = (tid + WN_NT * k) % XROWS;
    }
  }
  // the loads of tile t; a row outside the map reads row 0 of its channel instead and is staged as zeros
  [[maybe_unused]] auto load_ahead = [&](int t) {
    int q = t;
    const int y0 = (q % pl.tiles_y) * TY; q /= pl.tiles_y;
    const int z0 = (q % pl.tiles_z) * TZ;
    const int b = q / pl.tiles_z;
    const float* gb = gy + ((size_t)b * cout + (size_t)cb * 32) * DHW;
#pragma unroll
    for (int i = 0; i < GI; ++i) {
      const int rc = tid + WN_NT * i, row = rc & (GROWS - 1), c = rc < 32 * GROWS ? rc >> 4 : 0;
      const int zz = z0 + (row >> 3), yy = y0 + (row & 7);
      gok[i] = (zz < D) & (yy < H);
      const float* rp = gb + (size_t)c * DHW + (gok[i] ? (size_t)zz * HW + (size_t)yy * W : 0);
      gq[i][0] = load_quad(rp, 0, W, true);
      gq[i][1] = load_quad(rp + 4, 4, W, 4 < W);
    }
    const float* xb = x + ((size_t)b * cin + (size_t)ib * 32) * DHW;
#pragma unroll
    for (int k = 0; k < XK; ++k) {
      const int zz = z0 + xr[k] / HY - DIL, yy = y0 + xr[k] % HY - DIL;
      xok[k] = ((unsigned)zz < (unsigned)D) & ((unsigned)yy < (unsigned)H);
      const float* rp = xb + (size_t)xc[k] * DHW + (xok[k] ? (size_t)zz * HW + (size_t)yy * W : 0);
#pragma unroll
      for (int m = 0; m < XM; ++m) {
        xq[k][m][0] = load_quad(rp + (size_t)(XCS * m) * DHW, 0, W, true);
        xq[k][m][1] = load_quad(rp + (size_t)(XCS * m) * DHW + 4, 4, W, 4 < W);
      }
    }
  };
  // one row: 8 voxels cut, 16 bytes to each image
  [[maybe_unused]] auto stage_row = [&](unsigned char* hi, unsigned char* lo, int off, const f32x4 (&v)[2], bool ok, float s) {
    _Float16 hh[8], ll[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cut(ok ? v[j >> 2][j & 3] : 0.f, s, hh[j], ll[j]);
    *reinterpret_cast<u32x4*>(hi + off) = u32x4{pack2(hh[0], hh[1]), pack2(hh[2], hh[3]), pack2(hh[4], hh[5]), pack2(hh[6], hh[7])};
    *reinterpret_cast<u32x4*>(lo + off) = u32x4{pack2(ll[0], ll[1]), pack2(ll[2], ll[3]), pack2(ll[4], ll[5]), pack2(ll[6], ll[7])};
  };
  if constexpr (AHEAD) {
    if (slot * pl.tps < t_end) load_ahead(slot * pl.tps);
  }

  for (int t = slot * pl.tps; t < t_end; ++t) {
    int q = t;
    [[maybe_unused]] const int y0 = (q % pl.tiles_y) * TY; q /= pl.tiles_y;
    [[maybe_unused]] const int z0 = (q % pl.tiles_z) * TZ;
    [[maybe_unused]] const int b = q / pl.tiles_z;
    __syncthreads();                                   // the previous tile's MFMAs have read the images
    if constexpr (AHEAD) {
#pragma unroll
      for (int i = 0; i < GI; ++i) {
        const int rc = tid + WN_NT * i;
        if (rc < 32 * GROWS) stage_row(gh, gl, (rc >> 4) * GP + (rc & (GROWS - 1)) * 16, gq[i], gok[i], sg);
      }
#pragma unroll
      for (int k = 0; k < XK; ++k)
#pragma unroll
        for (int m = 0; m < XM; ++m) stage_row(xh, xl, (xc[k] + XCS * m) * XP + xr[k] * 16, xq[k][m], xok[k], sx);
      __syncthreads();
      if (t + 1 < t_end) load_ahead(t + 1);            // in flight under this tile's MFMAs
    } else {
    // ---- gy[cb * 32 + c][row][4 q ..]: one quad per item, cut, 8 bytes to each image
    {
      const float* gb = gy + ((size_t)b * cout + (size_t)cb * 32) * DHW;
      for (int e = tid; e < G_ITEMS; e += WN_NT) {
        const int qq = e & 1, row = (e >> 1) & (GROWS - 1), c = e >> 5;
        const int zz = z0 + (row >> 3), yy = y0 + (row & 7), xf = 4 * qq;
        const bool rok = (zz < D) & (yy < H);
        const float* rp = gb + (size_t)c * DHW + (rok ? (size_t)zz * HW + (size_t)yy * W : 0);
        stage_quad(gh, gl, c * GP + row * 16 + qq * 8, load_quad(rp + xf, xf, W, rok & (xf < W)), sg);
      }
    }
    // ---- x[ib * 32 + c][halo row][4 q ..]: the row's 8 aligned voxels, no halo columns
    {
      const float* xb = x + ((size_t)b * cin + (size_t)ib * 32) * DHW;
#pragma unroll 2
      for (int e = tid; e < X_ITEMS; e += WN_NT) {
        const int qq = e & 1, rc = e >> 1, row = rc % XROWS, c = rc / XROWS;
        const int zz = z0 + row / HY - DIL, yy = y0 + row % HY - DIL, xf = 4 * qq;
        const bool rok = ((unsigned)zz < (unsigned)D) & ((unsigned)yy < (unsigned)H);
        const float* rp = xb + (size_t)c * DHW + (rok ? (size_t)zz * HW + (size_t)yy * W : 0);
        stage_quad(xh, xl, c * XP + row * 16 + qq * 8, load_quad(rp + xf, xf, W, rok & (xf < W)), sx);
      }
    }
    __syncthreads();
    }
    // ---- MFMA: k-step = rows (2 ks, 2 ks + 1) of the tile; A = gy[co = r][row 2 ks + h][0..7], B = x[ci = r][halo row][DIL (dx - 1) ..]
#pragma unroll 2
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int tz = ks >> 2, ty = (ks & 3) * 2;
      const f16x8 ah = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(gh + gmain + ks * 32));
      const f16x8 al = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(gl + gmain + ks * 32));
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const int hr = (tz + DIL * dz) * HY + ty + DIL * dy;
        u32x4 w[2], f0[2], f2[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const unsigned char* im = p ? xl : xh;
          w[p] = *reinterpret_cast<const u32x4*>(im + xmain + hr * 16);
          if constexpr (DIL == 2) {
            f0[p] = u32x4{0u, w[p][0], w[p][1], w[p][2]};                   // x = -2, -1 are padding: a zero dword shifted in
            f2[p] = u32x4{w[p][1], w[p][2], w[p][3], 0u};                   // x = 8, 9 are outside the map
          } else {
            f0[p][0] = __builtin_amdgcn_alignbit(w[p][0], 0u, 16);          // x = -1 is padding
            f0[p][1] = __builtin_amdgcn_alignbit(w[p][1], w[p][0], 16);
            f0[p][2] = __builtin_amdgcn_alignbit(w[p][2], w[p][1], 16);
            f0[p][3] = __builtin_amdgcn_alignbit(w[p][3], w[p][2], 16);
            f2[p][0] = __builtin_amdgcn_alignbit(w[p][1], w[p][0], 16);
            f2[p][1] = __builtin_amdgcn_alignbit(w[p][2], w[p][1], 16);
            f2[p][2] = __builtin_amdgcn_alignbit(w[p][3], w[p][2], 16);
            f2[p][3] = __builtin_amdgcn_alignbit(0u, w[p][3], 16);          // x = 8 is outside the map
          }
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

bool wn_shape_ok(int batch, int cin, int cout, int D, int H, int W) {
  if (!extents_ok(batch, cin, cout, D, H, W)) return false;
  if (W > MAX_W) return false;
  if (cin % 32 || cout % 32 || cin > 4096 || cout > 4096) return false;
  const long long tz = ((long long)D + TZ - 1) / TZ, ty = ((long long)H + TY - 1) / TY;
  if (tz * ty > (1ll << 30)) return false;                                     // the product below 2^61
  return (long long)batch * (tz * ty) <= (1ll << 30);
}

WnPlan wn_plan(int batch, int cin, int cout, int D, int H) {
  WnPlan p;
  p.tiles_y = (H + TY - 1) / TY; p.tiles_z = (D + TZ - 1) / TZ;
  p.NT = batch * p.tiles_y * p.tiles_z;
  slot_rule(p, cin, cout);
  return p;
}

// the two launches of a call; the shape has passed every check
template <int DIL>
int wn_launch(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout, int depth, int height,
              int width, const float* d_in_max, const float* d_gy_max, float* partial, const WnPlan& p, hipStream_t st) {
  auto kern = conv3d_wgrad_narrow_f16_kernel<DIL>;
  constexpr int LDS_BYTES = Halo<DIL>::LDS_BYTES;
  // 58 KB / 90 KB of LDS: asked for per launch, as conv3d_wgrad_f16.hip does (the attribute belongs to the current device's copy of the kernel)
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  const unsigned blocks = (unsigned)((long long)p.slots * p.cbs * p.ibs);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(WN_NT), LDS_BYTES, st, d_in, d_grad_out, partial, d_in_max, d_gy_max, batch, cin, cout,
                     depth, height, width, p);
  int rc = m3d::check_launch(DIL == 1 ? "conv3d_wgrad_narrow_f16x2" : "conv3d_wgrad_narrow_dilated_f16x2");
  if (rc != M3D_OK) return rc;
  hipLaunchKernelGGL(conv3d_wgrad_f16_reduce_kernel, dim3((unsigned)(p.n / 32)), dim3(256), 0, st, partial, p.slots, p.n, cin,
                     cout, d_in_max, d_gy_max, d_grad_weight);
  return m3d::check_launch(DIL == 1 ? "conv3d_wgrad_narrow_f16x2_reduce" : "conv3d_wgrad_narrow_dilated_f16x2_reduce");
}

}  // namespace

// The entry points that take the dilation (1 or 2) do the work.  The tiles and the slot rule do not depend on it, so the shape checks,
// the plan and the workspace are the same for both.
M3D_API int m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(int batch, int cin, int cout, int depth, int height, int width, int dilation) {
  if (dilation != 1 && dilation != 2) return 0;
  if (!wn_shape_ok(batch, cin, cout, depth, height, width)) return 0;
  const WnPlan p = wn_plan(batch, cin, cout, depth, height);
  return (long long)p.slots * p.cbs * p.ibs <= WN_MAX_WGS ? 1 : 0;
}

M3D_API size_t m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width,
                                                                     int dilation) {
  if (!m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(batch, cin, cout, depth, height, width, dilation)) return 0;
  const WnPlan p = wn_plan(batch, cin, cout, depth, height);
  return (size_t)p.slots * (size_t)p.n * sizeof(float);
}

M3D_API int m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(int batch, int cin, int cout, int depth, int height, int width, int dilation,
                                                       int* tile_z, int* slots, int* tiles_per_slot, int* chain, int* folds) {
  if (!extents_ok(batch, cin, cout, depth, height, width) || dilation < 1) return M3D_EINVAL;
  if (!m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(batch, cin, cout, depth, height, width, dilation)) return M3D_EUNSUPPORTED;
  if (tile_z) *tile_z = TZ;
  report_plan(wn_plan(batch, cin, cout, depth, height), MFMA_PER_TILE, slots, tiles_per_slot, chain, folds);
  return M3D_OK;
}

M3D_API int m3d_conv3d_wgrad_narrow_dilated_f16x2(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin,
                                                  int cout, int depth, int height, int width, int dilation, const float* d_in_max,
                                                  const float* d_gy_max, void* d_ws, size_t ws_bytes, void* stream) {
  if (check_args(d_in, d_grad_out, d_grad_weight, d_in_max, d_gy_max, d_ws) != M3D_OK) return M3D_EINVAL;
  if (!extents_ok(batch, cin, cout, depth, height, width) || dilation < 1) return M3D_EINVAL;
  if (!m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(batch, cin, cout, depth, height, width, dilation)) return M3D_EUNSUPPORTED;
  if (ws_bytes < m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(batch, cin, cout, depth, height, width, dilation)) return M3D_EINVAL;
  const WnPlan p = wn_plan(batch, cin, cout, depth, height);
  hipStream_t st = m3d::as_stream(stream);
  return dilation == 1
             ? wn_launch<1>(d_in, d_grad_out, d_grad_weight, batch, cin, cout, depth, height, width, d_in_max, d_gy_max, (float*)d_ws, p, st)
             : wn_launch<2>(d_in, d_grad_out, d_grad_weight, batch, cin, cout, depth, height, width, d_in_max, d_gy_max, (float*)d_ws, p, st);
}

// The entry points without the argument: dilation 1.
M3D_API int m3d_conv3d_wgrad_narrow_f16x2_supported(int batch, int cin, int cout, int depth, int height, int width) {
  return m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(batch, cin, cout, depth, height, width, 1);
}

M3D_API size_t m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width) {
  return m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(batch, cin, cout, depth, height, width, 1);
}

M3D_API int m3d_conv3d_wgrad_narrow_f16x2_plan(int batch, int cin, int cout, int depth, int height, int width, int* tile_z, int* slots,
                                               int* tiles_per_slot, int* chain, int* folds) {
  return m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(batch, cin, cout, depth, height, width, 1, tile_z, slots, tiles_per_slot, chain, folds);
}

M3D_API int m3d_conv3d_wgrad_narrow_f16x2(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                          int depth, int height, int width, const float* d_in_max, const float* d_gy_max, void* d_ws,
                                          size_t ws_bytes, void* stream) {
  return m3d_conv3d_wgrad_narrow_dilated_f16x2(d_in, d_grad_out, d_grad_weight, batch, cin, cout, depth, height, width, 1, d_in_max,
                                               d_gy_max, d_ws, ws_bytes, stream);
}
