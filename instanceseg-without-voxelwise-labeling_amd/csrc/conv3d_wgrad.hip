// 3-D convolution backward-weights (wgrad) as an fp32 MFMA implicit GEMM for gfx950, plus the bias gradient.
//   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+d(dz-p),y+d(dy-p),x+d(dx-p)]     (stride 1, dilation d, pad d * (k/2))
// Reference: the gradient autograd computes for F.conv3d in lib/prm/peak_backprop_3d.py:40-42 / every nn.Conv3d of
// lib/modeling/DSN.py:19-36 during training (SURVEY 8b "conv boundary": fwd / dgrad / wgrad), for the per-RoI convs of
// lib/modeling/fast_rcnn_heads.py:120-179 (roi_Xconv1fc_head) and for the nn.Conv3d(dim, dim, 3, 1, padding=d, dilation=d) layers of
// lib/modeling/mask_rcnn_heads.py:141-151 at MRCNN.DILATION = 1 and 2 (lib/core/config.py:767).
//
// GEMM view: M = cout (32 per block), N = cin (32 per block) for one tap, K = voxels (v_mfma_f32_32x32x2f32, k = two
// x-adjacent voxels).  The reduction dimension is the voxel index, which is the CONTIGUOUS dimension of both operands
// in HBM, so both tiles are staged through LDS: coalesced reads along x, written as [channel][voxel] with an odd channel
// stride, then read back with lane = channel (conflict-free ds_read_b32).  One workgroup = (cout block, cin block,
// split-K slot); its 4 waves share the staged tiles and split the k^3 taps (k = 3) or the voxel pairs (k = 1).
// Split-K partials are written to a workspace and summed by a second kernel in a fixed order: deterministic.
//
// One kernel template serves five shapes of that scheme, all on voxel tiles of 128 voxels (64 MFMA k-steps):
//   entry point                   k  d  tile        halo per channel              LDS       workgroups per CU (160 KiB)
//   m3d_conv3d_wgrad              3  1  2 x 4 x 16  4 x  6 x 18            = 432   70.3 KB  2
//   m3d_conv3d_wgrad              1  1  2 x 4 x 16  the tile itself        = 128   32.3 KB  4
//   m3d_conv3d_wgrad_narrow       3  1  2 x 8 x 8   4 x 10 x 10, rows of 12 = 480  76.3 KB  2: one stages while the other multiplies
//   m3d_conv3d_wgrad_dilated      3  2  2 x 4 x 16  6 x  8 x 20            = 960  136.3 KB  1
//   m3d_conv3d_wgrad_dilated      3  2  2 x 8 x 8   6 x 12 x 12            = 864  124.3 KB  1; a 7^3 RoI grid is 4 of these tiles, not 8
// The narrow entry point takes maps at most 8 wide (one tile along x: a 7^3 grid fills 343 of 512 voxel slots, not 343 of 1024); its
// halo rows are padded to three 16-byte quads (x = -1 .. 10; columns 10, 11 are staged, never read).  The dilated entry point picks
// its tile by the width alone.  DESIGN, "Dilated conv backward" and "Conv box head".
#include <limits.h>
#include <stdlib.h>

#include "m3d_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TZ = 2, TV = 128;                              // every voxel tile is 2 x TY x TX = 128 voxels
constexpr int GS = TV + 1;                                   // odd channel stride of the gy tile in LDS

// K: kernel size (3 or 1); DIL: dilation; tile 2 x (1 << TYL) x (1 << TXL); HXS: floats per halo row in LDS (>= TX + 2 P)
// ONE_X: the map is one tile wide, x0 = 0.  The narrow kernel needs it: 200 VGPRs, as the separate kernel it replaces had; 204 without
// MOD_TW: tw = wave % TW, vg = wave / TW, not the shortcut tw = wave, vg = 0 that TW = 4 allows.  The k = 3 kernel of m3d_conv3d_wgrad
//   needs it: on the shortcut 128 -> 256 channels on 16^3 ran 1.07 x as long as before the fold, with MOD_TW 0.96 x
//   (profiles/conv_wgrad_fp32_fold.txt has the table of the forms kept)
template <int K_, int DIL_, int TYL_, int TXL_, int HXS_, bool ONE_X_ = false, bool MOD_TW_ = false>
struct WG {
  static constexpr int K = K_, DIL = DIL_, TYL = TYL_, TXL = TXL_, HXS = HXS_;
  static constexpr bool ONE_X = ONE_X_, MOD_TW = MOD_TW_;
  static constexpr int TY = 1 << TYL, TX = 1 << TXL;
  static_assert(TZ * TY * TX == TV, "a tile is 128 voxels");
  static constexpr int P = DIL * (K / 2), HZ = TZ + 2 * P, HY = TY + 2 * P, HX = TX + 2 * P, HV = HZ * HY * HXS;
  static_assert(HXS >= HX, "a halo row holds the tile and both margins");
  static constexpr int XS = HV | 1;                          // odd channel stride of the x halo tile
  static constexpr int TAPS = K * K * K;
  static constexpr int TW = TAPS >= 4 ? 4 : 1;               // waves splitting the taps
  static constexpr int VG = 4 / TW;                          // waves splitting the voxel pairs
  static_assert(MOD_TW || TW == 4, "the shortcut is for TW = 4");
  static constexpr int NTW = (TAPS + TW - 1) / TW;           // taps per wave (k = 3: 7, 7, 7, 6; the surplus slot is computed, never stored)
  static constexpr int LDS_FLOATS = 32 * GS + 32 * XS;
  static constexpr int QX = (HX + 3) / 4;                    // 16-byte quads per halo row (x0-P .. x0-P+4*QX-1)
  static constexpr bool RAGGED_ROW = 4 * QX > HXS;           // the last quad of a row would run into the next row: guard its stores
  static constexpr int NQX = 32 * HZ * HY * QX;
  static constexpr int UB = NQX % (256 * 5) == 0 ? 5 : NQX % (256 * 4) == 0 ? 4 : 3;   // quads per thread and batch
  static_assert(NQX % (256 * UB) == 0, "no ragged batch");
};
using WgK3 = WG<3, 1, 2, 4, 18, false, true>;   // m3d_conv3d_wgrad, k = 3: unpadded rows of 18, the last quad of a row is cut
using WgK1 = WG<1, 1, 2, 4, 16, false, true>;   // m3d_conv3d_wgrad, k = 1
using WgNarrow = WG<3, 1, 3, 3, 12, true>;   // m3d_conv3d_wgrad_narrow (width <= 8): rows of 10 padded to 12
using WgDil16 = WG<3, 2, 2, 4, 20>;     // m3d_conv3d_wgrad_dilated, width > 8
using WgDil8 = WG<3, 2, 3, 3, 12>;      // m3d_conv3d_wgrad_dilated, width <= 8
// the dynamic LDS of each decides its workgroups per CU
static_assert(WgK3::LDS_FLOATS == 17984 && WgK1::LDS_FLOATS == 8256 && WgNarrow::LDS_FLOATS == 19520 && WgDil16::LDS_FLOATS == 34880 &&
                  WgDil8::LDS_FLOATS == 31808, "LDS footprint");

// partial[slot][co][ci][tap], slot = split * VG + voxel group
template <class C>
__global__ __launch_bounds__(256) void conv3d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                           float* __restrict__ partial, int B, int cin, int cout, int D, int H,
                                                           int W, int tiles_x, int tiles_y, int tiles_z, int S) {
  constexpr int K = C::K, TY = C::TY, TX = C::TX;
  extern __shared__ float lds[];
  float* lds_g = lds;
  float* lds_x = lds + 32 * GS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tw = C::MOD_TW ? wave % C::TW : wave, vg = C::MOD_TW ? wave / C::TW : 0;
  const int ci_blocks = (cin + 31) / 32;
  int bid = blockIdx.x;
  const int ib = bid % ci_blocks; bid /= ci_blocks;
  const int s = bid % S;
  const int cb = bid / S;
  const int NT = B * tiles_z * tiles_y * tiles_x;
  const size_t DHW = (size_t)D * H * W;

  f32x16 acc[C::NTW];
#pragma unroll
  for (int n = 0; n < C::NTW; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  int tapoff[C::NTW];
#pragma unroll
  for (int n = 0; n < C::NTW; ++n) {
    int t = tw + C::TW * n;
    if (t >= C::TAPS) t = C::TAPS - 1;                  // surplus slot of the last wave: computed, never stored
    const int dz = t / (K * K), dy = (t / K) % K, dx = t % K;
    tapoff[n] = C::DIL * ((dz * C::HY + dy) * C::HXS + dx);
  }
  const int cl = lane & 31, kh = lane >> 5;

  for (int t = s; t < NT; t += S) {
    int q = t;
    const int tx = q % tiles_x; q /= tiles_x;
    const int ty = q % tiles_y; q /= tiles_y;
    const int tz = q % tiles_z;
    const int b = q / tiles_z;
    const int x0 = C::ONE_X ? 0 : tx * TX, y0 = ty * TY, z0 = tz * TZ;
    __syncthreads();                                   // the previous tile's MFMAs have read the LDS
    // ---- stage gy[cb*32 + c][tile] and x[ib*32 + c][halo tile] (zero padded) as 16-byte quads of four consecutive x: one
    // buffer_load_dwordx4 each, all loads of a batch issued before the first LDS write.  Rows and columns outside the volume are masked,
    // a quad with nothing to keep is not loaded (offset 0 instead), and no load starts before or ends behind the cin * DHW (cout * DHW)
    // floats of the image it reads.  A channel past the last is not masked: the buffer's range check returns 0 for it, or, where its
    // 32-bit offset wraps, floats of this image; either way they meet only rows and columns of the product that are never stored.
    {
      const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(gy + (size_t)b * cout * DHW), 0, (unsigned)((size_t)cout * DHW * sizeof(float)), 0x00020000);
      constexpr int QG = TX / 4, ROWS = TZ * TY;                       // quads per row, rows per channel
      constexpr int NG = 32 * ROWS * QG / 256;                         // 1024 quads: 4 per thread
      f32x4 v[NG];
      int mk[NG], ld[NG];
#pragma unroll
      for (int u = 0; u < NG; ++u) {
        const int e = tid + u * 256;
        const int q4 = e % QG, row = (e / QG) % ROWS, c = e / (QG * ROWS);
        const int zz = z0 + row / TY, yy = y0 + row % TY, xf = x0 + 4 * q4;
        const bool rok = (zz < D) & (yy < H);
        int m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= (rok && xf + j < W) ? (1 << j) : 0;
        const long long lin = (long long)(cb * 32 + c) * (long long)DHW + ((long long)zz * H + yy) * W + xf;
        mk[u] = m; ld[u] = c * GS + row * TX + 4 * q4;
        v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rg, m ? (int)(lin * 4) : 0, 0, 0));
      }
#pragma unroll
      for (int u = 0; u < NG; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_g[ld[u] + j] = ((mk[u] >> j) & 1) ? v[u][j] : 0.f;
    }
    {
      const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(x + (size_t)b * cin * DHW), 0, (unsigned)((size_t)cin * DHW * sizeof(float)), 0x00020000);
      constexpr int QX = C::QX, UB = C::UB;
#pragma unroll 1
      for (int e0 = 0; e0 < C::NQX; e0 += 256 * UB) {
        f32x4 v[UB];
        int mk[UB], ld[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int e = e0 + u * 256 + tid;
          const int q4 = e % QX, row = (e / QX) % (C::HZ * C::HY), c = e / (QX * C::HZ * C::HY);
          const int hz = row / C::HY, hy = row % C::HY;
          const int zz = z0 + hz - C::P, yy = y0 + hy - C::P, xf = x0 - C::P + 4 * q4;
          const bool rok = ((unsigned)zz < (unsigned)D) & ((unsigned)yy < (unsigned)H);
          int m = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) m |= (rok && xf + j >= 0 && xf + j < W && (!C::RAGGED_ROW || 4 * q4 + j < C::HXS)) ? (1 << j) : 0;
          long long lin = (long long)(ib * 32 + c) * (long long)DHW + ((long long)zz * H + yy) * W + xf;
          // a quad that begins before the image's first float (channel 0, row 0, xf = -P .. -1) would be dropped whole by the range
          // check: load from offset 0 and shift instead (-lin <= P <= 3; P = 1 spelled out: the k = 3, dilation 1 kernels need fewer VGPRs)
          if (C::P > 0 && m && lin < 0) { m |= (C::P == 1 ? 1 : (int)(-lin)) << 4; lin = 0; }
          mk[u] = m; ld[u] = c * C::XS + row * C::HXS + 4 * q4;
          v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, m ? (int)(lin * 4) : 0, 0, 0));
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int sh = mk[u] >> 4;
          f32x4 w4 = v[u];
          if (sh == 1) w4 = f32x4{0.f, w4[0], w4[1], w4[2]};
          else if (sh == 2) w4 = f32x4{0.f, 0.f, w4[0], w4[1]};
          else if (sh == 3) w4 = f32x4{0.f, 0.f, 0.f, w4[0]};
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (!C::RAGGED_ROW || 4 * ((e0 + u * 256 + tid) % QX) + j < C::HXS) lds_x[ld[u] + j] = ((mk[u] >> j) & 1) ? w4[j] : 0.f;
        }
      }
    }
    __syncthreads();
    // ---- MFMA: k-step = voxel pair (v, v+1); A = gy[co = lane%32][v + lane/32], B = x[ci = lane%32][v + lane/32 + DIL * tap]
    const float* ga = lds_g + cl * GS + kh;
    const float* xa = lds_x + cl * C::XS + kh;
#pragma unroll 4
    for (int i = 0; i < TV / 2 / C::VG; ++i) {
      const int v = (vg + i * C::VG) * 2;
      const float a = ga[v];
      const int hb = ((v >> (C::TYL + C::TXL)) * C::HY + ((v >> C::TXL) & (TY - 1))) * C::HXS + (v & (TX - 1));
      float bv[C::NTW];
#pragma unroll
      for (int n = 0; n < C::NTW; ++n) bv[n] = xa[hb + tapoff[n]];
#pragma unroll
      for (int n = 0; n < C::NTW; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[n], acc[n], 0, 0, 0);
    }
  }
  // ---- write this workgroup's partial: acc[i = co][j = ci]; col j = lane&31, row i = (r&3) + 8*(r>>2) + 4*(lane>>5)
  const int slot = s * C::VG + vg;
  float* pp = partial + (size_t)slot * cout * cin * C::TAPS;
  const int ci = ib * 32 + cl;
#pragma unroll
  for (int n = 0; n < C::NTW; ++n) {
    const int tp = tw + C::TW * n;
    if (tp >= C::TAPS) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (co < cout && ci < cin) pp[((size_t)co * cin + ci) * C::TAPS + tp] = acc[n][r];
    }
  }
}

// Stem: cin = 1, k = 5.  N dimension = taps (125 -> 4 blocks of 32, one per wave): B[k][j] = x[v_k + shift(tap_j)].
constexpr int TY = 4, TX = 16;                               // its voxel tile: 2 x 4 x 16
constexpr int SP = 2, SHZ = TZ + 4, SHY = TY + 4, SHX = TX + 4, SHV = SHZ * SHY * SHX;

__global__ __launch_bounds__(256) void conv3d_wgrad_stem5_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                 float* __restrict__ partial, int B, int cout, int D, int H, int W,
                                                                 int tiles_x, int tiles_y, int tiles_z, int S) {
  __shared__ float lds_g[32 * GS];
  __shared__ float lds_x[SHV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bid = blockIdx.x;
  const int s = bid % S;
  const int cb = bid / S;
  const int NT = B * tiles_z * tiles_y * tiles_x;
  const size_t DHW = (size_t)D * H * W;
  const int cl = lane & 31, kh = lane >> 5;
  const int tap = wave * 32 + cl;                       // this lane's tap (column j of the MFMA)
  const bool tap_ok = tap < 125;
  const int tq = tap_ok ? tap : 0;
  const int toff = ((tq / 25) * SHY + (tq / 5) % 5) * SHX + tq % 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int t = s; t < NT; t += S) {
    int q = t;
    const int tx = q % tiles_x; q /= tiles_x;
    const int ty = q % tiles_y; q /= tiles_y;
    const int tz = q % tiles_z;
    const int b = q / tiles_z;
    const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
    __syncthreads();
    for (int e = tid; e < 32 * TV; e += 256) {
      const int c = e / TV, v = e % TV;
      const int xx = x0 + (v & 15), yy = y0 + ((v >> 4) & 3), zz = z0 + (v >> 6);
      const int co = cb * 32 + c;
      float val = 0.f;
      if (co < cout && xx < W && yy < H && zz < D) val = gy[((size_t)b * cout + co) * DHW + ((size_t)zz * H + yy) * W + xx];
      lds_g[c * GS + v] = val;
    }
    for (int r = tid; r < SHV; r += 256) {
      const int hx = r % SHX, hy = (r / SHX) % SHY, hz = r / (SHX * SHY);
      const int xx = x0 + hx - SP, yy = y0 + hy - SP, zz = z0 + hz - SP;
      float val = 0.f;
      if ((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D)
        val = x[(size_t)b * DHW + ((size_t)zz * H + yy) * W + xx];
      lds_x[r] = val;
    }
    __syncthreads();
    const float* ga = lds_g + cl * GS + kh;
#pragma unroll 4
    for (int vp = 0; vp < TV / 2; ++vp) {
      const int v = vp * 2 + kh;
      const float a = ga[vp * 2];
      const int hb = ((v >> 6) * SHY + ((v >> 4) & 3)) * SHX + (v & 15);
      const float bv = tap_ok ? lds_x[hb + toff] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
    }
  }
  float* pp = partial + (size_t)s * cout * 125;
  if (tap_ok) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (co < cout) pp[(size_t)co * 125 + tap] = acc[r];
    }
  }
}

__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int slots, long long n,
                                                           float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int s = 0; s < slots; ++s) sum += partial[(size_t)s * n + i];      // fixed order: deterministic
  dw[i] = sum;
}

// db[co] = sum_{b,v} gy[b,co,v]: one workgroup per channel, fixed-order tree
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* __restrict__ gy, int B, int cout, long long DHW,
                                                        float* __restrict__ db) {
  __shared__ float sm[256];
  const int co = blockIdx.x;
  float sum = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* p = gy + ((size_t)b * cout + co) * DHW;
    for (long long i = threadIdx.x; i < DHW; i += 256) sum += p[i];
  }
  sm[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sm[threadIdx.x] += sm[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) db[co] = sm[0];
}

// ---------------------------------------------------------------------------------------------- host: one plan for every entry point
struct Plan { int tile_x, tile_y, tiles_x, tiles_y, tiles_z, NT, blocks_c, S, slots; long long nt, n; };

// tile_x: 16 (2 x 4 x 16), 8 (2 x 8 x 8) or 0 = by the width alone (what m3d_conv3d_wgrad_dilated takes when it is not told)
Plan make_plan(int batch, int cin, int cout, int D, int H, int W, int k, int tile_x) {
  Plan p;
  if (tile_x == 0) tile_x = (W <= 8) ? 8 : 16;
  p.tile_x = tile_x; p.tile_y = TV / TZ / tile_x;
  p.tiles_x = (W + p.tile_x - 1) / p.tile_x; p.tiles_y = (H + p.tile_y - 1) / p.tile_y; p.tiles_z = (D + TZ - 1) / TZ;
  p.nt = (long long)batch * p.tiles_x * p.tiles_y * p.tiles_z;
  p.NT = (int)p.nt;                                      // what the kernel computes; tile_rc refuses a count that does not fit
  const int cbs = (cout + 31) / 32, ibs = (k == 5) ? 1 : (cin + 31) / 32;
  p.blocks_c = cbs * ibs;
  int S = (1024 + p.blocks_c - 1) / p.blocks_c;          // aim at >= 1024 workgroups (4 per CU)
  if (S > p.NT) S = p.NT;
  if (S < 1) S = 1;
  p.S = S;
  p.slots = (k == 1) ? S * 4 : S;                        // k = 1: the 4 waves split the voxel pairs, one partial each
  p.n = (long long)cout * cin * k * k * k;
  return p;
}

size_t ws_bytes_of(int slots, long long n) { return (size_t)slots * n * sizeof(float) + 256; }

bool extents_ok(int batch, int cin, int cout, int D, int H, int W) {
  return batch > 0 && cin > 0 && cout > 0 && D > 0 && H > 0 && W > 0;
}

// the k = 1 / 3 kernel addresses one image of x and of gy with 32-bit buffer offsets
bool offsets_ok(int cin, int cout, int D, int H, int W) {
  const size_t dhw = (size_t)D * H * W;
  return (size_t)cin * dhw * sizeof(float) < 0x7FFFFFFFull && (size_t)cout * dhw * sizeof(float) < 0x7FFFFFFFull;
}

// what the narrow and the dilated entry points refuse for a shape (M3D_OK: it runs); served: k, dilation, width and tile are theirs
int tile_rc(int batch, int cin, int cout, int D, int H, int W, bool served, int tile_x) {
  if (!extents_ok(batch, cin, cout, D, H, W)) return M3D_EINVAL;
  if (!served || !offsets_ok(cin, cout, D, H, W)) return M3D_EUNSUPPORTED;
  const Plan p = make_plan(batch, cin, cout, D, H, W, 3, tile_x);
  if (p.nt > INT_MAX || (long long)p.blocks_c * p.S > INT_MAX) return M3D_EUNSUPPORTED;
  return M3D_OK;
}
int narrow_rc(int batch, int cin, int cout, int D, int H, int W, int k) {
  return tile_rc(batch, cin, cout, D, H, W, k == 3 && W <= 8, 8);
}
int dilated_rc(int batch, int cin, int cout, int D, int H, int W, int k, int dilation, int tile_x) {
  return tile_rc(batch, cin, cout, D, H, W, k == 3 && dilation == 2 && (tile_x == 0 || tile_x == 8 || tile_x == 16), tile_x);
}
// the larger of the two tiles' needs, so that one workspace serves m3d_conv3d_wgrad_dilated and m3d_conv3d_wgrad_dilated_tile
size_t dilated_ws_bytes(int batch, int cin, int cout, int D, int H, int W) {
  const Plan a = make_plan(batch, cin, cout, D, H, W, 3, 16), b = make_plan(batch, cin, cout, D, H, W, 3, 8);
  return ws_bytes_of(a.S > b.S ? a.S : b.S, a.n);
}

template <class C>
void launch(const float* x, const float* gy, float* partial, int batch, int cin, int cout, int D, int H, int W, const Plan& p,
            hipStream_t st) {
  const size_t lds = sizeof(float) * C::LDS_FLOATS;
  auto kern = conv3d_wgrad_kernel<C>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kern, dim3((unsigned)((long long)p.blocks_c * p.S)), dim3(256), lds, st, x, gy, partial, batch, cin, cout, D, H, W,
                     p.tiles_x, p.tiles_y, p.tiles_z, p.S);
}

// the partials are written: sum them in slot order
int reduce(const Plan& p, const float* partial, float* dw, hipStream_t st, const char* launched, const char* reduced) {
  const int rc = m3d::check_launch(launched);
  if (rc != M3D_OK) return rc;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, st, partial, p.slots, p.n, dw);
  return m3d::check_launch(reduced);
}

}  // namespace

M3D_API size_t m3d_conv3d_wgrad_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width, int k) {
  if (!extents_ok(batch, cin, cout, depth, height, width)) return 0;
  const Plan p = make_plan(batch, cin, cout, depth, height, width, k, 16);
  return ws_bytes_of(p.slots, p.n);
}

M3D_API int m3d_conv3d_wgrad(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                             int depth, int height, int width, int k, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_in || !d_grad_out || !d_grad_weight || !d_ws || !extents_ok(batch, cin, cout, depth, height, width)) return M3D_EINVAL;
  if (!(k == 1 || k == 3 || (k == 5 && cin == 1))) return M3D_EUNSUPPORTED;
  if (k != 5 && !offsets_ok(cin, cout, depth, height, width)) return M3D_EUNSUPPORTED;
  if (ws_bytes < m3d_conv3d_wgrad_workspace_bytes(batch, cin, cout, depth, height, width, k)) return M3D_EWORKSPACE;
  const Plan p = make_plan(batch, cin, cout, depth, height, width, k, 16);
  float* partial = (float*)m3d::align_up((size_t)d_ws, 256);
  hipStream_t st = m3d::as_stream(stream);
  const long long blocks = (long long)p.blocks_c * p.S;
  if (blocks > 0x7FFFFFFFll) return M3D_EUNSUPPORTED;    // the only launch this entry point refuses (the tile count is not checked)
  if (k == 5)
    hipLaunchKernelGGL(conv3d_wgrad_stem5_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_in, d_grad_out, partial, batch, cout,
                       depth, height, width, p.tiles_x, p.tiles_y, p.tiles_z, p.S);
  else if (k == 3)
    launch<WgK3>(d_in, d_grad_out, partial, batch, cin, cout, depth, height, width, p, st);
  else
    launch<WgK1>(d_in, d_grad_out, partial, batch, cin, cout, depth, height, width, p, st);
  return reduce(p, partial, d_grad_weight, st, "conv3d_wgrad", "conv3d_wgrad_reduce");
}

M3D_API int m3d_conv3d_bias_grad(const float* d_grad_out, float* d_grad_bias, int batch, int cout, int depth, int height, int width,
                                 void* stream) {
  if (!d_grad_out || !d_grad_bias || batch <= 0 || cout <= 0 || depth <= 0 || height <= 0 || width <= 0) return M3D_EINVAL;
  hipLaunchKernelGGL(bias_grad_kernel, dim3(cout), dim3(256), 0, m3d::as_stream(stream), d_grad_out, batch, cout,
                     (long long)depth * height * width, d_grad_bias);
  return m3d::check_launch("conv3d_bias_grad");
}

// ---- k = 3, dilation 1, maps at most 8 wide: the 2 x 8 x 8 tile
M3D_API int m3d_conv3d_wgrad_narrow_supported(int batch, int cin, int cout, int depth, int height, int width, int k) {
  return narrow_rc(batch, cin, cout, depth, height, width, k) == M3D_OK;
}

M3D_API size_t m3d_conv3d_wgrad_narrow_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width, int k) {
  if (narrow_rc(batch, cin, cout, depth, height, width, k) != M3D_OK) return 0;
  const Plan p = make_plan(batch, cin, cout, depth, height, width, 3, 8);
  return ws_bytes_of(p.slots, p.n);
}

M3D_API int m3d_conv3d_wgrad_narrow_plan(int batch, int cin, int cout, int depth, int height, int width, int k, int* tile_x_out,
                                         int* tile_y_out, int* slots_out) {
  const int rc = narrow_rc(batch, cin, cout, depth, height, width, k);
  if (rc != M3D_OK) return rc;
  const Plan p = make_plan(batch, cin, cout, depth, height, width, 3, 8);
  if (tile_x_out) *tile_x_out = p.tile_x;
  if (tile_y_out) *tile_y_out = p.tile_y;
  if (slots_out) *slots_out = p.S;
  return M3D_OK;
}

M3D_API int m3d_conv3d_wgrad_narrow(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                    int depth, int height, int width, int k, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_in || !d_grad_out || !d_grad_weight || !d_ws || !extents_ok(batch, cin, cout, depth, height, width)) return M3D_EINVAL;
  const int rc = narrow_rc(batch, cin, cout, depth, height, width, k);
  if (rc != M3D_OK) return rc;
  const Plan p = make_plan(batch, cin, cout, depth, height, width, 3, 8);
  if (ws_bytes < ws_bytes_of(p.slots, p.n)) return M3D_EWORKSPACE;
  float* partial = (float*)m3d::align_up((size_t)d_ws, 256);
  hipStream_t st = m3d::as_stream(stream);
  launch<WgNarrow>(d_in, d_grad_out, partial, batch, cin, cout, depth, height, width, p, st);
  return reduce(p, partial, d_grad_weight, st, "conv3d_wgrad_narrow", "conv3d_wgrad_narrow_reduce");
}

// ---- k = 3, dilation 2 (dilation 1 forwards to m3d_conv3d_wgrad)
M3D_API size_t m3d_conv3d_wgrad_dilated_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width, int k,
                                                        int dilation) {
  if (dilation == 1) return m3d_conv3d_wgrad_workspace_bytes(batch, cin, cout, depth, height, width, k);
  if (dilated_rc(batch, cin, cout, depth, height, width, k, dilation, 0) != M3D_OK) return 0;
  return dilated_ws_bytes(batch, cin, cout, depth, height, width);
}

M3D_API int m3d_conv3d_wgrad_dilated_plan(int batch, int cin, int cout, int depth, int height, int width, int k, int dilation, int tile_x,
                                          int* tile_x_out, int* tile_y_out, int* slots_out) {
  const int rc = dilated_rc(batch, cin, cout, depth, height, width, k, dilation, tile_x);
  if (rc != M3D_OK) return rc;
  const Plan p = make_plan(batch, cin, cout, depth, height, width, 3, tile_x);
  if (tile_x_out) *tile_x_out = p.tile_x;
  if (tile_y_out) *tile_y_out = p.tile_y;
  if (slots_out) *slots_out = p.S;
  return M3D_OK;
}

M3D_API int m3d_conv3d_wgrad_dilated_tile(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                          int depth, int height, int width, int k, int dilation, int tile_x, void* d_ws, size_t ws_bytes,
                                          void* stream) {
  if (!d_in || !d_grad_out || !d_grad_weight || !d_ws || !extents_ok(batch, cin, cout, depth, height, width)) return M3D_EINVAL;
  const int rc = dilated_rc(batch, cin, cout, depth, height, width, k, dilation, tile_x);
  if (rc != M3D_OK) return rc;
  if (ws_bytes < dilated_ws_bytes(batch, cin, cout, depth, height, width)) return M3D_EWORKSPACE;
  const Plan p = make_plan(batch, cin, cout, depth, height, width, 3, tile_x);
  float* partial = (float*)m3d::align_up((size_t)d_ws, 256);
  hipStream_t st = m3d::as_stream(stream);
  if (p.tile_x == 8)
    launch<WgDil8>(d_in, d_grad_out, partial, batch, cin, cout, depth, height, width, p, st);
  else
    launch<WgDil16>(d_in, d_grad_out, partial, batch, cin, cout, depth, height, width, p, st);
  return reduce(p, partial, d_grad_weight, st, "conv3d_wgrad_dilated", "conv3d_wgrad_dilated_reduce");
}

M3D_API int m3d_conv3d_wgrad_dilated(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                     int depth, int height, int width, int k, int dilation, void* d_ws, size_t ws_bytes, void* stream) {
  if (dilation == 1)
    return m3d_conv3d_wgrad(d_in, d_grad_out, d_grad_weight, batch, cin, cout, depth, height, width, k, d_ws, ws_bytes, stream);
  return m3d_conv3d_wgrad_dilated_tile(d_in, d_grad_out, d_grad_weight, batch, cin, cout, depth, height, width, k, dilation, 0, d_ws,
                                       ws_bytes, stream);
}
