// Backward-weights of the 3x3x3 stride-1 "same" convolution (dilation 1, padding 1) on maps at most 8 voxels wide, as an fp32 MFMA
// implicit GEMM for gfx950:
//   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+dz-1,y+dy-1,x+dx-1]                     (zero outside the volume)
// Reference: the gradient autograd computes for the nn.Conv3d(., CONV_HEAD_DIM, 3, 1, 1) layers of lib/modeling/fast_rcnn_heads.py:
// 120-179 (roi_Xconv1fc_head) and for the mask head's convs at MRCNN.DILATION = 1 (lib/modeling/mask_rcnn_heads.py:141-151), all of
// them per-RoI convs on 7^3 grids.
//
// m3d_conv3d_wgrad has only the 2 x 4 x 16 voxel tile: a 7^3 grid fills 343 of its 1024 voxel slots.  This file is the scheme of
// conv3d_wgrad_dilated.hip (M = 32 cout, N = 32 cin per tap, K = voxel pairs of v_mfma_f32_32x32x2f32, both operands staged through
// LDS as [channel][voxel] with an odd channel stride, the 27 taps split over the 4 waves, split-K partials summed by a second launch
// in slot order) on the 2 x 8 x 8 tile with a 1-voxel halo: 343 of 512 slots.  A map at most 8 wide is one tile along x.
//   halo 4 x 10 x 10, kept with a row stride of 12 floats (three 16-byte quads: x = -1 .. 10; columns 10, 11 are staged, never read)
//   LDS 32 * 129 + 32 * 481 floats = 76.25 KB: two workgroups per CU (160 KiB), so one stages while the other multiplies
// It lives in a file of its own so that the code objects of the other two wgrad kernels stay what they were.  DESIGN, "Conv box head".
#include "m3d_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int K = 3, TAPS = 27, TW = 4, NTW = 7;          // taps per wave: 7, 7, 7, 6 (the surplus slot is computed, never stored)
constexpr int TZ = 2, TY = 8, TX = 8, TV = TZ * TY * TX;  // 128 voxels = 64 MFMA k-steps
constexpr int GS = TV + 1;                                // odd gy channel stride
constexpr int HZ = TZ + 2, HY = TY + 2, HXS = 12;         // halo rows of 12 floats: x = -1 .. 10
constexpr int HV = HZ * HY * HXS, XS = HV | 1;            // odd channel stride of the x halo tile
constexpr int LDS_FLOATS = 32 * GS + 32 * XS;
constexpr int MAX_W = TX;

// partial[slot = s][co][ci][tap]
__global__ __launch_bounds__(256) void conv3d_wgrad_narrow_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                  float* __restrict__ partial, int B, int cin, int cout, int D, int H,
                                                                  int W, int tiles_y, int tiles_z, int S) {
  extern __shared__ float lds[];
  float* lds_g = lds;
  float* lds_x = lds + 32 * GS;
  const int tid = threadIdx.x, lane = tid & 63, tw = tid >> 6;
  const int ci_blocks = (cin + 31) / 32;
  int bid = blockIdx.x;
  const int ib = bid % ci_blocks; bid /= ci_blocks;
  const int s = bid % S;
  const int cb = bid / S;
  const int NT = B * tiles_z * tiles_y;
  const size_t DHW = (size_t)D * H * W;

  f32x16 acc[NTW];
#pragma unroll
  for (int n = 0; n < NTW; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  int tapoff[NTW];
#pragma unroll
  for (int n = 0; n < NTW; ++n) {
    int t = tw + TW * n;
    if (t >= TAPS) t = TAPS - 1;
    const int dz = t / (K * K), dy = (t / K) % K, dx = t % K;
    tapoff[n] = (dz * HY + dy) * HXS + dx;
  }
  const int cl = lane & 31, kh = lane >> 5;

  for (int t = s; t < NT; t += S) {
    int q = t;
    const int ty = q % tiles_y; q /= tiles_y;
    const int tz = q % tiles_z;
    const int b = q / tiles_z;
    const int y0 = ty * TY, z0 = tz * TZ;
    __syncthreads();                                   // the previous tile's MFMAs have read the LDS
    // ---- stage gy[cb*32 + c][tile] and x[ib*32 + c][halo tile] (zero padded) as 16-byte quads of four consecutive x, as
    // conv3d_wgrad_dilated.hip does: the buffer's range check returns 0 past the last channel of this image, rows and columns outside
    // the volume are masked, and no load starts before the first float of the image it reads.
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
        const int zz = z0 + row / TY, yy = y0 + row % TY, xf = 4 * q4;
        const bool rok = (zz < D) & (yy < H) & (cb * 32 + c < cout);      // (a channel past the last: its 32-bit offset may wrap)
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
      constexpr int QX = HXS / 4;                                      // quads per halo row (x = -1 .. 10)
      constexpr int NQX = 32 * HZ * HY * QX;                           // 3840 quads = 3 batches of 5 per thread
      constexpr int UB = 5;
      static_assert(NQX % (256 * UB) == 0, "no ragged batch");
#pragma unroll 1
      for (int e0 = 0; e0 < NQX; e0 += 256 * UB) {
        f32x4 v[UB];
        int mk[UB], ld[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int e = e0 + u * 256 + tid;
          const int q4 = e % QX, row = (e / QX) % (HZ * HY), c = e / (QX * HZ * HY);
          const int hz = row / HY, hy = row % HY;
          const int zz = z0 + hz - 1, yy = y0 + hy - 1, xf = 4 * q4 - 1;
          const bool rok = ((unsigned)zz < (unsigned)D) & ((unsigned)yy < (unsigned)H) & (ib * 32 + c < cin);
          int m = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) m |= (rok && xf + j >= 0 && xf + j < W) ? (1 << j) : 0;
          long long lin = (long long)(ib * 32 + c) * (long long)DHW + ((long long)zz * H + yy) * W + xf;
          // the quad that begins one float before the image (channel 0, row 0, xf = -1) would be dropped whole by the range check:
          // load from offset 0 and shift instead
          if (m && lin < 0) { m |= 1 << 4; lin = 0; }
          mk[u] = m; ld[u] = c * XS + row * HXS + 4 * q4;
          v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, m ? (int)(lin * 4) : 0, 0, 0));
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          f32x4 w4 = v[u];
          if (mk[u] >> 4) w4 = f32x4{0.f, w4[0], w4[1], w4[2]};
#pragma unroll
          for (int j = 0; j < 4; ++j) lds_x[ld[u] + j] = ((mk[u] >> j) & 1) ? w4[j] : 0.f;
        }
      }
    }
    __syncthreads();
    // ---- MFMA: k-step = voxel pair (v, v+1); A = gy[co = lane%32][v + lane/32], B = x[ci = lane%32][v + lane/32 + tap]
    const float* ga = lds_g + cl * GS + kh;
    const float* xa = lds_x + cl * XS + kh;
#pragma unroll 4
    for (int i = 0; i < TV / 2; ++i) {
      const int v = i * 2;
      const float a = ga[v];
      const int hb = ((v >> 6) * HY + ((v >> 3) & (TY - 1))) * HXS + (v & (TX - 1));
      float bv[NTW];
#pragma unroll
      for (int n = 0; n < NTW; ++n) bv[n] = xa[hb + tapoff[n]];
#pragma unroll
      for (int n = 0; n < NTW; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[n], acc[n], 0, 0, 0);
    }
  }
  // ---- write this workgroup's partial: acc[i = co][j = ci]; col j = lane&31, row i = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* pp = partial + (size_t)s * cout * cin * TAPS;
  const int ci = ib * 32 + cl;
#pragma unroll
  for (int n = 0; n < NTW; ++n) {
    const int tp = tw + TW * n;
    if (tp >= TAPS) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = cb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (co < cout && ci < cin) pp[((size_t)co * cin + ci) * TAPS + tp] = acc[n][r];
    }
  }
}

__global__ __launch_bounds__(256) void wgrad_narrow_reduce_kernel(const float* __restrict__ partial, int slots, long long n,
                                                                  float* __restrict__ dw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int s = 0; s < slots; ++s) sum += partial[(size_t)s * n + i];      // slot order: deterministic
  dw[i] = sum;
}

struct Plan { int tiles_y, tiles_z, NT, blocks_c, S; long long n; };

Plan make_plan(int batch, int cin, int cout, int D, int H) {
  Plan p;
  p.tiles_y = (H + TY - 1) / TY; p.tiles_z = (D + TZ - 1) / TZ;
  const long long nt = (long long)batch * p.tiles_y * p.tiles_z;
  p.NT = nt > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)nt;
  p.blocks_c = ((cout + 31) / 32) * ((cin + 31) / 32);
  int S = (1024 + p.blocks_c - 1) / p.blocks_c;          // aim at >= 1024 workgroups (2 rounds of 2 per CU), as m3d_conv3d_wgrad does
  if (S > p.NT) S = p.NT;
  if (S < 1) S = 1;
  p.S = S;
  p.n = (long long)cout * cin * TAPS;
  return p;
}

bool extents_ok(int batch, int cin, int cout, int D, int H, int W) {
  return batch > 0 && cin > 0 && cout > 0 && D > 0 && H > 0 && W > 0;
}

// what the launch refuses for its shape (M3D_OK: it runs)
int shape_rc(int batch, int cin, int cout, int D, int H, int W, int k) {
  if (!extents_ok(batch, cin, cout, D, H, W)) return M3D_EINVAL;
  if (k != 3 || W > MAX_W) return M3D_EUNSUPPORTED;
  const size_t dhw = (size_t)D * H * W;                   // one image of x and of gy is addressed with 32-bit buffer offsets
  if ((size_t)cin * dhw * sizeof(float) >= 0x7FFFFFFFull || (size_t)cout * dhw * sizeof(float) >= 0x7FFFFFFFull) return M3D_EUNSUPPORTED;
  const Plan p = make_plan(batch, cin, cout, D, H);
  if ((long long)batch * p.tiles_y * p.tiles_z > 0x7FFFFFFFll || (long long)p.blocks_c * p.S > 0x7FFFFFFFll) return M3D_EUNSUPPORTED;
  return M3D_OK;
}

size_t ws_bytes_of(const Plan& p) { return (size_t)p.S * p.n * sizeof(float) + 256; }

}  // namespace

M3D_API int m3d_conv3d_wgrad_narrow_supported(int batch, int cin, int cout, int depth, int height, int width, int k) {
  return shape_rc(batch, cin, cout, depth, height, width, k) == M3D_OK;
}

M3D_API size_t m3d_conv3d_wgrad_narrow_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width, int k) {
  if (shape_rc(batch, cin, cout, depth, height, width, k) != M3D_OK) return 0;
  return ws_bytes_of(make_plan(batch, cin, cout, depth, height));
}

M3D_API int m3d_conv3d_wgrad_narrow_plan(int batch, int cin, int cout, int depth, int height, int width, int k, int* tile_x_out,
                                         int* tile_y_out, int* slots_out) {
  const int rc = shape_rc(batch, cin, cout, depth, height, width, k);
  if (rc != M3D_OK) return rc;
  const Plan p = make_plan(batch, cin, cout, depth, height);
  if (tile_x_out) *tile_x_out = TX;
  if (tile_y_out) *tile_y_out = TY;
  if (slots_out) *slots_out = p.S;
  return M3D_OK;
}

M3D_API int m3d_conv3d_wgrad_narrow(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                    int depth, int height, int width, int k, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_in || !d_grad_out || !d_grad_weight || !d_ws || !extents_ok(batch, cin, cout, depth, height, width)) return M3D_EINVAL;
  const int rc = shape_rc(batch, cin, cout, depth, height, width, k);
  if (rc != M3D_OK) return rc;
  const Plan p = make_plan(batch, cin, cout, depth, height);
  if (ws_bytes < ws_bytes_of(p)) return M3D_EWORKSPACE;
  float* partial = (float*)m3d::align_up((size_t)d_ws, 256);
  hipStream_t st = m3d::as_stream(stream);
  const size_t lds = sizeof(float) * LDS_FLOATS;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv3d_wgrad_narrow_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(conv3d_wgrad_narrow_kernel, dim3((unsigned)((long long)p.blocks_c * p.S)), dim3(256), lds, st, d_in, d_grad_out,
                     partial, batch, cin, cout, depth, height, width, p.tiles_y, p.tiles_z, p.S);
  int lrc = m3d::check_launch("conv3d_wgrad_narrow");
  if (lrc != M3D_OK) return lrc;
  hipLaunchKernelGGL(wgrad_narrow_reduce_kernel, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, st, partial, p.S, p.n, d_grad_weight);
  return m3d::check_launch("conv3d_wgrad_narrow_reduce");
}
