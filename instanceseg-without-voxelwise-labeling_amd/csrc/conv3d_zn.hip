// 3x3x3 convolution (stride 1, pad 1) [+ scale / shift + ReLU] on NARROW maps (width <= 8: the per-RoI convs on 7^3 RoI grids of the conv
// box head and of the mask head at dilation 1) on the f16 matrix cores at fp32 accuracy: the "f16x2" cut of fc_gemm.hip / conv3d_zw.hip
// (both operands scaled by a power of two and cut into two fp16 numbers, 22 bits; three v_mfma_f32_32x32x16_f16 per fp32 product, fp32
// accumulation, un-scaled by an exact power of two) in the DIRECT form: 27 taps, no Winograd.  Along a depth of 7 F(2,3)z would pad to 8
// planes anyway, its transform rounds once more before the cut, and the direct form keeps zero products exact (C == 0: the output is
// exactly the shift).
//
// Decomposition: a UNIT is 64 output channels x a tile of 8 (x) x 8 (y) x 4 (z) voxels = 8 column blocks of 32 voxels; one workgroup of
// four waves per unit, the whole K = 27 cin inside it (no split-K, no atomics on the output: bit-identical run to run).  Wave = (32-channel
// block, y half of the tile): four 32 x 32 accumulator blocks.  GEMM view per tap and 16-channel chunk: A = weights (32 co x 16 ci, packed
// fragment-ready in global memory, requested one tap ahead), B = the input (16 ci x 32 voxels, one ds_read_b128 per fragment from the
// channel-contiguous LDS image [hi / lo][k half][halo voxel]).  The halo tile of a chunk (10 x 10 x 6 voxels x 16 channels) is requested
// into registers before the previous chunk's taps, scaled and cut after them, and serves all 27 taps.
//
// A column block is 8 x of the rows (y, z), (y, z + 1), (y + 1, z), (y + 1, z + 1), laid on the lanes so that each 16-lane group
// ds_read_b128 is served in ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}) reads the two rows (y, z), (y, z + 1): with a halo row pitch of
// 10 units and a plane pitch of 104 (= 8 mod 16) those are 16 different 16-byte slots of the 256-byte bank row - no bank conflicts.
//
// DILATION 2 (padding 2: the mask head at MRCNN.DILATION = 2) is the second instantiation of the same kernel, conv3d_zn_kernel<2>: the
// same unit, waves, weight packs (a pack does not depend on the dilation), cut, MFMA order and epilogue; a tap reads at 2 (d - 1), so the
// halo is 2 voxels per side: 12 x 12 x 8 voxels, row pitch 12, plane pitch 144 -> 152 (= 8 mod 16: the same two-rows-one-plane-apart
// reads, the same argument), four images of 8 planes = 77 824 bytes of LDS, asked for dynamically.  The map is at most 8 wide, so the
// halo columns x < 0 and x >= 8 are padding in every chunk: they are written as zero units ONCE, before the first chunk, and staging
// covers the 8 columns that can hold data - 12 x 8 x 8 voxels x 2 channel halves = 1536 items, exactly 6 per thread (48 raw registers
// against the 40 of dilation 1), which keeps the kernel at two workgroups per CU without scratch.
#include "f16x2.h"

namespace {

using namespace m3d::f16x2;      // the cut, its vector types and the bound slots: f16x2.h

constexpr int ZN_NT = 256;
constexpr int ZN_STEP_UNITS = 2 * 2 * 2 * 32;      // packed weights of one (chunk, tap): [block 2][hi / lo][k half][row 32] 16-byte units
constexpr int ZN_TY = 8, ZN_TZ = 4;                // tile: 8 x 8 x 4 voxels (x: the whole row)
// the geometry of the halo tile at dilation DIL (1 or 2)
template <int DIL>
struct ZnGeom {
  static constexpr int HX = 8 + 2 * DIL, HY = ZN_TY + 2 * DIL, HZ = ZN_TZ + 2 * DIL;      // halo tile: 10 x 10 x 6 / 12 x 12 x 8
  // pitches in 16-byte units; plane: the smallest count >= HY * HX that is 8 mod 16 (100 -> 104, 144 -> 152), see above
  static constexpr int ROW = HX, PLANE = HY * HX + (24 - HY * HX % 16) % 16;
  static constexpr int IMG = HZ * PLANE;                       // one (piece, k half) image
  // staged columns of a halo row: all 10 at dilation 1; at dilation 2 the 8 that can lie inside the map (the other 4 are zeroed once)
  static constexpr int SX0 = DIL == 1 ? 0 : DIL, SXN = DIL == 1 ? HX : 8;
  static constexpr int ITEMS = 2 * HZ * HY * SXN;              // staging items of a chunk: (8-channel half, halo voxel)
  static constexpr int PER = (ITEMS + ZN_NT - 1) / ZN_NT;      // items per thread
  static constexpr int LDS_BYTES = 4 * IMG * 16;
  static constexpr bool DYNAMIC = LDS_BYTES > 64 * 1024 - 64;  // above the static limit: asked for at the launch
  static_assert(PLANE % 16 == 8 && PLANE >= HY * HX, "plane pitch");
  static_assert(LDS_BYTES <= 160 * 1024 / 2, "two workgroups per CU");
};
static_assert(ZnGeom<1>::PLANE == 104 && ZnGeom<1>::ITEMS == 1200 && ZnGeom<1>::PER == 5 && !ZnGeom<1>::DYNAMIC, "dilation 1 as it was");
static_assert(ZnGeom<2>::PLANE == 152 && ZnGeom<2>::ITEMS == 1536 && ZnGeom<2>::PER == 6 && ZnGeom<2>::LDS_BYTES == 77824, "dilation 2");

// column (lane % 32) of a column block -> (x, row y, row z) inside the block's 8 x 2 x 2 voxels
__device__ __forceinline__ void col_xyz(int c, int* x, int* y, int* z) {
  if (c < 4) { *x = c; *y = 0; *z = 0; }
  else if (c < 12) { *x = c - 4; *y = 1; *z = 0; }
  else if (c < 16) { *x = c - 8; *y = 0; *z = 0; }
  else if (c < 20) { *x = c - 16; *y = 1; *z = 1; }
  else if (c < 28) { *x = c - 20; *y = 0; *z = 1; }
  else { *x = c - 24; *y = 1; *z = 1; }
}

// packed[cout group 64][step = chunk * 27 + dz * 9 + dy * 3 + dx][block][hi / lo][k half][row 32] <- weight [cout][cin][3][3][3] fp32
// DGRAD: `w` is the FORWARD conv's parameter [cin][cout][3][3][3] as it lies in memory and the pack is the backward-data conv's (cin / cout
// are the PACK's: the forward layer's cout / cin): element (co, ci, dz, dy, dx) of the packed conv is w[ci][co][2 - dz][2 - dy][2 - dx] -
// what packing w.flip(2, 3, 4).transpose(0, 1).contiguous() reads, without that copy.
template <bool DGRAD>
__global__ __launch_bounds__(256) void zn_pack_kernel(const float* __restrict__ w, int cin, int cout, u32x4* __restrict__ packed,
                                                      const float* __restrict__ wamax) {
  float sw, inv;
  f16_scale_of(*wamax, sw, inv);
  const int chunks = cin / 16, ncg = (cout + 63) / 64;
  const long long total = (long long)ncg * chunks * 27 * 2 * 64;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int row = (int)(e & 31), kh = (int)((e >> 5) & 1), cb = (int)((e >> 6) & 1);
    long long r = e >> 7;
    const int tap = (int)(r % 27); r /= 27;
    const int ch = (int)(r % chunks), cg = (int)(r / chunks);
    const int co = cg * 64 + cb * 32 + row;
    u32x4 ph, pl;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f16x2 hh, ll;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float v = 0.f;
        if (co < cout) {
          const int ci = ch * 16 + 8 * kh + 2 * j + u;
          v = (DGRAD ? w[((size_t)ci * cout + co) * 27 + (26 - tap)] : w[((size_t)co * cin + ci) * 27 + tap]) * sw;
        }
        cut(v, hh, ll, u);
      }
      ph[j] = __builtin_bit_cast(unsigned, hh); pl[j] = __builtin_bit_cast(unsigned, ll);
    }
    u32x4* dst = packed + ((size_t)(cg * chunks + ch) * 27 + tap) * ZN_STEP_UNITS + cb * 128 + kh * 32 + row;
    dst[0] = ph; dst[64] = pl;
  }
}

struct ZnArgs {
  const float* x; const u32x4* wp; float* out; const float* scale; const float* shift;
  const float* in_max; unsigned* out_max; const float* wamax;
  int B, cin, cout, D, H, W, relu;
  int tiles_y, tiles_z, ncg;
};

// (launch bounds: DIL waves per SIMD at least.  1 is what a kernel of 256 threads has anyway - dilation 1 is built as before; dilation 2
// stages 48 raw registers per chunk against 40 and, left alone, the register allocator takes 264 registers and with them the whole SIMD
// for one wave: asked for two - its 76 KB of LDS allow two workgroups per CU - it stays inside 256 without scratch)
template <int DIL>
__global__ __launch_bounds__(ZN_NT, DIL) void conv3d_zn_kernel(ZnArgs a) {
  typedef ZnGeom<DIL> G;
  constexpr int ZN_HX = G::HX, ZN_HY = G::HY, ZN_ROW = G::ROW, ZN_PLANE = G::PLANE, ZN_IMG = G::IMG, ZN_ITEMS = G::ITEMS, ZN_PER = G::PER;
  // the four LDS images: static at dilation 1; at dilation 2 above the 64 KB static limit, so dynamic (the static array is then one
  // unit that nothing touches).  ZN_LDS names the array itself under a constant condition: through a reference or a pointer the
  // dilation-1 instantiation comes out with two registers renamed, named directly it is the code it was before the template
  __shared__ u32x4 zn_lds_static[G::DYNAMIC ? 1 : 4 * G::IMG];
  extern __shared__ u32x4 zn_lds_dynamic[];
#define ZN_LDS(i) (G::DYNAMIC ? zn_lds_dynamic[i] : zn_lds_static[i])
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = wave & 1, yh = wave >> 1;
  const size_t HW = (size_t)a.H * a.W, DHW = HW * a.D;
  const int chunks = a.cin / 16, steps = chunks * 27;

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

  // ---- the unit: (cout group fastest, y tile, z tile, batch item)
  int u = blockIdx.x;
  const int cg = u % a.ncg; u /= a.ncg;
  const int y0 = (u % a.tiles_y) * ZN_TY; u /= a.tiles_y;
  const int z0 = (u % a.tiles_z) * ZN_TZ;
  const int b = u / a.tiles_z;
  const float* const xb = a.x + (size_t)b * a.cin * DHW;

  // ---- staging items of this thread: (8-channel half g, halo voxel); offsets inside one batch item (host: cin * D * H * W < 2^29)
  int soff[ZN_PER], sdst[ZN_PER];
  bool sok[ZN_PER];
#pragma unroll
  for (int q = 0; q < ZN_PER; ++q) {
    const int i = tid + q * ZN_NT;
    const bool has = i < ZN_ITEMS;
    const int g = has ? i / (ZN_ITEMS / 2) : 0, r = has ? i % (ZN_ITEMS / 2) : 0;
    const int hz = r / (ZN_HY * G::SXN), hy = (r / G::SXN) % ZN_HY, hx = G::SX0 + r % G::SXN;
    const int z = z0 - DIL + hz, y = y0 - DIL + hy, x = hx - DIL;
    sok[q] = has & (z >= 0) & (z < a.D) & (y >= 0) & (y < a.H) & (x >= 0) & (x < a.W);
    soff[q] = sok[q] ? (int)((size_t)8 * g * DHW + (size_t)z * HW + (size_t)y * a.W + x) : 0;
    sdst[q] = has ? g * ZN_IMG + hz * ZN_PLANE + hy * ZN_ROW + hx : -1;
  }
  float raw[ZN_PER][8];
  auto fetch_in = [&](int c) __attribute__((always_inline)) {
    const float* base = xb + (size_t)c * 16 * DHW;
#pragma unroll
    for (int q = 0; q < ZN_PER; ++q)
#pragma unroll
      for (int j = 0; j < 8; ++j) raw[q][j] = sok[q] ? base[(size_t)soff[q] + (size_t)j * DHW] : 0.f;     // outside the volume: the zero padding
  };
  auto commit_in = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < ZN_PER; ++q) {
      u32x4 ph, pl;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f16x2 hh, ll;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float v = raw[q][2 * j + e] * xs;
          cut(v, hh, ll, e);
        }
        ph[j] = __builtin_bit_cast(unsigned, hh); pl[j] = __builtin_bit_cast(unsigned, ll);
      }
      if (sdst[q] >= 0) { ZN_LDS(sdst[q]) = ph; ZN_LDS(sdst[q] + 2 * ZN_IMG) = pl; }
    }
  };

  // ---- fragments.  Column block j of this wave: rows y = 4 yh + 2 (j >> 1) + {0, 1}, z = 2 (j & 1) + {0, 1}
  const int fr = lane & 31, fh = lane >> 5;
  int cx, cy, cz;
  col_xyz(fr, &cx, &cy, &cz);
  const int bB = fh * ZN_IMG + cz * ZN_PLANE + (4 * yh + cy) * ZN_ROW + cx;      // + block, tap and piece parts
  const u32x4* const wsrc = a.wp + (size_t)cg * steps * ZN_STEP_UNITS + cb * 128 + lane;
  f16x8 A0[2], A1[2];
  auto fetch_a = [&](f16x8 (&A)[2], int s) __attribute__((always_inline)) {
    const u32x4* p = wsrc + (size_t)(s < steps ? s : steps - 1) * ZN_STEP_UNITS;
    A[0] = __builtin_bit_cast(f16x8, p[0]);
    A[1] = __builtin_bit_cast(f16x8, p[64]);
  };

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[j][g] = 0.f;

  fetch_in(0);
  fetch_a(A0, 0);
  if constexpr (G::SXN < ZN_HX) {
    // the halo columns staging never writes (x < 0, x >= 8: outside every map): zero units, once
    constexpr int NP = ZN_HX - G::SXN, PADS = 4 * G::HZ * ZN_HY * NP;
    for (int i = tid; i < PADS; i += ZN_NT) {
      const int img = i / (PADS / 4), r = i % (PADS / 4);
      const int row = r / NP, k = r % NP;
      const int hx = k < G::SX0 ? k : G::SXN + k;
      ZN_LDS(img * ZN_IMG + (row / ZN_HY) * ZN_PLANE + (row % ZN_HY) * ZN_ROW + hx) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  commit_in();
  __syncthreads();

#pragma unroll 1
  for (int c = 0; c < chunks; ++c) {
    const bool more = c + 1 < chunks;
    if (more) fetch_in(c + 1);
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      f16x8 (&Ac)[2] = (t & 1) ? A1 : A0;
      f16x8 (&An)[2] = (t & 1) ? A0 : A1;
      fetch_a(An, c * 27 + t + 1);
      const int dz = t / 9, dy = (t / 3) % 3, dx = t % 3;
      f16x8 Bf[4][2];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          Bf[j][p] = __builtin_bit_cast(f16x8, ZN_LDS(bB + (2 * (j & 1) + DIL * dz) * ZN_PLANE + (2 * (j >> 1) + DIL * dy) * ZN_ROW + DIL * dx + p * 2 * ZN_IMG));
      constexpr int PA[3] = {1, 0, 0}, PB[3] = {0, 1, 0};                     // small products first: (lo, hi) (hi, lo) (hi, hi)
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ac[PA[q]], Bf[j][PB[q]], acc[j], 0, 0, 0);
      // a tap is one scheduling region: without the fence the scheduler hoists the weight requests of all 27 taps to the chunk's head
      __builtin_amdgcn_sched_barrier(0);
    }
    // 27 is odd: the fragments of the next chunk's tap 0 are in A1 - move them where tap 0 reads
    A0[0] = A1[0]; A0[1] = A1[1];
    if (more) {
      __syncthreads();                                   // every wave has read this chunk's tile
      commit_in();
      __syncthreads();
    }
  }

  // ---- epilogue from the accumulators: lane = one voxel of each column block, 16 channels
  float vmax = 0.f;
  float* const ob = a.out + (size_t)b * a.cout * DHW;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int co = cg * 64 + cb * 32 + 4 * fh + acc_row(g);
    if (co >= a.cout) continue;
    const float sc = a.scale ? a.scale[co] * un : un;    // (un: a power of two)
    const float sh = a.shift ? a.shift[co] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int z = z0 + 2 * (j & 1) + cz, y = y0 + 4 * yh + 2 * (j >> 1) + cy;
      if (z >= a.D || y >= a.H || cx >= a.W) continue;
      float v = acc[j][g] * sc + sh;
      if (a.relu) v = fmaxf(v, 0.f);
      ob[(size_t)co * DHW + (size_t)z * HW + (size_t)y * a.W + cx] = v;
      vmax = fmaxf(vmax, fabsf(v));
    }
  }
  // ---- the next layer's operand bound: one atomic per workgroup into slot (block % 32)
  if (a.out_max) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
    __shared__ float wm[4];
    if (lane == 0) wm[wave] = vmax;
    __syncthreads();
    if (tid == 0) {
      const float m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
      if (m > 0.f) atomicMax(a.out_max + (blockIdx.x & (kBoundSlots - 1)), __float_as_uint(m));
    }
  }
}

#undef ZN_LDS

inline size_t zn_plane_bytes(int cin, int cout) { return (size_t)((cout + 63) / 64) * (cin / 16) * 27 * ZN_STEP_UNITS * 16; }

inline long long zn_units(int batch, int cout, int depth, int height) {
  return (long long)batch * ((cout + 63) / 64) * ((height + ZN_TY - 1) / ZN_TY) * ((depth + ZN_TZ - 1) / ZN_TZ);
}

}  // namespace

M3D_API int m3d_conv3d_zn_supported(int cin, int cout, int depth, int height, int width) {
  if (cin <= 0 || cout <= 0 || cin % 16 != 0 || depth < 1 || height < 1 || width < 1 || width > 8) return 0;
  if ((size_t)cin * depth * height * width >= (1ull << 29)) return 0;       // 32-bit element offsets inside one batch item
  return 1;
}

M3D_API size_t m3d_conv3d_zn_packed_bytes(int cin, int cout) {
  if (cin <= 0 || cout <= 0 || cin % 16 != 0) return 0;
  return zn_plane_bytes(cin, cout) + 256;            // + the weight's largest magnitude (one float) behind the fragments
}

M3D_API int m3d_conv3d_zn_pack(const float* d_weight, int cin, int cout, void* d_packed, void* stream) {
  if (!d_weight || !d_packed || cin <= 0 || cout <= 0 || cin % 16 != 0) return M3D_EINVAL;
  float* wamax = reinterpret_cast<float*>(static_cast<char*>(d_packed) + zn_plane_bytes(cin, cout));
  if (const int rc = m3d_absmax(d_weight, (long long)cout * cin * 27, wamax, stream)) return rc;
  hipLaunchKernelGGL(zn_pack_kernel<false>, dim3(1024), dim3(256), 0, m3d::as_stream(stream), d_weight, cin, cout, (u32x4*)d_packed, (const float*)wamax);
  return m3d::check_launch("conv3d_zn_pack");
}

/* The pack of the BACKWARD-DATA conv of a forward layer [cout, cin, 3, 3, 3], straight from the parameter: m3d_conv3d_zn_pack of
 * w.flip(2, 3, 4).transpose(0, 1).contiguous() byte for byte (the largest magnitude is the same set's), m3d_conv3d_zn_packed_bytes(cout, cin) bytes. */
M3D_API int m3d_conv3d_zn_pack_dgrad(const float* d_weight, int cin, int cout, void* d_packed, void* stream) {
  if (!d_weight || !d_packed || cin <= 0 || cout <= 0 || cout % 16 != 0) return M3D_EINVAL;
  float* wamax = reinterpret_cast<float*>(static_cast<char*>(d_packed) + zn_plane_bytes(cout, cin));
  if (const int rc = m3d_absmax(d_weight, (long long)cout * cin * 27, wamax, stream)) return rc;
  hipLaunchKernelGGL(zn_pack_kernel<true>, dim3(1024), dim3(256), 0, m3d::as_stream(stream), d_weight, cout, cin, (u32x4*)d_packed, (const float*)wamax);
  return m3d::check_launch("conv3d_zn_pack_dgrad");
}

/* host only: workgroups of an m3d_conv3d_zn_forward launch, (64 output channels) x (8 x 8 x 4 voxels) x batch */
M3D_API long long m3d_conv3d_zn_launch_units(int batch, int cin, int cout, int depth, int height, int width) {
  (void)cin; (void)width;
  if (batch <= 0 || cout <= 0 || depth <= 0 || height <= 0) return 0;
  return zn_units(batch, cout, depth, height);
}

namespace {

// every refusal of a forward launch, before a pointer is followed; then the launch of instantiation DIL
template <int DIL>
int zn_launch(const char* what, const float* d_in, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth, int height,
              int width, const float* d_scale, const float* d_shift, int relu, const float* d_in_max, float* d_out_max, void* stream) {
  if (!d_in || !d_packed || !d_out || !d_in_max || batch <= 0) return M3D_EINVAL;
  if (!m3d_conv3d_zn_supported(cin, cout, depth, height, width)) return M3D_EUNSUPPORTED;
  ZnArgs a{};
  a.x = d_in; a.wp = static_cast<const u32x4*>(d_packed); a.out = d_out; a.scale = d_scale; a.shift = d_shift;
  a.in_max = d_in_max; a.out_max = reinterpret_cast<unsigned*>(d_out_max);
  a.wamax = reinterpret_cast<const float*>(static_cast<const char*>(d_packed) + zn_plane_bytes(cin, cout));
  a.B = batch; a.cin = cin; a.cout = cout; a.D = depth; a.H = height; a.W = width; a.relu = relu;
  a.tiles_y = (height + ZN_TY - 1) / ZN_TY; a.tiles_z = (depth + ZN_TZ - 1) / ZN_TZ; a.ncg = (cout + 63) / 64;
  const long long units = zn_units(batch, cout, depth, height);
  if (units > 0x7FFFFFFFll) return M3D_EUNSUPPORTED;
  auto kern = conv3d_zn_kernel<DIL>;
  unsigned dyn = 0;
  if (ZnGeom<DIL>::DYNAMIC) {
    // 76 KB of LDS: asked for per launch, as conv3d_wgrad_narrow_f16.hip does (the attribute belongs to the current device's copy of the kernel)
    dyn = ZnGeom<DIL>::LDS_BYTES;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)units), dim3(ZN_NT), dyn, m3d::as_stream(stream), a);
  return m3d::check_launch(what);
}

}  // namespace

M3D_API int m3d_conv3d_zn_forward(const float* d_in, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth, int height,
                                  int width, const float* d_scale, const float* d_shift, int relu, const float* d_in_max, float* d_out_max,
                                  void* stream) {
  return zn_launch<1>("conv3d_zn_forward", d_in, d_packed, d_out, batch, cin, cout, depth, height, width, d_scale, d_shift, relu, d_in_max,
                      d_out_max, stream);
}

/* ---- dilation 1 or 2 (padding = dilation) ---- */
M3D_API int m3d_conv3d_zn_dilated_supported(int cin, int cout, int depth, int height, int width, int dilation) {
  if (dilation != 1 && dilation != 2) return 0;
  return m3d_conv3d_zn_supported(cin, cout, depth, height, width);           // the tile and the limits are the same at both
}

/* host only: workgroups of an m3d_conv3d_zn_dilated_forward launch (both dilations run the 8 x 8 x 4 tile; 0 for another dilation) */
M3D_API long long m3d_conv3d_zn_dilated_launch_units(int batch, int cin, int cout, int depth, int height, int width, int dilation) {
  if (dilation != 1 && dilation != 2) return 0;
  return m3d_conv3d_zn_launch_units(batch, cin, cout, depth, height, width);
}

M3D_API int m3d_conv3d_zn_dilated_forward(const float* d_in, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth,
                                          int height, int width, int dilation, const float* d_scale, const float* d_shift, int relu,
                                          const float* d_in_max, float* d_out_max, void* stream) {
  if (!d_in || !d_packed || !d_out || !d_in_max || batch <= 0) return M3D_EINVAL;
  if (dilation == 1)
    return m3d_conv3d_zn_forward(d_in, d_packed, d_out, batch, cin, cout, depth, height, width, d_scale, d_shift, relu, d_in_max, d_out_max, stream);
  if (dilation != 2) return M3D_EUNSUPPORTED;
  return zn_launch<2>("conv3d_zn_dilated_forward", d_in, d_packed, d_out, batch, cin, cout, depth, height, width, d_scale, d_shift, relu,
                      d_in_max, d_out_max, stream);
}
