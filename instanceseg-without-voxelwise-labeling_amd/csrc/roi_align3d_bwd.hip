// RoIAlign 3D backward, ordered (gather) form for gfx950: no atomics, every element of the gradient written exactly once, the result a
// pure function of (top, rois, shapes).  DESIGN.md, "RoIAlign3D backward, ordered".
//
// Semantics are those of roi_align3d_kernel<true> (roi_align3d.hip; roi_align_kernel_3d.cu:180-338 of the reference): the backward's
// `z < -0.1` validity rule, `top` in natural [R, C, AS, AH, AW] order, count = grid_z * grid_y * grid_x, the batch index clamped into
// [0, B), weight h to voxel lo and l to voxel hi.  Only the order of the fp32 operations differs.  Validity and weights are separable
// per axis, so with M[p, d] = the sum over the valid sub-samples of bin p of the weight that lands on voxel d (folded in sub-sample order,
// h before l) the gradient of image b is
//     gx[b, c, z, y, x] = sum_{r on image b}  sum_pw Mx_r[pw, x] ( sum_ph My_r[ph, y] ( sum_ps Mz_r[ps, z] (top[r, c, ps, ph, pw] / count_r) ) )
// evaluated innermost first, every sum in ascending index order, the RoIs of an image in ascending RoI index.
//
// Launches.  (1) roi_bwd_prologue_kernel: per image the list of its RoIs in ascending index (stable compaction by ballots), per RoI the
// voxel range its valid samples reach on each axis, and one status word (an adaptive grid beyond the tables).  (2) roi_bwd_main_kernel: one
// workgroup per (image, channel, tile of <= 16^3 voxels).  Wave w of the nw waves takes entries [w L / nw, (w + 1) L / nw) of the image's
// list (L its length) and accumulates them, in list order, into its OWN copy of the tile in LDS: a voxel is owned by one lane at a time,
// plain read-add-write.  The copies are then added in wave order and the tile is stored.  This file is compiled with -ffp-contract=off:
// the operation order is the contract with tests/roi_align_backward_ordered_cases.py.
#include <stddef.h>
#include <stdint.h>

#include "m3d_common.h"

#include "roi_align3d_geom.h"   // AxisSample, kMaxTable, make_sample, RoiGeom, roi_geom

namespace {

constexpr int kTile = 16;                   // tile edge: min(dim, 16) per axis
constexpr int kMaxWaves = 4;
constexpr int kLdsBudget = 65024;           // dynamic LDS of a workgroup, bytes (64 KB less the static part): two workgroups per CU
constexpr int kTopStageMax = 1024;          // AS * AH * AW floats a wave stages in LDS per (RoI, channel); above: read from global
constexpr int kWsHead = 4;                  // workspace ints before the per-image records: [0] status

// The launch plan: a function of the shapes alone (tests/roi_align_backward_ordered_cases.py: plan()).
struct Plan {
  int tz, ty, tx;        // tile edges (also the strides of the LDS tile)
  int ntz, nty, ntx;     // tiles per axis
  int stage;             // 1: top[r, c] / count is staged in LDS
  int per_wave;          // floats of LDS per wave (multiple of 4)
  int nw;                // waves per workgroup
};

inline Plan make_plan(int AS, int AH, int AW, int S, int H, int W) {
  Plan p;
  p.tz = S < kTile ? S : kTile; p.ty = H < kTile ? H : kTile; p.tx = W < kTile ? W : kTile;
  p.ntz = (S + p.tz - 1) / p.tz; p.nty = (H + p.ty - 1) / p.ty; p.ntx = (W + p.tx - 1) / p.tx;
  const int nbins = AS * AH * AW;           // <= 64^3
  p.stage = nbins <= kTopStageMax ? 1 : 0;
  int f = p.tz * p.ty * p.tx + AS * p.tz + AH * p.ty + AW * p.tx + AH * AW + p.ty * AW + (p.stage ? nbins : 0);
  p.per_wave = (f + 3) / 4 * 4;             // <= 13312 floats: one wave always fits
  int nw = kLdsBudget / (4 * p.per_wave);
  p.nw = nw > kMaxWaves ? kMaxWaves : nw;
  return p;
}

// LDS traffic of one wave needs no workgroup barrier: the wave's ds operations execute in order.  This keeps the compiler from moving
// them across a pass boundary.
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// workspace (ints): [0] status, [4 + b] first list entry of image b, [4 + B + b] its RoI count, [4 + 2 B ...] the R list entries,
// then 6 ints per RoI: z, y, x voxel ranges [lo, hi] of its valid samples (lo > hi: none)
__device__ __host__ inline size_t ws_ints(int R, int B) { return (size_t)kWsHead + 2 * (size_t)B + 7 * (size_t)R; }

// grid = B + ceil(R / 256) workgroups of 256: workgroup b < B builds the list of image b (and workgroup 0 the status word), the others
// compute the ranges of 256 RoIs each
__global__ __launch_bounds__(256) void roi_bwd_prologue_kernel(const float* __restrict__ rois, int R, int B, int S, int H, int W, int AS,
                                                               int AH, int AW, float scale, int ratio, int* __restrict__ ws) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int* first = ws + kWsHead;
  int* cnt = first + B;
  int* list = cnt + B;
  int* rng = list + R;
  if ((int)blockIdx.x >= B) {                                  // ---- ranges
    const int r = ((int)blockIdx.x - B) * 256 + tid;
    if (r >= R) return;
    const RoiGeom g = roi_geom(rois + 7 * (size_t)r, scale, AS, AH, AW, ratio, B);
    const bool tabled = g.grid_s <= kMaxTable / AS && g.grid_h <= kMaxTable / AH && g.grid_w <= kMaxTable / AW;
#pragma unroll 1
    for (int ax = 0; ax < 3; ++ax) {
      const int A = ax == 0 ? AS : (ax == 1 ? AH : AW), dim = ax == 0 ? S : (ax == 1 ? H : W);
      const int grid = ax == 0 ? g.grid_s : (ax == 1 ? g.grid_h : g.grid_w);
      const float start = ax == 0 ? g.start_s : (ax == 1 ? g.start_h : g.start_w);
      const float bin = ax == 0 ? g.bin_s : (ax == 1 ? g.bin_h : g.bin_w);
      int lo = 1, hi = 0;
      bool any = false;
      if (tabled) {
        for (int t = 0; t < A * grid; ++t) {
          const AxisSample s = make_sample(start, bin, t / grid, t % grid, grid, dim, ax == 0 ? -0.1 : -1.0);
          if (!s.valid) continue;
          lo = any ? min(lo, s.lo) : s.lo;
          hi = any ? max(hi, s.hi) : s.hi;
          any = true;
        }
      }
      rng[6 * (size_t)r + 2 * ax] = lo;
      rng[6 * (size_t)r + 2 * ax + 1] = hi;
    }
    return;
  }
  // ---- the list of image b: RoIs whose clamped batch index is b, in ascending RoI index
  const int b = blockIdx.x;
  int less = 0, bad = 0;
  for (int r0 = 0; r0 < R; r0 += 256) {
    const int r = r0 + tid;
    int bb = -1, unsupported = 0;
    if (r < R) {
      const RoiGeom g = roi_geom(rois + 7 * (size_t)r, scale, AS, AH, AW, ratio, B);
      bb = g.batch;
      unsupported = (g.grid_s > kMaxTable / AS || g.grid_h > kMaxTable / AH || g.grid_w > kMaxTable / AW) ? 1 : 0;
    }
    less += __syncthreads_count(r < R && bb < b);
    bad |= __syncthreads_or(unsupported);
  }
  int base = 0;
  for (int r0 = 0; r0 < R; r0 += 256) {
    const int r = r0 + tid;
    const bool mine = r < R && min(max((int)rois[7 * (size_t)r], 0), B - 1) == b;
    const unsigned long long m = __ballot(mine);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int pre = base;
    for (int w = 0; w < wave; ++w) pre += wsum[w];
    const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (mine) list[less + pre + __popcll(m & ((1ull << lane) - 1ull))] = r;
    base += tot;
    __syncthreads();
  }
  if (tid == 0) {
    first[b] = less;
    cnt[b] = base;
    if (b == 0) ws[0] = bad ? 1 : 0;
  }
}

// grid = (C * tiles, B); block = 64 * nw; dynamic LDS = nw * per_wave floats
__global__ __launch_bounds__(256) void roi_bwd_main_kernel(const float* __restrict__ top, const float* __restrict__ rois,
                                                           float* __restrict__ grad, const int* __restrict__ ws, int R, int B, int C, int S,
                                                           int H, int W, int AS, int AH, int AW, float scale, int ratio, Plan P, int vec) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  if (ws[0] != 0) return;                                     // an adaptive grid beyond the tables: nothing is written (the caller reads ws[0])
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y;
  const int ntiles = P.ntz * P.nty * P.ntx;
  const int c = blockIdx.x / ntiles;
  int t = blockIdx.x - c * ntiles;
  const int tzi = t / (P.nty * P.ntx); t -= tzi * P.nty * P.ntx;
  const int tyi = t / P.ntx, txi = t - tyi * P.ntx;
  const int z0 = tzi * P.tz, y0 = tyi * P.ty, x0 = txi * P.tx;               // tile origin and extents
  const int ez = min(P.tz, S - z0), ey = min(P.ty, H - y0), ex = min(P.tx, W - x0);
  const int tile_n = P.tz * P.ty * P.tx;
  const int nbins = AS * AH * AW, nplane = AH * AW;

  float* acc = dyn + (size_t)wave * P.per_wave;                             // this wave's copy of the tile and its scratch
  float* mz = acc + tile_n;
  float* my = mz + AS * P.tz;
  float* mx = my + AH * P.ty;
  float* u = mx + AW * P.tx;
  float* v = u + nplane;
  float* tq = v + P.ty * AW;
  const int ntab = AS * P.tz + AH * P.ty + AW * P.tx;

  for (int e = lane; e < tile_n; e += 64) acc[e] = 0.f;

  const int* first = ws + kWsHead;
  const int* cnt = first + B;
  const int* list = cnt + B + first[b];
  const int* rng = cnt + B + R;
  const int L = cnt[b];
  const int i0 = (int)((long long)wave * L / P.nw), i1 = (int)((long long)(wave + 1) * L / P.nw);
  const float inv_aw = 1.0f / (float)AW;

  for (int i = i0; i < i1; ++i) {
    const int r = list[i];
    const int* rr = rng + 6 * (size_t)r;
    // the part of the RoI's range inside this tile, tile-local
    const int a0 = max(rr[0], z0) - z0, a1 = min(rr[1], z0 + ez - 1) - z0;
    const int b0 = max(rr[2], y0) - y0, b1 = min(rr[3], y0 + ey - 1) - y0;
    const int c0 = max(rr[4], x0) - x0, c1 = min(rr[5], x0 + ex - 1) - x0;
    if (a0 > a1 || b0 > b1 || c0 > c1) continue;
    const RoiGeom g = roi_geom(rois + 7 * (size_t)r, scale, AS, AH, AW, ratio, B);
    // ---- folded tables of this RoI, restricted to the tile: M[p][d - origin] += h at lo, then += l at hi, sub-samples in order
    wave_sync();                                                            // the previous RoI's passes have read theirs
    for (int e = lane; e < ntab; e += 64) mz[e] = 0.f;
    wave_sync();
    for (int e = lane; e < AS + AH + AW; e += 64) {
      const int ax = e < AS ? 0 : (e < AS + AH ? 1 : 2);
      const int p = ax == 0 ? e : (ax == 1 ? e - AS : e - AS - AH);
      const int dim = ax == 0 ? S : (ax == 1 ? H : W), org = ax == 0 ? z0 : (ax == 1 ? y0 : x0), ext = ax == 0 ? ez : (ax == 1 ? ey : ex);
      const int grid = ax == 0 ? g.grid_s : (ax == 1 ? g.grid_h : g.grid_w);
      const float start = ax == 0 ? g.start_s : (ax == 1 ? g.start_h : g.start_w);
      const float bin = ax == 0 ? g.bin_s : (ax == 1 ? g.bin_h : g.bin_w);
      float* row = ax == 0 ? mz + p * P.tz : (ax == 1 ? my + p * P.ty : mx + p * P.tx);
      for (int k = 0; k < grid; ++k) {
        const AxisSample s = make_sample(start, bin, p, k, grid, dim, ax == 0 ? -0.1 : -1.0);
        if (!s.valid) continue;
        const int lo = s.lo - org, hi = s.hi - org;
        if (lo >= 0 && lo < ext) row[lo] = row[lo] + s.h;
        if (hi >= 0 && hi < ext) row[hi] = row[hi] + s.l;
      }
    }
    const float count = (float)(g.grid_s * g.grid_h * g.grid_w);
    const float* tg = top + ((size_t)r * C + c) * nbins;
    if (P.stage)
      for (int e = lane; e < nbins; e += 64) tq[e] = tg[e] / count;         // 343 contiguous floats: coalesced, once per (RoI, channel, tile)
    wave_sync();

    const int ny = b1 - b0 + 1, nx = c1 - c0 + 1;
    const float inv_nx = 1.0f / (float)nx;
    for (int zl = a0; zl <= a1; ++zl) {
      // pass Z: u[ph, pw] = sum_ps Mz[ps, z] * (top[ps, ph, pw] / count); Mz[ps, z] is wave-uniform, zero rows are skipped
      for (int e = lane; e < nplane; e += 64) {
        float s = 0.f;
        for (int ps = 0; ps < AS; ++ps) {
          const float m = mz[ps * P.tz + zl];
          if (m == 0.f) continue;
          const float tv = P.stage ? tq[ps * nplane + e] : tg[ps * nplane + e] / count;
          s = s + m * tv;
        }
        u[e] = s;
      }
      wave_sync();
      // pass Y: v[y, pw] = sum_ph My[ph, y] * u[ph, pw]
      for (int e = lane; e < ny * AW; e += 64) {
        const int yl = (int)(((float)e + 0.5f) * inv_aw), pw = e - yl * AW;
        const float* col = my + b0 + yl;
        float s = 0.f;
        for (int ph = 0; ph < AH; ++ph) s = s + col[ph * P.ty] * u[ph * AW + pw];
        v[e] = s;
      }
      wave_sync();
      // pass X into the tile: acc[z, y, x] += sum_pw Mx[pw, x] * v[y, pw]; one lane per voxel
      for (int e = lane; e < ny * nx; e += 64) {
        const int yl = (int)(((float)e + 0.5f) * inv_nx), xl = e - yl * nx;
        const float* col = mx + c0 + xl;
        const float* vr = v + yl * AW;
        float s = 0.f;
        for (int pw = 0; pw < AW; ++pw) s = s + col[pw * P.tx] * vr[pw];
        float* a = acc + (zl * P.ty + b0 + yl) * P.tx + c0 + xl;
        *a = *a + s;
      }
      wave_sync();
    }
  }
  __syncthreads();
  // ---- the copies summed in wave order, every element of the tile stored once
  float* gb = grad + (((size_t)b * C + c) * S + z0) * (size_t)H * W + (size_t)y0 * W + x0;
  const int nthreads = 64 * P.nw;
  if (vec) {                                                                // rows of whole, aligned 16-byte pieces
    const int q = ex >> 2;
    for (int e = tid; e < ez * ey * q; e += nthreads) {
      const int xq = e % q, yl = (e / q) % ey, zl = e / (q * ey);
      const int o = (zl * P.ty + yl) * P.tx + 4 * xq;
      float4 s = *reinterpret_cast<const float4*>(dyn + o);
      for (int w = 1; w < P.nw; ++w) {
        const float4 d = *reinterpret_cast<const float4*>(dyn + (size_t)w * P.per_wave + o);
        s.x = s.x + d.x; s.y = s.y + d.y; s.z = s.z + d.z; s.w = s.w + d.w;
      }
      *reinterpret_cast<float4*>(gb + ((size_t)zl * H + yl) * W + 4 * xq) = s;
    }
  } else {
    for (int e = tid; e < ez * ey * ex; e += nthreads) {
      const int xl = e % ex, yl = (e / ex) % ey, zl = e / (ex * ey);
      const int o = (zl * P.ty + yl) * P.tx + xl;
      float s = dyn[o];
      for (int w = 1; w < P.nw; ++w) s = s + dyn[(size_t)w * P.per_wave + o];
      gb[((size_t)zl * H + yl) * W + xl] = s;
    }
  }
}

}  // namespace

M3D_API size_t m3d_roi_align3d_backward_ordered_workspace_bytes(int num_rois, int batch) {
  return sizeof(int) * ws_ints(num_rois > 0 ? num_rois : 0, batch > 0 ? batch : 0);
}

M3D_API int m3d_roi_align3d_backward_ordered(int AS, int AH, int AW, float spatial_scale, int sampling_ratio, const float* d_top_grad,
                                             const float* d_rois, int num_rois, int roi_cols, float* d_bottom_grad, int batch, int channels,
                                             int slices, int height, int width, void* d_workspace, size_t workspace_bytes, void* stream) {
  const int R = num_rois, B = batch, C = channels, S = slices, H = height, W = width;
  if (roi_cols != 7) return M3D_EINVAL;
  if (R < 0 || B <= 0 || C <= 0 || S <= 0 || H <= 0 || W <= 0 || AS <= 0 || AH <= 0 || AW <= 0) return M3D_EINVAL;
  if (!d_bottom_grad || (R > 0 && (!d_top_grad || !d_rois))) return M3D_EINVAL;
  if (!d_workspace || workspace_bytes < m3d_roi_align3d_backward_ordered_workspace_bytes(R, B)) return M3D_EINVAL;
  if (B > 65535) return M3D_EINVAL;                                        // the launch grid's y extent
  if (sampling_ratio > 0 && (AS * (long long)sampling_ratio > kMaxTable || AH * (long long)sampling_ratio > kMaxTable ||
                             AW * (long long)sampling_ratio > kMaxTable))
    return M3D_EUNSUPPORTED;
  if (AS > kMaxTable || AH > kMaxTable || AW > kMaxTable) return M3D_EUNSUPPORTED;   // adaptive: every grid is >= 1
  const Plan P = make_plan(AS, AH, AW, S, H, W);
  const long long blocks_x = (long long)C * P.ntz * P.nty * P.ntx;
  if (blocks_x > 0x7FFFFFFFll) return M3D_EUNSUPPORTED;
  int* ws = reinterpret_cast<int*>(d_workspace);
  hipStream_t st = m3d::as_stream(stream);
  hipLaunchKernelGGL(roi_bwd_prologue_kernel, dim3(B + (R + 255) / 256), dim3(256), 0, st, d_rois, R, B, S, H, W, AS, AH, AW, spatial_scale,
                     sampling_ratio, ws);
  const int vec = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(d_bottom_grad) & 15u) == 0) ? 1 : 0;
  hipLaunchKernelGGL(roi_bwd_main_kernel, dim3((unsigned)blocks_x, B), dim3(64 * P.nw), sizeof(float) * (size_t)P.nw * P.per_wave, st,
                     d_top_grad, d_rois, d_bottom_grad, (const int*)ws, R, B, C, S, H, W, AS, AH, AW, spatial_scale, sampling_ratio, P, vec);
  return m3d::check_launch("roi_align3d_backward_ordered");
}
