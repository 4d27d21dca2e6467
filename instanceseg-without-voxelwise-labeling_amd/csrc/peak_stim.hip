// Peak stimulation (lib/prm/peak_stimulation_3d.py:6-52) for gfx950: local-maximum peak map, per-channel filter threshold, ordered
// peak list and masked-mean aggregation of a response map x [B,C,S,H,W], and the backward peak_map * grad.
//
// A voxel is a peak iff it is the arg-max of its win^3 window clipped to the volume, ties to the FIRST maximum in raster order, a NaN
// above everything and among NaNs the LAST one (what max_pool3d's `val > maxval || isnan(val)` scan gives, :20-25).  Both rules are the
// maximum of ONE 64-bit key, so the window maximum is separable: x, then y, then z.
//   not NaN: (ordered(value) << 32) | (0xFFFFFFFF - raster index)      ordered(): monotone u32 image of the float, -0.0 == +0.0
//   NaN:     (0xFFFFFFFF     << 32) | raster index
// -inf is an ordinary value here (the smallest one): the reference pads with -inf, so its answer on -inf voxels comes from indices that
// point into the padding; this kernel's rule stays "arg-max of the clipped window", which an all -inf volume answers with (0,0,0).
//
// Launches of one call (no atomics on global memory, nothing depends on workgroup order: bit-identical from run to run):
//   peak_thresh_kernel   one workgroup per (b,c): median by an 8-bit radix select (4 histogram passes, no sort), fp64 mean, max, or a copy
//   peak_map_kernel      one workgroup per 4x4x16 tile: keys of the tile + halo through LDS, three passes -> uint8 peak map
//   peak_count_kernel    one workgroup per 1024 raster-contiguous voxels of one (b,c): peak count and fp64 sum of x * peak
//   peak_finish_kernel   one workgroup: exclusive scan of the chunk counts, total (device + pinned mirror), aggregation per (b,c)
//   peak_compact_kernel  one workgroup per chunk: rows (b,c,z,y,x) at its scanned offset, in raster order, below `cap` only
// The 3-D tiles of the map kernel are not raster-contiguous, which is why the counts come from a pass over the byte map of its own.
#include "m3d_common.h"

namespace {

constexpr int TZ = 4, TY = 4, TX = 16;     // outputs of one workgroup of peak_map_kernel (TZ * TY * TX == 256 threads)
constexpr int MAXO = 4;                    // win <= 9
constexpr int CHUNK = 1024;                // voxels of one workgroup of the count / compact kernels: 256 threads x 4 consecutive voxels
constexpr unsigned kNaNOrd = 0xFFFFFFFFu;

enum { F_NONE = M3D_PEAK_FILTER_NONE, F_MEDIAN = M3D_PEAK_FILTER_MEDIAN, F_MEAN = M3D_PEAK_FILTER_MEAN, F_MAX = M3D_PEAK_FILTER_MAX,
       F_CONST = M3D_PEAK_FILTER_CONST, F_TENSOR = M3D_PEAK_FILTER_TENSOR };

// monotone u32 image of a non-NaN float (-inf lowest ... +inf = 0xFF800000), -0.0 and +0.0 the same; NaN -> 0xFFFFFFFF
__device__ __forceinline__ unsigned ord_of(float v) {
  if (v != v) return kNaNOrd;
  unsigned u = __float_as_uint(v);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord_inv(unsigned k) {
  if (k == kNaNOrd) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ unsigned long long key_of(float v, unsigned idx) {
  const unsigned o = ord_of(v);
  return ((unsigned long long)o << 32) | (o == kNaNOrd ? idx : 0xFFFFFFFFu - idx);
}
__device__ __forceinline__ unsigned long long kmax(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------------------------------------------- thresholds
__global__ __launch_bounds__(1024) void peak_thresh_kernel(const float* __restrict__ x, long long n, int kind, float value,
                                                           const float* __restrict__ thr_in, float* __restrict__ thr) {
  __shared__ unsigned hist[256];
  __shared__ double dsum[1024];
  __shared__ unsigned s_prefix, s_mask, s_k, s_nan;
  const int bc = blockIdx.x, t = threadIdx.x;
  if (kind == F_NONE || kind == F_CONST || kind == F_TENSOR) {
    if (t == 0) thr[bc] = kind == F_NONE ? -INFINITY : (kind == F_CONST ? value : thr_in[bc]);
    return;
  }
  const float* p = x + (size_t)bc * (size_t)n;
  if (kind == F_MEAN) {                      // fp64, fixed order: thread t takes elements t, t + 1024, ..; then a fixed tree
    double s = 0.0;
    for (long long i = t; i < n; i += 1024) s += (double)p[i];
    dsum[t] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
      if (t < w) dsum[t] += dsum[t + w];
      __syncthreads();
    }
    if (t == 0) thr[bc] = (float)(dsum[0] / (double)n);
    return;
  }
  if (kind == F_MAX) {                       // torch.max: NaN if the channel holds one
    unsigned m = 0u;
    for (long long i = t; i < n; i += 1024) { const unsigned k = ord_of(p[i]); m = k > m ? k : m; }
    hist[t & 255] = 0u;
    __syncthreads();
    atomicMax(&hist[t & 255], m);            // LDS integer maximum: order-independent
    __syncthreads();
    if (t == 0) {
      unsigned r = 0u;
      for (int i = 0; i < 256; ++i) r = hist[i] > r ? hist[i] : r;
      thr[bc] = ord_inv(r);
    }
    return;
  }
  // F_MEDIAN: the element of rank (n - 1) / 2 ascending (torch.median's lower median), NaN if any; 8 bits of the key per pass
  if (t == 0) { s_prefix = 0u; s_mask = 0u; s_k = (unsigned)((n - 1) / 2); s_nan = 0u; }
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (t < 256) hist[t] = 0u;
    __syncthreads();
    const unsigned prefix = s_prefix, mask = s_mask;
    bool nan = false;
    for (long long i = t; i < n; i += 1024) {
      const unsigned k = ord_of(p[i]);
      nan |= (k == kNaNOrd);
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
    }
    if (nan) s_nan = 1u;
    __syncthreads();
    if (t == 0) {
      unsigned k = s_k, b = 0;
      for (; b < 255u; ++b) {
        if (k < hist[b]) break;
        k -= hist[b];
      }
      s_k = k; s_prefix = prefix | (b << shift); s_mask = mask | (255u << shift);
    }
    __syncthreads();
  }
  if (t == 0) thr[bc] = s_nan ? __uint_as_float(0x7FC00000u) : ord_inv(s_prefix);
}

// ---------------------------------------------------------------------------------------------------------------- peak map
__global__ __launch_bounds__(256) void peak_map_kernel(const float* __restrict__ x, int S, int H, int W, int o, int tiles_y, int tiles_x,
                                                       long long tiles, int use_thr, const float* __restrict__ thr,
                                                       uint8_t* __restrict__ map) {
  __shared__ unsigned long long A[(TZ + 2 * MAXO) * (TY + 2 * MAXO) * TX];     // maximum over x, tile + z / y halo
  __shared__ unsigned long long Bm[(TZ + 2 * MAXO) * TY * TX];                 // maximum over x and y, tile + z halo
  const long long blk = blockIdx.x;
  const long long bc = blk / tiles;
  int tile = (int)(blk - bc * tiles);
  const int x0 = (tile % tiles_x) * TX; tile /= tiles_x;
  const int y0 = (tile % tiles_y) * TY;
  const int z0 = (tile / tiles_y) * TZ;
  const size_t n = (size_t)S * H * W;
  const float* p = x + (size_t)bc * n;
  const int EZ = TZ + 2 * o, EY = TY + 2 * o;
  const int t = threadIdx.x;
  for (int e = t; e < EZ * EY * TX; e += 256) {
    const int lx = e % TX, ly = (e / TX) % EY, lz = e / (TX * EY);
    const int gz = z0 - o + lz, gy = y0 - o + ly, gx = x0 + lx;
    unsigned long long k = 0ull;                                              // below every key of a voxel
    if (gz >= 0 && gz < S && gy >= 0 && gy < H && gx < W) {
      const unsigned row = ((unsigned)gz * (unsigned)H + (unsigned)gy) * (unsigned)W;
      const int xa = gx - o < 0 ? 0 : gx - o, xb = gx + o > W - 1 ? W - 1 : gx + o;
      for (int xx = xa; xx <= xb; ++xx) k = kmax(k, key_of(p[row + xx], row + xx));
    }
    A[e] = k;
  }
  __syncthreads();
  for (int e = t; e < EZ * TY * TX; e += 256) {
    const int lx = e % TX, ly = (e / TX) % TY, lz = e / (TX * TY);
    unsigned long long k = 0ull;
    for (int j = 0; j <= 2 * o; ++j) k = kmax(k, A[(lz * EY + ly + j) * TX + lx]);
    Bm[e] = k;
  }
  __syncthreads();
  const int lx = t % TX, ly = (t / TX) % TY, lz = t / (TX * TY);
  const int gz = z0 + lz, gy = y0 + ly, gx = x0 + lx;
  if (gz < S && gy < H && gx < W) {
    unsigned long long k = 0ull;
    for (int j = 0; j <= 2 * o; ++j) k = kmax(k, Bm[((lz + j) * TY + ly) * TX + lx]);
    const unsigned idx = ((unsigned)gz * (unsigned)H + (unsigned)gy) * (unsigned)W + (unsigned)gx;
    const float v = p[idx];
    bool peak = (k == key_of(v, idx));
    if (use_thr) peak = peak && (v >= thr[bc]);                               // false for a NaN on either side (:29)
    map[(size_t)bc * n + idx] = peak ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- counts, sums
// chunk (bc, k) = voxels [1024 k, 1024 k + 1024) of channel bc; chunk id = bc * nchunk + k, so chunk order is raster order of the tensor
__global__ __launch_bounds__(256) void peak_count_kernel(const float* __restrict__ x, const uint8_t* __restrict__ map, long long n,
                                                         long long nchunk, int* __restrict__ counts, double* __restrict__ partial) {
  __shared__ double dsum[256];
  __shared__ int csum[256];
  const long long chunk = blockIdx.x;
  const long long bc = chunk / nchunk, k = chunk - bc * nchunk;
  const int t = threadIdx.x;
  const long long i0 = k * CHUNK + 4 * t;
  const size_t base = (size_t)bc * (size_t)n;
  double s = 0.0;
  int c = 0;
  for (int j = 0; j < 4; ++j) {
    if (i0 + j < n) {
      const uint8_t m = map[base + i0 + j];
      s += (double)(x[base + i0 + j] * (float)m);         // input * peak_map (:38): 0 * NaN and 0 * inf are NaN there too
      c += m;
    }
  }
  dsum[t] = s; csum[t] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) { dsum[t] += dsum[t + w]; csum[t] += csum[t + w]; }
    __syncthreads();
  }
  if (t == 0) { counts[chunk] = csum[0]; partial[chunk] = dsum[0]; }
}

__global__ __launch_bounds__(1024) void peak_finish_kernel(const int* __restrict__ counts, const double* __restrict__ partial,
                                                           long long total_chunks, long long nchunk, long long BC,
                                                           long long* __restrict__ offsets, long long* __restrict__ d_num,
                                                           long long* __restrict__ h_num, float* __restrict__ agg) {
  __shared__ int sc[1024];
  __shared__ long long running;
  const int t = threadIdx.x;
  if (t == 0) running = 0;
  __syncthreads();
  for (long long b0 = 0; b0 < total_chunks; b0 += 1024) {
    const int v = (b0 + t < total_chunks) ? counts[b0 + t] : 0;
    sc[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {                 // inclusive scan
      const int a = t >= d ? sc[t - d] : 0;
      __syncthreads();
      sc[t] += a;
      __syncthreads();
    }
    if (b0 + t < total_chunks) offsets[b0 + t] = running + (long long)(sc[t] - v);
    __syncthreads();
    if (t == 1023) running += sc[1023];
    __syncthreads();
  }
  if (t == 0) {
    *d_num = running;
    if (h_num) *h_num = running;
  }
  if (agg) {
    for (long long bc = t; bc < BC; bc += 1024) {        // chunks of a channel in raster order, fp64
      double s = 0.0;
      long long c = 0;
      for (long long k = 0; k < nchunk; ++k) { s += partial[bc * nchunk + k]; c += counts[bc * nchunk + k]; }
      agg[bc] = (float)(s / (double)c);                  // 0 / 0 = NaN (:38-39)
    }
  }
}

__global__ __launch_bounds__(256) void peak_compact_kernel(const uint8_t* __restrict__ map, long long n, long long nchunk, int C, int H,
                                                           int W, const long long* __restrict__ offsets, long long cap,
                                                           int32_t* __restrict__ peaks) {
  __shared__ int sc[256];
  const long long chunk = blockIdx.x;
  const long long bc = chunk / nchunk, k = chunk - bc * nchunk;
  const int t = threadIdx.x;
  const long long i0 = k * CHUNK + 4 * t;
  const size_t base = (size_t)bc * (size_t)n;
  uint8_t m[4];
  int c = 0;
  for (int j = 0; j < 4; ++j) {
    m[j] = (i0 + j < n) ? map[base + i0 + j] : 0;
    c += m[j];
  }
  sc[t] = c;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int a = t >= d ? sc[t - d] : 0;
    __syncthreads();
    sc[t] += a;
    __syncthreads();
  }
  long long row = offsets[chunk] + (long long)(sc[t] - c);
  for (int j = 0; j < 4; ++j) {
    if (!m[j]) continue;
    if (row < cap) {
      const long long i = i0 + j;
      int32_t* r = peaks + row * 5;
      r[0] = (int32_t)(bc / C); r[1] = (int32_t)(bc % C);
      r[2] = (int32_t)(i / ((long long)H * W)); r[3] = (int32_t)((i / W) % H); r[4] = (int32_t)(i % W);
    }
    ++row;
  }
}

__global__ __launch_bounds__(256) void peak_backward_kernel(const uint8_t* __restrict__ map, const float* __restrict__ gy, long long n,
                                                            long long total, float* __restrict__ gx) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256)
    gx[i] = (float)map[i] * gy[i / n];                   // peak_map * grad_output (:47), every element written
}

struct Layout { size_t map, counts, partial, offsets, total; long long nchunk, chunks; };
Layout layout(long long BC, long long n) {
  Layout L;
  L.nchunk = (n + CHUNK - 1) / CHUNK;
  L.chunks = BC * L.nchunk;
  L.map = 0;
  L.counts = m3d::align_up((size_t)BC * (size_t)n, 256);
  L.partial = L.counts + m3d::align_up((size_t)L.chunks * sizeof(int), 256);
  L.offsets = L.partial + m3d::align_up((size_t)L.chunks * sizeof(double), 256);
  L.total = L.offsets + m3d::align_up((size_t)L.chunks * sizeof(long long), 256);
  return L;
}

// the refusals shared by the three entry points; M3D_OK with *empty = true: nothing to do
int check_dims(int B, int C, int S, int H, int W, bool* empty) {
  *empty = false;
  if (B < 0 || C < 0 || S < 1 || H < 1 || W < 1) return M3D_EINVAL;
  if ((long long)S * H * W >= (1ll << 31)) return M3D_EUNSUPPORTED;
  if (B == 0 || C == 0) *empty = true;
  return M3D_OK;
}

}  // namespace

M3D_API size_t m3d_peak_stimulation3d_workspace_bytes(int B, int C, int S, int H, int W, int win) {
  bool empty;
  if (check_dims(B, C, S, H, W, &empty) != M3D_OK || empty || win < 1 || !(win & 1) || win > 2 * MAXO + 1) return 0;
  return layout((long long)B * C, (long long)S * H * W).total;
}

M3D_API int m3d_peak_stimulation3d(const float* d_x, int B, int C, int S, int H, int W, int win, int filter_kind, float filter_value,
                                   const float* d_thresh_in, uint8_t* d_peak_map, int32_t* d_peaks, int cap, int64_t* d_num,
                                   int64_t* h_num, float* d_thresh, float* d_agg, void* d_ws, size_t ws_bytes, void* stream) {
  bool empty;
  if (win < 1 || !(win & 1)) return M3D_EINVAL;
  if (filter_kind < F_NONE || filter_kind > F_TENSOR) return M3D_EINVAL;
  int rc = check_dims(B, C, S, H, W, &empty);
  if (rc != M3D_OK) return rc;
  if (win > 2 * MAXO + 1) return M3D_EUNSUPPORTED;
  if (cap < 0 || !d_num || (cap > 0 && !d_peaks)) return M3D_EINVAL;
  hipStream_t st = m3d::as_stream(stream);
  if (empty) return M3D_OK;                              // no (b,c): nothing is launched, nothing written
  if (!d_x || !d_thresh || !d_ws || (filter_kind == F_TENSOR && !d_thresh_in)) return M3D_EINVAL;
  const long long BC = (long long)B * C, n = (long long)S * H * W;
  const Layout L = layout(BC, n);
  if (ws_bytes < L.total) return M3D_EINVAL;
  const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY, tiles_z = (S + TZ - 1) / TZ;
  const long long tiles = (long long)tiles_x * tiles_y * tiles_z;
  if (BC * tiles >= (1ll << 31) || L.chunks >= (1ll << 31) || BC >= (1ll << 31)) return M3D_EUNSUPPORTED;   // one grid dimension
  char* ws = static_cast<char*>(d_ws);
  uint8_t* map = d_peak_map ? d_peak_map : reinterpret_cast<uint8_t*>(ws + L.map);
  int* counts = reinterpret_cast<int*>(ws + L.counts);
  double* partial = reinterpret_cast<double*>(ws + L.partial);
  long long* offsets = reinterpret_cast<long long*>(ws + L.offsets);
  hipLaunchKernelGGL(peak_thresh_kernel, dim3((unsigned)BC), dim3(1024), 0, st, d_x, n, filter_kind, filter_value, d_thresh_in, d_thresh);
  hipLaunchKernelGGL(peak_map_kernel, dim3((unsigned)(BC * tiles)), dim3(256), 0, st, d_x, S, H, W, win / 2, tiles_y, tiles_x, tiles,
                     filter_kind != F_NONE ? 1 : 0, (const float*)d_thresh, map);
  hipLaunchKernelGGL(peak_count_kernel, dim3((unsigned)L.chunks), dim3(256), 0, st, d_x, (const uint8_t*)map, n, L.nchunk, counts, partial);
  hipLaunchKernelGGL(peak_finish_kernel, dim3(1), dim3(1024), 0, st, (const int*)counts, (const double*)partial, L.chunks, L.nchunk, BC,
                     offsets, reinterpret_cast<long long*>(d_num), reinterpret_cast<long long*>(h_num), d_agg);
  if (cap > 0)
    hipLaunchKernelGGL(peak_compact_kernel, dim3((unsigned)L.chunks), dim3(256), 0, st, (const uint8_t*)map, n, L.nchunk, C, H, W,
                       (const long long*)offsets, (long long)cap, d_peaks);
  return m3d::check_launch("peak_stimulation3d");
}

M3D_API int m3d_peak_stimulation3d_backward(const uint8_t* d_peak_map, const float* d_gy, int B, int C, int S, int H, int W, float* d_gx,
                                            void* stream) {
  bool empty;
  int rc = check_dims(B, C, S, H, W, &empty);
  if (rc != M3D_OK) return rc;
  if (empty) return M3D_OK;
  if (!d_peak_map || !d_gy || !d_gx) return M3D_EINVAL;
  const long long n = (long long)S * H * W, total = (long long)B * C * n;
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(peak_backward_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, m3d::as_stream(stream),
                     d_peak_map, d_gy, n, total, d_gx);
  return m3d::check_launch("peak_stimulation3d_backward");
}
