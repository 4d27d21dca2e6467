// Evaluation of instance-label volumes for gfx950 (integer work and fp64 divides; HBM / atomic bound).
// Reference (tools/evaluation/):
//   eval_instance_segmentation_soma.py:186-202  one full-volume bool mask per predicted and per GT instance, then
//       mask_iou.py:50-68 mask_iou_fast: a P x G x V triple loop, iou[n,k] = float32(inter / union) with both counts exact in fp64.
//       Masks on one side are `labels == id`, hence disjoint: a contingency table of (pred id, GT id) voxel counts gives every entry.
//   evaluation_nuclei_f1score_seg.py:88-133  Σ(pred>0), Σ(gt>0) and Σ(keep & gt>0), keep = pred>0 inside the union of the TP boxes.
//
// m3d_label_overlap (the hot path) - one streaming pass over the two volumes:
//   1. every thread reads 16 consecutive voxels and folds runs of equal (a, b) in registers (label volumes are runs along x);
//   2. each run goes into the workgroup's LDS hash table (2048 slots, 64-bit CAS to claim a key, 32-bit add for the count); a run
//      whose key finds no slot within 32 probes goes to the global table directly;
//   3. at the end the workgroup flushes its LDS table into the global open-addressed table (linear probing, 64-bit keys
//      (a << 24 | b) + 1, 0 = empty): one global atomic per distinct pair per workgroup instead of one per voxel;
//   4. one pass over the table scatters the pair counts into count_a / count_b (the (a, 0) / (0, b) / (0, 0) keys included, so the
//      per-label counts need no pass of their own) and counts the pairs with a > 0 and b > 0 per pred label;
//   5. a tiled scan turns those counts into bucket offsets, the pairs are placed into their pred-label bucket and finally written
//      at offset + rank of b within the bucket: the list is sorted by (a, b) and, counts being integers, bit-identical run to run.
// Labels above the declared maxima (or >= 2^24, or negative int32) are never used as an index: they set bit 0 of d_status[0].
// A key that finds no global slot within min(capacity, 1024) probes sets bit 1 ("table full"); the caller re-launches with a
// larger table.  Nothing is dropped silently.
#include "m3d_common.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kPerThread = 16;                 // voxels per thread and step: 32 B of uint16 / 64 B of int32 labels
constexpr int kLdsSlots = 2048;                // 24 KB of LDS per workgroup
constexpr int kLdsProbes = 32;
constexpr int kGlobalProbes = 1024;
constexpr uint32_t kLabelLimit = 1u << 24;
constexpr int kScanThreads = 1024;

__device__ __forceinline__ uint32_t slot_hash(u64 key) {
  const u64 h = key * 0x9E3779B97F4A7C15ull;
  return (uint32_t)(h >> 40) ^ (uint32_t)(h >> 17);
}

__device__ __forceinline__ bool global_insert(u64* keys, uint32_t* counts, u64 mask, int probes, u64 key, uint32_t c) {
  u64 h = slot_hash(key) & mask;
  for (int p = 0; p < probes; ++p) {
    u64 k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == 0) {
      k = atomicCAS(&keys[h], 0ull, key);
      if (k == 0) k = key;
    }
    if (k == key) {
      atomicAdd(&counts[h], c);
      return true;
    }
    h = (h + 1) & mask;
  }
  return false;
}

__device__ __forceinline__ bool lds_insert(u64* lkeys, uint32_t* lcnt, u64 key, uint32_t c) {
  uint32_t h = slot_hash(key) & (kLdsSlots - 1);
  for (int p = 0; p < kLdsProbes; ++p) {
    u64 k = __hip_atomic_load(&lkeys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == 0) {
      k = atomicCAS(&lkeys[h], 0ull, key);
      if (k == 0) k = key;
    }
    if (k == key) {
      atomicAdd(&lcnt[h], c);
      return true;
    }
    h = (h + 1) & (kLdsSlots - 1);
  }
  return false;
}

// n <= 16 labels from p[v0..] as uint32 (int32 labels keep their bits: a negative one becomes >= 2^31 and fails the range test)
template <typename T, int N>
__device__ __forceinline__ int load_labels(const T* p, long long v0, long long V, bool vec, uint32_t* out) {
  if (v0 >= V) return 0;
  if (vec && v0 + N <= V) {
    constexpr int nv = N * (int)sizeof(T) / 16;
    const uint4* q = reinterpret_cast<const uint4*>(p + v0);
    uint4 w[nv];
#pragma unroll
    for (int i = 0; i < nv; ++i) w[i] = q[i];
    const T* t = reinterpret_cast<const T*>(w);
#pragma unroll
    for (int j = 0; j < N; ++j) out[j] = (uint32_t)t[j];
    return N;
  }
  const int n = (int)((V - v0) < N ? (V - v0) : N);
  for (int j = 0; j < n; ++j) out[j] = (uint32_t)p[v0 + j];
  return n;
}

__device__ __forceinline__ void or_status(u64* status, uint32_t flags) {
  if (flags) atomicOr(&status[0], (u64)flags);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void overlap_pass(const T* __restrict__ a, const T* __restrict__ b, long long V, uint32_t max_a,
                                                         uint32_t max_b, bool vec, u64* keys, uint32_t* counts, u64 mask, int probes,
                                                         u64* status) {
  __shared__ u64 lkeys[kLdsSlots];
  __shared__ uint32_t lcnt[kLdsSlots];
  for (int i = threadIdx.x; i < kLdsSlots; i += kThreads) {
    lkeys[i] = 0;
    lcnt[i] = 0;
  }
  __syncthreads();
  uint32_t flags = 0;
  const long long step = (long long)kThreads * kPerThread;
  for (long long base = (long long)blockIdx.x * step; base < V; base += (long long)gridDim.x * step) {
    const long long v0 = base + (long long)threadIdx.x * kPerThread;
    uint32_t la[kPerThread], lb[kPerThread];
    const int n = load_labels<T, kPerThread>(a, v0, V, vec, la);
    load_labels<T, kPerThread>(b, v0, V, vec, lb);
    u64 cur = 0;
    uint32_t run = 0;
    for (int j = 0; j < n; ++j) {
      const uint32_t x = la[j], y = lb[j];
      if (x > max_a || y > max_b) {       // max_a, max_b < 2^24 (checked on the host): also rejects >= 2^24 and negative int32
        flags |= 1u;
        continue;
      }
      const u64 key = (((u64)x << 24) | y) + 1;
      if (key != cur) {
        if (run && !lds_insert(lkeys, lcnt, cur, run) && !global_insert(keys, counts, mask, probes, cur, run)) flags |= 2u;
        cur = key;
        run = 0;
      }
      ++run;
    }
    if (run && !lds_insert(lkeys, lcnt, cur, run) && !global_insert(keys, counts, mask, probes, cur, run)) flags |= 2u;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kLdsSlots; i += kThreads) {
    const u64 k = lkeys[i];
    if (k && !global_insert(keys, counts, mask, probes, k, lcnt[i])) flags |= 2u;
  }
  or_status(status, flags);
}

// table -> count_a / count_b (all keys), per-pred-label pair counts nb[a] and the number of pairs (a > 0 and b > 0)
__global__ __launch_bounds__(kThreads) void overlap_scatter(const u64* __restrict__ keys, const uint32_t* __restrict__ counts, long long cap,
                                                            uint32_t max_a, uint32_t max_b, u64* count_a, u64* count_b, int* nb) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < cap; i += (long long)gridDim.x * kThreads) {
    const u64 k = keys[i];
    if (!k) continue;
    const uint32_t x = (uint32_t)((k - 1) >> 24), y = (uint32_t)((k - 1) & (kLabelLimit - 1));
    if (x > max_a || y > max_b) continue;   // never inserted; kept as a bound on every index below
    const u64 c = counts[i];
    atomicAdd(&count_a[x], c);
    atomicAdd(&count_b[y], c);
    if (x && y) atomicAdd(&nb[x], 1);
  }
}

// Bucket offsets offs[0..n] = exclusive prefix sums of nb[0..n) (n = max_a + 1 labels) in three launches: per-tile totals, one
// workgroup scans the (<= 16 K) tile totals, every tile scans itself from its offset.  nb is zeroed on the way (it becomes the
// placement cursor); offs[n] = d_status[1] = the number of pairs.
constexpr int kScanTile = kThreads * 4;

// exclusive prefix of v over the workgroup and its total (one call per kernel: wsum is not re-synchronised)
__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
  __shared__ int wsum[kThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kThreads / 64; ++w) {
    before += w < wv ? wsum[w] : 0;
    all += wsum[w];
  }
  *total = all;
  return before + x - v;
}

__global__ __launch_bounds__(kThreads) void tile_sums(const int* __restrict__ nb, int n, int* tsum) {
  const int i0 = blockIdx.x * kScanTile + threadIdx.x * 4;
  int s = 0;
  for (int j = 0; j < 4; ++j) s += i0 + j < n ? nb[i0 + j] : 0;
  int tot;
  block_exclusive_scan(s, &tot);
  if (threadIdx.x == 0) tsum[blockIdx.x] = tot;
}

// one workgroup: in-place exclusive scan of v[0..n), total -> *total_out and status[1]
__global__ __launch_bounds__(kScanThreads) void scan_tile_sums(int* v, int n, int* total_out, u64* status) {
  __shared__ int part[kScanThreads];
  const int per = (n + kScanThreads - 1) / kScanThreads;
  const int lo = threadIdx.x * per, hi = min(n, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {     // Hillis-Steele inclusive scan of the per-thread totals
    const int x = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  int run = part[threadIdx.x] - s;
  for (int i = lo; i < hi; ++i) {
    const int x = v[i];
    v[i] = run;
    run += x;
  }
  if (threadIdx.x == kScanThreads - 1) {
    *total_out = part[kScanThreads - 1];
    status[1] = (u64)part[kScanThreads - 1];
  }
}

__global__ __launch_bounds__(kThreads) void tile_scan(int* nb, int n, const int* __restrict__ toffs, int* offs) {
  const int i0 = blockIdx.x * kScanTile + threadIdx.x * 4;
  int v[4], s = 0;
  for (int j = 0; j < 4; ++j) {
    v[j] = i0 + j < n ? nb[i0 + j] : 0;
    s += v[j];
  }
  int tot;
  int run = toffs[blockIdx.x] + block_exclusive_scan(s, &tot);
  for (int j = 0; j < 4; ++j) {
    if (i0 + j < n) {
      offs[i0 + j] = run;
      nb[i0 + j] = 0;
    }
    run += v[j];
  }
}

__global__ __launch_bounds__(kThreads) void bucket_place(const u64* __restrict__ keys, const uint32_t* __restrict__ counts, long long cap,
                                                         uint32_t max_a, uint32_t max_b, const int* __restrict__ offs, int* cursor,
                                                         u64* tmp_key, uint32_t* tmp_cnt) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < cap; i += (long long)gridDim.x * kThreads) {
    const u64 k = keys[i];
    if (!k) continue;
    const uint32_t x = (uint32_t)((k - 1) >> 24), y = (uint32_t)((k - 1) & (kLabelLimit - 1));
    if (!x || !y || x > max_a || y > max_b) continue;
    const int pos = offs[x] + atomicAdd(&cursor[x], 1);
    tmp_key[pos] = k - 1;
    tmp_cnt[pos] = counts[i];
  }
}

// position = bucket offset + rank of b among the bucket's entries (b values within a bucket are distinct)
__global__ __launch_bounds__(kThreads) void bucket_rank(const u64* __restrict__ tmp_key, const uint32_t* __restrict__ tmp_cnt, long long cap,
                                                        const int* __restrict__ offs, const u64* status, int32_t* pairs,
                                                        int64_t* pair_counts) {
  const long long np = (long long)status[1];
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < np && i < cap; i += (long long)gridDim.x * kThreads) {
    const u64 k = tmp_key[i];
    const uint32_t x = (uint32_t)(k >> 24), y = (uint32_t)(k & (kLabelLimit - 1));
    const int lo = offs[x], hi = offs[x + 1];
    int r = 0;
    for (int j = lo; j < hi; ++j) r += (uint32_t)(tmp_key[j] & (kLabelLimit - 1)) < y;
    const long long o = lo + r;
    pairs[2 * o] = (int32_t)x;
    pairs[2 * o + 1] = (int32_t)y;
    pair_counts[o] = (int64_t)tmp_cnt[i];
  }
}

// one thread per row: the pairs of pred id `id` are the contiguous run with a == id of the sorted list
__global__ __launch_bounds__(kThreads) void iou_best(const int32_t* __restrict__ pairs, const int64_t* __restrict__ pcnt, long long np,
                                                     const int64_t* __restrict__ count_a, int max_a, const int64_t* __restrict__ count_b,
                                                     int max_b, const int32_t* __restrict__ col, int num_cols, const int32_t* __restrict__ rows,
                                                     int num_rows, float* max_iou, int32_t* argmax, float* dense) {
  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= num_rows) return;
  const int id = rows[r];
  float best = 0.0f;
  int bcol = 0;
  if (id >= 1 && id <= max_a) {
    long long lo = 0, hi = np;                       // lower_bound of a == id
    while (lo < hi) {
      const long long m = (lo + hi) >> 1;
      if (pairs[2 * m] < id) lo = m + 1; else hi = m;
    }
    const double na = (double)count_a[id];
    for (long long i = lo; i < np && pairs[2 * i] == id; ++i) {
      const int gb = pairs[2 * i + 1];
      if (gb > max_b) continue;
      const int c = col[gb];
      if (c < 0 || c >= num_cols) continue;
      const double inter = (double)pcnt[i];
      // mask_iou.py:57-67: intersect and union counted in fp64 (exact integers), one division, one rounding to fp32
      const float v = (float)(inter / (na + (double)count_b[gb] - inter));
      if (dense) dense[(long long)r * num_cols + c] = v;
      if (v > best || (v == best && c < bcol)) {      // np.argmax: the first (lowest) column of the largest fp32 value
        best = v;
        bcol = c;
      }
    }
  }
  max_iou[r] = best;
  argmax[r] = bcol;
}

__global__ __launch_bounds__(kThreads) void box_paint(const int32_t* __restrict__ ranges, int num_boxes, int D, int H, int W, uint32_t* bits) {
  for (int k = blockIdx.x; k < num_boxes; k += gridDim.x) {
    const int32_t* q = ranges + 6 * k;
    const int z0 = max(q[0], 0), z1 = min(q[1], D), y0 = max(q[2], 0), y1 = min(q[3], H), x0 = max(q[4], 0), x1 = min(q[5], W);
    if (z1 <= z0 || y1 <= y0 || x1 <= x0) continue;
    const int ny = y1 - y0, rows = (z1 - z0) * ny;
    for (int r = threadIdx.x; r < rows; r += kThreads) {
      const long long row = ((long long)(z0 + r / ny) * H + (y0 + r % ny)) * W;
      const long long b0 = row + x0, b1 = row + x1;            // bits [b0, b1)
      for (long long w = b0 >> 5; w <= (b1 - 1) >> 5; ++w) {
        const long long lo = max(b0, w * 32) - w * 32, hi = min(b1, w * 32 + 32) - w * 32;
        const uint32_t m = (hi - lo == 32) ? 0xFFFFFFFFu : (((1u << (hi - lo)) - 1u) << lo);
        atomicOr(&bits[w], m);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void box_count(const T* __restrict__ pred, const T* __restrict__ gt, long long V, bool vec,
                                                      const uint32_t* __restrict__ bits, u64* out) {
  u64 np = 0, ng = 0, nt = 0;
  const long long words = (V + 31) >> 5;
  for (long long w = (long long)blockIdx.x * kThreads + threadIdx.x; w < words; w += (long long)gridDim.x * kThreads) {
    const uint32_t m = bits[w];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      uint32_t p[16], g[16];
      const long long v0 = w * 32 + h * 16;
      const int n = load_labels<T, 16>(pred, v0, V, vec, p);
      load_labels<T, 16>(gt, v0, V, vec, g);
      for (int j = 0; j < n; ++j) {
        const bool pp = p[j] != 0, gg = g[j] != 0;
        np += pp;
        ng += gg;
        nt += pp && gg && ((m >> (h * 16 + j)) & 1u);
      }
    }
  }
  __shared__ u64 red[3][kThreads / 64];
  for (int o = 32; o > 0; o >>= 1) {
    np += __shfl_down(np, o);
    ng += __shfl_down(ng, o);
    nt += __shfl_down(nt, o);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wv] = np;
    red[1][wv] = ng;
    red[2][wv] = nt;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    u64 s = 0;
    for (int i = 0; i < kThreads / 64; ++i) s += red[threadIdx.x][i];
    if (s) atomicAdd(&out[threadIdx.x], s);
  }
}

struct OverlapWs {
  u64* keys; uint32_t* counts; int* nb; int* offs; int* tsum; u64* tmp_key; uint32_t* tmp_cnt; size_t bytes;
};
OverlapWs overlap_ws(char* base, int max_a, long long cap) {
  OverlapWs w;
  size_t o = 0;
  auto take = [&](size_t n) { const size_t r = o; o = m3d::align_up(o + n, 256); return base ? base + r : nullptr; };
  w.keys = (u64*)take(sizeof(u64) * cap);
  w.counts = (uint32_t*)take(sizeof(uint32_t) * cap);
  w.nb = (int*)take(sizeof(int) * ((size_t)max_a + 1));
  w.offs = (int*)take(sizeof(int) * ((size_t)max_a + 2));
  w.tsum = (int*)take(sizeof(int) * (((size_t)max_a + kScanTile) / kScanTile));
  w.tmp_key = (u64*)take(sizeof(u64) * cap);
  w.tmp_cnt = (uint32_t*)take(sizeof(uint32_t) * cap);
  w.bytes = o;
  return w;
}

bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }
int grid_for(long long n, int cap) { const long long g = (n + kThreads - 1) / kThreads; return (int)(g < 1 ? 1 : (g > cap ? cap : g)); }

}  // namespace

M3D_API size_t m3d_label_overlap_workspace_bytes(int max_a, int64_t capacity) {
  if (max_a < 0 || max_a >= (int)kLabelLimit || !pow2(capacity)) return 0;
  return overlap_ws(nullptr, max_a, capacity).bytes;
}

M3D_API int m3d_label_overlap(const void* d_a, const void* d_b, int label_bytes, int64_t num_voxels, int max_a, int max_b, int64_t capacity,
                              int64_t* d_count_a, int64_t* d_count_b, int32_t* d_pairs, int64_t* d_pair_counts, int64_t* d_status,
                              void* d_ws, size_t ws_bytes, void* stream) {
  if ((label_bytes != 2 && label_bytes != 4) || num_voxels < 0 || num_voxels >= (1LL << 31) || max_a < 0 || max_b < 0 ||
      max_a >= (int)kLabelLimit || max_b >= (int)kLabelLimit || !pow2(capacity) || capacity >= (1LL << 31) || !d_count_a || !d_count_b ||
      !d_pairs || !d_pair_counts || !d_status || (num_voxels > 0 && (!d_a || !d_b)))
    return M3D_EINVAL;
  const OverlapWs w = overlap_ws((char*)d_ws, max_a, capacity);
  if (!d_ws || ws_bytes < w.bytes) return M3D_EWORKSPACE;
  hipStream_t st = m3d::as_stream(stream);
  u64* status = reinterpret_cast<u64*>(d_status);
  if (hipMemsetAsync(w.keys, 0, sizeof(u64) * capacity, st) != hipSuccess ||
      hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * capacity, st) != hipSuccess ||
      hipMemsetAsync(w.nb, 0, sizeof(int) * ((size_t)max_a + 1), st) != hipSuccess ||
      hipMemsetAsync(d_count_a, 0, sizeof(int64_t) * ((size_t)max_a + 1), st) != hipSuccess ||
      hipMemsetAsync(d_count_b, 0, sizeof(int64_t) * ((size_t)max_b + 1), st) != hipSuccess ||
      hipMemsetAsync(d_status, 0, 2 * sizeof(int64_t), st) != hipSuccess)
    return M3D_ELAUNCH;
  const u64 mask = (u64)capacity - 1;
  const int probes = capacity < kGlobalProbes ? (int)capacity : kGlobalProbes;
  if (num_voxels > 0) {
    const long long step = (long long)kThreads * kPerThread;
    long long g = (num_voxels + step - 1) / step;
    if (g > 1024) g = 1024;                       // 4 workgroups per CU, each loops: its LDS table then folds more voxels per flush
    const bool vec = ((uintptr_t)d_a % 16 == 0) && ((uintptr_t)d_b % 16 == 0);
    if (label_bytes == 2)
      overlap_pass<uint16_t><<<(int)g, kThreads, 0, st>>>((const uint16_t*)d_a, (const uint16_t*)d_b, num_voxels, (uint32_t)max_a,
                                                          (uint32_t)max_b, vec, w.keys, w.counts, mask, probes, status);
    else
      overlap_pass<int32_t><<<(int)g, kThreads, 0, st>>>((const int32_t*)d_a, (const int32_t*)d_b, num_voxels, (uint32_t)max_a,
                                                         (uint32_t)max_b, vec, w.keys, w.counts, mask, probes, status);
  }
  const int gs = grid_for(capacity, 2048);
  overlap_scatter<<<gs, kThreads, 0, st>>>(w.keys, w.counts, capacity, (uint32_t)max_a, (uint32_t)max_b, (u64*)d_count_a, (u64*)d_count_b,
                                           w.nb);
  const int n = max_a + 1, tiles = (n + kScanTile - 1) / kScanTile;
  tile_sums<<<tiles, kThreads, 0, st>>>(w.nb, n, w.tsum);
  scan_tile_sums<<<1, kScanThreads, 0, st>>>(w.tsum, tiles, w.offs + n, status);
  tile_scan<<<tiles, kThreads, 0, st>>>(w.nb, n, w.tsum, w.offs);
  bucket_place<<<gs, kThreads, 0, st>>>(w.keys, w.counts, capacity, (uint32_t)max_a, (uint32_t)max_b, w.offs, w.nb, w.tmp_key, w.tmp_cnt);
  bucket_rank<<<gs, kThreads, 0, st>>>(w.tmp_key, w.tmp_cnt, capacity, w.offs, status, d_pairs, d_pair_counts);
  return m3d::check_launch("label_overlap");
}

M3D_API int m3d_label_iou_best(const int32_t* d_pairs, const int64_t* d_pair_counts, int64_t num_pairs, const int64_t* d_count_a, int max_a,
                               const int64_t* d_count_b, int max_b, const int32_t* d_gt_col, int num_cols, const int32_t* d_row_ids,
                               int num_rows, float* d_max_iou, int32_t* d_argmax, float* d_iou, void* stream) {
  if (num_pairs < 0 || num_rows < 0 || num_cols < 0 || max_a < 0 || max_b < 0 || (num_pairs > 0 && (!d_pairs || !d_pair_counts)) ||
      !d_count_a || !d_count_b || !d_gt_col)
    return M3D_EINVAL;
  if (num_rows == 0) return M3D_OK;
  if (!d_row_ids || !d_max_iou || !d_argmax) return M3D_EINVAL;
  hipStream_t st = m3d::as_stream(stream);
  if (d_iou && num_cols > 0 && hipMemsetAsync(d_iou, 0, sizeof(float) * (size_t)num_rows * num_cols, st) != hipSuccess) return M3D_ELAUNCH;
  iou_best<<<(num_rows + kThreads - 1) / kThreads, kThreads, 0, st>>>(d_pairs, d_pair_counts, num_pairs, d_count_a, max_a, d_count_b, max_b,
                                                                     d_gt_col, num_cols, d_row_ids, num_rows, d_max_iou, d_argmax,
                                                                     num_cols > 0 ? d_iou : nullptr);
  return m3d::check_launch("label_iou_best");
}

M3D_API size_t m3d_box_union_overlap_workspace_bytes(int64_t num_voxels) {
  return num_voxels < 0 ? 0 : m3d::align_up(sizeof(uint32_t) * (size_t)((num_voxels + 31) / 32), 256) + 256;
}

M3D_API int m3d_box_union_overlap_counts(const void* d_pred, const void* d_gt, int label_bytes, int depth, int height, int width,
                                         const int32_t* d_ranges, int num_boxes, int64_t* d_counts, void* d_ws, size_t ws_bytes,
                                         void* stream) {
  if ((label_bytes != 2 && label_bytes != 4) || depth < 0 || height < 0 || width < 0 || num_boxes < 0 || !d_counts ||
      (num_boxes > 0 && !d_ranges))
    return M3D_EINVAL;
  const long long V = (long long)depth * height * width;
  if (V > 0 && (!d_pred || !d_gt)) return M3D_EINVAL;
  if (!d_ws || ws_bytes < m3d_box_union_overlap_workspace_bytes(V)) return M3D_EWORKSPACE;
  hipStream_t st = m3d::as_stream(stream);
  const long long words = (V + 31) / 32;
  uint32_t* bits = (uint32_t*)d_ws;
  if (hipMemsetAsync(d_counts, 0, 3 * sizeof(int64_t), st) != hipSuccess) return M3D_ELAUNCH;
  if (V == 0) return M3D_OK;
  if (hipMemsetAsync(bits, 0, sizeof(uint32_t) * words, st) != hipSuccess) return M3D_ELAUNCH;
  if (num_boxes > 0) box_paint<<<num_boxes < 4096 ? num_boxes : 4096, kThreads, 0, st>>>(d_ranges, num_boxes, depth, height, width, bits);
  const bool vec = ((uintptr_t)d_pred % 16 == 0) && ((uintptr_t)d_gt % 16 == 0);
  const int g = grid_for(words, 2048);
  if (label_bytes == 2)
    box_count<uint16_t><<<g, kThreads, 0, st>>>((const uint16_t*)d_pred, (const uint16_t*)d_gt, V, vec, bits, (u64*)d_counts);
  else
    box_count<int32_t><<<g, kThreads, 0, st>>>((const int32_t*)d_pred, (const int32_t*)d_gt, V, vec, bits, (u64*)d_counts);
  return m3d::check_launch("box_union_overlap_counts");
}
