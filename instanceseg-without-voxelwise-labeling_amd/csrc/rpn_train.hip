// RPN training step on the device (reference: lib/roi_data/rpn.py:120-279 -> lib/modeling/rpn_heads.py:140-170, sigmoid branch):
// anchor labelling over the whole wide field, seeded sampling, regression targets, the dense "wide" export, and the fused loss with
// its gradients.  Nothing of size anchors x boxes is ever stored: the label pass recomputes the IoUs the per-box maxima came from.
//
//   gt_max_kernel     per ground-truth box the largest IoU over all inside anchors: LDS atomicMax per hit, one global atomicMax per
//                     box and workgroup.  IoUs are >= 0, so their bit patterns order like the values and an integer max does not
//                     depend on arrival order.
//   label_kernel      fg = tie with a box's maximum (fp32 equality, 0 == 0 included) or max IoU >= positive threshold; the fg anchors
//                     are appended to a list (an unordered SET; everything downstream orders by value), the bg candidates become one
//                     bit per anchor in field order.
//   scan_kernel       exclusive prefix of the candidate bits per 64-bit word (one workgroup).
//   draw_kernel       draw j picks candidate r_j = (key(2^40 + j) * n) >> 32: binary search over the word prefixes, then the r-th set bit.
//   finalize_kernel   one workgroup: radix-select the num_fg smallest (key, index) of the fg set, sort, fold duplicate draws, flip the
//                     fg anchors a draw hit, regression targets, counts.
//   wide_kernel       scatter into the four dense blobs;  loss_kernel: both losses and both gradients, O(batch) work.
#include "box_common.h"
#include "train_common.h"

namespace {
using namespace m3dbox;
using namespace m3dtrain;

constexpr int kMaxA = 64;          // cell anchors per position (PropParams has the same limit)
constexpr int kChunk = 256;        // ground-truth boxes per LDS chunk
constexpr int kTPB = 256;          // threads per workgroup of the two field passes
constexpr int kPerThread = 4;      // anchors per thread there: one workgroup covers 1024 consecutive anchors = 16 candidate words
constexpr int kMaxBatch = 4096;    // RPN_BATCH_SIZE_PER_IM limit: the finalize kernel's rank sorts are quadratic in it (shipped: 64 / 128)
enum { C_FG = 0, C_INSIDE, C_CAND, C_COUNT = 8 };

struct Geom {
  double cell[6 * kMaxA];          // generate_anchors_3d rows (fp64, data_utils.py:62-64)
  double t, im_w, im_h, im_s;      // RPN_STRADDLE_THRESH and the image extent (rpn.py:124-135)
  float pos, neg;                  // thresholds as fp32: NumPy compares the fp32 IoU array with a weak Python scalar (rpn.py:177,202)
  int A, F, stride, K, Kdc;
  unsigned int N, F3;
};

struct Ws {
  unsigned int* cnt;               // [C_COUNT] counters, then gt_max [K] (float bits)
  unsigned int* gt_max;
  unsigned long long* bits;        // [nwords] bg candidates, bit i%64 of word i/64, i = flat field index
  unsigned int* wordpref;          // [nwords] exclusive prefix of popcounts
  unsigned int* fglist;            // [N] flat field indices of the fg anchors before sampling, any order
  unsigned int *kept_a, *kept_s;   // [num_fg] sampled fg: as gathered / sorted by wide index
  unsigned int *draws, *drw_s, *bgu;   // [batch] bg draws: by j / sorted by wide index / duplicates folded
  size_t bytes;
  unsigned int nwords;
};

inline Ws carve(void* base, unsigned int N, int K, int num_fg, int batch) {
  Ws w;
  char* p = reinterpret_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t n) { char* q = p ? p + off : nullptr; off += m3d::align_up(n, 256); return q; };
  w.nwords = (unsigned int)(((size_t)N + kTPB * kPerThread - 1) / (kTPB * kPerThread)) * (kTPB * kPerThread / 64);
  w.cnt = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * ((size_t)C_COUNT + (K > 0 ? K : 0))));
  w.gt_max = w.cnt ? w.cnt + C_COUNT : nullptr;
  w.bits = reinterpret_cast<unsigned long long*>(take(sizeof(unsigned long long) * w.nwords));
  w.wordpref = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * w.nwords));
  w.fglist = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * (size_t)N));
  w.kept_a = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * (size_t)(num_fg > 0 ? num_fg : 1)));
  w.kept_s = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * (size_t)(num_fg > 0 ? num_fg : 1)));
  w.draws = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * (size_t)batch));
  w.drw_s = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * (size_t)batch));
  w.bgu = reinterpret_cast<unsigned int*>(take(sizeof(unsigned int) * (size_t)batch));
  w.bytes = off;
  return w;
}

// The sampling contract (DESIGN, "RPN training targets"): seed_stream / mix_key of train_common.h
__device__ inline unsigned long long fg_order(unsigned long long seed, unsigned int i) {
  return ((unsigned long long)mix_key(seed, i) << 32) | i;
}

// anchor i = position i / A (z-major, x-minor), cell anchor i % A: fp64 cell anchor + integer shift, rounded to fp32 (data_utils.py:88-94)
__device__ inline void anchor_of(const double* cell, const Geom& g, unsigned int i, float* b) {
  const unsigned int pos = i / (unsigned int)g.A, a = i % (unsigned int)g.A;
  const unsigned int x = pos % (unsigned int)g.F, y = (pos / (unsigned int)g.F) % (unsigned int)g.F, z = pos / ((unsigned int)g.F * g.F);
  const double sx = (double)((long long)x * g.stride), sy = (double)((long long)y * g.stride), sz = (double)((long long)z * g.stride);
  const double* c = cell + 6 * a;
  b[0] = (float)(c[0] + sx); b[1] = (float)(c[1] + sy); b[2] = (float)(c[2] + sz);
  b[3] = (float)(c[3] + sx); b[4] = (float)(c[4] + sy); b[5] = (float)(c[5] + sz);
}
__device__ inline bool anchor_inside(const Geom& g, const float* b) {   // rpn.py:124-140
  if (g.t < 0) return true;
  return (double)b[0] >= -g.t && (double)b[1] >= -g.t && (double)b[2] >= -g.t && (double)b[3] < g.im_w + g.t &&
         (double)b[4] < g.im_h + g.t && (double)b[5] < g.im_s + g.t;
}
__device__ inline unsigned long long wide_of(const Geom& g, unsigned int i) {   // [A,F,F,F] layout of rpn.py:260-261
  return (unsigned long long)(i % (unsigned int)g.A) * g.F3 + i / (unsigned int)g.A;
}

__device__ inline void load_boxes(float* q, const float* src, int k0, int kc) {   // 8 floats per box: the box, its volume, pad
  for (int k = threadIdx.x; k < kc; k += blockDim.x) {
    const float* s = src + 6 * (size_t)(k0 + k);
    float* d = q + 8 * k;
#pragma unroll
    for (int c = 0; c < 6; ++c) d[c] = s[c];
    d[6] = iou_query_volume(s);
    d[7] = 0.f;
  }
}

__global__ __launch_bounds__(kTPB) void gt_max_kernel(Geom g, const float* __restrict__ gt, unsigned int* __restrict__ gt_max) {
  __shared__ double cell[6 * kMaxA];
  __shared__ float q[8 * kChunk];
  __shared__ unsigned int smax[kChunk];
  for (int c = threadIdx.x; c < 6 * g.A; c += kTPB) cell[c] = g.cell[c];
  __syncthreads();
  float b[kPerThread][6];
  bool in[kPerThread];
  int any = 0;
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    const unsigned long long i = ((unsigned long long)blockIdx.x * kPerThread + u) * kTPB + threadIdx.x;
    in[u] = false;
    if (i < g.N) {
      anchor_of(cell, g, (unsigned int)i, b[u]);
      in[u] = anchor_inside(g, b[u]);
    }
    any |= in[u];
  }
  if (!__syncthreads_or(any)) return;
  for (int k0 = 0; k0 < g.K; k0 += kChunk) {
    const int kc = g.K - k0 < kChunk ? g.K - k0 : kChunk;
    __syncthreads();
    load_boxes(q, gt, k0, kc);
    for (int k = threadIdx.x; k < kc; k += kTPB) smax[k] = 0u;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
      if (!in[u]) continue;
      for (int k = 0; k < kc; ++k) {
        const float v = iou3d(b[u], q + 8 * k, q[8 * k + 6]);
        if (v > 0.f) atomicMax(&smax[k], __float_as_uint(v));
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kc; k += kTPB)
      if (smax[k]) atomicMax(&gt_max[k0 + k], smax[k]);
  }
}

__global__ __launch_bounds__(kTPB) void label_kernel(Geom g, const float* __restrict__ gt, const float* __restrict__ dc,
                                                     const unsigned int* __restrict__ gt_max, unsigned int* __restrict__ cnt,
                                                     unsigned int* __restrict__ fglist, unsigned long long* __restrict__ bits) {
  __shared__ double cell[6 * kMaxA];
  __shared__ float q[8 * kChunk];
  __shared__ float smax[kChunk];
  for (int c = threadIdx.x; c < 6 * g.A; c += kTPB) cell[c] = g.cell[c];
  __syncthreads();
  float b[kPerThread][6], mx[kPerThread], dmx[kPerThread];
  bool in[kPerThread], tie[kPerThread];
  unsigned int idx[kPerThread];
  int any = 0;
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    const unsigned long long i = ((unsigned long long)blockIdx.x * kPerThread + u) * kTPB + threadIdx.x;
    idx[u] = (unsigned int)i;
    in[u] = false; tie[u] = false; mx[u] = 0.f; dmx[u] = 0.f;
    if (i < g.N) {
      anchor_of(cell, g, (unsigned int)i, b[u]);
      in[u] = anchor_inside(g, b[u]);
    }
    any |= in[u];
  }
  if (__syncthreads_or(any)) {
    for (int k0 = 0; k0 < g.K; k0 += kChunk) {
      const int kc = g.K - k0 < kChunk ? g.K - k0 : kChunk;
      __syncthreads();
      load_boxes(q, gt, k0, kc);
      for (int k = threadIdx.x; k < kc; k += kTPB) smax[k] = __uint_as_float(gt_max[k0 + k]);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kPerThread; ++u) {
        if (!in[u]) continue;
        for (int k = 0; k < kc; ++k) {
          const float v = iou3d(b[u], q + 8 * k, q[8 * k + 6]);
          tie[u] = tie[u] || v == smax[k];      // rpn.py:169-175, zero maxima included
          mx[u] = v > mx[u] ? v : mx[u];        // rpn.py:155-158 (the value only; the argmax is redone for the few sampled fg)
        }
      }
    }
    for (int k0 = 0; k0 < g.Kdc; k0 += kChunk) {   // rpn.py:180-184
      const int kc = g.Kdc - k0 < kChunk ? g.Kdc - k0 : kChunk;
      __syncthreads();
      load_boxes(q, dc, k0, kc);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kPerThread; ++u) {
        if (!in[u]) continue;
        for (int k = 0; k < kc; ++k) {
          const float v = iou3d(b[u], q + 8 * k, q[8 * k + 6]);
          dmx[u] = v > dmx[u] ? v : dmx[u];
        }
      }
    }
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int u = 0; u < kPerThread; ++u) {
    const bool fg = in[u] && g.K > 0 && (tie[u] || mx[u] >= g.pos);          // rpn.py:175-177
    const bool cand = in[u] && mx[u] < g.neg && dmx[u] < g.neg;              // rpn.py:202-203
    const unsigned long long mc = __ballot(cand), mi = __ballot(in[u]), mf = __ballot(fg);
    const size_t word = (((size_t)blockIdx.x * kPerThread + u) * kTPB + threadIdx.x) / 64;
    if (lane == 0) {
      bits[word] = mc;
      if (mi) atomicAdd(&cnt[C_INSIDE], (unsigned int)__popcll(mi));
    }
    if (mf) {
      const int lead = __ffsll((long long)mf) - 1;
      unsigned int base = 0;
      if (lane == lead) base = atomicAdd(&cnt[C_FG], (unsigned int)__popcll(mf));
      base = __shfl(base, lead);
      if (fg) fglist[base + (unsigned int)__popcll(mf & ((1ull << lane) - 1ull))] = idx[u];
    }
  }
}

__global__ __launch_bounds__(kOne) void scan_kernel(const unsigned long long* __restrict__ bits, unsigned int nwords,
                                                    unsigned int* __restrict__ wordpref, unsigned int* __restrict__ cnt) {
  __shared__ unsigned int sh[kOne];
  const unsigned int per = (nwords + kOne - 1) / kOne;
  const unsigned int lo = threadIdx.x * per, hi = lo + per < nwords ? lo + per : nwords;
  unsigned int s = 0;
  for (unsigned int w = lo; w < hi; ++w) s += (unsigned int)__popcll(bits[w]);
  unsigned int total;
  unsigned int run = block_exscan(s, sh, &total);
  for (unsigned int w = lo; w < hi; ++w) {
    wordpref[w] = run;
    run += (unsigned int)__popcll(bits[w]);
  }
  if (threadIdx.x == 0) cnt[C_CAND] = total;
}

__global__ __launch_bounds__(kTPB) void draw_kernel(const unsigned long long* __restrict__ bits, const unsigned int* __restrict__ wordpref,
                                                    unsigned int nwords, const unsigned int* __restrict__ cnt, int batch, int num_fg,
                                                    unsigned long long seed, unsigned int* __restrict__ draws) {
  const int j = blockIdx.x * kTPB + threadIdx.x;
  if (j >= batch) return;
  const unsigned int fg = cnt[C_FG] < (unsigned int)num_fg ? cnt[C_FG] : (unsigned int)num_fg;
  const unsigned int num_bg = (unsigned int)batch - fg, n = cnt[C_CAND];                 // rpn.py:201
  unsigned int pick = 0xFFFFFFFFu;
  if (n > num_bg && (unsigned int)j < num_bg) {                                          // rpn.py:204-205
    const unsigned int r = (unsigned int)(((unsigned long long)mix_key(seed, (1ull << 40) + (unsigned long long)j) * n) >> 32);
    unsigned int lo = 0, hi = nwords;                  // the last word whose prefix is <= r holds candidate r (r < n)
    while (hi - lo > 1) {
      const unsigned int mid = lo + (hi - lo) / 2;
      if (wordpref[mid] <= r) lo = mid; else hi = mid;
    }
    unsigned long long m = bits[lo];
    for (unsigned int rem = r - wordpref[lo]; rem; --rem) m &= m - 1;
    pick = lo * 64u + (unsigned int)(__ffsll((long long)m) - 1);
  }
  draws[j] = pick;
}

// bbox_transform_inv_3d with unit weights (boxes_3d.py:241-264) in fp32, operation for operation; the three logs in fp64, rounded once
__device__ inline void targets_of(const float* b, const float* q, float* o) {
  float ew = b[3] - b[0]; ew = ew + 1.0f;
  float eh = b[4] - b[1]; eh = eh + 1.0f;
  float es = b[5] - b[2]; es = es + 1.0f;
  const float ex = b[0] + 0.5f * ew, ey = b[1] + 0.5f * eh, ez = b[2] + 0.5f * es;
  float gw = q[3] - q[0]; gw = gw + 1.0f;
  float gh = q[4] - q[1]; gh = gh + 1.0f;
  float gs = q[5] - q[2]; gs = gs + 1.0f;
  const float gx = q[0] + 0.5f * gw, gy = q[1] + 0.5f * gh, gz = q[2] + 0.5f * gs;
  o[0] = (gx - ex) / ew;
  o[1] = (gy - ey) / eh;
  o[2] = (gz - ez) / es;
  o[3] = (float)log((double)(gw / ew));
  o[4] = (float)log((double)(gh / eh));
  o[5] = (float)log((double)(gs / es));
}

__device__ inline bool contains_wide(const Geom& g, const unsigned int* sorted, unsigned int n, unsigned long long w) {
  unsigned int lo = 0, hi = n;
  while (lo < hi) {
    const unsigned int mid = lo + (hi - lo) / 2;
    const unsigned long long v = wide_of(g, sorted[mid]);
    if (v == w) return true;
    if (v < w) lo = mid + 1; else hi = mid;
  }
  return false;
}

__global__ __launch_bounds__(kOne) void finalize_kernel(Geom g, const float* __restrict__ gt, Ws w, int batch, int num_fg,
                                                        unsigned long long seed, int64_t* __restrict__ fg_index,
                                                        int64_t* __restrict__ bg_index, int64_t* __restrict__ target_index,
                                                        float* __restrict__ targets, int64_t* __restrict__ counts) {
  __shared__ double cell[6 * kMaxA];
  __shared__ unsigned int sh[kOne];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int s_sel, s_rem, s_cnt;
  const int t = threadIdx.x;
  for (int c = t; c < 6 * g.A; c += kOne) cell[c] = g.cell[c];
  const unsigned int M = w.cnt[C_FG], n = w.cnt[C_CAND];
  const unsigned int nt = M < (unsigned int)num_fg ? M : (unsigned int)num_fg;
  // -- the num_fg smallest (key, index) of the fg set (stands in for npr.choice without replacement, rpn.py:189-196)
  unsigned long long T = ~0ull;
  if (M > nt && nt > 0) {
    unsigned long long prefix = 0, mask = 0;
    unsigned int remaining = nt;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0u;
      __syncthreads();
      for (unsigned int e = t; e < M; e += kOne) {
        const unsigned long long c = fg_order(seed, w.fglist[e]);
        if ((c & mask) == prefix) atomicAdd(&hist[(unsigned int)(c >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (t == 0) {
        unsigned int cum = 0, b = 0;
        for (; b < 255; ++b) {
          if (cum + hist[b] >= remaining) break;
          cum += hist[b];
        }
        s_sel = b; s_rem = remaining - cum;
      }
      __syncthreads();
      prefix |= (unsigned long long)s_sel << shift;
      mask |= 0xFFull << shift;
      remaining = s_rem;
      __syncthreads();
    }
    T = prefix;   // the orders are distinct, so exactly nt of them are <= T
  }
  if (t == 0) s_cnt = 0u;
  __syncthreads();
  if (nt > 0)
    for (unsigned int e = t; e < M; e += kOne) {
      const unsigned int i = w.fglist[e];
      if (fg_order(seed, i) <= T) {
        const unsigned int p = atomicAdd(&s_cnt, 1u);
        if (p < nt) w.kept_a[p] = i;
      }
    }
  __syncthreads();
  for (unsigned int e = t; e < nt; e += kOne) {   // sort by wide index (distinct): rank = number of smaller ones
    const unsigned int i = w.kept_a[e];
    const unsigned long long wi = wide_of(g, i);
    unsigned int r = 0;
    for (unsigned int f = 0; f < nt; ++f) r += wide_of(g, w.kept_a[f]) < wi;
    w.kept_s[r] = i;
  }
  // -- the bg draws (with replacement, rpn.py:204-206): sort by (wide index, j), fold duplicates
  const unsigned int num_bg = (unsigned int)batch - nt;
  const unsigned int nd = n > num_bg ? num_bg : 0u;
  for (unsigned int e = t; e < nd; e += kOne) {
    const unsigned long long wi = wide_of(g, w.draws[e]);
    unsigned int r = 0;
    for (unsigned int f = 0; f < nd; ++f) {
      const unsigned long long wf = wide_of(g, w.draws[f]);
      r += wf < wi || (wf == wi && f < e);
    }
    w.drw_s[r] = w.draws[e];
  }
  __syncthreads();
  unsigned int n_bg, n_fg;
  {
    const unsigned int per = (nd + kOne - 1) / kOne;
    const unsigned int lo = t * per < nd ? t * per : nd, hi = lo + per < nd ? lo + per : nd;
    unsigned int c = 0;
    for (unsigned int r = lo; r < hi; ++r) c += r == 0 || w.drw_s[r] != w.drw_s[r - 1];
    unsigned int off = block_exscan(c, sh, &n_bg);
    for (unsigned int r = lo; r < hi; ++r)
      if (r == 0 || w.drw_s[r] != w.drw_s[r - 1]) w.bgu[off++] = w.drw_s[r];
  }
  __syncthreads();
  {   // a draw that hit a sampled fg anchor turns it into bg (rpn.py:206 overwrites the label)
    const unsigned int per = (nt + kOne - 1) / kOne;
    const unsigned int lo = t * per < nt ? t * per : nt, hi = lo + per < nt ? lo + per : nt;
    unsigned int c = 0;
    for (unsigned int r = lo; r < hi; ++r) c += !contains_wide(g, w.bgu, n_bg, wide_of(g, w.kept_s[r]));
    unsigned int off = block_exscan(c, sh, &n_fg);
    for (unsigned int r = lo; r < hi; ++r) {
      const unsigned long long wi = wide_of(g, w.kept_s[r]);
      if (!contains_wide(g, w.bgu, n_bg, wi)) fg_index[off++] = (int64_t)wi;
    }
  }
  for (unsigned int e = t; e < (unsigned int)num_fg; e += kOne) {
    if (e >= n_fg) fg_index[e] = -1;
    if (e >= nt) {
      target_index[e] = -1;
#pragma unroll
      for (int c = 0; c < 6; ++c) targets[6 * (size_t)e + c] = 0.f;
      continue;
    }
    // targets of the fg set as sampled, before the bg draws (rpn.py:196,209-212)
    const unsigned int i = w.kept_s[e];
    float b[6], o[6];
    anchor_of(cell, g, i, b);
    float best = -1.f;
    int arg = 0;
    for (int k = 0; k < g.K; ++k) {                   // first argmax (rpn.py:155)
      const float* qk = gt + 6 * (size_t)k;
      const float v = iou3d(b, qk, iou_query_volume(qk));
      if (v > best) { best = v; arg = k; }
    }
    targets_of(b, gt + 6 * (size_t)arg, o);
    target_index[e] = (int64_t)wide_of(g, i);
#pragma unroll
    for (int c = 0; c < 6; ++c) targets[6 * (size_t)e + c] = o[c];
  }
  for (unsigned int e = t; e < (unsigned int)batch; e += kOne) bg_index[e] = e < n_bg ? (int64_t)wide_of(g, w.bgu[e]) : -1;
  if (t == 0) {
    counts[0] = n_fg; counts[1] = n_bg; counts[2] = nt; counts[3] = (int64_t)n_fg + n_bg;   // num_examples, rpn.py:229
    counts[4] = w.cnt[C_INSIDE]; counts[5] = M; counts[6] = n; counts[7] = nd;
  }
}

__device__ inline bool contains_i64(const int64_t* sorted, int n, int64_t v, int* where) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (sorted[mid] == v) { *where = mid; return true; }
    if (sorted[mid] < v) lo = mid + 1; else hi = mid;
  }
  return false;
}

// outside weight of a labelled anchor: float32(1.0 / num_examples), one rounding (rpn.py:229-231)
__device__ inline float outside_weight(int64_t num_examples) { return (float)(1.0 / (double)num_examples); }

__device__ inline int clamp_count(int64_t v, int cap) { return (int)(v < 0 ? 0 : (v > cap ? cap : v)); }

// counts and indices are clamped: a caller's stale buffer must not scatter out of bounds
__global__ __launch_bounds__(kTPB) void wide_kernel(const int64_t* __restrict__ fg_index, const int64_t* __restrict__ bg_index,
                                                    const int64_t* __restrict__ target_index, const float* __restrict__ targets,
                                                    const int64_t* __restrict__ counts, int A, unsigned int F3, int cap, int batch,
                                                    int32_t* __restrict__ labels, float* __restrict__ tw, float* __restrict__ iw,
                                                    float* __restrict__ ow) {
  const unsigned long long total = (unsigned long long)A * F3;
  const int n_fg = clamp_count(counts[0], cap), n_bg = clamp_count(counts[1], batch), n_t = clamp_count(counts[2], cap);
  const float o = counts[3] > 0 ? outside_weight(counts[3]) : 0.f;
  const int e = blockIdx.x * kTPB + threadIdx.x;
  // channel layout of rpn.py:263-270: anchor a, component c -> channel 6 a + c
  if (e < n_t) {
    const unsigned long long wi = (unsigned long long)target_index[e];
    if (wi < total) {
      const size_t base = (size_t)(wi / F3) * 6 * F3 + (size_t)(wi % F3);
#pragma unroll
      for (int c = 0; c < 6; ++c) tw[base + (size_t)c * F3] = targets[6 * (size_t)e + c];
    }
  }
  if (e < n_fg) {
    const unsigned long long wi = (unsigned long long)fg_index[e];
    if (wi < total) {
      const size_t base = (size_t)(wi / F3) * 6 * F3 + (size_t)(wi % F3);
      labels[wi] = 1;
#pragma unroll
      for (int c = 0; c < 6; ++c) { iw[base + (size_t)c * F3] = 1.0f; ow[base + (size_t)c * F3] = o; }
    }
  }
  if (e >= cap && e - cap < n_bg) {
    const unsigned long long wi = (unsigned long long)bg_index[e - cap];
    if (wi < total) {
      const size_t base = (size_t)(wi / F3) * 6 * F3 + (size_t)(wi % F3);
      labels[wi] = 0;
#pragma unroll
      for (int c = 0; c < 6; ++c) ow[base + (size_t)c * F3] = o;
    }
  }
}

struct LossGeom { int B, A, s, h, w, F, cap_fg, cap_bg; };

// wide index -> offset of the anchor's logit in [B,A,s,h,w], or -1 outside the crop [:s,:h,:w] (rpn_heads.py:145-150)
__device__ inline long long crop_offset(const LossGeom& g, int b, int64_t wi, int* a_out, long long* sp_out) {
  const long long F3 = (long long)g.F * g.F * g.F;
  if (wi < 0 || wi >= F3 * g.A) return -1;
  const int a = (int)(wi / F3);
  const long long pos = wi % F3;
  const int x = (int)(pos % g.F), y = (int)((pos / g.F) % g.F), z = (int)(pos / ((long long)g.F * g.F));
  if (z >= g.s || y >= g.h || x >= g.w) return -1;
  const long long sp = ((long long)z * g.h + y) * g.w + x;
  *a_out = a; *sp_out = sp;
  return ((long long)b * g.A + a) * ((long long)g.s * g.h * g.w) + sp;
}

__global__ __launch_bounds__(kOne) void loss_kernel(LossGeom g, const float* __restrict__ logits, const float* __restrict__ pred,
                                                    const int64_t* __restrict__ fg_index, const int64_t* __restrict__ bg_index,
                                                    const int64_t* __restrict__ target_index, const float* __restrict__ targets,
                                                    const int64_t* __restrict__ counts, float* __restrict__ losses,
                                                    float* __restrict__ grad_logits, float* __restrict__ grad_pred) {
  __shared__ double shd[kOne];
  __shared__ unsigned int shu[kOne];
  const int t = threadIdx.x;
  const int per = g.cap_fg + g.cap_bg, total = g.B * per;
  const long long shw = (long long)g.s * g.h * g.w;
  // sum of the classification weights = labelled anchors inside the crop, over the batch (rpn_heads.py:161-164)
  unsigned int c = 0;
  for (int e = t; e < total; e += kOne) {
    const int b = e / per, r = e % per;
    const int64_t* cn = counts + 8 * (size_t)b;
    const bool is_fg = r < g.cap_fg;
    const int k = is_fg ? r : r - g.cap_fg;
    if (k >= (is_fg ? clamp_count(cn[0], g.cap_fg) : clamp_count(cn[1], g.cap_bg))) continue;
    int a; long long sp;
    c += crop_offset(g, b, is_fg ? fg_index[(size_t)b * g.cap_fg + k] : bg_index[(size_t)b * g.cap_bg + k], &a, &sp) >= 0;
  }
  const unsigned int sw = block_sum<unsigned int>(c, shu);
  const float swf = (float)sw, beta = (float)(1.0 / 9.0), half_beta = (float)(0.5 * (1.0 / 9.0)), fB = (float)g.B;
  double acc_cls = 0.0, acc_box = 0.0;
  for (int e = t; e < total; e += kOne) {
    const int b = e / per, r = e % per;
    const int64_t* cn = counts + 8 * (size_t)b;
    const bool is_fg = r < g.cap_fg;
    const int k = is_fg ? r : r - g.cap_fg;
    if (k >= (is_fg ? clamp_count(cn[0], g.cap_fg) : clamp_count(cn[1], g.cap_bg))) continue;
    const int64_t wi = is_fg ? fg_index[(size_t)b * g.cap_fg + k] : bg_index[(size_t)b * g.cap_bg + k];
    int a; long long sp;
    const long long off = crop_offset(g, b, wi, &a, &sp);
    if (off < 0) continue;
    const float x = logits[off], y = is_fg ? 1.f : 0.f;
    const float ex = expf(-fabsf(x));
    float term = (x > 0.f ? x : 0.f) - x * y;          // max(x, 0) - x y + log1p(exp(-|x|))
    term = term + log1pf(ex);
    acc_cls += (double)term;
    const float sig = x >= 0.f ? 1.0f / (1.0f + ex) : ex / (1.0f + ex);
    grad_logits[off] = (sig - y) / swf;
    if (!is_fg) continue;                              // inside weight 0: no box term off the fg anchors (rpn.py:219-220)
    int row = 0;
    if (!contains_i64(target_index + (size_t)b * g.cap_fg, clamp_count(cn[2], g.cap_fg), wi, &row)) continue;
    const float o = outside_weight(cn[3]);
#pragma unroll
    for (int d = 0; d < 6; ++d) {                      // smooth L1, beta = 1/9 (net.py:22-31)
      const long long po = ((long long)b * 6 * g.A + 6 * a + d) * shw + sp;
      const float v = pred[po] - targets[((size_t)b * g.cap_fg + row) * 6 + d];
      const float av = fabsf(v);
      float l;
      if (av < beta) { l = 0.5f * (v * v); l = l / beta; } else { l = av - half_beta; }
      acc_box += (double)(o * l);
      float cl = v / beta;
      cl = cl < -1.f ? -1.f : (cl > 1.f ? 1.f : cl);
      grad_pred[po] = (o * cl) / fB;
    }
  }
  const double s_cls = block_sum<double>(acc_cls, shd);
  const double s_box = block_sum<double>(acc_box, shd);
  if (t == 0) {
    losses[0] = sw ? (float)(s_cls / (double)sw) : 0.f;
    losses[1] = (float)(s_box / (double)g.B);
  }
}

int fill_geom(Geom& g, const double* cell, int A, int F, int stride, int K, int Kdc, double im_s, double im_h, double im_w,
              double straddle, double pos, double neg) {
  if (!cell || A < 1 || F < 1 || stride < 1 || K < 0 || Kdc < 0) return M3D_EINVAL;
  if (A > kMaxA) return M3D_EUNSUPPORTED;
  const unsigned long long N = (unsigned long long)F * F * F * A;
  if (F > 2048 || N >= (1ull << 32) - kTPB * kPerThread) return M3D_EUNSUPPORTED;   // flat indices are 32-bit on the device
  memset(&g, 0, sizeof(g));
  for (int c = 0; c < 6 * A; ++c) g.cell[c] = cell[c];
  g.t = straddle; g.im_w = im_w; g.im_h = im_h; g.im_s = im_s;
  g.pos = (float)pos; g.neg = (float)neg;
  g.A = A; g.F = F; g.stride = stride; g.K = K; g.Kdc = Kdc;
  g.N = (unsigned int)N; g.F3 = (unsigned int)((unsigned long long)F * F * F);
  return M3D_OK;
}

}  // namespace

M3D_API size_t m3d_rpn_targets_workspace_bytes(int num_cell_anchors, int field_size, int num_gt, int batch_per_im, int num_fg) {
  if (num_cell_anchors < 1 || num_cell_anchors > kMaxA || field_size < 1 || field_size > 2048 || batch_per_im < 1 || num_fg < 0 || num_gt < 0)
    return 0;
  const unsigned long long N = (unsigned long long)field_size * field_size * field_size * num_cell_anchors;
  if (N >= (1ull << 32) - kTPB * kPerThread) return 0;
  return carve(nullptr, (unsigned int)N, num_gt, num_fg, batch_per_im).bytes;
}

M3D_API int m3d_rpn_targets(const double* cell_anchors, int num_cell_anchors, int field_size, int stride, const float* d_gt, int num_gt,
                            const float* d_dc, int num_dc, double im_slices, double im_height, double im_width, double straddle_thresh,
                            double positive_overlap, double negative_overlap, int batch_per_im, int num_fg, uint64_t seed,
                            int64_t* d_fg_index, int64_t* d_bg_index, int64_t* d_target_index, float* d_targets, int64_t* d_counts,
                            void* d_ws, size_t ws_bytes, void* stream) {
  Geom g;
  const int rc = fill_geom(g, cell_anchors, num_cell_anchors, field_size, stride, num_gt, num_dc, im_slices, im_height, im_width,
                           straddle_thresh, positive_overlap, negative_overlap);
  if (rc != M3D_OK) return rc;
  if (batch_per_im < 1 || num_fg < 0 || num_fg > batch_per_im) return M3D_EINVAL;
  if (batch_per_im > kMaxBatch) return M3D_EUNSUPPORTED;
  if ((num_gt > 0 && !d_gt) || (num_dc > 0 && !d_dc) || !d_bg_index || !d_counts || !d_ws) return M3D_EINVAL;
  if (num_fg > 0 && (!d_fg_index || !d_target_index || !d_targets)) return M3D_EINVAL;
  const Ws w = carve(d_ws, g.N, num_gt, num_fg, batch_per_im);
  if (ws_bytes < w.bytes) return M3D_EWORKSPACE;
  hipStream_t st = m3d::as_stream(stream);
  const unsigned long long sampling_stream = seed_stream((unsigned long long)seed);
  (void)hipMemsetAsync(w.cnt, 0, sizeof(unsigned int) * ((size_t)C_COUNT + num_gt), st);
  const unsigned int blocks = w.nwords / (kTPB * kPerThread / 64);
  if (num_gt > 0) hipLaunchKernelGGL(gt_max_kernel, dim3(blocks), dim3(kTPB), 0, st, g, d_gt, w.gt_max);
  hipLaunchKernelGGL(label_kernel, dim3(blocks), dim3(kTPB), 0, st, g, d_gt, d_dc, w.gt_max, w.cnt, w.fglist, w.bits);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kOne), 0, st, w.bits, w.nwords, w.wordpref, w.cnt);
  hipLaunchKernelGGL(draw_kernel, dim3((batch_per_im + kTPB - 1) / kTPB), dim3(kTPB), 0, st, w.bits, w.wordpref, w.nwords, w.cnt,
                     batch_per_im, num_fg, sampling_stream, w.draws);
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(kOne), 0, st, g, d_gt, w, batch_per_im, num_fg, sampling_stream, d_fg_index,
                     d_bg_index, d_target_index, d_targets, d_counts);
  return m3d::check_launch("rpn_targets");
}

M3D_API int m3d_rpn_targets_wide(const int64_t* d_fg_index, const int64_t* d_bg_index, const int64_t* d_target_index,
                                 const float* d_targets, const int64_t* d_counts, int num_cell_anchors, int field_size, int num_fg,
                                 int batch_per_im, int32_t* d_labels, float* d_targets_wide, float* d_inside_wide, float* d_outside_wide,
                                 void* stream) {
  if (num_cell_anchors < 1 || field_size < 1 || batch_per_im < 1 || num_fg < 0 || num_fg > batch_per_im) return M3D_EINVAL;
  if (num_cell_anchors > kMaxA || field_size > 2048 || batch_per_im > kMaxBatch) return M3D_EUNSUPPORTED;
  const unsigned long long F3 = (unsigned long long)field_size * field_size * field_size;
  if (F3 * num_cell_anchors >= (1ull << 32) - kTPB * kPerThread) return M3D_EUNSUPPORTED;
  if (!d_bg_index || !d_counts || !d_labels || !d_targets_wide || !d_inside_wide || !d_outside_wide) return M3D_EINVAL;
  if (num_fg > 0 && (!d_fg_index || !d_target_index || !d_targets)) return M3D_EINVAL;
  hipStream_t st = m3d::as_stream(stream);
  const size_t n = (size_t)F3 * num_cell_anchors;
  (void)hipMemsetAsync(d_labels, 0xFF, sizeof(int32_t) * n, st);   // every byte 0xFF = int32 -1 (data_utils.unmap fill, rpn.py:234)
  (void)hipMemsetAsync(d_targets_wide, 0, sizeof(float) * 6 * n, st);
  (void)hipMemsetAsync(d_inside_wide, 0, sizeof(float) * 6 * n, st);
  (void)hipMemsetAsync(d_outside_wide, 0, sizeof(float) * 6 * n, st);
  const int items = num_fg + batch_per_im;
  hipLaunchKernelGGL(wide_kernel, dim3((items + kTPB - 1) / kTPB), dim3(kTPB), 0, st, d_fg_index, d_bg_index, d_target_index, d_targets,
                     d_counts, num_cell_anchors, (unsigned int)F3, num_fg, batch_per_im, d_labels, d_targets_wide, d_inside_wide, d_outside_wide);
  return m3d::check_launch("rpn_targets_wide");
}

M3D_API int m3d_rpn_loss(const float* d_cls_logits, const float* d_bbox_pred, int batch, int num_cell_anchors, int slices, int height,
                         int width, int field_size, const int64_t* d_fg_index, const int64_t* d_bg_index, const int64_t* d_target_index,
                         const float* d_targets, const int64_t* d_counts, int num_fg, int batch_per_im, float* d_losses,
                         float* d_grad_logits, float* d_grad_pred, void* stream) {
  if (batch < 1 || num_cell_anchors < 1 || slices < 1 || height < 1 || width < 1 || field_size < 1 || batch_per_im < 1 || num_fg < 0 ||
      num_fg > batch_per_im)
    return M3D_EINVAL;
  if (num_cell_anchors > kMaxA || field_size > 2048 || batch_per_im > kMaxBatch) return M3D_EUNSUPPORTED;
  if (slices > field_size || height > field_size || width > field_size) return M3D_EINVAL;   // the crop lies inside the field
  const unsigned long long vox = (unsigned long long)slices * height * width;
  if ((unsigned long long)batch * (num_fg + batch_per_im) > (1ull << 30) || vox * 6 * num_cell_anchors * batch >= (1ull << 40))
    return M3D_EUNSUPPORTED;
  if (!d_cls_logits || !d_bbox_pred || !d_bg_index || !d_counts || !d_losses || !d_grad_logits || !d_grad_pred) return M3D_EINVAL;
  if (num_fg > 0 && (!d_fg_index || !d_target_index || !d_targets)) return M3D_EINVAL;
  hipStream_t st = m3d::as_stream(stream);
  const size_t n = (size_t)batch * num_cell_anchors * vox;
  (void)hipMemsetAsync(d_grad_logits, 0, sizeof(float) * n, st);
  (void)hipMemsetAsync(d_grad_pred, 0, sizeof(float) * 6 * n, st);
  const LossGeom g = {batch, num_cell_anchors, slices, height, width, field_size, num_fg, batch_per_im};
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(kOne), 0, st, g, d_cls_logits, d_bbox_pred, d_fg_index, d_bg_index, d_target_index,
                     d_targets, d_counts, d_losses, d_grad_logits, d_grad_pred);
  return m3d::check_launch("rpn_loss");
}
