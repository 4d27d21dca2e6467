// Box-head training step on the device (reference: lib/modeling/generate_proposal_labels_3d.py -> lib/datasets/nuclei_dataset.py:429-547
// (add_proposals) -> lib/roi_data/fast_rcnn.py:129-248 (_sample_rois) -> lib/modeling/fast_rcnn_heads.py:50-66 (fast_rcnn_losses)):
// proposal labelling against the ground-truth boxes, seeded fg / bg sampling, regression targets, the dense blobs, and the fused
// softmax / smooth-L1 loss with its gradients.  Nothing of size rows x boxes is stored and nothing goes to the host.
//
//   label_kernel      grid rows x images.  "roidb rows" of an image: r < K its ground-truth boxes, then its proposals.  Per row the
//                     maximum overlap and the first arg-max over the non-crowd boxes (LDS chunks of 256); the assignment goes to the
//                     workspace, the fg / bg candidate sets become one ballot word per wave (bit = row, so ascending row order is free).
//   select_kernel     one workgroup per image: radix-select the smallest (key, row) of each candidate set, emit the kept rows in
//                     ascending order through a prefix sum, then labels, boxes, regression targets and counts per output slot.
//   blobs_kernel      compact targets -> the reference's [rows, 6 C] blobs.   loss_kernel: one workgroup, fp64 per-row terms, fixed tree.
#include "box_common.h"
#include "train_common.h"

namespace {
using namespace m3dbox;
using namespace m3dtrain;

constexpr int kChunk = 256;        // ground-truth boxes per LDS chunk
constexpr int kTPB = 256;          // threads per workgroup of the label pass, one row each
constexpr int kMaxBatch = 4096;    // BATCH_SIZE_PER_IM limit (shipped: 64 / 128)
constexpr int kMaxClasses = 64;    // NUM_CLASSES limit (shipped: 2)
constexpr int kMaxImages = 64;     // images per call: their box offsets and sampling streams travel as kernel arguments

struct Params {
  unsigned long long stream[kMaxImages];   // seed_stream(seed of image b)
  int gt_off[kMaxImages + 1];              // image b's boxes are d_gt[gt_off[b] .. gt_off[b + 1])
  double wlog[3];                          // BBOX_REG_WEIGHTS[3:6]: applied in fp64 to the fp64 log
  float wctr[3];                           // BBOX_REG_WEIGHTS[0:3] as fp32: NumPy multiplies the fp32 array by a weak Python scalar
  float fg, hi, lo;                        // FG_THRESH, BG_THRESH_HI, BG_THRESH_LO as fp32, for the same reason
  int B, rows, batch, fg_per_im;
  unsigned int Rp, nwords;                 // roidb rows per image padded to the workgroup size; candidate words = Rp / 64
};

struct Ws {
  int* assign;                     // [B, Rp] ground-truth row a roidb row is assigned to, -1 = none
  unsigned long long *fgbits, *bgbits;   // [B, nwords] candidate sets, bit r % 64 of word r / 64
  size_t bytes;
};

inline Ws carve(void* base, int B, unsigned int Rp) {
  Ws w;
  char* p = reinterpret_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t n) { char* q = p ? p + off : nullptr; off += m3d::align_up(n, 256); return q; };
  w.assign = reinterpret_cast<int*>(take(sizeof(int) * (size_t)B * Rp));
  w.fgbits = reinterpret_cast<unsigned long long*>(take(sizeof(unsigned long long) * (size_t)B * (Rp / 64)));
  w.bgbits = reinterpret_cast<unsigned long long*>(take(sizeof(unsigned long long) * (size_t)B * (Rp / 64)));
  w.bytes = off;
  return w;
}

__device__ inline unsigned int clamp_num(int v, int rows) { return (unsigned int)(v < 0 ? 0 : (v > rows ? rows : v)); }

// the box of roidb row r of image b: a ground-truth box, or columns 1..6 of a proposal row
__device__ inline const float* row_box(const Params& p, const float* gt, const float* rois, int b, unsigned int r, unsigned int K) {
  return r < K ? gt + 6 * ((size_t)p.gt_off[b] + r) : rois + ((size_t)b * p.rows + (r - K)) * 7 + 1;
}

__global__ __launch_bounds__(kTPB) void label_kernel(Params p, const float* __restrict__ gt, const unsigned char* __restrict__ crowd,
                                                     const float* __restrict__ rois, const int* __restrict__ num, Ws w) {
  __shared__ float q[8 * kChunk];
  const int b = blockIdx.y;
  const unsigned int K = (unsigned int)(p.gt_off[b + 1] - p.gt_off[b]);
  const unsigned int total = K + clamp_num(num[b], p.rows);
  const unsigned int r = blockIdx.x * kTPB + threadIdx.x;
  const bool live = r < total, is_gt = r < K;
  const float* gtb = gt + 6 * (size_t)p.gt_off[b];
  const unsigned char* cr = crowd ? crowd + p.gt_off[b] : nullptr;
  float box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float ov = 0.f;
  int arg = -1;
  if (live) {
    const float* s = row_box(p, gt, rois, b, r, K);
#pragma unroll
    for (int c = 0; c < 6; ++c) box[c] = s[c];
  }
  if (live && is_gt) {                                   // nuclei_dataset.py:299-303: a crowd row is -1 in every class
    const bool c = cr && cr[r];
    ov = c ? -1.f : 1.f;
    arg = c ? -1 : (int)r;                               // a crowd row has class 0 (arg-max over -1s, :538): no label, no targets
  }
  // a workgroup whose rows are all ground truth or beyond the end has no IoU to compute
  const int need = live && !is_gt;
  if (__syncthreads_or(need)) {
    for (unsigned int k0 = 0; k0 < K; k0 += kChunk) {
      const int kc = K - k0 < (unsigned int)kChunk ? (int)(K - k0) : kChunk;
      __syncthreads();
      for (int k = threadIdx.x; k < kc; k += kTPB) {     // 8 floats per box: the box, its volume, crowd flag
        const float* s = gtb + 6 * (size_t)(k0 + k);
        float* d = q + 8 * k;
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] = s[c];
        d[6] = iou_query_volume(s);
        d[7] = (cr && cr[k0 + k]) ? 1.f : 0.f;
      }
      __syncthreads();
      if (need)
        for (int k = 0; k < kc; ++k) {
          if (q[8 * k + 7] != 0.f) continue;             // nuclei_dataset.py:462: crowd boxes take no part
          const float v = iou3d(box, q + 8 * k, q[8 * k + 6]);
          if (v > ov) { ov = v; arg = (int)k0 + k; }     // first arg-max; a maximum of 0 assigns nothing (:476-479)
        }
    }
  }
  const bool fg = live && ov >= p.fg;                    // fast_rcnn.py:138
  const bool bg = live && ov < p.hi && ov >= p.lo;       // fast_rcnn.py:148-149
  const unsigned long long mf = __ballot(fg), mb = __ballot(bg);
  w.assign[(size_t)b * p.Rp + r] = arg;
  if ((threadIdx.x & 63) == 0) {
    w.fgbits[(size_t)b * p.nwords + r / 64] = mf;
    w.bgbits[(size_t)b * p.nwords + r / 64] = mb;
  }
}

__device__ inline unsigned long long order_of(unsigned long long stream, unsigned long long base, unsigned int r) {
  return ((unsigned long long)mix_key(stream, base + r) << 32) | r;
}

// Of the M candidates in `bits`, keep the `want` <= M with the smallest (key(base + row), row) and write their rows, ascending, to
// out[0 .. want).  Stands in for npr.choice without replacement (fast_rcnn.py:144-145, 156-157).  Every thread of the workgroup calls it.
__device__ void select_rows(const unsigned long long* __restrict__ bits, unsigned int nwords, unsigned int M, unsigned int want,
                            unsigned long long stream, unsigned long long base, int64_t* out, unsigned int* sh,
                            unsigned int* hist, unsigned int* s_pair) {
  const int t = threadIdx.x;
  if (want == 0) return;
  unsigned long long T = ~0ull;
  if (M > want) {
    unsigned long long prefix = 0, mask = 0;
    unsigned int remaining = want;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0u;
      __syncthreads();
      for (unsigned int wd = t; wd < nwords; wd += kOne)
        for (unsigned long long m = bits[wd]; m; m &= m - 1) {
          const unsigned long long c = order_of(stream, base, wd * 64u + (unsigned int)(__ffsll((long long)m) - 1));
          if ((c & mask) == prefix) atomicAdd(&hist[(unsigned int)(c >> shift) & 255u], 1u);
        }
      __syncthreads();
      if (t == 0) {
        unsigned int cum = 0, d = 0;
        for (; d < 255; ++d) {
          if (cum + hist[d] >= remaining) break;
          cum += hist[d];
        }
        s_pair[0] = d; s_pair[1] = remaining - cum;
      }
      __syncthreads();
      prefix |= (unsigned long long)s_pair[0] << shift;
      mask |= 0xFFull << shift;
      remaining = s_pair[1];
      __syncthreads();
    }
    T = prefix;   // the orders are distinct, so exactly `want` of them are <= T
  }
  // consecutive words per thread, so that the prefix sum hands out the output slots in ascending row order
  const unsigned int per = (nwords + kOne - 1) / kOne;
  const unsigned int lo = (unsigned int)t * per < nwords ? (unsigned int)t * per : nwords, hi = lo + per < nwords ? lo + per : nwords;
  unsigned int c = 0;
  for (unsigned int wd = lo; wd < hi; ++wd)
    for (unsigned long long m = bits[wd]; m; m &= m - 1)
      c += order_of(stream, base, wd * 64u + (unsigned int)(__ffsll((long long)m) - 1)) <= T;
  unsigned int kept;
  unsigned int off = block_exscan(c, sh, &kept);
  for (unsigned int wd = lo; wd < hi; ++wd)
    for (unsigned long long m = bits[wd]; m; m &= m - 1) {
      const unsigned int r = wd * 64u + (unsigned int)(__ffsll((long long)m) - 1);
      if (order_of(stream, base, r) <= T && off < want) out[off++] = (int64_t)r;
    }
  __syncthreads();
}

// bbox_transform_inv_3d (boxes_3d.py:241-264) on fp32 boxes: dx,dy,dz in fp32 in the reference's order (w * (g - e)) / size; dw,dh,ds =
// fp32(w * log in fp64 of the fp32 ratio), one rounding (the reference's fp32 log and fp32 product lie within 4 ulp of it)
__device__ inline void targets_of(const Params& p, const float* b, const float* g, float* o) {
  float e[3], s[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    e[d] = b[3 + d] - b[d]; e[d] = e[d] + 1.0f;
    s[d] = g[3 + d] - g[d]; s[d] = s[d] + 1.0f;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float ec = b[d] + 0.5f * e[d], gc = g[d] + 0.5f * s[d];
    float v = gc - ec; v = p.wctr[d] * v;
    o[d] = v / e[d];
    o[3 + d] = (float)(p.wlog[d] * log((double)(s[d] / e[d])));
  }
}

__global__ __launch_bounds__(kOne) void select_kernel(Params p, const float* __restrict__ gt, const int* __restrict__ gt_classes,
                                                      const unsigned char* __restrict__ crowd, const float* __restrict__ rois,
                                                      const int* __restrict__ num, Ws w, int64_t* __restrict__ out_rows,
                                                      int* __restrict__ out_labels, float* __restrict__ out_rois,
                                                      float* __restrict__ out_targets, int64_t* __restrict__ out_counts) {
  __shared__ unsigned int sh[kOne];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int s_pair[2];
  const int t = threadIdx.x, b = blockIdx.x;
  const unsigned int K = (unsigned int)(p.gt_off[b + 1] - p.gt_off[b]);
  const unsigned long long* fgb = w.fgbits + (size_t)b * p.nwords;
  const unsigned long long* bgb = w.bgbits + (size_t)b * p.nwords;
  unsigned int cf = 0, cb = 0, cc = 0;
  for (unsigned int wd = t; wd < p.nwords; wd += kOne) { cf += (unsigned int)__popcll(fgb[wd]); cb += (unsigned int)__popcll(bgb[wd]); }
  if (crowd)
    for (unsigned int k = t; k < K; k += kOne) cc += crowd[p.gt_off[b] + k] != 0;
  const unsigned int Mf = block_sum<unsigned int>(cf, sh), Mb = block_sum<unsigned int>(cb, sh), Kc = block_sum<unsigned int>(cc, sh);
  const unsigned int nf = Mf < (unsigned int)p.fg_per_im ? Mf : (unsigned int)p.fg_per_im;            // fast_rcnn.py:141
  const unsigned int nb = Mb < (unsigned int)p.batch - nf ? Mb : (unsigned int)p.batch - nf;           // fast_rcnn.py:152-153
  int64_t* rows = out_rows + (size_t)b * p.batch;
  select_rows(fgb, p.nwords, Mf, nf, p.stream[b], 0ull, rows, sh, hist, s_pair);
  select_rows(bgb, p.nwords, Mb, nb, p.stream[b], 1ull << 40, rows + nf, sh, hist, s_pair);
  const unsigned int n = nf + nb;
  for (unsigned int e = t; e < (unsigned int)p.batch; e += kOne) {
    const size_t o = (size_t)b * p.batch + e;
    float box[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, tg[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int label = -1;
    if (e < n) {
      const unsigned int r = (unsigned int)rows[e];
      const float* s = row_box(p, gt, rois, b, r, K);
#pragma unroll
      for (int c = 0; c < 6; ++c) box[c] = s[c];
      label = 0;                                          // fast_rcnn.py:163
      const int a = w.assign[(size_t)b * p.Rp + r];
      if (e < nf && a >= 0) {                             // max_classes of the row (nuclei_dataset.py:538): 0 without an assignment
        label = gt_classes ? gt_classes[p.gt_off[b] + a] : 1;
        label = label < 0 ? 0 : label;
        if (label > 0) targets_of(p, box, gt + 6 * ((size_t)p.gt_off[b] + a), tg);   // _expand_bbox_targets keeps classes > 0 only
      }
    } else {
      rows[e] = -1;
    }
    out_labels[o] = label;
#pragma unroll
    for (int c = 0; c < 6; ++c) { out_rois[6 * o + c] = box[c]; out_targets[6 * o + c] = tg[c]; }
  }
  if (t == 0) {
    int64_t* c = out_counts + 8 * (size_t)b;
    c[0] = n; c[1] = nf; c[2] = nb; c[3] = Mf; c[4] = Mb; c[5] = Kc; c[6] = (int64_t)K - Kc; c[7] = clamp_num(num[b], p.rows);
  }
}

// _expand_bbox_targets (fast_rcnn.py:222-248) and the outside weights of :177-178: one thread per blob element
__global__ __launch_bounds__(kTPB) void blobs_kernel(const int* __restrict__ labels, const float* __restrict__ targets, long long n_rows,
                                                     int C, float* __restrict__ bt, float* __restrict__ iw, float* __restrict__ ow) {
  const long long i = (long long)blockIdx.x * kTPB + threadIdx.x;
  if (i >= n_rows * 6 * C) return;
  const long long row = i / (6 * C);
  const int slot = (int)(i % (6 * C));
  const int label = labels[row];
  const bool on = label > 0 && label < C && slot / 6 == label;
  bt[i] = on ? targets[6 * row + slot % 6] : 0.f;
  iw[i] = on ? 1.f : 0.f;
  ow[i] = on ? 1.f : 0.f;
}

// fast_rcnn_losses (fast_rcnn_heads.py:50-66) with smooth L1, beta = 1 (net.py:15-32), over the rows the counts name.  Every row's
// terms are evaluated in fp64 from the fp32 inputs and summed in fp64 in a fixed tree; each result is rounded to fp32 once.
__global__ __launch_bounds__(kOne) void loss_kernel(const float* __restrict__ score, const float* __restrict__ pred,
                                                    const int* __restrict__ labels, const float* __restrict__ targets,
                                                    const int64_t* __restrict__ counts, int B, int batch, int C,
                                                    float* __restrict__ losses, float* __restrict__ g_score, float* __restrict__ g_pred) {
  __shared__ double shd[kOne];
  __shared__ unsigned int shu[kOne];
  const int t = threadIdx.x;
  unsigned int cr = 0;
  for (int b = t; b < B; b += kOne) {
    const int64_t c = counts[8 * (size_t)b];
    cr += (unsigned int)(c < 0 ? 0 : (c > batch ? batch : c));
  }
  const unsigned int R = block_sum<unsigned int>(cr, shu);
  const double dR = (double)R;
  double a_cls = 0.0, a_box = 0.0;
  unsigned int a_hit = 0;
  const long long total = (long long)B * batch;
  for (long long row = t; row < total; row += kOne) {
    const int64_t c = counts[8 * (size_t)(row / batch)];
    const int label = labels[row];
    if (row % batch >= c || label < 0 || label >= C) continue;      // padding (and, defensively, a label the blobs cannot hold)
    const float* s = score + (size_t)row * C;
    float mx = s[0];
    int arg = 0;
    for (int k = 1; k < C; ++k)
      if (s[k] > mx) { mx = s[k]; arg = k; }                        // first arg-max (fast_rcnn_heads.py:63)
    double sum = 0.0;
    for (int k = 0; k < C; ++k) sum += exp((double)s[k] - (double)mx);
    const double lse = (double)mx + log(sum);
    a_cls += lse - (double)s[label];
    a_hit += arg == label;
    for (int k = 0; k < C; ++k)
      g_score[(size_t)row * C + k] = (float)((exp((double)s[k] - lse) - (k == label ? 1.0 : 0.0)) / dR);
    if (label == 0) continue;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const size_t po = (size_t)row * 6 * C + 6 * label + j;
      const double d = (double)pred[po] - (double)targets[6 * (size_t)row + j];
      const double ad = fabs(d);
      a_box += ad < 1.0 ? 0.5 * d * d : ad - 0.5;
      g_pred[po] = (float)((d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d)) / dR);
    }
  }
  const double s_cls = block_sum<double>(a_cls, shd);
  const double s_box = block_sum<double>(a_box, shd);
  const unsigned int hits = block_sum<unsigned int>(a_hit, shu);
  if (t == 0) {
    losses[0] = R ? (float)(s_cls / dR) : 0.f;
    losses[1] = R ? (float)(s_box / dR) : 0.f;
    losses[2] = R ? (float)((double)hits / dR) : 0.f;
  }
}

int check_shape(int num_images, long long max_gt, int rows, unsigned int* Rp) {
  if (num_images < 1 || max_gt < 0 || rows < 0) return M3D_EINVAL;
  if (num_images > kMaxImages) return M3D_EUNSUPPORTED;
  if (max_gt + rows >= (1ll << 31) - kTPB) return M3D_EUNSUPPORTED;   // roidb rows are 32-bit on the device
  const long long n = max_gt + rows;
  *Rp = (unsigned int)((n > 0 ? n : 1) + kTPB - 1) / kTPB * kTPB;
  return M3D_OK;
}

}  // namespace

M3D_API size_t m3d_box_head_targets_workspace_bytes(int num_images, int max_gt, int rows) {
  unsigned int Rp;
  if (check_shape(num_images, max_gt, rows, &Rp) != M3D_OK) return 0;
  return carve(nullptr, num_images, Rp).bytes;
}

M3D_API int m3d_box_head_targets(const float* d_gt, const int32_t* d_gt_classes, const uint8_t* d_gt_crowd, const int32_t* gt_offsets,
                                 int num_images, const float* d_rois, const int32_t* d_num, int rows, int batch_per_im, int fg_per_im,
                                 double fg_thresh, double bg_thresh_hi, double bg_thresh_lo, const double* bbox_reg_weights,
                                 int num_classes, int cls_agnostic_bbox_reg, const uint64_t* seeds, int64_t* d_rows, int32_t* d_labels,
                                 float* d_out_rois, float* d_targets, int64_t* d_counts, void* d_ws, size_t ws_bytes, void* stream) {
  if (!gt_offsets || !seeds || !bbox_reg_weights || num_images < 1 || rows < 0 || batch_per_im < 1 || fg_per_im < 0 ||
      fg_per_im > batch_per_im || num_classes < 2)
    return M3D_EINVAL;
  if (cls_agnostic_bbox_reg || num_classes > kMaxClasses || batch_per_im > kMaxBatch || num_images > kMaxImages) return M3D_EUNSUPPORTED;
  long long max_gt = 0;
  if (gt_offsets[0] != 0) return M3D_EINVAL;
  for (int b = 0; b < num_images; ++b) {
    const long long k = (long long)gt_offsets[b + 1] - gt_offsets[b];
    if (k < 0) return M3D_EINVAL;
    max_gt = k > max_gt ? k : max_gt;
  }
  unsigned int Rp;
  const int rc = check_shape(num_images, max_gt, rows, &Rp);
  if (rc != M3D_OK) return rc;
  if ((gt_offsets[num_images] > 0 && !d_gt) || (rows > 0 && !d_rois) || !d_num || !d_rows || !d_labels || !d_out_rois || !d_targets ||
      !d_counts || !d_ws)
    return M3D_EINVAL;
  const Ws w = carve(d_ws, num_images, Rp);
  if (ws_bytes < w.bytes) return M3D_EWORKSPACE;
  Params p;
  memset(&p, 0, sizeof(p));
  for (int b = 0; b < num_images; ++b) p.stream[b] = seed_stream((unsigned long long)seeds[b]);
  for (int b = 0; b <= num_images; ++b) p.gt_off[b] = gt_offsets[b];
  for (int d = 0; d < 3; ++d) { p.wctr[d] = (float)bbox_reg_weights[d]; p.wlog[d] = bbox_reg_weights[3 + d]; }
  p.fg = (float)fg_thresh; p.hi = (float)bg_thresh_hi; p.lo = (float)bg_thresh_lo;
  p.B = num_images; p.rows = rows; p.batch = batch_per_im; p.fg_per_im = fg_per_im;
  p.Rp = Rp; p.nwords = Rp / 64;
  hipStream_t st = m3d::as_stream(stream);
  hipLaunchKernelGGL(label_kernel, dim3(Rp / kTPB, num_images), dim3(kTPB), 0, st, p, d_gt, d_gt_crowd, d_rois, d_num, w);
  hipLaunchKernelGGL(select_kernel, dim3(num_images), dim3(kOne), 0, st, p, d_gt, d_gt_classes, d_gt_crowd, d_rois, d_num, w, d_rows,
                     d_labels, d_out_rois, d_targets, d_counts);
  return m3d::check_launch("box_head_targets");
}

M3D_API int m3d_box_head_target_blobs(const int32_t* d_labels, const float* d_targets, int64_t num_rows, int num_classes,
                                      float* d_bbox_targets, float* d_inside_weights, float* d_outside_weights, void* stream) {
  if (num_rows < 0 || num_classes < 2) return M3D_EINVAL;
  if (num_classes > kMaxClasses || num_rows > (1ll << 31) / (6 * kMaxClasses)) return M3D_EUNSUPPORTED;
  if (num_rows == 0) return M3D_OK;
  if (!d_labels || !d_targets || !d_bbox_targets || !d_inside_weights || !d_outside_weights) return M3D_EINVAL;
  const long long n = (long long)num_rows * 6 * num_classes;
  hipLaunchKernelGGL(blobs_kernel, dim3((unsigned int)((n + kTPB - 1) / kTPB)), dim3(kTPB), 0, m3d::as_stream(stream), d_labels,
                     d_targets, (long long)num_rows, num_classes, d_bbox_targets, d_inside_weights, d_outside_weights);
  return m3d::check_launch("box_head_target_blobs");
}

M3D_API int m3d_box_head_loss(const float* d_cls_score, const float* d_bbox_pred, const int32_t* d_labels, const float* d_targets,
                              const int64_t* d_counts, int num_images, int batch_per_im, int num_classes, float* d_losses,
                              float* d_grad_score, float* d_grad_pred, void* stream) {
  if (num_images < 1 || batch_per_im < 1 || num_classes < 2) return M3D_EINVAL;
  if (num_classes > kMaxClasses || batch_per_im > kMaxBatch || num_images > kMaxImages) return M3D_EUNSUPPORTED;
  if (!d_cls_score || !d_bbox_pred || !d_labels || !d_targets || !d_counts || !d_losses || !d_grad_score || !d_grad_pred) return M3D_EINVAL;
  hipStream_t st = m3d::as_stream(stream);
  const size_t n = (size_t)num_images * batch_per_im * num_classes;
  (void)hipMemsetAsync(d_grad_score, 0, sizeof(float) * n, st);
  (void)hipMemsetAsync(d_grad_pred, 0, sizeof(float) * 6 * n, st);
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(kOne), 0, st, d_cls_score, d_bbox_pred, d_labels, d_targets, d_counts, num_images,
                     batch_per_im, num_classes, d_losses, d_grad_score, d_grad_pred);
  return m3d::check_launch("box_head_loss");
}
