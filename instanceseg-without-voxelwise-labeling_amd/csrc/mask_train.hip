// Mask-branch training step on the device (reference: lib/roi_data/mask_rcnn.py:34-135 (add_mask_rcnn_blobs) -> lib/utils/segms.py:120-193
// (spot_to_mask_wrt_box, rle_to_mask_wrt_box), :209-225 (spots_to_boxes) -> lib/modeling/mask_rcnn_heads.py:90-99 (mask_rcnn_losses)):
// per sampled fg RoI the ground-truth object with the largest box overlap, its M^3 binary target, and the sigmoid cross entropy over the
// labelled target voxels with its gradient.  The reference fills an int(s) x int(h) x int(w) volume on the host, resizes it with
// skimage.transform.resize(anti_aliasing=True) and thresholds at 0.  Every term of that resize is a product of non-negative weights and
// 0/1 voxels, so - with the resize carried out in fp64 - "resize > 0" at output (i, j, k) is "some voxel is set inside F_s(i) x F_h(j) x
// F_w(k)", F_n(i) = the source indices whose weight at output i is not 0: an interval [lo, hi] per axis and output index.  The
// reference's fp32 resize underflows where a corner weight near 2e-15 meets the Gaussian tails of other axes (extents 18, 34, 58, ...):
// there this file sets voxels the reference leaves 0, never the reverse (DESIGN, "Mask-branch training targets").
//
//   targets_kernel   one workgroup per (fg slot, image).  First arg-max of the IoU over the image's objects with class > 0 that are not
//                    crowd; the interval ends of the three axes in fp64; then
//                      spot: per axis and output index the smallest fp32 (t - c)^2 over the interval (reached at an end or next to c,
//                            as the fp32 expression is monotone in |t - c|), and the voxel is (dz_i + dy_j) + dx_k < r^2;
//                      mask: slab by slab of the copied region an "any" along x into one bit per output column (LDS word per row), along
//                            y into one word per output row, along z into the M x M result words.  Every label is read once.
//   loss: partial_kernel (fp64 terms and a count per chunk of 4096 elements, fixed tree) -> finish_kernel (the partials in ascending order,
//         W and the loss, each rounded once) -> grad_kernel (the whole gradient).  No floating-point atomics.
#include "box_common.h"
#include "train_common.h"

namespace {
using namespace m3dbox;
using namespace m3dtrain;

constexpr int kMaxImages = 64;     // images per call: their descriptors travel as kernel arguments
constexpr int kMaxRes = 32;        // MRCNN.RESOLUTION limit: one output row is one 32-bit word (shipped: 14)
constexpr int kMaxClasses = 64;
constexpr int kMaxFg = 4096;       // fg rows per image
constexpr int kMaxGt = 2048;       // objects per image
constexpr int kMaxExtent = 1024;   // RoI extents are clamped to [2, 1024] before any size is derived from them
constexpr int kLossTPB = 256;
constexpr int kLossChunk = 4096;   // elements per workgroup of the loss passes: a function of the element count only

struct Image {
  const void* labels;              // mask mode: the label volume [depth, height, width] in tile coordinates
  int dtype, depth, height, width; // 0 = uint16, 1 = int32
};

struct Params {
  Image img[kMaxImages];
  int gt_off[kMaxImages + 1];
  float top[3];                    // spot mode: IN_SIZE - 1 along x, y, z
  int B, batch, fg_per_im, M, num_classes, cls_specific, mode;
};

__device__ inline int mirror(int j, int n) {      // scipy.ndimage 'mirror': period 2 (n - 1), n >= 2
  const int p = 2 * (n - 1);
  int m = j % p;
  m = m < 0 ? m + p : m;
  return m > n - 1 ? p - m : m;
}

// [lo, hi] = the source indices of an axis of length n whose unit impulse gives resize > 0 at output index i of M: the Gaussian of
// sigma = max(0, (n / M - 1) / 2) with radius int(4 sigma + 0.5) (no filter for sigma <= 1e-15) around the order-1 corners of the fp64
// coordinate n / M (i + 0.5) - 0.5, the upper corner only where its weight is not exactly 0; mirror boundary.
__device__ inline void footprint(int n, int M, int i, int* lo, int* hi) {
  const double fac = (double)n / (double)M;
  double sigma = (fac - 1.0) / 2.0;
  sigma = sigma > 0.0 ? sigma : 0.0;
  const int lw = sigma > 1e-15 ? (int)(4.0 * sigma + 0.5) : 0;
  double c = fac * ((double)i + 0.5);
  c = c - 0.5;
  if (c < 0.0) c = -c;
  if (c > (double)(n - 1)) c = (double)(2 * n - 2) - c;
  const int c0 = (int)floor(c);
  const int top = (c - (double)c0) != 0.0 ? c0 + 1 : c0;
  int a = n - 1, b = 0;
  for (int j = c0 - lw; j <= top + lw; ++j) {
    const int m = mirror(j, n);
    a = m < a ? m : a;
    b = m > b ? m : b;
  }
  *lo = a; *hi = b;
}

__device__ inline int extent_of(float e) {        // max(e, 2) of segms.py:130-132 / :164-166, int(), clamped; NaN -> 2
  e = e >= 2.f ? e : 2.f;
  e = e > (float)kMaxExtent ? (float)kMaxExtent : e;
  return (int)e;
}
__device__ inline int trunc_coord(float v) {      // astype(int): towards zero; clamped so that differences stay in range; NaN -> 0
  v = v > -536870912.f ? v : -536870912.f;
  v = v < 536870912.f ? v : 536870912.f;
  return v == v ? (int)v : 0;
}

// spots_to_boxes (segms.py:209-225) of one fp32 spot (x, y, z, r): Python's max(0, v) / min(top, v) keep 0 / top unless v is strictly beyond
__device__ inline void spot_box(const float* s, const float* top, float* o) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float lo = s[a] - s[3]; lo = lo + 1.0f;
    float hi = s[a] + s[3]; hi = hi - 1.0f;
    o[a] = lo > 0.f ? lo : 0.f;
    o[3 + a] = hi < top[a] ? hi : top[a];
  }
}

__device__ inline unsigned long long block_max64(unsigned long long v, unsigned long long* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = kOne / 2; off > 0; off >>= 1) {
    if (t < off) sh[t] = sh[t] > sh[t + off] ? sh[t] : sh[t + off];
    __syncthreads();
  }
  const unsigned long long r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kOne) void targets_kernel(Params p, const int* __restrict__ labels, const float* __restrict__ rois,
                                                       const int64_t* __restrict__ counts, const int* __restrict__ gt_classes,
                                                       const unsigned char* __restrict__ crowd, const float* __restrict__ spots,
                                                       const float* __restrict__ gt, const int* __restrict__ markers,
                                                       int* __restrict__ out_masks, float* __restrict__ out_rois,
                                                       int* __restrict__ out_assign, unsigned long long* __restrict__ out_counts) {
  __shared__ unsigned long long sh64[kOne];
  __shared__ unsigned int shu[kOne];
  __shared__ unsigned int colmask[kMaxExtent], rowmask[kMaxExtent], slabmask[kMaxExtent], rowbits[kMaxExtent];
  __shared__ unsigned int wj[kMaxRes], acc[kMaxRes * kMaxRes];
  __shared__ int lo[3][kMaxRes], hi[3][kMaxRes];
  __shared__ float dmin[3][kMaxRes];
  const int t = threadIdx.x, e = blockIdx.x, b = blockIdx.y;
  const int M = p.M, M3 = M * M * M;
  const int Cm = p.cls_specific ? p.num_classes : 1;
  const int cap = p.fg_per_im < p.batch ? p.fg_per_im : p.batch;
  int64_t nf64 = counts[8 * (size_t)b + 1];
  nf64 = nf64 < 0 ? 0 : (nf64 > cap ? cap : nf64);
  const int nf = (int)nf64;
  const size_t slot = (size_t)b * p.fg_per_im + e;
  int* om = out_masks + slot * (size_t)Cm * M3;
  if (e == 0 && t == 0) atomicAdd(out_counts + 4 * (size_t)b, (unsigned long long)nf);
  if (e >= nf) {                                          // a padding row: -1 / 0 / -1
    for (int v = t; v < Cm * M3; v += kOne) om[v] = -1;
    if (t < 6) out_rois[6 * slot + t] = 0.f;
    if (t == 0) out_assign[slot] = -1;
    return;
  }
  const size_t row = (size_t)b * p.batch + e;
  float box[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) box[c] = rois[6 * row + c];
  const int g0 = p.gt_off[b];
  int K = p.gt_off[b + 1] - g0;
  K = K > kMaxGt ? kMaxGt : K;

  // ---- mask_rcnn.py:41-70: the first arg-max of the IoU over the objects with class > 0 that are not crowd
  unsigned long long best = 0ull;
  for (int k = t; k < K; k += kOne) {
    if ((gt_classes && gt_classes[g0 + k] <= 0) || (crowd && crowd[g0 + k])) continue;
    float q[6];
    if (p.mode == 0) {
      spot_box(spots + 4 * (size_t)(g0 + k), p.top, q);
    } else {
#pragma unroll
      for (int c = 0; c < 6; ++c) q[c] = gt[6 * (size_t)(g0 + k) + c];
    }
    const float v = iou3d(box, q, iou_query_volume(q));
    const unsigned long long key = ((unsigned long long)score_bits(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)k);
    best = key > best ? key : best;
  }
  best = block_max64(best, sh64);
  const int obj = best ? (int)(0xFFFFFFFFu - (unsigned int)(best & 0xFFFFFFFFull)) : -1;   // no such object: an empty target

  // ---- extents and origin of the RoI, footprint intervals of the three axes (0 = z, 1 = y, 2 = x)
  int ext[3], org[3] = {0, 0, 0};
  if (p.mode == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) ext[a] = extent_of(box[5 - a] - box[2 - a]);               // segms.py:126-132
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      org[a] = trunc_coord(box[2 - a]);
      int d = trunc_coord(box[5 - a]) - org[a];                                            // segms.py:158-166
      d = d < 2 ? 2 : (d > kMaxExtent ? kMaxExtent : d);
      ext[a] = d;
    }
  }
  if (t < 3 * M) footprint(ext[t / M], M, t % M, &lo[t / M][t % M], &hi[t / M][t % M]);
  for (int v = t; v < kMaxRes * kMaxRes; v += kOne) acc[v] = 0u;
  __syncthreads();

  if (p.mode == 0 && obj >= 0) {
    // ---- segms.py:135-146 without the volume: centre = sp - lo in fp32, voxel (i, j, k) is set iff some integer point of the footprint
    // box has ((i - z)^2 + (j - y)^2) + (k - x)^2 < r^2 in fp32; the left side is smallest at the per-axis nearest integers
    const float* s = spots + 4 * (size_t)(g0 + obj);
    if (t < 3 * M) {
      const int a = t / M, q = t % M;
      const float c = s[2 - a] - box[2 - a];
      const float flo = (float)lo[a][q], fhi = (float)hi[a][q], fl = floorf(c);
      float d = flo - c;
      float m = d * d;
      d = fhi - c; d = d * d; m = d < m ? d : m;
      if (fl >= flo && fl <= fhi) { d = fl - c; d = d * d; m = d < m ? d : m; }
      const float fu = fl + 1.0f;
      if (fu >= flo && fu <= fhi) { d = fu - c; d = d * d; m = d < m ? d : m; }
      dmin[a][q] = m;
    }
    __syncthreads();
    const float r2 = s[3] * s[3];
    if (t < M * M) {
      const int i = t / M, j = t % M;
      const float zy = dmin[0][i] + dmin[1][j];
      unsigned int w = 0u;
      for (int k = 0; k < M; ++k) w |= ((zy + dmin[2][k]) < r2 ? 1u : 0u) << k;
      acc[i * kMaxRes + j] = w;
    }
  } else if (p.mode == 1 && obj >= 0) {
    // ---- segms.py:158-189: both boxes truncated, the copied region [max(lo), min(hi)) per axis, cut to the RoI's extent and the volume
    const Image im = p.img[b];
    const int dims[3] = {im.depth, im.height, im.width};
    const float* gb = gt + 6 * (size_t)(g0 + obj);
    const int marker = markers[g0 + obj];
    int r1[3], r2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int glo = trunc_coord(gb[2 - a]), ghi = trunc_coord(gb[5 - a]), rhi = trunc_coord(box[5 - a]);
      int u = org[a] > glo ? org[a] : glo;
      u = u > 0 ? u : 0;
      int v = rhi < ghi ? rhi : ghi;
      v = v < org[a] + ext[a] ? v : org[a] + ext[a];
      v = v < dims[a] ? v : dims[a];
      r1[a] = u; r2[a] = v > u ? v : u;
    }
    // per source index the output indices whose footprint holds it
    for (int v = t; v < kMaxExtent; v += kOne) {
      unsigned int mz = 0u, my = 0u, mx = 0u;
      for (int q = 0; q < M; ++q) {
        mz |= (v >= lo[0][q] && v <= hi[0][q] ? 1u : 0u) << q;
        my |= (v >= lo[1][q] && v <= hi[1][q] ? 1u : 0u) << q;
        mx |= (v >= lo[2][q] && v <= hi[2][q] ? 1u : 0u) << q;
      }
      slabmask[v] = v < ext[0] ? mz : 0u;
      rowmask[v] = v < ext[1] ? my : 0u;
      colmask[v] = v < ext[2] ? mx : 0u;
      rowbits[v] = 0u;
    }
    if (t < kMaxRes) wj[t] = 0u;
    __syncthreads();
    const int ny = r2[1] - r1[1], nx = r2[2] - r1[2];
    const int y0 = r1[1] - org[1], x0 = r1[2] - org[2];     // region start in RoI coordinates: 0 <= y0, y0 + ny <= ext[1] <= 1024
    const long long plane = (long long)ny * nx;
    if (plane > 0)
      for (int z = r1[0]; z < r2[0]; ++z) {
        const unsigned int zm = slabmask[z - org[0]];
        const size_t zbase = (size_t)z * im.height;
        for (long long idx = t; idx < plane; idx += kOne) {                                 // along x: one bit per output column
          const int y = (int)(idx / nx), x = (int)(idx % nx);
          const size_t at = (zbase + (size_t)(r1[1] + y)) * im.width + (size_t)(r1[2] + x);
          const int v = im.dtype == 0 ? (int)reinterpret_cast<const unsigned short*>(im.labels)[at]
                                      : reinterpret_cast<const int*>(im.labels)[at];
          if (v == marker) atomicOr(&rowbits[y0 + y], colmask[x0 + x]);
        }
        __syncthreads();
        for (int y = t; y < ny; y += kOne) {                                                // along y: one word per output row
          const unsigned int w = rowbits[y0 + y];
          rowbits[y0 + y] = 0u;
          if (w)
            for (unsigned int m = rowmask[y0 + y]; m; m &= m - 1) atomicOr(&wj[__ffs((int)m) - 1], w);
        }
        __syncthreads();
        if (t < M * M && ((zm >> (t / M)) & 1u)) acc[(t / M) * kMaxRes + t % M] |= wj[t % M];   // along z
        __syncthreads();
        if (t < kMaxRes) wj[t] = 0u;
        __syncthreads();
      }
  }
  __syncthreads();

  // ---- the row's blob (mask_rcnn.py:84-85, 115-135): z-major M^3, with cls_specific every slot outside the row's class block is -1
  const int label = labels[row];
  const int block = p.cls_specific ? (label > 0 && label < p.num_classes ? label : -1) : 0;
  unsigned int pos = 0u, lab = 0u;
  for (int v = t; v < Cm * M3; v += kOne) {
    int val = -1;
    if (v / M3 == block) {
      const int u = v % M3;
      val = (int)((acc[(u / (M * M)) * kMaxRes + (u / M) % M] >> (u % M)) & 1u);
      pos += (unsigned int)val;
      lab += 1u;
    }
    om[v] = val;
  }
  if (t < 6) out_rois[6 * slot + t] = box[t];
  if (t == 0) out_assign[slot] = obj;
  const unsigned int npos = block_sum<unsigned int>(pos, shu), nlab = block_sum<unsigned int>(lab, shu);
  if (t == 0) {
    atomicAdd(out_counts + 4 * (size_t)b + 1, (unsigned long long)npos);
    atomicAdd(out_counts + 4 * (size_t)b + 2, (unsigned long long)nlab);
  }
}

// ---------------------------------------------------------------- mask_rcnn_losses (mask_rcnn_heads.py:90-99)
struct LossWs {
  double* psum;                    // [chunks] fp64 sum of the chunk's terms
  unsigned long long* pcnt;        // [chunks] labelled elements of the chunk
  double* scale;                   // [1] weight / W, 0 for W = 0
  size_t bytes;
};
inline LossWs carve_loss(void* base, long long chunks) {
  LossWs w;
  char* p = reinterpret_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t n) { char* q = p ? p + off : nullptr; off += m3d::align_up(n, 256); return q; };
  w.psum = reinterpret_cast<double*>(take(sizeof(double) * (size_t)chunks));
  w.pcnt = reinterpret_cast<unsigned long long*>(take(sizeof(unsigned long long) * (size_t)chunks));
  w.scale = reinterpret_cast<double*>(take(sizeof(double)));
  w.bytes = off;
  return w;
}

__global__ __launch_bounds__(kLossTPB) void partial_kernel(const float* __restrict__ x, const int* __restrict__ tg, long long n, LossWs w) {
  __shared__ double shd[kLossTPB];
  __shared__ unsigned int shc[kLossTPB];
  const int t = threadIdx.x;
  const long long base = (long long)blockIdx.x * kLossChunk;
  double s = 0.0;
  unsigned int c = 0u;
  for (int k = t; k < kLossChunk; k += kLossTPB) {
    const long long i = base + k;
    if (i >= n) break;
    const int tv = tg[i];
    if (tv <= -1) continue;
    const double xv = (double)x[i];
    s += (xv > 0.0 ? xv : 0.0) - xv * (double)tv + log1p(exp(-fabs(xv)));
    c += 1u;
  }
  shd[t] = s; shc[t] = c;
  __syncthreads();
  for (int off = kLossTPB / 2; off > 0; off >>= 1) {
    if (t < off) { shd[t] += shd[t + off]; shc[t] += shc[t + off]; }
    __syncthreads();
  }
  if (t == 0) { w.psum[blockIdx.x] = shd[0]; w.pcnt[blockIdx.x] = shc[0]; }
}

__global__ __launch_bounds__(kLossTPB) void finish_kernel(LossWs w, long long chunks, double weight, float* __restrict__ loss,
                                                          int64_t* __restrict__ num) {
  __shared__ double shd[kLossTPB];
  __shared__ unsigned long long shc[kLossTPB];
  const int t = threadIdx.x;
  double s = 0.0;
  unsigned long long c = 0ull;
  for (long long k = t; k < chunks; k += kLossTPB) { s += w.psum[k]; c += w.pcnt[k]; }
  shd[t] = s; shc[t] = c;
  __syncthreads();
  for (int off = kLossTPB / 2; off > 0; off >>= 1) {
    if (t < off) { shd[t] += shd[t + off]; shc[t] += shc[t + off]; }
    __syncthreads();
  }
  if (t == 0) {
    const double W = (double)shc[0];
    loss[0] = shc[0] ? (float)(weight * shd[0] / W) : 0.f;      // W = 0 (the reference divides 0 by 0): loss 0, gradient 0
    w.scale[0] = shc[0] ? weight / W : 0.0;
    if (num) num[0] = (int64_t)shc[0];
  }
}

__global__ __launch_bounds__(kLossTPB) void grad_kernel(const float* __restrict__ x, const int* __restrict__ tg, long long n, LossWs w,
                                                        float* __restrict__ grad) {
  const long long i = (long long)blockIdx.x * kLossTPB + threadIdx.x;
  if (i >= n) return;
  const int tv = tg[i];
  float g = 0.f;
  if (tv > -1) {
    const double xv = (double)x[i], ex = exp(-fabs(xv));
    const double sig = xv >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex);
    g = (float)(w.scale[0] * (sig - (double)tv));
  }
  grad[i] = g;
}

inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

int loss_shape(long long num_rois, int mask_classes, int resolution, long long* n) {
  if (num_rois < 0 || mask_classes < 1 || resolution < 2) return M3D_EINVAL;
  if (resolution > kMaxRes || mask_classes > kMaxClasses || num_rois > (long long)kMaxFg * kMaxImages) return M3D_EUNSUPPORTED;
  *n = num_rois * mask_classes * resolution * resolution * resolution;
  if (*n >= (1ll << 31)) return M3D_EUNSUPPORTED;
  return M3D_OK;
}

}  // namespace

M3D_API int m3d_mask_targets(const int32_t* d_labels, const float* d_rois, const int64_t* d_counts, int num_images, int batch_per_im,
                             int fg_per_im, int resolution, int num_classes, int cls_specific, int mode, const int32_t* gt_offsets,
                             const int32_t* d_gt_classes, const uint8_t* d_gt_crowd, const float* d_spots, const int32_t* in_size,
                             const float* d_gt, const int32_t* d_markers, const m3d_mask_image* images, int32_t* d_masks,
                             float* d_mask_rois, int32_t* d_assign, int64_t* d_mask_counts, void* stream) {
  if (num_images < 1 || batch_per_im < 1 || fg_per_im < 1 || resolution < 2 || num_classes < 2 || !gt_offsets) return M3D_EINVAL;
  if (mode != M3D_MASK_SPOT && mode != M3D_MASK_LABELS) return M3D_EINVAL;
  if (num_images > kMaxImages || resolution > kMaxRes || num_classes > kMaxClasses || fg_per_im > kMaxFg) return M3D_EUNSUPPORTED;
  if (gt_offsets[0] != 0) return M3D_EINVAL;
  for (int b = 0; b < num_images; ++b) {
    const long long k = (long long)gt_offsets[b + 1] - gt_offsets[b];
    if (k < 0) return M3D_EINVAL;
    if (k > kMaxGt) return M3D_EUNSUPPORTED;
  }
  const int total = gt_offsets[num_images];
  if (!d_labels || !d_rois || !d_counts || !d_masks || !d_mask_rois || !d_assign || !d_mask_counts) return M3D_EINVAL;
  if (misaligned(d_labels, 4) || misaligned(d_rois, 4) || misaligned(d_counts, 8) || misaligned(d_masks, 4) || misaligned(d_mask_rois, 4) ||
      misaligned(d_assign, 4) || misaligned(d_mask_counts, 8) || misaligned(d_gt_classes, 4) || misaligned(d_spots, 4) ||
      misaligned(d_gt, 4) || misaligned(d_markers, 4))
    return M3D_EINVAL;
  Params p;
  memset(&p, 0, sizeof(p));
  if (mode == M3D_MASK_SPOT) {
    if (!in_size || in_size[0] < 1 || in_size[1] < 1 || in_size[2] < 1 || (total > 0 && !d_spots)) return M3D_EINVAL;
    p.top[0] = (float)(in_size[2] - 1); p.top[1] = (float)(in_size[1] - 1); p.top[2] = (float)(in_size[0] - 1);
  } else {
    if (!images || (total > 0 && (!d_gt || !d_markers))) return M3D_EINVAL;
    for (int b = 0; b < num_images; ++b) {
      const m3d_mask_image& im = images[b];
      // the sampler's counts stay on the device, so every image may hold fg rows: each needs an object list to rasterise from
      if (gt_offsets[b + 1] == gt_offsets[b]) return M3D_EINVAL;
      if (!im.labels || (im.dtype != 0 && im.dtype != 1) || im.depth < 1 || im.height < 1 || im.width < 1 ||
          misaligned(im.labels, im.dtype == 0 ? 2 : 4))
        return M3D_EINVAL;
      if ((long long)im.depth * im.height * im.width >= (1ll << 40)) return M3D_EUNSUPPORTED;
      p.img[b].labels = im.labels; p.img[b].dtype = im.dtype;
      p.img[b].depth = im.depth; p.img[b].height = im.height; p.img[b].width = im.width;
    }
  }
  for (int b = 0; b <= num_images; ++b) p.gt_off[b] = gt_offsets[b];
  p.B = num_images; p.batch = batch_per_im; p.fg_per_im = fg_per_im; p.M = resolution; p.num_classes = num_classes;
  p.cls_specific = cls_specific != 0; p.mode = mode;
  hipStream_t st = m3d::as_stream(stream);
  (void)hipMemsetAsync(d_mask_counts, 0, sizeof(int64_t) * 4 * (size_t)num_images, st);
  hipLaunchKernelGGL(targets_kernel, dim3(fg_per_im, num_images), dim3(kOne), 0, st, p, d_labels, d_rois, d_counts, d_gt_classes,
                     d_gt_crowd, d_spots, d_gt, d_markers, d_masks, d_mask_rois, d_assign,
                     reinterpret_cast<unsigned long long*>(d_mask_counts));
  return m3d::check_launch("mask_targets");
}

M3D_API size_t m3d_mask_loss_workspace_bytes(int64_t num_rois, int mask_classes, int resolution) {
  long long n;
  if (loss_shape(num_rois, mask_classes, resolution, &n) != M3D_OK) return 0;
  return carve_loss(nullptr, (n + kLossChunk - 1) / kLossChunk + 1).bytes;
}

M3D_API int m3d_mask_loss(const float* d_mask_pred, const int32_t* d_masks, int64_t num_rois, int mask_classes, int resolution,
                          double weight_loss_mask, float* d_loss, int64_t* d_num, float* d_grad, void* d_ws, size_t ws_bytes,
                          void* stream) {
  long long n;
  const int rc = loss_shape(num_rois, mask_classes, resolution, &n);
  if (rc != M3D_OK) return rc;
  if (!d_loss || !d_ws || misaligned(d_loss, 4) || misaligned(d_num, 8) || misaligned(d_ws, 8)) return M3D_EINVAL;
  if (n > 0 && (!d_mask_pred || !d_masks || !d_grad || misaligned(d_mask_pred, 4) || misaligned(d_masks, 4) || misaligned(d_grad, 4)))
    return M3D_EINVAL;
  const long long chunks = (n + kLossChunk - 1) / kLossChunk;
  const LossWs w = carve_loss(d_ws, chunks + 1);
  if (ws_bytes < w.bytes) return M3D_EWORKSPACE;
  hipStream_t st = m3d::as_stream(stream);
  if (chunks > 0) hipLaunchKernelGGL(partial_kernel, dim3((unsigned int)chunks), dim3(kLossTPB), 0, st, d_mask_pred, d_masks, n, w);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kLossTPB), 0, st, w, chunks, weight_loss_mask, d_loss, d_num);
  if (n > 0)
    hipLaunchKernelGGL(grad_kernel, dim3((unsigned int)((n + kLossTPB - 1) / kLossTPB)), dim3(kLossTPB), 0, st, d_mask_pred, d_masks, n, w,
                       d_grad);
  return m3d::check_launch("mask_loss");
}
