// Training minibatches on the device for gfx950 (DESIGN, "Training samples"): the volumes stay resident as uint16 with their norm1
// statistics, and a call produces the fp32 tiles [count, s, h, w] and their ground-truth boxes.  Reference: prep_im_for_blob(...,
// 'train') and crop_data_3d of lib/utils/blob.py:97-202, which do this with NumPy on the host for every sample of every step.
//
// Two launches.  The search kernel (one workgroup per image) draws the start of the candidate grid from the sampling contract, scores
// every candidate crop by the clipped box volume it contains (fp64, in box order), takes the first strict maximum and then shifts, clips,
// filters and compacts the boxes for that origin.  The apply kernel reads the origin from d_info and writes the normalised crop with the
// arithmetic of norm1_apply_kernel (f32_arith = 1): the output is bit-equal to m3d_norm1 of the whole volume, cropped.
// The descriptors travel as kernel arguments: a call copies nothing to the device, allocates nothing and never waits.  Selection is by
// value and index only - no floating-point atomics - so the results are bit-identical run to run.
#include "train_common.h"

namespace {

using m3dtrain::kOne;

constexpr int kMaxImages = 64;        // descriptors per call (48 bytes each for the search, 32 for the apply: the kernel-argument space holds 4 KB)
constexpr int kMaxBoxes = 2048;       // boxes of one image: staged in LDS (48 KB), two per thread in the compaction
constexpr int kTPB = 256;             // apply kernel
constexpr int kApplyBlocks = 4096;    // workgroups per image of the apply kernel, at most

struct SearchImg {
  const float* boxes;
  unsigned long long stream;          // seed_stream(seed)
  int dim[3];                         // width, height, depth: axis order x, y, z
  int start[3];                       // start_max, or the fixed origin
  int num_boxes;
};
struct SearchArgs {
  SearchImg img[kMaxImages];
  int size[3];                        // x, y, z
  int mode;                           // 0: search, 1: fixed origin, 2: no crop
  int max_boxes;
};
struct ApplyImg {
  const void* vol;
  const double* stats;
  int dim[3];
  int dtype;
};
struct ApplyArgs {
  ApplyImg img[kMaxImages];
  int size[3];
};
static_assert(sizeof(SearchArgs) + 64 <= 4096 && sizeof(ApplyArgs) + 64 <= 4096, "the descriptors must fit the kernel-argument space");

// fp32 shift and clip of blob.py:134-139: np.clip(b - o, 0, size - 1)
__device__ __forceinline__ float shift_clip(float b, float o, float hi) { return fminf(fmaxf(b - o, 0.f), hi); }

// the volume a box contributes at origin o, or 0 if the crop makes it degenerate (blob.py:140-143)
__device__ __forceinline__ double box_score(const float* b, const float* o, const float* hi) {
  float c[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) c[j] = shift_clip(b[j], o[j % 3], hi[j % 3]);
  if (c[0] == c[3] || c[1] == c[4] || c[2] == c[5]) return 0.0;
  return ((((double)c[3] - (double)c[0]) + 1.0) * (((double)c[4] - (double)c[1]) + 1.0)) * (((double)c[5] - (double)c[2]) + 1.0);
}

// candidates of one axis: range(start, last, step) followed by last  (blob.py:121-127)
__device__ __forceinline__ int axis_count(int start, int last, int step) { return (start < last ? (last - start + step - 1) / step : 0) + 1; }
__device__ __forceinline__ int axis_value(int start, int last, int step, int n, int i) { return i == n - 1 ? last : start + i * step; }

__global__ __launch_bounds__(kOne) void train_search_kernel(const SearchArgs a, float* __restrict__ out_boxes, int* __restrict__ out_keep,
                                                            int* __restrict__ info, double* __restrict__ score) {
  __shared__ float sbox[kMaxBoxes * 6];
  __shared__ double sval[kOne];
  __shared__ unsigned int sidx[kOne];
  const int b = blockIdx.x, t = threadIdx.x;
  const SearchImg im = a.img[b];
  const int K = im.num_boxes;
  for (int i = t; i < K * 6; i += kOne) sbox[i] = im.boxes[i];
  __syncthreads();

  const float hi[3] = {(float)(a.size[0] - 1), (float)(a.size[1] - 1), (float)(a.size[2] - 1)};
  int org[3] = {0, 0, 0};
  int ncand = 0, status = 0;
  double best = 0.0;
  if (a.mode != 2) {
    int start[3], last[3], step[3], cnt[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      last[ax] = im.dim[ax] - a.size[ax];
      step[ax] = a.size[ax] / 2;
      if (a.mode == 1) {
        start[ax] = im.start[ax];
        cnt[ax] = 1;
      } else {
        const unsigned int sm = (unsigned int)im.start[ax];
        start[ax] = sm == 0 ? 0 : (int)(((unsigned long long)m3dtrain::mix_key(im.stream, (unsigned long long)ax) * (sm + 1ull)) >> 32);
        cnt[ax] = axis_count(start[ax], last[ax], step[ax]);
      }
    }
    ncand = cnt[0] * cnt[1] * cnt[2];           // < 2^31: checked by the host
    // every thread scores the candidates t, t + kOne, ... in ascending order and keeps its first strict maximum
    unsigned int bi = 0xffffffffu;
    for (int c = t; c < ncand; c += kOne) {
      const int ix = c % cnt[0], iy = (c / cnt[0]) % cnt[1], iz = c / (cnt[0] * cnt[1]);
      float o[3];
      if (a.mode == 1) {
        o[0] = (float)start[0]; o[1] = (float)start[1]; o[2] = (float)start[2];
      } else {
        o[0] = (float)axis_value(start[0], last[0], step[0], cnt[0], ix);
        o[1] = (float)axis_value(start[1], last[1], step[1], cnt[1], iy);
        o[2] = (float)axis_value(start[2], last[2], step[2], cnt[2], iz);
      }
      double s = 0.0;
      for (int k = 0; k < K; ++k) s += box_score(sbox + 6 * k, o, hi);
      if (s > best) { best = s; bi = (unsigned int)c; }
    }
    // the workgroup's maximum; among equal scores the smallest candidate index
    sval[t] = best; sidx[t] = bi;
    __syncthreads();
    for (int off = kOne / 2; off > 0; off >>= 1) {
      if (t < off) {
        const double v = sval[t + off];
        const unsigned int i = sidx[t + off];
        if (v > sval[t] || (v == sval[t] && i < sidx[t])) { sval[t] = v; sidx[t] = i; }
      }
      __syncthreads();
    }
    best = sval[0];
    unsigned int win = sidx[0];
    __syncthreads();
    if (win == 0xffffffffu) { win = 0; status = 1; }          // no candidate scores above 0
    if (a.mode == 1) {
      org[0] = start[0]; org[1] = start[1]; org[2] = start[2];
    } else {
      const int c = (int)win;
      org[0] = axis_value(start[0], last[0], step[0], cnt[0], c % cnt[0]);
      org[1] = axis_value(start[1], last[1], step[1], cnt[1], (c / cnt[0]) % cnt[1]);
      org[2] = axis_value(start[2], last[2], step[2], cnt[2], c / (cnt[0] * cnt[1]));
    }
  }

  // shift, clip, filter and compact the boxes in order (blob.py:150-199): thread t takes boxes 2t and 2t + 1
  const float o[3] = {(float)org[0], (float)org[1], (float)org[2]};
  float c[2][6];
  bool keep[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = 2 * t + h;
    keep[h] = false;
    if (k < K) {
      if (a.mode == 2) {
#pragma unroll
        for (int j = 0; j < 6; ++j) c[h][j] = sbox[6 * k + j];
        keep[h] = true;
      } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) c[h][j] = shift_clip(sbox[6 * k + j], o[j % 3], hi[j % 3]);
        keep[h] = !(c[h][0] == c[h][3] || c[h][1] == c[h][4] || c[h][2] == c[h][5]);
      }
    }
  }
  unsigned int kept = 0;
  unsigned int at = m3dtrain::block_exscan((unsigned int)keep[0] + (unsigned int)keep[1], sidx, &kept);
  float* ob = out_boxes + (size_t)b * a.max_boxes * 6;
  int* ok = out_keep + (size_t)b * a.max_boxes;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (keep[h]) {
#pragma unroll
      for (int j = 0; j < 6; ++j) ob[6 * at + j] = c[h][j];
      ok[at] = 2 * t + h;
      ++at;
    }
  }
  for (int r = (int)kept + t; r < a.max_boxes; r += kOne) {
#pragma unroll
    for (int j = 0; j < 6; ++j) ob[6 * r + j] = 0.f;
    ok[r] = -1;
  }
  if (t == 0) {
    int* fo = info + 8 * b;
    fo[0] = org[0]; fo[1] = org[1]; fo[2] = org[2]; fo[3] = (int)kept; fo[4] = status; fo[5] = ncand; fo[6] = 0; fo[7] = 0;
    score[b] = best;
  }
}

// 4 elements of T on any element boundary
template <typename T> struct __attribute__((packed, aligned(sizeof(T)))) Quad { T v[4]; };
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Work items of an image: (row of the output, slot), slots = ceil(w / 4) + 1 per row.  Slot 0 stores the elements in front of the row's
// first 16-byte boundary, slots 1 .. nv one aligned 16-byte vector each, slot nv + 1 the elements behind the last whole vector.  A tile
// whose width is a multiple of 4 on a 16-byte aligned base has neither head nor tail; a row too short or misplaced for a vector goes
// element by element.  The source row starts wherever the origin puts it.
// I: the type the item index is taken apart in (32-bit division where the tile allows it)
template <typename T, typename I>
__device__ __forceinline__ void apply_rows(const T* __restrict__ vol, const int* dim, const int* size, const int* org, float mf, float sf,
                                           float* __restrict__ out) {
  const int w = size[0], h = size[1];
  const int nslot = (w + 3) / 4 + 1;
  const I items = (I)size[2] * h * nslot;
  for (I it = (I)blockIdx.x * kTPB + threadIdx.x; it < items; it += (I)gridDim.x * kTPB) {
    const I row = it / nslot;
    const int slot = (int)(it - row * nslot);
    const int z = (int)(row / h), y = (int)(row - (I)z * h);
    float* orow = out + (long long)row * w;
    const T* irow = vol + ((long long)(org[2] + z) * dim[1] + (org[1] + y)) * dim[0] + org[0];
    int head = (int)(((16 - ((uintptr_t)orow & 15)) & 15) >> 2);
    head = head < w ? head : w;
    const int nv = (w - head) >> 2;
    if (slot >= 1 && slot <= nv) {
      const int x = head + 4 * (slot - 1);
      const Quad<T> p = *reinterpret_cast<const Quad<T>*>(irow + x);
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ((float)p.v[j] - mf) / sf;
      *reinterpret_cast<f32x4*>(orow + x) = v;
    } else if (slot == 0) {
      for (int x = 0; x < head; ++x) orow[x] = ((float)irow[x] - mf) / sf;
    } else if (slot == nv + 1) {
      for (int x = head + 4 * nv; x < w; ++x) orow[x] = ((float)irow[x] - mf) / sf;
    }
  }
}
template <typename T>
__device__ __forceinline__ void apply_image(const T* __restrict__ vol, const int* dim, const int* size, const int* org, float mf, float sf,
                                            float* __restrict__ out) {
  const long long reach = (long long)size[2] * size[1] * ((size[0] + 3) / 4 + 1) + (long long)kApplyBlocks * kTPB;
  if (reach < (1ll << 32)) apply_rows<T, unsigned int>(vol, dim, size, org, mf, sf, out);
  else apply_rows<T, long long>(vol, dim, size, org, mf, sf, out);
}

__global__ __launch_bounds__(kTPB) void train_apply_kernel(const ApplyArgs a, const int* __restrict__ info, float* __restrict__ data) {
  const int b = blockIdx.y;
  const ApplyImg im = a.img[b];
  int org[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {            // the origin comes from device memory: keep every read inside the volume whatever it holds
    const int o = info[8 * b + ax], last = im.dim[ax] - a.size[ax];
    org[ax] = o < 0 ? 0 : (o > last ? last : o);
  }
  const float mf = (float)im.stats[0], sf = (float)im.stats[1];
  float* out = data + (size_t)b * a.size[0] * a.size[1] * a.size[2];
  if (im.dtype == 0) apply_image((const uint16_t*)im.vol, im.dim, a.size, org, mf, sf, out);
  else apply_image((const float*)im.vol, im.dim, a.size, org, mf, sf, out);
}

// M3D_OK or the refusal; no device pointer is followed and nothing is launched
int validate(const m3d_train_image* im, int count, const int* in_size, int need_crop, const uint64_t* seeds, const int* fixed, int max_boxes,
             const float* d_data, const float* d_boxes, const int32_t* d_keep, const int32_t* d_info, const double* d_score) {
  if (count < 0) return M3D_EINVAL;
  if (count > kMaxImages) return M3D_EUNSUPPORTED;
  if (count == 0) return M3D_OK;
  if (!im || !in_size || !d_data || !d_boxes || !d_keep || !d_info || !d_score) return M3D_EINVAL;
  if (need_crop && !fixed && !seeds) return M3D_EINVAL;
  if ((((uintptr_t)d_data | (uintptr_t)d_boxes | (uintptr_t)d_keep | (uintptr_t)d_info) & 3) || ((uintptr_t)d_score & 7)) return M3D_EINVAL;
  const int size[3] = {in_size[2], in_size[1], in_size[0]};       // x, y, z
  for (int ax = 0; ax < 3; ++ax)
    if (size[ax] < 2) return M3D_EINVAL;
  for (int i = 0; i < count; ++i) {
    const m3d_train_image& e = im[i];
    if (e.dtype != 0 && e.dtype != 1) return M3D_EINVAL;
    if (!e.vol || !e.stats || !e.boxes) return M3D_EINVAL;
    if (((uintptr_t)e.vol % (e.dtype == 0 ? 2 : 4)) || ((uintptr_t)e.stats & 7) || ((uintptr_t)e.boxes & 3)) return M3D_EINVAL;
    if (e.num_boxes < 1) return M3D_EINVAL;
    const int dim[3] = {e.width, e.height, e.depth};
    long long cand = 1;
    for (int ax = 0; ax < 3; ++ax) {
      const int last = dim[ax] - size[ax];
      if (last < 0) return M3D_EINVAL;
      if (!need_crop) {
        if (last != 0) return M3D_EINVAL;
      } else if (fixed) {
        if (fixed[3 * i + ax] < 0 || fixed[3 * i + ax] > last) return M3D_EINVAL;
      } else {
        if (e.start_max[ax] < 0 || e.start_max[ax] > last) return M3D_EINVAL;
        cand *= last / (size[ax] / 2) + 2;                          // at most, whatever the start
      }
    }
    if (e.num_boxes > kMaxBoxes || max_boxes < e.num_boxes) return M3D_EUNSUPPORTED;
    if (cand >= (1ll << 31)) return M3D_EUNSUPPORTED;
  }
  return M3D_OK;
}

}  // namespace

M3D_API int m3d_train_sample(const m3d_train_image* images, int count, const int* in_size, int need_crop, const uint64_t* seeds,
                             const int* fixed_origin, int max_boxes, float* d_data, float* d_boxes, int32_t* d_keep, int32_t* d_info,
                             double* d_score, void* d_ws, size_t* ws_bytes, void* stream) {
  const int rc = validate(images, count, in_size, need_crop, seeds, fixed_origin, max_boxes, d_data, d_boxes, d_keep, d_info, d_score);
  if (rc != M3D_OK) return rc;
  if (!d_ws && ws_bytes) {           // the size query
    *ws_bytes = 0;
    return M3D_OK;
  }
  if (count == 0) return M3D_OK;     // nothing to do: the runtime is not touched
  hipStream_t st = m3d::as_stream(stream);
  SearchArgs sa;
  ApplyArgs aa;
  memset(&sa, 0, sizeof(sa));
  memset(&aa, 0, sizeof(aa));
  for (int ax = 0; ax < 3; ++ax) sa.size[ax] = aa.size[ax] = in_size[2 - ax];
  sa.mode = !need_crop ? 2 : (fixed_origin ? 1 : 0);
  sa.max_boxes = max_boxes;
  for (int i = 0; i < count; ++i) {
    const m3d_train_image& e = images[i];
    const int dim[3] = {e.width, e.height, e.depth};
    SearchImg& s = sa.img[i];
    ApplyImg& p = aa.img[i];
    s.boxes = e.boxes;
    s.stream = sa.mode == 0 ? m3dtrain::seed_stream(seeds[i]) : 0ull;
    s.num_boxes = e.num_boxes;
    p.vol = e.vol;
    p.stats = e.stats;
    p.dtype = e.dtype;
    for (int ax = 0; ax < 3; ++ax) {
      s.dim[ax] = p.dim[ax] = dim[ax];
      s.start[ax] = sa.mode == 1 ? fixed_origin[3 * i + ax] : (sa.mode == 0 ? e.start_max[ax] : 0);
    }
  }
  hipLaunchKernelGGL(train_search_kernel, dim3(count), dim3(kOne), 0, st, sa, d_boxes, d_keep, d_info, d_score);
  const long long items = (long long)in_size[0] * in_size[1] * ((in_size[2] + 3) / 4 + 1);
  long long blocks = (items + kTPB * 4 - 1) / (kTPB * 4);
  if (blocks > kApplyBlocks) blocks = kApplyBlocks;
  hipLaunchKernelGGL(train_apply_kernel, dim3((unsigned)blocks, count), dim3(kTPB), 0, st, aa, (const int*)d_info, d_data);
  return m3d::check_launch("train_sample");
}
