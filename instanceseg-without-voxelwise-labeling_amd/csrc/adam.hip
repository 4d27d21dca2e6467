// The solver's other optimiser and its gradient clip for gfx950 (DESIGN, "Solver"): the single-tensor torch.optim.Adam (amsgrad off,
// maximize off, coupled weight decay) over a whole parameter list in one launch per 64 descriptors, and the global-norm clip coefficient
// of clip_gradient (lib/utils/net.py:35-47) as a device scalar that the update kernels of this file and of sgd.hip read.
//
// fp32, built with -ffp-contract=off; per element, every operation rounded once, square root and division correctly rounded:
//   d = s g (only with a coefficient) ; d = (wd == 0) ? d : d + wd p ; m' = m + (1-b1) (d - m) ; v' = b2 v + (1-b2) (d d) ;
//   q = sqrt(v') / bc2_sqrt + eps ; p' = p - lr_step (m' / q)
// lr_step = lr / (1 - b1^t) and bc2_sqrt = sqrt(1 - b2^t) come from the host per tensor; 1-b1, b2, 1-b2 and eps are rounded from doubles.
// Chunking, descriptor passing and the statistics tree are those of sgd.hip (solver_common.h).  The order in which a thread adds its
// squares is that of sgd.hip's 16-byte path for the gradient's residue modulo 16, also where p, m or v lie at another residue and the
// chunk goes element by element: the statistics of m3d_adam_step and of m3d_grad_clip_coef depend on the gradients alone.
#include <math.h>

#include "solver_common.h"

namespace {

struct Seg {
  float* p;
  const float* g;
  float* m;
  float* v;
  long long n;
  float lr_step, bc2_sqrt, wd;
};
struct Args {
  Seg seg[kMaxSeg];
  int first[kMaxSeg + 1];   // workgroup of the launch at which segment s begins; first[nseg] = workgroups of the launch
  int nseg;
  float omb1, b2, omb2, eps;
  long long part0;          // index of the launch's first chunk among the chunks of the call
};
static_assert(sizeof(Args) <= 4096 - 16, "the descriptors and the two pointers must fit the kernel-argument space");

struct GradSeg {
  const float* g;
  long long n;
};
struct GradArgs {
  GradSeg seg[kMaxSeg];
  int first[kMaxSeg + 1];
  int nseg;
  long long part0;
};

struct Hyper {
  float lr_step, bc2_sqrt, wd, omb1, b2, omb2, eps, gs;
};

template <bool SCALED>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const Hyper& h) {
  float d = SCALED ? h.gs * g : g;
  d = h.wd == 0.f ? d : d + h.wd * p;
  m = m + h.omb1 * (d - m);
  v = h.b2 * v + h.omb2 * (d * d);
  const float q = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p - h.lr_step * (m / q);
}

// first[lo] <= b < first[hi]
__device__ __forceinline__ int segment_of(const int* first, int nseg, int b) {
  int lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// elements in front of the first 16-byte boundary of g, at most len
__device__ __forceinline__ int head_of(const float* g, int len) {
  const int head = (int)((4u - (unsigned)(((uintptr_t)g >> 2) & 3u)) & 3u);
  return head < len ? head : len;
}

template <bool STATS, bool SCALED>
__global__ __launch_bounds__(kTPB) void adam_step_kernel(const Args a, double* __restrict__ part, const float* __restrict__ gscale) {
  __shared__ double sm[8];
  const int b = blockIdx.x;
  const int lo = segment_of(a.first, a.nseg, b);
  const Seg sg = a.seg[lo];
  const long long off = (long long)(b - a.first[lo]) * kChunk;
  const long long left = sg.n - off;
  const int len = (int)(left < kChunk ? left : kChunk);
  float* p = sg.p + off;
  const float* g = sg.g + off;
  float* m = sg.m + off;
  float* v = sg.v + off;
  Hyper h;
  h.lr_step = sg.lr_step; h.bc2_sqrt = sg.bc2_sqrt; h.wd = sg.wd;
  h.omb1 = a.omb1; h.b2 = a.b2; h.omb2 = a.omb2; h.eps = a.eps;
  h.gs = SCALED ? *gscale : 1.f;
  double s = 0.0, bad = 0.0;

  // head, quads and tail are cut at g's 16-byte boundaries; the quads go in 16-byte accesses where p, m and v share g's residue
  const uintptr_t diff = ((uintptr_t)p ^ (uintptr_t)g) | ((uintptr_t)m ^ (uintptr_t)g) | ((uintptr_t)v ^ (uintptr_t)g);
  const bool wide = (diff & 15) == 0;
  const int head = head_of(g, len);
  for (int i = threadIdx.x; i < head; i += kTPB) {
    float pv = p[i], mv = m[i], vv = v[i];
    const float gv = g[i];
    if (STATS) stat_of(gv, s, bad);
    adam_one<SCALED>(pv, gv, mv, vv, h);
    p[i] = pv; m[i] = mv; v[i] = vv;
  }
  const int nq = (len - head) >> 2;
  if (wide) {
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    float4* m4 = reinterpret_cast<float4*>(m + head);
    float4* v4 = reinterpret_cast<float4*>(v + head);
#pragma unroll 2
    for (int i = threadIdx.x; i < nq; i += kTPB) {
      float4 pv = p4[i], mv = m4[i], vv = v4[i];
      const float4 gv = g4[i];
      if (STATS) { stat_of(gv.x, s, bad); stat_of(gv.y, s, bad); stat_of(gv.z, s, bad); stat_of(gv.w, s, bad); }
      adam_one<SCALED>(pv.x, gv.x, mv.x, vv.x, h);
      adam_one<SCALED>(pv.y, gv.y, mv.y, vv.y, h);
      adam_one<SCALED>(pv.z, gv.z, mv.z, vv.z, h);
      adam_one<SCALED>(pv.w, gv.w, mv.w, vv.w, h);
      p4[i] = pv; m4[i] = mv; v4[i] = vv;
    }
  } else {
    for (int i = threadIdx.x; i < nq; i += kTPB) {
      const int e = head + 4 * i;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pv = p[e + k], mv = m[e + k], vv = v[e + k];
        const float gv = g[e + k];
        if (STATS) stat_of(gv, s, bad);
        adam_one<SCALED>(pv, gv, mv, vv, h);
        p[e + k] = pv; m[e + k] = mv; v[e + k] = vv;
      }
    }
  }
  const int t = head + 4 * nq + (int)threadIdx.x;
  if (t < len) {
    float pv = p[t], mv = m[t], vv = v[t];
    const float gv = g[t];
    if (STATS) stat_of(gv, s, bad);
    adam_one<SCALED>(pv, gv, mv, vv, h);
    p[t] = pv; m[t] = mv; v[t] = vv;
  }
  if (STATS) {
    block_sum2(s, bad, sm);
    if (threadIdx.x == 0) {
      double* o = part + 2 * (a.part0 + b);
      o[0] = s; o[1] = bad;
    }
  }
}

// the statistics half of the update kernels alone: reads g, writes one partial and one count per chunk
__global__ __launch_bounds__(kTPB) void grad_stats_kernel(const GradArgs a, double* __restrict__ part) {
  __shared__ double sm[8];
  const int b = blockIdx.x;
  const int lo = segment_of(a.first, a.nseg, b);
  const GradSeg sg = a.seg[lo];
  const long long off = (long long)(b - a.first[lo]) * kChunk;
  const long long left = sg.n - off;
  const int len = (int)(left < kChunk ? left : kChunk);
  const float* g = sg.g + off;
  double s = 0.0, bad = 0.0;
  const int head = head_of(g, len);
  for (int i = threadIdx.x; i < head; i += kTPB) stat_of(g[i], s, bad);
  const int nq = (len - head) >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
#pragma unroll 2
  for (int i = threadIdx.x; i < nq; i += kTPB) {
    const float4 gv = g4[i];
    stat_of(gv.x, s, bad); stat_of(gv.y, s, bad); stat_of(gv.z, s, bad); stat_of(gv.w, s, bad);
  }
  const int t = head + 4 * nq + (int)threadIdx.x;
  if (t < len) stat_of(g[t], s, bad);
  block_sum2(s, bad, sm);
  if (threadIdx.x == 0) {
    double* o = part + 2 * (a.part0 + b);
    o[0] = s; o[1] = bad;
  }
}

// the finish of sgd.hip; with coef also clip_norm / max(sqrt(sum), clip_norm) in fp64, rounded to fp32.  The larger of the two is taken
// as Python's max(norm, clip_norm) takes it: a NaN norm stays and makes the coefficient NaN.
__global__ __launch_bounds__(kTPB) void adam_stats_finish_kernel(const double* __restrict__ part, long long chunks, double* __restrict__ stats,
                                                                 double clip_norm, float* __restrict__ coef) {
  __shared__ double sm[8];
  double s, bad;
  finish_sum2(part, chunks, s, bad, sm);
  if (threadIdx.x == 0) {
    stats[0] = s; stats[1] = bad;
    if (coef) {
      const double norm = sqrt(s);
      *coef = (float)(clip_norm / (clip_norm > norm ? clip_norm : norm));
    }
  }
}

int validate_adam(const m3d_adam_tensor* t, int count, double beta1, double beta2, double eps, const float* d_gscale, long long* chunks) {
  if (count < 0) return M3D_EINVAL;
  if (count > kMaxCount) return M3D_EUNSUPPORTED;
  if (count > 0 && !t) return M3D_EINVAL;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !((float)eps > 0.f)) return M3D_EINVAL;
  if ((uintptr_t)d_gscale & 3) return M3D_EINVAL;
  long long total = 0;
  for (int i = 0; i < count; ++i) {
    const m3d_adam_tensor& e = t[i];
    if (e.n < 0) return M3D_EINVAL;
    if (e.n >= kMaxN) return M3D_EUNSUPPORTED;
    if (e.n == 0) continue;
    if (!e.p || !e.g || !e.m || !e.v) return M3D_EINVAL;
    if (((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v) & 3) return M3D_EINVAL;
    if (!apart(e.p, e.g, e.n) || !apart(e.p, e.m, e.n) || !apart(e.p, e.v, e.n) || !apart(e.g, e.m, e.n) || !apart(e.g, e.v, e.n) ||
        !apart(e.m, e.v, e.n))
      return M3D_EINVAL;
    if (!(e.bc2_sqrt > 0.f && e.bc2_sqrt <= 1.f)) return M3D_EINVAL;
    total += chunks_of(e.n);
  }
  *chunks = total;
  return M3D_OK;
}

int validate_grads(const m3d_grad_tensor* t, int count, long long* chunks) {
  if (count < 0) return M3D_EINVAL;
  if (count > kMaxCount) return M3D_EUNSUPPORTED;
  if (count > 0 && !t) return M3D_EINVAL;
  long long total = 0;
  for (int i = 0; i < count; ++i) {
    const m3d_grad_tensor& e = t[i];
    if (e.n < 0) return M3D_EINVAL;
    if (e.n >= kMaxN) return M3D_EUNSUPPORTED;
    if (e.n == 0) continue;
    if (!e.g || ((uintptr_t)e.g & 3)) return M3D_EINVAL;
    total += chunks_of(e.n);
  }
  *chunks = total;
  return M3D_OK;
}

void launch_adam(const Args& a, double* part, const float* gscale, hipStream_t st) {
  const dim3 grid((unsigned)a.first[a.nseg]), block(kTPB);
  if (gscale) {
    if (part) hipLaunchKernelGGL((adam_step_kernel<true, true>), grid, block, 0, st, a, part, gscale);
    else hipLaunchKernelGGL((adam_step_kernel<false, true>), grid, block, 0, st, a, part, gscale);
  } else {
    if (part) hipLaunchKernelGGL((adam_step_kernel<true, false>), grid, block, 0, st, a, part, gscale);
    else hipLaunchKernelGGL((adam_step_kernel<false, false>), grid, block, 0, st, a, part, gscale);
  }
}

// cuts the chunks of `count` tensors of size_of(i) elements into launches of at most kMaxSeg segments and kMaxBlocks workgroups:
// fill(seg, i, first element, elements) writes a segment's descriptor, flush() launches what `a` holds
template <class A, class Size, class Fill, class Flush>
void for_each_launch(A& a, int count, Size size_of, Fill fill, Flush flush) {
  a.nseg = 0;
  a.first[0] = 0;
  a.part0 = 0;
  long long at = 0;                  // chunks of the call in front of the current position
  for (int i = 0; i < count; ++i) {
    const long long n = size_of(i);
    const long long nc = chunks_of(n);
    long long done = 0;
    while (done < nc) {
      if (a.nseg == 0) a.part0 = at + done;
      long long take = nc - done;
      const long long room = kMaxBlocks - a.first[a.nseg];
      if (take > room) take = room;
      const long long left = n - done * kChunk;
      fill(a.seg[a.nseg], i, done * kChunk, left < take * kChunk ? left : take * kChunk);
      a.first[a.nseg + 1] = a.first[a.nseg] + (int)take;
      ++a.nseg;
      done += take;
      if (a.nseg == kMaxSeg || a.first[a.nseg] == kMaxBlocks) {
        flush();
        a.nseg = 0;
      }
    }
    at += nc;
  }
  if (a.nseg > 0) flush();
}

}  // namespace

M3D_API int m3d_adam_step(const m3d_adam_tensor* tensors, int count, double beta1, double beta2, double eps, const float* d_gscale,
                          double* d_stats, void* d_ws, size_t* ws_bytes, void* stream) {
  long long chunks = 0;
  int rc = validate_adam(tensors, count, beta1, beta2, eps, d_gscale, &chunks);
  if (rc != M3D_OK) return rc;
  bool query = false;
  rc = stats_workspace(d_stats, d_ws, ws_bytes, chunks, &query);
  if (rc != M3D_OK || query) return rc;
  if (chunks == 0 && !d_stats) return M3D_OK;   // nothing to do: the runtime is not touched
  hipStream_t st = m3d::as_stream(stream);
  double* part = d_stats ? (double*)d_ws : nullptr;
  Args a;
  a.omb1 = (float)(1.0 - beta1);
  a.b2 = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  for_each_launch(
      a, count, [&](int i) { return tensors[i].n; },
      [&](Seg& s, int i, long long from, long long n) {
        const m3d_adam_tensor& e = tensors[i];
        s.p = e.p + from; s.g = e.g + from; s.m = e.m + from; s.v = e.v + from;
        s.n = n;
        s.lr_step = e.lr_step; s.bc2_sqrt = e.bc2_sqrt; s.wd = e.wd;
      },
      [&]() { launch_adam(a, part, d_gscale, st); });
  if (d_stats)
    hipLaunchKernelGGL(adam_stats_finish_kernel, dim3(1), dim3(kTPB), 0, st, (const double*)part, chunks, d_stats, 0.0, (float*)nullptr);
  return m3d::check_launch("adam_step");
}

M3D_API int m3d_grad_clip_coef(const m3d_grad_tensor* tensors, int count, double clip_norm, double* d_stats, float* d_coef, void* d_ws,
                               size_t* ws_bytes, void* stream) {
  long long chunks = 0;
  int rc = validate_grads(tensors, count, &chunks);
  if (rc != M3D_OK) return rc;
  if (!(clip_norm > 0.0 && clip_norm < INFINITY)) return M3D_EINVAL;
  if (!d_stats || !d_coef || ((uintptr_t)d_coef & 3)) return M3D_EINVAL;
  bool query = false;
  rc = stats_workspace(d_stats, d_ws, ws_bytes, chunks, &query);
  if (rc != M3D_OK || query) return rc;
  hipStream_t st = m3d::as_stream(stream);
  double* part = (double*)d_ws;
  GradArgs a;
  for_each_launch(
      a, count, [&](int i) { return tensors[i].n; },
      [&](GradSeg& s, int i, long long from, long long n) {
        s.g = tensors[i].g + from;
        s.n = n;
      },
      [&]() { hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)a.first[a.nseg]), dim3(kTPB), 0, st, a, part); });
  hipLaunchKernelGGL(adam_stats_finish_kernel, dim3(1), dim3(kTPB), 0, st, (const double*)part, chunks, d_stats, clip_norm, d_coef);
  return m3d::check_launch("grad_clip_coef");
}
