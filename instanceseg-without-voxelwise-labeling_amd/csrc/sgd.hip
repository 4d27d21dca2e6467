// The solver's parameter update for gfx950: SGD with momentum, weight decay and a momentum-buffer scale over a whole parameter list in
// one launch, and optionally the squared gradient norm and the count of non-finite gradient elements (DESIGN, "Solver").  Reference:
// torch.optim.SGD as tools/train_net_step.py:316-331 builds it, and _CorrectMomentum of lib/utils/net.py:86-99 (the buffer scale).
//
// fp32, built with -ffp-contract=off; per element, every operation rounded once:
//   c = mscale m ; d = (wd == 0) ? g : g + wd p ; m' = momentum c + d ; p' = p - lr m'          (m == NULL: p' = p - lr d)
// m3d_sgd_step_scaled: the same with g replaced by s g, s one fp32 read from device memory (the clip coefficient of adam.hip); the
// statistics stay those of the raw gradients.  Without s it runs the very kernels of m3d_sgd_step.
// Work is cut into chunks of kChunk elements of one tensor (a function of the tensors' sizes and order only); one workgroup per chunk.
// The tensors' descriptors travel as kernel arguments: a step copies nothing to the device, allocates nothing and never waits.
// Statistics: one fp64 partial and one count per chunk, summed by a finish kernel in a fixed order - no floating-point atomics.
#include "solver_common.h"

namespace {

// a run of whole chunks of one tensor (a tensor of more than kMaxBlocks chunks takes several)
struct Seg {
  float* p;
  const float* g;
  float* m;
  long long n;
  float lr, wd;
};
struct Args {
  Seg seg[kMaxSeg];
  int first[kMaxSeg + 1];   // workgroup of the launch at which segment s begins; first[nseg] = workgroups of the launch
  int nseg;
  float momentum, mscale;
  long long part0;          // index of the launch's first chunk among the chunks of the call
};
static_assert(sizeof(Args) <= 4096 - 16, "the descriptors must fit the kernel-argument space");

__device__ __forceinline__ float sgd_d(float p, float g, float wd) { return wd == 0.f ? g : g + wd * p; }

template <bool HAS_M>
__device__ __forceinline__ void sgd_one(float& p, float g, float& m, float lr, float wd, float momentum, float mscale) {
  const float d = sgd_d(p, g, wd);
  if (HAS_M) {
    const float c = mscale * m;
    m = momentum * c + d;
    p = p - lr * m;
  } else {
    p = p - lr * d;
  }
}

template <bool HAS_M, bool STATS, bool SCALED>
__global__ __launch_bounds__(kTPB) void sgd_step_kernel(const Args a, double* __restrict__ part, const float* __restrict__ gscale) {
  __shared__ double sm[8];
  const int b = blockIdx.x;
  int lo = 0, hi = a.nseg;          // first[lo] <= b < first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first[mid] <= b) lo = mid; else hi = mid;
  }
  const Seg sg = a.seg[lo];
  const long long off = (long long)(b - a.first[lo]) * kChunk;
  const long long left = sg.n - off;
  const int len = (int)(left < kChunk ? left : kChunk);
  float* p = sg.p + off;
  const float* g = sg.g + off;
  float* m = HAS_M ? sg.m + off : nullptr;
  const float lr = sg.lr, wd = sg.wd, mu = a.momentum, ms = a.mscale;
  const float gs = SCALED ? *gscale : 1.f;
  double s = 0.0, bad = 0.0;

  // 16-byte accesses from the first common 16-byte boundary; a tensor whose pointers differ modulo 16 goes element by element
  uintptr_t diff = (uintptr_t)p ^ (uintptr_t)g;
  if (HAS_M) diff |= (uintptr_t)p ^ (uintptr_t)m;
  int head = len;
  if ((diff & 15) == 0) {
    head = (int)((4u - (unsigned)(((uintptr_t)p >> 2) & 3u)) & 3u);
    head = head < len ? head : len;
  }
  for (int i = threadIdx.x; i < head; i += kTPB) {
    float pv = p[i], mv = HAS_M ? m[i] : 0.f;
    const float gv = g[i];
    if (STATS) stat_of(gv, s, bad);
    sgd_one<HAS_M>(pv, SCALED ? gs * gv : gv, mv, lr, wd, mu, ms);
    p[i] = pv;
    if (HAS_M) m[i] = mv;
  }
  const int nq = (len - head) >> 2;
  float4* p4 = reinterpret_cast<float4*>(p + head);
  const float4* g4 = reinterpret_cast<const float4*>(g + head);
  float4* m4 = HAS_M ? reinterpret_cast<float4*>(m + head) : nullptr;
#pragma unroll 2
  for (int i = threadIdx.x; i < nq; i += kTPB) {
    float4 pv = p4[i];
    const float4 gv = g4[i];
    float4 mv = HAS_M ? m4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (STATS) { stat_of(gv.x, s, bad); stat_of(gv.y, s, bad); stat_of(gv.z, s, bad); stat_of(gv.w, s, bad); }
    sgd_one<HAS_M>(pv.x, SCALED ? gs * gv.x : gv.x, mv.x, lr, wd, mu, ms);
    sgd_one<HAS_M>(pv.y, SCALED ? gs * gv.y : gv.y, mv.y, lr, wd, mu, ms);
    sgd_one<HAS_M>(pv.z, SCALED ? gs * gv.z : gv.z, mv.z, lr, wd, mu, ms);
    sgd_one<HAS_M>(pv.w, SCALED ? gs * gv.w : gv.w, mv.w, lr, wd, mu, ms);
    p4[i] = pv;
    if (HAS_M) m4[i] = mv;
  }
  const int t = head + 4 * nq + (int)threadIdx.x;
  if (t < len) {
    float pv = p[t], mv = HAS_M ? m[t] : 0.f;
    const float gv = g[t];
    if (STATS) stat_of(gv, s, bad);
    sgd_one<HAS_M>(pv, SCALED ? gs * gv : gv, mv, lr, wd, mu, ms);
    p[t] = pv;
    if (HAS_M) m[t] = mv;
  }
  if (STATS) {
    block_sum2(s, bad, sm);
    if (threadIdx.x == 0) {
      double* o = part + 2 * (a.part0 + b);
      o[0] = s; o[1] = bad;
    }
  }
}

__global__ __launch_bounds__(kTPB) void sgd_stats_finish_kernel(const double* __restrict__ part, long long chunks, double* __restrict__ stats) {
  __shared__ double sm[8];
  double s, bad;
  finish_sum2(part, chunks, s, bad, sm);
  if (threadIdx.x == 0) { stats[0] = s; stats[1] = bad; }
}

// M3D_OK and the number of chunks of the call, or the refusal; no device pointer is followed and nothing is launched
int validate(const m3d_sgd_tensor* t, int count, float momentum, long long* chunks) {
  if (count < 0) return M3D_EINVAL;
  if (count > kMaxCount) return M3D_EUNSUPPORTED;
  if (count > 0 && !t) return M3D_EINVAL;
  long long total = 0;
  for (int i = 0; i < count; ++i) {
    const m3d_sgd_tensor& e = t[i];
    if (e.n < 0) return M3D_EINVAL;
    if (e.n >= kMaxN) return M3D_EUNSUPPORTED;
    if (e.n == 0) continue;
    if (!e.m && momentum != 0.f) return M3D_EINVAL;
    if (!e.p || !e.g) return M3D_EINVAL;
    if (((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m) & 3) return M3D_EINVAL;
    if (!apart(e.p, e.g, e.n) || (e.m && (!apart(e.p, e.m, e.n) || !apart(e.g, e.m, e.n)))) return M3D_EINVAL;
    total += chunks_of(e.n);
  }
  *chunks = total;
  return M3D_OK;
}

template <bool SCALED>
void launch_as(const Args& a, bool has_m, double* part, const float* gscale, hipStream_t st) {
  const dim3 grid((unsigned)a.first[a.nseg]), block(kTPB);
  if (has_m) {
    if (part) hipLaunchKernelGGL((sgd_step_kernel<true, true, SCALED>), grid, block, 0, st, a, part, gscale);
    else hipLaunchKernelGGL((sgd_step_kernel<true, false, SCALED>), grid, block, 0, st, a, part, gscale);
  } else {
    if (part) hipLaunchKernelGGL((sgd_step_kernel<false, true, SCALED>), grid, block, 0, st, a, part, gscale);
    else hipLaunchKernelGGL((sgd_step_kernel<false, false, SCALED>), grid, block, 0, st, a, part, gscale);
  }
}

void launch(const Args& a, bool has_m, double* part, const float* gscale, hipStream_t st) {
  if (gscale) launch_as<true>(a, has_m, part, gscale, st);
  else launch_as<false>(a, has_m, part, gscale, st);
}

int sgd_step(const m3d_sgd_tensor* tensors, int count, float momentum, float mscale, const float* d_gscale, double* d_stats, void* d_ws,
             size_t* ws_bytes, void* stream) {
  long long chunks = 0;
  int rc = validate(tensors, count, momentum, &chunks);
  if (rc != M3D_OK) return rc;
  if ((uintptr_t)d_gscale & 3) return M3D_EINVAL;
  bool query = false;
  rc = stats_workspace(d_stats, d_ws, ws_bytes, chunks, &query);
  if (rc != M3D_OK || query) return rc;
  if (chunks == 0 && !d_stats) return M3D_OK;   // nothing to do: the runtime is not touched
  hipStream_t st = m3d::as_stream(stream);
  double* part = d_stats ? (double*)d_ws : nullptr;
  // with a buffer on every tensor the list goes through the momentum kernel; tensors without one (momentum == 0) through the plain one
  for (int pass = 0; pass < 2; ++pass) {
    const bool has_m = pass == 0;
    Args a;
    a.nseg = 0;
    a.first[0] = 0;
    a.momentum = momentum;
    a.mscale = mscale;
    a.part0 = 0;
    long long at = 0;                // chunks of the call in front of the current position
    for (int i = 0; i < count; ++i) {
      const m3d_sgd_tensor& e = tensors[i];
      const long long nc = chunks_of(e.n);
      if ((e.m != nullptr) == has_m) {
        long long done = 0;
        while (done < nc) {
          if (a.nseg == 0) a.part0 = at + done;
          long long take = nc - done;
          const long long room = kMaxBlocks - a.first[a.nseg];
          if (take > room) take = room;
          Seg& s = a.seg[a.nseg];
          s.p = e.p + done * kChunk;
          s.g = e.g + done * kChunk;
          s.m = e.m ? e.m + done * kChunk : nullptr;
          const long long left = e.n - done * kChunk;
          s.n = left < take * kChunk ? left : take * kChunk;
          s.lr = e.lr;
          s.wd = e.wd;
          a.first[a.nseg + 1] = a.first[a.nseg] + (int)take;
          ++a.nseg;
          done += take;
          if (a.nseg == kMaxSeg || a.first[a.nseg] == kMaxBlocks) {
            launch(a, has_m, part, d_gscale, st);
            a.nseg = 0;
          }
        }
      } else if (a.nseg > 0 && nc > 0) {
        // a tensor of the other kind lies between: its chunks keep their place in the call's order, so this launch ends here
        launch(a, has_m, part, d_gscale, st);
        a.nseg = 0;
      }
      at += nc;
    }
    if (a.nseg > 0) launch(a, has_m, part, d_gscale, st);
  }
  if (d_stats) hipLaunchKernelGGL(sgd_stats_finish_kernel, dim3(1), dim3(kTPB), 0, st, (const double*)part, chunks, d_stats);
  return m3d::check_launch("sgd_step");
}

}  // namespace

M3D_API int m3d_sgd_chunk(void) { return kChunk; }

M3D_API int m3d_sgd_step(const m3d_sgd_tensor* tensors, int count, float momentum, float mscale, double* d_stats, void* d_ws,
                         size_t* ws_bytes, void* stream) {
  return sgd_step(tensors, count, momentum, mscale, nullptr, d_stats, d_ws, ws_bytes, stream);
}

M3D_API int m3d_sgd_step_scaled(const m3d_sgd_tensor* tensors, int count, float momentum, float mscale, const float* d_gscale,
                                double* d_stats, void* d_ws, size_t* ws_bytes, void* stream) {
  return sgd_step(tensors, count, momentum, mscale, d_gscale, d_stats, d_ws, ws_bytes, stream);
}
