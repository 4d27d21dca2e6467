// The detection box head as ONE library call (lib/modeling/fast_rcnn_heads.py:104-117,39-47 + lib/core/test.py:225,250-251):
//   RoIAlign3D -> fc1 -> fc2 -> (cls_score | bbox_pred as one GEMM) -> softmax / deltas / decoded + clipped boxes.
// Host code only: it launches, on one stream and with the plans each entry picks for itself, exactly what the per-layer entries launch
// when they are called one after the other - m3d_roi_align3d_forward_ws, m3d_linear_f16x2_forward_bounds (twice), m3d_linear_forward,
// m3d_box_head_outputs - so the results are theirs bit for bit.  What it saves is the host time BETWEEN those launches: the call
// follows the one host read of a detection step (the proposal counts, which size every launch here), and until its first launch is
// queued the GPU has nothing to do.  Every buffer is the caller's: nothing is allocated or queried on the way.
#include "m3d_common.h"

namespace {

struct Dims { int K1, N1, N2, NO; long long vox; };

bool dims_of(const m3d_box_head* d, Dims& o) {
  if (!d || d->channels <= 0 || d->roi_res <= 0 || d->fc1_out <= 0 || d->fc2_out <= 0 || d->num_classes <= 0) return false;
  const long long k1 = (long long)d->channels * d->roi_res * d->roi_res * d->roi_res;
  if (k1 > 0x7FFFFFFF) return false;
  o.K1 = (int)k1; o.N1 = d->fc1_out; o.N2 = d->fc2_out; o.NO = 7 * d->num_classes;
  return true;
}

size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// one workspace serves the stages in turn (they run one after the other on the stream)
size_t stage_bytes(const Dims& s, int R) {
  const size_t ra = m3d::align_up(m3d_roi_align3d_workspace_bytes(R), 256);
  const size_t f1 = m3d_linear_f16x2_workspace_bytes(R, s.N1, s.K1), f2 = m3d_linear_f16x2_workspace_bytes(R, s.N2, s.N1);
  const size_t lo = m3d_linear_workspace_bytes(R, s.NO, s.N2);
  return max3(ra, f1 > f2 ? f1 : f2, lo);
}

}  // namespace

/* bytes of d->ws that serve EVERY num_rois in 1 .. max_rois (a split-K factor, and with it a stage's partials, can shrink as rows are
 * added, so the largest count alone does not bound the smaller ones).  0: unusable description. */
M3D_API size_t m3d_box_head_workspace_bytes(const m3d_box_head* d, int max_rois) {
  Dims s;
  if (!dims_of(d, s) || max_rois <= 0 || s.K1 % 32 != 0 || s.N1 % 32 != 0) return 0;
  size_t best = 0;
  for (int R = 1; R <= max_rois; ++R) {
    const size_t b = stage_bytes(s, R);
    best = b > best ? b : best;
  }
  return best;
}

M3D_API int m3d_box_head_forward(const m3d_box_head* d, void* stream) {
  Dims s;
  if (!dims_of(d, s) || d->num_rois < 0) return M3D_EINVAL;
  const int R = d->num_rois;
  if (R == 0) return M3D_OK;
  if (R <= 32) return M3D_EUNSUPPORTED;                       // a handful of rows runs the fp32-input GEMM: the per-layer entries
  if (!d->fc1_packed || !d->fc2_packed || !d->outs_weight || !d->features || !d->rois || !d->x || !d->h1 || !d->h2 || !d->outs ||
      !d->cls || !d->bbox || !d->pred || !d->ws)
    return M3D_EINVAL;
  if (d->ws_bytes < stage_bytes(s, R)) return M3D_EWORKSPACE;
  const int res = d->roi_res;
  int rc = m3d_roi_align3d_forward_ws(res, res, res, d->spatial_scale, d->sampling_ratio, d->features, d->batch, d->channels, d->slices,
                                      d->height, d->width, d->rois, R, 7, d->x, d->ws, m3d_roi_align3d_workspace_bytes(R), stream);
  if (rc) return rc;
  // fc1's operand bound: the feature maps' (a RoIAlign value is a convex combination of theirs) - from their producer when it left one
  rc = m3d_linear_f16x2_forward_bounds(d->x, d->fc1_packed, d->fc1_bias, d->h1, R, s.N1, s.K1, 1, d->feat_bound, d->feat_bound_slots,
                                       d->fc1_bound, d->ws, d->ws_bytes, stream);
  if (rc) return rc;
  // fc2's: what fc1's storing launch left (else fc2 sweeps its input itself)
  rc = m3d_linear_f16x2_forward_bounds(d->h1, d->fc2_packed, d->fc2_bias, d->h2, R, s.N2, s.N1, 1, d->fc1_bound,
                                       m3d_conv3d_zw_slots(), nullptr, d->ws, d->ws_bytes, stream);
  if (rc) return rc;
  rc = m3d_linear_forward(d->h2, d->outs_weight, d->outs_bias, d->outs, R, s.NO, s.N2, 0, d->ws, d->ws_bytes, stream);
  if (rc) return rc;
  return m3d_box_head_outputs(d->outs, d->rois, R, d->num_classes, d->weights, d->xform_clip, d->clip[0], d->clip[1], d->clip[2], d->cls,
                              d->bbox, d->pred, stream);
}
