// The per-axis sample arithmetic of RoIAlign 3D, shared by roi_align3d.hip (forward, atomic backward) and roi_align3d_bwd.hip (ordered
// backward).  Both files are compiled with -ffp-contract=off: the fp32 operation order below is the contract with oracle/m3d_oracle.c,
// and the table values (lo, hi, l, h, valid) are the same fp32 numbers in every kernel that includes this header.
#ifndef M3D_ROI_ALIGN3D_GEOM_H_
#define M3D_ROI_ALIGN3D_GEOM_H_

#include "m3d_common.h"

namespace {

struct AxisSample {  // one (bin, sub-sample) along one axis
  int lo, hi;        // clamped corner indices
  float l, h;        // weights of hi / lo corners (l = frac, h = 1 - frac)
  int valid;         // 0 => whole sample contributes 0 (coordinate outside [-1, dim])
};

constexpr int kMaxTable = 64;   // A * grid per axis (7 bins * adaptive grid <= 9); larger adaptive grids take roi_untabled_range

__device__ inline AxisSample make_sample(float start, float bin, int p, int i, int grid, int dim, double lo_limit) {
  // coordinate: roi_start + p*bin + (i + .5f)*bin/grid   (roi_align_kernel_3d.cu:130-138)
  float c = start + p * bin;
  c = c + (i + .5f) * bin / grid;
  AxisSample s;
  s.valid = !((double)c < lo_limit || c > dim);  // :19 (forward: -1.0 on every axis; backward: -0.1 on z, :187)
  if (c <= 0) c = 0;                     // :23-31
  int lo = (int)c;
  int hi;
  if (lo >= dim - 1) { hi = lo = dim - 1; c = (float)lo; } else { hi = lo + 1; }   // :40-58
  float l = c - lo;
  float h = (float)(1. - l);             // :63 (double literal)
  s.lo = lo; s.hi = hi; s.l = l; s.h = h;
  return s;
}

struct RoiGeom {
  float start_w, start_h, start_s, bin_w, bin_h, bin_s;
  int grid_w, grid_h, grid_s, batch;
};

__device__ inline RoiGeom roi_geom(const float* r, float scale, int AS, int AH, int AW, int ratio, int B) {
  RoiGeom g;
  g.batch = min(max((int)r[0], 0), B - 1);                              // :94 (clamped: a garbage row must not fault the GPU)
  g.start_w = r[1] * scale; g.start_h = r[2] * scale; g.start_s = r[3] * scale;   // :97-102
  float end_w = r[4] * scale, end_h = r[5] * scale, end_s = r[6] * scale;
  float roi_s = fmaxf(end_s - g.start_s, 1.f);                          // :105-107
  float roi_w = fmaxf(end_w - g.start_w, 1.f);
  float roi_h = fmaxf(end_h - g.start_h, 1.f);
  g.bin_s = roi_s / AS; g.bin_h = roi_h / AH; g.bin_w = roi_w / AW;     // :108-110
  g.grid_s = ratio > 0 ? ratio : (int)ceilf(roi_s / AS);                // :116-123
  g.grid_h = ratio > 0 ? ratio : (int)ceilf(roi_h / AH);
  g.grid_w = ratio > 0 ? ratio : (int)ceilf(roi_w / AW);
  return g;
}

}  // namespace

#endif  // M3D_ROI_ALIGN3D_GEOM_H_
