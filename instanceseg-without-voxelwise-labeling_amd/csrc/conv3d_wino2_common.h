// What the 2-D Winograd kernel files share (conv3d_wino2.hip: the F(2x2,3x3) kernel and the entry points of both families;
// conv3d_wino24.hip: the F(2x4,3x3) kernels): the slot index of the F(2x2) weight pack and the epilogue every kernel takes by value.
#pragma once
#include "m3d_common.h"

namespace m3d_w2 {

// element index inside one (channel pair, cout block) segment of the packed weights: [dz*4 + eta][lane64][xi] (conv3d_wino2.hip)
__device__ __host__ __forceinline__ constexpr int w2_slot(int dz, int eta, int xi, int lane) { return ((dz * 4 + eta) * 64 + lane) * 4 + xi; }

struct Epi {
  const float* scale;
  const float* shift;
  int relu;
  int xcd_map;
  // split-K over workgroups (small maps: too few output blocks to fill the chip): blockIdx.z = slice; slice s handles 4-channel chunks
  // [s*cps, (s+1)*cps) and writes its un-scaled partial result to out + s*slice_stride (ksplit <= 1: no split)
  int ksplit, cps;
  size_t slice_stride;
  unsigned char* argmax;   // fused pool + arg-max (kernels instantiated with AM): index 0..7 = (dz, dy, dx) of each pooled value's first maximum
#ifdef M3D_W2_STAMPS
  unsigned long long* stamps;
#endif
};

}  // namespace m3d_w2
