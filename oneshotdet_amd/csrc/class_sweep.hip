// Class sweep (include/oneshotdet_hip.h): K category slots per target image in one pass.  The correlation of
// generalized_rcnn.py:307-311, run K times on the same target pyramid, as one launch that reads each map once per GROUP of
// query vectors instead of once per vector.  HBM-bound: (ceil(K/G) + K) maps of traffic against 2K for the per-pair launches.
// (The sweep's ROI pooling shares its device code with the per-pair kernel and lives next to it in box_head.hip; the walk of this
// kernel is correlate_sweep.h's, which the query gallery's entry in gallery.hip instantiates with another staging.)
#include "correlate_sweep.h"

#define OSD_STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" int osd_class_sweep_group(void) { return kGroup; }

extern "C" int osd_correlate_levels_sweep(int n_levels, const void* const* xs, const float* const* qs, void* const* ys,
                                          const int32_t* hws, int n, int classes, int c, int dtype, void* stream) {
  SweepLevels L;
  long long blocks;
  const int rc = correlate_sweep_plan("correlate_levels_sweep", n_levels, xs, qs, ys, hws, n, classes, c, dtype, &L, &blocks);
  if (rc != OSD_OK || blocks == 0) return rc;
  const int groups = (classes + kGroup - 1) / kGroup;
  const size_t lds = (size_t)kGroup * c * sizeof(float);
  if (dtype == OSD_F32)
    hipLaunchKernelGGL((correlate_sweep_kernel<float, false>), dim3((unsigned)blocks), dim3(256), lds, OSD_STREAM(stream), L, c,
                       classes, groups, (const int32_t*)nullptr, 0);
  else
    hipLaunchKernelGGL((correlate_sweep_kernel<__bf16, false>), dim3((unsigned)blocks), dim3(256), lds, OSD_STREAM(stream), L, c,
                       classes, groups, (const int32_t*)nullptr, 0);
  return osd_check_launch("correlate_levels_sweep");
}
