// Query gallery (include/oneshotdet_hip.h): the supports of G gallery slots are enrolled once, and a call detects its images
// against rows of that bank picked by a slot table in device memory.  Two kernels read the enrolled data through the table:
//   * the class sweep's correlation walk (correlate_sweep.h) with the staged query vectors taken as q[slots[row]]
//   * the box head's GroupNorm + LeakyReLU (gn_act_rois.h) with the addend map taken as addend[add_index[set] * stride + offset]
// Both are the existing device code with another way to find a row, so both give the existing entries' bits on gathered operands,
// and neither gathers: the table costs one scalar load per staged vector / per workgroup.
// Compiler's resource report (gfx950, -O3): correlate_sweep_kernel<__bf16, true> 90 VGPRs = 5 waves per SIMD, <float, true> 52 VGPRs =
// 8 waves per SIMD (the sweep's own instantiations: 136 = 3 and 98 = 4), no scratch, no static LDS, dynamic LDS G * 4c bytes = 8 KiB
// at c = 256 (of a CU's 160 KiB: never the limit); gn_act_rois_kernel<__bf16, 49, true> and <float, 49, true> 122 VGPRs = 4 waves per
// SIMD (the plain instantiations: 127 and 122, 4 waves), no LDS, no scratch.  The `false` instantiations are instruction for instruction what
// the two kernels compiled to before they took the template parameter (their trailing arguments are never read).
#include "correlate_sweep.h"
#include "gn_act_rois.h"

#define OSD_STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" int osd_correlate_levels_gallery(int n_levels, const void* const* xs, const float* const* qs, const int32_t* slots,
                                            void* const* ys, const int32_t* hws, int n, int classes, int n_gallery, int c, int dtype,
                                            void* stream) {
  if (!slots) return osd_fail(OSD_ERR_INVALID_ARG, "correlate_levels_gallery: null slot table");
  if (n_gallery < 1) return osd_fail(OSD_ERR_INVALID_ARG, "correlate_levels_gallery: a gallery of %d slots", n_gallery);
  SweepLevels L;
  long long blocks;
  const int rc = correlate_sweep_plan("correlate_levels_gallery", n_levels, xs, qs, ys, hws, n, classes, c, dtype, &L, &blocks);
  if (rc != OSD_OK || blocks == 0) return rc;
  const int groups = (classes + kGroup - 1) / kGroup;
  const size_t lds = (size_t)kGroup * c * sizeof(float);
  if (dtype == OSD_F32)
    hipLaunchKernelGGL((correlate_sweep_kernel<float, true>), dim3((unsigned)blocks), dim3(256), lds, OSD_STREAM(stream), L, c,
                       classes, groups, slots, n_gallery);
  else
    hipLaunchKernelGGL((correlate_sweep_kernel<__bf16, true>), dim3((unsigned)blocks), dim3(256), lds, OSD_STREAM(stream), L, c,
                       classes, groups, slots, n_gallery);
  return osd_check_launch("correlate_levels_gallery");
}

extern "C" int osd_groupnorm_act_rois_gallery(const void* x, const void* addend, const int32_t* add_index, const float* gamma,
                                              const float* beta, void* y, int n_samples, int hw, int c, int groups, float eps,
                                              float slope, int rois_per_add, int add_stride, int add_offset, int n_add, int dtype,
                                              void* stream) {
  if (!x || !addend || !add_index || !gamma || !beta || !y)
    return osd_fail(OSD_ERR_INVALID_ARG, "groupnorm_act_rois_gallery: null argument");
  if (n_samples < 0 || rois_per_add < 1 || add_stride < 1 || add_offset < 0 || n_add < 1)
    return osd_fail(OSD_ERR_INVALID_ARG, "groupnorm_act_rois_gallery: n_samples %d, rois_per_add %d, add_stride %d, add_offset %d, "
                    "n_add %d", n_samples, rois_per_add, add_stride, add_offset, n_add);
  if (dtype != OSD_F32 && dtype != OSD_BF16) return osd_fail(OSD_ERR_INVALID_ARG, "groupnorm_act_rois_gallery: bad dtype %d", dtype);
  if (const int rc = gn_act_rois_shape("groupnorm_act_rois_gallery", hw, c, groups)) return rc;
  if (n_samples == 0) return OSD_OK;
  // a 2-D grid (ROI within its set, set): the kernel finds its table entry without a division
  const int n_sets = (n_samples + rois_per_add - 1) / rois_per_add;
  if (n_sets > 65535) return osd_fail(OSD_ERR_UNSUPPORTED, "groupnorm_act_rois_gallery: %d ROI sets (at most 65535)", n_sets);
  const dim3 grid(n_samples < rois_per_add ? n_samples : rois_per_add, n_sets);
  if (dtype == OSD_F32)
    hipLaunchKernelGGL((gn_act_rois_kernel<float, 49, true>), grid, dim3(c / 2), 0, OSD_STREAM(stream), (const float*)x,
                       (const float*)addend, gamma, beta, (float*)y, c, groups, eps, slope, rois_per_add, add_stride, add_offset,
                       add_index, n_add, n_samples);
  else
    hipLaunchKernelGGL((gn_act_rois_kernel<__bf16, 49, true>), grid, dim3(c / 2), 0, OSD_STREAM(stream),
                       (const __bf16*)x, (const __bf16*)addend, gamma, beta, (__bf16*)y, c, groups, eps, slope, rois_per_add,
                       add_stride, add_offset, add_index, n_add, n_samples);
  return osd_check_launch("groupnorm_act_rois_gallery");
}
