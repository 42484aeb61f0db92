/*
 * oneshotdet_hip_gallery.h — C-ABI of liboneshotdet_hip.so, seventh part: the query gallery.  The supports of G gallery slots are
 * enrolled once (pooled query vectors, query halves of the box head's first conv); every later call detects its images against
 * rows of that bank, picked per (image, category slot) by a table of slot numbers in device memory.  The two places where the
 * enrolled data enters the per-(image, category) work read it THROUGH the table, so nothing is gathered, copied or recomputed per
 * call.  Same conventions as oneshotdet_hip.h (raw device pointers, asynchronous on `stream`, 0 = OK / negative = OSD_ERR_*);
 * paths relative to the reference's maskrcnn_benchmark/.  The ABI version is unchanged.
 */
#ifndef ONESHOTDET_HIP_GALLERY_H
#define ONESHOTDET_HIP_GALLERY_H

#include "oneshotdet_hip_class_sweep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* modeling/detector/generalized_rcnn.py:307-311 for `classes` category slots per image, the query vectors taken from a gallery:
 *   xs[l] [n][hw_l][c] (dtype), qs[l] [n_gallery][c] fp32, slots [n*classes] int32 (device), ys[l] [n*classes][hw_l][c] (dtype),
 *   ys[l][b*classes + k] = xs[l][b] * qs[l][slots[b*classes + k]]   (broadcast over the pixels)
 * osd_correlate_levels_sweep's walk (OSD_CLASS_SWEEP_GROUP vectors staged per workgroup, each 16-byte chunk of x loaded once, one
 * store per staged vector, the same level table) with the staged vectors read through `slots`: the same bits as that entry on
 * the gathered vectors qs[l][slots].  Slots may repeat and come in any order.  A slot outside [0, n_gallery) is never used as an
 * address: its output row is NaN (the callers validate the table on the host; this is the device's own guard).  Levels with
 * hws[l] <= 0 are skipped.  Channel rule as osd_correlate_levels.  OSD_ERR_INVALID_ARG for null arrays, tensors or slots, n < 0,
 * classes < 1, n_gallery < 1, a bad channel count or dtype; nothing is launched then.  n == 0 is a no-op. */
int osd_correlate_levels_gallery(int n_levels, const void* const* xs, const float* const* qs, const int32_t* slots, void* const* ys,
                                 const int32_t* hws, int n, int classes, int n_gallery, int c, int dtype, void* stream);

/* modeling/roi_heads/box_head/box_head.py:43-66,146-148: osd_groupnorm_act_rois with the addend row of sample i taken through a
 * table, addend [n_add][hw][c] (dtype), add_index [ceil(n_samples / rois_per_add)] int32 (device):
 *   row(i) = add_index[i / rois_per_add] * add_stride + add_offset
 * (add_stride = shots of a gallery slot, add_offset = the shot).  The same device code as that entry, so the same bits as that
 * entry on the gathered addend.  A row outside [0, n_add) is never used as an address: the sample's output is NaN.  Shapes as
 * osd_groupnorm_act_rois, and at most 65535 ROI sets: the launch is a 2-D grid (ROI within its set, set), so a workgroup finds its
 * table entry without a division (OSD_ERR_UNSUPPORTED otherwise).  OSD_ERR_INVALID_ARG for a null x, addend, add_index, gamma, beta or y,
 * n_samples < 0, rois_per_add < 1, add_stride < 1, add_offset < 0, n_add < 1 or a bad dtype; nothing is launched then.
 * n_samples == 0 is a no-op. */
int osd_groupnorm_act_rois_gallery(const void* x, const void* addend, const int32_t* add_index, const float* gamma, const float* beta,
                                   void* y, int n_samples, int hw, int c, int groups, float eps, float slope, int rois_per_add,
                                   int add_stride, int add_offset, int n_add, int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_GALLERY_H */
