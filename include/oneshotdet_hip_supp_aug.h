/*
 * oneshotdet_hip_supp_aug.h — C-ABI of liboneshotdet_hip.so, fourth part: query augmentation groups (FEW_SHOT.SUPP_AUG /
 * NUM_SUPP_AUG / SUPP_AUG_METHOD 'avg' and 'max', config/defaults.py).  Same conventions as oneshotdet_hip.h (raw device pointers,
 * caller-allocated outputs, asynchronous on `stream`, 0 = OK / negative = OSD_ERR_*); paths relative to the reference's
 * maskrcnn_benchmark/.  The ABI version is unchanged.
 *
 * The query batch holds groups of A = NUM_SUPP_AUG + 1 consecutive rows: a support crop followed by its augmentations.  The query
 * backbone runs on all rows; every FPN level is then split into groups of A maps and each group merged into ONE map before any
 * pooling (modeling/detector/generalized_rcnn.py:235-294).  Maps are NHWC; group g of x is rows g*A .. g*A + A - 1
 * (feat.split(A, dim=0)).
 *
 * Both entries take up to 8 levels and make one launch for all of them: 16-byte vector loads and stores, no atomics, no workspace,
 * no memset.  Every output element is written exactly once, and a group's result does not depend on the other groups.
 *
 * Argument checks, in this order and before anything is launched: a null array, aug < 2, aug > 8, n_levels outside 1..8, an unknown
 * dtype or method, groups < 0 or c < 1: OSD_ERR_INVALID_ARG; c no multiple of one 16-byte group (4 fp32 / 8 bf16):
 * OSD_ERR_UNSUPPORTED; groups == 0: a no-op that returns 0 (the level pointers are not looked at); per level a null pointer or
 * hw[l] < 1: OSD_ERR_INVALID_ARG, a pointer that is not 16-byte aligned or a level of 2^31 elements or more: OSD_ERR_UNSUPPORTED.
 */
#ifndef ONESHOTDET_HIP_SUPP_AUG_H
#define ONESHOTDET_HIP_SUPP_AUG_H

#include "oneshotdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSD_SUPP_AUG_AVG 0 /* 'avg': the mean over the group */
#define OSD_SUPP_AUG_MAX 1 /* 'max': the element-wise maximum over the group */

/* The merge of generalized_rcnn.py:280-288: x[l] [groups*aug, h_l, w_l, c] -> y[l] [groups, h_l, w_l, c], both `dtype`;
 * hw[l] = h_l * w_l.  OSD_SUPP_AUG_AVG: the members are added in member order in fp32 (starting from member 0), the sum is divided
 * by aug (a true division, no reciprocal) and rounded once to `dtype`.  OSD_SUPP_AUG_MAX: the exact maximum. */
int osd_supp_aug_reduce_levels(int n_levels, const void* const* x, void* const* y, const int32_t* hw, int groups, int aug, int c,
                               int dtype, int method, void* stream);

/* Backward of the merge of generalized_rcnn.py:280-288: dy[l] [groups, h_l, w_l, c] -> dx[l] [groups*aug, h_l, w_l, c]; x[l] is the
 * forward's input.  x, dy and dx are all `dtype`, the engine's activation dtype: the gradient of the merged maps is accumulated in
 * that dtype by the pooling backward and the second stage.  Every element of dx is written.  OSD_SUPP_AUG_AVG: every member gets
 * dy / aug (computed in fp32, rounded once; x is not read).  OSD_SUPP_AUG_MAX: the whole dy goes to the LOWEST member index that
 * attains the group's maximum, the other members get 0 (what torch.max(dim=1)'s backward does on the CPU); the argmax is recomputed
 * from x, no index plane is stored. */
int osd_supp_aug_reduce_levels_bwd(int n_levels, const void* const* x, const void* const* dy, void* const* dx, const int32_t* hw,
                                   int groups, int aug, int c, int dtype, int method, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_SUPP_AUG_H */
