/*
 * oneshotdet_hip_neg_support.h — C-ABI of liboneshotdet_hip.so, fourth part: the second stage's negative support
 * (FEW_SHOT.NEG_SUPPORT.TURN_ON with SECOND_STAGE_METHOD 'concat' and SECOND_STAGE_CLS_LOSS 'ce_loss', config/defaults.py).  Same
 * conventions as oneshotdet_hip.h (raw device pointers, caller-allocated outputs, asynchronous on `stream`, 0 = OK / negative =
 * OSD_ERR_*); paths relative to the reference's maskrcnn_benchmark/.  The ABI version is unchanged.
 *
 * The box head scores the sampled ROIs twice with the same weights (modeling/roi_heads/box_head/box_head.py:128-139): against the
 * support crop of the queried category (pred) and against a crop of another category (pred_neg).  Both are rows of 2 class logits
 * followed by the 2 x 4 box deltas; the deltas of pred_neg are never read (box_head.py: neg_box_regression is unused).
 */
#ifndef ONESHOTDET_HIP_NEG_SUPPORT_H
#define ONESHOTDET_HIP_NEG_SUPPORT_H

#include "oneshotdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* FastRCNNLossComputation.__call__ with a negative support (loss.py:359,379-393,435-444, gt_label == -1), the weights of
 * box_head.py:180-188 folded in.  osd_box_loss's arguments, with the same meaning, plus pred_neg [n*rois_per_image][pred_stride] (the
 * dtype of pred; required), d_pred_neg [n*rois_per_image][grad_stride] (given exactly when d_pred is), margin (0.3 in the reference)
 * and w_suppress (2.5).  OSD_ERR_INVALID_ARG for a null pred_neg, for one of d_pred / d_pred_neg without the other, or for
 * pred_stride (grad_stride, when the gradients are given) below 2 + 8.
 *   losses[5] = {w_cls * cross-entropy, w_box * smooth-L1, M, w_suppress * suppress, K}
 * M = the valid rows (the first min(s_count[image], rois_per_image) of every image), K = the valid rows with label 1, and
 *   suppress = (1 / K) sum over those K rows of relu(q - p + margin),  p = softmax(pred row)[1], q = softmax(pred_neg row)[1].
 * Gradients: d_pred[r][0:2] = the cross-entropy's plus the hinge's, (w_suppress / K) p (1 - p) * (+1, -1) where q - p + margin > 0;
 * d_pred[r][2:10] as osd_box_loss; d_pred_neg[r][0:2] = (w_suppress / K) q (1 - q) * (-1, +1) where the hinge is active.  Every other
 * element of the grad_stride columns of d_pred_neg is written 0: the delta columns, and the whole row where it is past
 * s_count[image], background, or has q - p + margin <= 0.  With d_pred == NULL only the losses are computed.
 * K == 0: suppress = 0 and no hinge gradient.  (The reference takes the mean of an empty tensor, NaN, there; its matcher and the
 * appended ground-truth proposals keep a real step from reaching that state.  Zero is this kernel's documented answer.)
 * Rows past s_count[image] are never read.  A label > 1 has no columns in the row: losses[0], [1] and [3] come back NaN.  With
 * w_suppress == 0 losses[0..2] and d_pred are osd_box_loss's bit for bit.  One workgroup, any M, fixed summation order, no
 * floating-point atomics. */
int osd_box_loss_neg_support(const void* pred, const void* pred_neg, const int32_t* labels, const float* targets,
                             const int32_t* s_count, int n, int rois_per_image, int pred_stride, float w_cls, float w_box,
                             float margin, float w_suppress, float* losses, void* d_pred, void* d_pred_neg, int grad_stride,
                             int dtype, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_NEG_SUPPORT_H */
