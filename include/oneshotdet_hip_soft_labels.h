/*
 * oneshotdet_hip_soft_labels.h — C-ABI of liboneshotdet_hip.so, third part: the second stage's IoU soft labels
 * (FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC, config/defaults.py) and the three classification losses that read them.  Same
 * conventions as oneshotdet_hip.h (raw device pointers, caller-allocated outputs, asynchronous on `stream`, 0 = OK / negative =
 * OSD_ERR_*); paths relative to the reference's maskrcnn_benchmark/.  The ABI version is unchanged.
 *
 * Soft label of a proposal (modeling/roi_heads/box_head/loss.py:52-62,81-104,118-120): t = its IoU with the matched ground truth,
 * 0 where the matcher returned a negative index (background), then soft = f(t) by SOFT_LABELING_FUNC, float32 in the reference's
 * operation order; the comparisons are against the float32 values of 0.5 and 0.1:
 *   OSD_SOFT_LABEL_DISCRETE          (t >= 0.5) as 0 / 1
 *   OSD_SOFT_LABEL_LINEAR            t                                                     (the reference's default)
 *   OSD_SOFT_LABEL_TRANS_LINEAR      (0.2 t + 0.8) [t >= 0.5] + (2.25 t - 0.225) [t >= 0.1] [t < 0.5]
 *   OSD_SOFT_LABEL_TRANS_4TH_LINEAR  (0.2 t + 0.8) [t >= 0.5] + 0.9 (2 t)^4 [t < 0.5]
 * The soft label travels with the proposal through the sampler (loss.py:260-287): one fp32 value per sampled row, in the sampled
 * rows' order.
 *
 * Row layout of the predictor (modeling/roi_heads/box_head/roi_box_predictors.py:63-68,76-77): L class logits followed by the
 * 2 x 4 box deltas of bbox_pred; L = 2 for 'cxe_loss', L = 1 for 'mse_loss' and 'l1_loss' (bbox_pred keeps its 8 columns).
 */
#ifndef ONESHOTDET_HIP_SOFT_LABELS_H
#define ONESHOTDET_HIP_SOFT_LABELS_H

#include "oneshotdet_hip_box_modes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSD_SOFT_LABEL_DISCRETE 0
#define OSD_SOFT_LABEL_LINEAR 1
#define OSD_SOFT_LABEL_TRANS_LINEAR 2
#define OSD_SOFT_LABEL_TRANS_4TH_LINEAR 3

/* OSD_BOX_CLS_MSE (2, oneshotdet_hip_box_modes.h) means its soft-label variant here */
#define OSD_BOX_CLS_L1 3  /* 'l1_loss':  L = 1, |sigmoid - soft label| / sigmoid score (decode: OSD_BOX_CLS_MSE) */
#define OSD_BOX_CLS_CXE 4 /* 'cxe_loss': L = 2, soft cross-entropy of the softmax / softmax score (decode: OSD_BOX_CLS_CE) */

/* FastRCNNLossComputation.subsample with FEW_SHOT.SOFT_LABELING (loss.py:234-292).  osd_box_match_sample's arguments and outputs,
 * bit for bit, plus: soft_func (OSD_SOFT_LABEL_*, anything else is OSD_ERR_INVALID_ARG), s_soft [n][batch_per_image] fp32 (required):
 * f(best IoU) for the sampled rows with label >= 1, 0 for background rows and for rows past s_count[image]; all_soft (nullable)
 * [n][max_props] fp32: the same per proposal, 0 past counts[image].  One workgroup per image. */
int osd_box_match_sample_soft(const float* boxes, const int32_t* counts, const float* gt_boxes, const int32_t* gt_count,
                              const int32_t* gt_labels, const float* keys, int n, int max_props, int max_gt, int batch_per_image,
                              float positive_fraction, float iou_thresh, const float* reg_weights, float* s_boxes, int32_t* s_labels,
                              float* s_targets, int32_t* s_index, int32_t* s_count, int32_t* all_labels, int32_t* all_matched,
                              int soft_func, float* s_soft, float* all_soft, void* stream);

/* FastRCNNLossComputation.__call__ with FEW_SHOT.SOFT_LABELING (loss.py:333-334,360-367, gt_label == -1), the weights of
 * box_head.py:193-194 folded in.  osd_box_loss's arguments plus soft [n*rois_per_image] fp32 (the rows' soft labels t; required) and
 * cls_loss; OSD_ERR_INVALID_ARG for OSD_BOX_CLS_CE / OSD_BOX_CLS_FOCAL (they never read soft labels: osd_box_loss_opt), an unknown
 * mode, a null soft, or pred_stride (grad_stride, when d_pred is given) below L + 8.  M = the valid rows (the first
 * min(s_count[image], rois_per_image) of every image), s = sigmoid(logit).  losses[3] = {w_cls * classification, w_box * box, M}:
 *   OSD_BOX_CLS_MSE  loss.py:361: sigmoid [M][1] minus soft [M] broadcasts to [M][M]; the mean over the M x M pairs is
 *                    mean_i (s_i - mt)^2 + mean_j (t_j - mt)^2 with mt = mean(t) (reduced first; both sums are of non-negative terms);
 *                    d/dx_i = (2 / M) (s_i - mt) s_i (1 - s_i).
 *   OSD_BOX_CLS_L1   loss.py:365: the same broadcast, (1 / M^2) sum_i sum_j |s_i - t_j|: no closed form, the kernel walks the M x M
 *                    pairs (soft labels staged through LDS in tiles of 1,024 rows); d/dx_i = (1 / M^2) s_i (1 - s_i) sum_j sign(s_i - t_j),
 *                    sign(0) = 0, the sum kept as an integer.
 *   OSD_BOX_CLS_CXE  loss.py:294-296,367: -mean([1 - t, t] * log softmax(logits)) over the [M][2] tensor: the mean runs over 2M
 *                    elements, HALF the soft cross-entropy; d/dx = (softmax - [1 - t, t]) / (2M).  Stable log-softmax.
 *   box regression   as osd_box_loss, by the hard labels (loss.py:379-393).
 * Rows past s_count[image] contribute nothing, neither as i nor as t_j, and their gradient rows are zero.  A label > 1 has no columns
 * in the row: losses[0..1] come back NaN.  One workgroup, fixed summation order, no floating-point atomics. */
int osd_box_loss_soft(const void* pred, const int32_t* labels, const float* targets, const int32_t* s_count, int n,
                      int rois_per_image, int pred_stride, float w_cls, float w_box, float* losses, void* d_pred, int grad_stride,
                      int dtype, const float* soft, int cls_loss, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_SOFT_LABELS_H */
