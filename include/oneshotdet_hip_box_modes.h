/*
 * oneshotdet_hip_box_modes.h — C-ABI of liboneshotdet_hip.so, second part: the second stage's classification-loss modes
 * (FEW_SHOT.SECOND_STAGE_CLS_LOSS, config/defaults.py:511).  Same conventions as oneshotdet_hip.h (raw device pointers, caller-
 * allocated outputs, asynchronous on `stream`, 0 = OK / negative = OSD_ERR_*); paths relative to the reference's maskrcnn_benchmark/.
 * The entries of oneshotdet_hip.h (osd_box_loss, osd_box_decode) are these with OSD_BOX_CLS_CE; the ABI version is unchanged.
 *
 * Row layout of the predictor (modeling/roi_heads/box_head/roi_box_predictors.py:47-50,66-68,76-77,88-99): L class logits
 * followed by the 2 x 4 box deltas of bbox_pred.  L = 2 for 'ce_loss', L = 1 for 'focal_loss' and 'mse_loss' (cls_score has ONE
 * output there; bbox_pred keeps 8).  The class-l deltas are columns L + 4l .. L + 4l + 3; the regression loss and the decode use
 * class 1, i.e. columns 4..7 of the 8 (loss.py:384-393, inference.py:144).
 */
#ifndef ONESHOTDET_HIP_BOX_MODES_H
#define ONESHOTDET_HIP_BOX_MODES_H

#include "oneshotdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSD_BOX_CLS_CE 0    /* 'ce_loss':    L = 2, softmax cross-entropy / softmax score: exactly osd_box_loss / osd_box_decode */
#define OSD_BOX_CLS_FOCAL 1 /* 'focal_loss': L = 1, sigmoid focal loss / sigmoid score */
#define OSD_BOX_CLS_MSE 2   /* 'mse_loss':   L = 1, squared error of the sigmoid (no soft labels) / sigmoid score */

/* FastRCNNLossComputation.__call__ (modeling/roi_heads/box_head/loss.py:306-393, gt_label == -1) in the mode `cls_loss`, with the
 * weights of box_head.py:193-194 folded in.  Arguments as osd_box_loss; pred [n*rois_per_image][pred_stride] `dtype` in the row
 * layout above, pred_stride >= L + 8 (and grad_stride >= L + 8 when d_pred is given), else OSD_ERR_INVALID_ARG; an unknown
 * cls_loss is OSD_ERR_INVALID_ARG too.  M = the valid rows (the first min(s_count[image], rois_per_image) of every image),
 * n_pos = the valid rows with label > 0.  losses[3] = {w_cls * classification, w_box * box regression, M}:
 *   OSD_BOX_CLS_CE     cross-entropy over the 2 logits, mean over the M rows (loss.py:359); gamma / alpha unused.
 *   OSD_BOX_CLS_FOCAL  sigmoid focal loss over the [M][1] logits (layers/sigmoid_focal_loss.py, the CUDA formula with a stable
 *                      log-sigmoid, csrc/cuda/SigmoidFocalLoss_cuda.cu:21-101; gamma = MODEL.FCOS.LOSS_GAMMA, alpha =
 *                      FEW_SHOT.SECOND_STAGE_LOSS_ALPHA), SUMMED and divided by max(n_pos, 1) (loss.py:343-347).
 *   OSD_BOX_CLS_MSE    loss.py:362-363 as the reference evaluates it: sigmoid(logits) [M][1] minus labels.float() [M] broadcasts to
 *                      [M][M], so the mean runs over M x M pairs, not over M rows: with s = sigmoid(x), ml = n_pos / M it is
 *                      mean(s^2) - 2 mean(s) ml + ml = mean((s - ml)^2) + ml (1 - ml)  (labels are 0 / 1), and
 *                      d/dx_i = (2 / M) (s_i - ml) s_i (1 - s_i).  gamma / alpha unused.
 *   box regression     in every mode: smooth-L1 (beta 1) over the positives' class-1 deltas, summed, divided by M (loss.py:387-393).
 * d_pred (nullable) [..][grad_stride] `dtype`: the gradient w.r.t. pred; rows past s_count[image] and every column the loss does
 * not read are zero.  Labels are 0 or 1: a label > 1 has no columns in the row, nothing is read for it and losses[0..1] come back
 * NaN.  One workgroup, fixed summation order (n_pos is counted in a pass of its own before any gradient is written). */
int osd_box_loss_opt(const void* pred, const int32_t* labels, const float* targets, const int32_t* s_count, int n,
                     int rois_per_image, int pred_stride, float w_cls, float w_box, float* losses, void* d_pred, int grad_stride,
                     int dtype, int cls_loss, float gamma, float alpha, void* stream);

/* PostProcessor.forward (modeling/roi_heads/box_head/inference.py:46-103) in the mode `cls_loss`.  Arguments as osd_box_decode;
 * pred [shots][n*max_rois][pred_stride] `dtype` in the row layout above, pred_stride >= L + 8, else OSD_ERR_INVALID_ARG; an
 * unknown cls_loss is OSD_ERR_INVALID_ARG.  The score is softmax(logits)[1] for OSD_BOX_CLS_CE (inference.py:65-66) and
 * sigmoid(logit) for OSD_BOX_CLS_FOCAL / OSD_BOX_CLS_MSE (inference.py:61-64,67-69); decode of the class-1 deltas, clip and
 * threshold as osd_box_decode.  logits_out (optional) is [n*max_rois][L], reg_out [n*max_rois][8].  The reference's arg-max over
 * shots (box_head.py:246-253) fails for shots > 1 in the one-logit modes (a 4-column index into 8 regression columns): the
 * kernel takes each of the 8 deltas from the shot with the largest logit there; the Python layer refuses shots > 1 before it. */
int osd_box_decode_opt(const void* pred, const float* rois, const int32_t* counts, float* scores, float* boxes,
                       float* logits_out, float* reg_out, int n, int max_rois, int shots, int pred_stride,
                       const float* reg_weights, float img_h, float img_w, const float* img_hw, float score_thresh, int dtype,
                       int cls_loss, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_BOX_MODES_H */
