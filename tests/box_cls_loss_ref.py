"""Test infrastructure: CPU restatement of the second stage's classification-loss modes (FEW_SHOT.SECOND_STAGE_CLS_LOSS) — the
three losses of FastRCNNLossComputation.__call__ this build supports and the score of PostProcessor.forward.  oracle/ restates
'ce_loss' only (oracle/box_train_ref.py, oracle/box_head_ref.py); the restatement with the switch lives here and is pinned to the
REAL reference by tests/golden/make_golden_box_cls_modes.py (fixture tests/golden/box_cls_modes.npz) and tests/test_box_cls_modes.py.

Paths relative to the reference's maskrcnn_benchmark/:
  modeling/roi_heads/box_head/roi_box_predictors.py:47-50,66-68,76-77   cls_score has ONE output unless 'ce_loss' / 'cxe_loss'
  modeling/roi_heads/box_head/loss.py:340-393                           __call__, gt_label == -1
  layers/sigmoid_focal_loss.py:42-54, csrc/cuda/SigmoidFocalLoss_cuda.cu:21-101   the CPU / CUDA focal formulas
  modeling/roi_heads/box_head/inference.py:58-69                        the score

Row layout: L logits, then 8 deltas; L = 2 for 'ce_loss', 1 for 'focal_loss' / 'mse_loss'.  The regression loss reads the class-1
deltas, columns 4..7 of the 8 (loss.py:384-393), in every mode.

Quirk ('mse_loss' without soft labels, loss.py:362-363): `class_logits.sigmoid() - labels.float()` subtracts an [M] tensor from an
[M, 1] one.  Broadcasting makes that an [M, M] matrix, so `torch.mean` runs over M x M (row, label) pairs: every sigmoid is held
against EVERY row's label, i.e. against the mean label.  With s = sigmoid(x), l the labels:
    loss = mean(s^2) - 2 mean(s) mean(l) + mean(l^2),      d loss / d x_i = (2 / M) (s_i - mean(l)) s_i (1 - s_i).
This is what the reference trains on, so it is what is restated (`mse_loss_closed_form` is the algebra, `losses` the broadcast).
"""
import torch
import torch.nn.functional as F

from oracle import hotpath_ref as orc

W_CLS, W_BOX = 5.0, 2.5        # box_head.py:193-194
GAMMA, ALPHA = 2.0, 0.25       # MODEL.FCOS.LOSS_GAMMA, FEW_SHOT.SECOND_STAGE_LOSS_ALPHA (loss.py:40-44)
CLS_LOSSES = ("ce_loss", "focal_loss", "mse_loss")
REFUSED = ("l1_loss", "cxe_loss")


def n_logits(cls_loss):
    if cls_loss not in CLS_LOSSES:
        raise ValueError("cls_loss %r" % (cls_loss,))
    return 2 if cls_loss == "ce_loss" else 1


def box_loss(box_regression, labels, targets):
    """loss.py:379-393: smooth-L1 (beta 1, summed) over the positives' class deltas / labels.numel()."""
    pos = torch.nonzero(labels > 0).squeeze(1)
    cols = 4 * labels[pos][:, None] + torch.tensor([0, 1, 2, 3])
    d = box_regression[pos[:, None], cols] - targets[pos]
    n = d.abs()
    return torch.where(n < 1.0, 0.5 * n ** 2, n - 0.5).sum() / labels.numel()


def mse_loss_closed_form(class_logits, labels):
    """The [M, M]-broadcast mean of loss.py:363 written out (see the module docstring)."""
    s = torch.sigmoid(class_logits.reshape(-1))
    l = labels.to(s.dtype)
    return (s * s).mean() - 2 * s.mean() * l.mean() + (l * l).mean()


def cls_loss_value(class_logits, labels, cls_loss, gamma=GAMMA, alpha=ALPHA, focal="cuda"):
    """The unweighted classification loss.  class_logits [M, L], labels [M] int64 (0 / 1).  focal: "cuda" = the formula the
    reference evaluates on a GPU and the HIP kernel computes, "cpu" = what it evaluates on the CPU (log(p + 1e-6))."""
    if n_logits(cls_loss) != class_logits.shape[1]:
        raise ValueError("%s has %d logit(s) per row, got %d" % (cls_loss, n_logits(cls_loss), class_logits.shape[1]))
    if cls_loss == "ce_loss":
        return F.cross_entropy(class_logits, labels)                                      # loss.py:359
    if cls_loss == "focal_loss":
        fl = orc.sigmoid_focal_loss_cuda_formula if focal == "cuda" else orc.sigmoid_focal_loss_cpu_formula
        n_pos = int((labels > 0).sum())
        return fl(class_logits, labels.int(), gamma, alpha).sum() / max(n_pos, 1)         # loss.py:343-347
    return torch.mean((class_logits.sigmoid() - labels.to(class_logits.dtype)) ** 2)      # loss.py:363: [M,1] - [M] -> [M,M]


def losses(class_logits, box_regression, labels, targets, cls_loss="ce_loss", gamma=GAMMA, alpha=ALPHA, focal="cuda"):
    """loss.py:340-393 with the weights of box_head.py:193-194 -> (5 * classification, 2.5 * box regression)."""
    return (W_CLS * cls_loss_value(class_logits, labels, cls_loss, gamma, alpha, focal),
            W_BOX * box_loss(box_regression, labels, targets))


def scores(class_logits, cls_loss):
    """inference.py:61-69: the class-1 probability, [M]."""
    if n_logits(cls_loss) != class_logits.shape[1]:
        raise ValueError("%s has %d logit(s) per row, got %d" % (cls_loss, n_logits(cls_loss), class_logits.shape[1]))
    if cls_loss == "ce_loss":
        return F.softmax(class_logits, -1)[:, 1]
    return class_logits.sigmoid()[:, 0]


def decode_clip(box_regression, rois, image_size):
    """BoxCoder.decode of the class-1 deltas + clip_to_image (inference.py:79-81,100) -> [M, 4].  image_size: (h, w)."""
    from oracle import box_head_ref as obh
    dec = obh.decode_boxes(box_regression[:, :8], rois)[:, 4:8].clone()
    ih, iw = image_size
    dec[:, 0::2] = dec[:, 0::2].clamp(min=0, max=iw - 1)
    dec[:, 1::2] = dec[:, 1::2].clamp(min=0, max=ih - 1)
    return dec


def postprocess(class_logits, box_regression, proposals, image_sizes, cls_loss, nms_thresh=0.5, cuda_nms=False):
    """inference.py:46-166 in the mode: per image (boxes [K,4], scores [K]) in the reference's order (ascending proposal index).
    obh.box_postprocess restates the 'ce_loss' branch; a one-logit score is its softmax over (0, logit) = sigmoid(logit)."""
    from oracle import box_head_ref as obh
    if cls_loss != "ce_loss":
        n_logits(cls_loss)
        class_logits = torch.cat([torch.zeros_like(class_logits), class_logits], 1)
    return obh.box_postprocess(class_logits, box_regression, proposals, image_sizes, nms_thresh=nms_thresh, cuda_nms=cuda_nms)
