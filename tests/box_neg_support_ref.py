"""Test infrastructure: CPU restatement of the second stage's negative support (FEW_SHOT.NEG_SUPPORT.TURN_ON with
SECOND_STAGE_METHOD 'concat' and SECOND_STAGE_CLS_LOSS 'ce_loss').  Pinned to the REAL reference by
tests/golden/make_golden_box_neg_support.py (fixtures tests/golden/box_neg_support.npz, tests/golden/boxtrain_small_neg.npz) and
tests/test_box_neg_support.py.

Paths relative to the reference's maskrcnn_benchmark/:
  modeling/roi_heads/box_head/box_head.py:128-139,156-161,180-188   the head run twice with the same weights; the weights 5 / 2.5 / 2.5
  modeling/roi_heads/box_head/loss.py:435-444                       the margin loss over the rows with labels == 1

With p = softmax(class_logits)[:, 1] and q = softmax(neg_class_logits)[:, 1] of the K rows with label 1,
    suppress = mean(relu(q - p + 0.3)),
    d suppress / d class_logits[r]     = (1 / K) [q_r - p_r + 0.3 > 0] p_r (1 - p_r) * (+1, -1),
    d suppress / d neg_class_logits[r] = (1 / K) [q_r - p_r + 0.3 > 0] q_r (1 - q_r) * (-1, +1),
since d softmax(x)[1] / d x = s1 (1 - s1) * (-1, +1).  K == 0: the reference's mean of an empty tensor is NaN; the kernel's
documented answer is 0 with zero gradients (include/oneshotdet_hip.h), and `suppress_loss(..., empty="zero")` says so.
"""
import torch
import torch.nn.functional as F

import box_cls_loss_ref as bcl

W_CLS, W_BOX = bcl.W_CLS, bcl.W_BOX
W_SUPPRESS, MARGIN = 2.5, 0.3      # box_head.py:188, loss.py:442


def suppress_loss(class_logits, neg_class_logits, labels, margin=MARGIN, empty="nan"):
    """loss.py:435-444, unweighted.  empty: what K == 0 gives, "nan" (the reference) or "zero" (the kernel)."""
    fg = labels == 1
    if empty == "zero" and not bool(fg.any()):
        return class_logits.new_zeros(())
    q = neg_class_logits[fg].softmax(dim=1)[:, 1]
    p = class_logits[fg].softmax(dim=1)[:, 1]
    return F.relu(q - p + margin).mean()


def suppress_active(class_logits, neg_class_logits, labels, margin=MARGIN):
    """[M] bool: the rows whose hinge is active (label 1 and q - p + margin > 0)."""
    p, q = class_logits.softmax(dim=1)[:, 1], neg_class_logits.softmax(dim=1)[:, 1]
    return (labels == 1) & (q - p + margin > 0)


def suppress_grads(class_logits, neg_class_logits, labels, margin=MARGIN):
    """The closed-form gradient of the unweighted loss w.r.t. both logit sets ([M, 2] each), in the inputs' dtype; zeros for K == 0."""
    p, q = class_logits.softmax(dim=1)[:, 1], neg_class_logits.softmax(dim=1)[:, 1]
    k = int((labels == 1).sum())
    act = suppress_active(class_logits, neg_class_logits, labels, margin).to(p.dtype) / max(k, 1)
    sign = torch.tensor([1.0, -1.0], dtype=p.dtype)
    g_pos = (act * p * (1 - p))[:, None] * sign
    g_neg = (act * q * (1 - q))[:, None] * (-sign)
    return g_pos, g_neg


def losses(class_logits, neg_class_logits, box_regression, labels, targets, margin=MARGIN, w_suppress=W_SUPPRESS, empty="nan"):
    """box_head.py:180-188 -> (5 * cross-entropy, 2.5 * box regression, 2.5 * suppress)."""
    lc, lb = bcl.losses(class_logits, box_regression, labels, targets, "ce_loss")
    return lc, lb, w_suppress * suppress_loss(class_logits, neg_class_logits, labels, margin, empty)


def two_branch_logits(feats, qfeats, neg_qfeats, boxes, q_sizes, neg_q_sizes, sd):
    """box_head.py:128-139,156-161: the head on the same sampled ROIs against the support and against the negative support, as two
    calls of oracle.box_head_ref.box_head_logits with the same weights -> (class_logits, box_regression, neg_class_logits); the
    negative branch's box regression is unused in the reference."""
    from oracle import box_head_ref as obh
    logits, reg, _ = obh.box_head_logits(feats, qfeats, boxes, q_sizes, sd)
    neg_logits, _, _ = obh.box_head_logits(feats, neg_qfeats, boxes, neg_q_sizes, sd)
    return logits, reg, neg_logits
