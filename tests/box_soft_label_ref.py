"""Test infrastructure: CPU restatement of the second stage's IoU soft labels (FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC) and of the
three classification losses that read them, written as the reference writes them (the broadcasts are left in place), next to the
closed forms the HIP kernel computes.  Pinned to the REAL reference by tests/golden/make_golden_box_soft_labels.py (fixture
tests/golden/box_soft_labels.npz) and tests/test_box_soft_labels.py.

Paths relative to the reference's maskrcnn_benchmark/:
  modeling/roi_heads/box_head/loss.py:52-62      match_iou = the IoU with the matched ground truth, 0 where the matcher's index is negative
  modeling/roi_heads/box_head/loss.py:81-104     soft_labeling_function: 'discrete', 'linear', 'transLinear', 'trans4thLinear'
  modeling/roi_heads/box_head/loss.py:260-287    the soft labels travel through the sampler with the proposals
  modeling/roi_heads/box_head/loss.py:294-296    CXE: -(stack([1 - t, t], 1) * log(p)).mean()
  modeling/roi_heads/box_head/loss.py:360-367    'mse_loss' / 'l1_loss' / 'cxe_loss' with SOFT_LABELING
  modeling/roi_heads/box_head/roi_box_predictors.py:63-68,76-77    cls_score: 2 outputs for 'cxe_loss', 1 for 'mse_loss' / 'l1_loss'
  modeling/roi_heads/box_head/inference.py:61-69 'cxe_loss' scores like 'ce_loss' (softmax), 'l1_loss' like 'mse_loss' (sigmoid)

Two quirks, both reproduced because they are what the reference trains on:
  * 'mse_loss' and 'l1_loss' subtract soft labels [M] from sigmoids [M, 1]: broadcasting makes that [M, M], so `torch.mean` runs over
    M x M (row, label) pairs.  With s = sigmoid(x), t the soft labels, mt = mean(t):
        mse = mean_i (s_i - mt)^2 + mean_j (t_j - mt)^2,        d mse / d x_i = (2 / M) (s_i - mt) s_i (1 - s_i)
        l1  = (1 / M^2) sum_i sum_j |s_i - t_j| (no closed form), d l1 / d x_i = (1 / M^2) s_i (1 - s_i) sum_j sign(s_i - t_j), sign(0) = 0
  * 'cxe_loss' takes the mean over the 2M elements of an [M, 2] tensor: HALF the soft cross-entropy; d / d x = (softmax - [1 - t, t]) / (2M).
"""
import torch

import box_cls_loss_ref as bcl
from oracle import box_train_ref as obt

W_CLS, W_BOX = bcl.W_CLS, bcl.W_BOX
FUNCS = ("discrete", "linear", "transLinear", "trans4thLinear")
SOFT_LOSSES = ("mse_loss", "l1_loss", "cxe_loss")


def n_logits(cls_loss):
    if cls_loss not in SOFT_LOSSES:
        raise ValueError("cls_loss %r reads no soft labels" % (cls_loss,))
    return 2 if cls_loss == "cxe_loss" else 1


def soft_labeling_function(t, func):
    """loss.py:81-104, verbatim arithmetic on a float32 tensor."""
    if func == "discrete":
        return (t >= 0.5).float()
    if func == "linear":
        return t
    if func == "transLinear":
        upper = (0.2 * t + 0.8) * (t >= 0.5).float()
        middle = (2.25 * t - 0.225) * (t >= 0.1).float() * (t < 0.5).float()
        lower = 0
        return upper + middle + lower
    if func == "trans4thLinear":
        upper = (0.2 * t + 0.8) * (t >= 0.5).float()
        lower = 0.9 * ((2 * t) ** 4) * (t < 0.5).float()
        return upper + lower
    raise ValueError("soft labeling function %r" % (func,))


def match_iou(props, gt, thresh=obt.IOU_THRESH):
    """loss.py:47-62 for one image -> (matched index [P] (-1 below the threshold: high == low threshold), the IoU with the matched
    ground truth [P] float32, 0 where the index is negative)."""
    q = obt.boxlist_iou(gt, props)
    vals, matches = q.max(dim=0)
    matches = matches.clone()
    matches[vals < thresh] = -1
    iou = q.t()[torch.arange(len(matches)), matches.clamp(min=0)].clone()
    iou[matches < 0] = 0
    return matches, iou


def soft_labels(props, gt, thresh, func):
    """The soft label of every proposal of one image, [P] float32 (an image without ground truth has none: the caller skips it)."""
    return soft_labeling_function(match_iou(props, gt, thresh)[1], func)


def subsample(props, gt, keys, thresh, func, batch=obt.BATCH_PER_IMAGE, fraction=obt.POSITIVE_FRACTION):
    """loss.py:234-292 with SOFT_LABELING for one image: oracle.box_train_ref.subsample's rows (randperm := argsort(keys)) at the
    matcher threshold `thresh`, plus the soft labels of the sampled rows and of every proposal."""
    matches, iou = match_iou(props, gt, thresh)
    lab = torch.ones(len(props), dtype=torch.int64)
    lab[matches == -1] = 0
    idx, p1, p2 = obt.sample(lab, keys, batch=batch, fraction=fraction)
    soft = soft_labeling_function(iou, func)
    return dict(index=idx, labels=lab[idx], soft=soft[idx], all_labels=lab, all_soft=soft, perms=(p1, p2))


def cls_loss_value(class_logits, soft, cls_loss):
    """loss.py:360-367 as written (the broadcasts left in place).  class_logits [M, L], soft [M]."""
    if n_logits(cls_loss) != class_logits.shape[1]:
        raise ValueError("%s has %d logit(s) per row, got %d" % (cls_loss, n_logits(cls_loss), class_logits.shape[1]))
    soft = soft.to(class_logits.dtype)
    if cls_loss == "mse_loss":
        return torch.mean((class_logits.sigmoid() - soft) ** 2)                 # [M,1] - [M] -> [M,M]
    if cls_loss == "l1_loss":
        return torch.mean(torch.abs(class_logits.sigmoid() - soft))             # [M,1] - [M] -> [M,M]
    my_target = torch.stack([1 - soft, soft], dim=1)
    return -(my_target * torch.log(class_logits.softmax(dim=1))).mean()        # CXE: mean over 2M elements


def losses(class_logits, box_regression, labels, soft, targets, cls_loss):
    """-> (5 * classification, 2.5 * box regression); the regression loss goes by the hard labels (loss.py:379-393)."""
    return W_CLS * cls_loss_value(class_logits, soft, cls_loss), W_BOX * bcl.box_loss(box_regression, labels, targets)


def closed_form(class_logits, soft, cls_loss):
    """The value the kernel computes: no [M, M] tensor for mse, the pair sum for l1, a stable log-softmax for cxe."""
    soft = soft.to(class_logits.dtype)
    M = len(soft)
    if cls_loss == "mse_loss":
        s = torch.sigmoid(class_logits.reshape(-1))
        mt = soft.mean()
        return ((s - mt) ** 2).mean() + ((soft - mt) ** 2).mean()
    if cls_loss == "l1_loss":
        s = torch.sigmoid(class_logits.reshape(-1))
        return sum((s[i] - soft).abs().sum() for i in range(M)) / (M * M)
    lp = torch.log_softmax(class_logits, dim=1)
    return -((1 - soft) * lp[:, 0] + soft * lp[:, 1]).sum() / (2 * M)


def closed_form_grad(class_logits, soft, cls_loss):
    """d closed_form / d class_logits, [M, L], as the kernel writes it (before the weight 5)."""
    soft = soft.to(class_logits.dtype)
    M = len(soft)
    if cls_loss == "cxe_loss":
        return (class_logits.softmax(dim=1) - torch.stack([1 - soft, soft], dim=1)) / (2 * M)
    s = torch.sigmoid(class_logits.reshape(-1))
    if cls_loss == "mse_loss":
        return ((2.0 / M) * (s - soft.mean()) * s * (1 - s)).reshape(M, 1)
    sg = torch.sign(s[:, None] - soft[None, :]).sum(dim=1)
    return (s * (1 - s) * sg / (M * M)).reshape(M, 1)


def rowwise_value(class_logits, soft, cls_loss):
    """What a reader expects and the reference does NOT compute: the mean over the M rows (mse / l1), the full soft cross-entropy (cxe)."""
    soft = soft.to(class_logits.dtype)
    if cls_loss == "mse_loss":
        return ((torch.sigmoid(class_logits.reshape(-1)) - soft) ** 2).mean()
    if cls_loss == "l1_loss":
        return (torch.sigmoid(class_logits.reshape(-1)) - soft).abs().mean()
    lp = torch.log_softmax(class_logits, dim=1)
    return -((1 - soft) * lp[:, 0] + soft * lp[:, 1]).mean()


def decode_mode(cls_loss):
    """inference.py:61-69: the mode of tests/box_cls_loss_ref.py whose score a soft loss uses."""
    return {"cxe_loss": "ce_loss", "l1_loss": "mse_loss", "mse_loss": "mse_loss"}[cls_loss]
