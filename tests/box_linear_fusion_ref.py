"""Test infrastructure: CPU restatement of the second-stage box head with FEW_SHOT.LINEAR_FUSION True — forward, losses and, through
torch autograd, every gradient.  oracle/box_head_ref.py restates the default head (compress_dim_conv in front of feature_aggreg)
only; the restatement of the option lives here and is pinned to the REAL reference by tests/golden/make_golden_linear_fusion.py
(fixtures tests/golden/box_*_linear.npz, boxtrain_*_linear.npz) and tests/test_box_linear_fusion.py.

Paths relative to the reference's maskrcnn_benchmark/:
  modeling/roi_heads/box_head/box_head.py:43        no compress_dim_conv module is built
  modeling/roi_heads/box_head/box_head.py:61-72     feature_aggreg = Conv2d(512, 128, 3, 1, 1), GroupNorm(32, 128), LeakyReLU(0.2)
  modeling/roi_heads/box_head/box_head.py:147-155   cat((x, expanded_supp), 1) -> feature_aggreg -> flatten -> fc6 -> fc7 -> predictor
  modeling/roi_heads/box_head/box_head.py:123,241-253   the loop over shots and the per-class arg-max over them (unchanged)

The Pooler (level routing + 7 x 7 ROIAlign) is the oracle's differentiable one, so autograd reaches the FPN features of both
branches.  `double=True` evaluates everything behind the pooling geometry in float64 (the geometry stays fp32 as in the reference).
"""
import torch
import torch.nn.functional as F

import box_cls_loss_ref as bcl
from oracle import box_head_ref as obh

P = "roi_heads.box."


def fuse(x, supp, sd, prefix=P):
    """box_head.py:147-151 with LINEAR_FUSION: x [M, C, 7, 7] ROI maps, supp [M, C, 7, 7] the query map of each ROI's image ->
    [M, C / 2, 7, 7]."""
    y = torch.cat((x, supp), dim=1)
    y = F.conv2d(y, sd[prefix + "feature_aggreg.0.weight"], sd[prefix + "feature_aggreg.0.bias"], padding=1)
    return F.leaky_relu(F.group_norm(y, 32, sd[prefix + "feature_aggreg.1.weight"], sd[prefix + "feature_aggreg.1.bias"], 1e-5), 0.2)


def fuse_split(x, supp_maps, image_of_roi, sd, prefix=P):
    """The same numbers the way the engines compute them: conv3x3(cat(x, q)) = W_x * x + (W_q * q + b), the query half once per
    query map.  supp_maps [n, C, 7, 7], image_of_roi [M] int64.  Zero padding commutes with the split, so this equals `fuse`."""
    w, b = sd[prefix + "feature_aggreg.0.weight"], sd[prefix + "feature_aggreg.0.bias"]
    c = x.shape[1]
    u = F.conv2d(x, w[:, :c], None, padding=1)
    q3 = F.conv2d(supp_maps, w[:, c:], b, padding=1)
    y = u + q3[image_of_roi]
    return F.leaky_relu(F.group_norm(y, 32, sd[prefix + "feature_aggreg.1.weight"], sd[prefix + "feature_aggreg.1.bias"], 1e-5), 0.2)


def box_head_logits(feats, query_feats, proposals, query_sizes, sd, prefix=P, double=False):
    """ROIBoxHead.forward (eval, 'concat' without negative support, LINEAR_FUSION True): as oracle.box_head_ref.box_head_logits.
    proposals: list of [R, 4] per image.  -> class_logits [B*R, L], box_regression [B*R, 8] (after the arg-max over shots),
    pooled ROI maps [B, R, C, 7, 7]."""
    x = obh.pooler(feats, proposals)
    B, R, C, Hh, Ww = x.shape
    supp = obh.query_roi_features(query_feats, query_sizes).view(B, -1, C, Hh, Ww)
    if double:
        sd = {k: (v.double() if k.startswith(prefix) else v) for k, v in sd.items()}
        x, supp = x.double(), supp.double()
    all_logits, all_reg = [], []
    for s in range(supp.shape[1]):
        e = supp[:, [s]].expand_as(x).contiguous().view(-1, C, Hh, Ww)
        y = fuse(x.view(-1, C, Hh, Ww), e, sd, prefix)
        y = y.view(y.size(0), -1)
        y = F.relu(F.linear(y, sd[prefix + "fc6.weight"], sd[prefix + "fc6.bias"]))
        y = F.relu(F.linear(y, sd[prefix + "fc7.weight"], sd[prefix + "fc7.bias"]))
        all_logits.append(F.linear(y, sd[prefix + "predictor.cls_score.weight"], sd[prefix + "predictor.cls_score.bias"]))
        all_reg.append(F.linear(y, sd[prefix + "predictor.bbox_pred.weight"], sd[prefix + "predictor.bbox_pred.bias"]))
    if len(all_logits) > 1:
        tl, tr = torch.stack(all_logits, 0), torch.stack(all_reg, 0)
        idx = torch.argmax(tl, dim=0)
        logits = torch.gather(tl, 0, idx.unsqueeze(0))[0]
        reg = torch.gather(tr, 0, idx[:, :, None].expand(-1, -1, 4).reshape(idx.shape[0], -1).unsqueeze(0))[0]
    else:
        logits, reg = all_logits[0], all_reg[0]
    return logits, reg, x


def box_head_forward(feats, query_feats, proposals, image_sizes, query_sizes, sd, cls_loss="ce_loss", cuda_nms=False, double=False):
    """Second stage end to end -> dict(logits, box_regression, pooled, detections)."""
    logits, reg, pooled = box_head_logits(feats, query_feats, proposals, query_sizes, sd, double=double)
    det = bcl.postprocess(logits.float(), reg.float(), proposals, image_sizes, cls_loss, cuda_nms=cuda_nms)
    return dict(logits=logits, box_regression=reg, pooled=pooled, detections=det)


def box_train_forward(feats, query_feats, sampled, query_sizes, sd, shots=1, cls_loss="ce_loss", focal="cuda", double=False):
    """ROIBoxHead.forward in training on ALREADY sampled proposals (oracle.box_train_ref.box_train_forward with the option): the
    first query of every image only (box_head.py:123-203).  -> (5 * classification, 2.5 * box regression, logits, deltas)."""
    B = len(sampled)
    qf = [q.view(B, shots, *q.shape[1:])[:, 0] for q in query_feats]
    qs = [query_sizes[i * shots] for i in range(B)]
    logits, reg, _ = box_head_logits(feats, qf, [s["boxes"] for s in sampled], qs, sd, double=double)
    labels = torch.cat([s["labels"] for s in sampled])
    targets = torch.cat([s["targets"] for s in sampled])
    lc, lb = bcl.losses(logits, reg, labels, targets.to(reg.dtype), cls_loss, focal=focal)
    return lc, lb, logits, reg
