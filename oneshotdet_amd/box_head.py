"""Second-stage few-shot ROI box head on MI355X, inference path.

Mirrors ROIBoxHead.forward (modeling/roi_heads/box_head/box_head.py:81-259) for the config of record
(SECOND_STAGE_METHOD 'concat', no negative support; SECOND_STAGE_CLS_LOSS 'ce_loss', or with box_cls_loss 'focal_loss' /
'mse_loss': cls_score has ONE output and the score is its sigmoid, inference.py:61-69):
  feature_extractor = Pooler 7x7 over P3..P7 of the TARGET backbone (not the correlated maps: generalized_rcnn.py:317)
  supproi_pooling   = the same Pooler on one whole-image box per query (generalized_rcnn.py:257,290)
  cat(x, query) -> conv1x1 512->512, GN, LeakyReLU -> conv1x1 512->256, GN, LeakyReLU -> conv3x3 256->128, GN, LeakyReLU
  -> fc6 6272->1024, ReLU -> fc7, ReLU -> cls_score (2) | bbox_pred (8) -> softmax, decode, clip, NMS 0.5.
MI355X design: the first 1x1 conv is split at the concatenation, conv(cat(x, q)) = W_x x + (W_q q + b).  The query half
is one 7x7 map per (image, shot) instead of one per ROI; it is added inside the GroupNorm kernel that follows, so the
concatenated [R,7,7,512] tensor never exists, the conv does half the FLOPs, and with several shots the ROI half is
computed once.  The Linear layers are 1x1 convs on the implicit-GEMM kernels (fc6 reads the [R,7,7,128] maps as
[R,1,1,6272] with its weight columns permuted to (h, w, c) order at pack time).
"""
import numpy as np
import torch

from . import ops, spec
from .ops import ACT_NONE, ACT_RELU, PackedConv


class BoxHeadWeights(object):
    """Packed `roi_heads.box.*` (spec.box_head_shapes)."""

    def __init__(self, sd, dtype, prefix="roi_heads.box.", box_cls_loss="ce_loss", soft_labeling=False, linear_fusion=False,
                 neg_support=False):
        # spec.MODEL_OPTIONS, and the state_dict's layout and cls_score against them: ValueError by name before anything is packed.
        # FEW_SHOT.NEG_SUPPORT is validated and otherwise nothing: inference discards the negative branch
        given = spec.options_in(locals())
        options = spec.check_options("the box head", True, box_sd=sd, box_prefix=prefix, **given)
        vars(self).update((name, getattr(options, name)) for name in given)
        c = spec.FPN_OUT
        if self.linear_fusion:
            # FEW_SHOT.LINEAR_FUSION: the 3x3 conv over cat(x, query), split at the concatenation like the 1x1 conv below (zero
            # padding commutes with the split): conv3x3(cat(x, q)) = W_x * x + (W_q * q + b)
            wa, ba = sd[prefix + "feature_aggreg.0.weight"], sd[prefix + "feature_aggreg.0.bias"]
            self.aggreg_x = ops.pack_conv(wa[:, :c].contiguous(), bias=None, dtype=dtype)     # ROI half, no bias
            self.aggreg_q = ops.pack_conv(wa[:, c:].contiguous(), bias=ba, dtype=dtype)       # query half + bias
            self.gn = [tuple(sd[prefix + "feature_aggreg.1." + leaf].float().contiguous() for leaf in ("weight", "bias"))]
        else:
            w0, b0 = sd[prefix + "compress_dim_conv.0.weight"], sd[prefix + "compress_dim_conv.0.bias"]
            self.conv0_x = ops.pack_conv(w0[:, :c].contiguous(), bias=None, dtype=dtype)          # ROI half, no bias
            self.conv0_q = ops.pack_conv(w0[:, c:].contiguous(), bias=b0, dtype=dtype)            # query half + bias
            self.conv3 = ops.pack_conv(sd[prefix + "compress_dim_conv.3.weight"], bias=sd[prefix + "compress_dim_conv.3.bias"],
                                       dtype=dtype)
            self.aggreg = ops.pack_conv(sd[prefix + "feature_aggreg.0.weight"], bias=sd[prefix + "feature_aggreg.0.bias"],
                                        dtype=dtype)
            self.gn = [tuple(sd[prefix + name + "." + leaf].float().contiguous() for leaf in ("weight", "bias"))
                       for name in ("compress_dim_conv.1", "compress_dim_conv.4", "feature_aggreg.1")]
        p, mid = spec.BOX_POOL, c // 2
        # fc6 columns are (c, h, w) in the reference (x.view(N, -1) of NCHW, box_head.py:151); as an OIHW conv weight the
        # packer writes them in (h, w, c) order = the flattening of this build's NHWC ROI maps
        fc6 = ops.pack_conv(sd[prefix + "fc6.weight"].reshape(spec.BOX_MLP_DIM, mid, p, p), bias=sd[prefix + "fc6.bias"],
                            dtype=dtype)
        self.fc6 = PackedConv(fc6.w.view(fc6.w_rows, 1, 1, p * p * fc6.cin_k), fc6.bias, fc6.cout, fc6.cout_store,
                              fc6.w_rows, p * p * fc6.cin_k, 1, 1)
        self.fc7 = ops.pack_conv(sd[prefix + "fc7.weight"][:, :, None, None], bias=sd[prefix + "fc7.bias"], dtype=dtype)
        wp = torch.cat([sd[prefix + "predictor.cls_score.weight"], sd[prefix + "predictor.bbox_pred.weight"]], 0)
        bp = torch.cat([sd[prefix + "predictor.cls_score.bias"], sd[prefix + "predictor.bbox_pred.bias"]], 0)
        self.pred = ops.pack_conv(wp[:, :, None, None].contiguous(), bias=bp, dtype=dtype)  # cols 0..L-1 cls (L = 2, or 1 in the sigmoid modes), then 8 deltas


def check_shots(box_cls_loss, shots):
    """Inference with several queries per image exists for 'ce_loss' only: in the one-logit modes the reference's arg-max over
    shots builds a 4-column index ([M, 1] logits) for the 8 regression columns and raises IndexError (box_head.py:246-253).
    Training is unaffected: it uses the first query only (box_head.py:123-203)."""
    if shots > 1 and spec.BOX_CLS_MODES[box_cls_loss].logits != 2:         # 'cxe_loss' has two logits: it scores and decodes as 'ce_loss'
        raise ValueError("box_cls_loss=%r with %d shots: the reference's arg-max over shots indexes the 8 regression columns of a "
                         "one-logit predictor with a 4-column index and raises IndexError (box_head.py:246-253); the second stage "
                         "detects with one shot in this mode" % (box_cls_loss, shots))


def query_level(qh, qw):
    """LevelMapper for the whole-image query box [0, 0, h, w] (generalized_rcnn.py:257), fp32 like the reference."""
    f = np.float32
    s = np.sqrt((f(qh) + f(1)) * (f(qw) + f(1)), dtype=np.float32)
    lv = np.floor(f(spec.LEVEL_MAP_LEVEL) + np.log2(s / f(spec.LEVEL_MAP_SCALE) + f(spec.LEVEL_MAP_EPS), dtype=np.float32))
    return int(min(max(lv, 3), 3 + len(spec.POOLER_SCALES) - 1)) - 3


def run_query_roi(qfeats, q_size, dtype):
    """supproi_pooling: [B*S, 7, 7, C] in the activation dtype.  q_size: (h, w) shared by all queries, or one per query
    (padded batch): each whole-image box goes through the level-routed Pooler like any other ROI."""
    from .model import whole_image_rois
    n = qfeats[0].shape[0]
    sizes = [tuple(q_size)] * n if isinstance(q_size[0], int) else [tuple(s) for s in q_size]
    if len(set(sizes)) == 1:
        lvl = query_level(*sizes[0])
        rois = whole_image_rois(sizes, qfeats[0].device)
        v = ops.roi_align(qfeats[lvl], rois, spec.POOLER_SCALES[lvl], spec.BOX_POOL, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO)
        return v if dtype == torch.float32 else ops.cast_f32(v, dtype)
    boxes = whole_image_rois(sizes, qfeats[0].device)[:, 1:].reshape(n, 1, 4).contiguous()      # [0, 0, h, w] per query
    return ops.roi_pool_levels(qfeats, spec.POOLER_SCALES, boxes, None, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO)


def run_query_half(bw, qfeats, q_size, dtype):
    """The query's share of the head in front of fc6: supproi_pooling, then the query half of the split first conv.
    -> (q [N*S,7,7,C], q_half [N*S,7,7,512 | 128] = W_q q + b).  What HotPathEngine.enroll keeps in a QueryBank."""
    q = run_query_roi(qfeats, q_size, dtype)
    # FEW_SHOT.LINEAR_FUSION (box_head.py:61-72,148): the head in front of fc6 is the split 3x3 conv, GroupNorm, LeakyReLU
    conv_q, pad = (bw.aggreg_q, 1) if bw.linear_fusion else (bw.conv0_q, 0)
    return q, ops.conv2d(q, conv_q, pad=pad)


def run_box_head(bw, feats, qfeats, q_size, boxes, counts, img_h, img_w, shots=1, cuda_nms=True, want_raw=False, img_hw=None,
                 classes=1, bank=None, slots=None):
    """feats / qfeats: NHWC P3..P7 of the target / query backbone; boxes [N,R,4], counts [N] = first-stage proposals.
    Returns dict(boxes [N,K,4], scores [N,K] descending, counts [N]) (+ raw logits / deltas / pooled maps).
    classes = K (the class sweep): N = B*K rows of proposals (row b*K + k), feats has B images, qfeats B*K*shots, img_hw N rows; the
    ROI pooling reads image row // K and everything after it is the per-pair head on N rows.
    bank + slots (the query gallery; qfeats and q_size unused): the query halves are rows of bank.q_half, [G*shots] maps enrolled once,
    picked by the device int32 [N] table: row slots[j]*shots + s for ROI set j.  They are gathered by one index_select and go to the
    existing GroupNorm entry: osd_groupnorm_act_rois_gallery, which reads them through the table, measured 1 % SLOWER than that
    composition at bs 4 and 8 (profiles/query_bank.md), so it is not on this path (ops.groupnorm_act_rois(add_index=) is the entry).
    No query backbone, pooling or conv launch either way."""
    n, r, _ = boxes.shape
    dtype = feats[0].dtype
    check_shots(bw.box_cls_loss, shots)                                                # nothing has been launched yet
    linear = bw.linear_fusion
    conv_x, pad = (bw.aggreg_x, 1) if linear else (bw.conv0_x, 0)
    if bank is not None:
        assert bank.shots == shots and slots.shape == (n,)
        rows = slots if shots == 1 else (slots[:, None] * shots + torch.arange(shots, device=slots.device, dtype=slots.dtype)).reshape(-1)
        q_half = bank.q_half.index_select(0, rows)                                     # [N*S,7,7,512 | 128], on the device
        q = bank.query_roi.index_select(0, rows) if want_raw else None
    else:
        q, q_half = run_query_half(bw, qfeats, q_size, dtype)                          # [N*S,7,7,C], [N*S,7,7,512 | 128]  W_q q + b
        assert q.shape[0] == n * shots
    x = ops.roi_pool_levels(feats, spec.POOLER_SCALES, boxes, counts, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO,
                            sets_per_image=classes)
    u0 = ops.conv2d(x, conv_x, pad=pad)                                                # [N*R,7,7,512 | 128]  W_x x, once for all shots
    preds = torch.empty((shots, n * r, bw.pred.cout_store), device=boxes.device, dtype=dtype)
    for s in range(shots):                                                             # box_head.py:122
        g0, b0 = bw.gn[0]
        t = ops.groupnorm_act_rois(u0, g0, b0, spec.GN_GROUPS, spec.GN_EPS, spec.BOX_LEAKY_SLOPE, addend=q_half,
                                   rois_per_add=r, add_stride=shots, add_offset=s)
        if not linear:
            (g1, b1), (g2, b2) = bw.gn[1:]
            t = ops.conv2d(t, bw.conv3)
            t = ops.groupnorm_act_rois(t, g1, b1, spec.GN_GROUPS, spec.GN_EPS, spec.BOX_LEAKY_SLOPE, out=t)
            t = ops.conv2d(t, bw.aggreg, pad=1)
            t = ops.groupnorm_act_rois(t, g2, b2, spec.GN_GROUPS, spec.GN_EPS, spec.BOX_LEAKY_SLOPE, out=t)
        t = ops.conv2d(t.view(n * r, 1, 1, -1), bw.fc6, act=ACT_RELU)
        t = ops.conv2d(t, bw.fc7, act=ACT_RELU)
        ops.conv2d(t, bw.pred, act=ACT_NONE, out=preds[s].view(n * r, 1, 1, -1))
    dec = ops.box_decode(preds, boxes, counts, spec.BOX_REG_WEIGHTS, img_h, img_w, spec.BOX_SCORE_THRESH, want_raw=want_raw,
                         img_hw=img_hw, cls_loss=bw.box_cls_loss, soft_labeling=bw.soft_labeling)
    scores, dboxes = dec[0], dec[1]
    bs, ss, _, cnt = ops.rank_sort_gather(scores, dboxes, r)
    keep = min(spec.BOX_DETECTIONS_PER_IMG, r)
    ob, os_, _, oc = ops.nms_sorted(bs, ss, cnt, spec.BOX_NMS_THRESH, keep, cuda_semantics=cuda_nms)
    out = dict(boxes=ob, scores=os_, counts=oc)
    if want_raw:
        out.update(logits=dec[2], box_regression=dec[3], pooled=x, query_roi=q)
    return out
