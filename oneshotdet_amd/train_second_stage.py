"""The second stage inside the training step (TrainEngine mixin, second_stage=True): ROIBoxHead in training on the training
proposals — subsample, box head forward, classification loss (self.box_cls_loss) + smooth-L1, the whole backward.  Reference: box_head.py:100-203."""

import torch

from . import ops, spec
from .ops import ACT_RELU


class SecondStage(object):
    def box_head_forward_backward(self, feats, qfeats, q_sizes, shots, proposals, gt_boxes, gt_count, keys=None,
                                  want_debug=False, neg_qfeats=None, neg_q_sizes=None):
        """ROIBoxHead in training (box_head.py:100-203) on the training proposals (ground truth appended): subsample on the
        device, box head forward on the 128 sampled ROIs per image with the FIRST query of every image (the reference returns
        the losses from inside its loop over shots), cross-entropy (or, by self.box_cls_loss, the sigmoid focal / mse loss over the one
        logit) + smooth-L1 with the weights 5 / 2.5, and the whole
        backward on the current stream: weight / bias / GroupNorm gradients into the flat buffer, the gradient w.r.t. the
        target FPN features as fp32 level maps and w.r.t. the query features' level.
        proposals = (boxes [N,P,4], scores, counts).  keys [N,P]: uniform randoms of the sampler (default: torch.rand).
        -> (losses [3] = (loss_classifier, loss_box_reg, sampled rows), gx: 5 fp32 maps, (query level, fp32 map [N,h,w,C]))
        neg_qfeats / neg_q_sizes (FEW_SHOT.NEG_SUPPORT, box_head.py:128-139,156-161,180-188; one shot, 'ce_loss'): the feature maps and
        true sizes of one negative support per image.  The same sampled ROIs are scored against it with the same weights: the ROI half
        of compress_dim_conv.0 runs once, the first GroupNorm once per addend, and from its output on the trunk runs on one stacked
        batch of 2M rows, the positive branch's rows first.  losses is then [5] = (loss_classifier, loss_box_reg, sampled rows,
        loss_cls_suppress, foreground rows) and a fourth value is returned: the negative query's gradient, as the third is the query's."""
        from . import box_head as bh
        from . import model
        b, cv, dt = "roi_heads.box.", self.convs, self.dtype
        pb, _, pc = proposals
        n, P, _ = pb.shape
        S = spec.BOX_BATCH_PER_IMAGE
        if keys is None:
            keys = torch.rand((n, P), device=self.device, dtype=torch.float32)
        # FEW_SHOT.SOFT_LABELING: the soft labels travel from the sampler to the loss (loss.py:260-287,333-334) when the loss reads
        # them; 'ce_loss' / 'focal_loss' never do, and make the launches they make without the option
        soft = spec.box_loss_reads_soft_labels(self.box_cls_loss, self.soft_labeling)
        ss = None
        if soft:
            sb, sl, st, si, sc, ss = ops.box_match_sample(pb, pc, gt_boxes, gt_count, keys, S, spec.BOX_POSITIVE_FRACTION,
                                                          spec.BOX_FG_IOU_THRESH, spec.BOX_REG_WEIGHTS,
                                                          soft_func=self.soft_labeling_func)
        else:
            sb, sl, st, si, sc = ops.box_match_sample(pb, pc, gt_boxes, gt_count, keys, S, spec.BOX_POSITIVE_FRACTION,
                                                      spec.BOX_FG_IOU_THRESH, spec.BOX_REG_WEIGHTS)
        M = n * S
        slope, gr, eps = spec.BOX_LEAKY_SLOPE, spec.GN_GROUPS, spec.GN_EPS
        linear = self.linear_fusion
        neg = neg_qfeats is not None
        if neg != self.neg_support:
            raise ValueError("neg_qfeats (FEW_SHOT.NEG_SUPPORT) is passed exactly when the engine was built with neg_support=True")
        if neg and (shots != 1 or linear or self.box_cls_loss != "ce_loss"):
            spec.check_neg_support(True, True, linear, self.box_cls_loss, self.soft_labeling, shots)
        (g2, dg2), (b2, db2) = self.extra[b + "feature_aggreg.1.weight"], self.extra[b + "feature_aggreg.1.bias"]
        if linear:
            # FEW_SHOT.LINEAR_FUSION (box_head.py:61-72,148): the split 3x3 conv takes the place of the split 1x1 conv, its
            # GroupNorm is feature_aggreg.1 and nothing stands between it and fc6
            c0x, c0q, pad0 = cv[b + "feature_aggreg.0x"], cv[b + "feature_aggreg.0q"], 1
            (g0, dg0), (b0, db0) = (g2, dg2), (b2, db2)
        else:
            (g0, dg0), (b0, db0) = self.extra[b + "compress_dim_conv.1.weight"], self.extra[b + "compress_dim_conv.1.bias"]
            (g1, dg1), (b1, db1) = self.extra[b + "compress_dim_conv.4.weight"], self.extra[b + "compress_dim_conv.4.bias"]
            c0x, c0q, c3, ca = (cv[b + k] for k in ("compress_dim_conv.0x", "compress_dim_conv.0q", "compress_dim_conv.3",
                                                     "feature_aggreg.0"))
            pad0 = 0
        fc6, fc7, cp = cv[b + "fc6"], cv[b + "fc7"], cv[b + "pred"]
        # ---- forward
        qf1 = qfeats if shots == 1 else [q[::shots].contiguous() for q in qfeats]
        qs1 = [q_sizes[i * shots] for i in range(n)]
        uniform = len(set(qs1)) == 1
        q = bh.run_query_roi(qf1, qs1[0] if uniform else qs1, dt)                                # [N,7,7,C]
        qh = ops.conv2d(q, c0q.pc, pad=pad0)                                                     # W_q q + b
        x = ops.roi_pool_levels(feats, spec.POOLER_SCALES, sb, sc, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO)
        u0 = ops.conv2d(x, c0x.pc, pad=pad0)
        q_neg = qh_neg = None
        R = 2 * M if neg else M                              # rows of the trunk behind the first GroupNorm
        if neg:
            nqs = [tuple(s) for s in neg_q_sizes]
            q_neg = bh.run_query_roi(neg_qfeats, nqs[0] if len(set(nqs)) == 1 else nqs, dt)
            qh_neg = ops.conv2d(q_neg, c0q.pc, pad=pad0)
            t0 = torch.empty((R,) + tuple(u0.shape[1:]), device=u0.device, dtype=u0.dtype)
            for half, add in ((t0[:M], qh), (t0[M:], qh_neg)):
                ops.groupnorm_act_rois(u0, g0, b0, gr, eps, slope, addend=add, rois_per_add=S, add_stride=1, add_offset=0, out=half)
        else:
            t0 = ops.groupnorm_act_rois(u0, g0, b0, gr, eps, slope, addend=qh, rois_per_add=S, add_stride=1, add_offset=0)
        u1 = t1 = u2 = d_u2 = d_t1 = d_u1 = None
        if linear:
            t2 = t0
        else:
            u1 = ops.conv2d(t0, c3.pc)
            t1 = ops.groupnorm_act_rois(u1, g1, b1, gr, eps, slope)
            u2 = ops.conv2d(t1, ca.pc, pad=1)
            t2 = ops.groupnorm_act_rois(u2, g2, b2, gr, eps, slope)
        t2f = t2.view(R, 1, 1, -1)
        f6 = ops.conv2d(t2f, fc6.pc, act=ACT_RELU)
        f7 = ops.conv2d(f6, fc7.pc, act=ACT_RELU)
        pred = ops.conv2d(f7, cp.pc)
        if neg:
            d_pred = torch.empty((R, cp.pd.cin_k), device=pred.device, dtype=pred.dtype)     # d_pred stacked over d_pred_neg
            losses, _, _ = ops.box_loss_neg_support(pred[:M], pred[M:], sl, st, sc, n, S, spec.BOX_LOSS_WEIGHTS[0],
                                                    spec.BOX_LOSS_WEIGHTS[1], grad_stride=cp.pd.cin_k, d_out=d_pred)
        else:
            losses, d_pred = ops.box_loss(pred, sl, st, sc, n, S, spec.BOX_LOSS_WEIGHTS[0], spec.BOX_LOSS_WEIGHTS[1],
                                          grad_stride=cp.pd.cin_k, cls_loss=self.box_cls_loss, soft=ss)
        # ---- backward (inline on this stream: M = 1024 ROIs)

        def wg(c, xin, dy, pad=0):
            ops.conv2d_wgrad(xin, dy, c.gw, c.r, c.s, 1, pad, c.cout, db=c.gb if c.has_bias else None)

        def dg(c, dy, mask=None):
            return ops.conv2d(dy, c.pd, pad=c.r - 1 - (c.r // 2), mask=mask)
        d_pred = d_pred.view(R, 1, 1, -1)
        wg(cp, f7, d_pred)
        d_f7 = dg(cp, d_pred, mask=f7)
        wg(fc7, f6, d_f7)
        d_f6 = dg(fc7, d_f7, mask=f6)
        wg(fc6, t2f, d_f6)
        d_t2 = dg(fc6, d_f6).view(t2.shape)
        if linear:
            d_t0 = d_t2
        else:
            d_u2 = ops.groupnorm_act_rois_bwd(u2, g2, b2, d_t2, dg2, db2, gr, eps, slope)
            wg(ca, t1, d_u2, pad=1)
            d_t1 = dg(ca, d_u2)
            d_u1 = ops.groupnorm_act_rois_bwd(u1, g1, b1, d_t1, dg1, db1, gr, eps, slope)
            wg(c3, t0, d_u1)
            d_t0 = dg(c3, d_u1)
        d_u0_pos = d_u0_neg = d_qh_neg = d_q_neg = None
        if neg:
            # the same u0 under two addends: each half's gradient w.r.t. u0 (dgamma / dbeta accumulate over both calls), their sum
            # into the ROI half of the conv, each half's ROI sum into the query half (the weight gradient accumulates too)
            d_u0_pos = ops.groupnorm_act_rois_bwd(u0, g0, b0, d_t0[:M], dg0, db0, gr, eps, slope, addend=qh, rois_per_add=S,
                                                  add_stride=1, add_offset=0)
            d_u0_neg = ops.groupnorm_act_rois_bwd(u0, g0, b0, d_t0[M:], dg0, db0, gr, eps, slope, addend=qh_neg, rois_per_add=S,
                                                  add_stride=1, add_offset=0)
            d_u0 = ops.add_mask(d_u0_pos, d_u0_neg)
        else:
            d_u0 = ops.groupnorm_act_rois_bwd(u0, g0, b0, d_t0, dg0, db0, gr, eps, slope, addend=qh, rois_per_add=S, add_stride=1,
                                              add_offset=0)
        wg(c0x, x, d_u0, pad=pad0)
        d_x = dg(c0x, d_u0)
        d_qh = ops.rois_sum(d_u0_pos if neg else d_u0, n, S)   # the query half was added to every ROI of its image
        wg(c0q, q, d_qh, pad=pad0)
        d_q = dg(c0q, d_qh)
        if neg:
            d_qh_neg = ops.rois_sum(d_u0_neg, n, S)
            wg(c0q, q_neg, d_qh_neg, pad=pad0)
            d_q_neg = dg(c0q, d_qh_neg)
        gx = ops.roi_pool_levels_bwd([(f.shape[1], f.shape[2]) for f in feats], spec.POOLER_SCALES, sb, sc, d_x, spec.BOX_POOL,
                                     spec.POOLER_SAMPLING_RATIO)

        def query_grad(d_q, qf, qs):
            if len(set(qs)) == 1:
                lvl = bh.query_level(*qs[0])
                rois = model.whole_image_rois(qs, self.device)
                gq = ops.roi_align_bwd(d_q.float(), rois, qf[lvl].shape, spec.POOLER_SCALES[lvl], spec.BOX_POOL, spec.BOX_POOL,
                                       spec.POOLER_SAMPLING_RATIO)
                return [(lvl, gq)]
            # padded query batch: every whole-image box picks its own level
            boxes = model.whole_image_rois(qs, self.device)[:, 1:].reshape(n, 1, 4).contiguous()
            maps = ops.roi_pool_levels_bwd([(f.shape[1], f.shape[2]) for f in qf], spec.POOLER_SCALES, boxes, None, d_q,
                                           spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO)
            return list(enumerate(maps))
        gqs = query_grad(d_q, qf1, qs1)
        gqs_neg = query_grad(d_q_neg, neg_qfeats, nqs) if neg else None
        self._keep.append((sb, sl, st, si, sc, q, qh, x, u0, t0, u1, t1, u2, t2, f6, f7, pred, d_pred, d_f7, d_f6, d_t2, d_u2,
                           d_t1, d_u1, d_t0, d_u0, d_x, d_qh, d_q, keys, ss, q_neg, qh_neg, d_u0_pos, d_u0_neg, d_qh_neg, d_q_neg,
                           neg_qfeats))
        if want_debug:
            self.last_box = dict(boxes=sb, labels=sl, targets=st, index=si, counts=sc, pred=pred[:M] if neg else pred, soft=ss)
            if neg:
                self.last_box["pred_neg"] = pred[M:]
        return (losses, gx, gqs, gqs_neg) if neg else (losses, gx, gqs)
