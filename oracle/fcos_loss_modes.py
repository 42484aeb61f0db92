"""ORACLE — test infrastructure only.  CPU restatement of the reference's FCOS loss with BOTH of its mode switches:
FCOS.CENTER_SAMPLE (modeling/rpn/fcos/loss.py:141-204: positives inside a box's sampling region, or inside the whole box) and
FCOS.LOC_LOSS_TYPE (layers/iou_loss.py:10-49: 'giou', 'iou', 'linear_iou').  oracle/hotpath_ref.py restates the config of record
only (centre sampling + GIoU); for that mode this file computes the same tensors in the same order of operations and must
reproduce `orc.fcos_loss` to the last bit (tests/test_fcos_loss_modes.py).  The other five modes are held to fixtures recorded
through the real reference (tests/golden/make_golden_fcos_loss.py -> fcos_loss_modes.npz).  The tests import it as
tests/fcos_loss_ref.py; oracle/launch_replay.py's loss-gradient launch differentiates it."""
import torch
import torch.nn.functional as F

from . import hotpath_ref as orc

INF = 100000000
SIZES = [[-1, 64], [64, 128], [128, 256], [256, 512], [512, INF]]          # loss.py:102-108
LOC_LOSS_TYPES = ("giou", "iou", "linear_iou")
MODES = [(cs, lt) for cs in (True, False) for lt in LOC_LOSS_TYPES]


def sample_region(bboxes, npl, xs, ys, radius):
    """get_sample_region, loss.py:52-99 -> inside [K, G] bool.  :58-61: no region at all (nothing positive in the image) when
    there is no box or the FIRST box's centre x is 0."""
    K, G = len(xs), bboxes.shape[0]
    gt = bboxes[None].expand(K, G, 4)
    cx = (gt[..., 0] + gt[..., 2]) / 2
    cy = (gt[..., 1] + gt[..., 3]) / 2
    if G == 0 or cx[..., 0].sum() == 0:
        return torch.zeros((K, G), dtype=torch.bool)
    cgt = torch.zeros_like(gt)
    beg = 0
    for lvl, n_p in enumerate(npl):
        end = beg + n_p
        st = orc.FPN_STRIDES[lvl] * radius
        xmin, ymin = cx[beg:end] - st, cy[beg:end] - st
        xmax, ymax = cx[beg:end] + st, cy[beg:end] + st
        cgt[beg:end, :, 0] = torch.where(xmin > gt[beg:end, :, 0], xmin, gt[beg:end, :, 0])
        cgt[beg:end, :, 1] = torch.where(ymin > gt[beg:end, :, 1], ymin, gt[beg:end, :, 1])
        cgt[beg:end, :, 2] = torch.where(xmax > gt[beg:end, :, 2], gt[beg:end, :, 2], xmax)
        cgt[beg:end, :, 3] = torch.where(ymax > gt[beg:end, :, 3], gt[beg:end, :, 3], ymax)
        beg = end
    cb = torch.stack((xs[:, None] - cgt[..., 0], ys[:, None] - cgt[..., 1], cgt[..., 2] - xs[:, None], cgt[..., 3] - ys[:, None]), -1)
    return cb.min(-1)[0] > 0


def fcos_targets(locations, gt_boxes_per_image, center_sample=True, radius=1.5):
    """prepare_targets + compute_targets_for_locations, loss.py:101-204.  locations: [n_l, 2] per level; gt: [n, 4] xyxy per image
    (labels all 1).  -> level-first (labels [sum N * n_l] int64, reg_targets [.., 4]).  An image without boxes is all label 0 with
    zero targets in BOTH modes (the reference fails on it when CENTER_SAMPLE is off: min over an empty dimension)."""
    npl = [len(l) for l in locations]
    soi = torch.cat([torch.tensor(SIZES[l], dtype=torch.float32)[None].expand(n, -1) for l, n in enumerate(npl)], 0)
    pts = torch.cat(locations, dim=0)
    xs, ys = pts[:, 0], pts[:, 1]
    K = len(xs)
    labels_all, reg_all = [], []
    for bboxes in gt_boxes_per_image:
        bboxes = torch.as_tensor(bboxes, dtype=torch.float32).reshape(-1, 4)
        if bboxes.shape[0] == 0:
            labels_all.append(torch.split(torch.zeros(K, dtype=torch.int64), npl, dim=0))
            reg_all.append(torch.split(torch.zeros(K, 4), npl, dim=0))
            continue
        area = (bboxes[:, 2] - bboxes[:, 0] + 1) * (bboxes[:, 3] - bboxes[:, 1] + 1)     # bounding_box.py:226-231
        l = xs[:, None] - bboxes[:, 0][None]
        t = ys[:, None] - bboxes[:, 1][None]
        r = bboxes[:, 2][None] - xs[:, None]
        b = bboxes[:, 3][None] - ys[:, None]
        reg = torch.stack([l, t, r, b], dim=2)
        if center_sample:                                                                 # :168-175
            inside = sample_region(bboxes, npl, xs, ys, radius)
        else:                                                                             # :176-177
            inside = reg.min(dim=2)[0] > 0
        mx = reg.max(dim=2)[0]
        cared = (mx >= soi[:, [0]]) & (mx <= soi[:, [1]])                                 # :180-184
        l2a = area[None].repeat(K, 1)
        l2a[inside == 0] = INF
        l2a[cared == 0] = INF
        min_area, inds = l2a.min(dim=1)                                                   # :186-196 (all-INF row: index 0)
        reg_i = reg[range(K), inds]
        lab = torch.ones(K, dtype=torch.int64)
        lab[min_area == INF] = 0
        labels_all.append(torch.split(lab, npl, dim=0))
        reg_all.append(torch.split(reg_i, npl, dim=0))
    labels = torch.cat([torch.cat([li[lvl] for li in labels_all], 0) for lvl in range(len(npl))], 0)
    regs = torch.cat([torch.cat([ri[lvl] for ri in reg_all], 0) for lvl in range(len(npl))], 0)
    return labels, regs


def iou_loss(pred, target, weight, loc_loss_type="giou", reduce=True):
    """layers/iou_loss.py:10-49.  reduce=False: the per-location losses (before the weighted / plain mean of :45-49)."""
    if loc_loss_type not in LOC_LOSS_TYPES:
        raise ValueError("loc_loss_type %r" % (loc_loss_type,))
    pl, pt, pr, pb = pred[:, 0], pred[:, 1], pred[:, 2], pred[:, 3]
    tl, tt, tr, tb = target[:, 0], target[:, 1], target[:, 2], target[:, 3]
    target_area = (tl + tr) * (tt + tb)
    pred_area = (pl + pr) * (pt + pb)
    w_int = torch.min(pl, tl) + torch.min(pr, tr)
    g_w = torch.max(pl, tl) + torch.max(pr, tr)
    h_int = torch.min(pb, tb) + torch.min(pt, tt)
    g_h = torch.max(pb, tb) + torch.max(pt, tt)
    ac = g_w * g_h + 1e-7
    a_int = w_int * h_int
    a_union = target_area + pred_area - a_int
    ious = (a_int + 1.0) / (a_union + 1.0)                                                # :34
    gious = ious - (ac - a_union) / ac
    if loc_loss_type == "iou":
        losses = -torch.log(ious)
    elif loc_loss_type == "linear_iou":
        losses = 1 - ious
    else:
        losses = 1 - gious
    if not reduce:
        return losses
    if weight is not None and weight.sum() > 0:
        return (losses * weight).sum() / weight.sum()
    return losses.mean()


def fcos_loss(logits, bbox_reg, centerness, gt_boxes_per_image, gamma=2.0, alpha=0.25, focal="cuda", center_sample=True,
              loc_loss_type="giou"):
    """FCOSLossComputation.__call__, loss.py:213-276, NCHW head outputs per level -> (cls, reg, centerness, info).  focal as in
    orc.fcos_loss.  info also holds the un-normalised sums the device kernel accumulates: {num_pos, sum_w, sum_focal,
    sum_w * loc_loss, sum_bce} (float64)."""
    N = logits[0].shape[0]
    locations = orc.compute_locations([tuple(t.shape[-2:]) for t in logits])
    labels, reg_t = fcos_targets(locations, gt_boxes_per_image, center_sample)
    cls_f = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, 1) for t in logits], 0)
    reg_f = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, 4) for t in bbox_reg], 0)
    ctr_f = torch.cat([t.permute(0, 2, 3, 1).reshape(-1) for t in centerness], 0)
    pos = torch.nonzero(labels > 0).squeeze(1)
    fl = orc.sigmoid_focal_loss_cuda_formula if focal == "cuda" else orc.sigmoid_focal_loss_cpu_formula
    focal_sum = fl(cls_f, labels.int(), gamma, alpha).sum()
    cls_loss = focal_sum / (pos.numel() + N)                                              # :251-254
    reg_p, reg_tp, ctr_p = reg_f[pos], reg_t[pos], ctr_f[pos]
    sums = [float(pos.numel()), 0.0, float(focal_sum.detach().double()), 0.0, 0.0]
    if pos.numel() > 0:
        ct = orc.centerness_targets(reg_tp)
        reg_loss = iou_loss(reg_p, reg_tp, ct, loc_loss_type)
        ctr_loss = F.binary_cross_entropy_with_logits(ctr_p, ct)
        with torch.no_grad():
            per = iou_loss(reg_p.double(), reg_tp.double(), None, loc_loss_type, reduce=False)
            sums[1] = float(ct.double().sum())
            sums[3] = float((per * ct.double()).sum())
            sums[4] = float(F.binary_cross_entropy_with_logits(ctr_p.double(), ct.double(), reduction="sum"))
    else:
        if loc_loss_type not in LOC_LOSS_TYPES:
            raise ValueError("loc_loss_type %r" % (loc_loss_type,))
        reg_loss, ctr_loss = reg_p.sum(), ctr_p.sum()
    return cls_loss, reg_loss, ctr_loss, dict(labels=labels, reg_targets=reg_t, num_pos=int(pos.numel()), sums=sums)
