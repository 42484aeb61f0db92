"""Generate the fixtures of the second stage's IoU soft labels (FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC) and of the losses that
read them ('mse_loss' with soft labels, 'l1_loss', 'cxe_loss') from the REAL reference (build container only).

    python tests/golden/make_golden_box_soft_labels.py

1. box_soft_labels.npz — the reference's FastRCNNLossComputation.subsample / __call__ (modeling/roi_heads/box_head/loss.py:234-292,
   306-393) and PostProcessor.forward (box_head/inference.py:46-103), built from the config of record with FEW_SHOT.SOFT_LABELING True
   and the function / loss overridden.  The restatement tests/box_soft_label_ref.py must agree with the reference (sampled rows and
   labels exactly, soft labels bit for bit, losses within 1e-5 * max(1, |loss|): the existing makers' bound) before anything is
   written.  Every input is rounded to bfloat16 first (and stored as float32).
     match.<case>.props [N, P, 4], .counts [N], .gt [N, G, 4], .gt_count [N], .keys [N, P], .thresh, .batch, .fraction: the inputs of
       the sampler (randperm := argsort(keys), as tests/golden/boxtrain_*.npz).  Cases: `iou` = one image, one 10 x 10 ground truth and 12
       proposals with the IoUs 1, 0.5, 0.1, 0.3, 0.07, 0.03, 0, 0.7, 0.25, 0.4, 0, 0.9 at the thresholds of record (0.5); `iou_low` = the
       same with FG_IOU_THRESHOLD = BG_IOU_THRESHOLD = 0.05, which reaches the middle / 4th-order branches and makes the two trans*
       functions differ (both with BATCH_SIZE_PER_IMAGE 12 and POSITIVE_FRACTION 0.75: every proposal is sampled); `wide` = three images
       with P = 1100 > the kernel's 1,024 threads, counts (1100, 700, 500), the third WITHOUT ground truth: the reference's matcher
       raises for it (matcher.py:53-58; recorded as match.wide.reference_raises_without_gt), so its rows are the kernel's documented
       answer: nothing sampled, count 0.
     match.<case>.<func>.index / .labels / .soft [N, S] (-1 / -1 / 0 past .count [N]), .all_soft [N, P]: what subsample returned.
     loss.<case>.*: the four shapes of box_cls_modes.npz (the same logits, deltas, labels, targets) plus .soft [M]: uniform in [0, 1]
       where the label is 1, 0 where it is 0; rows past the count hold soft label 0.7 and label 1 on purpose.  `mixed` row 0 has logit
       exactly 0 and soft label exactly 0.5: sign(0) of the l1 gradient.
     loss.<case>.<mode>.losses_ref [2] (reference, before the weights 5 / 2.5), .losses_f64 [2] (restatement in float64),
       .grad_logits [M, L] / loss.<case>.grad_deltas [M, 8] (reference autograd of 5 * cls + 2.5 * box, zero rows past the count),
       .grad_logits_f64 (the closed-form gradient in float64, x 5).
     decode.<mode>.* for 'l1_loss' / 'cxe_loss': as box_cls_modes.npz.   shapes.<mode>: the reference predictor's shapes.
2. boxtrain_small_cxe.npz — the `small` geometry end to end with a 'cxe_loss' + 'transLinear' model, made the way
   boxtrain_small_focal.npz was made (make_golden_box_cls_modes.gen_box_train_case), plus soft.<i>: the sampled rows' soft labels.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                  # noqa: E402  (sets up sys.path for the package, the oracle and the tests' helpers)
import make_golden_box_cls_modes as mcm   # noqa: E402
import golden_utils as gu                 # noqa: E402
import ref_harness as rh                  # noqa: E402
import box_cls_loss_ref as bcl            # noqa: E402
import box_soft_label_ref as bsl          # noqa: E402
from oneshotdet_amd import spec, synth    # noqa: E402
from oracle import box_head_ref as obh    # noqa: E402
from oracle import hotpath_ref as orc     # noqa: E402

E2E = ("cxe_loss", "transLinear")


def soft_opts(cls_loss, func="linear", extra=()):
    return ["FEW_SHOT.SECOND_STAGE_CLS_LOSS", cls_loss, "FEW_SHOT.SOFT_LABELING", True, "FEW_SHOT.SOFT_LABELING_FUNC", func] + list(extra)


def make_cfg(cls_loss, func="linear", extra=()):
    """make_golden_box_cls_modes.make_cfg plus the soft-label options."""
    from maskrcnn_benchmark.config import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(rh.REFERENCE_ROOT, rh.CONFIG_OF_RECORD))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.WEIGHT", ""] + soft_opts(cls_loss, func, extra))
    cfg.freeze()
    assert cfg.FEW_SHOT.SOFT_LABELING is True and cfg.FEW_SHOT.SOFT_LABELING_FUNC == func and not cfg.FEW_SHOT.LOSS_WEIGHTED
    return cfg


class recorded_randperm(object):
    """torch.randperm := the next recorded permutation (argsort of the sampler keys)."""

    def __init__(self, perms):
        self.it = iter(perms)

    def __enter__(self):
        self.orig = torch.randperm

        def rp(n, **kw):
            p = next(self.it)
            assert len(p) == n, (len(p), n)
            return p.clone()
        torch.randperm = rp

    def __exit__(self, *a):
        torch.randperm = self.orig


# ---- matcher / sampler ----------------------------------------------------------------------------------------------------------------

def iou_case():
    gt = np.array([[[10, 10, 19, 19]]], np.float32)
    props = np.array([[[10, 10, 19, 19], [10, 10, 19, 14], [10, 10, 19, 10], [10, 10, 19, 12], [10, 10, 16, 10], [10, 10, 12, 10],
                       [40, 40, 49, 49], [10, 10, 19, 16], [5, 5, 24, 24], [10, 10, 19, 13], [0, 0, 5, 5], [10, 10, 19, 18]]], np.float32)
    return props, np.array([12], np.int32), gt, np.array([1], np.int32)


def wide_case():
    rng = np.random.RandomState(11)
    N, P, G = 3, 1100, 3
    counts, gcnt = np.array([1100, 700, 500], np.int32), np.array([3, 2, 0], np.int32)
    gt = np.zeros((N, G, 4), np.float32)
    props = np.zeros((N, P, 4), np.float32)
    for i in range(N):
        xy = rng.rand(G, 2) * 120 + 8
        gt[i] = np.concatenate([xy, xy + rng.rand(G, 2) * 60 + 24], -1)
        base = gt[i][rng.randint(0, max(int(gcnt[i]), 1), P)]
        jit = rng.randn(P, 4) * np.where(rng.rand(P, 1) < 0.5, 6.0, 30.0)
        b = base + jit
        b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 2)
        props[i] = b
        if gcnt[i]:
            props[i, counts[i] - gcnt[i]:counts[i]] = gt[i, :gcnt[i]]           # the ground truth appended (t = 1)
    gt, props = mg.t2n(mcm.bf16_round(gt)), mg.t2n(mcm.bf16_round(props))
    for i in range(N):
        if gcnt[i]:
            props[i, counts[i] - gcnt[i]:counts[i]] = gt[i, :gcnt[i]]
        gt[i, gcnt[i]:] = 0
        props[i, counts[i]:] = 0
    return props, counts, gt, gcnt


MATCH_CASES = {       # name -> (inputs, threshold, BATCH_SIZE_PER_IMAGE, POSITIVE_FRACTION)
    "iou": (iou_case, 0.5, 12, 0.75),
    "iou_low": (iou_case, 0.05, 12, 0.75),
    "wide": (wide_case, 0.5, 128, 0.25),
}


def gen_match_cases(out):
    from maskrcnn_benchmark.modeling.roi_heads.box_head.loss import make_roi_box_loss_evaluator
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    for name, (inputs, thresh, batch, fraction) in MATCH_CASES.items():
        props, counts, gt, gcnt = inputs()
        N, P, _ = props.shape
        keys = synth.uniform01("softlabels.keys." + name, N * P, seed=5).reshape(N, P).astype(np.float32)
        key = "match.%s." % name
        out[key + "props"], out[key + "counts"], out[key + "gt"], out[key + "gt_count"], out[key + "keys"] = props, counts, gt, gcnt, keys
        out[key + "thresh"], out[key + "batch"], out[key + "fraction"] = np.float32(thresh), np.int64(batch), np.float64(fraction)
        extra = ["MODEL.ROI_HEADS.FG_IOU_THRESHOLD", thresh, "MODEL.ROI_HEADS.BG_IOU_THRESHOLD", thresh,
                 "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", batch, "MODEL.ROI_HEADS.POSITIVE_FRACTION", fraction]
        live = [i for i in range(N) if gcnt[i] > 0]
        for func in bsl.FUNCS:
            ev = make_roi_box_loss_evaluator(make_cfg("mse_loss", func, extra))
            if len(live) < N:       # the reference has no answer for an image without ground truth: its matcher raises
                i = [j for j in range(N) if gcnt[j] == 0][0]
                bl = BoxList(torch.from_numpy(props[i, :counts[i]]), (256, 256), mode="xyxy")
                tg = BoxList(torch.zeros(0, 4), (256, 256), mode="xyxy")
                tg.add_field("labels", torch.ones(0, dtype=torch.int64))
                try:
                    ev.subsample([bl], [tg])
                    raised = False
                except (ValueError, RuntimeError, IndexError):
                    raised = True
                assert raised
                out[key + "reference_raises_without_gt"] = np.bool_(True)
            rest, perms, bls, tgs = [], [], [], []
            for i in live:
                p_i, g_i = torch.from_numpy(props[i, :counts[i]]), torch.from_numpy(gt[i, :gcnt[i]])
                k_i = torch.from_numpy(keys[i, :counts[i]].copy())
                r = bsl.subsample(p_i, g_i, k_i, thresh, func, batch=batch, fraction=fraction)
                rest.append(r)
                perms += list(r["perms"])
                bl = BoxList(p_i.clone(), (256, 256), mode="xyxy")
                bl.add_field("idx", torch.arange(len(p_i)))
                tg = BoxList(g_i.clone(), (256, 256), mode="xyxy")
                tg.add_field("labels", torch.ones(len(g_i), dtype=torch.int64))
                bls.append(bl)
                tgs.append(tg)
            with recorded_randperm(perms):
                sampled = ev.subsample(bls, tgs)
            S = batch
            index = np.full((N, S), -1, np.int32)
            labels = np.full((N, S), -1, np.int32)
            soft = np.zeros((N, S), np.float32)
            all_soft = np.zeros((N, P), np.float32)
            cnt = np.zeros(N, np.int32)
            for i, bl, full, r in zip(live, sampled, bls, rest):
                k = len(bl)
                idx = bl.get_field("idx")
                # restatement == reference: rows and labels exactly, soft labels bit for bit
                assert torch.equal(idx, r["index"]) and torch.equal(bl.get_field("labels"), r["labels"]), (name, func, i)
                assert torch.equal(bl.get_field("soft_labels"), r["soft"]), (name, func, i)
                assert torch.equal(full.get_field("soft_labels"), r["all_soft"]), (name, func, i)
                assert bl.get_field("soft_labels").dtype == torch.float32
                index[i, :k], labels[i, :k], soft[i, :k], cnt[i] = idx.numpy(), bl.get_field("labels").numpy(), bl.get_field("soft_labels").numpy(), k
                all_soft[i, :counts[i]] = full.get_field("soft_labels").numpy()
                assert (soft[i, :k][labels[i, :k] == 0] == 0).all()
            fk = key + func + "."
            out[fk + "index"], out[fk + "labels"], out[fk + "soft"], out[fk + "all_soft"], out[fk + "count"] = index, labels, soft, all_soft, cnt
            print("match %-8s %-15s sampled %s positives %s soft (positives) %.4f .. %.4f"
                  % (name, func, cnt.tolist(), [(labels[i] > 0).sum() for i in range(N)],
                     soft[labels > 0].min(), soft[labels > 0].max()))
    a, b = out["match.iou_low.transLinear.soft"], out["match.iou_low.trans4thLinear.soft"]
    assert not np.array_equal(a, b) and np.array_equal(out["match.iou.transLinear.soft"], out["match.iou.trans4thLinear.soft"])
    # the 12 IoUs are the intended ones, exactly (float32)
    want = np.array([1, 0.5, 0.1, 0.3, 0.07, 0.03, 0, 0.7, 0.25, 0.4, 0, 0.9], np.float32)
    lin = out["match.iou_low.linear.all_soft"][0]
    assert np.array_equal(lin, np.where(want >= np.float32(0.05), want, 0).astype(np.float32)), lin
    mid = out["match.iou_low.transLinear.all_soft"][0]
    assert mid[4] == 0 and mid[2] > 0 and 0 < mid[3] < 0.9 and b[0].max() <= 1.0 and out["match.iou_low.trans4thLinear.all_soft"][0][4] > 0


# ---- losses ---------------------------------------------------------------------------------------------------------------------------

def loss_inputs(name):
    """make_golden_box_cls_modes.loss_inputs plus soft labels; 'cxe_loss' reads logits2, the one-logit losses logits1."""
    d = mcm.loss_inputs(name)
    M = len(d["valid"])
    rng = np.random.RandomState(len(name) * 7 + M)
    soft = mcm.bf16_round(rng.rand(M))
    soft[d["labels"] == 0] = 0.0
    soft[~d["valid"]] = 0.7                               # past the count: label 1 and a soft label, on purpose
    if name == "mixed":                                   # sigmoid(0) - 0.5 == 0 exactly: sign(0) of the l1 gradient
        assert int(d["labels"][0]) == 1
        d["logits1"][0, 0], soft[0] = 0.0, 0.5
    d["soft"] = soft
    return d


def run_reference_loss(cfg, logits, deltas, labels, soft, targets):
    from maskrcnn_benchmark.modeling.roi_heads.box_head.loss import make_roi_box_loss_evaluator
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    ev = make_roi_box_loss_evaluator(cfg)
    bl = BoxList(torch.zeros(len(labels), 4), (64, 64), mode="xyxy")
    bl.add_field("labels", labels.to(torch.int64))
    bl.add_field("soft_labels", soft)
    bl.add_field("regression_targets", targets)
    ev._proposals = [bl]
    lg, dl = logits.clone().requires_grad_(True), deltas.clone().requires_grad_(True)
    lc, lb = ev([lg], [dl])
    (bcl.W_CLS * lc + bcl.W_BOX * lb).backward()
    return lc, lb, lg.grad, (dl.grad if dl.grad is not None else torch.zeros_like(dl))


def gen_loss_cases(out):
    for name in mcm.LOSS_CASES:
        d = loss_inputs(name)
        v = d["valid"]
        M = len(v)
        for k in ("logits2", "logits1", "deltas", "targets", "soft"):
            out["loss.%s.%s" % (name, k)] = mg.t2n(d[k])
        out["loss.%s.labels" % name] = d["labels"].numpy().astype(np.int32)
        out["loss.%s.counts" % name] = d["counts"]
        out["loss.%s.S" % name] = np.int64(d["S"])
        labels_v, soft_v = d["labels"][v].to(torch.int64), d["soft"][v]
        for mode in bsl.SOFT_LOSSES:
            cfg = make_cfg(mode)
            logits = d["logits2" if mode == "cxe_loss" else "logits1"]
            lc, lb, g_log, g_del = run_reference_loss(cfg, logits[v], d["deltas"][v], labels_v, soft_v, d["targets"][v])
            oc, ob = bsl.losses(logits[v], d["deltas"][v], labels_v, soft_v, d["targets"][v], mode)
            for a, b, w in ((lc, oc, bcl.W_CLS), (lb, ob, bcl.W_BOX)):
                assert abs(w * a.item() - b.item()) <= 1e-5 * max(1.0, abs(w * a.item())), (name, mode, a.item(), b.item() / w)
            fc, fb = bsl.losses(logits[v].double(), d["deltas"][v].double(), labels_v, soft_v.double(), d["targets"][v].double(), mode)
            cf = bsl.closed_form(logits[v].double(), soft_v.double(), mode)
            assert abs(cf.item() * bcl.W_CLS - fc.item()) <= 1e-12 * max(1.0, abs(fc.item())), (name, mode)
            gcf = bcl.W_CLS * bsl.closed_form_grad(logits[v].double(), soft_v.double(), mode)
            assert (gcf - g_log.double()).abs().max().item() <= 1e-6, (name, mode, (gcf - g_log.double()).abs().max().item())
            key = "loss.%s.%s" % (name, mode)
            out[key + ".losses_ref"] = np.array([lc.item(), lb.item()], np.float64)
            out[key + ".losses_f64"] = np.array([fc.item() / bcl.W_CLS, fb.item() / bcl.W_BOX], np.float64)
            for tag, g in ((".grad_logits", g_log), (".grad_logits_f64", gcf)):
                full = torch.zeros(M, logits.shape[1], dtype=g.dtype)
                full[v] = g
                out[key + tag] = mg.t2n(full)
            full = torch.zeros(M, 8)
            full[v] = g_del
            if "loss.%s.grad_deltas" % name in out:
                assert np.array_equal(out["loss.%s.grad_deltas" % name], mg.t2n(full)), (name, mode)
            out["loss.%s.grad_deltas" % name] = mg.t2n(full)
            print("loss %-6s %-8s reference %.7f %.7f | float64 restatement %.7f | row-wise / full-CE value %.7f"
                  % (name, mode, lc.item(), lb.item(), fc.item() / bcl.W_CLS,
                     bsl.rowwise_value(logits[v].double(), soft_v.double(), mode).item()))


def gen_decode_cases(out):
    """make_golden_box_cls_modes.gen_decode_cases for the two names that exist with soft labels only."""
    from maskrcnn_benchmark.modeling.roi_heads.box_head.inference import make_roi_box_post_processor
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    n, R, counts, (ih, iw) = mcm.DECODE["n"], mcm.DECODE["rois"], mcm.DECODE["counts"], mcm.DECODE["image_size"]
    rng = np.random.RandomState(78)
    xy = rng.rand(n, R, 2) * np.array([200.0, 140.0])
    rois = mcm.bf16_round(np.concatenate([xy, xy + rng.rand(n, R, 2) * 150 + 1], -1))
    deltas = mcm.bf16_round(rng.randn(n * R, 8) * 3.0)
    deltas[1, 6] = 60.0
    for mode in spec.BOX_CLS_LOSSES_SOFT:
        L = bsl.n_logits(mode)
        logits = mcm.bf16_round(rng.randn(n * R, L) * 2.0)
        logits[0, L - 1], logits[1, L - 1] = 1.5, -1.5
        pp = make_roi_box_post_processor(make_cfg(mode))
        pp.filter_results = lambda boxlist, num_classes, target_id=None: boxlist
        valid = np.concatenate([np.arange(R) < c for c in counts])
        boxes = [BoxList(rois[i, :c], (iw, ih), mode="xyxy") for i, c in enumerate(counts)]
        vt = torch.from_numpy(valid)
        with torch.no_grad():
            res = pp((logits[vt], deltas[vt]), boxes, target_ids=[1] * n)
        scores = np.full((n, R), -1.0, np.float32)
        dec = np.zeros((n, R, 4), np.float32)
        for i, (bl, c) in enumerate(zip(res, counts)):
            scores[i, :c] = mg.t2n(bl.get_field("scores")).reshape(c, 2)[:, 1]
            dec[i, :c] = mg.t2n(bl.bbox).reshape(c, 2, 4)[:, 1]
        rs = bcl.scores(logits, bsl.decode_mode(mode)).reshape(n, R).numpy()
        rb = bcl.decode_clip(deltas, rois.reshape(-1, 4), (ih, iw)).reshape(n, R, 4).numpy()
        v2 = valid.reshape(n, R)
        assert np.abs(rs[v2] - scores[v2]).max() <= 1e-6 and np.abs(rb[v2] - dec[v2]).max() <= 1e-4, mode
        assert (scores[v2] > 0.5).any() and (scores[v2] < 0.5).any()
        key = "decode.%s." % mode
        out[key + "logits"] = mg.t2n(logits).reshape(1, n * R, L)
        out[key + "scores"], out[key + "boxes"] = scores, dec
        print("decode %-10s scores %.4f .. %.4f" % (mode, scores[v2].min(), scores[v2].max()))
    out["decode.deltas"], out["decode.rois"] = mg.t2n(deltas), mg.t2n(rois)
    out["decode.counts"] = np.asarray(counts, np.int32)
    out["decode.image_size"] = np.asarray([ih, iw], np.int64)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

def load_synth_weights(model, mode, seed=0):
    full = spec.full_model_shapes(box_cls_loss=mode, soft_labeling=True)
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(full.keys())
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(full[k]), (k, tuple(v.shape), full[k])
    np_sd = synth.make_state_dict(full, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np_sd.items()}, strict=True)
    return np_sd


def gen_box_train_case(model, np_sd, name, mode, func):
    """make_golden_box_cls_modes.gen_box_train_case with soft labels carried from the sampler to the loss."""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    B, H, W, S, qh, qw = gu.CASES[name]
    img_np, q_np = gu.case_inputs(name)
    cap = mg.run_reference(model, torch.from_numpy(img_np), torch.from_numpy(q_np), B)
    feats, qfeats = [f.detach() for f in cap["features"]], [f.detach() for f in cap["query_features"]]
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    targets = []
    for g in gts:
        bl = BoxList(torch.from_numpy(g), (W, H), mode="xyxy")
        bl.add_field("labels", torch.ones(len(g), dtype=torch.int64))
        targets.append(bl)
    props = model.rpn.box_selector_train.add_gt_proposals([bl for bl in cap["proposals"]], targets)
    pmax = max(len(p) for p in props)
    keys = synth.uniform01("boxtrain.keys." + name, B * pmax, seed=9).reshape(B, pmax).astype(np.float32)
    samp, perms = [], []
    for i in range(B):
        k = torch.from_numpy(keys[i, :len(props[i])].copy())
        sm = bsl.obt.subsample(props[i].bbox, torch.from_numpy(gts[i]), k)
        sm["soft"] = bsl.soft_labels(props[i].bbox, torch.from_numpy(gts[i]), bsl.obt.IOU_THRESH, func)[sm["index"]]
        _, p1, p2 = bsl.obt.sample(sm["all_labels"], k)
        samp.append(sm)
        perms += [p1, p2]
    assert len({len(sm["index"]) for sm in samp}) == 1
    with recorded_randperm(perms):
        model.train()
        model.zero_grad()
        with torch.no_grad():
            supp_boxes = [BoxList([[0, 0, qh, qw]], image_size=(qh, qw), mode="xyxy") for _ in range(B * S)]
            supp_roi = model.supproi_pooling(qfeats, supp_boxes)
        x, sampled_props, loss_dict = model.roi_heads(feats, [p for p in props], targets, supp_roi, target_ids=[1] * B)
    lc, lb = loss_dict["loss_classifier"], loss_dict["loss_box_reg"]
    (lc + lb).backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.eval()
    for i, (bl, sm) in enumerate(zip(sampled_props, samp)):
        assert torch.equal(bl.bbox, sm["boxes"]) and torch.equal(bl.get_field("labels"), sm["labels"]), (name, i)
        assert torch.equal(bl.get_field("regression_targets"), sm["targets"]), (name, i)
        assert torch.equal(bl.get_field("soft_labels"), sm["soft"]), (name, i)
    labels = torch.cat([s["labels"] for s in samp])
    soft = torch.cat([s["soft"] for s in samp])
    tg = torch.cat([s["targets"] for s in samp])

    def restated(with_grad):
        sd = orc.to_torch_state_dict(np_sd)
        for k in sd:
            if k.startswith("roi_heads.box."):
                sd[k].requires_grad_(with_grad)
        fg = [f.clone().requires_grad_(with_grad) for f in feats]
        qg = [f.clone().requires_grad_(with_grad) for f in qfeats]
        qf = [q.view(B, S, *q.shape[1:])[:, 0] for q in qg]
        logits, reg, _ = obh.box_head_logits(fg, qf, [s["boxes"] for s in samp], [(qh, qw)] * B, sd)
        a, b = bsl.losses(logits, reg, labels, soft, tg, mode)
        if with_grad:
            (a + b).backward()
        return a, b, sd, fg, qg
    olc, olb, sd, fg, qg = restated(True)
    assert abs(lc.item() - olc.item()) <= 1e-5 * max(1.0, abs(lc.item())) and abs(lb.item() - olb.item()) <= 1e-5 * max(1.0, abs(lb.item()))
    print(name, mode, func, "box train: %d sampled per image (%d positives, soft %.3f .. %.3f), losses ref %.6f %.6f | restatement %.6f %.6f"
          % (len(samp[0]["index"]), int((labels > 0).sum()), soft[labels > 0].min(), soft[labels > 0].max(), lc.item(), lb.item(),
             olc.item(), olb.item()))
    worst = 0.0
    for k, g in ref_grads.items():
        if k.startswith("roi_heads.box."):
            worst = max(worst, (sd[k].grad - g).abs().max().item() / max(g.abs().max().item(), 1e-12))
    print("   worst relative parameter-gradient error restatement-vs-reference: %.2e" % worst)
    assert worst < 1e-3, worst
    out = {"losses": np.array([lc.item(), lb.item()], dtype=np.float64),
           "n_props": np.asarray([len(p) for p in props], np.int64), "n_sampled": np.int64(len(samp[0]["index"]))}
    for i in range(B):
        out["props.%d" % i] = mg.t2n(props[i].bbox)
        out["gt.%d" % i] = gts[i]
        out["index.%d" % i] = mg.t2n(samp[i]["index"]).astype(np.int32)
        out["labels.%d" % i] = mg.t2n(sampled_props[i].get_field("labels")).astype(np.int32)
        out["soft.%d" % i] = mg.t2n(sampled_props[i].get_field("soft_labels"))
        out["targets.%d" % i] = mg.t2n(sampled_props[i].get_field("regression_targets"))
    for k in mg.BOXTRAIN_GRAD_KEYS:
        g = mg.t2n(ref_grads[k]).reshape(-1)
        idx = gu.sample_indices(g.size, "boxgrad." + k)[:256]
        out["refgrad.%s.samples" % k] = g[idx]
        out["refgrad.%s.absmax" % k] = np.float32(np.abs(g).max())
    for lvl in range(5):
        for tag, t in (("dfeat", fg[lvl]), ("dqfeat", qg[lvl])):
            g = mg.t2n(t.grad) if t.grad is not None else np.zeros(tuple(t.shape), np.float32)
            out.update(gu.checksum(g, "oracle_only.%s.%d" % (tag, lvl)))
    path = os.path.join(HERE, "boxtrain_%s_%s.npz" % (name, mode.split("_")[0]))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    torch.set_num_threads(8)
    rh.load_reference()
    out = {}
    gen_match_cases(out)
    gen_loss_cases(out)
    gen_decode_cases(out)
    for mode in bsl.SOFT_LOSSES:
        func = E2E[1] if mode == E2E[0] else "linear"
        model, cfg = rh.build_reference_model(soft_opts(mode, func))
        p = model.roi_heads.box.predictor
        out["shapes.%s" % mode] = np.asarray([list(p.cls_score.weight.shape), [p.cls_score.bias.shape[0], 0],
                                              list(p.bbox_pred.weight.shape), [p.bbox_pred.bias.shape[0], 0]], np.int64)
        if mode == E2E[0]:
            np_sd = load_synth_weights(model, mode)
            gen_box_train_case(model, np_sd, "small", mode, func)
    path = os.path.join(HERE, "box_soft_labels.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
