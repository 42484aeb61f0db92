"""Generate the fixtures of the second stage's classification-loss modes (FEW_SHOT.SECOND_STAGE_CLS_LOSS 'ce_loss', 'focal_loss',
'mse_loss') from the REAL reference (build container only).

    python tests/golden/make_golden_box_cls_modes.py

1. box_cls_modes.npz — the reference's FastRCNNLossComputation.__call__ (modeling/roi_heads/box_head/loss.py:306-393) and
   PostProcessor.forward (box_head/inference.py:46-103), built from the config of record with FEW_SHOT.SECOND_STAGE_CLS_LOSS
   overridden, on small hand-made predictor outputs.  The restatement tests/box_cls_loss_ref.py must agree with the reference's
   losses within 1e-5 * max(1, |loss|) (CPU focal formula; make_golden.py's bound for this comparison) before anything is written.
   Every input is rounded to bfloat16 first (and stored as float32), so the fp32 and the bf16 kernels are given the same numbers.
     loss.<case>.logits2 [M, 2] / .logits1 [M, 1] (the 'ce_loss' / one-logit class logits), .deltas [M, 8], .labels [M] int32,
       .targets [M, 4], .counts [n] int32, .S: M = n * S rows, image i's valid rows are its first counts[i].  Rows past the count
       hold label 1 and arbitrary numbers on purpose (a kernel must not look at them); the reference is given the valid rows only.
     loss.<case>.<mode>.losses_ref [2] float64: (classification, box regression) as the reference returns them, i.e. BEFORE the
       weights 5 / 2.5 of box_head.py:193-194 and, for 'focal_loss', with the CPU formula (log(p + 1e-6)),
     loss.<case>.<mode>.losses_f64 [2]: the restatement in float64 ('focal_loss': the CUDA formula, which the kernel computes),
     loss.<case>.<mode>.n_pos,
     loss.<case>.<mode>.grad_logits [M, L], loss.<case>.grad_deltas [M, 8] (the same in every mode): reference autograd of
       5 * classification + 2.5 * box regression (zero rows past the count),
     loss.<case>.focal_loss.grad_logits_f64 [M, 1]: the restatement's float64 autograd with the CUDA formula.
     decode.<mode>.*: logits [S=1, N*R, L], deltas [N*R, 8], rois [N, R, 4], counts [N], image_size (h, w) -> scores [N, R] (class-1
       probability, -1 past the count) and boxes [N, R, 4] (class-1 box) of the reference after clip_to_image, before NMS.
2. box_small_focal.npz / boxtrain_small_focal.npz — the `small` geometry end to end with a 'focal_loss' model: what make_golden.py's
   gen_box_case / gen_box_train_case record for 'ce_loss' (box_small.npz / boxtrain_small.npz), made the same way from a reference
   model built with the override and loaded with synth weights of spec.full_model_shapes(box_cls_loss="focal_loss").  The training
   file also holds losses_cuda_formula (restatement) next to the reference's CPU-formula losses; the feature gradients come from
   the oracle's differentiable forward + the restatement of the loss.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                  # noqa: E402  (sets up sys.path for the package, the oracle and the tests' helpers)
import golden_utils as gu                 # noqa: E402
import ref_harness as rh                  # noqa: E402
import box_cls_loss_ref as bcl            # noqa: E402
from oneshotdet_amd import spec, synth    # noqa: E402
from oracle import box_head_ref as obh    # noqa: E402
from oracle import box_train_ref as obt   # noqa: E402
from oracle import hotpath_ref as orc     # noqa: E402

# name -> (images n, rows per image S, valid rows per image, labels of the valid rows: "mixed" / 0 / 1)
LOSS_CASES = {
    "mixed": (2, 8, (8, 5), "mixed"),
    "nopos": (1, 4, (4,), 0),              # max(n_pos, 1) of the focal loss; mean label 0 of the mse loss
    "allpos": (1, 4, (4,), 1),
    "large": (9, 128, (128,) * 9, "mixed"),   # M = 1152 > the 1024 threads of the loss kernel: the row loop's second trip
}
DECODE = dict(n=2, rois=5, counts=(5, 3), image_size=(240, 320))


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float32)


def make_cfg(cls_loss):
    from maskrcnn_benchmark.config import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(rh.REFERENCE_ROOT, rh.CONFIG_OF_RECORD))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.WEIGHT", "", "FEW_SHOT.SECOND_STAGE_CLS_LOSS", cls_loss])
    cfg.freeze()
    return cfg


def loss_inputs(name):
    n, S, counts, kind = LOSS_CASES[name]
    M = n * S
    rng = np.random.RandomState(len(name) * 100 + M)
    valid = np.concatenate([np.arange(S) < c for c in counts])
    if kind == "mixed":
        labels = (rng.rand(M) < 0.3).astype(np.int32)
        labels[0], labels[1] = 1, 0
    else:
        labels = np.full(M, kind, np.int32)
    labels[~valid] = 1                                   # past the count: must not be counted as positives
    logits2 = bf16_round(rng.randn(M, 2) * 1.5)
    logits1 = bf16_round(rng.randn(M, 1) * 1.5)
    deltas = bf16_round(rng.randn(M, 8) * 1.5)
    targets = bf16_round(rng.randn(M, 4))
    if kind == "mixed":                                  # a smooth-L1 difference of exactly 1 and one beyond it
        deltas[0, 4], targets[0, 0] = 2.0, 1.0
        deltas[0, 5], targets[0, 1] = -3.0, 0.5
    return dict(logits2=logits2, logits1=logits1, deltas=deltas, labels=torch.from_numpy(labels), targets=targets,
                counts=np.asarray(counts, np.int32), S=S, valid=torch.from_numpy(valid))


def run_reference_loss(cfg, logits, deltas, labels, targets):
    from maskrcnn_benchmark.modeling.roi_heads.box_head.loss import make_roi_box_loss_evaluator
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    ev = make_roi_box_loss_evaluator(cfg)
    bl = BoxList(torch.zeros(len(labels), 4), (64, 64), mode="xyxy")
    bl.add_field("labels", labels.to(torch.int64))
    bl.add_field("regression_targets", targets)
    ev._proposals = [bl]
    lg, dl = logits.clone().requires_grad_(True), deltas.clone().requires_grad_(True)
    lc, lb = ev([lg], [dl])
    (bcl.W_CLS * lc + bcl.W_BOX * lb).backward()
    return lc, lb, lg.grad, (dl.grad if dl.grad is not None else torch.zeros_like(dl))


def gen_loss_cases(out):
    for name in LOSS_CASES:
        d = loss_inputs(name)
        v = d["valid"]
        M = len(v)
        for k in ("logits2", "logits1", "deltas", "targets"):
            out["loss.%s.%s" % (name, k)] = mg.t2n(d[k])
        out["loss.%s.labels" % name] = d["labels"].numpy().astype(np.int32)
        out["loss.%s.counts" % name] = d["counts"]
        out["loss.%s.S" % name] = np.int64(d["S"])
        labels_v = d["labels"][v].to(torch.int64)
        for mode in bcl.CLS_LOSSES:
            cfg = make_cfg(mode)
            assert cfg.FEW_SHOT.SECOND_STAGE_CLS_LOSS == mode and not cfg.FEW_SHOT.SOFT_LABELING and not cfg.FEW_SHOT.LOSS_WEIGHTED
            logits = d["logits2" if mode == "ce_loss" else "logits1"]
            lc, lb, g_log, g_del = run_reference_loss(cfg, logits[v], d["deltas"][v], labels_v, d["targets"][v])
            # restatement, fp32, the formula the reference evaluated
            oc, ob = bcl.losses(logits[v], d["deltas"][v], labels_v, d["targets"][v], mode, focal="cpu")
            for a, b, w in ((lc, oc, bcl.W_CLS), (lb, ob, bcl.W_BOX)):
                assert abs(w * a.item() - b.item()) <= 1e-5 * max(1.0, abs(w * a.item())), (name, mode, a.item(), b.item() / w)
            # restatement, float64, the formula the kernel computes
            lg64 = logits[v].double().requires_grad_(True)
            dl64 = d["deltas"][v].double().requires_grad_(True)
            fc, fb = bcl.losses(lg64, dl64, labels_v, d["targets"][v].double(), mode, focal="cuda")
            (fc + fb).backward()
            if mode == "mse_loss":                       # the closed form of the [M, M] broadcast and its gradient (module docstring)
                cf = bcl.mse_loss_closed_form(logits[v].double(), labels_v)
                assert abs(cf.item() - lc.item()) <= 1e-6 * max(1.0, abs(lc.item())), (name, cf.item(), lc.item())
                s = torch.sigmoid(logits[v].double().reshape(-1))
                gcf = bcl.W_CLS * (2.0 / len(s)) * (s - labels_v.double().mean()) * s * (1 - s)
                assert (gcf - g_log.reshape(-1).double()).abs().max().item() <= 1e-7, name
                if len(s) > 1 and 0 < int(labels_v.sum()) < len(s):   # it is NOT the row-wise mean
                    rowwise = ((s - labels_v.double()) ** 2).mean().item()
                    assert abs(rowwise - lc.item()) > 1e-3, (name, rowwise, lc.item())
            n_pos = int((labels_v > 0).sum())
            key = "loss.%s.%s" % (name, mode)
            out[key + ".losses_ref"] = np.array([lc.item(), lb.item()], np.float64)
            out[key + ".losses_f64"] = np.array([fc.item() / bcl.W_CLS, fb.item() / bcl.W_BOX], np.float64)
            out[key + ".n_pos"] = np.int64(n_pos)
            full = torch.zeros(M, logits.shape[1])
            full[v] = g_log
            out[key + ".grad_logits"] = mg.t2n(full)
            full = torch.zeros(M, 8)
            full[v] = g_del
            if "loss.%s.grad_deltas" % name in out:      # the regression loss does not depend on the mode
                assert np.array_equal(out["loss.%s.grad_deltas" % name], mg.t2n(full)), (name, mode)
            out["loss.%s.grad_deltas" % name] = mg.t2n(full)
            if mode == "focal_loss":
                full = torch.zeros(M, 1, dtype=torch.float64)
                full[v] = lg64.grad
                out[key + ".grad_logits_f64"] = mg.t2n(full)
            print("loss %-6s %-10s reference %.7f %.7f | float64 restatement %.7f %.7f  n_pos %d of %d"
                  % (name, mode, lc.item(), lb.item(), fc.item() / bcl.W_CLS, fb.item() / bcl.W_BOX, n_pos, int(v.sum())))


def gen_decode_cases(out):
    from maskrcnn_benchmark.modeling.roi_heads.box_head.inference import make_roi_box_post_processor
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    n, R, counts, (ih, iw) = DECODE["n"], DECODE["rois"], DECODE["counts"], DECODE["image_size"]
    rng = np.random.RandomState(77)
    xy = rng.rand(n, R, 2) * np.array([200.0, 140.0])
    rois = bf16_round(np.concatenate([xy, xy + rng.rand(n, R, 2) * 150 + 1], -1))
    deltas = bf16_round(rng.randn(n * R, 8) * 3.0)
    deltas[1, 6] = 60.0                                  # dw / 5 beyond log(1000 / 16): clamped (box_coder.py:19,75-76)
    for mode in bcl.CLS_LOSSES:
        L = bcl.n_logits(mode)
        logits = bf16_round(rng.randn(n * R, L) * 2.0)
        logits[0, L - 1], logits[1, L - 1] = 1.5, -1.5   # both sides of 0 for certain
        pp = make_roi_box_post_processor(make_cfg(mode))
        pp.filter_results = lambda boxlist, num_classes, target_id=None: boxlist          # after clip_to_image, before NMS
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
        # restatement
        rs = bcl.scores(logits, mode).reshape(n, R).numpy()
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


def load_synth_weights(model, mode, seed=0):
    full = spec.full_model_shapes(box_cls_loss=mode)
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(full.keys()), "spec.full_model_shapes(box_cls_loss=%r) key list differs from the reference" % mode
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(full[k]), (k, tuple(v.shape), full[k])
    np_sd = synth.make_state_dict(full, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np_sd.items()}, strict=True)
    return np_sd


def gen_box_case(model, np_sd, name, mode):
    """make_golden.py gen_box_case in the mode `mode` (one shot)."""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    B, H, W, S, qh, qw = gu.CASES[name]
    assert S == 1
    img_np, q_np = gu.case_inputs(name)
    cap = mg.run_reference(model, torch.from_numpy(img_np), torch.from_numpy(q_np), B)
    feats, qfeats = list(cap["features"]), list(cap["query_features"])
    rmin = min(len(bl) for bl in cap["proposals"])
    props = [bl[:rmin] for bl in cap["proposals"]]
    grabbed = {}

    def grab_pred(m, i, o):
        grabbed["logits"], grabbed["reg"] = o[0], o[1]

    def grab_x(m, i, o):
        grabbed["x"] = o
    hooks = [model.roi_heads.box.predictor.register_forward_hook(grab_pred),
             model.roi_heads.box.feature_extractor.register_forward_hook(grab_x)]
    model.eval()
    with torch.no_grad():
        supp_boxes = [BoxList([[0, 0, qh, qw]], image_size=(qh, qw), mode="xyxy") for _ in range(B * S)]
        supp_roi = model.supproi_pooling(qfeats, supp_boxes)
        _, result, _ = model.roi_heads(feats, props, None, supp_roi, target_ids=[1] * B)
    for h in hooks:
        h.remove()
    sd = orc.to_torch_state_dict(np_sd)
    with torch.no_grad():
        ol, oreg, opooled = obh.box_head_logits(feats, qfeats, [bl.bbox for bl in props], [(qh, qw)] * (B * S), sd)
        odet = bcl.postprocess(ol, oreg, [bl.bbox for bl in props], [(H, W)] * B, mode)
        o_supp = obh.query_roi_features(qfeats, [(qh, qw)] * (B * S))
    assert tuple(grabbed["logits"].shape) == (B * rmin, bcl.n_logits(mode)) and grabbed["reg"].shape[1] == 8
    err = {"supp_roi": (o_supp - supp_roi).abs().max().item() / max(supp_roi.abs().max().item(), 1e-6),
           "pooled": (opooled - grabbed["x"]).abs().max().item() / max(grabbed["x"].abs().max().item(), 1e-6),
           "logits": (ol - grabbed["logits"]).abs().max().item(), "reg": (oreg - grabbed["reg"]).abs().max().item()}
    print(name, mode, "box head: R=%d per image, oracle-vs-reference:" % rmin, {k: "%.2e" % v for k, v in err.items()})
    assert err["supp_roi"] < 1e-5 and err["pooled"] < 1e-5 and err["logits"] < 2e-4 and err["reg"] < 2e-4, err
    out = {"image_size": np.asarray([H, W], dtype=np.int64), "logits": mg.t2n(grabbed["logits"]),
           "box_regression": mg.t2n(grabbed["reg"]), "n_shots_outputs": np.int64(1)}
    out.update(gu.checksum(mg.t2n(grabbed["x"]).reshape(B * rmin, -1, 7, 7), "pooled"))
    out.update(gu.checksum(mg.t2n(supp_roi).reshape(B * S, -1, 7, 7), "supp_roi"))
    for i, bl in enumerate(result):
        rb, rs = mg.t2n(bl.bbox), mg.t2n(bl.get_field("scores"))
        ob, os_ = mg.t2n(odet[i][0]), mg.t2n(odet[i][1])
        frac = gu.match_boxes(rb, rs, ob, os_)
        print("  image %d: reference %d detections, restatement %d, overlap %.4f" % (i, len(rb), len(ob), frac))
        assert len(rb) == len(ob) and frac >= 0.999, (len(rb), len(ob), frac)
        order = np.argsort(-rs, kind="stable")
        out["proposals.%d.boxes" % i] = mg.t2n(props[i].bbox)
        out["detections.%d.boxes" % i] = rb[order]
        out["detections.%d.scores" % i] = rs[order]
    path = os.path.join(HERE, "box_%s_%s.npz" % (name, mode.split("_")[0]))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def gen_box_train_case(model, np_sd, name, mode):
    """make_golden.py gen_box_train_case in the mode `mode`."""
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
        sm = obt.subsample(props[i].bbox, torch.from_numpy(gts[i]), k)
        _, p1, p2 = obt.sample(sm["all_labels"], k)
        samp.append(sm)
        perms += [p1, p2]
    assert len({len(sm["index"]) for sm in samp}) == 1
    it = iter(perms)
    orig_randperm = torch.randperm

    def recorded_randperm(n, **kw):
        p = next(it)
        assert len(p) == n, (len(p), n)
        return p.clone()
    torch.randperm = recorded_randperm
    try:
        model.train()
        model.zero_grad()
        with torch.no_grad():
            supp_boxes = [BoxList([[0, 0, qh, qw]], image_size=(qh, qw), mode="xyxy") for _ in range(B * S)]
            supp_roi = model.supproi_pooling(qfeats, supp_boxes)
        x, sampled_props, loss_dict = model.roi_heads(feats, [p for p in props], targets, supp_roi, target_ids=[1] * B)
    finally:
        torch.randperm = orig_randperm
    lc, lb = loss_dict["loss_classifier"], loss_dict["loss_box_reg"]
    (lc + lb).backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.eval()
    for i, (bl, sm) in enumerate(zip(sampled_props, samp)):
        assert torch.equal(bl.bbox, sm["boxes"]) and torch.equal(bl.get_field("labels"), sm["labels"]), (name, i)
        assert torch.equal(bl.get_field("regression_targets"), sm["targets"]), (name, i)
    labels = torch.cat([s["labels"] for s in samp])
    tg = torch.cat([s["targets"] for s in samp])

    def restated(focal, with_grad):
        sd = orc.to_torch_state_dict(np_sd)
        for k in sd:
            if k.startswith("roi_heads.box."):
                sd[k].requires_grad_(with_grad)
        fg = [f.clone().requires_grad_(with_grad) for f in feats]
        qg = [f.clone().requires_grad_(with_grad) for f in qfeats]
        qf = [q.view(B, S, *q.shape[1:])[:, 0] for q in qg]
        logits, reg, _ = obh.box_head_logits(fg, qf, [s["boxes"] for s in samp], [(qh, qw)] * B, sd)
        a, b = bcl.losses(logits, reg, labels, tg, mode, focal=focal)
        if with_grad:
            (a + b).backward()
        return a, b, sd, fg, qg
    with torch.no_grad():
        cc, cb, _, _, _ = restated("cpu", False)
    assert abs(lc.item() - cc.item()) <= 1e-5 * max(1.0, abs(lc.item())) and abs(lb.item() - cb.item()) <= 1e-5 * max(1.0, abs(lb.item()))
    olc, olb, sd, fg, qg = restated("cuda", True)
    print(name, mode, "box train: %d sampled per image (%d positives), losses ref %.6f %.6f | restatement (cuda formula) %.6f %.6f"
          % (len(samp[0]["index"]), int((labels > 0).sum()), lc.item(), lb.item(), olc.item(), olb.item()))
    worst = 0.0
    for k, g in ref_grads.items():
        if k.startswith("roi_heads.box."):
            worst = max(worst, (sd[k].grad - g).abs().max().item() / max(g.abs().max().item(), 1e-12))
    print("   worst relative parameter-gradient error restatement-vs-reference: %.2e" % worst)
    assert worst < 1e-3, worst
    out = {"losses": np.array([lc.item(), lb.item()], dtype=np.float64),
           "losses_cuda_formula": np.array([olc.item(), olb.item()], dtype=np.float64),
           "n_props": np.asarray([len(p) for p in props], np.int64), "n_sampled": np.int64(len(samp[0]["index"]))}
    for i in range(B):
        out["props.%d" % i] = mg.t2n(props[i].bbox)
        out["gt.%d" % i] = gts[i]
        out["index.%d" % i] = mg.t2n(samp[i]["index"]).astype(np.int32)
        out["labels.%d" % i] = mg.t2n(sampled_props[i].get_field("labels")).astype(np.int32)
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
    gen_loss_cases(out)
    gen_decode_cases(out)
    # the reference's predictor shapes in every mode (roi_box_predictors.py:47-50,66-68,76-77)
    for mode in bcl.CLS_LOSSES:
        model, cfg = rh.build_reference_model(["FEW_SHOT.SECOND_STAGE_CLS_LOSS", mode])
        p = model.roi_heads.box.predictor
        out["shapes.%s" % mode] = np.asarray([list(p.cls_score.weight.shape), [p.cls_score.bias.shape[0], 0],
                                              list(p.bbox_pred.weight.shape), [p.bbox_pred.bias.shape[0], 0]], np.int64)
        if mode == "focal_loss":
            np_sd = load_synth_weights(model, mode)
            gen_box_case(model, np_sd, "small", mode)
            gen_box_train_case(model, np_sd, "small", mode)
    path = os.path.join(HERE, "box_cls_modes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
