"""Generate the query augmentation fixtures (FEW_SHOT.SUPP_AUG, SUPP_AUG_METHOD 'avg' / 'max') from the REAL reference (build container
only).

    python tests/golden/make_golden_supp_aug.py

The reference model is built with FEW_SHOT.SUPP_AUG True, NUM_SUPP_AUG 1 and SUPP_AUG_METHOD 'avg' or 'max' (generalized_rcnn.py:73-74,
235-294: the query pyramid is split into groups of NUM_SUPP_AUG + 1 consecutive maps and every group merged before any pooling),
loaded with oneshotdet_amd.synth weights by key and recorded like make_golden / make_golden_shared / make_golden_avgpool.  The queries
are each case's queries, every one followed by its horizontal flip: the rows the dataset yields with supp_aug=True (coco.py:343-349).
oracle/ does not restate the merge: this script puts the two lines of torch (supp_aug_ref.merge) in front of `hotpath_ref.query_pool`
for its own process, and oracle and reference must agree, at make_golden_avgpool.record_first_stage's thresholds, before anything is
written.

Forward: case_suppaug_{avg,max}_{small,nonsquare,shots5}.npz and case_suppaug_shared_max_small.npz (FEW_SHOT.SIAMESE_BACKBONE False).
`query_features.*` are the MERGED maps (what the reference hands to supp_pooling), `query_features_unmerged.*` the query backbone's.
Training: train_suppaug_{avg,max}_small.npz with the ROIAlign pooling (no CPU backward in the reference: its gradients with the pooled
vector detached, the oracle's full gradients beside them, as make_golden.gen_train_case) and train_suppaug_max_nonsquare.npz with
FEW_SHOT.SUPP_ROIALIGN False (AdaptiveAvgPool2d has a CPU backward: the reference's OWN gradients of both backbones, torch's max
backward included, as make_golden_avgpool.gen_train_case).  Second stage: box_suppaug_max_small.npz, the reference's full eval forward
with roi_heads, recorded like box_small.npz.

Near ties under 'max' decide which member a gradient goes to.  Every 'max' fixture stores, per level, the number of elements whose
top-two gap is below 1e-6 of the level's absmax (asserted 0 on levels of at most 4 pixels per map, where one flipped element is a whole
row of a weight gradient), the share below 1e-4 and the share of elements member 0 wins.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                 # noqa: E402  (sets up sys.path for the package, the oracle and golden_utils)
import make_golden_avgpool as mga        # noqa: E402
import make_golden_shared as mgs         # noqa: E402
import golden_utils as gu                # noqa: E402
import ref_harness as rh                 # noqa: E402
import supp_aug_ref as sar               # noqa: E402
from oneshotdet_amd import spec, synth   # noqa: E402
from oracle import hotpath_ref as orc    # noqa: E402
from oracle import box_head_ref as obh   # noqa: E402

A = sar.AUG
ROIALIGN_POOL = orc.query_pool           # the oracle's own poolings, before this process puts the merge in front of one
MERGED = {}                              # the oracle's merged maps of the last pooling call


def merging_pool(method, inner):
    """`hotpath_ref.query_pool` for this process: the merge of generalized_rcnn.py:280-288, then the pooling, with one size per group"""
    def pool(query_feats, image_sizes, batch_size):
        MERGED["maps"] = [sar.merge(f, A, method) for f in query_feats]
        return inner(MERGED["maps"], None if image_sizes is None else list(image_sizes)[::A], batch_size)
    return pool


def near_tie_stats(unmerged):
    """per level of the oracle's un-merged maps [G*A, C, h, w]: (elements with a top-two gap < 1e-6 absmax, share < 1e-4 absmax,
    share of elements member 0 wins)"""
    count, share, first = [], [], []
    for f in unmerged:
        g = f.detach().reshape((f.shape[0] // A, A) + tuple(f.shape[1:]))
        top = g.topk(2, dim=1)[0]
        gap = (top[:, 0] - top[:, 1]) / g.abs().max()
        count.append(int((gap < 1e-6).sum()))
        share.append(float((gap < 1e-4).float().mean()))
        first.append(float((g.argmax(dim=1) == 0).float().mean()))
        if f.shape[2] * f.shape[3] <= 4:
            assert count[-1] == 0, ("a near tie on a level of %d pixels" % (f.shape[2] * f.shape[3]), count[-1])
    return {"near_ties.count_1e-6": np.asarray(count, np.int64), "near_ties.share_1e-4": np.asarray(share, np.float64),
            "near_ties.member0_share": np.asarray(first, np.float64)}


def run_reference(model, images, queries, batch, shared, roialign=True):
    """make_golden(_shared / _avgpool).run_reference, plus the merged maps: what the reference hands to supp_pooling"""
    merged, raw = [], []

    def grab(m, i, o):          # a hook that returns a value would replace the module's output
        merged.append(i[0])
        raw.append(o)
    hooks = [model.supp_pooling.register_forward_hook(grab)]
    try:
        cap = (mgs.run_reference if shared else mg.run_reference)(model, images, queries, batch)
    finally:
        for h in hooks:
            h.remove()
    if roialign:          # SuppAlignLayer: one call over the list of levels
        assert len(merged) == 1 and len(merged[0]) == 5
        cap["merged"] = list(merged[0])
    else:                 # AdaptiveAvgPool2d: one call per level
        assert len(merged) == 5
        cap["merged"], cap["pooled_raw"] = merged, raw
    cap["query_features_unmerged"], cap["query_features"] = cap["query_features"], cap["merged"]
    return cap


def gen_case(model, np_sd, method, name, shared):
    B, H, W, S, qh, qw = gu.CASES[name]
    img_np, q_np = sar.case_inputs(name)
    assert q_np.shape[0] == B * S * A
    images, queries = torch.from_numpy(img_np), torch.from_numpy(q_np)
    cap = run_reference(model, images, queries, B, shared)
    sd = orc.to_torch_state_dict(np_sd)
    orc.query_pool = merging_pool(method, ROIALIGN_POOL)
    with torch.no_grad():
        o = orc.hot_path_forward(images, queries, mgs.tied(sd) if shared else sd, shots=S)
    o["query_features_unmerged"], o["query_features"] = o["query_features"], MERGED["maps"]
    tag = sar.forward_name(method, name, shared)[:-4]
    for lvl in range(5):          # the un-merged maps too, at record_first_stage's threshold for the merged ones
        ref_t = cap["query_features_unmerged"][lvl]
        assert ref_t.shape[0] == B * S * A and cap["query_features"][lvl].shape[0] == B * S
        d = (o["query_features_unmerged"][lvl] - ref_t).abs().max().item() / max(ref_t.abs().max().item(), 1e-6)
        assert d < 1e-4, (lvl, d)
    out = mga.record_first_stage(model, cap, o, B, [(H, W)] * B, tag)
    for lvl in range(5):
        out.update(gu.checksum(mg.t2n(cap["query_features_unmerged"][lvl]), "query_features_unmerged.%d" % lvl))
    if method == "max":
        out.update(near_tie_stats(o["query_features_unmerged"]))
        print("  near ties:", {k: v.tolist() for k, v in out.items() if k.startswith("near_ties.")})
    np.savez_compressed(os.path.join(HERE, tag + ".npz"), **out)


def gen_train_case(model, np_sd, method, name, roialign):
    """make_golden.gen_train_case (roialign: the reference's pooled vector detached) / make_golden_avgpool.gen_train_case (global
    average: the query branch attached in the reference too) with the merge between the query backbone and the pooling."""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    B, H, W, S, qh, qw = gu.CASES[name]
    img_np, q_np = sar.case_inputs(name)
    images, queries = torch.from_numpy(img_np), torch.from_numpy(q_np)
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    targets = []
    for g in gts:
        bl = BoxList(torch.from_numpy(g), (W, H), mode="xyxy")
        bl.add_field("labels", torch.ones(len(g), dtype=torch.int64))
        targets.append(bl)
    model.train()
    model.zero_grad()
    feats = model.backbone(images)
    qfeats = [sar.merge(f, A, method) for f in model.supp_backbone(queries)]       # generalized_rcnn.py:280-288
    if roialign:
        rois_boxes = [BoxList([[0, 0, qh, qw]], image_size=(qh, qw), mode="xyxy") for _ in range(B * S)]
        with torch.no_grad():
            pooled = [model.batch_pooling(p, B) for p in model.supp_pooling([f.detach() for f in qfeats], rois_boxes)]
    else:
        pooled = [model.batch_pooling(model.supp_pooling(f), B) for f in qfeats]
    combined = [f * p.expand(-1, -1, f.shape[2], f.shape[3]) for f, p in zip(feats, pooled)]
    box_cls, box_reg, ctr = model.rpn.head(combined)
    locations = model.rpn.compute_locations(combined)
    lc, lr, lctr = model.rpn.loss_evaluator(locations, box_cls, box_reg, ctr, model.rpn.clean_targets(targets))
    (lc + lr + lctr).backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.eval()
    assert roialign != any(k.startswith("supp_backbone.") for k in ref_grads)
    orc.query_pool = merging_pool(method, ROIALIGN_POOL if roialign else mga.avg_query_pool)
    unmerged = {}

    def oracle_run(detach_pooled, focal):
        sd = orc.to_torch_state_dict(np_sd)
        for k in sd:
            if not spec.is_frozen(k):
                sd[k].requires_grad_(True)
        f = orc.backbone(images, sd, "backbone.")
        qf = orc.backbone(queries, sd, "supp_backbone.")
        unmerged["maps"] = qf
        pl = orc.query_pool(qf, [(qh, qw)] * (B * S * A), B)
        if detach_pooled:
            pl = [p.detach() for p in pl]
        comb = orc.correlate(f, pl)
        lg, br, ct = orc.fcos_head(comb, sd)
        c, r, t, info = orc.fcos_loss(lg, br, ct, gts, focal=focal)
        (c + r + t).backward()
        return (c, r, t), {k: v.grad for k, v in sd.items() if v.grad is not None}, info

    tag = sar.train_name(method, name)[:-4]
    (oc, orr, octr), og, info = oracle_run(roialign, "cpu")
    print(tag, "reference losses", lc.item(), lr.item(), lctr.item(), "| oracle", oc.item(), orr.item(), octr.item(),
          "num_pos", info["num_pos"])
    for a, b in ((lc, oc), (lr, orr), (lctr, octr)):
        assert abs(a.item() - b.item()) <= 1e-5 * max(1.0, abs(a.item())), (a.item(), b.item())
    worst = 0.0
    for k, g in ref_grads.items():
        assert k in og, k
        worst = max(worst, (og[k] - g).abs().max().item() / max(g.abs().max().item(), 1e-8))
    assert set(og) == set(ref_grads), set(og) ^ set(ref_grads)
    print(tag, "worst relative grad error oracle-vs-reference (%s): %.2e over %d tensors"
          % ("pooled detached" if roialign else "query branch attached", worst, len(ref_grads)))
    assert worst < 2e-3, worst
    out = {"losses_ref_cpu_formula": np.array([lc.item(), lr.item(), lctr.item()], dtype=np.float64),
           "num_pos": np.int64(info["num_pos"]), "supp_roialign": np.bool_(roialign),
           "labels": mg.t2n(info["labels"]).astype(np.int8), "reg_targets": mg.t2n(info["reg_targets"])}
    (fc, fr, ft), fg, _ = oracle_run(False, "cuda")
    out["losses_cuda_formula"] = np.array([fc.item(), fr.item(), ft.item()], dtype=np.float64)
    if method == "max":
        out.update(near_tie_stats(unmerged["maps"]))
        print("  near ties:", {k: v.tolist() for k, v in out.items() if k.startswith("near_ties.")})
    for k in mga.GRAD_NAMES[False]:
        for key, gd in (("refgrad_detached" if roialign else "refgrad", ref_grads), ("fullgrad_oracle", fg)):
            if k not in gd:       # query-branch parameters get no gradient when the pooled vector is detached
                continue
            g = mg.t2n(gd[k]).reshape(-1)
            idx = gu.sample_indices(g.size, "grad." + k)[:256]
            out["%s.%s.samples" % (key, k)] = g[idx]
            out["%s.%s.absmax" % (key, k)] = np.float32(np.abs(g).max())
            out["%s.%s.sum" % (key, k)] = np.float64(g.astype(np.float64).sum())
    out["gt_boxes"] = np.concatenate([np.concatenate([np.full((len(g), 1), i, np.float32), g], 1)
                                      for i, g in enumerate(gts)], 0)
    np.savez_compressed(os.path.join(HERE, tag + ".npz"), **out)


def gen_box_case(model, np_sd, method, name):
    """The reference's FULL eval forward, roi_heads included (generalized_rcnn.py:296-318: supproi_pooling and roi_heads read the
    merged maps), recorded like make_golden.gen_box_case records box_<name>.npz; B = 1, so poolers.py:80 holds."""
    B, H, W, S, qh, qw = gu.CASES[name]
    assert B == 1
    img_np, q_np = sar.case_inputs(name)
    images, queries = torch.from_numpy(img_np), torch.from_numpy(q_np)
    grabbed = {"logits": [], "reg": []}

    def grab_pred(m, i, o):
        grabbed["logits"].append(o[0])
        grabbed["reg"].append(o[1])
    hooks = [model.roi_heads.box.predictor.register_forward_hook(grab_pred),
             model.roi_heads.box.feature_extractor.register_forward_hook(lambda m, i, o: grabbed.__setitem__("x", o)),
             model.supproi_pooling.register_forward_hook(lambda m, i, o: grabbed.__setitem__("supp_roi", o)),
             model.supp_pooling.register_forward_hook(lambda m, i, o: grabbed.__setitem__("merged", list(i[0]))),
             model.backbone.register_forward_hook(lambda m, i, o: grabbed.__setitem__("features", list(o))),
             model.rpn.box_selector_test.register_forward_hook(lambda m, i, o: grabbed.__setitem__("proposals", o))]
    model.eval()
    try:
        with torch.no_grad():
            result = model(images, queries, None, device=torch.device("cpu"), target_ids=[1] * B)
    finally:
        for h in hooks:
            h.remove()
    assert len(grabbed["logits"]) == S == 1 and grabbed["merged"][0].shape[0] == B * S
    feats, qfeats, props = grabbed["features"], grabbed["merged"], grabbed["proposals"]
    supp_roi = grabbed["supp_roi"]
    sd = orc.to_torch_state_dict(np_sd)
    with torch.no_grad():
        o = obh.box_head_forward(feats, qfeats, [bl.bbox for bl in props], [(H, W)] * B, [(qh, qw)] * (B * S), sd)
        o_supp = obh.query_roi_features(qfeats, [(qh, qw)] * (B * S))
    ref_logits, ref_reg = grabbed["logits"][0], grabbed["reg"][0]
    err = {"supp_roi": (o_supp - supp_roi).abs().max().item() / max(supp_roi.abs().max().item(), 1e-6),
           "pooled": (o["pooled"] - grabbed["x"]).abs().max().item() / max(grabbed["x"].abs().max().item(), 1e-6),
           "logits": (o["logits"] - ref_logits).abs().max().item(), "reg": (o["box_regression"] - ref_reg).abs().max().item()}
    tag = "box_suppaug_%s_%s" % (method, name)
    print(tag, "R=%d, oracle-vs-reference:" % len(props[0]), {k: "%.2e" % v for k, v in err.items()})
    assert err["supp_roi"] < 1e-5 and err["pooled"] < 1e-5 and err["logits"] < 2e-4 and err["reg"] < 2e-4, err
    out = {"image_size": np.asarray([H, W], dtype=np.int64), "logits": mg.t2n(ref_logits), "box_regression": mg.t2n(ref_reg),
           "n_shots_outputs": np.int64(len(grabbed["logits"]))}
    out.update(gu.checksum(mg.t2n(grabbed["x"]).reshape(B * len(props[0]), -1, 7, 7), "pooled"))
    out.update(gu.checksum(mg.t2n(supp_roi).reshape(B * S, -1, 7, 7), "supp_roi"))
    for i, bl in enumerate(result):
        rb, rs = mg.t2n(bl.bbox), mg.t2n(bl.get_field("scores"))
        ob, os_ = mg.t2n(o["detections"][i][0]), mg.t2n(o["detections"][i][1])
        frac = gu.match_boxes(rb, rs, ob, os_)
        print("  image %d: reference %d detections, oracle %d, overlap %.4f" % (i, len(rb), len(ob), frac))
        assert len(rb) == len(ob) and frac >= 0.999, (len(rb), len(ob), frac)
        order = np.argsort(-rs, kind="stable")
        out["proposals.%d.boxes" % i] = mg.t2n(props[i].bbox)
        out["detections.%d.boxes" % i] = rb[order]
        out["detections.%d.scores" % i] = rs[order]
    np.savez_compressed(os.path.join(HERE, tag + ".npz"), **out)


def build(method, shared=False, roialign=True):
    opts = ["FEW_SHOT.SUPP_AUG", True, "FEW_SHOT.NUM_SUPP_AUG", A - 1, "FEW_SHOT.SUPP_AUG_METHOD", method]
    opts += ["FEW_SHOT.SIAMESE_BACKBONE", False] if shared else []
    opts += [] if roialign else ["FEW_SHOT.SUPP_ROIALIGN", False]
    model, cfg = rh.build_reference_model(opts)
    assert model.supp_aug and model.supp_aug_num == A and cfg.FEW_SHOT.SUPP_AUG_METHOD == method
    assert not hasattr(model, "supp_aug_conv")
    return model, (mgs.load_synth_weights if shared else mg.load_synth_weights)(model)


def main():
    torch.set_num_threads(8)
    try:
        for method in ("avg", "max"):
            model, np_sd = build(method)
            for m, name, shared in sar.FORWARD_CASES:
                if m == method and not shared:
                    gen_case(model, np_sd, method, name, False)
            for m, name, roialign in sar.TRAIN_CASES:
                if m == method and roialign:
                    gen_train_case(model, np_sd, method, name, True)
            if method == sar.BOX_CASE[0]:
                gen_box_case(model, np_sd, *sar.BOX_CASE)
        for m, name, shared in sar.FORWARD_CASES:
            if shared:
                model, np_sd = build(m, shared=True)
                gen_case(model, np_sd, m, name, True)
        for m, name, roialign in sar.TRAIN_CASES:
            if not roialign:
                model, np_sd = build(m, roialign=False)
                assert isinstance(model.supp_pooling, torch.nn.AdaptiveAvgPool2d), type(model.supp_pooling)
                gen_train_case(model, np_sd, m, name, False)
    finally:
        orc.query_pool = ROIALIGN_POOL


if __name__ == "__main__":
    main()
