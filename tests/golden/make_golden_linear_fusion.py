"""Generate the fixtures of the second stage with FEW_SHOT.LINEAR_FUSION True from the REAL reference (build container only).

    python tests/golden/make_golden_linear_fusion.py

The reference model is built from the config of record with FEW_SHOT.LINEAR_FUSION overridden (box_head.py:43,61-72,148: no
compress_dim_conv, feature_aggreg.0 = Conv2d(512, 128, 3, 1, 1) over cat(x, query)) and loaded with synth weights of
spec.full_model_shapes(linear_fusion=True); the key list and every shape must equal the reference model's own.

  box_small_linear.npz, box_nonsquare_linear.npz, box_shots5_linear.npz — what make_golden.py's gen_box_case records (the
    reference's own features and proposals through model.supproi_pooling + model.roi_heads in eval): logits, box deltas (after
    the arg-max over shots), pooled-map checksums, detections.  `nonsquare` has two images (one query map per image), `shots5`
    five queries per image (the loop and the arg-max over shots).  box_small_linear.npz also holds the reference model's
    `roi_heads.box.*` names and shapes under the option (ref_shapes.names / ref_shapes.dims, dims padded with 0 to four).
  boxtrain_small_linear.npz, boxtrain_nonsquare_linear.npz — what gen_box_train_case records (train mode, torch.randperm :=
    argsort of recorded keys): sampled rows, both losses, gradient samples of the box head's parameters (reference autograd) and
    — restatement only, flagged `oracle_only` — the gradients w.r.t. the FPN features of both branches.

The restatement tests/box_linear_fusion_ref.py must agree with the reference before anything is written: logits / deltas 2e-4,
losses 1e-5 * max(1, |loss|), parameter gradients 1e-3 of the largest entry (make_golden.py's bounds for these comparisons).
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
import box_linear_fusion_ref as blf       # noqa: E402
from oneshotdet_amd import spec, synth    # noqa: E402
from oracle import box_head_ref as obh    # noqa: E402
from oracle import box_train_ref as obt   # noqa: E402
from oracle import hotpath_ref as orc     # noqa: E402

GRAD_KEYS = ["roi_heads.box.feature_aggreg.0.weight", "roi_heads.box.feature_aggreg.0.bias", "roi_heads.box.feature_aggreg.1.weight",
             "roi_heads.box.feature_aggreg.1.bias", "roi_heads.box.fc6.weight", "roi_heads.box.fc6.bias", "roi_heads.box.fc7.weight",
             "roi_heads.box.fc7.bias", "roi_heads.box.predictor.cls_score.weight", "roi_heads.box.predictor.cls_score.bias",
             "roi_heads.box.predictor.bbox_pred.weight", "roi_heads.box.predictor.bbox_pred.bias"]


def load_synth_weights(model, seed=0):
    full = spec.full_model_shapes(linear_fusion=True)
    ref_sd = model.state_dict()
    assert list(ref_sd.keys()) == list(full.keys()), "spec.full_model_shapes(linear_fusion=True) key list differs from the reference"
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(full[k]), (k, tuple(v.shape), full[k])
    np_sd = synth.make_state_dict(full, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np_sd.items()}, strict=True)
    return np_sd


def ref_shapes(model):
    box = [(k, tuple(v.shape)) for k, v in model.state_dict().items() if k.startswith("roi_heads.box.")]
    return {"ref_shapes.names": np.asarray([k for k, _ in box]),
            "ref_shapes.dims": np.asarray([list(s) + [0] * (4 - len(s)) for _, s in box], np.int64)}


def gen_box_case(model, np_sd, name, extra=None):
    """make_golden.py gen_box_case on the linear-fusion model."""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    B, H, W, S, qh, qw = gu.CASES[name]
    img_np, q_np = gu.case_inputs(name)
    cap = mg.run_reference(model, torch.from_numpy(img_np), torch.from_numpy(q_np), B)
    feats, qfeats = list(cap["features"]), list(cap["query_features"])
    rmin = min(len(bl) for bl in cap["proposals"])
    props = [bl[:rmin] for bl in cap["proposals"]]
    grabbed = {"logits": [], "reg": []}

    def grab_pred(m, i, o):
        grabbed["logits"].append(o[0])
        grabbed["reg"].append(o[1])

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
    assert len(grabbed["logits"]) == S
    sd = orc.to_torch_state_dict(np_sd)
    with torch.no_grad():
        o = blf.box_head_forward(feats, qfeats, [bl.bbox for bl in props], [(H, W)] * B, [(qh, qw)] * (B * S), sd)
        o_supp = obh.query_roi_features(qfeats, [(qh, qw)] * (B * S))
    if S == 1:
        ref_logits, ref_reg = grabbed["logits"][0], grabbed["reg"][0]
    else:   # the reference's per-class arg-max over shots is internal to ROIBoxHead.forward: redo it on its outputs
        tl, tr = torch.stack(grabbed["logits"], 0), torch.stack(grabbed["reg"], 0)
        idx = torch.argmax(tl, dim=0)
        ref_logits = torch.gather(tl, 0, idx.unsqueeze(0))[0]
        ref_reg = torch.gather(tr, 0, idx[:, :, None].expand(-1, -1, 4).reshape(idx.shape[0], -1).unsqueeze(0))[0]
    err = {"supp_roi": (o_supp - supp_roi).abs().max().item() / max(supp_roi.abs().max().item(), 1e-6),
           "pooled": (o["pooled"] - grabbed["x"]).abs().max().item() / max(grabbed["x"].abs().max().item(), 1e-6),
           "logits": (o["logits"] - ref_logits).abs().max().item(), "reg": (o["box_regression"] - ref_reg).abs().max().item()}
    print(name, "linear box head: R=%d per image, restatement-vs-reference:" % rmin, {k: "%.2e" % v for k, v in err.items()})
    assert err["supp_roi"] < 1e-5 and err["pooled"] < 1e-5 and err["logits"] < 2e-4 and err["reg"] < 2e-4, err
    out = {"image_size": np.asarray([H, W], dtype=np.int64), "logits": mg.t2n(ref_logits), "box_regression": mg.t2n(ref_reg),
           "n_shots_outputs": np.int64(len(grabbed["logits"]))}
    out.update(gu.checksum(mg.t2n(grabbed["x"]).reshape(B * rmin, -1, 7, 7), "pooled"))
    out.update(gu.checksum(mg.t2n(supp_roi).reshape(B * S, -1, 7, 7), "supp_roi"))
    for i, bl in enumerate(result):
        rb, rs = mg.t2n(bl.bbox), mg.t2n(bl.get_field("scores"))
        ob, os_ = mg.t2n(o["detections"][i][0]), mg.t2n(o["detections"][i][1])
        frac = gu.match_boxes(rb, rs, ob, os_)
        print("  image %d: reference %d detections, restatement %d, overlap %.4f" % (i, len(rb), len(ob), frac))
        assert len(rb) == len(ob) and frac >= 0.999, (len(rb), len(ob), frac)
        order = np.argsort(-rs, kind="stable")
        out["proposals.%d.boxes" % i] = mg.t2n(props[i].bbox)
        out["detections.%d.boxes" % i] = rb[order]
        out["detections.%d.scores" % i] = rs[order]
    out.update(extra or {})
    path = os.path.join(HERE, "box_%s_linear.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def gen_box_train_case(model, np_sd, name):
    """make_golden_box_cls_modes.py gen_box_train_case on the linear-fusion model ('ce_loss')."""
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
    assert not any("compress_dim_conv" in k for k in ref_grads)
    model.eval()
    for i, (bl, sm) in enumerate(zip(sampled_props, samp)):
        assert torch.equal(bl.bbox, sm["boxes"]) and torch.equal(bl.get_field("labels"), sm["labels"]), (name, i)
        assert torch.equal(bl.get_field("regression_targets"), sm["targets"]), (name, i)
    sd = orc.to_torch_state_dict(np_sd)
    for k in sd:
        if k.startswith("roi_heads.box."):
            sd[k].requires_grad_(True)
    fg = [f.clone().requires_grad_(True) for f in feats]
    qg = [f.clone().requires_grad_(True) for f in qfeats]
    olc, olb, _, _ = blf.box_train_forward(fg, qg, samp, [(qh, qw)] * (B * S), sd, shots=S)
    (olc + olb).backward()
    print(name, "linear box train: %d sampled per image (%d positives), losses ref %.6f %.6f | restatement %.6f %.6f"
          % (len(samp[0]["index"]), int(sum((sm["labels"] > 0).sum() for sm in samp)), lc.item(), lb.item(), olc.item(), olb.item()))
    assert abs(lc.item() - olc.item()) <= 1e-5 * max(1.0, abs(lc.item())) and abs(lb.item() - olb.item()) <= 1e-5 * max(1.0, abs(lb.item()))
    worst = 0.0
    for k, g in ref_grads.items():
        if k.startswith("roi_heads.box."):
            worst = max(worst, (sd[k].grad - g).abs().max().item() / max(g.abs().max().item(), 1e-12))
    print("   worst relative parameter-gradient error restatement-vs-reference: %.2e" % worst)
    assert worst < 1e-3, worst
    out = {"losses": np.array([lc.item(), lb.item()], dtype=np.float64), "n_props": np.asarray([len(p) for p in props], np.int64),
           "n_sampled": np.int64(len(samp[0]["index"]))}
    for i in range(B):
        out["props.%d" % i] = mg.t2n(props[i].bbox)
        out["gt.%d" % i] = gts[i]
        out["index.%d" % i] = mg.t2n(samp[i]["index"]).astype(np.int32)
        out["labels.%d" % i] = mg.t2n(sampled_props[i].get_field("labels")).astype(np.int32)
        out["targets.%d" % i] = mg.t2n(sampled_props[i].get_field("regression_targets"))
    for k in GRAD_KEYS:
        g = mg.t2n(ref_grads[k]).reshape(-1)
        idx = gu.sample_indices(g.size, "boxgrad." + k)[:256]
        out["refgrad.%s.samples" % k] = g[idx]
        out["refgrad.%s.absmax" % k] = np.float32(np.abs(g).max())
    for lvl in range(5):
        for tag, t in (("dfeat", fg[lvl]), ("dqfeat", qg[lvl])):
            g = mg.t2n(t.grad) if t.grad is not None else np.zeros(tuple(t.shape), np.float32)
            out.update(gu.checksum(g, "oracle_only.%s.%d" % (tag, lvl)))
    path = os.path.join(HERE, "boxtrain_%s_linear.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    torch.set_num_threads(8)
    rh.load_reference()
    model, cfg = rh.build_reference_model(["FEW_SHOT.LINEAR_FUSION", True])
    assert cfg.FEW_SHOT.LINEAR_FUSION is True and not hasattr(model.roi_heads.box, "compress_dim_conv")
    np_sd = load_synth_weights(model)
    gen_box_case(model, np_sd, "small", extra=ref_shapes(model))
    gen_box_case(model, np_sd, "nonsquare")
    gen_box_case(model, np_sd, "shots5")
    gen_box_train_case(model, np_sd, "small")
    gen_box_train_case(model, np_sd, "nonsquare")


if __name__ == "__main__":
    main()
