"""Generate the shared-backbone golden fixtures (FEW_SHOT.SIAMESE_BACKBONE False) from the REAL reference (build container only).

    python tests/golden/make_golden_shared.py

The reference model is built with FEW_SHOT.SIAMESE_BACKBONE False (generalized_rcnn.py:274-275: the query goes through the
target's own `backbone`; the state dict has no `supp_backbone.*`), loaded with oneshotdet_amd.synth weights by key and
recorded like make_golden.gen_case / gen_train_case.  The oracle needs no change: it reads `supp_backbone.*` by prefix, so it
is handed a dict whose `supp_backbone.*` entries are the SAME leaf tensors as `backbone.*` and autograd sums the two branches.
Oracle and reference must agree before anything is written.  Writes case_shared_{small,nonsquare}.npz,
train_shared_{small,nonsquare,shots5}.npz and state_dict_keys_shared.json.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                 # noqa: E402  (sets up sys.path for the package, the oracle and golden_utils)
import golden_utils as gu                # noqa: E402
import ref_harness as rh                 # noqa: E402
from oneshotdet_amd import spec, synth   # noqa: E402
from oracle import hotpath_ref as orc    # noqa: E402

FORWARD_CASES = ("small", "nonsquare")
TRAIN_CASES = ("small", "nonsquare", "shots5")


def tied(sd):
    """The oracle's two-backbone dict with the query backbone tied to the target's: the SAME tensor objects."""
    out = dict(sd)
    for k in list(sd):
        if k.startswith("backbone."):
            out["supp_" + k] = sd[k]
    return out


def load_synth_weights(model, seed=0):
    ref_sd = model.state_dict()
    assert not any(k.startswith("supp_backbone.") for k in ref_sd), "the reference built a query backbone"
    hot = [k for k in ref_sd if k.split(".")[0] in ("backbone", "rpn")]
    assert hot == list(spec.hot_path_shapes(False)), "spec.hot_path_shapes(False) key list/order differs from reference"
    full = spec.full_model_shapes(False)
    assert list(ref_sd.keys()) == list(full.keys()), "spec.full_model_shapes(False) key list/order differs from reference"
    for k, v in ref_sd.items():
        assert tuple(v.shape) == tuple(full[k]), (k, v.shape, full[k])
    np_sd = synth.make_state_dict(full, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in np_sd.items()}, strict=True)
    return np_sd


def run_reference(model, images, queries, batch):
    """make_golden.run_reference with the query features taken from the SECOND call of the shared backbone."""
    calls = []
    h = model.backbone.register_forward_hook(lambda m, i, o: calls.append(o))

    class _Alias(torch.nn.Module):          # run_reference hooks model.supp_backbone: a module that is never called
        pass
    model.supp_backbone = _Alias()
    try:
        cap = mg.run_reference(model, images, queries, batch)
    finally:
        del model.supp_backbone
        h.remove()
    assert len(calls) == 2, len(calls)      # target first, then the query (generalized_rcnn.py:270,275)
    cap["features"], cap["query_features"] = calls[0], calls[1]
    return cap


def gen_case(model, np_sd, name):
    B, H, W, S, qh, qw = gu.CASES[name]
    img_np, q_np = gu.case_inputs(name)
    images, queries = torch.from_numpy(img_np), torch.from_numpy(q_np)
    cap = run_reference(model, images, queries, B)
    with torch.no_grad():
        o = orc.hot_path_forward(images, queries, tied(orc.to_torch_state_dict(np_sd)), shots=S)
    out, maxerr = {}, {}
    for lvl in range(5):
        for key, ref_t in (("features", cap["features"][lvl]), ("query_features", cap["query_features"][lvl]),
                           ("combined", cap["head_in"][lvl])):
            d = (o[key][lvl] - ref_t).abs().max().item()
            maxerr[key] = max(maxerr.get(key, 0.0), d / max(ref_t.abs().max().item(), 1e-6))
        pooled_ref = model.batch_pooling(cap["pooled_raw"][lvl], B)
        d = (o["pooled"][lvl] - pooled_ref).abs().max().item()
        maxerr["pooled"] = max(maxerr.get("pooled", 0.0), d / max(pooled_ref.abs().max().item(), 1e-6))
        out["pooled.%d" % lvl] = mg.t2n(pooled_ref).reshape(B, -1)
    ref_head = gu.flatten_head(*[[mg.t2n(t) for t in lst] for lst in cap["head_out"]])
    orc_head = gu.flatten_head(*[[mg.t2n(t) for t in o[k]] for k in ("logits", "bbox_reg", "centerness")])
    maxerr["head"] = float(np.abs(ref_head - orc_head).max())
    print("shared", name, "oracle-vs-reference rel/abs err:", {k: "%.2e" % v for k, v in maxerr.items()})
    assert maxerr["features"] < 1e-4 and maxerr["query_features"] < 1e-4 and maxerr["combined"] < 1e-4, maxerr
    assert maxerr["pooled"] < 1e-5 and maxerr["head"] < 2e-4, maxerr
    out["head"] = ref_head
    for lvl in range(5):
        out.update(gu.checksum(mg.t2n(cap["features"][lvl]), "features.%d" % lvl))
        out.update(gu.checksum(mg.t2n(cap["query_features"][lvl]), "query_features.%d" % lvl))
        out.update(gu.checksum(mg.t2n(cap["head_in"][lvl]), "combined.%d" % lvl))
    orc_props = orc.fcos_postprocess(*cap["head_out"], [(H, W)] * B)
    for i, bl in enumerate(cap["proposals"]):
        rb, rs = mg.t2n(bl.bbox), mg.t2n(bl.get_field("scores"))
        ob, os_ = mg.t2n(orc_props[i][0]), mg.t2n(orc_props[i][1])
        frac = gu.match_boxes(rb, rs, ob, os_)
        assert len(rb) == len(ob) and frac >= 0.999, (len(rb), len(ob), frac)
        order = np.argsort(-rs, kind="stable")
        out["proposals.%d.boxes" % i] = rb[order]
        out["proposals.%d.scores" % i] = rs[order]
    np.savez_compressed(os.path.join(HERE, "case_shared_%s.npz" % name), **out)


# sampled gradient tensors: only `backbone.*` exists, and it carries both branches
GRAD_NAMES = ["backbone.body.layer2.0.conv1.weight", "backbone.body.layer3.1.conv2.weight", "backbone.body.layer4.2.conv3.weight",
              "backbone.fpn.fpn_inner2.weight", "backbone.fpn.fpn_layer2.weight", "backbone.fpn.fpn_layer4.bias",
              "backbone.fpn.top_blocks.p7.weight", "rpn.head.cls_tower.0.weight", "rpn.head.cls_tower.1.weight",
              "rpn.head.bbox_tower.9.bias", "rpn.head.bbox_tower.10.bias", "rpn.head.cls_logits.weight",
              "rpn.head.bbox_pred.weight", "rpn.head.centerness.bias", "rpn.head.scales.0.scale", "rpn.head.scales.4.scale"]


def gen_train_case(model, np_sd, name):
    """make_golden.gen_train_case for the shared model: the reference's gradients with the pooled query detached (ROIAlign has
    no CPU backward), which the tied oracle must reproduce; the tied oracle's full gradient (query branch attached) beside them."""
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    B, H, W, S, qh, qw = gu.CASES[name]
    img_np, q_np = gu.case_inputs(name)
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
    qfeats = model.backbone(queries)
    rois_boxes = [BoxList([[0, 0, qh, qw]], image_size=(qh, qw), mode="xyxy") for _ in range(B * S)]
    with torch.no_grad():
        pooled = [model.batch_pooling(p, B) for p in model.supp_pooling([f.detach() for f in qfeats], rois_boxes)]
    combined = [f * p.expand(-1, -1, f.shape[2], f.shape[3]) for f, p in zip(feats, pooled)]
    box_cls, box_reg, ctr = model.rpn.head(combined)
    locations = model.rpn.compute_locations(combined)
    lc, lr, lctr = model.rpn.loss_evaluator(locations, box_cls, box_reg, ctr, model.rpn.clean_targets(targets))
    (lc + lr + lctr).backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.eval()

    def oracle_run(detach_pooled, focal):
        sd = orc.to_torch_state_dict(np_sd)
        for k in sd:
            if not spec.is_frozen(k):
                sd[k].requires_grad_(True)
        td = tied(sd)
        f = orc.backbone(images, td, "backbone.")
        qf = orc.backbone(queries, td, "supp_backbone.")
        pl = orc.query_pool(qf, [(qh, qw)] * (B * S), B)
        if detach_pooled:
            pl = [p.detach() for p in pl]
        comb = orc.correlate(f, pl)
        lg, br, ct = orc.fcos_head(comb, td)
        c, r, t, info = orc.fcos_loss(lg, br, ct, gts, focal=focal)
        (c + r + t).backward()
        return (c, r, t), {k: v.grad for k, v in sd.items() if v.grad is not None}, info

    (oc, orr, octr), og, info = oracle_run(True, "cpu")
    print("shared train %s: reference losses" % name, lc.item(), lr.item(), lctr.item(), "| oracle", oc.item(), orr.item(),
          octr.item(), "num_pos", info["num_pos"])
    for a, b in ((lc, oc), (lr, orr), (lctr, octr)):
        assert abs(a.item() - b.item()) <= 1e-5 * max(1.0, abs(a.item())), (a.item(), b.item())
    worst = 0.0
    for k, g in ref_grads.items():
        assert k in og, k
        worst = max(worst, (og[k] - g).abs().max().item() / max(g.abs().max().item(), 1e-8))
    print("shared train %s: worst relative grad error oracle-vs-reference (pooled detached): %.2e over %d tensors"
          % (name, worst, len(ref_grads)))
    assert worst < 2e-3, worst
    out = {"losses_ref_cpu_formula": np.array([lc.item(), lr.item(), lctr.item()], dtype=np.float64),
           "num_pos": np.int64(info["num_pos"]),
           "labels": mg.t2n(info["labels"]).astype(np.int8), "reg_targets": mg.t2n(info["reg_targets"])}
    (fc, fr, ft), fg, _ = oracle_run(False, "cuda")
    out["losses_cuda_formula"] = np.array([fc.item(), fr.item(), ft.item()], dtype=np.float64)
    for k in GRAD_NAMES:
        for tag, gd in (("refgrad_detached", ref_grads), ("fullgrad_oracle", fg)):
            g = mg.t2n(gd[k]).reshape(-1)
            idx = gu.sample_indices(g.size, "grad." + k)[:256]
            out["%s.%s.samples" % (tag, k)] = g[idx]
            out["%s.%s.absmax" % (tag, k)] = np.float32(np.abs(g).max())
            out["%s.%s.sum" % (tag, k)] = np.float64(g.astype(np.float64).sum())
    out["gt_boxes"] = np.concatenate([np.concatenate([np.full((len(g), 1), i, np.float32), g], 1)
                                      for i, g in enumerate(gts)], 0)
    np.savez_compressed(os.path.join(HERE, "train_shared_%s.npz" % name), **out)


def gen_keys(model):
    sd = model.state_dict()
    hot = {k: list(v.shape) for k, v in sd.items() if k.split(".")[0] in ("backbone", "rpn")}
    frozen = sorted(n for n, p in model.named_parameters() if not p.requires_grad and n in hot)
    box = {k: list(v.shape) for k, v in sd.items() if k.startswith("roi_heads.")}
    with open(os.path.join(HERE, "state_dict_keys_shared.json"), "w") as f:
        json.dump({"shapes": hot, "frozen_params": frozen, "num_all_keys": len(sd), "box_head_shapes": box}, f, indent=0)


def main():
    torch.set_num_threads(8)
    model, _ = rh.build_reference_model(["FEW_SHOT.SIAMESE_BACKBONE", False])
    np_sd = load_synth_weights(model)
    gen_keys(model)
    for name in FORWARD_CASES:
        gen_case(model, np_sd, name)
    for name in TRAIN_CASES:
        gen_train_case(model, np_sd, name)


if __name__ == "__main__":
    main()
