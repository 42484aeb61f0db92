"""Generate the fixtures of the second stage's negative support (FEW_SHOT.NEG_SUPPORT.TURN_ON, SECOND_STAGE_METHOD 'concat',
SECOND_STAGE_CLS_LOSS 'ce_loss') from the REAL reference (build container only).

    python tests/golden/make_golden_box_neg_support.py

The config of record plus FEW_SHOT.NEG_SUPPORT.TURN_ON True.  The restatement tests/box_neg_support_ref.py must agree with the reference
within 1e-5 * max(1, |loss|) (the existing makers' bound) before anything is written.  Every input is rounded to bfloat16 first (and
stored as float32).

1. box_neg_support.npz — FastRCNNLossComputation.__call__ with neg_class_logits (modeling/roi_heads/box_head/loss.py:306-393,435-444).
     loss.<case>.logits / .neg_logits [M, 2], .deltas [M, 8], .labels [M], .targets [M, 4], .counts [N], .S, .active [M] (the rows
       whose hinge is active).  Rows past the count hold label 1 and the negative-branch logits (-30, 30) on purpose: q = 1 there, so
       reading them as foreground rows shows in the loss, in K and in the gradients.  Cases:
         mixed  2 images x 8 rows, counts (8, 5): row 0 is foreground with the hinge active (p = 0.5, q = 0.88), row 1 background, row 2
                foreground with the hinge inactive by a clear margin (q - p + 0.3 = -0.66); the rest random.
         wide   9 x 128 = 1,152 rows (more than the kernel's 1,024 threads), ragged counts, the third image's count 0.
         nofg   no row with label 1 among the valid rows: the reference returns NaN for the suppress loss (recorded as
                loss.nofg.reference_nan_without_foreground); .losses_f64 / gradients hold the kernel's documented zeros.
       No foreground row of any case has |q - p + 0.3| below 0.02: float32 and float64 agree on which hinges are active.
     loss.<case>.losses_ref [3] (reference, before the weights 5 / 2.5 / 2.5), .losses_f64 [3] (restatement in float64, unweighted),
       .K, .grad_logits / .grad_neg_logits [M, 2], .grad_deltas [M, 8] (reference autograd of 5 cls + 2.5 box + 2.5 suppress, zero rows
       past the count), .grad_logits_f64 / .grad_neg_logits_f64 (the closed forms in float64, weighted).
2. boxtrain_small_neg.npz — the `small` geometry end to end, made the way boxtrain_small_focal.npz was made
   (make_golden_box_cls_modes.gen_box_train_case): the real model in train mode, torch.randperm replaced by the recorded permutations
   — three per image here, the third of length 0 (balanced_positive_negative_sampler.py:82-84).  The negative query is
   synth.make_images(neg_query.name, ...) with the seed neg_query.seed.  In addition to that fixture's entries: losses [3],
   dqfeat_pos / dqfeat_neg (the full gradient w.r.t. the positive / negative query's feature map at query_level), and
   oracle_only.dfeat.<level> samples (the gradients through the differentiable restatement of the Pooler: the reference has no CPU
   ROIAlign backward).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                  # noqa: E402  (sets up sys.path for the package, the oracle and the tests' helpers)
import make_golden_box_cls_modes as mcm   # noqa: E402
import make_golden_box_soft_labels as msl  # noqa: E402
import golden_utils as gu                 # noqa: E402
import ref_harness as rh                  # noqa: E402
import box_cls_loss_ref as bcl            # noqa: E402
import box_neg_support_ref as bns         # noqa: E402
from oneshotdet_amd import spec, synth    # noqa: E402
from oracle import box_head_ref as obh    # noqa: E402
from oracle import box_train_ref as obt   # noqa: E402
from oracle import hotpath_ref as orc     # noqa: E402

NEG_OPTS = ["FEW_SHOT.NEG_SUPPORT.TURN_ON", True]
NEG_QUERY = ("neg_query.small", 11)       # name and seed of synth.make_images for the negative query
LOSS_CASES = {                            # name -> (images, rows per image, counts, kind)
    "mixed": (2, 8, (8, 5), "mixed"),
    "wide": (9, 128, (128, 100, 0, 128, 77, 128, 1, 128, 128), "mixed"),
    "nofg": (2, 8, (8, 3), "nofg"),
}
CLEAR = 0.02


def make_cfg():
    from maskrcnn_benchmark.config import cfg as global_cfg
    cfg = global_cfg.clone()
    cfg.defrost()
    cfg.merge_from_file(os.path.join(rh.REFERENCE_ROOT, rh.CONFIG_OF_RECORD))
    cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.WEIGHT", ""] + NEG_OPTS)
    cfg.freeze()
    assert cfg.FEW_SHOT.NEG_SUPPORT.TURN_ON is True and cfg.FEW_SHOT.SECOND_STAGE_CLS_LOSS == "ce_loss"
    assert cfg.FEW_SHOT.SECOND_STAGE_METHOD == "concat" and not cfg.FEW_SHOT.LINEAR_FUSION
    return cfg


# ---- losses ---------------------------------------------------------------------------------------------------------------------------

def loss_inputs(name):
    n, S, counts, kind = LOSS_CASES[name]
    M = n * S
    rng = np.random.RandomState(len(name) * 31 + M)
    valid = np.concatenate([np.arange(S) < c for c in counts])
    labels = (rng.rand(M) < 0.35).astype(np.int32) if kind == "mixed" else np.zeros(M, np.int32)
    logits = mcm.bf16_round(rng.randn(M, 2) * 1.5)
    neg = mcm.bf16_round(rng.randn(M, 2) * 1.5)
    deltas = mcm.bf16_round(rng.randn(M, 8) * 1.5)
    targets = mcm.bf16_round(rng.randn(M, 4))
    if name == "mixed":
        labels[:3] = (1, 0, 1)
        logits[0], neg[0] = torch.tensor([0.0, 0.0]), torch.tensor([-1.0, 1.0])       # p = 0.5, q = 0.88: active
        logits[2], neg[2] = torch.tensor([-2.0, 2.0]), torch.tensor([2.0, -2.0])      # p = 0.98, q = 0.02: inactive
    labels[~valid] = 1                                   # past the count: label 1 and q = 1, on purpose
    neg[torch.from_numpy(~valid)] = torch.tensor([-30.0, 30.0])
    # a hinge within CLEAR of its kink is moved clear of it (q = 0.98: active whatever p is)
    lab = torch.from_numpy(labels)
    h = neg.double().softmax(1)[:, 1] - logits.double().softmax(1)[:, 1] + bns.MARGIN
    near = (lab == 1) & (h.abs() < CLEAR)
    neg[near] = torch.tensor([-2.0, 2.0])
    h = neg.double().softmax(1)[:, 1] - logits.double().softmax(1)[:, 1] + bns.MARGIN
    v = torch.from_numpy(valid)
    assert not bool(((lab == 1) & (h.abs() < CLEAR)).any())
    if kind == "mixed":
        fg = v & (lab == 1)
        assert bool((fg & (h > 0)).any()) and bool((fg & (h < -0.1)).any()) and bool((v & (lab == 0)).any())
    else:
        assert not bool((v & (lab == 1)).any())
    return dict(logits=logits, neg_logits=neg, deltas=deltas, labels=lab, targets=targets, counts=np.asarray(counts, np.int32), S=S,
                valid=v)


def run_reference_loss(cfg, logits, neg_logits, deltas, labels, targets):
    from maskrcnn_benchmark.modeling.roi_heads.box_head.loss import make_roi_box_loss_evaluator
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    ev = make_roi_box_loss_evaluator(cfg)
    bl = BoxList(torch.zeros(len(labels), 4), (64, 64), mode="xyxy")
    bl.add_field("labels", labels.to(torch.int64))
    bl.add_field("regression_targets", targets)
    ev._proposals = [bl]
    lg, ng, dl = (t.clone().requires_grad_(True) for t in (logits, neg_logits, deltas))
    lc, lb, ls = ev([lg], [dl], [ng])
    if bool(torch.isnan(ls)):
        (bcl.W_CLS * lc + bcl.W_BOX * lb).backward()
    else:
        (bcl.W_CLS * lc + bcl.W_BOX * lb + bns.W_SUPPRESS * ls).backward()
    z = lambda t, like: t.grad if t.grad is not None else torch.zeros_like(like)      # noqa: E731
    return lc, lb, ls, z(lg, logits), z(ng, neg_logits), z(dl, deltas)


def gen_loss_cases(out):
    cfg = make_cfg()
    for name in LOSS_CASES:
        d = loss_inputs(name)
        v = d["valid"]
        M = len(v)
        key = "loss.%s." % name
        for k in ("logits", "neg_logits", "deltas", "targets"):
            out[key + k] = mg.t2n(d[k])
        out[key + "labels"] = d["labels"].numpy().astype(np.int32)
        out[key + "counts"], out[key + "S"] = d["counts"], np.int64(d["S"])
        lab = d["labels"][v].to(torch.int64)
        lg, ng, dl, tg = d["logits"][v], d["neg_logits"][v], d["deltas"][v], d["targets"][v]
        lc, lb, ls, g_log, g_neg, g_del = run_reference_loss(cfg, lg, ng, dl, lab, tg)
        K = int((lab == 1).sum())
        nan = bool(torch.isnan(ls))
        assert nan == (K == 0), (name, K, ls)
        if nan:
            out[key + "reference_nan_without_foreground"] = np.bool_(True)
        oc, ob, osup = bns.losses(lg, ng, dl, lab, tg, empty="zero")
        for a, b, w in ((lc, oc, bcl.W_CLS), (lb, ob, bcl.W_BOX)) + (() if nan else ((ls, osup, bns.W_SUPPRESS),)):
            assert abs(w * a.item() - b.item()) <= 1e-5 * max(1.0, abs(w * a.item())), (name, a.item(), b.item() / w)
        fc, fb, fs = bns.losses(lg.double(), ng.double(), dl.double(), lab, tg.double(), empty="zero")
        # closed forms, float64: 5 (softmax - onehot) / M + 2.5 x the hinge's
        onehot = torch.nn.functional.one_hot(lab, 2).double()
        hp, hn = bns.suppress_grads(lg.double(), ng.double(), lab)
        gcf = bcl.W_CLS * (lg.double().softmax(1) - onehot) / len(lab) + bns.W_SUPPRESS * hp
        gnf = bns.W_SUPPRESS * hn
        assert (gcf - g_log.double()).abs().max().item() <= 1e-6 and (gnf - g_neg.double()).abs().max().item() <= 1e-6, name
        act = bns.suppress_active(lg.double(), ng.double(), lab)
        assert torch.equal(act, bns.suppress_active(lg, ng, lab))                      # float32 agrees on the active set
        assert not bool(g_neg[~act].any())
        out[key + "losses_ref"] = np.array([lc.item(), lb.item(), ls.item()], np.float64)
        out[key + "losses_f64"] = np.array([fc.item() / bcl.W_CLS, fb.item() / bcl.W_BOX, fs.item() / bns.W_SUPPRESS], np.float64)
        out[key + "K"] = np.int64(K)
        full = torch.zeros(M, dtype=torch.bool)
        full[v] = act
        out[key + "active"] = full.numpy()
        for tag, g, w in (("grad_logits", g_log, 2), ("grad_neg_logits", g_neg, 2), ("grad_deltas", g_del, 8),
                          ("grad_logits_f64", gcf, 2), ("grad_neg_logits_f64", gnf, 2)):
            full = torch.zeros(M, w, dtype=g.dtype)
            full[v] = g
            out[key + tag] = mg.t2n(full)
        print("loss %-6s M %4d valid %4d K %3d active %3d | reference %.7f %.7f %.7f | float64 restatement %.7f %.7f %.7f"
              % (name, M, int(v.sum()), K, int(act.sum()), lc.item(), lb.item(), ls.item(), fc.item() / bcl.W_CLS, fb.item() / bcl.W_BOX,
                 fs.item() / bns.W_SUPPRESS))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

def run_reference_neg(model, images, queries, neg_queries, batch):
    """make_golden.run_reference for a model that takes a negative support: the query backbone runs twice (generalized_rcnn.py:272-274),
    the positive supports first."""
    cap = {"query_features": []}
    hooks = [model.backbone.register_forward_hook(lambda m, i, o: cap.__setitem__("features", o)),
             model.supp_backbone.register_forward_hook(lambda m, i, o: cap["query_features"].append(o)),
             model.rpn.box_selector_test.register_forward_hook(lambda m, i, o: cap.__setitem__("proposals", o))]
    model.eval()
    with torch.no_grad():
        try:
            model(images, queries, None, images_neg_supp=neg_queries, device=torch.device("cpu"), target_ids=[1] * batch)
        except (AssertionError, TypeError):
            # in evaluation the reference drops target_ids on this path (generalized_rcnn.py:316) and its PostProcessor zips over None
            # (box_head/inference.py:96); everything recorded here has been captured by the hooks at that point
            if "proposals" not in cap:
                raise
    for h in hooks:
        h.remove()
    assert len(cap["query_features"]) == 2
    return cap


def gen_box_train_case(model, np_sd, name):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    B, H, W, S, qh, qw = gu.CASES[name]
    assert S == 1
    img_np, q_np = gu.case_inputs(name)
    nq_np = synth.make_images(NEG_QUERY[0], B * S, qh, qw, NEG_QUERY[1])
    assert not np.array_equal(nq_np, q_np)
    cap = run_reference_neg(model, torch.from_numpy(img_np), torch.from_numpy(q_np), torch.from_numpy(nq_np), B)
    feats = [f.detach() for f in cap["features"]]
    qfeats, nqfeats = ([f.detach() for f in fs] for fs in cap["query_features"])
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
        perms += [p1, p2, torch.zeros(0, dtype=torch.int64)]       # the third draw: the label-2 proposals, of which there are none
    assert len({len(sm["index"]) for sm in samp}) == 1
    rp = msl.recorded_randperm(perms)
    with rp:
        model.train()
        model.zero_grad()
        with torch.no_grad():
            supp_boxes = [BoxList([[0, 0, qh, qw]], image_size=(qh, qw), mode="xyxy") for _ in range(B * S)]
            supp_roi = model.supproi_pooling(qfeats, supp_boxes)
            neg_roi = model.supproi_pooling(nqfeats, supp_boxes)
        x, sampled_props, loss_dict = model.roi_heads(feats, [p for p in props], targets, supp_roi, neg_roi)
    assert next(rp.it, None) is None                                # all three permutations per image were drawn
    lc, lb, ls = loss_dict["loss_classifier"], loss_dict["loss_box_reg"], loss_dict["loss_cls_suppress"]
    (lc + lb + ls).backward()
    ref_grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.eval()
    for i, (bl, sm) in enumerate(zip(sampled_props, samp)):
        assert torch.equal(bl.bbox, sm["boxes"]) and torch.equal(bl.get_field("labels"), sm["labels"]), (name, i)
        assert torch.equal(bl.get_field("regression_targets"), sm["targets"]), (name, i)
    labels = torch.cat([s["labels"] for s in samp])
    tg = torch.cat([s["targets"] for s in samp])
    sd = orc.to_torch_state_dict(np_sd)
    for k in sd:
        if k.startswith("roi_heads.box."):
            sd[k].requires_grad_(True)
    fg = [f.clone().requires_grad_(True) for f in feats]
    qg = [f.clone().requires_grad_(True) for f in qfeats]
    ng = [f.clone().requires_grad_(True) for f in nqfeats]
    logits, reg, neg_logits = bns.two_branch_logits(fg, qg, ng, [s["boxes"] for s in samp], [(qh, qw)] * B, [(qh, qw)] * B, sd)
    olc, olb, ols = bns.losses(logits, neg_logits, reg, labels, tg)
    (olc + olb + ols).backward()
    for a, b in ((lc, olc), (lb, olb), (ls, ols)):
        assert abs(a.item() - b.item()) <= 1e-5 * max(1.0, abs(a.item())), (a.item(), b.item())
    act = bns.suppress_active(logits.detach(), neg_logits.detach(), labels)
    print(name, "box train with a negative support: %d sampled per image (%d positives, %d with an active hinge), losses ref %.6f %.6f %.6f | "
          "restatement %.6f %.6f %.6f" % (len(samp[0]["index"]), int((labels == 1).sum()), int(act.sum()), lc.item(), lb.item(), ls.item(),
                                          olc.item(), olb.item(), ols.item()))
    assert ls.item() > 0 and int(act.sum()) > 0
    worst = 0.0
    for k, g in ref_grads.items():
        if k.startswith("roi_heads.box."):
            worst = max(worst, (sd[k].grad - g).abs().max().item() / max(g.abs().max().item(), 1e-12))
    print("   worst relative parameter-gradient error restatement-vs-reference: %.2e" % worst)
    assert worst < 1e-3, worst
    out = {"losses": np.array([lc.item(), lb.item(), ls.item()], dtype=np.float64),
           "n_props": np.asarray([len(p) for p in props], np.int64), "n_sampled": np.int64(len(samp[0]["index"])),
           "n_foreground": np.int64(int((labels == 1).sum())), "neg_query.name": np.str_(NEG_QUERY[0]), "neg_query.seed": np.int64(NEG_QUERY[1])}
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
    lvl = int(obh.map_levels(torch.tensor([[0.0, 0.0, float(qh), float(qw)]]))[0])
    for j in range(5):                                             # the whole-image box pools from one level only
        if j != lvl:
            assert qg[j].grad is None or not bool(qg[j].grad.any())
            assert ng[j].grad is None or not bool(ng[j].grad.any())
    out["query_level"] = np.int64(lvl)
    out["dqfeat_pos"], out["dqfeat_neg"] = mg.t2n(qg[lvl].grad), mg.t2n(ng[lvl].grad)
    assert out["dqfeat_pos"].any() and out["dqfeat_neg"].any()
    for j in range(5):
        g = mg.t2n(fg[j].grad) if fg[j].grad is not None else np.zeros(tuple(fg[j].shape), np.float32)
        cs = gu.checksum(g, "oracle_only.dfeat.%d" % j)
        cs.pop("oracle_only.dfeat.%d.mean" % j)
        out.update(cs)
    path = os.path.join(HERE, "boxtrain_%s_neg.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def main():
    torch.set_num_threads(8)
    rh.load_reference()
    out = {}
    gen_loss_cases(out)
    path = os.path.join(HERE, "box_neg_support.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    model, cfg = rh.build_reference_model(NEG_OPTS)
    assert model.roi_heads.box.use_neg_supp
    # the same keys and shapes as the 'ce_loss' model without the option: checkpoints interchange
    np_sd = mcm.load_synth_weights(model, "ce_loss")
    gen_box_train_case(model, np_sd, "small")


if __name__ == "__main__":
    main()
