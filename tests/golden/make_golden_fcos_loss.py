"""Generate the FCOS loss-mode fixture (FCOS.CENTER_SAMPLE x FCOS.LOC_LOSS_TYPE) from the REAL reference (build container only).

    python tests/golden/make_golden_fcos_loss.py

For each of the six combinations of FCOS.CENTER_SAMPLE {True, False} and FCOS.LOC_LOSS_TYPE {'giou', 'iou', 'linear_iou'} the
reference's FCOSLossComputation (modeling/rpn/fcos/loss.py) is built from the config of record with those two keys overridden and
run on small synthetic head outputs and boxes; locations and target cleaning come from the reference's FCOSModule.  oracle/
restates the centre-sampled GIoU loss only, so the restatement with both switches lives in tests/fcos_loss_ref.py; it must agree
with the reference on labels / regression targets exactly and, with the CPU focal formula, on the three losses within
1e-5 * max(1, |loss|) (make_golden.py's bound for this comparison) before anything is written.

Every input is rounded to bfloat16 first (and stored as float32), so the fp32 and the bf16 kernels are given the same numbers.

Writes fcos_loss_modes.npz:
  <case>.hw [L, 2], <case>.gt_boxes [n, 5] (image index, x1, y1, x2, y2; in each image's box order),
  <case>.logits / .centerness [P], <case>.bbox_reg [P, 4]: level-first, then image, then row-major location (the order of the
      reference's flattened tensors, loss.py:237-248); bbox_reg is the head's output AFTER exp (what the loss is given),
  <case>.cs<0|1>.labels [P] int8, .reg_targets [P, 4]           (prepare_targets; they do not depend on the loss type),
  <case>.cs<0|1>.grad_logits_cuda_formula [P]   (the restatement's autograd with focal="cuda", the formula the kernel computes;
      the reference's CPU formula differs from it by its log(p + 1e-6)),
  <case>.cs<0|1>.<loss type>.losses_ref_cpu_formula [3], .losses_cuda_formula [3], .num_pos,
  <case>.cs<0|1>.<loss type>.grad_bbox_reg [P, 4], .grad_centerness [P]        (reference autograd).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                 # noqa: E402  (sets up sys.path for the package, the oracle and the tests' helpers)
import ref_harness as rh                 # noqa: E402
import fcos_loss_ref as flr              # noqa: E402
from oneshotdet_amd import spec, synth   # noqa: E402
from oracle import hotpath_ref as orc    # noqa: E402

# name -> (image H, W, boxes per image).  "quirks": image 0's FIRST box has centre x 0 (get_sample_region, loss.py:58-61: nothing is
# positive in that image with CENTER_SAMPLE, the whole-box mode has positives); image 1 holds two nested pairs (min-area rule, the
# larger box first in one pair and second in the other), a 120 x 110 box for P4 and a 300 x 110 box for P5, far larger than the
# 96 px sampling region there.  "random": synth boxes on a small image.
CASES = {
    "quirks": (192, 320, [[[-40, 30, 40, 110], [100, 80, 180, 180]],
                          [[60, 40, 180, 150], [90, 70, 150, 125], [200, 120, 240, 170], [190, 110, 260, 185], [10, 80, 310, 190]]]),
    "random": (96, 128, None),
}


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float32)


def level_hw(H, W):
    """FPN map sizes of an H x W image (stride-2 3 x 3 convs with padding 1: ceil)"""
    return [(-(-H // s), -(-W // s)) for s in spec.FPN_STRIDES]


def make_inputs(name):
    H, W, boxes = CASES[name]
    if boxes is None:
        gts = synth.make_gt_boxes(3, H, W, seed=11, max_boxes=3)
    else:
        gts = [np.asarray(b, np.float32) for b in boxes]
    hw = level_hw(H, W)
    N = len(gts)
    rng = np.random.RandomState(len(name) * 1000 + 7)
    locs = orc.compute_locations(hw)
    # predictions near the whole-box targets where there is one (IoUs away from 0), anything positive elsewhere
    lab, reg_t = flr.fcos_targets(locs, gts, center_sample=False)
    P = lab.numel()
    base = np.concatenate([np.full(N * h * w, float(s), np.float32) for (h, w), s in zip(hw, spec.FPN_STRIDES)])
    pred = base[:, None] * np.exp(rng.randn(P, 4).astype(np.float32) * 0.5)
    pos = lab.numpy() > 0
    pred[pos] = reg_t.numpy()[pos] * np.exp(rng.randn(int(pos.sum()), 4).astype(np.float32) * 0.3)
    logits = rng.randn(P).astype(np.float32) * 1.5 - 2.0
    ctr = rng.randn(P).astype(np.float32)
    return hw, gts, bf16_round(logits), bf16_round(pred), bf16_round(ctr)


def unflatten(flat, hw, N, C):
    """level-first [P(, C)] -> per level NCHW"""
    out, beg = [], 0
    for h, w in hw:
        n = N * h * w
        out.append(flat[beg:beg + n].reshape(N, h, w, C).permute(0, 3, 1, 2).contiguous())
        beg += n
    return out


def flatten(levels):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in levels], 0)


def run_reference(evaluator, rpn, hw, gts, W, H, logits, pred, ctr):
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    N = len(gts)
    targets = []
    for g in gts:
        bl = BoxList(torch.from_numpy(g), (W, H), mode="xyxy")
        bl.add_field("labels", torch.ones(len(g), dtype=torch.int64))
        targets.append(bl)
    targets = rpn.clean_targets(targets)
    lv = [unflatten(t.reshape(-1, c), hw, N, c) for t, c in ((logits, 1), (pred, 4), (ctr, 1))]
    for lst in lv:
        for t in lst:
            t.requires_grad_(True)
    locations = rpn.compute_locations(lv[0])
    labels, reg_t = evaluator.prepare_targets(locations, targets)
    lc, lr, lctr = evaluator(locations, lv[0], lv[1], lv[2], targets)
    (lc + lr + lctr).backward()
    grads = [flatten([t.grad if t.grad is not None else torch.zeros_like(t) for t in lst]) for lst in lv]
    return (lc, lr, lctr), torch.cat(labels, 0), torch.cat(reg_t, 0), grads


def run_restatement(hw, gts, logits, pred, ctr, cs, lt, focal):
    N = len(gts)
    lv = [unflatten(t.reshape(-1, c), hw, N, c) for t, c in ((logits, 1), (pred, 4), (ctr, 1))]
    for t in lv[0]:
        t.requires_grad_(True)
    c, r, t, info = flr.fcos_loss(lv[0], lv[1], lv[2], gts, focal=focal, center_sample=cs, loc_loss_type=lt)
    c.backward()
    return (c, r, t), info, flatten([x.grad for x in lv[0]])


def check_case_separates(name, hw, gts, per_mode, pred):
    """the properties the fixture is there for (each separates two behaviours of an implementation)"""
    N = len(gts)
    npl = [N * h * w for h, w in hw]
    lab = {cs: per_mode[cs]["labels"].numpy() for cs in (True, False)}
    tgt = {cs: per_mode[cs]["reg_targets"].numpy() for cs in (True, False)}

    def image_slices(img):
        beg = 0
        for (h, w), n in zip(hw, npl):
            yield slice(beg + img * h * w, beg + (img + 1) * h * w)
            beg += n
    if name == "quirks":
        assert (gts[0][0, 0] + gts[0][0, 2]) / 2 == 0
        n0 = {cs: sum(int(lab[cs][s].sum()) for s in image_slices(0)) for cs in (True, False)}
        assert n0[True] == 0 and n0[False] > 0, n0                      # the quirk belongs to centre sampling only
        for cs in (True, False):
            per_level = [int(lab[cs][s].sum()) for s in image_slices(1)]
            assert sum(p > 0 for p in per_level) >= 3, (cs, per_level)   # positives on at least three levels
        # P5 (stride 32): the 300 x 110 box is far larger than the 96 px sampling region
        s = list(image_slices(1))[2]
        assert lab[False][s].sum() > lab[True][s].sum() > 0, (lab[False][s].sum(), lab[True][s].sum())
        # a location inside two boxes that are both in range takes the SMALLER one, whichever comes first
        pts = torch.cat(orc.compute_locations(hw), 0).numpy()
        hits = 0
        for pair in ((0, 1), (3, 2)):
            big, small = gts[1][pair[0]], gts[1][pair[1]]
            s0 = list(image_slices(1))[0]
            h, w = hw[0]
            xy = pts[:h * w]
            both = (xy[:, 0] > small[0]) & (xy[:, 0] < small[2]) & (xy[:, 1] > small[1]) & (xy[:, 1] < small[3])
            m = np.maximum.reduce([xy[:, 0] - big[0], xy[:, 1] - big[1], big[2] - xy[:, 0], big[3] - xy[:, 1]])
            both &= m <= 64
            assert both.any(), pair
            want = np.stack([xy[:, 0] - small[0], xy[:, 1] - small[1], small[2] - xy[:, 0], small[3] - xy[:, 1]], 1)
            assert (lab[False][s0][both] == 1).all() and np.array_equal(tgt[False][s0][both], want[both]), pair
            hits += int(both.sum())
        assert hits > 0
    assert int(lab[False].sum()) > int(lab[True].sum()) > 0
    # a prediction equal to its target in one coordinate, at a location that is positive with the same target in both modes
    tie = (pred.numpy() == tgt[True]) & (lab[True] == 1)[:, None] & (lab[False] == 1)[:, None] & (tgt[True] == tgt[False])
    assert tie.any(), "no tie"


def main():
    torch.set_num_threads(8)
    model, _ = rh.build_reference_model()          # FCOSModule.compute_locations / clean_targets
    from maskrcnn_benchmark.config import cfg as global_cfg
    from maskrcnn_benchmark.modeling.rpn.fcos.loss import FCOSLossComputation
    out = {}
    for name in CASES:
        H, W, _ = CASES[name]
        hw, gts, logits, pred, ctr = make_inputs(name)
        # tie: at the first location that is positive with the same target in both modes, predicted left = target left
        lab_t, tgt_t = flr.fcos_targets(orc.compute_locations(hw), gts, center_sample=True)
        lab_f, tgt_f = flr.fcos_targets(orc.compute_locations(hw), gts, center_sample=False)
        same = (lab_t == 1) & (lab_f == 1) & (tgt_t == tgt_f).all(1) & (bf16_round(tgt_t.numpy()) == tgt_t).all(1)
        idx = torch.nonzero(same).reshape(-1)[:3]
        assert len(idx) == 3
        for k, i in enumerate(idx):
            pred[i, k] = tgt_t[i, k]
        per_mode = {}
        for cs in (True, False):
            for lt in flr.LOC_LOSS_TYPES:
                cfg = global_cfg.clone()
                cfg.defrost()
                cfg.merge_from_file(os.path.join(rh.REFERENCE_ROOT, rh.CONFIG_OF_RECORD))
                cfg.merge_from_list(["MODEL.DEVICE", "cpu", "MODEL.WEIGHT", "", "MODEL.FCOS.CENTER_SAMPLE", cs,
                                     "MODEL.FCOS.LOC_LOSS_TYPE", lt])
                cfg.freeze()
                ev = FCOSLossComputation(cfg)
                assert ev.center_sample is cs and ev.loc_loss_type == lt and ev.radius == spec.POS_RADIUS
                (lc, lr, lctr), labels, reg_t, (_, g_reg, g_ctr) = run_reference(ev, model.rpn, hw, gts, W, H, logits, pred, ctr)
                (oc, orr, octr), info, _ = run_restatement(hw, gts, logits, pred, ctr, cs, lt, "cpu")
                assert torch.equal(labels, info["labels"]) and torch.equal(reg_t, info["reg_targets"]), (name, cs, lt)
                for a, b in ((lc, oc), (lr, orr), (lctr, octr)):
                    assert abs(a.item() - b.item()) <= 1e-5 * max(1.0, abs(a.item())), (name, cs, lt, a.item(), b.item())
                (fc, fr, ft), finfo, g_log_cuda = run_restatement(hw, gts, logits, pred, ctr, cs, lt, "cuda")
                print("%s cs=%d %-10s reference %.6f %.6f %.6f | restatement (cuda focal) %.6f %.6f %.6f  num_pos %d"
                      % (name, cs, lt, lc.item(), lr.item(), lctr.item(), fc.item(), fr.item(), ft.item(), info["num_pos"]))
                key = "%s.cs%d" % (name, cs)
                if cs not in per_mode:
                    per_mode[cs] = {"labels": labels, "reg_targets": reg_t}
                    out[key + ".labels"] = mg.t2n(labels).astype(np.int8)
                    out[key + ".reg_targets"] = mg.t2n(reg_t)
                    out[key + ".grad_logits_cuda_formula"] = mg.t2n(g_log_cuda).reshape(-1)
                else:
                    assert torch.equal(per_mode[cs]["labels"], labels) and torch.equal(per_mode[cs]["reg_targets"], reg_t)
                    assert np.array_equal(out[key + ".grad_logits_cuda_formula"], mg.t2n(g_log_cuda).reshape(-1))
                key += "." + lt
                out[key + ".losses_ref_cpu_formula"] = np.array([lc.item(), lr.item(), lctr.item()], dtype=np.float64)
                out[key + ".losses_cuda_formula"] = np.array([fc.item(), fr.item(), ft.item()], dtype=np.float64)
                out[key + ".num_pos"] = np.int64(info["num_pos"])
                out[key + ".grad_bbox_reg"] = mg.t2n(g_reg)
                out[key + ".grad_centerness"] = mg.t2n(g_ctr).reshape(-1)
        check_case_separates(name, hw, gts, per_mode, pred)
        out[name + ".hw"] = np.asarray(hw, np.int64)
        out[name + ".gt_boxes"] = np.concatenate([np.concatenate([np.full((len(g), 1), i, np.float32), g], 1)
                                                  for i, g in enumerate(gts)], 0)
        out[name + ".logits"], out[name + ".bbox_reg"], out[name + ".centerness"] = mg.t2n(logits), mg.t2n(pred), mg.t2n(ctr)
    path = os.path.join(HERE, "fcos_loss_modes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
