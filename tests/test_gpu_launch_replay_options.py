"""GPU (-m gpu): the launch replay of tests/test_gpu_launch_replay.py for every first-stage OPTION of the engines, the class sweep
and the query gallery.  In these modes the step is not the default step with one kernel swapped: the shared backbone adds both
branches' weight gradients into one dW, supp_aug and the average pooling change the row counts of every query-backbone launch and
put merge / pooling backward launches on the side stream, the loss modes change what the loss-gradient launch writes into the
persistent gradient buffers, the sweep and the gallery replace the correlation launch and multiply the head's batch.  Each test
traces ONE real bf16 step (or forward) after a warm-up call, replays EVERY recorded launch from the engine's own input tensors
(tests/launch_replayer.Fp64Replayer: convs and weight gradients in float64 on the GPU, the rest by oracle/launch_replay.py on the
CPU) and holds it to the bars of test_gpu_launch_replay.py, unchanged: lr.compare for stored tensors with at most 2 % of a
tensor's elements on the neighbouring bf16 value, conv_ref's ACC_TOL / ACC_COS for accumulated gradients, 1e-4 x sum |terms| for
the Scale parameters' raw sums.  Coverage: the kinds the mode must (and must not) launch, and every trainable tensor's gradient
— the Scale parameters' included — accounted for by the replayed launches.

Geometry: B = 2 targets of 128 x 160 (levels 16 x 20 ... 1 x 2: grouped launches, one-workgroup levels and ragged tiles), 63 x 63
queries, synthetic inputs (seed 0, as the default replay's), ground truth of synth.make_gt_boxes(seed 4, max_boxes 3): 3 and 2 boxes.
The first stage only (second_stage=False, with_proposals=False), as the default replays."""
import numpy as np
import pytest
import torch

import conv_ref as cr
import supp_aug_ref as sar
from launch_replayer import DEFAULT_STEP_KINDS, Fp64Replayer, _traced, assert_gradients_covered, assert_kinds_occurred
from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
B, H, W, QS = 2, 128, 160, 63
GT_SEED = 4
FLIP_CAP = cr.FLIP_CAP
AVGPOOL_STEP_KINDS = tuple(k for k in DEFAULT_STEP_KINDS if k not in ("query_pool", "query_pool_bwd")) + ("query_avgpool", "query_avgpool_bwd")


def _images():
    return torch.from_numpy(synth.make_images("target.replay_options", B, H, W, seed=0)).cuda()


def _queries(rows, aug=1):
    q = torch.from_numpy(synth.make_images("query.replay_options", rows, QS, QS, seed=0))
    return (sar.aug_queries(q) if aug == 2 else q).cuda()


def _boxes(seed=GT_SEED):
    gts = synth.make_gt_boxes(B, H, W, seed=seed, max_boxes=3)
    gtb = torch.zeros(B, max(len(g) for g in gts), 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    return gtb.cuda(), torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda()


def _train_engine(dt="bf16", **kw):
    from oneshotdet_amd import train
    shapes = spec.hot_path_shapes(kw.get("siamese_backbone", True))
    return train.TrainEngine(synth.make_state_dict(shapes), dtype=DT[dt], **kw)


def _report(label, trace, rp, worst_acc=None):
    worst = {k: {a: round(b, 4) for a, b in v.items() if b} for k, v in rp.worst.items()}
    acc = "" if worst_acc is None else "\n  worst accumulated-gradient error %.2e of absmax over %d tensors" % (worst_acc, len(rp.acc))
    print("\n%s: %d launches replayed: %s\n  worst per kind: %s%s" % (label, len(trace), rp.counts, worst, acc))


def _replayed_step(eng, shots, label, aug=1, warm_boxes=None):
    """the default replay's pattern: one warm-up step, one traced step, every launch replayed, zero failures, full gradient
    coverage.  -> (trace, replayer, losses of the traced step)"""
    img, q = _images(), _queries(B * shots, aug)
    gtb, cnt = _boxes()
    assert int(cnt[0]) != int(cnt[1])                         # per-image box counts differ: a padded row of gt_boxes is in play
    wb, wc = (gtb, cnt) if warm_boxes is None else warm_boxes
    eng.forward_backward(img, q, wb, wc, with_proposals=False)      # warm-up: allocations, persistent buffers
    torch.cuda.synchronize()
    losses, trace = _traced(lambda: eng.forward_backward(img, q, gtb, cnt, with_proposals=False))
    rp = Fp64Replayer(FLIP_CAP, engine=eng)
    rp.run(trace)
    worst_acc = rp.check_accumulated()
    _report(label, trace, rp, worst_acc)
    assert not rp.failures, rp.failures[:6]
    assert_gradients_covered(rp, eng)
    assert rp.loss_info[3] == int(losses[3]) > 0            # the restatement's positives are the step's
    return trace, rp, losses.cpu()


def _conv_rows(trace):
    """batch sizes of the conv records, in trace order"""
    return [int(r["x"].shape[0]) for kind, r in trace if kind == "conv"]


def _count(trace, kind):
    return sum(1 for k, _ in trace if k == kind)


# ------------------------------------------------------------------------------------------------------------------- training
def test_shared_backbone_step_replays_launch_by_launch():
    """siamese_backbone=False, S = 2: both branches run on ONE backbone's weights and add their weight gradients into one dW.  Every
    trainable backbone conv's dW (body and FPN: both branches use all of them) must have been written by weight-gradient items of
    BOTH branches (B target rows and B*S query rows), and the replayed sum of both is what the engine holds."""
    S = 2
    eng = _train_engine(siamese_backbone=False)
    trace, rp, _ = _replayed_step(eng, S, "shared backbone S=2 bf16")
    assert_kinds_occurred(rp, DEFAULT_STEP_KINDS)
    trainable = [c for n, c in eng.convs.items() if n.startswith("backbone.") and c.trainable]
    assert len(trainable) > 40 and not any(n.startswith("supp_backbone.") for n in eng.convs)
    both = [c.name for c in trainable if {B, B * S} <= set(rp.wgrad_rows.get(c.gw.data_ptr(), []))]
    print("  dW written by both branches: %d of %d trainable backbone convs" % (len(both), len(trainable)))
    assert "backbone.body.layer4.2.conv3" in both and "backbone.body.layer2.0.conv1" in both, both
    assert len(both) == len(trainable), sorted(set(c.name for c in trainable) - set(both))
    eng.close()


def test_avgpool_step_replays_launch_by_launch():
    """supp_roialign=False, S = 2: the whole-map average pooling and its backward replace the ROIAlign pooling."""
    eng = _train_engine(supp_roialign=False)
    trace, rp, _ = _replayed_step(eng, 2, "avgpool S=2 bf16")
    assert_kinds_occurred(rp, AVGPOOL_STEP_KINDS)
    assert _count(trace, "query_avgpool") >= 1 and _count(trace, "query_avgpool_bwd") >= 1
    for kind in ("query_pool", "query_pool_bwd", "roi_align", "shot_mean"):
        assert _count(trace, kind) == 0 and rp.counts.get(kind, 0) == 0, kind
    eng.close()


@pytest.mark.parametrize("method,shots", [("avg", 1), ("max", 2)])
def test_supp_aug_step_replays_launch_by_launch(method, shots):
    """supp_aug=2: one merge launch per direction over all five levels; the query backbone runs on B*S*2 rows, everything behind
    the merge on B*S.  'max': the backward's tie rule (post-rounding bf16 maps of a crop and its flip do tie) is the restatement's."""
    eng = _train_engine(supp_aug=2, supp_aug_method=method)
    trace, rp, _ = _replayed_step(eng, shots, "supp_aug=2 %s S=%d bf16" % (method, shots), aug=2)
    assert_kinds_occurred(rp, DEFAULT_STEP_KINDS + ("supp_aug_reduce", "supp_aug_reduce_bwd"))
    assert _count(trace, "supp_aug_reduce") == 1 and _count(trace, "supp_aug_reduce_bwd") == 1
    assert rp.counts["supp_aug_reduce"] == 5 and rp.counts["supp_aug_reduce_bwd"] == 5          # five levels each
    rows = B * shots * 2
    fwd = [r for k, r in trace if k == "supp_aug_reduce"][0]
    assert fwd["method"] == method and fwd["aug"] == 2
    assert all(x.shape[0] == rows and y.shape[0] == rows // 2 for x, y in zip(fwd["xs"], fwd["outs"]))
    # the query backbone + FPN (every conv before the merge that is not the target's) runs on the unmerged rows, and so do the
    # data-gradient convs behind the merge's backward
    merge_at = [i for i, (k, _) in enumerate(trace) if k == "supp_aug_reduce"][0]
    back_at = [i for i, (k, _) in enumerate(trace) if k == "supp_aug_reduce_bwd"][0]
    before, after = _conv_rows(trace[:merge_at]), _conv_rows(trace[back_at:])
    assert set(before) <= {B, rows} and before.count(rows) >= 40, before
    assert after.count(rows) >= 20, after
    assert rows in [int(r["x"].shape[0]) for k, r in trace if k == "pack_image"]
    eng.close()


@pytest.mark.parametrize("center_sample,loc_loss_type", [(False, "iou"), (True, "linear_iou")])
def test_loss_mode_step_replays_launch_by_launch(center_sample, loc_loss_type):
    """center_sample / loc_loss_type, S = 1.  The loss-gradient launch writes into the engine's PERSISTENT gradient buffers: the
    warm-up step runs on ANOTHER box set (seed 3: two boxes each), so a location the traced step's launch left unwritten would
    still hold the warm-up's gradient — and the replay of the traced step, which restates every location, would see it."""
    eng = _train_engine(center_sample=center_sample, loc_loss_type=loc_loss_type)
    warm = _boxes(seed=3)
    assert not torch.equal(warm[1], _boxes()[1])
    trace, rp, losses = _replayed_step(eng, 1, "loss mode (%s, %s) S=1 bf16" % (center_sample, loc_loss_type), warm_boxes=warm)
    assert_kinds_occurred(rp, DEFAULT_STEP_KINDS)
    recs = [r for k, r in trace if k == "fcos_loss"]
    assert [r["phase"] for r in recs] == [0, 1]
    assert all((r["center_sample"], r["loc_loss_type"]) == (center_sample, loc_loss_type) for r in recs)
    # the buffers the traced launch wrote are the ones the warm-up step made: nothing was allocated for the second step
    bufs = {t.data_ptr() for pair in eng._pred_grad_bufs.values() for t in pair}
    assert len(eng._pred_grad_bufs) == 5
    assert {t.data_ptr() for t in recs[1]["d_cls_ctrs"] + recs[1]["d_regs"]} == bufs
    eng.close()


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_every_option_at_once_replays_launch_by_launch(dt):
    """siamese_backbone=False, supp_roialign=False, supp_aug=2 'max', center_sample=False, loc_loss_type='iou', S = 2: in bf16, and
    in fp32 with the fp32 bars of lr.compare."""
    S = 2
    mode = dict(siamese_backbone=False, supp_roialign=False, supp_aug=2, supp_aug_method="max", center_sample=False, loc_loss_type="iou")
    eng = _train_engine(dt, **mode)
    trace, rp, _ = _replayed_step(eng, S, "every option S=2 %s" % dt, aug=2)
    assert_kinds_occurred(rp, AVGPOOL_STEP_KINDS + ("supp_aug_reduce", "supp_aug_reduce_bwd"))
    assert _count(trace, "supp_aug_reduce") == 1 and _count(trace, "supp_aug_reduce_bwd") == 1
    for kind in ("query_pool", "query_pool_bwd", "roi_align", "shot_mean"):
        assert _count(trace, kind) == 0, kind
    rec = [r for k, r in trace if k == "fcos_loss" and r["phase"] == 1][0]
    assert (rec["center_sample"], rec["loc_loss_type"]) == (False, "iou")
    c = eng.convs["backbone.body.layer4.2.conv3"]
    rows = rp.wgrad_rows[c.gw.data_ptr()]
    assert B in rows and B * S * 2 in rows, rows
    eng.close()


# ------------------------------------------------------------------------------------------------------------------- inference
def _replayed_forward(call, label):
    call()                                                  # warm-up
    torch.cuda.synchronize()
    out, trace = _traced(call)
    rp = Fp64Replayer(FLIP_CAP)
    rp.run(trace)
    _report(label, trace, rp)
    assert not rp.failures, rp.failures[:6]
    return out, trace, rp


def _records_after_the_last(trace, kind):
    last = max(i for i, (k, _) in enumerate(trace) if k == kind)
    return trace[last + 1:]


def test_class_sweep_forward_replays_launch_by_launch():
    """forward(classes=9), one past the sweep kernel's group of 8 query vectors (a partial group): five correlate_sweep records, and
    the head — every launch after the correlation — runs on B*9 rows."""
    from oneshotdet_amd import model, ops
    K = 9
    assert K == ops.class_sweep_group() + 1
    eng = model.HotPathEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=torch.bfloat16)
    img, q = _images(), _queries(B * K)
    out, trace, rp = _replayed_forward(lambda: eng.forward(img, q, classes=K), "class sweep K=9 bf16")
    assert out["classes"] == K
    assert rp.counts.get("correlate_sweep", 0) == 5 and rp.counts.get("correlate", 0) == 0 and rp.counts.get("correlate_gallery", 0) == 0
    assert all(r["classes"] == K and r["x"].shape[0] == B and r["out"].shape[0] == B * K for k, r in trace if k == "correlate_sweep")
    head = _records_after_the_last(trace, "correlate_sweep")
    rows = _conv_rows(head)
    assert len(rows) >= 5 * (2 * spec.NUM_CONVS + 2) and set(rows) == {B * K}, rows
    gn = [int(r["x"].shape[0]) for k, r in head if k == "gn_relu"]
    assert len(gn) == 5 * 2 * spec.NUM_CONVS and set(gn) == {B * K}, gn
    assert rp.counts.get("conv1x1_src2", 0) == 8


def test_gallery_enrollment_and_forward_replay_launch_by_launch():
    """enroll G = 5 slots of 2 shots (traced and replayed: the query branch on its own), then forward(bank=, class_ids=) with a table
    that repeats a slot within an image and runs against the slot order: five correlate_gallery records, the head on B*3 rows, and no
    query-branch launch at all."""
    from oneshotdet_amd import model
    G, S, K = 5, 2, 3
    ids = [[3, 1, 3], [4, 0, 2]]
    flat = [v for r in ids for v in r]
    assert len(set(ids[0])) < K and any(b < a for a, b in zip(flat, flat[1:])) and any(b > a for a, b in zip(flat, flat[1:]))
    eng = model.HotPathEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=torch.bfloat16)
    img, supports = _images(), _queries(G * S)
    bank, tr_enroll, rp_e = _replayed_forward(lambda: eng.enroll(supports, shots=S), "gallery enrollment G=5 S=2 bf16")
    assert (bank.slots, bank.shots) == (G, S)
    assert rp_e.counts.get("query_pool", 0) == 5 and rp_e.counts.get("conv1x1_src2", 0) == 4 and rp_e.counts.get("pack_image", 0) == 1
    assert set(_conv_rows(tr_enroll)) == {G * S}
    out, trace, rp = _replayed_forward(lambda: eng.forward(img, bank=bank, class_ids=ids), "gallery forward K=3 bf16")
    assert out["classes"] == K and out["class_ids"] == ids
    assert rp.counts.get("correlate_gallery", 0) == 5 and rp.counts.get("correlate", 0) == 0 and rp.counts.get("correlate_sweep", 0) == 0
    for k, r in trace:
        if k == "correlate_gallery":
            assert r["slots"].tolist() == flat and r["q"].shape[0] == G and r["out"].shape[0] == B * K and r["classes"] == K
    assert rp.counts.get("query_pool", 0) == 0 and rp.counts.get("conv1x1_src2", 0) == 4 and rp.counts.get("pack_image", 0) == 1
    rows = _conv_rows(_records_after_the_last(trace, "correlate_gallery"))
    assert len(rows) >= 5 * (2 * spec.NUM_CONVS + 2) and set(rows) == {B * K}, rows


def test_option_inference_forward_replays_launch_by_launch():
    """siamese_backbone=False, supp_roialign=False, supp_aug=2 ('avg'), plain forward, S = 2.  The two branches are two passes over
    ONE packed backbone (model.HotPathEngine.repack: supp_backbone IS backbone), not one pass: 4 stages x 2 passes = 8 two-source
    conv3 + downsample launches, as with two backbones."""
    from oneshotdet_amd import model
    S = 2
    eng = model.HotPathEngine(synth.make_state_dict(spec.hot_path_shapes(False)), dtype=torch.bfloat16, siamese_backbone=False,
                              supp_roialign=False, supp_aug=2, supp_aug_method="avg")
    assert eng.supp_backbone is eng.backbone
    img, q = _images(), _queries(B * S, aug=2)
    out, trace, rp = _replayed_forward(lambda: eng.forward(img, q), "every inference option S=2 bf16")
    assert rp.counts.get("conv1x1_src2", 0) == 8, rp.counts
    assert _count(trace, "supp_aug_reduce") == 1 and rp.counts.get("supp_aug_reduce", 0) == 5
    assert _count(trace, "query_avgpool") == 1 and rp.counts.get("query_avgpool", 0) == 5
    assert rp.counts.get("correlate", 0) == 5
    for kind in ("query_pool", "roi_align", "shot_mean"):
        assert _count(trace, kind) == 0, kind
    assert sorted(int(r["x"].shape[0]) for k, r in trace if k == "pack_image") == [B, B * S * 2]
    assert np.isfinite(float(out["head"][0][0].float().abs().max()))
