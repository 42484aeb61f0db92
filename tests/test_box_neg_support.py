"""CPU: the second stage with neg_support=True (FEW_SHOT.NEG_SUPPORT.TURN_ON, SECOND_STAGE_METHOD 'concat', 'ce_loss'): the restatement
tests/box_neg_support_ref.py against the fixtures tests/golden/make_golden_box_neg_support.py recorded through the REAL reference, every
refusal by name, the unchanged key list, the checkpoint field, the documents and the example flags.

Tolerances: the loss restatement in float64 reproduces the recorded float64 values to 1e-12 and the reference's float32 values to
1e-5 * max(1, |loss|) (the recorder's bound); gradients 1e-6 absolute (the recorder's).  End to end the oracle's backbone on another host
CPU supplies the features: losses rtol 1e-3, gradient samples 2e-3 of the tensor's largest entry (tests/test_box_linear_fusion.py)."""
import os

import numpy as np
import pytest
import torch

import box_cls_loss_ref as bcl
import box_neg_support_ref as bns
from fake_engine import FakeEngine
import golden_utils as gu
from oneshotdet_amd import checkpoint, spec, synth
from oracle import box_train_ref as obt
from oracle import hotpath_ref as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = "roi_heads.box."
LOSS_CASES = ["mixed", "wide", "nofg"]


@pytest.fixture(scope="module")
def fx():
    return gu.load("box_neg_support.npz")


def _case(f, name, dtype=torch.float32):
    key = "loss.%s." % name
    S = int(f[key + "S"])
    valid = torch.from_numpy(np.concatenate([np.arange(S) < int(c) for c in f[key + "counts"]]))
    t = {k: torch.from_numpy(f[key + k]) for k in ("logits", "neg_logits", "deltas", "targets")}
    labels = torch.from_numpy(f[key + "labels"]).to(torch.int64)
    return {k: v[valid].to(dtype) for k, v in t.items()}, labels[valid], valid


# ---- the restatement against the recorded reference --------------------------------------------------------------------------------------

def test_fixture_holds_the_cases_the_kernel_has_to_get_right(fx):
    for name in LOSS_CASES:
        key = "loss.%s." % name
        t, labels, valid = _case(fx, name)
        all_labels, active = fx[key + "labels"], fx[key + "active"]
        v = valid.numpy()
        assert (all_labels[~v] == 1).all() and (fx[key + "neg_logits"][~v] == np.array([-30.0, 30.0], np.float32)).all()
        assert int(fx[key + "K"]) == int((labels == 1).sum()) and not active[~v].any()
        for k in ("logits", "neg_logits", "deltas", "targets"):                  # bf16-exact inputs
            a = torch.from_numpy(fx[key + k])
            assert torch.equal(a, a.to(torch.bfloat16).to(torch.float32)), (name, k)
        h = t["neg_logits"].double().softmax(1)[:, 1] - t["logits"].double().softmax(1)[:, 1] + bns.MARGIN
        fg = labels == 1
        assert not bool((h[fg].abs() < 0.02).any())                             # no hinge near its kink
        if name == "nofg":
            assert int(fx[key + "K"]) == 0 and bool(fx[key + "reference_nan_without_foreground"]) and np.isnan(fx[key + "losses_ref"][2])
            assert fx[key + "losses_f64"][2] == 0 and not fx[key + "grad_neg_logits"].any() and not fx[key + "grad_neg_logits_f64"].any()
        else:
            assert bool((fg & (h > 0)).any()) and bool((fg & (h < -0.1)).any()) and bool((labels == 0).any())
    assert fx["loss.wide.logits"].shape[0] == 1152 > 1024 and int(fx["loss.wide.counts"][2]) == 0
    assert fx["loss.mixed.logits"].shape[0] == 16 and len(set(fx["loss.mixed.counts"].tolist())) == 2


@pytest.mark.parametrize("name", LOSS_CASES)
def test_restatement_reproduces_the_loss_fixture(fx, name):
    key = "loss.%s." % name
    t, labels, valid = _case(fx, name)
    lg, ng, dl = (t[k].clone().requires_grad_(True) for k in ("logits", "neg_logits", "deltas"))
    lc, lb, ls = bns.losses(lg, ng, dl, labels, t["targets"], empty="zero")
    ref = fx[key + "losses_ref"]
    for got, want, w in ((lc, ref[0], bns.W_CLS), (lb, ref[1], bns.W_BOX)) + (() if np.isnan(ref[2]) else ((ls, ref[2], bns.W_SUPPRESS),)):
        assert abs(got.item() - w * want) <= 1e-5 * max(1.0, abs(w * want)), (name, got.item() / w, want)
    (lc + lb + ls).backward()
    z = lambda g, like: torch.zeros_like(like) if g is None else g      # noqa: E731
    M = len(valid)
    for g, like, tag, w in ((lg.grad, lg, "grad_logits", 2), (ng.grad, ng, "grad_neg_logits", 2), (dl.grad, dl, "grad_deltas", 8)):
        full = torch.zeros(M, w)
        full[valid] = z(g, like)
        assert np.abs(full.numpy() - fx[key + tag]).max() <= 1e-6, (name, tag)
    # float64: the losses and the closed-form gradients
    d = _case(fx, name, torch.float64)[0]
    fc, fb, fs = bns.losses(d["logits"], d["neg_logits"], d["deltas"], labels, d["targets"], empty="zero")
    want = fx[key + "losses_f64"] * np.array([bns.W_CLS, bns.W_BOX, bns.W_SUPPRESS])
    np.testing.assert_allclose([fc.item(), fb.item(), fs.item()], want, rtol=1e-12, atol=1e-15)
    hp, hn = bns.suppress_grads(d["logits"], d["neg_logits"], labels)
    onehot = torch.nn.functional.one_hot(labels, 2).double()
    gcf = bcl.W_CLS * (d["logits"].softmax(1) - onehot) / len(labels) + bns.W_SUPPRESS * hp
    for g, tag in ((gcf, "grad_logits_f64"), (bns.W_SUPPRESS * hn, "grad_neg_logits_f64")):
        full = torch.zeros(M, 2, dtype=torch.float64)
        full[valid] = g
        np.testing.assert_allclose(full.numpy(), fx[key + tag], rtol=1e-12, atol=1e-15)
    act = torch.zeros(M, dtype=torch.bool)
    act[valid] = bns.suppress_active(d["logits"], d["neg_logits"], labels)
    assert np.array_equal(act.numpy(), fx[key + "active"])
    # the reference's own answer without a foreground row
    if int(fx[key + "K"]) == 0:
        assert bool(torch.isnan(bns.suppress_loss(d["logits"], d["neg_logits"], labels)))


def test_identical_supports_give_the_margin(fx):
    """p == q on every foreground row: the hinge is exactly the margin (what the engine test holds the step to)."""
    t, labels, _ = _case(fx, "wide", torch.float64)
    assert abs(bns.suppress_loss(t["logits"], t["logits"].clone(), labels).item() - bns.MARGIN) <= 1e-15


def test_restatement_reproduces_the_training_fixture():
    name = "small"
    f = gu.load("boxtrain_small_neg.npz")
    B, H, W, S, qh, qw = gu.CASES[name]
    n_props = [int(v) for v in f["n_props"]]
    keys = synth.uniform01("boxtrain.keys." + name, B * max(n_props), seed=9).reshape(B, max(n_props)).astype(np.float32)
    img, q = gu.case_inputs(name)
    nq = synth.make_images(str(f["neg_query.name"]), B * S, qh, qw, int(f["neg_query.seed"]))
    sd0 = orc.to_torch_state_dict(synth.make_state_dict(spec.full_model_shapes()))
    with torch.no_grad():
        o = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(q), sd0, shots=S)
        on = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(nq), sd0, shots=S)
    sd = {k: (v.clone().requires_grad_(True) if k.startswith(P) else v) for k, v in sd0.items()}
    samp = [obt.subsample(torch.from_numpy(f["props.%d" % i]), torch.from_numpy(f["gt.%d" % i]),
                          torch.from_numpy(keys[i, :n_props[i]].copy())) for i in range(B)]
    for i in range(B):
        assert np.array_equal(samp[i]["index"].numpy(), f["index.%d" % i]) and np.array_equal(samp[i]["labels"].numpy(), f["labels.%d" % i])
    labels = torch.cat([s["labels"] for s in samp])
    targets = torch.cat([s["targets"] for s in samp])
    assert int((labels == 1).sum()) == int(f["n_foreground"]) > 0
    qg = [t.clone().requires_grad_(True) for t in o["query_features"]]
    ng = [t.clone().requires_grad_(True) for t in on["query_features"]]
    logits, reg, neg_logits = bns.two_branch_logits(o["features"], qg, ng, [s["boxes"] for s in samp], [(qh, qw)] * B, [(qh, qw)] * B, sd)
    lc, lb, ls = bns.losses(logits, neg_logits, reg, labels, targets)
    np.testing.assert_allclose([lc.item(), lb.item(), ls.item()], f["losses"], rtol=1e-3)
    (lc + lb + ls).backward()
    checked = 0
    for key in f.files:
        if key.startswith("refgrad.") and key.endswith(".samples"):
            k = key[len("refgrad."):-len(".samples")]
            g = sd[k].grad.numpy().reshape(-1)
            idx = gu.sample_indices(g.size, "boxgrad." + k)[:256]
            assert np.abs(g[idx] - f[key]).max() <= 2e-3 * float(f["refgrad.%s.absmax" % k]), k
            checked += 1
    assert checked == 14
    lvl = int(f["query_level"])
    for maps, tag in ((qg, "dqfeat_pos"), (ng, "dqfeat_neg")):
        ref = f[tag]
        assert np.abs(maps[lvl].grad.numpy() - ref).max() <= 2e-3 * np.abs(ref).max(), tag
        assert all(m.grad is None or not bool(m.grad.any()) for j, m in enumerate(maps) if j != lvl)
    # no larger than a handful of the existing end-to-end fixtures, and far below the limit for a committed file
    assert os.path.getsize(os.path.join(gu.GOLDEN_DIR, "boxtrain_small_neg.npz")) < 256 * 1024


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------

def test_spec_validates_the_combinations():
    assert (spec.NEG_SUPPORT, spec.BOX_SUPPRESS_MARGIN, spec.BOX_SUPPRESS_WEIGHT) == (False, 0.3, 2.5)
    assert spec.box_cls_loss_mode("ce_loss", neg_support=True) == "ce_loss"
    assert spec.box_cls_loss_mode("ce_loss", neg_support=True, soft_labeling=True) == "ce_loss"
    for mode, soft in (("focal_loss", False), ("mse_loss", False), ("l1_loss", True), ("cxe_loss", True), ("l1_loss", False)):
        with pytest.raises(ValueError, match="NEG_SUPPORT"):
            spec.box_cls_loss_mode(mode, neg_support=True, soft_labeling=soft)
    assert spec.check_neg_support() is False and spec.check_neg_support(False, second_stage=False, linear_fusion=True) is False
    assert spec.check_neg_support(True) is True and spec.check_neg_support(True, soft_labeling=True) is True
    with pytest.raises(ValueError, match=r"NEG_SUPPORT.*second_stage=True"):
        spec.check_neg_support(True, second_stage=False)
    with pytest.raises(ValueError, match=r"NEG_SUPPORT.*LINEAR_FUSION.*linear_fusion=False"):
        spec.check_neg_support(True, linear_fusion=True)
    with pytest.raises(ValueError, match=r"NEG_SUPPORT.*'ce_loss'"):
        spec.check_neg_support(True, box_cls_loss="focal_loss")
    with pytest.raises(ValueError, match=r"NEG_SUPPORT.*one shot"):
        spec.check_neg_support(True, shots=5)


def test_engines_refuse_by_name_before_anything_is_built():
    """The constructors validate the option before they look for a GPU or at the state_dict (nothing here touches one)."""
    from oneshotdet_amd import model, modules, train
    from oneshotdet_amd.box_head import BoxHeadWeights
    with pytest.raises(ValueError, match=r"NEG_SUPPORT.*second_stage=True"):
        train.TrainEngine({}, neg_support=True)
    with pytest.raises(ValueError, match=r"NEG_SUPPORT.*LINEAR_FUSION"):
        train.TrainEngine({}, second_stage=True, neg_support=True, linear_fusion=True)
    for mode, soft in (("focal_loss", False), ("mse_loss", False), ("cxe_loss", True)):
        with pytest.raises(ValueError, match="NEG_SUPPORT"):
            train.TrainEngine({}, second_stage=True, neg_support=True, box_cls_loss=mode, soft_labeling=soft)
        with pytest.raises(ValueError, match="NEG_SUPPORT"):
            model.HotPathEngine({}, neg_support=True, box_cls_loss=mode, soft_labeling=soft)
        with pytest.raises(ValueError, match="NEG_SUPPORT"):
            modules.OneShotDetector({}, neg_support=True, box_cls_loss=mode, soft_labeling=soft)
        with pytest.raises(ValueError, match="NEG_SUPPORT"):
            BoxHeadWeights({}, torch.float32, neg_support=True, box_cls_loss=mode, soft_labeling=soft)
    for make in (lambda: model.HotPathEngine({}, neg_support=True, linear_fusion=True),
                 lambda: modules.OneShotDetector({}, neg_support=True, linear_fusion=True),
                 lambda: BoxHeadWeights({}, torch.float32, neg_support=True, linear_fusion=True)):
        with pytest.raises(ValueError, match=r"NEG_SUPPORT.*LINEAR_FUSION"):
            make()


class _Eng(object):
    def __init__(self, neg_support):
        self.neg_support = neg_support


def test_step_refuses_the_wrong_negative_queries_before_anything_is_launched():
    """TrainEngine._neg_query_batch is what forward_backward calls first; it reads the engine's neg_support and nothing else."""
    from oneshotdet_amd import layers, ops, train
    check = train.TrainEngine._neg_query_batch
    images, queries = torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 32, 32)
    on, off = _Eng(True), _Eng(False)
    assert check(off, images, queries, None) == (queries, None)
    with pytest.raises(ValueError, match=r"neg_support=False \(FEW_SHOT.NEG_SUPPORT\).*neg_queries=None"):
        check(off, images, queries, queries)
    with pytest.raises(ValueError, match=r"FEW_SHOT.NEG_SUPPORT.*pass neg_queries="):
        check(on, images, queries, None)
    with pytest.raises(ValueError, match=r"FEW_SHOT.NEG_SUPPORT.*one shot"):
        check(on, images, torch.zeros(4, 3, 32, 32), torch.zeros(4, 3, 32, 32))
    for bad in (torch.zeros(2, 3, 32, 64), torch.zeros(1, 3, 32, 32),
                ops.PackedImages(torch.zeros(2, 40, 40, 4), (32, 32), [(32, 32)] * 2)):
        with pytest.raises(ValueError, match=r"FEW_SHOT.NEG_SUPPORT.*collate both to one shape"):
            check(on, images, queries, bad)
    neg = torch.ones(2, 3, 32, 32)
    both, sizes = check(on, images, queries, neg)
    assert sizes is None and tuple(both.shape) == (4, 3, 32, 32) and torch.equal(both[:2], queries) and torch.equal(both[2:], neg)
    both, sizes = check(on, images, queries, layers.ImageList(neg, [(30, 32), (32, 20)]))
    assert sizes == [(30, 32), (32, 20)] and torch.equal(both[2:], neg)
    pq = ops.PackedImages(torch.zeros(2, 40, 40, 4), (32, 32), [(32, 32), (31, 30)])
    pn = ops.PackedImages(torch.ones(2, 40, 40, 4), (32, 32), [(20, 32), (32, 32)])
    both, sizes = check(on, images, pq, pn)
    assert isinstance(both, ops.PackedImages) and both.shape == (4, 3, 32, 32) and sizes == [(20, 32), (32, 32)]
    assert both.image_sizes == pq.image_sizes + pn.image_sizes and torch.equal(both.tensor[2:], pn.tensor)
    with pytest.raises(ValueError, match=r"capture\(\).*FEW_SHOT.NEG_SUPPORT"):
        train.TrainEngine.capture(on, images, queries, None, None)


# ---- keys, checkpoints, documents --------------------------------------------------------------------------------------------------------

def test_the_option_changes_no_key_and_no_shape():
    """The reference's predictor has two class outputs with and without the option (roi_box_predictors.py:55-62): the recorder loaded
    spec.full_model_shapes() into the NEG_SUPPORT model with strict=True.  spec has no neg_support argument to get wrong."""
    import inspect
    import json
    ref = json.load(open(os.path.join(gu.GOLDEN_DIR, "state_dict_keys.json")))
    mine = spec.box_head_shapes()
    assert list(mine.keys()) == list(ref["box_head_shapes"].keys()) and all(list(s) == ref["box_head_shapes"][k] for k, s in mine.items())
    for fn in (spec.full_model_shapes, spec.box_head_shapes, spec.hot_path_shapes):
        assert "neg_support" not in inspect.signature(fn).parameters
    assert mine[P + "predictor.cls_score.weight"][0] == 2


def test_checkpoint_round_trip_and_resume_refusal(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.full_model_shapes()).items()}
    p = str(tmp_path / "model_0000010.pth")
    checkpoint.save_training_checkpoint(p, FakeEngine(sd, neg_support=True), 10)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert raw["neg_support"] is True and list(raw["model"].keys()) == list(spec.full_model_shapes().keys())
    back, extras = checkpoint.load_checkpoint(p)                               # the weights interchange with the plain model's
    assert extras["neg_support"] is True and all(torch.equal(back[k], sd[k]) for k in sd)
    eng, it = checkpoint.resume_training(p, lambda s: FakeEngine(s, neg_support=True), neg_support=True)
    assert it == 10 and eng.opt_state["steps"] == 3
    checkpoint.resume_training(p, lambda s: FakeEngine(s, neg_support=True))              # the caller need not say it: the file does
    called = []
    with pytest.raises(ValueError) as e:                                       # refused before make_engine, naming both values
        checkpoint.resume_training(p, lambda s: called.append(1), neg_support=False)
    assert "neg_support=True" in str(e.value) and "neg_support=False" in str(e.value) and "NEG_SUPPORT" in str(e.value) and not called
    with pytest.raises(ValueError, match=r"NEG_SUPPORT.*make_engine built an engine with neg_support=False"):
        checkpoint.resume_training(p, lambda s: FakeEngine(s))
    # the default model: recorded as False; a file without the field reads as False
    p2 = str(tmp_path / "model_old.pth")
    checkpoint.save_training_checkpoint(p2, FakeEngine(sd), 7)
    raw2 = torch.load(p2, map_location="cpu", weights_only=False)
    assert raw2["neg_support"] is False
    del raw2["neg_support"]
    torch.save(raw2, p2)
    eng, it = checkpoint.resume_training(p2, lambda s: FakeEngine(s), neg_support=False)
    assert it == 7
    with pytest.raises(ValueError, match=r"neg_support=False.*neg_support=True"):
        checkpoint.resume_training(p2, lambda s: FakeEngine(s, neg_support=True), neg_support=True)


def test_documents_describe_the_option():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "neg_support" in text and "oneshotdet_hip.h" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "osd_box_loss_neg_support" in design and "K == 0" in design and "profiles/neg_support_step.md" in design
    assert "stacked" in design
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "osd_box_loss_neg_support" in integ and "loss_cls_suppress" in integ
    sentence = integ[integ.index("Still refused by name"):]
    sentence = sentence[:sentence.index("\n\n")]
    for word in ("LOSS_WEIGHTED", "NEG_SUPPORT", "SECOND_STAGE_METHOD", "'rn'", "'matching'", "REVERSE_ORDER", "SUPP_AUG"):
        assert word in sentence, word
    assert "with any loss but 'ce_loss', with more than one shot" in sentence and "LINEAR_FUSION" not in sentence
    for out_of_scope in ("dataset.py", "capture", "cxe_loss"):
        assert out_of_scope in integ[integ.index("neg_support"):], out_of_scope
    assert os.path.exists(os.path.join(ROOT, "profiles", "neg_support_step.md"))
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_neg_support.py"))


def test_examples_take_the_flag():
    for ex in ("train.py", "detect.py"):
        text = open(os.path.join(ROOT, "examples", ex)).read()
        assert "--neg-support" in text and "neg_support=" in text, ex
    text = open(os.path.join(ROOT, "examples", "train.py")).read()
    assert "loss_cls_suppress" in text and "neg_queries=neg_queries" in text and "ships no" in text.replace("\n", " ")
