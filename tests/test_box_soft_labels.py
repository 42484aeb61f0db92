"""CPU: the second stage's IoU soft labels (soft_labeling / soft_labeling_func = FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC) and the
losses that read them ('mse_loss' with soft labels, 'l1_loss', 'cxe_loss').  The restatement tests/box_soft_label_ref.py against the
fixture recorded through the REAL reference (tests/golden/box_soft_labels.npz, tests/golden/make_golden_box_soft_labels.py); the closed
forms the kernel computes against the broadcasts the reference writes; the acceptance / refusal rules of the option; its checkpoint
fields; the argument checks of the two C entries (they run before any launch: no GPU needed).

Tolerances: sampled rows, labels and soft labels exact (the same float32 operations on the CPU); losses 1e-5 * max(1, |loss|) against
the reference's own values (the makers' bound); closed forms against the broadcasts 1e-12 in float64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import box_cls_loss_ref as bcl
import box_soft_label_ref as bsl
from fake_engine import FakeEngine
import golden_utils as gu
from oneshotdet_amd import checkpoint, spec, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_CASES = ["mixed", "nopos", "allpos", "large"]
MATCH_CASES = ["iou", "iou_low", "wide"]


@pytest.fixture(scope="module")
def fx():
    return gu.load("box_soft_labels.npz")


def loss_case(f, name, mode):
    S = int(f["loss.%s.S" % name])
    valid = torch.from_numpy(np.concatenate([np.arange(S) < c for c in f["loss.%s.counts" % name]]))
    logits = torch.from_numpy(f["loss.%s.%s" % (name, "logits2" if mode == "cxe_loss" else "logits1")])
    return (logits[valid], torch.from_numpy(f["loss.%s.deltas" % name])[valid], torch.from_numpy(f["loss.%s.labels" % name])[valid].long(),
            torch.from_numpy(f["loss.%s.soft" % name])[valid], torch.from_numpy(f["loss.%s.targets" % name])[valid], valid)


@pytest.mark.parametrize("func", bsl.FUNCS)
@pytest.mark.parametrize("name", MATCH_CASES)
def test_soft_label_restatement_matches_the_reference_fixture(fx, name, func):
    key = "match.%s." % name
    thresh, batch, fraction = float(fx[key + "thresh"]), int(fx[key + "batch"]), float(fx[key + "fraction"])
    for i, (c, g) in enumerate(zip(fx[key + "counts"], fx[key + "gt_count"])):
        k = int(fx[key + func + ".count"][i])
        if g == 0:              # the reference's matcher raises without ground truth: nothing is sampled
            assert k == 0 and bool(fx[key + "reference_raises_without_gt"])
            continue
        r = bsl.subsample(torch.from_numpy(fx[key + "props"][i, :c]), torch.from_numpy(fx[key + "gt"][i, :g]),
                          torch.from_numpy(fx[key + "keys"][i, :c].copy()), thresh, func, batch=batch, fraction=fraction)
        assert np.array_equal(r["index"].numpy(), fx[key + func + ".index"][i, :k])
        assert np.array_equal(r["labels"].numpy(), fx[key + func + ".labels"][i, :k])
        assert np.array_equal(r["soft"].numpy(), fx[key + func + ".soft"][i, :k])
        assert np.array_equal(r["all_soft"].numpy(), fx[key + func + ".all_soft"][i, :c])
        lab, soft = fx[key + func + ".labels"][i, :k], fx[key + func + ".soft"][i, :k]
        assert (soft[lab == 0] == 0).all() and (soft >= 0).all() and (soft <= 1).all()
        assert (fx[key + func + ".soft"][i, k:] == 0).all() and (fx[key + func + ".labels"][i, k:] == -1).all()


def test_the_iou_case_reaches_every_branch(fx):
    """The 12 hand-made IoUs at both thresholds: with the thresholds of record (0.5) the two trans* functions coincide, at 0.05 they
    differ (the middle branch, the [0.05, 0.1) gap of transLinear, the 4th-order branch); 'linear' is not the hard label."""
    lo = {f: fx["match.iou_low.%s.all_soft" % f][0] for f in bsl.FUNCS}
    hi = {f: fx["match.iou.%s.all_soft" % f][0] for f in bsl.FUNCS}
    iou = np.array([1, 0.5, 0.1, 0.3, 0.07, 0.03, 0, 0.7, 0.25, 0.4, 0, 0.9], np.float32)
    assert np.array_equal(lo["linear"], np.where(iou >= np.float32(0.05), iou, np.float32(0)))
    assert np.array_equal(hi["linear"], np.where(iou >= 0.5, iou, np.float32(0)))
    assert np.array_equal(hi["transLinear"], hi["trans4thLinear"]) and not np.array_equal(lo["transLinear"], lo["trans4thLinear"])
    assert np.array_equal(lo["discrete"], (iou >= 0.5).astype(np.float32))
    t = lo["transLinear"]
    assert t[0] == 1 and abs(t[1] - 0.9) < 1e-6 and t[2] == np.float32(np.float32(2.25) * np.float32(0.1) - np.float32(0.225))
    assert t[2] > 0 and t[4] == 0 and t[5] == 0 and abs(t[3] - 0.45) < 1e-6
    q = lo["trans4thLinear"]
    assert abs(q[3] - 0.9 * 0.6 ** 4) < 1e-6 and 0 < q[4] < 1e-3 and q[5] == 0            # 0.03 is background at 0.05
    assert (hi["linear"] != (iou >= 0.5)).any()


@pytest.mark.parametrize("mode", bsl.SOFT_LOSSES)
@pytest.mark.parametrize("name", LOSS_CASES)
def test_loss_restatement_and_closed_forms_match_the_reference_fixture(fx, name, mode):
    logits, deltas, labels, soft, targets, valid = loss_case(fx, name, mode)
    key = "loss.%s.%s" % (name, mode)
    assert (fx["loss.%s.soft" % name][~valid.numpy()] == np.float32(0.7)).all() and (fx["loss.%s.labels" % name][~valid.numpy()] == 1).all()
    lg, dl = logits.clone().requires_grad_(True), deltas.clone().requires_grad_(True)
    lc, lb = bsl.losses(lg, dl, labels, soft, targets, mode)
    ref = fx[key + ".losses_ref"] * np.array([bcl.W_CLS, bcl.W_BOX])
    f64 = fx[key + ".losses_f64"] * np.array([bcl.W_CLS, bcl.W_BOX])
    for got, want in ((lc.item(), ref[0]), (lb.item(), ref[1]), (lc.item(), f64[0]), (lb.item(), f64[1])):
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    (lc + lb).backward()
    np.testing.assert_allclose(lg.grad.numpy(), fx[key + ".grad_logits"][valid.numpy()], rtol=1e-5, atol=1e-7)
    assert not fx[key + ".grad_logits"][~valid.numpy()].any() and not fx["loss.%s.grad_deltas" % name][~valid.numpy()].any()
    # closed forms == broadcast forms (float64)
    l64, s64 = logits.double(), soft.double()
    broadcast = bsl.cls_loss_value(l64, s64, mode).item()
    assert abs(bsl.closed_form(l64, s64, mode).item() - broadcast) <= 1e-12
    assert abs(broadcast - f64[0] / bcl.W_CLS) <= 1e-12
    lg64 = l64.clone().requires_grad_(True)
    bsl.cls_loss_value(lg64, s64, mode).backward()
    np.testing.assert_allclose(bsl.closed_form_grad(l64, s64, mode).numpy(), lg64.grad.numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(bcl.W_CLS * bsl.closed_form_grad(l64, s64, mode).numpy(), fx[key + ".grad_logits_f64"][valid.numpy()], atol=1e-15)
    # the quirks: not the row-wise mean (mixed soft labels), half the soft cross-entropy
    row = bsl.rowwise_value(l64, s64, mode).item()
    if mode == "cxe_loss":
        assert abs(row - 2 * broadcast) <= 1e-12
    elif name in ("mixed", "large", "allpos"):
        assert abs(row - broadcast) > 1e-3


def test_sign_of_zero_row_is_in_the_fixture(fx):
    """`mixed` row 0: logit exactly 0, soft label exactly 0.5: the pair (0, 0) adds sign(0) = 0 to the l1 gradient's count."""
    assert fx["loss.mixed.logits1"][0, 0] == 0 and fx["loss.mixed.soft"][0] == 0.5 and fx["loss.mixed.labels"][0] == 1
    logits, _, _, soft, _, _ = loss_case(fx, "mixed", "l1_loss")
    s = torch.sigmoid(logits.reshape(-1))
    assert float(s[0]) == 0.5
    M = len(s)
    g = bcl.W_CLS * bsl.closed_form_grad(logits.double(), soft.double(), "l1_loss")[0, 0].item()
    other = bcl.W_CLS * 0.25 / (M * M)            # what sign(0) = +-1 would add
    assert abs(g - float(fx["loss.mixed.l1_loss.grad_logits"][0, 0])) < 1e-7 < other


@pytest.mark.parametrize("mode", spec.BOX_CLS_LOSSES_SOFT)
def test_decode_restatement_matches_the_reference_fixture(fx, mode):
    n, R = fx["decode.rois"].shape[:2]
    logits = torch.from_numpy(fx["decode.%s.logits" % mode])[0]
    assert spec.box_cls_decode_mode(mode, True) == bsl.decode_mode(mode)
    sc = bcl.scores(logits, bsl.decode_mode(mode)).reshape(n, R).numpy()
    live = np.arange(R)[None, :] < fx["decode.counts"][:, None]
    np.testing.assert_allclose(sc[live], fx["decode.%s.scores" % mode][live], rtol=0, atol=1e-6)
    assert (fx["decode.%s.scores" % mode][~live] == -1).all()


def test_spec_accepts_the_soft_losses_with_soft_labeling_only(fx):
    assert spec.SOFT_LABELING is False and spec.SOFT_LABELING_FUNC == "linear" and spec.SOFT_LABELING_FUNCS == bsl.FUNCS
    assert spec.BOX_CLS_LOSSES == bcl.CLS_LOSSES and spec.BOX_CLS_LOSSES_SOFT == ("l1_loss", "cxe_loss") == bcl.REFUSED
    p = "roi_heads.box.predictor."
    for mode, L in (("l1_loss", 1), ("cxe_loss", 2), ("mse_loss", 1)):
        assert spec.box_cls_loss_mode(mode, soft_labeling=True) == mode
        assert spec.box_cls_logits(mode, soft_labeling=True) == L == bsl.n_logits(mode)
        sh = spec.box_head_shapes(box_cls_loss=mode, soft_labeling=True)
        rec = fx["shapes.%s" % mode]
        assert sh[p + "cls_score.weight"] == tuple(rec[0]) == (L, 1024) and sh[p + "bbox_pred.weight"] == tuple(rec[2]) == (8, 1024)
        full = spec.full_model_shapes(box_cls_loss=mode, soft_labeling=True)
        assert full[p + "cls_score.bias"] == (L,) and list(full) == list(spec.full_model_shapes())
        assert spec.box_loss_reads_soft_labels(mode, True) and not spec.box_loss_reads_soft_labels("mse_loss", False)
        sd = {k: torch.zeros(s) for k, s in sh.items()}
        spec.check_box_cls_score(sd, mode, soft_labeling=True)
    for mode in ("ce_loss", "focal_loss"):           # soft labels are computed and never read (loss.py:343-359): nothing changes
        assert spec.box_cls_loss_mode(mode, soft_labeling=True) == mode and not spec.box_loss_reads_soft_labels(mode, True)
        assert spec.box_head_shapes(box_cls_loss=mode, soft_labeling=True) == spec.box_head_shapes(box_cls_loss=mode)
    for bad in spec.BOX_CLS_LOSSES_SOFT:             # without the option: refused exactly as before
        for call in (lambda: spec.box_cls_loss_mode(bad), lambda: spec.box_cls_logits(bad), lambda: spec.box_head_shapes(box_cls_loss=bad),
                     lambda: spec.full_model_shapes(box_cls_loss=bad), lambda: spec.box_cls_decode_mode(bad)):
            with pytest.raises(ValueError, match="SOFT_LABELING"):
                call()
    assert spec.box_cls_decode_mode("l1_loss", True) == "mse_loss" and spec.box_cls_decode_mode("cxe_loss", True) == "ce_loss"
    assert spec.soft_labeling_mode(1, "transLinear") == (True, "transLinear")
    for bad in ("Linear", "translinear", "", None):
        with pytest.raises(ValueError, match="discrete, linear, transLinear, trans4thLinear"):
            spec.soft_labeling_mode(True, bad)
    # what stays out of scope stays refused by name, with soft labels too
    with pytest.raises(ValueError, match="LOSS_WEIGHTED"):
        spec.box_cls_loss_mode("cxe_loss", loss_weighted=True, soft_labeling=True)
    with pytest.raises(ValueError, match="NEG_SUPPORT"):
        spec.box_cls_loss_mode("l1_loss", neg_support=True, soft_labeling=True)
    with pytest.raises(ValueError, match="'rn'"):
        spec.box_cls_loss_mode("l1_loss", method="rn", soft_labeling=True)
    with pytest.raises(ValueError, match="box_cls_loss must be one of"):
        spec.box_cls_loss_mode("hinge", soft_labeling=True)


def test_checkpoint_records_both_options_and_refuses_a_mismatch(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.full_model_shapes(box_cls_loss="l1_loss", soft_labeling=True)).items()}
    p = str(tmp_path / "model_0000010.pth")

    def make(func="transLinear", soft=True, loss="l1_loss"):
        return lambda s: FakeEngine(s, box_cls_loss=loss, soft_labeling=soft, soft_labeling_func=func)
    checkpoint.save_training_checkpoint(p, make()(sd), 10)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert raw["soft_labeling"] is True and raw["soft_labeling_func"] == "transLinear" and raw["box_cls_loss"] == "l1_loss"
    back, extras = checkpoint.load_checkpoint(p, box_cls_loss="l1_loss", soft_labeling=True)
    assert all(torch.equal(back[k], sd[k]) for k in sd) and extras["soft_labeling_func"] == "transLinear"
    with pytest.raises(ValueError, match="SOFT_LABELING"):
        checkpoint.load_checkpoint(p, box_cls_loss="l1_loss")
    eng, it = checkpoint.resume_training(p, make(), box_cls_loss="l1_loss", soft_labeling=True, soft_labeling_func="transLinear")
    assert it == 10 and eng.opt_state["steps"] == 3
    checkpoint.resume_training(p, make())                  # the caller need not say it: the file does
    called = []
    for kw in (dict(soft_labeling=False), dict(soft_labeling_func="linear"), dict(soft_labeling=True, soft_labeling_func="discrete")):
        with pytest.raises(ValueError) as e:               # refused before make_engine, naming both values
            checkpoint.resume_training(p, lambda s: called.append(1), **kw)
        msg = str(e.value)
        assert "soft_labeling=True, soft_labeling_func='transLinear'" in msg
        assert "soft_labeling=%r, soft_labeling_func=%r" % (kw.get("soft_labeling", True), kw.get("soft_labeling_func", "transLinear")) in msg
    assert not called
    with pytest.raises(ValueError, match="discrete, linear"):
        checkpoint.resume_training(p, lambda s: called.append(1), soft_labeling_func="cubic")
    for other in (make(func="linear"), make(soft=False, loss="mse_loss")):           # make_engine built another engine
        with pytest.raises(ValueError) as e:
            checkpoint.resume_training(p, other)
        assert "soft_labeling=True, soft_labeling_func='transLinear'" in str(e.value) and "make_engine" in str(e.value)
    # a file without the fields (every file written before) was trained with (False, "linear")
    sd2 = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.full_model_shapes(box_cls_loss="mse_loss")).items()}
    p2 = str(tmp_path / "model_old.pth")
    checkpoint.save_training_checkpoint(p2, FakeEngine(sd2, box_cls_loss="mse_loss"), 7)
    raw2 = torch.load(p2, map_location="cpu", weights_only=False)
    assert raw2["soft_labeling"] is False and raw2["soft_labeling_func"] == "linear"
    del raw2["soft_labeling"], raw2["soft_labeling_func"]
    torch.save(raw2, p2)
    eng, it = checkpoint.resume_training(p2, lambda s: FakeEngine(s, box_cls_loss="mse_loss"), soft_labeling=False)
    assert it == 7
    checkpoint.resume_training(p2, lambda s: FakeEngine(s, box_cls_loss="mse_loss"), soft_labeling_func="transLinear")    # the function is moot without soft labels
    with pytest.raises(ValueError, match="soft_labeling=False, soft_labeling_func='linear'.*soft_labeling=True"):
        checkpoint.resume_training(p2, lambda s: FakeEngine(s, box_cls_loss="mse_loss", soft_labeling=True), soft_labeling=True)
    with pytest.raises(ValueError, match="make_engine built an engine with soft_labeling=True"):
        checkpoint.resume_training(p2, lambda s: FakeEngine(s, box_cls_loss="mse_loss", soft_labeling=True))


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """osd_box_match_sample_soft / osd_box_loss_soft return OSD_ERR_INVALID_ARG (-1) for every call here: nothing reaches the GPU,
    present or not."""
    from oneshotdet_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "oneshotdet_hip_soft_labels.h")).read()
    consts = dict(re.findall(r"#define (OSD_[A-Z0-9_]+) (\d+)", hdr))
    assert [int(consts["OSD_SOFT_LABEL_" + n]) for n in ("DISCRETE", "LINEAR", "TRANS_LINEAR", "TRANS_4TH_LINEAR")] == [0, 1, 2, 3]
    assert (int(consts["OSD_BOX_CLS_L1"]), int(consts["OSD_BOX_CLS_CXE"])) == (_lib.BOX_CLS_L1, _lib.BOX_CLS_CXE) == (3, 4)
    assert (_lib.SOFT_LABEL_DISCRETE, _lib.SOFT_LABEL_LINEAR, _lib.SOFT_LABEL_TRANS_LINEAR, _lib.SOFT_LABEL_TRANS_4TH_LINEAR) == (0, 1, 2, 3)
    p = ctypes.c_void_p(64)
    rw = (ctypes.c_float * 4)(10.0, 10.0, 5.0, 5.0)
    for bad in (0, 1, 5, -1, 99):                      # ce / focal never read soft labels; unknown modes
        assert lib.osd_box_loss_soft(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 0, p, bad, None) == -1
        assert b"cls_loss" in lib.osd_last_error_string()
    for mode, width in ((2, 9), (3, 9), (4, 10)):
        assert lib.osd_box_loss_soft(p, p, p, p, 1, 4, width - 1, 5.0, 2.5, p, None, 0, 0, p, mode, None) == -1
        assert b"deltas per row" in lib.osd_last_error_string()
        assert lib.osd_box_loss_soft(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, p, width - 1, 0, p, mode, None) == -1
        assert lib.osd_box_loss_soft(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 0, None, mode, None) == -1      # null soft
        assert b"null" in lib.osd_last_error_string()
        assert lib.osd_box_loss_soft(None, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 0, p, mode, None) == -1
        assert lib.osd_box_loss_soft(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 7, p, mode, None) == -1         # dtype
    # the older entries still refuse the new codes
    assert lib.osd_box_loss_opt(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 0, 3, 2.0, 0.25, None) == -1
    assert lib.osd_box_loss_opt(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 0, 4, 2.0, 0.25, None) == -1

    def match(soft_func=1, s_soft=p, boxes=p, props=16, batch=8):
        return lib.osd_box_match_sample_soft(boxes, None, p, p, None, p, 1, props, 2, batch, 0.25, 0.5, rw, p, p, p, p, p, None, None,
                                             soft_func, s_soft, None, None)
    for bad in (-1, 4, 99):
        assert match(soft_func=bad) == -1 and b"soft_func" in lib.osd_last_error_string()
    assert match(s_soft=None) == -1 and b"null" in lib.osd_last_error_string()
    assert match(boxes=None) == -1
    assert match(batch=32) == -1 and match(props=0) != 0 and match(props=10000) != 0
    # the Python wrappers refuse a name before they touch their tensors
    from oneshotdet_amd import ops
    with pytest.raises(ValueError, match="SOFT_LABELING"):
        ops.box_loss(None, None, None, None, 1, 4, 5.0, 2.5, cls_loss="l1_loss")
    with pytest.raises(ValueError, match="soft_labeling_func must be one of"):
        ops.box_match_sample(None, None, None, None, None, 8, 0.25, 0.5, spec.BOX_REG_WEIGHTS, soft_func="cubic")
    with pytest.raises(ValueError, match="SOFT_LABELING"):
        ops.box_decode(None, None, None, spec.BOX_REG_WEIGHTS, 64, 64, 0.0, cls_loss="cxe_loss")


def test_documents_describe_the_option_and_what_stays_refused():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "soft_labeling" in text and "l1_loss" in text and "cxe_loss" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for word in ("2M", "M x M", "LOSS_WEIGHTED", "NEG_SUPPORT", "REVERSE_ORDER", "SUPP_AUG"):
        assert word in design, word
