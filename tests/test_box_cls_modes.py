"""CPU: the second stage's classification-loss modes (box_cls_loss = FEW_SHOT.SECOND_STAGE_CLS_LOSS: 'ce_loss', 'focal_loss',
'mse_loss').  The restatement tests/box_cls_loss_ref.py against the fixture recorded through the REAL reference
(tests/golden/box_cls_modes.npz, tests/golden/make_golden_box_cls_modes.py); the shapes, validators and checkpoint fields of the
option; the argument checks of the two C entries (they run before any launch: no GPU needed).

Tolerances: losses 1e-5 * max(1, |loss|) against the reference's own values with the CPU focal formula (make_golden.py's bound for
this comparison); labels / positive counts exact; the float64 restatement against itself in fp32 the same 1e-5."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import box_cls_loss_ref as bcl
from fake_engine import FakeEngine
import golden_utils as gu
from oneshotdet_amd import checkpoint, spec, synth
from oracle import box_train_ref as obt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_CASES = ["mixed", "nopos", "allpos", "large"]
ONE_LOGIT = ["focal_loss", "mse_loss"]


@pytest.fixture(scope="module")
def fx():
    return gu.load("box_cls_modes.npz")


def loss_case(f, name, mode):
    """-> valid-row tensors (logits, deltas, labels int64, targets) of a fixture case"""
    S = int(f["loss.%s.S" % name])
    counts = f["loss.%s.counts" % name]
    valid = torch.from_numpy(np.concatenate([np.arange(S) < c for c in counts]))
    logits = torch.from_numpy(f["loss.%s.%s" % (name, "logits2" if mode == "ce_loss" else "logits1")])
    return (logits[valid], torch.from_numpy(f["loss.%s.deltas" % name])[valid],
            torch.from_numpy(f["loss.%s.labels" % name])[valid].long(), torch.from_numpy(f["loss.%s.targets" % name])[valid], valid)


@pytest.mark.parametrize("mode", bcl.CLS_LOSSES)
@pytest.mark.parametrize("name", LOSS_CASES)
def test_restatement_matches_the_reference_fixture(fx, name, mode):
    logits, deltas, labels, targets, valid = loss_case(fx, name, mode)
    key = "loss.%s.%s" % (name, mode)
    assert int((labels > 0).sum()) == int(fx[key + ".n_pos"])
    assert int((torch.from_numpy(fx["loss.%s.labels" % name])[~valid] == 1).all())      # the trap for a count over invalid rows
    lg, dl = logits.clone().requires_grad_(True), deltas.clone().requires_grad_(True)
    lc, lb = bcl.losses(lg, dl, labels, targets, mode, focal="cpu")
    ref = fx[key + ".losses_ref"] * np.array([bcl.W_CLS, bcl.W_BOX])
    for got, want in ((lc.item(), ref[0]), (lb.item(), ref[1])):
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    # float64 values of the formula the kernel computes: the CUDA focal formula differs from the CPU one by its log(p + 1e-6)
    f64 = fx[key + ".losses_f64"] * np.array([bcl.W_CLS, bcl.W_BOX])
    cc, cb = bcl.losses(logits, deltas, labels, targets, mode, focal="cuda")
    for got, want in ((cc.item(), f64[0]), (cb.item(), f64[1])):
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    if mode == "focal_loss":
        assert abs(f64[0] - ref[0]) <= 1e-4 * max(1.0, abs(ref[0]))
    # the reference's autograd (CPU formula)
    (lc + lb).backward()
    np.testing.assert_allclose(lg.grad.numpy(), fx[key + ".grad_logits"][valid.numpy()], rtol=1e-4, atol=1e-6)
    if int(fx[key + ".n_pos"]):
        np.testing.assert_allclose(dl.grad.numpy(), fx["loss.%s.grad_deltas" % name][valid.numpy()], rtol=1e-5, atol=1e-7)
    assert not fx[key + ".grad_logits"][~valid.numpy()].any() and not fx["loss.%s.grad_deltas" % name][~valid.numpy()].any()


@pytest.mark.parametrize("name", LOSS_CASES)
def test_mse_is_the_mean_over_row_label_pairs_not_over_rows(fx, name):
    """loss.py:363 broadcasts [M, 1] - [M] to [M, M]: the closed form of that mean and its gradient equal the reference's value and
    autograd; the row-wise mean a reader expects is another number whenever the labels are mixed."""
    logits, _, labels, _, valid = loss_case(fx, name, "mse_loss")
    ref = float(fx["loss.%s.mse_loss.losses_ref" % name][0])
    cf = bcl.mse_loss_closed_form(logits.double(), labels).item()
    assert abs(cf - ref) <= 1e-6 * max(1.0, abs(ref))
    s = torch.sigmoid(logits.double().reshape(-1))
    g = bcl.W_CLS * (2.0 / len(s)) * (s - labels.double().mean()) * s * (1 - s)
    np.testing.assert_allclose(g.numpy(), fx["loss.%s.mse_loss.grad_logits" % name][valid.numpy()].reshape(-1), rtol=1e-5, atol=1e-7)
    rowwise = ((s - labels.double()) ** 2).mean().item()
    if 0 < int(labels.sum()) < len(labels):
        assert abs(rowwise - ref) > 1e-3
    # the kernel's form of the same mean: every term non-negative
    ml = labels.double().mean()
    assert abs((((s - ml) ** 2).mean() + ml * (1 - ml)).item() - cf) <= 1e-12


def test_ce_restatement_equals_the_oracle(fx):
    for name in LOSS_CASES:
        logits, deltas, labels, targets, _ = loss_case(fx, name, "ce_loss")
        a = bcl.losses(logits, deltas, labels, targets, "ce_loss")
        b = obt.losses(logits, deltas, labels, targets)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("mode", bcl.CLS_LOSSES)
def test_score_and_decode_restatement_match_the_reference_fixture(fx, mode):
    n, R = fx["decode.rois"].shape[:2]
    logits = torch.from_numpy(fx["decode.%s.logits" % mode])[0]
    sc = bcl.scores(logits, mode).reshape(n, R).numpy()
    ih, iw = (int(v) for v in fx["decode.image_size"])
    bx = bcl.decode_clip(torch.from_numpy(fx["decode.deltas"]), torch.from_numpy(fx["decode.rois"]).reshape(-1, 4), (ih, iw))
    live = np.arange(R)[None, :] < fx["decode.counts"][:, None]
    assert (fx["decode.%s.scores" % mode][~live] == -1).all()
    np.testing.assert_allclose(sc[live], fx["decode.%s.scores" % mode][live], rtol=0, atol=1e-6)
    np.testing.assert_allclose(bx.reshape(n, R, 4).numpy()[live], fx["decode.%s.boxes" % mode][live], rtol=0, atol=1e-4)
    if mode != "ce_loss":      # a softmax over the one logit would be 1 everywhere
        assert (fx["decode.%s.scores" % mode][live] < 0.5).any()


def test_shapes_of_every_mode_equal_the_reference(fx):
    for mode in spec.BOX_CLS_LOSSES:
        sh = spec.box_head_shapes(box_cls_loss=mode)
        rec = fx["shapes.%s" % mode]
        p = "roi_heads.box.predictor."
        assert sh[p + "cls_score.weight"] == tuple(rec[0]) and sh[p + "cls_score.bias"] == (int(rec[1][0]),)
        assert sh[p + "bbox_pred.weight"] == tuple(rec[2]) and sh[p + "bbox_pred.bias"] == (int(rec[3][0]),)
        want = ((1, 1024), (1,), (8, 1024), (8,)) if mode != "ce_loss" else ((2, 1024), (2,), (8, 1024), (8,))
        assert tuple(sh[p + k] for k in ("cls_score.weight", "cls_score.bias", "bbox_pred.weight", "bbox_pred.bias")) == want
        assert spec.box_cls_logits(mode) == want[1][0] == bcl.n_logits(mode)
        full = spec.full_model_shapes(box_cls_loss=mode)
        assert list(full) == list(spec.full_model_shapes()) and full[p + "cls_score.weight"] == want[0]
        # every other entry is the default mode's
        assert all(full[k] == v for k, v in spec.full_model_shapes().items() if "cls_score" not in k)
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")))       # dumped from the reference model
    default = spec.full_model_shapes()
    want = dict(ref["shapes"], **ref["box_head_shapes"])
    assert list(default) == list(ref["shapes"]) + list(ref["box_head_shapes"]) and len(default) == ref["num_all_keys"]
    assert all(list(default[k]) == want[k] for k in want)
    assert spec.box_head_shapes() == spec.box_head_shapes(box_cls_loss="ce_loss")
    # synthetic weights exist in every mode
    sd = synth.make_state_dict(spec.box_head_shapes(box_cls_loss="focal_loss"))
    assert sd["roi_heads.box.predictor.cls_score.weight"].shape == (1, 1024)


def test_unknown_and_out_of_scope_names_raise():
    assert spec.BOX_CLS_LOSSES == bcl.CLS_LOSSES and spec.BOX_CLS_LOSS == "ce_loss" and spec.BOX_LOSS_ALPHA == bcl.ALPHA
    assert spec.LOSS_GAMMA == bcl.GAMMA
    for mode in spec.BOX_CLS_LOSSES:
        assert spec.box_cls_loss_mode(mode) == mode
    for bad in ("l1_loss", "cxe_loss"):
        with pytest.raises(ValueError, match="SOFT_LABELING"):
            spec.box_cls_loss_mode(bad)
        with pytest.raises(ValueError, match=bad):
            spec.box_head_shapes(box_cls_loss=bad)
        with pytest.raises(ValueError):
            bcl.n_logits(bad)
    for bad in ("bce", "", None, "CE_LOSS"):
        with pytest.raises(ValueError, match="box_cls_loss must be one of"):
            spec.box_cls_loss_mode(bad)
    with pytest.raises(ValueError, match="LOSS_WEIGHTED"):
        spec.box_cls_loss_mode("ce_loss", loss_weighted=True)
    with pytest.raises(ValueError, match="NEG_SUPPORT"):
        spec.box_cls_loss_mode("focal_loss", neg_support=True)
    with pytest.raises(ValueError, match="'rn'"):
        spec.box_cls_loss_mode("focal_loss", method="rn")
    # a cls_score with the other mode's row count is refused by name, in both directions
    one = {k: torch.zeros(s) for k, s in spec.box_head_shapes(box_cls_loss="mse_loss").items()}
    two = {k: torch.zeros(s) for k, s in spec.box_head_shapes().items()}
    spec.check_box_cls_score(one, "focal_loss")
    spec.check_box_cls_score(two, "ce_loss")
    with pytest.raises(ValueError, match=r"1 row\(s\) but box_cls_loss='ce_loss'.*'focal_loss' or 'mse_loss'"):
        spec.check_box_cls_score(one, "ce_loss")
    with pytest.raises(ValueError, match=r"2 row\(s\) but box_cls_loss='focal_loss'.*box_cls_loss='ce_loss'"):
        spec.check_box_cls_score(two, "focal_loss")


def test_checkpoint_records_the_mode_and_refuses_a_mismatch(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.full_model_shapes(box_cls_loss="focal_loss")).items()}
    p = str(tmp_path / "model_0000010.pth")
    checkpoint.save_training_checkpoint(p, FakeEngine(sd, box_cls_loss="focal_loss"), 10)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert raw["box_cls_loss"] == "focal_loss" and raw["loc_loss_type"] == "giou"
    # .pth round trip in the new shapes
    back, extras = checkpoint.load_checkpoint(p, box_cls_loss="focal_loss")
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd) and extras["box_cls_loss"] == "focal_loss"
    assert back["roi_heads.box.predictor.cls_score.weight"].shape == (1, 1024)
    with pytest.raises(ValueError, match="cls_score"):                  # the default mode's shapes do not fit the file
        checkpoint.load_checkpoint(p)
    eng, it = checkpoint.resume_training(p, lambda s: FakeEngine(s, box_cls_loss="focal_loss"), box_cls_loss="focal_loss")
    assert it == 10 and eng.opt_state["steps"] == 3 and all(torch.equal(eng.sd[k], sd[k]) for k in sd)
    checkpoint.resume_training(p, lambda s: FakeEngine(s, box_cls_loss="focal_loss"))        # the caller need not say it: the file does
    called = []
    for other in ("ce_loss", "mse_loss"):       # refused before make_engine, naming both values
        with pytest.raises(ValueError) as e:
            checkpoint.resume_training(p, lambda s: called.append(1), box_cls_loss=other)
        assert "box_cls_loss='focal_loss'" in str(e.value) and "box_cls_loss=%r" % other in str(e.value)
    assert not called
    with pytest.raises(ValueError, match="l1_loss"):
        checkpoint.resume_training(p, lambda s: called.append(1), box_cls_loss="l1_loss")
    # the two one-logit modes share their shapes: only the record tells them apart (make_engine built the other one)
    with pytest.raises(ValueError) as e:
        checkpoint.resume_training(p, lambda s: FakeEngine(s, box_cls_loss="mse_loss"))
    assert "box_cls_loss='focal_loss'" in str(e.value) and "box_cls_loss='mse_loss'" in str(e.value)
    # a file without the field (every file written before) and an engine without the attribute are 'ce_loss'
    sd2 = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.full_model_shapes()).items()}
    p2 = str(tmp_path / "model_old.pth")
    checkpoint.save_training_checkpoint(p2, FakeEngine(sd2), 7)
    raw2 = torch.load(p2, map_location="cpu", weights_only=False)
    assert raw2["box_cls_loss"] == "ce_loss"
    del raw2["box_cls_loss"]
    torch.save(raw2, p2)
    eng, it = checkpoint.resume_training(p2, lambda s: FakeEngine(s), box_cls_loss="ce_loss")
    assert it == 7
    checkpoint.resume_training(p2, lambda s: FakeEngine(s, box_cls_loss="ce_loss"))
    with pytest.raises(ValueError, match="box_cls_loss='ce_loss'"):
        checkpoint.resume_training(p2, lambda s: FakeEngine(s), box_cls_loss="focal_loss")


def test_c_entries_refuse_a_bad_mode_or_stride():
    """The argument checks of osd_box_loss_opt / osd_box_decode_opt return OSD_ERR_INVALID_ARG (-1) before anything is launched
    (every call here fails a check: nothing reaches the GPU, present or not)."""
    from oneshotdet_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "oneshotdet_hip_box_modes.h")).read()
    consts = dict(re.findall(r"#define OSD_BOX_CLS_([A-Z]+) (\d+)", hdr))
    assert [int(consts[m.split("_")[0].upper()]) for m in spec.BOX_CLS_LOSSES] == [0, 1, 2]
    assert (_lib.BOX_CLS_CE, _lib.BOX_CLS_FOCAL, _lib.BOX_CLS_MSE) == (0, 1, 2)
    p = ctypes.c_void_p(64)
    rw = (ctypes.c_float * 4)(10.0, 10.0, 5.0, 5.0)
    for bad in (3, -1, 99):
        assert lib.osd_box_loss_opt(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 0, bad, 2.0, 0.25, None) == -1
        assert b"cls_loss" in lib.osd_last_error_string()
        assert lib.osd_box_decode_opt(p, p, None, p, p, None, None, 1, 4, 1, 16, rw, 64.0, 64.0, None, 0.0, 0, bad, None) == -1
        assert b"cls_loss" in lib.osd_last_error_string()
    for mode, width in ((0, 10), (1, 9), (2, 9)):
        # pred_stride, then grad_stride, below L + 8
        assert lib.osd_box_loss_opt(p, p, p, p, 1, 4, width - 1, 5.0, 2.5, p, None, 0, 0, mode, 2.0, 0.25, None) == -1
        assert b"deltas per row" in lib.osd_last_error_string()
        assert lib.osd_box_loss_opt(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, p, width - 1, 0, mode, 2.0, 0.25, None) == -1
        assert lib.osd_box_decode_opt(p, p, None, p, p, None, None, 1, 4, 1, width - 1, rw, 64.0, 64.0, None, 0.0, 0, mode, None) == -1
        # a valid mode reaches the null-argument check
        assert lib.osd_box_loss_opt(None, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 0, mode, 2.0, 0.25, None) == -1
        assert b"null" in lib.osd_last_error_string()
    assert lib.osd_box_loss(p, p, p, p, 1, 4, 9, 5.0, 2.5, p, None, 0, 0, None) == -1       # the old entries keep their 10 columns
    assert lib.osd_box_decode(p, p, None, p, p, None, None, 1, 4, 1, 9, rw, 64.0, 64.0, None, 0.0, 0, None) == -1
    # a bad dtype is refused before the launch too
    assert lib.osd_box_loss_opt(p, p, p, p, 1, 4, 16, 5.0, 2.5, p, None, 0, 7, 1, 2.0, 0.25, None) == -1
    # the Python wrappers refuse a name before they touch their tensors
    from oneshotdet_amd import ops
    with pytest.raises(ValueError, match="box_cls_loss"):
        ops.box_loss(None, None, None, None, 1, 4, 5.0, 2.5, cls_loss="hinge")
    with pytest.raises(ValueError, match="SOFT_LABELING"):
        ops.box_decode(None, None, None, spec.BOX_REG_WEIGHTS, 64, 64, 0.0, cls_loss="l1_loss")
