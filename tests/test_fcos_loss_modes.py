"""CPU: the reference's other FCOS loss modes (center_sample=False: FCOS.CENTER_SAMPLE False, fcos/loss.py:176-177;
loc_loss_type "iou" / "linear_iou": FCOS.LOC_LOSS_TYPE, layers/iou_loss.py:34-41).  tests/fcos_loss_ref.py restates the loss with
both switches: it is the oracle's loss to the last bit in the mode the oracle has, and the reference's own in all six modes
(fixture fcos_loss_modes.npz, recorded through the real reference by tests/golden/make_golden_fcos_loss.py).  The engine, the ops
wrappers and the C boundary refuse an unknown regression loss before anything is launched; training checkpoints record the
loss and refuse to resume on another."""
import ctypes

import numpy as np
import pytest
import torch

import fcos_loss_ref as flr
from fake_engine import FakeEngine
import golden_utils as gu
from oneshotdet_amd import checkpoint, spec, synth
from oracle import hotpath_ref as orc

CASES = ("quirks", "random")


def fixture_inputs(f, name):
    """-> hw, gt boxes per image, NCHW (logits, bbox_reg, centerness) per level"""
    hw = [tuple(int(v) for v in r) for r in f[name + ".hw"]]
    gb = f[name + ".gt_boxes"]
    N = int(gb[:, 0].max()) + 1
    gts = [gb[gb[:, 0] == i, 1:] for i in range(N)]
    out = []
    for key, c in (("logits", 1), ("bbox_reg", 4), ("centerness", 1)):
        flat, beg, lv = torch.from_numpy(f["%s.%s" % (name, key)]).reshape(-1, c), 0, []
        for h, w in hw:
            lv.append(flat[beg:beg + N * h * w].reshape(N, h, w, c).permute(0, 3, 1, 2).contiguous())
            beg += N * h * w
        out.append(lv)
    return hw, gts, out


@pytest.mark.parametrize("name", ["small", "nonsquare", "shots5"])
def test_restatement_is_the_oracle_in_the_default_mode(name):
    """(True, "giou") on the head outputs of an existing training case: same labels, same targets, losses equal to the last bit."""
    B, H, W, S, qh, qw = gu.CASES[name]
    f = gu.load("train_%s.npz" % name)
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    np.testing.assert_array_equal(np.concatenate(gts, 0), f["gt_boxes"][:, 1:])
    rng = np.random.RandomState(5)
    hw = [(-(-H // s), -(-W // s)) for s in spec.FPN_STRIDES]
    logits = [torch.from_numpy(rng.randn(B, 1, h, w).astype(np.float32)) - 2 for h, w in hw]
    ctr = [torch.from_numpy(rng.randn(B, 1, h, w).astype(np.float32)) for h, w in hw]
    reg = [torch.from_numpy(np.exp(rng.randn(B, 4, h, w).astype(np.float32)) * s) for (h, w), s in zip(hw, spec.FPN_STRIDES)]
    for focal in ("cuda", "cpu"):
        a = orc.fcos_loss(logits, reg, ctr, gts, focal=focal)
        b = flr.fcos_loss(logits, reg, ctr, gts, focal=focal, center_sample=True, loc_loss_type="giou")
        assert torch.equal(a[3]["labels"], b[3]["labels"]) and torch.equal(a[3]["reg_targets"], b[3]["reg_targets"])
        assert a[3]["num_pos"] == b[3]["num_pos"] > 0
        for x, y in zip(a[:3], b[:3]):
            assert x.item() == y.item(), (focal, x.item(), y.item())
    # ... and they are the labels the reference gave for this case
    np.testing.assert_array_equal(b[3]["labels"].numpy().astype(np.int8), f["labels"])
    np.testing.assert_array_equal(b[3]["reg_targets"].numpy(), f["reg_targets"])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("center_sample,loc_loss_type", flr.MODES)
def test_restatement_matches_the_reference_in_every_mode(name, center_sample, loc_loss_type):
    """labels and regression targets exactly, the three losses to rtol 1e-5 (the bound test_oracle_golden holds the oracle to)."""
    f = gu.load("fcos_loss_modes.npz")
    hw, gts, (logits, reg, ctr) = fixture_inputs(f, name)
    key = "%s.cs%d" % (name, center_sample)
    for focal, rec in (("cpu", "losses_ref_cpu_formula"), ("cuda", "losses_cuda_formula")):
        c, r, t, info = flr.fcos_loss(logits, reg, ctr, gts, focal=focal, center_sample=center_sample, loc_loss_type=loc_loss_type)
        np.testing.assert_array_equal(info["labels"].numpy().astype(np.int8), f[key + ".labels"])
        np.testing.assert_array_equal(info["reg_targets"].numpy(), f[key + ".reg_targets"])
        assert info["num_pos"] == int(f["%s.%s.num_pos" % (key, loc_loss_type)])
        np.testing.assert_allclose([c.item(), r.item(), t.item()], f["%s.%s.%s" % (key, loc_loss_type, rec)], rtol=1e-5)


def test_fixture_separates_the_modes():
    """What each case is in the fixture for."""
    f = gu.load("fcos_loss_modes.npz")
    hw, gts, _ = fixture_inputs(f, "quirks")
    npl = [len(gts) * h * w for h, w in hw]
    lab = {cs: f["quirks.cs%d.labels" % cs].astype(np.int64) for cs in (0, 1)}
    assert (gts[0][0, 0] + gts[0][0, 2]) / 2 == 0           # first box of image 0: centre x 0
    per_image = {cs: [sum(int(lab[cs][sum(npl[:l]) + i * h * w:sum(npl[:l]) + (i + 1) * h * w].sum()) for l, (h, w) in enumerate(hw))
                      for i in range(len(gts))] for cs in (0, 1)}
    assert per_image[1][0] == 0 and per_image[0][0] > 0     # get_sample_region's quirk: centre sampling only
    assert per_image[0][1] > per_image[1][1] > 0
    # the regression losses are three different numbers, the assignment changes every loss
    for cs in (0, 1):
        regs = [float(f["quirks.cs%d.%s.losses_cuda_formula" % (cs, lt)][1]) for lt in flr.LOC_LOSS_TYPES]
        assert len(set(round(v, 4) for v in regs)) == 3, regs
    assert not np.allclose(f["quirks.cs0.giou.losses_cuda_formula"], f["quirks.cs1.giou.losses_cuda_formula"], rtol=1e-2)
    # a prediction equal to its target (the gradient's tie rule) at a location positive in both modes
    tie = (f["quirks.bbox_reg"] == f["quirks.cs1.reg_targets"]) & (lab[1] == 1)[:, None] & (lab[0] == 1)[:, None]
    assert tie.any()


def test_restatement_without_boxes_is_all_background():
    """An image without boxes: label 0 everywhere in both modes (the reference itself cannot run it with CENTER_SAMPLE off)."""
    locs = orc.compute_locations([(8, 8), (4, 4), (2, 2), (1, 1), (1, 1)])
    for cs in (True, False):
        lab, reg = flr.fcos_targets(locs, [np.zeros((0, 4), np.float32), np.array([[8, 8, 40, 40]], np.float32)], cs)
        # level-first, then image: image 0 is [0, 64) of P3 and [128, 144) of P4
        assert int(lab[:64].sum()) == 0 and int(lab[128:144].sum()) == 0 and int(lab[64:128].sum()) > 0
        assert float(reg[:64].abs().max()) == 0.0


def test_unknown_loss_type_is_a_value_error_everywhere():
    from oneshotdet_amd import ops, train
    assert (spec.CENTER_SAMPLE, spec.LOC_LOSS_TYPE) == (True, "giou") and spec.LOC_LOSS_TYPES == flr.LOC_LOSS_TYPES
    assert spec.loss_mode(0, "linear_iou") == (False, "linear_iou")
    sd = synth.make_state_dict(spec.hot_path_shapes())
    for bad in ("l1", "GIoU", None, 1):
        with pytest.raises(ValueError, match="loc_loss_type"):
            spec.loss_mode(True, bad)
        with pytest.raises(ValueError, match="loc_loss_type"):          # before the engine looks for a GPU
            train.TrainEngine(sd, loc_loss_type=bad)
    x = torch.zeros(1, 2, 2, 4)
    z = torch.zeros(8)
    with pytest.raises(ValueError, match="loc_loss_type"):
        ops.fcos_loss_level(0, x, x, torch.zeros(1, 1, 4), torch.zeros(1, dtype=torch.int32), 8, -1, 64, 1.5, 2.0, 0.25, None, z,
                            loc_loss_type="smooth_l1")
    with pytest.raises(ValueError, match="loc_loss_type"):
        ops.fcos_loss_levels(0, [(x, x)], torch.zeros(1, 1, 4), torch.zeros(1, dtype=torch.int32), [8], [(-1, 64)], 1.5, 2.0, 0.25,
                             None, z, loc_loss_type="smooth_l1")
    if not torch.cuda.is_available():
        # a valid mode gets as far as the engine's own refusal to run without a GPU
        with pytest.raises(ops._lib.OsdError):
            train.TrainEngine(sd, center_sample=False, loc_loss_type="iou")


def test_c_entries_reject_a_bad_loss_type_before_any_launch():
    """OSD_ERR_INVALID_ARG (-1) + message, no GPU needed; the constants are the header's; the old entries still check theirs."""
    import os
    import re
    from oneshotdet_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oneshotdet_hip.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define OSD_LOC_LOSS_(\w+) (\d+)", header)}
    assert consts == {"GIOU": 0, "IOU": 1, "LINEAR_IOU": 2}
    assert [consts[t.upper()] for t in spec.LOC_LOSS_TYPES] == [0, 1, 2]
    p = ctypes.c_void_p(64)
    i32 = (ctypes.c_int32 * 1)(2)
    fl = (ctypes.c_float * 1)(1.0)
    ptrs = (ctypes.c_void_p * 1)(64)
    for bad in (3, -1, 99):
        rc = lib.osd_fcos_loss_level_opt(0, p, p, p, p, 1, 1, 2, 2, 8, -1.0, 64.0, 1.5, 2.0, 0.25, None, p, None, None, 4, None, 0,
                                         1, bad, None)
        assert rc == -1 and b"loc_loss_type" in lib.osd_last_error_string()
        rc = lib.osd_fcos_loss_levels_opt(0, 1, ptrs, ptrs, p, p, 1, 1, i32, i32, i32, fl, fl, 1.5, 2.0, 0.25, None, p, None, None, 4,
                                          None, 0, 0, bad, None)
        assert rc == -1 and b"loc_loss_type" in lib.osd_last_error_string()
    for lt in (0, 1, 2):
        # valid loss types reach the next checks: a null tensor, and the empty batch that is a no-op
        assert lib.osd_fcos_loss_level_opt(0, None, p, p, p, 1, 1, 2, 2, 8, -1.0, 64.0, 1.5, 2.0, 0.25, None, p, None, None, 4, None,
                                           0, 0, lt, None) == -1
        assert b"null" in lib.osd_last_error_string()
        assert lib.osd_fcos_loss_level_opt(0, p, p, p, p, 1, 0, 2, 2, 8, -1.0, 64.0, 1.5, 2.0, 0.25, None, p, None, None, 4, None,
                                           0, 0, lt, None) == 0
        assert lib.osd_fcos_loss_levels_opt(0, 1, ptrs, ptrs, p, p, 1, 0, i32, i32, i32, fl, fl, 1.5, 2.0, 0.25, None, p, None, None,
                                            4, None, 0, 0, lt, None) == 0
    assert lib.osd_fcos_loss_level(0, None, p, p, p, 1, 1, 2, 2, 8, -1.0, 64.0, 1.5, 2.0, 0.25, None, p, None, None, 4, None, 0,
                                   None) == -1
    assert lib.osd_fcos_loss_levels(0, 1, ptrs, ptrs, p, p, 1, 0, i32, i32, i32, fl, fl, 1.5, 2.0, 0.25, None, p, None, None, 4, None,
                                    0, None) == 0


def test_training_checkpoint_records_the_loss_and_refuses_a_mismatch(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.hot_path_shapes()).items()}
    mode = (False, "iou")
    p = str(tmp_path / "model_0000010.pth")
    checkpoint.save_training_checkpoint(p, FakeEngine(sd, center_sample=mode[0], loc_loss_type=mode[1]), 10)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert raw["center_sample"] is False and raw["loc_loss_type"] == "iou" and raw["supp_roialign"] is True
    eng, it = checkpoint.resume_training(p, lambda s: FakeEngine(s, center_sample=mode[0], loc_loss_type=mode[1]), center_sample=False, loc_loss_type="iou")
    assert it == 10 and eng.opt_state["steps"] == 3 and all(torch.equal(eng.sd[k], sd[k]) for k in sd)
    checkpoint.resume_training(p, lambda s: FakeEngine(s, center_sample=mode[0], loc_loss_type=mode[1]))               # the caller need not say it: the file does
    checkpoint.resume_training(p, lambda s: FakeEngine(s, center_sample=mode[0], loc_loss_type=mode[1]), loc_loss_type="iou")
    # the caller expects another loss: refused before make_engine, naming both
    called = []
    for kw in ({"center_sample": True}, {"loc_loss_type": "giou"}, {"center_sample": True, "loc_loss_type": "linear_iou"}):
        with pytest.raises(ValueError) as e:
            checkpoint.resume_training(p, lambda s: called.append(1), **kw)
        msg = str(e.value)
        assert "center_sample=False, loc_loss_type='iou'" in msg and "whole-box iou" in msg, msg
        want = (kw.get("center_sample", False), kw.get("loc_loss_type", "iou"))
        assert "center_sample=%r, loc_loss_type=%r" % want in msg, msg
    assert not called
    with pytest.raises(ValueError, match="loc_loss_type"):
        checkpoint.resume_training(p, lambda s: called.append(1), loc_loss_type="l1")
    # make_engine builds another loss than the file's: refused after it, naming both
    for other in ((True, "giou"), (False, "giou"), (True, "iou")):
        with pytest.raises(ValueError) as e:
            checkpoint.resume_training(p, lambda s: FakeEngine(s, center_sample=other[0], loc_loss_type=other[1]))
        assert "whole-box iou" in str(e.value) and "center_sample=%r, loc_loss_type=%r" % other in str(e.value)
    # the weights' keys do not depend on the loss
    p2 = str(tmp_path / "model_default.pth")
    checkpoint.save_training_checkpoint(p2, FakeEngine(sd, center_sample=True, loc_loss_type="giou"), 5)
    a, _ = checkpoint.load_checkpoint(p)
    b, _ = checkpoint.load_checkpoint(p2)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # an engine without the attributes is the default mode; a file without the fields (every file written before) is (True, "giou")
    p3 = str(tmp_path / "model_old.pth")
    checkpoint.save_training_checkpoint(p3, FakeEngine(sd), 7)
    raw3 = torch.load(p3, map_location="cpu", weights_only=False)
    assert raw3["center_sample"] is True and raw3["loc_loss_type"] == "giou"
    del raw3["center_sample"], raw3["loc_loss_type"]
    torch.save(raw3, p3)
    eng, it = checkpoint.resume_training(p3, lambda s: FakeEngine(s), center_sample=True, loc_loss_type="giou")
    assert it == 7
    checkpoint.resume_training(p3, lambda s: FakeEngine(s, center_sample=True, loc_loss_type="giou"))
    with pytest.raises(ValueError, match="centre-sampled giou"):
        checkpoint.resume_training(p3, lambda s: FakeEngine(s, center_sample=mode[0], loc_loss_type=mode[1]), center_sample=False, loc_loss_type="iou")
    with pytest.raises(ValueError, match="centre-sampled giou"):
        checkpoint.resume_training(p3, lambda s: FakeEngine(s, center_sample=mode[0], loc_loss_type=mode[1]))
    # plain save_checkpoint is untouched: weights only
    p4 = str(tmp_path / "weights.pth")
    checkpoint.save_checkpoint(p4, sd)
    assert set(torch.load(p4, map_location="cpu", weights_only=False)) == {"model"}
