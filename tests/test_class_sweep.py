"""CPU: the class sweep (K category slots per target image in one pass) as far as it goes without a device — the two entries' argument checks (they
return before any device call; the boundary's header, table and exports are tests/test_abi.py's), modules.merge_class_detections on hand-made tensors, the `classes` keyword of the engine, and the
documents that name the option."""
import ctypes
import inspect
import os

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)

@pytest.fixture(scope="module")
def lib():
    from oneshotdet_amd import _lib, build
    build.build_library(verbose=False)
    return _lib.load()


def _arrays(n_levels=2, null_at=None):
    """host arrays of fake, never dereferenced device addresses"""
    def arr(base):
        return (ctypes.c_void_p * n_levels)(*[None if null_at == l else base + 4096 * l for l in range(n_levels)])
    return arr(0x10000), arr(0x20000), arr(0x30000), (ctypes.c_int32 * n_levels)(*([12] * n_levels))


def test_correlate_sweep_argument_checks_need_no_device(lib):
    f = lib.osd_correlate_levels_sweep
    xs, qs, ys, hws = _arrays()
    bad = [
        (2, None, qs, ys, hws, 2, 3, 64, 0, None),                  # null arrays
        (2, xs, None, ys, hws, 2, 3, 64, 0, None),
        (2, xs, qs, None, hws, 2, 3, 64, 0, None),
        (2, xs, qs, ys, None, 2, 3, 64, 0, None),
        (2, _arrays(null_at=1)[0], qs, ys, hws, 2, 3, 64, 0, None),   # a null tensor at a level
        (2, xs, _arrays(null_at=0)[1], ys, hws, 2, 3, 64, 0, None),
        (2, xs, qs, _arrays(null_at=1)[2], hws, 2, 3, 64, 0, None),
        (2, xs, qs, ys, hws, 2, 0, 64, 0, None),                    # classes < 1
        (2, xs, qs, ys, hws, 2, -4, 64, 0, None),
        (0, xs, qs, ys, hws, 2, 3, 64, 0, None),                    # levels
        (7, xs, qs, ys, hws, 2, 3, 64, 0, None),
        (2, xs, qs, ys, hws, -1, 3, 64, 0, None),                   # n < 0
        (2, xs, qs, ys, hws, 2, 3, 60, 1, None),                    # channels: no multiple of a bf16 chunk
        (2, xs, qs, ys, hws, 2, 3, 4096, 0, None),                  # more than the staged group holds
        (2, xs, qs, ys, hws, 2, 3, 64, 7, None),                    # dtype
    ]
    for args in bad:
        assert f(*args) == -1, args
        assert lib.osd_last_error_string()
    assert f(2, xs, qs, ys, hws, 0, 3, 64, 0, None) == 0            # an empty batch is a no-op
    assert f(2, xs, qs, ys, hws, 0, 1, 256, 1, None) == 0
    assert f(2, xs, qs, ys, (ctypes.c_int32 * 2)(0, 0), 2, 3, 64, 0, None) == 0     # nothing but empty levels


def test_roi_pool_sweep_argument_checks_need_no_device(lib):
    f = lib.osd_roi_pool_levels_sweep
    xs = _arrays()[0]
    hs, ws = (ctypes.c_int32 * 2)(8, 4), (ctypes.c_int32 * 2)(8, 4)
    sc = (ctypes.c_float * 2)(0.125, 0.0625)
    boxes, y = ctypes.c_void_p(0x40000), ctypes.c_void_p(0x50000)

    def call(n_levels=2, xs=xs, hs=hs, ws=ws, sc=sc, boxes=boxes, y=y, n_sets=6, sets=3, c=64, rois=7, pool=7, stride=64, dtype=0):
        return f(n_levels, xs, hs, ws, sc, boxes, None, y, n_sets, sets, c, rois, pool, 2, stride, None, dtype, None)
    for kw in (dict(xs=None), dict(hs=None), dict(ws=None), dict(sc=None), dict(boxes=None), dict(y=None),       # null pointers
               dict(xs=_arrays(null_at=1)[0]),
               dict(n_sets=7, sets=3), dict(n_sets=6, sets=4), dict(n_sets=2, sets=3),                           # n_sets % sets_per_image != 0
               dict(sets=0), dict(sets=-1),
               dict(n_levels=0), dict(n_levels=9), dict(c=62), dict(c=60, dtype=1), dict(stride=32), dict(pool=0), dict(dtype=5)):
        assert call(**kw) == -1, kw
        assert lib.osd_last_error_string()
    assert call(n_sets=0) == 0                                       # an empty batch is a no-op
    assert call(rois=0) == 0


def _hand_made():
    """B = 2, K = 3, R = 4: counts 2, 0, 3 | 0, 0, 0 — ragged with zeros, image 1 has no detection at all.  Rows past a count hold
    values that would show up if they were read (score 9)."""
    scores = torch.full((6, 4), 9.0)
    scores[0, :2] = torch.tensor([0.9, 0.5])
    scores[2, :3] = torch.tensor([0.9, 0.7, 0.5])
    boxes = torch.arange(6 * 4 * 4, dtype=torch.float32).reshape(6, 4, 4)
    counts = torch.tensor([2, 0, 3, 0, 0, 0], dtype=torch.int32)
    return boxes, scores, counts


def test_merge_class_detections_orders_labels_and_keeps_empty_images():
    from oneshotdet_amd.modules import merge_class_detections
    boxes, scores, counts = _hand_made()
    ids = [[7, 3, 12], [5, 6, 2]]
    out = merge_class_detections(boxes, scores, counts, ids, [(96, 160), (80, 120)])
    assert len(out) == 2
    a, b = out
    # descending by score; 0.9 and 0.5 are ties between slot 0 and slot 2: the lower slot first
    assert a.get_field("scores").tolist() == pytest.approx([0.9, 0.9, 0.7, 0.5, 0.5])
    assert a.get_field("labels").tolist() == [7, 12, 12, 7, 12]
    assert a.get_field("labels").dtype == torch.int64
    want = torch.stack([boxes[0, 0], boxes[2, 0], boxes[2, 1], boxes[0, 1], boxes[2, 2]])
    assert torch.equal(a.bbox, want)
    assert a.size == (160, 96) and a.mode == "xyxy"
    # the image without detections: an empty BoxList that still has its fields
    assert len(b) == 0 and tuple(b.bbox.shape) == (0, 4) and b.size == (120, 80)
    assert b.has_field("scores") and b.has_field("labels")
    assert b.get_field("scores").shape == (0,) and b.get_field("labels").shape == (0,) and b.get_field("labels").dtype == torch.int64


def test_merge_class_detections_ties_within_a_slot_keep_their_rank_and_ids_may_be_shared():
    from oneshotdet_amd.modules import merge_class_detections
    scores = torch.tensor([[0.5, 0.5, 0.5], [0.8, 0.5, 0.1]])
    boxes = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    counts = torch.tensor([3, 2], dtype=torch.int32)
    (bl,) = merge_class_detections(boxes, scores, counts, [4, 9], [(10, 20)])          # one flat list of K ids: shared by all images
    assert bl.get_field("labels").tolist() == [9, 4, 4, 4, 9]
    assert torch.equal(bl.bbox, torch.stack([boxes[1, 0], boxes[0, 0], boxes[0, 1], boxes[0, 2], boxes[1, 1]]))
    with pytest.raises(ValueError):
        merge_class_detections(boxes, scores, counts, [[4, 9, 1]], [(10, 20)])         # 2 rows are not 1 image x 3 ids
    with pytest.raises(ValueError):
        merge_class_detections(boxes, scores, counts, [[4], [9, 1]], [(10, 20), (10, 20)])


def test_merged_boxlists_are_what_eval_detection_voc_reads():
    """fields and types only: the evaluation itself runs on the device (tests/test_gpu_class_sweep.py)"""
    from oneshotdet_amd.modules import merge_class_detections
    boxes, scores, counts = _hand_made()
    for bl in merge_class_detections(boxes, scores, counts, [[1, 2, 3]] * 2, [(96, 160)] * 2):
        assert bl.bbox.dtype == torch.float32 and bl.get_field("scores").dtype == torch.float32
        assert len(bl) == bl.get_field("scores").shape[0] == bl.get_field("labels").shape[0]


def test_classes_keyword_defaults_to_one_everywhere():
    from oneshotdet_amd import box_head, model, ops
    for name in ("forward_features", "forward", "detect", "tune", "box_detect"):
        p = inspect.signature(getattr(model.HotPathEngine, name)).parameters
        assert "classes" in p and p["classes"].default == 1, name
    p = inspect.signature(box_head.run_box_head).parameters
    assert p["classes"].default == 1
    assert inspect.signature(ops.roi_pool_levels).parameters["sets_per_image"].default == 1
    assert list(inspect.signature(ops.correlate_levels_sweep).parameters) == ["xs", "qs", "classes"]
    assert inspect.signature(model.run_correlate).parameters["classes"].default == 1


def test_row_rule_is_refused_with_both_numbers_before_anything_runs():
    from oneshotdet_amd import model
    assert model.check_classes(2, 12, 3) == 2
    with pytest.raises(ValueError) as e:
        model.check_classes(2, 13, 3)
    assert "13" in str(e.value) and "6" in str(e.value)
    with pytest.raises(ValueError):
        model.check_classes(2, 12, 0)


def test_documents_example_and_profile_name_the_sweep():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    assert "oneshotdet_hip.h" in read("README.md") and "classes=" in read("README.md")
    design = read("DESIGN.md")
    assert "### 4.5k" in design and design.index("### 4.5j") < design.index("### 4.5k") < design.index("## 5. Measurement")
    assert "classes=K" in design and "osd_correlate_levels_sweep" in design and "osd_roi_pool_levels_sweep" in design
    integ = read("INTEGRATION.md")
    assert "classes=" in integ and "engine/inference.py" in integ and "merge_class_detections" in integ
    assert "--classes" in read("examples", "detect.py")
    assert "bench_class_sweep.py" in read("tools", "README.md") and os.path.exists(os.path.join(ROOT, "tools", "bench_class_sweep.py"))
    prof = read("profiles", "class_sweep.md")
    assert "classes=K" in prof and "G = " in prof
