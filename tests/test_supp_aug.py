"""CPU: query augmentation groups (FEW_SHOT.SUPP_AUG, SUPP_AUG_METHOD 'avg' / 'max'): the validator and the three constructors'
keywords, the group-size rule, the tie rule the 'max' backward follows (pinned against torch on the CPU), the fixtures' own
near-tie record, and what the documents and examples say."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import golden_utils as gu
import supp_aug_ref as sar
from oneshotdet_amd import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- validation
def test_supp_aug_mode_accepts_and_refuses_by_config_name():
    assert spec.supp_aug_mode() == (1, "avg")
    assert spec.supp_aug_mode(2, "max") == (2, "max") and spec.supp_aug_mode(8, "avg") == (8, "avg")
    assert spec.supp_aug_mode(1, "max", neg_support=True) == (1, "max")          # off: nothing to combine
    a, m = spec.supp_aug_mode(np.int64(3), "avg")
    assert type(a) is int and type(m) is str
    for bad in (0, 9, -1, 2.5, True, "2"):
        with pytest.raises(ValueError, match="NUM_SUPP_AUG"):
            spec.supp_aug_mode(bad, "avg")
    with pytest.raises(ValueError, match="SUPP_AUG_METHOD"):
        spec.supp_aug_mode(2, "median")
    with pytest.raises(ValueError, match=r"SUPP_AUG_METHOD.*supp_aug_conv\.0\.weight"):
        spec.supp_aug_mode(2, "conv")
    with pytest.raises(ValueError, match="supp_aug_conv"):        # 'conv' is refused whether the option is on or not
        spec.supp_aug_mode(1, "conv")
    with pytest.raises(ValueError, match=r"FEW_SHOT\.SUPP_AUG.*FEW_SHOT\.NEG_SUPPORT"):
        spec.supp_aug_mode(2, "avg", neg_support=True)


def test_the_keywords_are_not_model_options_or_checkpoint_fields():
    """like `shots`: no row in spec.MODEL_OPTIONS (tests/test_model_options.py pins its 9 rows and the checkpoint's fields)"""
    assert len(spec.MODEL_OPTIONS) == 9
    assert not any("aug" in name for name in spec.MODEL_OPTIONS)
    from oneshotdet_amd import checkpoint
    assert "supp_aug" not in inspect.getsource(checkpoint)


def _constructors():
    from oneshotdet_amd import model, modules, train
    return [train.TrainEngine, model.HotPathEngine, modules.OneShotDetector]


def test_constructors_take_the_keywords_with_the_off_defaults():
    for ctor in _constructors():
        p = inspect.signature(ctor.__init__).parameters
        assert p["supp_aug"].default == 1 and p["supp_aug_method"].default == "avg", ctor


@pytest.mark.parametrize("kw,match", [(dict(supp_aug=2, supp_aug_method="conv"), "supp_aug_conv"),
                                      (dict(supp_aug=2, supp_aug_method="sum"), "SUPP_AUG_METHOD"),
                                      (dict(supp_aug=9), "NUM_SUPP_AUG"), (dict(supp_aug=0), "NUM_SUPP_AUG"),
                                      (dict(supp_aug=2, neg_support=True), "NEG_SUPPORT")])
def test_constructors_refuse_before_any_gpu_use(kw, match, monkeypatch):
    """validated first thing: the ValueError comes before the state_dict is looked at, the library loaded or the GPU asked for"""
    from oneshotdet_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the keywords were validated"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU was asked for before the keywords were validated"))
    for ctor in _constructors():
        extra = {"second_stage": True} if ctor.__name__ == "TrainEngine" else {}
        with pytest.raises(ValueError, match=match):
            ctor({}, **kw, **extra)


def test_group_query_sizes():
    sizes = [(63, 63), (63, 63), (96, 80), (96, 80)]
    assert spec.group_query_sizes(sizes, 1) == sizes
    assert spec.group_query_sizes(sizes, 2) == [(63, 63), (96, 80)]
    assert spec.group_query_sizes([torch.Size(s) for s in sizes], 2) == [(63, 63), (96, 80)]
    with pytest.raises(ValueError, match=r"group 1 \(rows 2 \.\. 3\).*generalized_rcnn\.py:236-250"):
        spec.group_query_sizes([(63, 63), (63, 63), (96, 80), (80, 96)], 2)
    with pytest.raises(ValueError, match="no multiple of supp_aug = 3"):
        spec.group_query_sizes(sizes, 3)


# ------------------------------------------------------------------------------------------------------------- the tie rule
def test_torch_cpu_max_backward_gives_a_tie_to_the_lowest_member():
    """What osd_supp_aug_reduce_levels_bwd restates: x.view(G, A, ...).max(1)'s CPU backward sends the whole gradient to the first
    member that attains the maximum — [1, 1, 1] -> member 0 — and nothing to the others."""
    x = torch.tensor([[1.0, 1.0, 1.0], [0.0, 2.0, 2.0], [3.0, -1.0, 3.0], [0.5, 0.25, 4.0]], requires_grad=True)      # [G = 4, A = 3]
    y = x.max(dim=1)[0]
    y.backward(torch.tensor([10.0, 20.0, 30.0, 40.0]))
    assert x.grad.tolist() == [[10.0, 0.0, 0.0], [0.0, 20.0, 0.0], [30.0, 0.0, 0.0], [0.0, 0.0, 40.0]]
    # through the merge as the generator and the GPU tests write it, on maps
    g = torch.Generator().manual_seed(0)
    xm = (torch.randint(0, 4, (6, 3, 2, 2), generator=g).float()).requires_grad_(True)       # 2 groups of 3, ties everywhere
    dy = torch.randn(2, 3, 2, 2, generator=g)
    sar.merge(xm, 3, "max").backward(dy)
    grouped = xm.detach().view(2, 3, 3, 2, 2)
    first = grouped.argmax(dim=1)
    assert bool((grouped == grouped.max(dim=1, keepdim=True)[0]).sum(dim=1).max() > 1)           # there are ties
    want = torch.zeros_like(grouped).scatter_(1, first.unsqueeze(1), dy.unsqueeze(1))
    # argmax returns the first maximal index too; the gradient went there and only there
    assert torch.equal(xm.grad.view(2, 3, 3, 2, 2), want)


def test_closed_forms_of_the_helper():
    x = np.array([[1.0, 3.0], [2.0, 4.0], [1e-8, 1.0], [1.0, 3.0], [5.0, 5.0], [7.0, 9.0]], np.float32)
    np.testing.assert_array_equal(sar.avg_closed_form(x, 2), np.array([[1.5, 3.5], [0.5, 2.0], [6.0, 7.0]], np.float32))
    three = sar.avg_closed_form(x, 3)
    np.testing.assert_array_equal(three[0], ((x[0] + x[1]) + x[2]) / np.float32(3))
    q = np.arange(24, dtype=np.float32).reshape(2, 3, 2, 2)
    aq = sar.aug_queries(q)
    assert aq.shape == (4, 3, 2, 2) and np.array_equal(aq[0], q[0]) and np.array_equal(aq[1], q[0][..., ::-1])
    assert np.array_equal(aq[2], q[1]) and np.array_equal(sar.aug_queries(torch.from_numpy(q)).numpy(), aq)
    assert sar.within_one_ulp(np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)))
    assert not sar.within_one_ulp(np.float32(1.0), np.float32(1.0) + np.float32(3e-7))


# ------------------------------------------------------------------------------------------------------------- fixtures
def test_fixtures_exist_and_record_the_near_ties():
    for method, case, shared in sar.FORWARD_CASES:
        f = gu.load(sar.forward_name(method, case, shared))
        B, H, W, S, qh, qw = gu.CASES[case]
        assert tuple(f["query_features.0.shape"])[0] == B * S and tuple(f["query_features_unmerged.0.shape"])[0] == B * S * sar.AUG
        assert f["head"].shape[0] == B
        if method == "max":
            _check_near_ties(f, [(qh + 31) // 32 * 32, (qw + 31) // 32 * 32])
    for method, case, roialign in sar.TRAIN_CASES:
        f = gu.load(sar.train_name(method, case))
        assert bool(f["supp_roialign"]) == roialign
        own = [k for k in f.files if k.startswith("refgrad.supp_backbone.") and k.endswith(".samples")]
        assert (len(own) >= 5) == (not roialign)          # the reference's own query-backbone gradients where it has a backward
        assert any(k.startswith("fullgrad_oracle.supp_backbone.") for k in f.files)
        if method == "max":
            assert "near_ties.count_1e-6" in f.files
    assert gu.load("box_suppaug_max_small.npz")["detections.0.boxes"].shape[1] == 4
    biggest = max(os.path.getsize(os.path.join(gu.GOLDEN_DIR, n)) for n in os.listdir(gu.GOLDEN_DIR)
                  if re.match(r"(case|train)_(?!suppaug)", n))
    for n in os.listdir(gu.GOLDEN_DIR):
        if "suppaug" in n:
            assert os.path.getsize(os.path.join(gu.GOLDEN_DIR, n)) <= biggest, n


def _check_near_ties(f, padded):
    count, share, first = f["near_ties.count_1e-6"], f["near_ties.share_1e-4"], f["near_ties.member0_share"]
    assert count.shape == share.shape == first.shape == (5,)
    for lvl, (h, w) in enumerate(spec.level_sizes(*padded)):
        if h * w <= 4:
            assert count[lvl] == 0, lvl          # one flipped element there is a whole row of a weight gradient
    assert share.max() <= 0.005                                   # an fp32 engine does not flip these inputs ...
    assert 0.4 <= first.min() and first.max() <= 0.6              # ... and both members win: the routing is exercised


# ------------------------------------------------------------------------------------------------------------- documents
def _doc(name):
    return open(os.path.join(ROOT, name)).read()


def test_documents_name_the_option():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        text = _doc(doc)
        assert "supp_aug" in text and "SUPP_AUG" in text, doc
    integ, design = _doc("INTEGRATION.md"), _doc("DESIGN.md")
    assert "oneshotdet_hip_supp_aug.h" in integ and "osd_supp_aug_reduce_levels_bwd" in integ
    section = integ[integ.index("FEW_SHOT.SUPP_AUG"):]
    assert "not recorded" in section and "checkpoint" in section           # like `shots`, the keywords are no checkpoint field
    for word in ("lowest", "rounded once", "one launch", "profiles/supp_aug.md"):
        assert word in design, word
    assert "supp_aug.hip" in _doc("README.md")
    assert os.path.exists(os.path.join(ROOT, "profiles", "supp_aug.md")) and os.path.exists(os.path.join(ROOT, "tools", "bench_supp_aug.py"))


@pytest.mark.parametrize("doc", ["INTEGRATION.md", "DESIGN.md"])
def test_still_refused_sentence(doc):
    text = _doc(doc)
    sentence = text[text.index("Still refused by name"):]
    sentence = sentence[:sentence.index("\n\n")]
    for word in ("LOSS_WEIGHTED", "NEG_SUPPORT", "SECOND_STAGE_METHOD", "'rn'", "'matching'", "REVERSE_ORDER", "SUPP_AUG"):
        assert word in sentence, word
    assert "with any loss but 'ce_loss', with more than one shot" in sentence and "LINEAR_FUSION" not in sentence
    # what stays refused of the option, and no longer the option itself
    assert "`SUPP_AUG_METHOD` 'conv'" in sentence and "`SUPP_AUG` with a negative support" in sentence
    assert not re.search(r"`REVERSE_ORDER`, `SUPP_AUG`\.", sentence)


def test_examples_take_the_flags():
    for ex in ("train.py", "detect.py"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert '"--supp-aug"' in src and '"--supp-aug-method"' in src and "spec.supp_aug_mode(" in src, ex
        assert "supp_aug=supp_aug, supp_aug_method=supp_aug_method" in src, ex
    src = open(os.path.join(ROOT, "examples", "train.py")).read()
    assert "supp_aug=supp_aug == 2" in src and "colour" in src          # the dataset's flip rows; other group sizes refused there
