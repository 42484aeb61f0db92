"""CPU: spec.MODEL_OPTIONS, the one table of the model's configuration options, against everything that derives from it: the
constructors' keywords, spec.check_options, the fields of a training checkpoint and the three phases of checkpoint.resume_training
(read the file's record, refuse a caller's other expectation before make_engine, refuse another built engine after it).

The state_dicts here have the model's shapes and one element of storage each (a zero expanded to the shape): the checkpoint code
looks at keys and shapes only, and a file is a few hundred kilobytes instead of a quarter of a gigabyte.

Precedence pins: which option is blamed when two are wrong was recorded from the commit before the table existed, by running the
same calls against it; the expectations below are those answers as literals."""
import inspect

import pytest
import torch

from fake_engine import FakeEngine
from oneshotdet_amd import checkpoint, model, modules, spec, train
from oneshotdet_amd.box_head import BoxHeadWeights

ROWS = spec.MODEL_OPTIONS
DEFAULTS = {name: row.default for name, row in ROWS.items()}
# one non-default value per row; each is a valid model on its own next to the other rows' defaults
OTHER = {"siamese_backbone": False, "supp_roialign": False, "center_sample": False, "loc_loss_type": "iou", "box_cls_loss": "focal_loss",
         "soft_labeling": True, "soft_labeling_func": "transLinear", "linear_fusion": True, "neg_support": True}
# what else a file needs for the row to matter: the function only counts where soft labels are on
NEEDS = {"soft_labeling_func": {"soft_labeling": True}}


class _Engine(FakeEngine):
    def optimizer_state_dict(self):
        return {"momentum_buffer": {}, "steps": 3, "lr": 0.01, "momentum": 0.9, "weight_decay": 1e-4}


def _sd(options):
    shapes = spec.full_model_shapes(**{name: options[name] for name in spec.SHAPE_OPTIONS})
    return {k: torch.zeros(()).expand(s) for k, s in shapes.items()}


def _file(tmp_path, options, drop=()):
    """A training checkpoint of a model with these options (the rows' defaults for the others), without the fields in `drop`."""
    options = dict(DEFAULTS, **options)
    p = str(tmp_path / "model.pth")
    checkpoint.save_training_checkpoint(p, _Engine(_sd(options), **options), 4)
    if drop:
        raw = torch.load(p, map_location="cpu", weights_only=False)
        for name in drop:
            del raw[name]
        torch.save(raw, p)
    return p, options


def _option_parameters(fn):
    return {n: p for n, p in inspect.signature(fn).parameters.items() if n in ROWS}


def test_every_row_is_a_keyword_with_the_rows_default():
    assert len(ROWS) == 9 and set(OTHER) == set(ROWS) and all(OTHER[n] != DEFAULTS[n] for n in ROWS)
    assert spec.ModelOptions._fields == tuple(ROWS)
    assert [n for names in spec.OPTION_GROUPS.values() for n in names] == list(ROWS)
    assert (spec.SIAMESE_BACKBONE, spec.SUPP_ROIALIGN) == (True, True)
    eng, resume = _option_parameters(train.TrainEngine.__init__), _option_parameters(checkpoint.resume_training)
    assert list(eng) == list(ROWS) == list(resume)                              # the table's order is the signatures'
    for name, row in ROWS.items():
        assert eng[name].default == row.default and type(eng[name].default) is type(row.default), name
        assert resume[name].default is None, name
    inference = [n for n, row in ROWS.items() if row.scope != "fcos_loss"]
    assert [n for n in ROWS if n not in inference] == ["center_sample", "loc_loss_type"]
    for fn in (model.HotPathEngine.__init__, modules.OneShotDetector.__init__):
        got = _option_parameters(fn)
        assert list(got) == inference and all(got[n].default == ROWS[n].default for n in got)
    got = _option_parameters(BoxHeadWeights.__init__)
    assert got and all(ROWS[n].scope == "second_stage" and got[n].default == ROWS[n].default for n in got)
    assert spec.SHAPE_OPTIONS == ("siamese_backbone", "box_cls_loss", "soft_labeling", "linear_fusion")
    for fn in (spec.full_model_shapes, checkpoint.load_checkpoint, checkpoint.load_c2_resnet):
        got = _option_parameters(fn)
        assert list(got) == list(spec.SHAPE_OPTIONS) and all(got[n].default == ROWS[n].default for n in got)
    for fn in (train.TrainEngine.__init__, model.HotPathEngine.__init__, modules.OneShotDetector.__init__, BoxHeadWeights.__init__,
               checkpoint.resume_training):
        assert all(p.kind is p.POSITIONAL_OR_KEYWORD for p in _option_parameters(fn).values())       # none positional-only


def test_check_options_returns_the_validated_values():
    got = spec.check_options("the test", False)
    assert got == spec.ModelOptions(**DEFAULTS) and got._asdict() == DEFAULTS
    got = spec.check_options("the test", True, siamese_backbone=0, center_sample=0, loc_loss_type="linear_iou", box_cls_loss="cxe_loss",
                             soft_labeling=1, soft_labeling_func="discrete", linear_fusion=1)
    assert got == (False, True, False, "linear_iou", "cxe_loss", True, "discrete", True, False)
    assert all(type(v) is type(DEFAULTS[n]) for n, v in got._asdict().items())
    assert spec.check_options("the test", True, neg_support=1).neg_support is True
    with pytest.raises(TypeError):
        spec.check_options("the test", True, no_such_option=1)
    assert spec.options_in(dict(self=1, neg_support=True, dtype=2, loc_loss_type="iou")) == dict(neg_support=True, loc_loss_type="iou")
    assert spec.describe_group("fcos_loss", (False, "iou")) == "the whole-box iou FCOS loss (center_sample=False, loc_loss_type='iou')"
    assert spec.describe_group("fcos_loss", (True, "giou"), words=False) == "center_sample=True, loc_loss_type='giou'"
    assert spec.describe_group("neg_support", (True,)) == "neg_support=True"


def test_a_training_checkpoint_holds_exactly_the_rows(tmp_path):
    p, _ = _file(tmp_path, {})
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert set(raw) == {"model", "optimizer", "iteration"} | set(ROWS)
    assert all(raw[n] is DEFAULTS[n] if isinstance(DEFAULTS[n], bool) else raw[n] == DEFAULTS[n] and type(raw[n]) is str for n in ROWS)
    # an engine without the attributes means the defaults; truthy / falsy attributes are recorded as bool
    assert checkpoint.engine_options(FakeEngine({})) == DEFAULTS
    assert checkpoint.engine_options(FakeEngine({}, neg_support=1, supp_roialign=0))["neg_support"] is True
    options = dict(DEFAULTS, siamese_backbone=False, supp_roialign=False, center_sample=False, loc_loss_type="iou", box_cls_loss="l1_loss",
                   soft_labeling=True, soft_labeling_func="transLinear", linear_fusion=True)
    p, _ = _file(tmp_path, options)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert {n: raw[n] for n in ROWS} == options and raw["soft_labeling"] is True and raw["siamese_backbone"] is False
    eng, it = checkpoint.resume_training(p, lambda s: _Engine(s, **options), **options)
    assert it == 4 and eng.opt_state["steps"] == 3 and checkpoint.engine_options(eng) == options


def _refusals(p, trained, name, other):
    """The file was trained with `trained`; for the row `name` the caller, then the built engine, have `other` instead."""
    group = ROWS[name].group
    names = spec.OPTION_GROUPS[group]
    was = spec.describe_group(group, tuple(trained[n] for n in names))
    now = spec.describe_group(group, tuple(other if n == name else trained[n] for n in names))
    configs = [ROWS[n].config for n in names]
    called = []
    with pytest.raises(ValueError) as e:
        checkpoint.resume_training(p, lambda s: called.append(1), **{name: other})
    msg = str(e.value)
    assert called == [] and p in msg and was in msg and now in msg and all(c in msg for c in configs), msg
    assert "build the engine with " + spec.describe_group(group, tuple(trained[n] for n in names), words=False) in msg, msg   # what to pass
    with pytest.raises(ValueError) as e:
        checkpoint.resume_training(p, lambda s: called.append(1) or _Engine(s, **dict(trained, **{name: other})))
    msg = str(e.value)
    assert called == [1] and p in msg and was in msg and all(c in msg for c in configs), msg
    assert "make_engine built an engine with " + now in msg, msg


@pytest.mark.parametrize("name", list(ROWS))
@pytest.mark.parametrize("file_has", ["default", "other"])
def test_one_option_differing_is_refused_before_and_after_make_engine(tmp_path, name, file_has):
    file_value, other = (DEFAULTS[name], OTHER[name]) if file_has == "default" else (OTHER[name], DEFAULTS[name])
    p, trained = _file(tmp_path, dict(NEEDS.get(name, {}), **{name: file_value}))
    _refusals(p, trained, name, other)
    # the caller says nothing: whatever the file holds; or says what it holds
    eng, it = checkpoint.resume_training(p, lambda s: _Engine(s, **trained))
    assert it == 4 and checkpoint.engine_options(eng) == trained and list(eng.sd) == list(_sd(trained))
    checkpoint.resume_training(p, lambda s: _Engine(s, **trained), **{name: file_value})


def test_the_function_is_moot_without_soft_labels(tmp_path):
    p, trained = _file(tmp_path, {})
    checkpoint.resume_training(p, lambda s: _Engine(s, **trained), soft_labeling_func="transLinear")
    checkpoint.resume_training(p, lambda s: _Engine(s, **dict(trained, soft_labeling_func="transLinear")))


def test_a_file_without_the_fields_resumes_as_the_defaults(tmp_path):
    p, _ = _file(tmp_path, {}, drop=list(ROWS))
    assert not set(torch.load(p, map_location="cpu", weights_only=False)) & set(ROWS)
    eng, it = checkpoint.resume_training(p, lambda s: FakeEngine(s))
    assert it == 4 and list(eng.sd) == list(spec.full_model_shapes())
    checkpoint.resume_training(p, lambda s: _Engine(s, **DEFAULTS), **DEFAULTS)
    for name in ROWS:
        if name == "soft_labeling_func":
            continue                     # moot while the file's soft_labeling is off (the test above)
        _refusals(p, DEFAULTS, name, OTHER[name])
    # siamese_backbone of such a file: whether it holds supp_backbone.*
    shared = dict(DEFAULTS, siamese_backbone=False)
    p, _ = _file(tmp_path, shared, drop=list(ROWS))
    eng, _ = checkpoint.resume_training(p, lambda s: _Engine(s, **shared))
    assert not any(k.startswith("supp_backbone.") for k in eng.sd)
    _refusals(p, shared, "siamese_backbone", True)


# ---- precedence pins (recorded from the commit before the table) ---------------------------------------------------------------

@pytest.mark.parametrize("expected, blamed", [
    (dict(neg_support=True, linear_fusion=True), r"trained with neg_support=False .*resuming it with neg_support=True"),
    (dict(linear_fusion=True, soft_labeling=True), r"trained with linear_fusion=False .*resuming it with linear_fusion=True"),
    (dict(soft_labeling=True, box_cls_loss="focal_loss"), r"trained with soft_labeling=False, soft_labeling_func='linear' .*resuming it with soft_labeling=True"),
    (dict(box_cls_loss="focal_loss", loc_loss_type="iou"), r"trained with box_cls_loss='ce_loss' .*resuming it with box_cls_loss='focal_loss'"),
    (dict(center_sample=False, supp_roialign=False), r"trained with the centre-sampled giou FCOS loss .*resuming it with the whole-box giou FCOS loss"),
    (dict(supp_roialign=False, siamese_backbone=False), r"trained with ROIAlign query pooling .*resuming it with global-average query pooling"),
    (dict(neg_support=True, siamese_backbone=False), r"trained with neg_support=False .*resuming it with neg_support=True"),
    # a value no validator knows is reported where its group is looked at: after a mismatch of an earlier group, before a later one
    (dict(box_cls_loss="focal_loss", soft_labeling_func="cubic"), r"^soft_labeling_func must be one of"),
    (dict(loc_loss_type="l1", box_cls_loss="focal_loss"), r"trained with box_cls_loss='ce_loss' .*resuming it with box_cls_loss='focal_loss'"),
    (dict(loc_loss_type="l1", supp_roialign=False), r"^loc_loss_type must be one of"),
])
def test_resume_blames_the_option_it_always_blamed(tmp_path, expected, blamed):
    p, _ = _file(tmp_path, {})
    called = []
    with pytest.raises(ValueError, match=blamed):
        checkpoint.resume_training(p, lambda s: called.append(1), **expected)
    assert called == []


LIN = {k: torch.zeros(()).expand(s) for k, s in spec.box_head_shapes(linear_fusion=True).items()}
STD = {k: torch.zeros(()).expand(s) for k, s in spec.box_head_shapes().items()}


@pytest.mark.parametrize("who, options, blamed", [
    ("train", dict(neg_support=True, loc_loss_type="l1"), r"^neg_support=True \(FEW_SHOT.NEG_SUPPORT\) needs the second stage: build the TrainEngine"),
    ("train", dict(second_stage=True, neg_support=True, linear_fusion=True, box_cls_loss="hinge"),
     r"^neg_support=True \(FEW_SHOT.NEG_SUPPORT\) does not exist with linear_fusion=True .*build the TrainEngine"),
    ("train", dict(second_stage=True, neg_support=True, box_cls_loss="focal_loss", loc_loss_type="l1"),
     r"^FEW_SHOT.NEG_SUPPORT is supported with box_cls_loss='ce_loss' only, not 'focal_loss'"),
    ("train", dict(loc_loss_type="l1", soft_labeling_func="cubic"), r"^loc_loss_type must be one of"),
    ("train", dict(loc_loss_type="l1", box_cls_loss="l1_loss"), r"^loc_loss_type must be one of"),
    ("train", dict(soft_labeling_func="cubic", box_cls_loss="hinge"), r"^soft_labeling_func must be one of"),
    ("hot", dict(neg_support=True, linear_fusion=True, soft_labeling_func="cubic"),
     r"^neg_support=True \(FEW_SHOT.NEG_SUPPORT\) does not exist with linear_fusion=True .*build the HotPathEngine"),
    ("hot", dict(soft_labeling_func="cubic", box_cls_loss="hinge"), r"^soft_labeling_func must be one of"),
    ("detector", dict(soft_labeling_func="cubic", box_cls_loss="l1_loss"), r"^soft_labeling_func must be one of"),
    # the box head looks at the state_dict's layout after neg_support and before box_cls_loss, at its cls_score last
    ("box_lin", dict(box_cls_loss="hinge"), r"trained with FEW_SHOT.LINEAR_FUSION True; build the engine with linear_fusion=True"),
    ("box_lin", dict(neg_support=True, box_cls_loss="focal_loss"), r"^FEW_SHOT.NEG_SUPPORT is supported with box_cls_loss='ce_loss' only"),
    ("box_std", dict(linear_fusion=True, box_cls_loss="l1_loss"), r"trained with FEW_SHOT.LINEAR_FUSION False; build the engine with linear_fusion=False"),
    ("box_std", dict(box_cls_loss="focal_loss"), r"cls_score.weight has 2 row\(s\) but box_cls_loss='focal_loss'"),
])
def test_constructors_blame_the_option_they_always_blamed(who, options, blamed):
    """Nothing here reaches a GPU: every call is refused by spec.check_options, which the constructors run first."""
    build = {"train": lambda: train.TrainEngine({}, **options), "hot": lambda: model.HotPathEngine({}, **options),
             "detector": lambda: modules.OneShotDetector({}, **options), "box_lin": lambda: BoxHeadWeights(LIN, torch.float32, **options),
             "box_std": lambda: BoxHeadWeights(STD, torch.float32, **options)}[who]
    with pytest.raises(ValueError, match=blamed):
        build()
    # the same answer from the one function, called the way that constructor calls it
    options = dict(options)
    second_stage = options.pop("second_stage", False) if who == "train" else True
    sd = {"box_lin": LIN, "box_std": STD}.get(who)
    with pytest.raises(ValueError, match=blamed):
        spec.check_options({"train": "the TrainEngine", "hot": "the HotPathEngine", "detector": "the HotPathEngine"}.get(who, "the box head"),
                           second_stage, box_sd=sd, **options)
