"""Weight interchange with the reference's native checkpoints (`.pth` part).

Mirrors utils/checkpoint.py:33-103 (`{"model": state_dict, "optimizer": ..., "iteration": ...}` written by torch.save,
`last_checkpoint` tag file) and utils/model_serialization.py:10-80 (strip a DataParallel `module.` prefix, then give every
expected key the loaded key that is its LONGEST suffix), so a reference `model_XXXXXXX.pth` feeds
`HotPathEngine` / `TrainEngine` unchanged and `TrainEngine.state_dict()` goes back out in the reference's format.
The Caffe2 / Detectron `.pkl` route (utils/c2_model_loading.py:12-175; `MODEL.WEIGHT: catalog://ImageNetPretrained/MSRA/R-50`)
is `load_c2_resnet`: blob names are translated to the torchvision-style names the reference maps them to, and the same
suffix alignment then fills BOTH backbones (every `*.body.layer1.0.conv1.weight` ends with `layer1.0.conv1.weight`).
The model's options (spec.MODEL_OPTIONS): training checkpoints record every one, and `resume_training` refuses to continue a run
with another value.  The loaders take those that decide a key or a shape (spec.SHAPE_OPTIONS); the others (a pooling, a loss, soft
labels, a negative support) have no weights.  siamese_backbone: True = the two-backbone model (a shared-backbone file fills
`supp_backbone.*` from `backbone.*` by that suffix match, as the reference does); False = the shared-backbone model, whose key
set has no `supp_backbone.*` (a two-backbone file's query backbone is ignored, as the reference ignores keys its model does not
have).  box_cls_loss (with soft_labeling for 'l1_loss' / 'cxe_loss'): `roi_heads.box.predictor.cls_score.*` has 2 rows or 1; the
one-row modes share their shapes.  linear_fusion: no `roi_heads.box.compress_dim_conv.*` and a 512-channel `feature_aggreg.0.weight`;
a file trained with the other setting is refused by name (spec.check_linear_fusion) before any key is looked up.
"""
import os
import pickle
import re
from collections import OrderedDict

import torch

from . import spec


def strip_prefix_if_present(state_dict, prefix="module."):
    """model_serialization.py:58-66: only when EVERY key carries the prefix."""
    if not state_dict or not all(k.startswith(prefix) for k in state_dict):
        return state_dict
    return OrderedDict((k.replace(prefix, ""), v) for k, v in state_dict.items())


def align_state_dict(expected_shapes, loaded):
    """model_serialization.py:10-55: for each expected key pick the loaded key that is a suffix of it, longest first.
    Returns (aligned {expected key: tensor}, missing expected keys).  Shapes are checked (the reference would fail later,
    inside nn.Module.load_state_dict)."""
    loaded = strip_prefix_if_present(loaded)
    loaded_keys = sorted(loaded.keys())
    out, missing = OrderedDict(), []
    for key in expected_shapes:
        best = None
        for lk in loaded_keys:
            if key.endswith(lk) and (best is None or len(lk) > len(best)):
                best = lk
        if best is None:
            missing.append(key)
            continue
        t = torch.as_tensor(loaded[best])
        if tuple(t.shape) != tuple(expected_shapes[key]):
            raise ValueError("%s: checkpoint entry %s has shape %s, expected %s"
                             % (key, best, tuple(t.shape), tuple(expected_shapes[key])))
        out[key] = t.detach().to(torch.float32).cpu()
    return out, missing


def _read(path):
    data = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(data, dict):
        raise ValueError("%s: not a checkpoint dictionary" % path)
    if "model" not in data:                                            # checkpoint.py:164-165
        data = {"model": data}
    return data


def has_query_backbone(path_or_sd):
    """True iff a checkpoint file (or a state_dict) holds a query backbone of its own (`supp_backbone.*`): it was written by a
    two-backbone model (FEW_SHOT.SIAMESE_BACKBONE True).  Picks the mode to build a model in from a file."""
    sd = path_or_sd
    if isinstance(path_or_sd, (str, bytes, os.PathLike)):
        sd = _read(path_or_sd)["model"]
    return any(k.startswith("supp_backbone.") for k in strip_prefix_if_present(sd))


def _model_shapes(siamese_backbone, box_cls_loss, soft_labeling, linear_fusion):
    """Which shapes the model of these options (spec.SHAPE_OPTIONS) has -> (the hot path's, the box head's, for a source that has one)."""
    return spec.hot_path_shapes(siamese_backbone), spec.box_head_shapes(box_cls_loss=box_cls_loss, soft_labeling=soft_labeling,
                                                                         linear_fusion=linear_fusion)


def load_checkpoint(path, second_stage=None, defaults=None, siamese_backbone=True, box_cls_loss="ce_loss", soft_labeling=False,
                    linear_fusion=False):
    """Read a reference `.pth` (or a bare state_dict file) -> (state_dict under the reference's key names, extras).
    second_stage: True = require roi_heads.box.*, False = first stage only, None = take it when present.
    defaults: values for keys the file lacks (utils/checkpoint.py:107-115 keeps the model's own initialisation for
    FEW_SHOT.UNLOAD_KEYWORD modules); without it a missing key is an error.
    siamese_backbone, box_cls_loss, soft_labeling, linear_fusion (spec.SHAPE_OPTIONS): of the model that wrote the file, see above."""
    data = _read(path)
    loaded = data.pop("model")
    shapes, box = _model_shapes(siamese_backbone, box_cls_loss, soft_labeling, linear_fusion)
    probe = strip_prefix_if_present(loaded)
    has_box = any(k.endswith("box.fc6.weight") for k in probe)
    if second_stage or (second_stage is None and has_box):
        _check_linear_fusion_file(probe, linear_fusion, path)
        shapes.update(box)
    sd, missing = align_state_dict(shapes, loaded)
    for k in list(missing):
        if defaults is not None and k in defaults:
            sd[k] = torch.as_tensor(defaults[k]).to(torch.float32).cpu()
            missing.remove(k)
    if missing:
        raise KeyError("%s lacks %d expected entries, e.g. %s" % (path, len(missing), missing[:3]))
    return OrderedDict((k, sd[k]) for k in shapes), data


def _check_linear_fusion_file(loaded, linear_fusion, path):
    """spec.check_linear_fusion on a file's own (suffix-matched) key names; a file without any feature_aggreg.0 is left to the
    missing-entries error."""
    box = {}
    for leaf in ("feature_aggreg.0.weight", "compress_dim_conv.0.weight"):
        hit = [k for k in loaded if ("roi_heads.box." + leaf).endswith(k) or k.endswith("box." + leaf)]
        if hit:
            box["roi_heads.box." + leaf] = torch.as_tensor(loaded[max(hit, key=len)])
    if "roi_heads.box.feature_aggreg.0.weight" in box:
        spec.check_linear_fusion(box, linear_fusion, who="the loader (%s)" % path)


def save_checkpoint(path, state_dict, tag_last=True, **extras):
    """utils/checkpoint.py:33-50: {"model": state_dict, **extras} + the `last_checkpoint` tag file next to it."""
    data = {"model": OrderedDict((k, torch.as_tensor(v).detach().cpu()) for k, v in state_dict.items())}
    data.update(extras)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    torch.save(data, path)
    if tag_last:
        with open(os.path.join(d, "last_checkpoint"), "w") as f:       # checkpoint.py:95-98
            f.write(path)
    return path


def engine_options(engine):
    """{name: value} of spec.MODEL_OPTIONS as an engine (or a stand-in for one) carries them: an attribute it lacks means the row's
    default."""
    return OrderedDict((name, type(row.default)(getattr(engine, name, row.default))) for name, row in spec.MODEL_OPTIONS.items())


def save_training_checkpoint(path, engine, iteration, tag_last=True):
    """utils/checkpoint.py:33-50 as the trainer calls it (engine/trainer.py:111-119): model + optimizer + iteration.
    `optimizer` holds TrainEngine.optimizer_state_dict() (momentum buffers under reference names, steps taken, lr).  One more field
    per row of spec.MODEL_OPTIONS: the options the engine trained with, most of which leave no other trace in the file.  An engine
    with a learning-rate schedule also writes the reference's `scheduler` field (checkpoint.py:44-45): solver.LRSchedule.state_dict()
    under the reference scheduler's attribute names, last_epoch = the engine's update count."""
    extras = OrderedDict(optimizer=engine.optimizer_state_dict(), iteration=int(iteration))
    schedule = getattr(engine, "lr_schedule", None)
    if schedule is not None:
        extras["scheduler"] = schedule.state_dict(last_epoch=engine.iteration)
    extras.update(engine_options(engine))
    return save_checkpoint(path, engine.state_dict(), tag_last=tag_last, **extras)


def _file_options(data):
    """{name: value} of spec.MODEL_OPTIONS as a checkpoint's dictionary records them; for a field it lacks (a file written before
    the option existed) the row's default, or what the group's rule reads from the keys."""
    sd, out = strip_prefix_if_present(data["model"]), {}
    for name, row in spec.MODEL_OPTIONS.items():
        v, absent = data.get(name), spec.OPTION_RULES[row.group].absent
        if v is None:
            v = row.default if absent is None else absent(sd)[spec.OPTION_GROUPS[row.group].index(name)]
        out[name] = type(row.default)(v)
    return out


def _trained_with(path, group, values):
    return "%s was trained with %s [%s]" % (path, spec.describe_group(group, values),
                                            " / ".join(spec.MODEL_OPTIONS[n].config for n in spec.OPTION_GROUPS[group]))


def resume_training(path, make_engine, siamese_backbone=None, supp_roialign=None, center_sample=None, loc_loss_type=None,
                    box_cls_loss=None, soft_labeling=None, soft_labeling_func=None, linear_fusion=None, neg_support=None):
    """Load a checkpoint written by save_training_checkpoint: make_engine(state_dict) -> TrainEngine; its momentum and
    step count are restored.  Returns (engine, iteration).  A resumed run never changes an option behind the caller's back.  For
    every row of spec.MODEL_OPTIONS the file's value is its record (a file written before the option existed: the row's default),
    and the keyword is what the caller expects (None: whatever the file holds).  An expectation that differs from the file is
    refused before make_engine is called, an engine that make_engine built otherwise after it: ValueError naming the file, the
    option and both values.  The table's groups are looked at from the last to the first, each by its spec.OPTION_RULES.
    The learning-rate schedule is solver state, not a model option, and has no keyword: a file with a `scheduler` field and an engine
    with lr_schedule must agree in every field but last_epoch (ValueError naming the field and both values); a file with one and an
    engine without continue at the constant rate of the optimiser state; an engine with one continues it at the restored update count,
    whatever the file holds.  (The reference's loader has its scheduler restore commented out, utils/checkpoint.py:68-70, so a
    resumed reference run starts its warmup again; here the rate is a function of the restored count, on purpose.)"""
    expected = spec.options_in(locals())
    data = _read(path)
    record, trained = _file_options(data), OrderedDict()
    for group in reversed(spec.OPTION_GROUPS):
        trained[group], want = spec.group_values(group, record), spec.group_values(group, record, expected)
        if spec.OPTION_RULES[group].differs(trained[group], want):
            raise ValueError("%s; resuming it with %s would %s: build the engine with %s"
                             % (_trained_with(path, group, trained[group]), spec.describe_group(group, want),
                                spec.OPTION_RULES[group].why, spec.describe_group(group, trained[group], words=False)))
    sd, extras = load_checkpoint(path, **{name: record[name] for name in spec.SHAPE_OPTIONS})
    eng = make_engine(sd)
    built = engine_options(eng)
    for group, values in trained.items():
        got = tuple(built[name] for name in spec.OPTION_GROUPS[group])
        if spec.OPTION_RULES[group].differs(values, got):
            raise ValueError("%s but make_engine built an engine with %s" % (_trained_with(path, group, values), spec.describe_group(group, got)))
    schedule, recorded = getattr(eng, "lr_schedule", None), extras.get("scheduler")
    if schedule is not None and isinstance(recorded, dict):
        for field, mine, theirs in schedule.differences(recorded):
            raise ValueError("%s was trained with the learning-rate schedule's %s = %r but make_engine built an engine whose schedule "
                             "has %s = %r" % (path, field, theirs, field, mine))
    if "optimizer" in extras and isinstance(extras["optimizer"], dict) and "momentum_buffer" in extras["optimizer"]:
        eng.load_optimizer_state_dict(extras["optimizer"])
    return eng, int(extras.get("iteration", 0))


_C2_BRANCH = {"branch2a": ("conv1", "bn1"), "branch2b": ("conv2", "bn2"), "branch2c": ("conv3", "bn3"),
              "branch1": ("downsample.0", "downsample.1")}
_C2_BLOB = re.compile(r"^res(\d)_(\d+)_(branch2a|branch2b|branch2c|branch1)(_bn)?_(w|s|b)$")


def translate_c2_resnet_name(name):
    """One Caffe2 ResNet blob name -> the name the reference gives it (utils/c2_model_loading.py:12-60: `res2_0_branch2a_w`
    -> `layer1.0.conv1.weight`, `res_conv1_bn_s` -> `bn1.weight`, `res3_0_branch1_bn_b` -> `layer2.0.downsample.1.bias`,
    ...; AffineChannel scale / bias become the FrozenBN weight / bias).  None for blobs the loader skips (momentum)."""
    if name.endswith("_momentum"):
        return None
    if name == "conv1_w":
        return "conv1.weight"
    if name == "conv1_b":
        return "conv1.bias"
    if name in ("res_conv1_bn_s", "conv1_bn_s"):
        return "bn1.weight"
    if name in ("res_conv1_bn_b", "conv1_bn_b"):
        return "bn1.bias"
    if name in ("fc1000_w", "pred_w"):
        return "fc1000.weight"
    if name in ("fc1000_b", "pred_b"):
        return "fc1000.bias"
    m = _C2_BLOB.match(name)
    if m is None:
        return name.replace("_", ".")          # anything else keeps the reference's basic `_` -> `.` renaming
    stage, block, branch, bn, kind = int(m.group(1)), int(m.group(2)), m.group(3), m.group(4), m.group(5)
    conv, norm = _C2_BRANCH[branch]
    if bn:
        leaf = {"s": "weight", "b": "bias"}.get(kind)
        if leaf is None:
            return None
        return "layer%d.%d.%s.%s" % (stage - 1, block, norm, leaf)
    leaf = {"w": "weight", "b": "bias"}.get(kind)
    return None if leaf is None else "layer%d.%d.%s.%s" % (stage - 1, block, conv, leaf)


def load_c2_resnet(path, defaults, second_stage=None, siamese_backbone=True, box_cls_loss="ce_loss", soft_labeling=False,
                   linear_fusion=False):
    """A Detectron ResNet `.pkl` (dict of numpy blobs, optionally under "blobs"; pickled by Python 2: latin1) -> a full
    state_dict: the ResNet bodies of BOTH backbones come from the file, every other entry (FrozenBN running statistics —
    AffineChannel has none —, FPN, FCOS head, second stage) from `defaults`, as `DetectronCheckpointer.load` leaves the
    model's own initialisation for what the file lacks.  siamese_backbone=False: the shared-backbone model's keys only."""
    with open(path, "rb") as f:
        data = pickle.load(f, encoding="latin1")
    blobs = data["blobs"] if isinstance(data, dict) and "blobs" in data else data
    loaded = OrderedDict()
    for k in sorted(blobs.keys()):
        name = translate_c2_resnet_name(k)
        if name is not None:
            loaded[name] = torch.as_tensor(blobs[k])
    shapes, box = _model_shapes(siamese_backbone, box_cls_loss, soft_labeling, linear_fusion)
    if second_stage is not False and "roi_heads.box.feature_aggreg.0.weight" in defaults:
        spec.check_linear_fusion(defaults, linear_fusion, who="the loader (defaults)")
    if second_stage or (second_stage is None and all(k in defaults for k in box)):
        shapes.update(box)
    body = OrderedDict((k, v) for k, v in shapes.items() if ".body." in k and not k.endswith(("running_mean", "running_var")))
    sd, missing = align_state_dict(body, loaded)
    if missing:
        raise KeyError("%s lacks %d ResNet entries, e.g. %s" % (path, len(missing), missing[:3]))
    out = OrderedDict()
    for k in shapes:
        out[k] = sd[k] if k in sd else torch.as_tensor(defaults[k]).to(torch.float32).cpu()
    return out
