"""Weight interchange with the reference's native checkpoints (`.pth` part).

Mirrors utils/checkpoint.py:33-103 (`{"model": state_dict, "optimizer": ..., "iteration": ...}` written by torch.save,
`last_checkpoint` tag file) and utils/model_serialization.py:10-80 (strip a DataParallel `module.` prefix, then give every
expected key the loaded key that is its LONGEST suffix), so a reference `model_XXXXXXX.pth` feeds
`HotPathEngine` / `TrainEngine` unchanged and `TrainEngine.state_dict()` goes back out in the reference's format.
The Caffe2 / Detectron `.pkl` route (utils/c2_model_loading.py:12-175; `MODEL.WEIGHT: catalog://ImageNetPretrained/MSRA/R-50`)
is `load_c2_resnet`: blob names are translated to the torchvision-style names the reference maps them to, and the same
suffix alignment then fills BOTH backbones (every `*.body.layer1.0.conv1.weight` ends with `layer1.0.conv1.weight`).
siamese_backbone (FEW_SHOT.SIAMESE_BACKBONE): True = the two-backbone model (a shared-backbone file fills `supp_backbone.*` from
`backbone.*` by that suffix match, as the reference does); False = the shared-backbone model, whose key set has no
`supp_backbone.*` (a two-backbone file's query backbone is ignored, as the reference ignores keys its model does not have).
supp_roialign (FEW_SHOT.SUPP_ROIALIGN) changes no key: the query pooling has no weights, so loading is the same in both modes;
training checkpoints record it, and `resume_training` refuses to continue a run in the other mode.  The same holds for the loss
options center_sample / loc_loss_type (FCOS.CENTER_SAMPLE / FCOS.LOC_LOSS_TYPE): the loss has no parameters.
box_cls_loss (FEW_SHOT.SECOND_STAGE_CLS_LOSS) changes a SHAPE: `roi_heads.box.predictor.cls_score.*` has 2 rows for 'ce_loss' and
1 for 'focal_loss' / 'mse_loss'.  Loading checks the shapes of the mode it is given; the two one-row modes share their shapes, so
training checkpoints record the mode and `resume_training` refuses to continue a run on the other loss.
soft_labeling / soft_labeling_func (FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC) change no key and no shape by themselves ('l1_loss'
has 'mse_loss's shapes, 'cxe_loss' has 'ce_loss's): training checkpoints record both, a file without the fields was trained with
(False, "linear"), and `resume_training` refuses a mismatch.
linear_fusion (FEW_SHOT.LINEAR_FUSION) changes the KEY SET: with it there is no `roi_heads.box.compress_dim_conv.*` and
`feature_aggreg.0.weight` has 512 input channels.  Loading a file trained with the other setting raises a ValueError that names the
option (spec.check_linear_fusion) before any key is looked up; training checkpoints record it, a file without the field means False.
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


def load_checkpoint(path, second_stage=None, defaults=None, siamese_backbone=True, box_cls_loss="ce_loss", soft_labeling=False,
                    linear_fusion=False):
    """Read a reference `.pth` (or a bare state_dict file) -> (state_dict under the reference's key names, extras).
    second_stage: True = require roi_heads.box.*, False = first stage only, None = take it when present.
    defaults: values for keys the file lacks (utils/checkpoint.py:107-115 keeps the model's own initialisation for
    FEW_SHOT.UNLOAD_KEYWORD modules); without it a missing key is an error.
    siamese_backbone=False: read the shared-backbone model's keys only (any `supp_backbone.*` in the file is ignored).
    box_cls_loss: the second stage's classification loss the file was trained with (the shape of its cls_score); 'l1_loss' /
    'cxe_loss' with soft_labeling=True.  linear_fusion: FEW_SHOT.LINEAR_FUSION of the model that wrote the file."""
    data = _read(path)
    loaded = data.pop("model")
    shapes = spec.hot_path_shapes(siamese_backbone)
    box = spec.box_head_shapes(box_cls_loss=box_cls_loss, soft_labeling=soft_labeling, linear_fusion=linear_fusion)
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


def save_training_checkpoint(path, engine, iteration, tag_last=True):
    """utils/checkpoint.py:33-50 as the trainer calls it (engine/trainer.py:111-119): model + optimizer + iteration.
    `optimizer` holds TrainEngine.optimizer_state_dict() (momentum buffers under reference names, steps taken, lr);
    `siamese_backbone` the engine's mode (a shared engine writes no `supp_backbone.*`); `supp_roialign` its query pooling (the
    only record of it: the pooling has no weights); `center_sample` / `loc_loss_type` the FCOS loss it trained with (likewise);
    `box_cls_loss` the second stage's classification loss (the two one-logit losses have the same shapes); `soft_labeling` /
    `soft_labeling_func` the soft labels it was held against (no weights either); `linear_fusion` the box head's layout (the key set
    shows it too); `neg_support` whether it trained with a negative support (FEW_SHOT.NEG_SUPPORT: no weights, no keys)."""
    return save_checkpoint(path, engine.state_dict(), tag_last=tag_last, optimizer=engine.optimizer_state_dict(),
                           iteration=int(iteration), siamese_backbone=bool(getattr(engine, "siamese_backbone", True)),
                           supp_roialign=bool(getattr(engine, "supp_roialign", True)),
                           center_sample=bool(getattr(engine, "center_sample", spec.CENTER_SAMPLE)),
                           loc_loss_type=str(getattr(engine, "loc_loss_type", spec.LOC_LOSS_TYPE)),
                           box_cls_loss=str(getattr(engine, "box_cls_loss", spec.BOX_CLS_LOSS)),
                           soft_labeling=bool(getattr(engine, "soft_labeling", spec.SOFT_LABELING)),
                           soft_labeling_func=str(getattr(engine, "soft_labeling_func", spec.SOFT_LABELING_FUNC)),
                           linear_fusion=bool(getattr(engine, "linear_fusion", spec.LINEAR_FUSION)),
                           neg_support=bool(getattr(engine, "neg_support", spec.NEG_SUPPORT)))


def _loss_name(mode):
    return "the %s FCOS loss (center_sample=%r, loc_loss_type=%r)" % (
        ("centre-sampled " if mode[0] else "whole-box ") + mode[1], mode[0], mode[1])


def resume_training(path, make_engine, siamese_backbone=None, supp_roialign=None, center_sample=None, loc_loss_type=None,
                    box_cls_loss=None, soft_labeling=None, soft_labeling_func=None, linear_fusion=None, neg_support=None):
    """Load a checkpoint written by save_training_checkpoint: make_engine(state_dict) -> TrainEngine; its momentum and
    step count are restored.  Returns (engine, iteration).  The file's mode (recorded by save_training_checkpoint; for
    older files: whether it holds `supp_backbone.*`) must be the engine's: a resumed run never ties or unties weights
    behind the caller's back.  siamese_backbone: the mode the caller expects (None: whatever the file holds).  The same
    for the query pooling: supp_roialign is the caller's expectation, the file's record (True when it has none, the
    files written before the option existed) must match it and the engine's.  And for the FCOS loss: center_sample /
    loc_loss_type are the caller's expectations (None: whatever the file holds), a file without the fields was trained with
    (True, "giou"), the only loss there was.  And for the second stage's classification loss: box_cls_loss is the caller's
    expectation (None: whatever the file holds), a file without the field was trained with "ce_loss".  And for the soft labels:
    soft_labeling / soft_labeling_func are the caller's expectations (None: whatever the file holds), a file without the fields was
    trained with (False, "linear"); the function only matters where soft labels are on.  And for the box head's layout:
    linear_fusion is the caller's expectation (None: whatever the file holds), a file without the field was trained with False.
    And for the negative support: neg_support is the caller's expectation (None: whatever the file holds), a file without the field
    was trained with False."""
    data = _read(path)
    neg = data.get("neg_support")
    neg = spec.NEG_SUPPORT if neg is None else bool(neg)
    if neg_support is not None and bool(neg_support) != neg:
        raise ValueError("%s was trained with neg_support=%r (FEW_SHOT.NEG_SUPPORT); resuming it with neg_support=%r would continue "
                         "the run on another objective: build the engine with neg_support=%r" % (path, neg, bool(neg_support), neg))
    fusion = data.get("linear_fusion")
    fusion = spec.LINEAR_FUSION if fusion is None else bool(fusion)
    if linear_fusion is not None and bool(linear_fusion) != fusion:
        raise ValueError("%s was trained with linear_fusion=%r (FEW_SHOT.LINEAR_FUSION); resuming it with linear_fusion=%r would "
                         "continue another model: build the engine with linear_fusion=%r"
                         % (path, fusion, bool(linear_fusion), fusion))
    soft = (data.get("soft_labeling"), data.get("soft_labeling_func"))
    soft = spec.soft_labeling_mode(spec.SOFT_LABELING if soft[0] is None else bool(soft[0]),
                                   spec.SOFT_LABELING_FUNC if soft[1] is None else str(soft[1]))
    want_soft = spec.soft_labeling_mode(soft[0] if soft_labeling is None else soft_labeling,
                                        soft[1] if soft_labeling_func is None else soft_labeling_func)
    if want_soft[0] != soft[0] or (soft[0] and want_soft[1] != soft[1]):
        raise ValueError("%s was trained with soft_labeling=%r, soft_labeling_func=%r; resuming it with soft_labeling=%r, "
                         "soft_labeling_func=%r would continue the run on other labels: build the engine with soft_labeling=%r, "
                         "soft_labeling_func=%r" % (path, soft[0], soft[1], want_soft[0], want_soft[1], soft[0], soft[1]))
    box = data.get("box_cls_loss")
    box = spec.BOX_CLS_LOSS if box is None else spec.box_cls_loss_mode(str(box), soft_labeling=soft[0])
    if box_cls_loss is not None and spec.box_cls_loss_mode(box_cls_loss, soft_labeling=soft[0]) != box:
        raise ValueError("%s was trained with box_cls_loss=%r; resuming it with box_cls_loss=%r would continue the run on another "
                         "objective: build the engine with box_cls_loss=%r" % (path, box, box_cls_loss, box))
    loss = (data.get("center_sample"), data.get("loc_loss_type"))
    loss = (spec.CENTER_SAMPLE if loss[0] is None else bool(loss[0]), spec.LOC_LOSS_TYPE if loss[1] is None else str(loss[1]))
    want = spec.loss_mode(loss[0] if center_sample is None else center_sample, loss[1] if loc_loss_type is None else loc_loss_type)
    if want != loss:
        raise ValueError("%s was trained with %s; resuming it with %s would continue the run on another objective: build the "
                         "engine with center_sample=%r, loc_loss_type=%r" % (path, _loss_name(loss), _loss_name(want), loss[0], loss[1]))
    pool = data.get("supp_roialign")
    pool = True if pool is None else bool(pool)
    if supp_roialign is not None and bool(supp_roialign) != pool:
        raise ValueError("%s was trained with %s; resuming it with %s would continue another model: build the engine with "
                         "supp_roialign=%r" % (path, _POOL[pool], _POOL[bool(supp_roialign)], pool))
    mode = data.get("siamese_backbone")
    mode = has_query_backbone(data["model"]) if mode is None else bool(mode)
    if siamese_backbone is not None and bool(siamese_backbone) != mode:
        raise ValueError("%s holds a %s model; resuming it as a %s model would %s the query backbone's weights: load it with "
                         "load_checkpoint(..., siamese_backbone=%r) into a fresh run instead"
                         % (path, _MODE[mode], _MODE[bool(siamese_backbone)], "untie" if siamese_backbone else "tie",
                            bool(siamese_backbone)))
    sd, extras = load_checkpoint(path, siamese_backbone=mode, box_cls_loss=box, soft_labeling=soft[0], linear_fusion=fusion)
    eng = make_engine(sd)
    built_neg = bool(getattr(eng, "neg_support", spec.NEG_SUPPORT))
    if built_neg != neg:
        raise ValueError("%s was trained with neg_support=%r (FEW_SHOT.NEG_SUPPORT) but make_engine built an engine with "
                         "neg_support=%r" % (path, neg, built_neg))
    built_fusion = bool(getattr(eng, "linear_fusion", spec.LINEAR_FUSION))
    if built_fusion != fusion:
        raise ValueError("%s was trained with linear_fusion=%r (FEW_SHOT.LINEAR_FUSION) but make_engine built an engine with "
                         "linear_fusion=%r" % (path, fusion, built_fusion))
    built_soft = (bool(getattr(eng, "soft_labeling", spec.SOFT_LABELING)), str(getattr(eng, "soft_labeling_func", spec.SOFT_LABELING_FUNC)))
    if built_soft[0] != soft[0] or (soft[0] and built_soft[1] != soft[1]):
        raise ValueError("%s was trained with soft_labeling=%r, soft_labeling_func=%r but make_engine built an engine with "
                         "soft_labeling=%r, soft_labeling_func=%r" % (path, soft[0], soft[1], built_soft[0], built_soft[1]))
    built_box = str(getattr(eng, "box_cls_loss", spec.BOX_CLS_LOSS))
    if built_box != box:
        raise ValueError("%s was trained with box_cls_loss=%r but make_engine built an engine with box_cls_loss=%r"
                         % (path, box, built_box))
    if bool(getattr(eng, "siamese_backbone", True)) != mode:
        raise ValueError("%s holds a %s model but make_engine built a %s engine (siamese_backbone=%r)"
                         % (path, _MODE[mode], _MODE[not mode], not mode))
    if bool(getattr(eng, "supp_roialign", True)) != pool:
        raise ValueError("%s was trained with %s but make_engine built an engine with %s (supp_roialign=%r)"
                         % (path, _POOL[pool], _POOL[not pool], not pool))
    built = (bool(getattr(eng, "center_sample", spec.CENTER_SAMPLE)), str(getattr(eng, "loc_loss_type", spec.LOC_LOSS_TYPE)))
    if built != loss:
        raise ValueError("%s was trained with %s but make_engine built an engine with %s" % (path, _loss_name(loss), _loss_name(built)))
    if "optimizer" in extras and isinstance(extras["optimizer"], dict) and "momentum_buffer" in extras["optimizer"]:
        eng.load_optimizer_state_dict(extras["optimizer"])
    return eng, int(extras.get("iteration", 0))


_MODE = {True: "two-backbone (siamese_backbone=True)", False: "shared-backbone (siamese_backbone=False)"}
_POOL = {True: "ROIAlign query pooling (supp_roialign=True)", False: "global-average query pooling (supp_roialign=False)"}


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
    shapes = spec.hot_path_shapes(siamese_backbone)
    box = spec.box_head_shapes(box_cls_loss=box_cls_loss, soft_labeling=soft_labeling, linear_fusion=linear_fusion)
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
