"""Static description of the siamese-FCOS hot path: parameter names/shapes and the config values it consumes.

The names are the reference's own state_dict keys so a reference `.pth` loads unchanged
(reference: modeling/backbone/resnet.py:80-145,228-293,318-337; fpn.py:28-41,82-94; rpn/fcos/fcos.py:12-81;
config of record configs/fcos/2019_10_25_vanilla_siamse_backbone.yaml + config/defaults.py).
tests/test_spec.py checks this list against tests/golden/state_dict_keys.json, which was dumped from the real
reference model.
"""
import inspect
from collections import OrderedDict, namedtuple

# ---- config of record (only the values the hot path reads) ----
STEM_OUT = 64
RES2_OUT = 256
STAGE_BLOCKS = (3, 4, 6, 3)           # resnet.py:65-68 (R-50-FPN-RETINANET)
FPN_OUT = 256                         # BACKBONE_OUT_CHANNELS
FPN_STRIDES = (8, 16, 32, 64, 128)    # defaults.py FCOS.FPN_STRIDES
POOLER_SCALES = (0.125, 0.0625, 0.03125, 0.015625, 0.0078125)
POOLER_SAMPLING_RATIO = 2
NUM_CONVS = 4
GN_GROUPS = 32
GN_EPS = 1e-5
PRIOR_PROB = 0.01
PRE_NMS_TOP_N_TEST = 6000
PRE_NMS_TOP_N_TRAIN = 12000
POST_NMS_TOP_N_TEST = 2000
POST_NMS_TOP_N_TRAIN = 4000
NMS_THRESH = 0.8
FREEZE_CONV_BODY_AT = 2               # stem + layer1 frozen (resnet.py:127-136)
LOSS_ALPHA = 0.25
LOSS_GAMMA = 2.0
POS_RADIUS = 1.5
CENTER_SAMPLE = True                  # yaml FCOS.CENTER_SAMPLE (defaults.py:309 has False: positives inside the whole box, loss.py:176-177)
LOC_LOSS_TYPE = "giou"                # yaml FCOS.LOC_LOSS_TYPE (defaults.py:311 has 'iou'; iou_loss.py:36-41 also 'linear_iou')
LOC_LOSS_TYPES = ("giou", "iou", "linear_iou")       # index = OSD_LOC_LOSS_* of include/oneshotdet_hip.h
SIAMESE_BACKBONE = True               # yaml FEW_SHOT.SIAMESE_BACKBONE: the query has a backbone of its own (generalized_rcnn.py:69-71,274-275)
SUPP_ROIALIGN = True                  # yaml FEW_SHOT.SUPP_ROIALIGN: the query pyramid is pooled by a 1 x 1 ROIAlign (generalized_rcnn.py:87-94)
SIZE_DIVISIBILITY = 32
INF = 100000000
# second stage: yaml ROI_BOX_HEAD + defaults.py:196-229,511
BOX_POOL = 7                          # ROI_BOX_HEAD.POOLER_RESOLUTION
BOX_MLP_DIM = 1024                    # ROI_BOX_HEAD.MLP_HEAD_DIM
BOX_NUM_CLASSES = 2                   # ROI_BOX_HEAD.NUM_CLASSES (background, the query's class)
BOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)   # ROI_HEADS.BBOX_REG_WEIGHTS
BOX_SCORE_THRESH = 0.0                # ROI_HEADS.SCORE_THRESH
BOX_NMS_THRESH = 0.5                  # ROI_HEADS.NMS
BOX_DETECTIONS_PER_IMG = 2000         # ROI_HEADS.DETECTIONS_PER_IMG
BOX_LEAKY_SLOPE = 0.2                 # box_head.py:46,49,64
# second stage, training (defaults.py:190-203, box_head.py:193-194)
BOX_FG_IOU_THRESH = 0.5               # ROI_HEADS.FG_IOU_THRESHOLD == BG_IOU_THRESHOLD
BOX_BATCH_PER_IMAGE = 128             # ROI_HEADS.BATCH_SIZE_PER_IMAGE
BOX_POSITIVE_FRACTION = 0.25          # ROI_HEADS.POSITIVE_FRACTION
BOX_LOSS_WEIGHTS = (5.0, 2.5)         # loss_classifier *= 5; loss_box_reg *= 2.5
BOX_CLS_LOSS = "ce_loss"               # yaml / defaults.py:511 FEW_SHOT.SECOND_STAGE_CLS_LOSS
# The classification-loss modes (FEW_SHOT.SECOND_STAGE_CLS_LOSS), one row each, and everything the code asks about one:
#   code       OSD_BOX_CLS_* of include/oneshotdet_hip_box_modes.h (0..2) and include/oneshotdet_hip_soft_labels.h (3, 4)
#   logits     outputs of predictor.cls_score (roi_box_predictors.py:47-50,63-68,76-77): 2 = softmax, 1 = sigmoid
#   decode     the mode whose decode it uses (inference.py:61-69)
#   soft_only  None, or the box_head/loss.py lines of a loss that exists with FEW_SHOT.SOFT_LABELING only (loss.py:364-369)
#   reads_soft whether the loss reads the soft labels when SOFT_LABELING is on; 'ce_loss' and 'focal_loss' compute them in the
#              reference and never read them (loss.py:343-359)
BoxClsMode = namedtuple("BoxClsMode", "code logits decode soft_only reads_soft")
BOX_CLS_MODES = OrderedDict((
    ("ce_loss", BoxClsMode(0, 2, "ce_loss", None, False)),
    ("focal_loss", BoxClsMode(1, 1, "focal_loss", None, False)),
    ("mse_loss", BoxClsMode(2, 1, "mse_loss", None, True)),
    ("l1_loss", BoxClsMode(3, 1, "mse_loss", "364-365", True)),
    ("cxe_loss", BoxClsMode(4, 2, "ce_loss", "366-367", True)),
))
BOX_CLS_LOSSES = tuple(m for m, row in BOX_CLS_MODES.items() if not row.soft_only)       # ce, focal, mse: index = code
SOFT_LABELING = False                  # yaml / defaults.py FEW_SHOT.SOFT_LABELING: IoU soft labels carried through the sampler (box_head/loss.py:52-62)
SOFT_LABELING_FUNC = "linear"          # FEW_SHOT.SOFT_LABELING_FUNC (box_head/loss.py:81-104)
SOFT_LABELING_FUNCS = ("discrete", "linear", "transLinear", "trans4thLinear")     # index = OSD_SOFT_LABEL_* of include/oneshotdet_hip_soft_labels.h
BOX_CLS_LOSSES_SOFT = tuple(m for m, row in BOX_CLS_MODES.items() if row.soft_only)      # l1, cxe: only with SOFT_LABELING
LINEAR_FUSION = False                  # defaults.py FEW_SHOT.LINEAR_FUSION: one 3x3 conv over cat(x, query) in front of fc6 (box_head.py:43,61-72,148)
NEG_SUPPORT = False                    # defaults.py FEW_SHOT.NEG_SUPPORT.TURN_ON: the sampled ROIs are also scored against a support of another category (box_head.py:128-139)
BOX_SUPPRESS_MARGIN = 0.3              # box_head/loss.py:442: relu(q - p + 0.3).mean() over the foreground rows
BOX_SUPPRESS_WEIGHT = 2.5              # box_head.py:188: loss_cls_suppress = cls_suppress * 2.5
BOX_LOSS_ALPHA = 0.25                 # FEW_SHOT.SECOND_STAGE_LOSS_ALPHA (defaults.py:512); gamma is FCOS.LOSS_GAMMA (box_head/loss.py:40-44)
LEVEL_MAP_SCALE = 224                 # poolers.py:16 LevelMapper canonical_scale / canonical_level / eps
LEVEL_MAP_LEVEL = 4
LEVEL_MAP_EPS = 1e-6


def loss_mode(center_sample, loc_loss_type):
    """-> (bool, str) of the two FCOS loss options, ValueError for a regression loss iou_loss.py:34-43 does not have."""
    if loc_loss_type not in LOC_LOSS_TYPES:
        raise ValueError("loc_loss_type must be one of %s (FCOS.LOC_LOSS_TYPE), not %r" % (", ".join(LOC_LOSS_TYPES), loc_loss_type))
    return bool(center_sample), str(loc_loss_type)


_BOX_CLS_REFUSED = {m: "it needs FEW_SHOT.SOFT_LABELING (IoU soft labels carried through the sampler, box_head/loss.py:52-64,%s): "
                       "pass soft_labeling=True" % BOX_CLS_MODES[m].soft_only for m in BOX_CLS_LOSSES_SOFT}


def soft_labeling_mode(soft_labeling=False, soft_labeling_func="linear"):
    """-> (bool, str) of FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC; ValueError for a function box_head/loss.py:92-104 does not have."""
    if soft_labeling_func not in SOFT_LABELING_FUNCS:
        raise ValueError("soft_labeling_func must be one of %s (FEW_SHOT.SOFT_LABELING_FUNC), not %r"
                         % (", ".join(SOFT_LABELING_FUNCS), soft_labeling_func))
    return bool(soft_labeling), str(soft_labeling_func)


def box_loss_reads_soft_labels(box_cls_loss, soft_labeling=False):
    """Whether the loss launch reads the soft labels: 'mse_loss' / 'l1_loss' / 'cxe_loss' with SOFT_LABELING.  'ce_loss' and
    'focal_loss' compute soft labels in the reference and never read them (box_head/loss.py:343-359): nothing changes for them."""
    return bool(soft_labeling) and BOX_CLS_MODES[box_cls_loss_mode(box_cls_loss, soft_labeling=True)].reads_soft


def box_cls_decode_mode(box_cls_loss, soft_labeling=False):
    """The BOX_CLS_LOSSES name whose decode a mode uses (inference.py:61-69): 'cxe_loss' scores like 'ce_loss' (softmax of two logits),
    'l1_loss' like 'mse_loss' (sigmoid of one)."""
    return BOX_CLS_MODES[box_cls_loss_mode(box_cls_loss, soft_labeling=soft_labeling)].decode


def box_cls_loss_mode(box_cls_loss, loss_weighted=False, neg_support=False, method="concat", soft_labeling=False):
    """-> the validated FEW_SHOT.SECOND_STAGE_CLS_LOSS name; ValueError for a loss box_head/loss.py:343-369 does not have and, by
    name, for what it has that this build does not support: FEW_SHOT.LOSS_WEIGHTED (its reference path
    calls .cuda() unconditionally, loss.py:349-357: nothing to record it against), SECOND_STAGE_METHOD 'rn', and negative support
    (FEW_SHOT.NEG_SUPPORT) with any loss but 'ce_loss' (the margin loss of loss.py:435-444 compares softmax scores).
    'l1_loss' / 'cxe_loss' exist with soft_labeling=True (FEW_SHOT.SOFT_LABELING) only, as in the reference (loss.py:364-369)."""
    if loss_weighted:
        raise ValueError("FEW_SHOT.LOSS_WEIGHTED is not supported (box_head/loss.py:349-357)")
    if neg_support and box_cls_loss != "ce_loss":
        raise ValueError("FEW_SHOT.NEG_SUPPORT is supported with box_cls_loss='ce_loss' only, not %r: the second stage runs the "
                         "other losses without negative support" % (box_cls_loss,))
    if method != "concat":
        raise ValueError("FEW_SHOT.SECOND_STAGE_METHOD %r is not supported: only 'concat' (not 'rn' or 'matching')" % (method,))
    row = BOX_CLS_MODES.get(box_cls_loss)
    if row is None:
        raise ValueError("box_cls_loss must be one of %s (FEW_SHOT.SECOND_STAGE_CLS_LOSS), not %r"
                         % (", ".join(BOX_CLS_LOSSES), box_cls_loss))
    if row.soft_only and not soft_labeling:
        raise ValueError("box_cls_loss %r is not supported: %s" % (box_cls_loss, _BOX_CLS_REFUSED[box_cls_loss]))
    return str(box_cls_loss)


def check_neg_support(neg_support=False, second_stage=True, linear_fusion=False, box_cls_loss="ce_loss", soft_labeling=False,
                      shots=1, who="the engine"):
    """-> bool of FEW_SHOT.NEG_SUPPORT.TURN_ON; ValueError, by name, for the combinations that do not exist: without the second
    stage, with FEW_SHOT.LINEAR_FUSION (the reference has no compress_dim_conv to call there, box_head.py:136), with any loss but
    'ce_loss', and with more than one shot (box_head.py:129 expands the negative support without a view per image)."""
    if not neg_support:
        return False
    if not second_stage:
        raise ValueError("neg_support=True (FEW_SHOT.NEG_SUPPORT) needs the second stage: build %s with second_stage=True" % who)
    if linear_fusion:
        raise ValueError("neg_support=True (FEW_SHOT.NEG_SUPPORT) does not exist with linear_fusion=True (FEW_SHOT.LINEAR_FUSION; "
                         "box_head.py:136 calls compress_dim_conv): build %s with linear_fusion=False" % who)
    box_cls_loss_mode(box_cls_loss, neg_support=True, soft_labeling=soft_labeling)
    if int(shots) != 1:
        raise ValueError("neg_support=True (FEW_SHOT.NEG_SUPPORT) works with one shot only (box_head.py:129), not %d: pass one "
                         "query per image" % int(shots))
    return True


SUPP_AUG_METHODS = ("avg", "max")      # FEW_SHOT.SUPP_AUG_METHOD as supported; index = OSD_SUPP_AUG_* of include/oneshotdet_hip_supp_aug.h
SUPP_AUG_MAX_GROUP = 8                 # members of a group the merge kernel takes


def supp_aug_mode(supp_aug=1, supp_aug_method="avg", neg_support=False):
    """-> (int A, str method) of FEW_SHOT.SUPP_AUG / NUM_SUPP_AUG / SUPP_AUG_METHOD: A = NUM_SUPP_AUG + 1 consecutive query rows (a
    support crop and its augmentations) are merged into one map per FPN level in front of every pooling (generalized_rcnn.py:235-294);
    A = 1 is FEW_SHOT.SUPP_AUG False.  Like `shots` this is a keyword of the engines and not a row of MODEL_OPTIONS: the merge has no
    weights, and a checkpoint does not record it.  ValueError, by config name, for a group size outside 1 .. 8, a method the
    reference does not have, 'conv' (it adds a `supp_aug_conv.0.weight` parameter: not supported), and A > 1 with a negative support
    (the reference merges only the positive support for 'avg' / 'max', :285-288: that model does not exist)."""
    if isinstance(supp_aug, bool) or int(supp_aug) != supp_aug or not 1 <= int(supp_aug) <= SUPP_AUG_MAX_GROUP:
        raise ValueError("supp_aug must be an integer in 1 .. %d (FEW_SHOT.NUM_SUPP_AUG + 1 rows per query group; 1 = FEW_SHOT.SUPP_AUG "
                         "False), not %r" % (SUPP_AUG_MAX_GROUP, supp_aug))
    if supp_aug_method == "conv":
        raise ValueError("supp_aug_method 'conv' (FEW_SHOT.SUPP_AUG_METHOD) is not supported: it adds a supp_aug_conv.0.weight "
                         "parameter to the model (generalized_rcnn.py:75-80); only %s" % " and ".join(repr(m) for m in SUPP_AUG_METHODS))
    if supp_aug_method not in SUPP_AUG_METHODS:
        raise ValueError("supp_aug_method must be one of %s (FEW_SHOT.SUPP_AUG_METHOD), not %r" % (", ".join(SUPP_AUG_METHODS), supp_aug_method))
    if int(supp_aug) > 1 and neg_support:
        raise ValueError("supp_aug=%d (FEW_SHOT.SUPP_AUG) does not exist with neg_support=True (FEW_SHOT.NEG_SUPPORT): the reference "
                         "merges only the positive support's group (generalized_rcnn.py:285-288); pass supp_aug=1 or neg_support=False"
                         % int(supp_aug))
    return int(supp_aug), str(supp_aug_method)


def group_query_sizes(q_sizes, aug):
    """The members of a query group must have equal sizes (the reference asserts it, generalized_rcnn.py:236-250): one (h, w) per
    group of `aug` consecutive rows; ValueError naming the first group whose members differ."""
    if aug == 1:
        return [tuple(s) for s in q_sizes]
    q_sizes = [tuple(int(v) for v in s) for s in q_sizes]
    if len(q_sizes) % aug != 0:
        raise ValueError("%d query rows are no multiple of supp_aug = %d (FEW_SHOT.SUPP_AUG: every query is a group of %d consecutive "
                         "rows)" % (len(q_sizes), aug, aug))
    for g in range(len(q_sizes) // aug):
        members = q_sizes[g * aug:(g + 1) * aug]
        if any(m != members[0] for m in members):
            raise ValueError("query group %d (rows %d .. %d) has members of different sizes %s: the rows of a FEW_SHOT.SUPP_AUG group "
                             "must have one size (generalized_rcnn.py:236-250)" % (g, g * aug, (g + 1) * aug - 1, members))
    return q_sizes[::aug]


def box_cls_logits(box_cls_loss="ce_loss", soft_labeling=False):
    """Outputs of predictor.cls_score = logits at the head of a predictor row (roi_box_predictors.py:47-50,63-68,76-77): 2 for
    'ce_loss' and 'cxe_loss', 1 for the sigmoid losses ('focal_loss', 'mse_loss', 'l1_loss')."""
    return BOX_CLS_MODES[box_cls_loss_mode(box_cls_loss, soft_labeling=soft_labeling)].logits


def check_box_cls_score(sd, box_cls_loss, prefix="roi_heads.box.", who="the engine", soft_labeling=False):
    """The state_dict's cls_score must have the mode's row count: a 1-row cls_score read as 2 logits (or the reverse) shifts
    every box delta by a column and detects garbage without an error."""
    want = box_cls_logits(box_cls_loss, soft_labeling)
    for leaf in ("weight", "bias"):
        rows = int(sd[prefix + "predictor.cls_score." + leaf].shape[0])
        if rows != want:
            other = [m for m in BOX_CLS_LOSSES if BOX_CLS_MODES[m].logits == rows]
            raise ValueError("%spredictor.cls_score.%s has %d row(s) but box_cls_loss=%r has %d logit(s) per ROI%s"
                             % (prefix, leaf, rows, box_cls_loss, want,
                                ": build %s with box_cls_loss=%s" % (who, " or ".join(repr(m) for m in other)) if other else ""))
    rows = int(sd[prefix + "predictor.bbox_pred.weight"].shape[0])
    if rows != 4 * BOX_NUM_CLASSES:
        raise ValueError("%spredictor.bbox_pred.weight has %d rows, expected %d" % (prefix, rows, 4 * BOX_NUM_CLASSES))


def check_linear_fusion(sd, linear_fusion=False, prefix="roi_heads.box.", who="the engine"):
    """The state_dict must have been trained with this FEW_SHOT.LINEAR_FUSION: with it there is no compress_dim_conv and
    feature_aggreg.0 reads the 2 * FPN_OUT channels of cat(x, query); without it feature_aggreg.0 reads compress_dim_conv's FPN_OUT
    (box_head.py:43-72).  ValueError that names the option and the value to pass, before anything is packed: never a KeyError on an
    entry the model was not built with."""
    linear_fusion = bool(linear_fusion)
    w = sd.get(prefix + "feature_aggreg.0.weight")
    if w is None:
        raise ValueError("%sfeature_aggreg.0.weight is missing: %s needs the roi_heads.box.* entries" % (prefix, who))
    cin = int(w.shape[1])
    has_compress = (prefix + "compress_dim_conv.0.weight") in sd
    if cin == 2 * FPN_OUT and not has_compress:
        trained = True
    elif cin == FPN_OUT and has_compress:
        trained = False
    else:
        raise ValueError("%sfeature_aggreg.0.weight has %d input channels and compress_dim_conv.0.weight is %s: neither a "
                         "FEW_SHOT.LINEAR_FUSION True model (%d channels, no compress_dim_conv) nor a False one (%d, with it)"
                         % (prefix, cin, "present" if has_compress else "absent", 2 * FPN_OUT, FPN_OUT))
    if trained != linear_fusion:
        raise ValueError("%sfeature_aggreg.0.weight has %d input channels and compress_dim_conv.0.weight is %s: the model was "
                         "trained with FEW_SHOT.LINEAR_FUSION %s; build %s with linear_fusion=%r"
                         % (prefix, cin, "present" if has_compress else "absent", trained, who, trained))
    return linear_fusion


# The model's configuration options, one row each, in the order of the constructors' keywords.  A row's name is the keyword of the
# engines and of checkpoint.resume_training, the engine's attribute and the field of a training checkpoint.
#   config   the reference's config name
#   default  what an engine built without the keyword has, and what a file without the field was trained with
#   scope    "fcos_loss": the TrainEngine only (detection computes no loss); "second_stage": nothing to say about a first-stage-only run
#   group    rows of one group are validated, compared and reported together
#   words    how a value reads in a message next to name=value: {value: words}, a % format, or None
ModelOption = namedtuple("ModelOption", "config default scope group words")
MODEL_OPTIONS = OrderedDict((
    ("siamese_backbone", ModelOption("FEW_SHOT.SIAMESE_BACKBONE", SIAMESE_BACKBONE, "model", "siamese_backbone",
                                     {True: "the two-backbone model", False: "the shared-backbone model"})),
    ("supp_roialign", ModelOption("FEW_SHOT.SUPP_ROIALIGN", SUPP_ROIALIGN, "model", "supp_roialign",
                                  {True: "ROIAlign query pooling", False: "global-average query pooling"})),
    ("center_sample", ModelOption("FCOS.CENTER_SAMPLE", CENTER_SAMPLE, "fcos_loss", "fcos_loss",
                                  {True: "the centre-sampled", False: "the whole-box"})),
    ("loc_loss_type", ModelOption("FCOS.LOC_LOSS_TYPE", LOC_LOSS_TYPE, "fcos_loss", "fcos_loss", "%s FCOS loss")),
    ("box_cls_loss", ModelOption("FEW_SHOT.SECOND_STAGE_CLS_LOSS", BOX_CLS_LOSS, "second_stage", "box_cls_loss", None)),
    ("soft_labeling", ModelOption("FEW_SHOT.SOFT_LABELING", SOFT_LABELING, "second_stage", "soft_labels", None)),
    ("soft_labeling_func", ModelOption("FEW_SHOT.SOFT_LABELING_FUNC", SOFT_LABELING_FUNC, "second_stage", "soft_labels", None)),
    ("linear_fusion", ModelOption("FEW_SHOT.LINEAR_FUSION", LINEAR_FUSION, "second_stage", "linear_fusion", None)),
    ("neg_support", ModelOption("FEW_SHOT.NEG_SUPPORT.TURN_ON", NEG_SUPPORT, "second_stage", "neg_support", None)),
))
ModelOptions = namedtuple("ModelOptions", tuple(MODEL_OPTIONS))
OPTION_GROUPS = OrderedDict((g, tuple(n for n, row in MODEL_OPTIONS.items() if row.group == g))       # group -> its rows' names
                            for g in OrderedDict.fromkeys(row.group for row in MODEL_OPTIONS.values()))
# How a file's record of one group is held against a caller's expectation or a built engine (checkpoint.resume_training):
#   validate  (the file's record, *values) -> the values as their validator returns them, ValueError by name
#   differs   (the file's values, the other values) -> bool
#   absent    None, or (the file's state_dict, a DataParallel prefix stripped) -> the values of a file that does not record them
#   why       what resuming the file with other values would do
OptionRule = namedtuple("OptionRule", "validate differs absent why")
_PLAIN = OptionRule(lambda record, *values: values, lambda trained, other: trained != other, None, "continue another run")
OPTION_RULES = dict.fromkeys(OPTION_GROUPS, _PLAIN)
OPTION_RULES.update(
    siamese_backbone=_PLAIN._replace(absent=lambda sd: (any(k.startswith("supp_backbone.") for k in sd),),
                                     why="tie or untie the query backbone's weights"),
    fcos_loss=_PLAIN._replace(validate=lambda record, *values: loss_mode(*values)),
    # validated against the soft labels of the FILE: 'l1_loss' / 'cxe_loss' exist with them only
    box_cls_loss=_PLAIN._replace(validate=lambda record, loss: (box_cls_loss_mode(loss, soft_labeling=record["soft_labeling"]),)),
    # the function only matters where soft labels are on
    soft_labels=_PLAIN._replace(validate=lambda record, *values: soft_labeling_mode(*values),
                                differs=lambda trained, other: trained[0] != other[0] or (trained[0] and trained[1] != other[1])))


def options_in(keywords):
    """The options among a mapping of keywords (a constructor's locals()), by name."""
    return {name: keywords[name] for name in MODEL_OPTIONS if name in keywords}


def check_options(who, second_stage, box_sd=None, box_prefix="roi_heads.box.", **options):
    """-> ModelOptions: the validated values of the options given, the rows' defaults for the others.  ValueError by name, from the
    options' own validators in the constructors' order: neg_support, the FCOS loss, the soft labels, box_cls_loss.  box_sd: a
    state_dict that holds the box head; its layout is checked against linear_fusion before box_cls_loss is looked at and its
    cls_score against box_cls_loss after (BoxHeadWeights)."""
    o = ModelOptions(**dict(((name, row.default) for name, row in MODEL_OPTIONS.items()), **options))._asdict()    # another name: TypeError
    o["neg_support"] = check_neg_support(o["neg_support"], second_stage, o["linear_fusion"], o["box_cls_loss"], o["soft_labeling"], who=who)
    o["center_sample"], o["loc_loss_type"] = loss_mode(o["center_sample"], o["loc_loss_type"])
    o["soft_labeling"], o["soft_labeling_func"] = soft_labeling_mode(o["soft_labeling"], o["soft_labeling_func"])
    if box_sd is not None:
        check_linear_fusion(box_sd, o["linear_fusion"], box_prefix)
    o["box_cls_loss"] = box_cls_loss_mode(o["box_cls_loss"], soft_labeling=o["soft_labeling"])
    if box_sd is not None:
        check_box_cls_score(box_sd, o["box_cls_loss"], box_prefix, soft_labeling=o["soft_labeling"])     # a 1-row cls_score must never be read as two logits
    return ModelOptions(**{name: type(MODEL_OPTIONS[name].default)(v) for name, v in o.items()})


def group_values(group, record, said=None):
    """The validated values of one group's rows in `record` ({name: value}, every row); with `said` ({name: value or None}), what is
    said put over the record's."""
    names = OPTION_GROUPS[group]
    values = OPTION_RULES[group].validate(record, *(record[n] if said is None or said.get(n) is None else said[n] for n in names))
    return tuple(type(MODEL_OPTIONS[n].default)(v) for n, v in zip(names, values))


def describe_group(group, values, words=True):
    """'the whole-box iou FCOS loss (center_sample=False, loc_loss_type='iou')', 'neg_support=True'; words=False: the keywords only."""
    names = OPTION_GROUPS[group]
    keywords = ", ".join("%s=%r" % nv for nv in zip(names, values))
    said = [w[v] if isinstance(w, dict) else w % v for w, v in zip((MODEL_OPTIONS[n].words for n in names), values) if w]
    return "%s (%s)" % (" ".join(said), keywords) if words and said else keywords


def _bn(prefix, n, out):
    for k in ("weight", "bias", "running_mean", "running_var"):
        out[prefix + "." + k] = (n,)


def resnet_body_shapes(prefix):
    """ResNet-50 body keys (resnet.py:80-125, Bottleneck :228-293, BaseStem :318-330)."""
    out = OrderedDict()
    out[prefix + "stem.conv1.weight"] = (STEM_OUT, 3, 7, 7)
    _bn(prefix + "stem.bn1", STEM_OUT, out)
    cin = STEM_OUT
    for si, nblocks in enumerate(STAGE_BLOCKS):
        mid = 64 * (2 ** si)
        cout = RES2_OUT * (2 ** si)
        for b in range(nblocks):
            p = "%slayer%d.%d." % (prefix, si + 1, b)
            if b == 0:  # in_channels != out_channels -> downsample branch (resnet.py:243-251)
                out[p + "downsample.0.weight"] = (cout, cin, 1, 1)
                _bn(p + "downsample.1", cout, out)
            out[p + "conv1.weight"] = (mid, cin, 1, 1)
            _bn(p + "bn1", mid, out)
            out[p + "conv2.weight"] = (mid, mid, 3, 3)
            _bn(p + "bn2", mid, out)
            out[p + "conv3.weight"] = (cout, mid, 1, 1)
            _bn(p + "bn3", cout, out)
            cin = cout
    return out


def fpn_shapes(prefix):
    """FPN keys; C2 lateral is skipped (fpn.py:33, backbone.py:59)."""
    out = OrderedDict()
    for idx, cin in ((2, 512), (3, 1024), (4, 2048)):
        out["%sfpn_inner%d.weight" % (prefix, idx)] = (FPN_OUT, cin, 1, 1)
        out["%sfpn_inner%d.bias" % (prefix, idx)] = (FPN_OUT,)
        out["%sfpn_layer%d.weight" % (prefix, idx)] = (FPN_OUT, FPN_OUT, 3, 3)
        out["%sfpn_layer%d.bias" % (prefix, idx)] = (FPN_OUT,)
    for name in ("p6", "p7"):
        out["%stop_blocks.%s.weight" % (prefix, name)] = (FPN_OUT, FPN_OUT, 3, 3)
        out["%stop_blocks.%s.bias" % (prefix, name)] = (FPN_OUT,)
    return out


def backbone_shapes(prefix):
    out = resnet_body_shapes(prefix + "body.")
    out.update(fpn_shapes(prefix + "fpn."))
    return out


def fcos_head_shapes(prefix="rpn.head."):
    """FCOSHead keys (fcos.py:27-81): Sequential indices 0,3,6,9 = conv; 1,4,7,10 = GroupNorm."""
    out = OrderedDict()
    for tower in ("cls_tower", "bbox_tower"):
        for i in range(NUM_CONVS):
            out["%s%s.%d.weight" % (prefix, tower, 3 * i)] = (FPN_OUT, FPN_OUT, 3, 3)
            out["%s%s.%d.bias" % (prefix, tower, 3 * i)] = (FPN_OUT,)
            out["%s%s.%d.weight" % (prefix, tower, 3 * i + 1)] = (FPN_OUT,)
            out["%s%s.%d.bias" % (prefix, tower, 3 * i + 1)] = (FPN_OUT,)
    for name, c in (("cls_logits", 1), ("bbox_pred", 4), ("centerness", 1)):
        out["%s%s.weight" % (prefix, name)] = (c, FPN_OUT, 3, 3)
        out["%s%s.bias" % (prefix, name)] = (c,)
    for i in range(5):
        out["%sscales.%d.scale" % (prefix, i)] = (1,)
    return out


def box_head_shapes(prefix="roi_heads.box.", box_cls_loss="ce_loss", soft_labeling=False, linear_fusion=False):
    """Second-stage few-shot ROI box head keys (modeling/roi_heads/box_head/box_head.py:40-78: compress_dim_conv =
    Sequential(conv1x1, GN, LeakyReLU, conv1x1, GN, LeakyReLU) -> indices 0,1,3,4; feature_aggreg = Sequential(conv3x3,
    GN, LeakyReLU); fc6/fc7 make_fc; roi_box_predictors.py:37-99 FPNPredictor with 2 classes and 2x4 box deltas).
    box_cls_loss (FEW_SHOT.SECOND_STAGE_CLS_LOSS): cls_score has 2 outputs for 'ce_loss' and ONE for 'focal_loss' / 'mse_loss'
    (roi_box_predictors.py:47-50,66-68,76-77); bbox_pred keeps its 8.  soft_labeling (FEW_SHOT.SOFT_LABELING) admits 'l1_loss' (one
    output) and 'cxe_loss' (two) and changes no shape by itself.  linear_fusion (FEW_SHOT.LINEAR_FUSION, box_head.py:43,61-72): no
    compress_dim_conv, and feature_aggreg.0 reads cat(x, query) = 2 * FPN_OUT channels."""
    out = OrderedDict()
    n_logits = box_cls_logits(box_cls_loss, soft_labeling)
    c2 = 2 * FPN_OUT
    if not linear_fusion:
        out[prefix + "compress_dim_conv.0.weight"] = (c2, c2, 1, 1)
        out[prefix + "compress_dim_conv.0.bias"] = (c2,)
        out[prefix + "compress_dim_conv.1.weight"] = (c2,)
        out[prefix + "compress_dim_conv.1.bias"] = (c2,)
        out[prefix + "compress_dim_conv.3.weight"] = (FPN_OUT, c2, 1, 1)
        out[prefix + "compress_dim_conv.3.bias"] = (FPN_OUT,)
        out[prefix + "compress_dim_conv.4.weight"] = (FPN_OUT,)
        out[prefix + "compress_dim_conv.4.bias"] = (FPN_OUT,)
    out[prefix + "feature_aggreg.0.weight"] = (FPN_OUT // 2, c2 if linear_fusion else FPN_OUT, 3, 3)
    out[prefix + "feature_aggreg.0.bias"] = (FPN_OUT // 2,)
    out[prefix + "feature_aggreg.1.weight"] = (FPN_OUT // 2,)
    out[prefix + "feature_aggreg.1.bias"] = (FPN_OUT // 2,)
    out[prefix + "fc6.weight"] = (BOX_MLP_DIM, (FPN_OUT // 2) * BOX_POOL ** 2)
    out[prefix + "fc6.bias"] = (BOX_MLP_DIM,)
    out[prefix + "fc7.weight"] = (BOX_MLP_DIM, BOX_MLP_DIM)
    out[prefix + "fc7.bias"] = (BOX_MLP_DIM,)
    out[prefix + "predictor.cls_score.weight"] = (n_logits, BOX_MLP_DIM)
    out[prefix + "predictor.cls_score.bias"] = (n_logits,)
    out[prefix + "predictor.bbox_pred.weight"] = (BOX_NUM_CLASSES * 4, BOX_MLP_DIM)
    out[prefix + "predictor.bbox_pred.bias"] = (BOX_NUM_CLASSES * 4,)
    return out


def hot_path_shapes(siamese_backbone=True):
    """All state_dict entries of the hot path: target backbone, query backbone (separate weights,
    generalized_rcnn.py:69-71), FCOS head.  siamese_backbone=False (FEW_SHOT.SIAMESE_BACKBONE False, the reference's
    default: the query goes through the target's `backbone`, generalized_rcnn.py:274-275): no `supp_backbone.*` entries."""
    out = backbone_shapes("backbone.")
    if siamese_backbone:
        out.update(backbone_shapes("supp_backbone."))
    out.update(fcos_head_shapes())
    return out


def full_model_shapes(siamese_backbone=True, box_cls_loss="ce_loss", soft_labeling=False, linear_fusion=False):
    """Hot path + second-stage box head = every state_dict entry of the reference model under the config of record
    (siamese_backbone: see hot_path_shapes; box_cls_loss, linear_fusion: see box_head_shapes)."""
    out = hot_path_shapes(siamese_backbone)
    out.update(box_head_shapes(box_cls_loss=box_cls_loss, soft_labeling=soft_labeling, linear_fusion=linear_fusion))
    return out


# the options that decide a key or a shape: the keywords of full_model_shapes and of the loaders (checkpoint.py)
SHAPE_OPTIONS = tuple(inspect.signature(full_model_shapes).parameters)


def is_query_backbone_key(key):
    """An entry of the query branch's own backbone (two-backbone model only)."""
    return key.startswith("supp_backbone.") or key.startswith("module.supp_backbone.")


def is_frozen(key):
    """Parameters with requires_grad=False: FrozenBN buffers, stem and layer1 (resnet.py:127-136)."""
    if ".bn" in key or "downsample.1." in key:
        return True
    return ".body.stem." in key or ".body.layer1." in key


def level_sizes(h, w):
    """Spatial sizes of P3..P7 for an (h, w) input that is a multiple of 32: stride-2 convs with pad 1 / k 3
    (P6, P7) give ceil(n/2) (fpn.py:95-99), the body gives exact halvings."""
    assert h % 32 == 0 and w % 32 == 0
    p5 = (h // 32, w // 32)
    p6 = ((p5[0] + 1) // 2, (p5[1] + 1) // 2)
    p7 = ((p6[0] + 1) // 2, (p6[1] + 1) // 2)
    return [(h // 8, w // 8), (h // 16, w // 16), p5, p6, p7]
