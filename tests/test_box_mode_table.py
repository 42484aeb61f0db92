"""CPU: the second stage's classification-loss modes (FEW_SHOT.SECOND_STAGE_CLS_LOSS) and soft-label functions, held against every
place that numbers or describes them — the `#define`s of the two headers, the constants of the binding, the index order of the spec's
tuples and the spec's table — and a truth table of what the code answers about each mode, written out here and not derived."""
import os
import re

import pytest

from oneshotdet_amd import _lib, box_head, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> the suffix of its OSD_BOX_CLS_* / OSD_SOFT_LABEL_* define and of its _lib.BOX_CLS_* / _lib.SOFT_LABEL_* constant
CLS_DEFINE = {"ce_loss": "CE", "focal_loss": "FOCAL", "mse_loss": "MSE", "l1_loss": "L1", "cxe_loss": "CXE"}
FUNC_DEFINE = {"discrete": "DISCRETE", "linear": "LINEAR", "transLinear": "TRANS_LINEAR", "trans4thLinear": "TRANS_4TH_LINEAR"}

# mode: (C code, logits L, decodes as, exists only with soft labelling, reads soft labels when soft labelling is on)
TRUTH = {
    "ce_loss": (0, 2, "ce_loss", False, False),
    "focal_loss": (1, 1, "focal_loss", False, False),
    "mse_loss": (2, 1, "mse_loss", False, True),
    "l1_loss": (3, 1, "mse_loss", True, True),
    "cxe_loss": (4, 2, "ce_loss", True, True),
}


def defines(prefix):
    """{suffix: value} of every `#define <prefix><suffix> <int>` in the box-mode and soft-label headers"""
    out = {}
    for header in ("oneshotdet_hip_box_modes.h", "oneshotdet_hip_soft_labels.h"):
        src = open(os.path.join(ROOT, "include", header)).read()
        for name, value in re.findall(r"^#define %s([A-Z0-9_]+)\s+(-?\d+)\b" % prefix, src, flags=re.M):
            assert name not in out, name
            out[name] = int(value)
    return out


def test_headers_binding_and_spec_tuples_number_the_modes_alike():
    cls, funcs = defines("OSD_BOX_CLS_"), defines("OSD_SOFT_LABEL_")
    assert sorted(cls) == sorted(CLS_DEFINE.values()) and sorted(funcs) == sorted(FUNC_DEFINE.values())
    for mode, suffix in CLS_DEFINE.items():
        assert cls[suffix] == getattr(_lib, "BOX_CLS_" + suffix) == TRUTH[mode][0], mode
    for func, suffix in FUNC_DEFINE.items():
        assert funcs[suffix] == getattr(_lib, "SOFT_LABEL_" + suffix) == spec.SOFT_LABELING_FUNCS.index(func), func
    # the soft-only modes continue the numbering of the three that always exist
    order = spec.BOX_CLS_LOSSES + spec.BOX_CLS_LOSSES_SOFT
    assert [cls[CLS_DEFINE[m]] for m in order] == list(range(5)) and len(spec.BOX_CLS_LOSSES) == 3
    assert [funcs[FUNC_DEFINE[f]] for f in spec.SOFT_LABELING_FUNCS] == list(range(4))


def test_the_spec_table_is_the_truth_table():
    cls = defines("OSD_BOX_CLS_")
    assert list(spec.BOX_CLS_MODES) == list(spec.BOX_CLS_LOSSES + spec.BOX_CLS_LOSSES_SOFT) == sorted(TRUTH, key=lambda m: TRUTH[m][0])
    for index, (mode, row) in enumerate(spec.BOX_CLS_MODES.items()):
        assert row.code == index == cls[CLS_DEFINE[mode]] == getattr(_lib, "BOX_CLS_" + CLS_DEFINE[mode]), mode
        assert (row.code, row.logits, row.decode, bool(row.soft_only), row.reads_soft) == TRUTH[mode], mode
        assert row.decode in spec.BOX_CLS_LOSSES           # a decode is one of the three the decode entries accept
    assert sorted(spec._BOX_CLS_REFUSED) == sorted(spec.BOX_CLS_LOSSES_SOFT)


@pytest.mark.parametrize("soft_labeling", [False, True])
@pytest.mark.parametrize("mode", sorted(TRUTH))
def test_what_the_code_answers_about_each_mode(mode, soft_labeling):
    code, logits, decode, soft_only, reads_soft = TRUTH[mode]
    if soft_only and not soft_labeling:      # 'l1_loss' / 'cxe_loss' exist with soft labelling only
        for ask in (spec.box_cls_loss_mode, spec.box_cls_logits, spec.box_cls_decode_mode):
            with pytest.raises(ValueError, match="SOFT_LABELING"):
                ask(mode, soft_labeling=soft_labeling)
    else:
        assert spec.box_cls_loss_mode(mode, soft_labeling=soft_labeling) == mode
        assert spec.box_cls_logits(mode, soft_labeling) == logits
        assert spec.box_cls_decode_mode(mode, soft_labeling) == decode
    assert spec.box_loss_reads_soft_labels(mode, soft_labeling) is (reads_soft and soft_labeling)
    # several shots: refused exactly in the one-logit modes, with or without soft labelling (the check is not told)
    box_head.check_shots(mode, 1)
    if logits == 1:
        with pytest.raises(ValueError, match="box_cls_loss=%r with 2 shots" % mode):
            box_head.check_shots(mode, 2)
    else:
        box_head.check_shots(mode, 2)
