"""CPU: the query gallery (supports enrolled once, images detected against the bank) as far as it goes without a device — the two entries' argument checks (they
return before any device call; the boundary's header, table and exports are tests/test_abi.py's), model.check_class_ids and QueryBank.slots_of (every refusal with its message), and the new keywords of
the engine."""
import ctypes
import inspect
import os
import types

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


def test_correlate_gallery_argument_checks_need_no_device(lib):
    f = lib.osd_correlate_levels_gallery
    xs, qs, ys, hws = _arrays()
    sl = ctypes.c_void_p(0x40000)
    bad = [
        (2, None, qs, sl, ys, hws, 2, 3, 5, 64, 0, None),                  # null arrays
        (2, xs, None, sl, ys, hws, 2, 3, 5, 64, 0, None),
        (2, xs, qs, None, ys, hws, 2, 3, 5, 64, 0, None),                  # no slot table
        (2, xs, qs, sl, None, hws, 2, 3, 5, 64, 0, None),
        (2, xs, qs, sl, ys, None, 2, 3, 5, 64, 0, None),
        (2, _arrays(null_at=1)[0], qs, sl, ys, hws, 2, 3, 5, 64, 0, None),   # a null tensor at a level
        (2, xs, _arrays(null_at=0)[1], sl, ys, hws, 2, 3, 5, 64, 0, None),
        (2, xs, qs, sl, _arrays(null_at=1)[2], hws, 2, 3, 5, 64, 0, None),
        (2, xs, qs, sl, ys, hws, 2, 0, 5, 64, 0, None),                    # classes < 1
        (2, xs, qs, sl, ys, hws, 2, -4, 5, 64, 0, None),
        (2, xs, qs, sl, ys, hws, 2, 3, 0, 64, 0, None),                    # n_gallery < 1
        (2, xs, qs, sl, ys, hws, 2, 3, -1, 64, 0, None),
        (0, xs, qs, sl, ys, hws, 2, 3, 5, 64, 0, None),                    # levels
        (7, xs, qs, sl, ys, hws, 2, 3, 5, 64, 0, None),
        (2, xs, qs, sl, ys, hws, -1, 3, 5, 64, 0, None),                   # n < 0
        (2, xs, qs, sl, ys, hws, 2, 3, 5, 60, 1, None),                    # channels: no multiple of a bf16 chunk
        (2, xs, qs, sl, ys, hws, 2, 3, 5, 4096, 0, None),                  # more than the staged group holds
        (2, xs, qs, sl, ys, hws, 2, 3, 5, 64, 7, None),                    # dtype
    ]
    for args in bad:
        assert f(*args) == -1, args
        assert lib.osd_last_error_string()
    assert f(2, xs, qs, sl, ys, hws, 0, 3, 5, 64, 0, None) == 0            # an empty batch is a no-op
    assert f(2, xs, qs, sl, ys, hws, 0, 1, 1, 256, 1, None) == 0
    assert f(2, xs, qs, sl, ys, (ctypes.c_int32 * 2)(0, 0), 2, 3, 5, 64, 0, None) == 0     # nothing but empty levels


def test_groupnorm_gallery_argument_checks_need_no_device(lib):
    f = lib.osd_groupnorm_act_rois_gallery
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(6)]      # x, addend, add_index, gamma, beta, y

    def call(null=None, n=15, hw=49, c=128, groups=32, per=5, stride=2, offset=1, n_add=8, dtype=0):
        p = [None if i == null else v for i, v in enumerate(P)]
        return f(p[0], p[1], p[2], p[3], p[4], p[5], n, hw, c, groups, 1e-5, 0.2, per, stride, offset, n_add, dtype, None)
    for kw in [dict(null=i) for i in range(6)] + [dict(n=-1), dict(per=0), dict(stride=0), dict(offset=-1), dict(n_add=0), dict(n_add=-3),
                                                  dict(dtype=5)]:
        assert call(**kw) == -1, kw
        assert lib.osd_last_error_string()
    # the shape rule is osd_groupnorm_act_rois': -2, as that entry answers
    g = lib.osd_groupnorm_act_rois
    for kw in (dict(hw=48), dict(c=64), dict(c=1024), dict(groups=0), dict(groups=24)):
        assert call(**kw) == -2, kw
        a = dict(hw=49, c=128, groups=32)
        a.update(kw)
        assert g(P[0], P[1], P[3], P[4], P[5], 15, a["hw"], a["c"], a["groups"], 1e-5, 0.2, 5, 2, 1, 0, None) == -2, kw
    assert call(n=0) == 0                                            # no samples: a no-op
    assert call(n=0, dtype=1, c=512) == 0


# ------------------------------------------------------------------------------------------------------- the host checks
def _fake(dtype=torch.float32, box_cls_loss="ce_loss", token=1):
    return types.SimpleNamespace(dtype=dtype, box_cls_loss=box_cls_loss, pack_token=token)


def _bank(engine, slots=4, shots=1, labels=None, dtype=None, token=None):
    from oneshotdet_amd import model
    return model.QueryBank(engine, engine.pack_token if token is None else token, None, None, None, shots, slots, labels,
                           engine.dtype if dtype is None else dtype)


def test_check_class_ids_accepts_and_flattens():
    from oneshotdet_amd import model
    eng = _fake()
    bank = _bank(eng)
    assert model.check_class_ids(eng, bank, 2, None) == (4, (0, 1, 2, 3, 0, 1, 2, 3))          # None: every slot in order, K = G
    assert model.check_class_ids(eng, bank, 2, [[2, 0, 3], [1, 1, 0]]) == (3, (2, 0, 3, 1, 1, 0))   # repeats allowed
    assert model.check_class_ids(eng, bank, 1, [(3,)]) == (1, (3,))
    assert model.check_class_ids(eng, bank, 2, torch.tensor([[3, 2], [0, 0]])) == (2, (3, 2, 0, 0))
    assert model.check_class_ids(eng, _bank(eng, shots=5), 1, [[0, 1]], second_stage=True) == (2, (0, 1))   # 'ce_loss' takes shots


def test_check_class_ids_refuses_by_name():
    from oneshotdet_amd import model
    eng = _fake()
    bank = _bank(eng)
    with pytest.raises(ValueError, match=r"ragged class_ids.*\[2, 3\]"):
        model.check_class_ids(eng, bank, 2, [[0, 1, 2], [0, 1]])
    with pytest.raises(ValueError, match=r"class_ids has 3 rows for 2 images"):
        model.check_class_ids(eng, bank, 2, [[0], [1], [2]])
    with pytest.raises(ValueError, match=r"class_ids has 1 rows for 2 images"):
        model.check_class_ids(eng, bank, 2, [[0, 1]])
    with pytest.raises(ValueError, match=r"class_ids\[1\] holds slot -1: not in \[0, 4\)"):
        model.check_class_ids(eng, bank, 2, [[0, 1], [2, -1]])
    with pytest.raises(ValueError, match=r"class_ids\[0\] holds slot 4: not in \[0, 4\)"):
        model.check_class_ids(eng, bank, 2, [[4, 1], [2, 3]])
    with pytest.raises(ValueError, match=r"slot 1\.5"):
        model.check_class_ids(eng, bank, 1, [[1.5]])
    with pytest.raises(ValueError, match=r"nested"):
        model.check_class_ids(eng, bank, 2, [0, 1])
    with pytest.raises(ValueError, match=r"empty"):
        model.check_class_ids(eng, bank, 2, [[], []])
    with pytest.raises(ValueError, match=r"stale QueryBank.*repack\(\)"):
        model.check_class_ids(eng, _bank(eng, token=0), 2, None)           # enrolled with the weights packed before
    with pytest.raises(ValueError, match=r"another engine"):
        model.check_class_ids(_fake(), bank, 2, None)
    with pytest.raises(ValueError, match=r"torch\.bfloat16.*torch\.float32"):
        model.check_class_ids(eng, _bank(eng, dtype=torch.bfloat16), 2, None)
    with pytest.raises(ValueError, match=r"must be a QueryBank"):
        model.check_class_ids(eng, object(), 2, None)
    focal = _fake(box_cls_loss="focal_loss")
    with pytest.raises(ValueError, match=r"focal_loss.*2 shots.*box_head\.py:246-253"):
        model.check_class_ids(focal, _bank(focal, shots=2), 2, None, second_stage=True)
    assert model.check_class_ids(focal, _bank(focal, shots=2), 2, None)[0] == 4       # the first stage alone takes any shots
    assert model.check_class_ids(focal, _bank(focal, shots=1), 2, None, second_stage=True)[0] == 4


def test_labels_map_to_slots_by_position():
    eng = _fake()
    bank = _bank(eng, labels=[17, 3, 44, 9])
    assert bank.slots_of(None, 2) is None                                   # None: all labels
    assert bank.slots_of([[44, 17], [9, 9]], 2) == [[2, 0], [3, 3]]
    with pytest.raises(ValueError, match=r"target_ids\[1\] names label 5, which is not among the bank's labels \[17, 3, 44, 9\]"):
        bank.slots_of([[44, 17], [5, 9]], 2)
    with pytest.raises(ValueError, match=r"one sequence of labels per image, for 2 images \(got 1"):
        bank.slots_of([[44, 17]], 2)
    with pytest.raises(ValueError, match=r"one sequence of labels per image"):
        bank.slots_of([44, 17], 2)
    with pytest.raises(ValueError, match=r"without labels"):
        _bank(eng).slots_of([[1]], 1)


def test_new_keywords_default_to_none_everywhere():
    from oneshotdet_amd import box_head, model, ops
    for name in ("forward_features", "forward", "detect", "tune", "box_detect"):
        p = inspect.signature(getattr(model.HotPathEngine, name)).parameters
        assert p["bank"].default is None and p["class_ids"].default is None, name
        assert p["classes"].default == 1, name
    for name in ("forward_features", "forward", "detect", "tune"):
        assert inspect.signature(getattr(model.HotPathEngine, name)).parameters["queries"].default is None, name
    assert list(inspect.signature(model.HotPathEngine.enroll).parameters) == ["self", "queries", "shots", "labels"]
    assert inspect.signature(model.HotPathEngine.enroll).parameters["shots"].default == 1
    p = inspect.signature(box_head.run_box_head).parameters
    assert p["bank"].default is None and p["slots"].default is None
    p = inspect.signature(model.run_correlate).parameters
    assert p["bank"].default is None and p["slots"].default is None and p["classes"].default == 1
    assert inspect.signature(ops.groupnorm_act_rois).parameters["add_index"].default is None
    assert list(inspect.signature(ops.correlate_levels_gallery).parameters) == ["xs", "qs", "slots", "classes"]
    assert inspect.signature(model.GraphedDetect.__call__).parameters["class_ids"].default is None


def test_slot_table_is_cached_by_content():
    from oneshotdet_amd import model
    a = model.slot_table_dev((2, 0, 3), "cpu")
    assert a.dtype == torch.int32 and a.tolist() == [2, 0, 3]
    assert model.slot_table_dev((2, 0, 3), "cpu") is a and model.slot_table_dev((2, 0, 1), "cpu") is not a


def test_documents_example_and_profile_name_the_gallery():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    assert "oneshotdet_hip.h" in read("README.md") and "enroll" in read("README.md")
    design = read("DESIGN.md")
    assert "### 4.5l" in design and design.index("### 4.5k") < design.index("### 4.5l") < design.index("## 5. Measurement")
    assert "osd_correlate_levels_gallery" in design and "osd_groupnorm_act_rois_gallery" in design
    assert "oneshotdet_hip.h" in read("INTEGRATION.md") and "enroll" in read("INTEGRATION.md")
    assert "--gallery" in read("examples", "detect.py")
    assert "bench_query_bank.py" in read("tools", "README.md") and os.path.exists(os.path.join(ROOT, "tools", "bench_query_bank.py"))
    assert "bank=" in read("profiles", "query_bank.md")
