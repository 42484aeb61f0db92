"""CPU: what the second stage's C entries answer to a bad argument — the return code and the head of the message, which names the entry
(osd_box_loss_opt speaks as `box_loss`).  Every call here returns from an argument check (or from the n == 0 early return): nothing
is launched, with a GPU present or without.  Device pointers are a fake non-null address; `reg_weights` is real host memory, because
the host reads it.  Only single violations are pinned: the order in which two at once are reported is not part of the contract."""
import ctypes

import pytest

P = ctypes.c_void_p(0x1000)
OK, INVALID, UNSUPPORTED = 0, -1, -2
CE, FOCAL, MSE, L1, CXE = range(5)
F32 = 0


@pytest.fixture(scope="module")
def lib():
    from oneshotdet_amd import _lib, build
    build.build_library(verbose=False)
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    return _lib.load()


@pytest.fixture(scope="module")
def rw():
    return (ctypes.c_float * 4)(10.0, 10.0, 5.0, 5.0)


def answer(lib, rc, want_rc, prefix):
    assert rc == want_rc, (rc, lib.osd_last_error_string())
    if prefix is not None:
        msg = lib.osd_last_error_string().decode()
        assert msg.startswith(prefix), msg


def loss_args(pred=P, pred_stride=16, d_pred=None, grad_stride=0, dtype=F32):
    """n 2, 8 rows per image -> the arguments the three loss entries share (pred .. dtype)"""
    return (pred, P, P, P, 2, 8, pred_stride, 5.0, 2.5, P, d_pred, grad_stride, dtype)


LOSS_OPT = [
    ("null pred", dict(pred=None), FOCAL, "box_loss: null argument"),
    ("cls_loss 3", {}, 3, "box_loss: cls_loss"),
    ("cls_loss -1", {}, -1, "box_loss: cls_loss"),
    ("ce, pred_stride 9", dict(pred_stride=9), CE, "box_loss: 2 logits + 8"),
    ("focal, pred_stride 8", dict(pred_stride=8), FOCAL, "box_loss: 1 logits + 8"),
    ("focal, grad_stride 8 with d_pred", dict(pred_stride=9, d_pred=P, grad_stride=8), FOCAL, "box_loss: 1 logits + 8"),
    # without d_pred the narrow grad_stride is not checked: the dtype check is reached
    ("focal, grad_stride 8 without d_pred, dtype 2", dict(pred_stride=9, grad_stride=8, dtype=2), FOCAL, "box_loss: bad dtype"),
    ("dtype 2", dict(dtype=2), FOCAL, "box_loss: bad dtype"),
]


@pytest.mark.parametrize("case,kw,cls_loss,prefix", LOSS_OPT, ids=[c[0] for c in LOSS_OPT])
def test_box_loss_opt(lib, case, kw, cls_loss, prefix):
    answer(lib, lib.osd_box_loss_opt(*loss_args(**kw), cls_loss, 2.0, 0.25, None), INVALID, prefix)


LOSS = [
    ("null pred", dict(pred=None), "box_loss: null argument"),
    ("pred_stride 9", dict(pred_stride=9), "box_loss: 2 logits + 8"),
    ("grad_stride 8 with d_pred", dict(pred_stride=10, d_pred=P, grad_stride=8), "box_loss: 2 logits + 8"),
    ("grad_stride 8 without d_pred, dtype 2", dict(pred_stride=10, grad_stride=8, dtype=2), "box_loss: bad dtype"),
    ("dtype 2", dict(dtype=2), "box_loss: bad dtype"),
]


@pytest.mark.parametrize("case,kw,prefix", LOSS, ids=[c[0] for c in LOSS])
def test_box_loss(lib, case, kw, prefix):
    answer(lib, lib.osd_box_loss(*loss_args(**kw), None), INVALID, prefix)


LOSS_SOFT = [
    ("cls_loss 0", {}, P, CE, "box_loss_soft: cls_loss"),
    ("cls_loss 1", {}, P, FOCAL, "box_loss_soft: cls_loss"),
    ("cls_loss 5", {}, P, 5, "box_loss_soft: cls_loss"),
    ("null soft", {}, None, MSE, "box_loss_soft: null argument"),
    ("cxe, pred_stride 9", dict(pred_stride=9), P, CXE, "box_loss_soft: 2 logits + 8"),
    ("l1, pred_stride 8", dict(pred_stride=8), P, L1, "box_loss_soft: 1 logits + 8"),
    ("dtype 2", dict(dtype=2), P, MSE, "box_loss_soft: bad dtype"),
]


@pytest.mark.parametrize("case,kw,soft,cls_loss,prefix", LOSS_SOFT, ids=[c[0] for c in LOSS_SOFT])
def test_box_loss_soft(lib, case, kw, soft, cls_loss, prefix):
    answer(lib, lib.osd_box_loss_soft(*loss_args(**kw), soft, cls_loss, None), INVALID, prefix)


def sample_args(rw, boxes=P, n=2, p=16, g=2, s=8, reg_weights=True):
    """n 2, P 16, G 2, S 8 -> the arguments the two sampler entries share (boxes .. all_matched)"""
    return (boxes, P, P, P, None, P, n, p, g, s, 0.25, 0.5, rw if reg_weights else None, P, P, P, P, P, None, None)


SAMPLE = [
    ("null boxes", dict(boxes=None), INVALID, "box_match_sample: null argument"),
    ("null reg_weights", dict(reg_weights=False), INVALID, "box_match_sample: null argument"),
    ("n 0", dict(n=0), OK, None),
    ("P 0", dict(p=0), UNSUPPORTED, "box_match_sample: 1..8192 proposals"),
    ("P 8193", dict(p=8193), UNSUPPORTED, "box_match_sample: 1..8192 proposals"),
    ("G 0", dict(g=0), INVALID, "box_match_sample: bad sizes"),
    ("S 17", dict(s=17), INVALID, "box_match_sample: bad sizes"),
]


@pytest.mark.parametrize("case,kw,rc,prefix", SAMPLE, ids=[c[0] for c in SAMPLE])
def test_box_match_sample(lib, rw, case, kw, rc, prefix):
    answer(lib, lib.osd_box_match_sample(*sample_args(rw, **kw), None), rc, prefix)


SAMPLE_SOFT = [
    ("soft_func -1", {}, -1, P, INVALID, "box_match_sample_soft: soft_func"),
    ("soft_func 4", {}, 4, P, INVALID, "box_match_sample_soft: soft_func"),
    ("null s_soft", {}, 1, None, INVALID, "box_match_sample_soft: null argument"),
    ("n 0", dict(n=0), 1, P, OK, None),
    ("P 8193", dict(p=8193), 1, P, UNSUPPORTED, "box_match_sample_soft: 1..8192 proposals"),
]


@pytest.mark.parametrize("case,kw,func,s_soft,rc,prefix", SAMPLE_SOFT, ids=[c[0] for c in SAMPLE_SOFT])
def test_box_match_sample_soft(lib, rw, case, kw, func, s_soft, rc, prefix):
    answer(lib, lib.osd_box_match_sample_soft(*sample_args(rw, **kw), func, s_soft, None, None), rc, prefix)


def decode_args(rw, pred=P, n=2, shots=1, pred_stride=16, dtype=F32):
    """n 2, R 8, one shot -> the arguments of osd_box_decode_opt up to dtype"""
    return (pred, P, None, P, P, None, None, n, 8, shots, pred_stride, rw, 64.0, 64.0, None, 0.0, dtype)


DECODE = [
    ("cls_loss 3", {}, 3, INVALID, "box_decode: cls_loss"),
    ("null pred", dict(pred=None), FOCAL, INVALID, "box_decode: bad args"),
    ("shots 0", dict(shots=0), FOCAL, INVALID, "box_decode: bad args"),
    ("ce, stride 9", dict(pred_stride=9), CE, INVALID, "box_decode: bad args"),
    ("focal, stride 8", dict(pred_stride=8), FOCAL, INVALID, "box_decode: bad args"),
    ("focal, stride 9, n 0", dict(pred_stride=9, n=0), FOCAL, OK, None),
    ("dtype 2", dict(dtype=2), FOCAL, INVALID, "bad dtype 2"),
]


@pytest.mark.parametrize("case,kw,cls_loss,rc,prefix", DECODE, ids=[c[0] for c in DECODE])
def test_box_decode_opt(lib, rw, case, kw, cls_loss, rc, prefix):
    answer(lib, lib.osd_box_decode_opt(*decode_args(rw, **kw), cls_loss, None), rc, prefix)
