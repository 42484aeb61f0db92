"""GPU (-m gpu): the second stage's `ops` wrappers (box_loss, box_match_sample, box_decode) marshal exactly what a direct call of the
C entry does — for every mode, the entry the wrapper must reach is called here by name on the same inputs and every output is
compared bit for bit (no tolerance: the same kernel on the same arguments).  The launch trace records the two soft entries and nothing
else.

Shapes, the smallest at which the marshalling can go wrong: 2 images; 16 proposals with counts (16, 11); 2 ground truths with counts
(2, 1); 8 sampled rows with counts (8, 5), so invalid rows exist; pred_stride = grad_stride = 16, wider than L + 8, so a wrong stride
shows; one shot."""
import ctypes

import pytest
import torch

from oneshotdet_amd import spec

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
N, P, G, S, STRIDE = 2, 16, 2, 8, 16
W_CLS, W_BOX = spec.BOX_LOSS_WEIGHTS
# (mode, soft labels given) -> the entry ops.box_loss must reach
LOSS_CASES = [
    ("ce_loss", False, "osd_box_loss"),
    ("focal_loss", False, "osd_box_loss_opt"),
    ("mse_loss", False, "osd_box_loss_opt"),
    ("mse_loss", True, "osd_box_loss_soft"),
    ("l1_loss", True, "osd_box_loss_soft"),
    ("cxe_loss", True, "osd_box_loss_soft"),
    ("ce_loss", True, "osd_box_loss"),              # never read soft labels: the launch they make without them
    ("focal_loss", True, "osd_box_loss_opt"),
]
# mode -> (soft_labeling, the entry ops.box_decode must reach, the code it passes)
DECODE_CASES = {
    "ce_loss": (False, "osd_box_decode", None),
    "focal_loss": (False, "osd_box_decode_opt", 1),
    "mse_loss": (False, "osd_box_decode_opt", 2),
    "l1_loss": (True, "osd_box_decode_opt", 2),     # decodes as 'mse_loss'
    "cxe_loss": (True, "osd_box_decode", None),     # decodes as 'ce_loss'
}
CODE = {"ce_loss": 0, "focal_loss": 1, "mse_loss": 2, "l1_loss": 3, "cxe_loss": 4}


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def traced(call):
    """-> (what `call` returned, the kinds of the launches it recorded)"""
    from oneshotdet_amd import trace
    trace.TRACE = []
    try:
        out = call()
        return out, [kind for kind, _ in trace.TRACE]
    finally:
        trace.TRACE = None


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    gt = torch.tensor([[[20.0, 30.0, 120.0, 150.0], [140.0, 40.0, 220.0, 110.0]], [[60.0, 50.0, 200.0, 180.0], [10.0, 10.0, 50.0, 40.0]]])
    # proposals 0..3: the image's first ground truth moved by a few pixels (IoU > 0.5), 4..5: its second one (image 1 counts one ground truth:
    # a background box), 6..15: boxes far from both (background; image 1 counts 11 of them)
    props = torch.tensor([300.0, 300.0, 340.0, 330.0]).repeat(N, P, 1) + 4 * torch.arange(P).float()[None, :, None]
    props[:, :4] = gt[:, :1]
    props[:, 4:6] = gt[:, 1:2]
    props += torch.rand((N, P, 4), generator=g) * 4 - 2
    return dict(
        props=props.cuda(), counts=torch.tensor([16, 11], dtype=torch.int32).cuda(), gt=gt.cuda(),
        gt_count=torch.tensor([2, 1], dtype=torch.int32).cuda(), keys=torch.rand((N, P), generator=g).cuda(),
        pred=(torch.randn((N * S, STRIDE), generator=g) * 2).cuda(), labels=torch.randint(0, 2, (N * S,), generator=g).int().cuda(),
        targets=torch.randn((N * S, 4), generator=g).cuda(), s_count=torch.tensor([8, 5], dtype=torch.int32).cuda(),
        soft=torch.rand((N * S,), generator=g).cuda(), rois=(torch.rand((N, S, 4), generator=g) * 100 + torch.tensor([0.0, 0.0, 120.0, 120.0])).cuda())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode,with_soft,entry", LOSS_CASES, ids=["%s%s" % (c[0], "+soft" if c[1] else "") for c in LOSS_CASES])
def test_box_loss_equals_the_direct_call(data, mode, with_soft, entry, dt):
    from oneshotdet_amd import _lib, ops
    pred = data["pred"].to(DT[dt])
    soft = data["soft"] if with_soft else None
    (losses, d), kinds = traced(lambda: ops.box_loss(pred, data["labels"], data["targets"], data["s_count"], N, S, W_CLS, W_BOX,
                                                     grad_stride=STRIDE, cls_loss=mode, soft=soft))
    assert kinds == (["box_loss_soft"] if entry == "osd_box_loss_soft" else [])
    want_l = torch.full((3,), 7.0, device="cuda")
    want_d = torch.full((N * S, STRIDE), 7.0, device="cuda", dtype=DT[dt])
    tail = {"osd_box_loss": (),
            "osd_box_loss_opt": (CODE[mode], spec.LOSS_GAMMA, spec.BOX_LOSS_ALPHA),
            "osd_box_loss_soft": (data["soft"].data_ptr(), CODE[mode])}[entry]
    _lib.call(entry, pred.data_ptr(), data["labels"].data_ptr(), data["targets"].data_ptr(), data["s_count"].data_ptr(), N, S, STRIDE,
              W_CLS, W_BOX, want_l.data_ptr(), want_d.data_ptr(), STRIDE, ops._dt(pred), *tail, stream())
    torch.cuda.synchronize()
    assert int(want_l[2]) == 13 and bool(torch.isfinite(want_l).all())          # 8 + 5 valid rows went in
    assert same(losses, want_l) and same(d, want_d)
    # without the gradient: no d_pred, the same losses
    l2, none = ops.box_loss(pred, data["labels"], data["targets"], data["s_count"], N, S, W_CLS, W_BOX, cls_loss=mode, soft=soft)
    assert none is None and same(l2, want_l)


@pytest.mark.parametrize("want_all", [False, True])
@pytest.mark.parametrize("soft_func", [None, "transLinear"])
def test_box_match_sample_equals_the_direct_call(data, soft_func, want_all):
    from oneshotdet_amd import _lib, ops
    got, kinds = traced(lambda: ops.box_match_sample(data["props"], data["counts"], data["gt"], data["gt_count"], data["keys"], S,
                                                     spec.BOX_POSITIVE_FRACTION, spec.BOX_FG_IOU_THRESH, spec.BOX_REG_WEIGHTS,
                                                     want_all=want_all, soft_func=soft_func))
    assert kinds == (["box_match_sample_soft"] if soft_func else [])
    assert len(got) == {(False, False): 5, (False, True): 7, (True, False): 6, (True, True): 9}[(soft_func is not None, want_all)]
    i32 = dict(device="cuda", dtype=torch.int32)
    sb, st = torch.full((N, S, 4), 7.0, device="cuda"), torch.full((N, S, 4), 7.0, device="cuda")
    sl, si, sc = torch.full((N, S), 7, **i32), torch.full((N, S), 7, **i32), torch.full((N,), 7, **i32)
    al, am = (torch.full((N, P), 7, **i32), torch.full((N, P), 7, **i32)) if want_all else (None, None)
    ss = torch.full((N, S), 7.0, device="cuda")
    as_ = torch.full((N, P), 7.0, device="cuda") if want_all else None
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    rw = (ctypes.c_float * 4)(*spec.BOX_REG_WEIGHTS)
    args = (data["props"].data_ptr(), data["counts"].data_ptr(), data["gt"].data_ptr(), data["gt_count"].data_ptr(), None,
            data["keys"].data_ptr(), N, P, G, S, spec.BOX_POSITIVE_FRACTION, spec.BOX_FG_IOU_THRESH, rw, sb.data_ptr(), sl.data_ptr(),
            st.data_ptr(), si.data_ptr(), sc.data_ptr(), ptr(al), ptr(am))
    if soft_func is None:
        _lib.call("osd_box_match_sample", *args, stream())
        want = (sb, sl, st, si, sc, al, am) if want_all else (sb, sl, st, si, sc)
    else:
        _lib.call("osd_box_match_sample_soft", *args, spec.SOFT_LABELING_FUNCS.index(soft_func), ss.data_ptr(), ptr(as_), stream())
        want = (sb, sl, st, si, sc, al, am, ss, as_) if want_all else (sb, sl, st, si, sc, ss)
    torch.cuda.synchronize()
    assert int(sc.min()) > 0 and int((sl > 0).sum()) > 0 and int((sl == 0).sum()) > 0      # positives and background rows are sampled
    for a, b in zip(got, want):
        assert same(a, b)


@pytest.mark.parametrize("mode", sorted(DECODE_CASES))
def test_box_decode_equals_the_direct_call(data, mode):
    from oneshotdet_amd import _lib, ops
    soft_labeling, entry, code = DECODE_CASES[mode]
    pred = data["pred"].reshape(1, N * S, STRIDE)
    got, kinds = traced(lambda: ops.box_decode(pred, data["rois"], data["s_count"], spec.BOX_REG_WEIGHTS, 240, 320, spec.BOX_SCORE_THRESH,
                                               want_raw=True, cls_loss=mode, soft_labeling=soft_labeling))
    assert kinds == []
    L = 2 if entry == "osd_box_decode" else 1
    want = [torch.full(shape, 7.0, device="cuda") for shape in ((N, S), (N, S, 4), (N * S, L), (N * S, 8))]
    rw = (ctypes.c_float * 4)(*spec.BOX_REG_WEIGHTS)
    tail = () if code is None else (code,)
    _lib.call(entry, pred.data_ptr(), data["rois"].data_ptr(), data["s_count"].data_ptr(), *[t.data_ptr() for t in want], N, S, 1, STRIDE,
              rw, 240.0, 320.0, None, spec.BOX_SCORE_THRESH, ops._dt(pred), *tail, stream())
    torch.cuda.synchronize()
    assert bool((want[0][1, 5:] == -1).all()) and bool((want[0][0] > 0).all())    # rows past counts (8, 5) are dropped
    assert len(got) == 4
    for a, b in zip(got, want):
        assert same(a, b)
    short = ops.box_decode(pred, data["rois"], data["s_count"], spec.BOX_REG_WEIGHTS, 240, 320, spec.BOX_SCORE_THRESH, cls_loss=mode,
                           soft_labeling=soft_labeling)
    assert len(short) == 2 and same(short[0], want[0]) and same(short[1], want[1])
