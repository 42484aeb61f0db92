"""GPU (-m gpu): query augmentation groups (supp_aug=A, supp_aug_method='avg' | 'max'; FEW_SHOT.SUPP_AUG, generalized_rcnn.py:235-294).
The two kernels of oneshotdet_amd/csrc/supp_aug.hip against torch and numpy closed forms, bit for bit where the header promises bits
(the maximum, the mean of two, the tie rule of the 'max' backward); both engines against the fixtures recorded through the reference
(tests/golden/make_golden_supp_aug.py) with the helpers and tolerances of tests/test_gpu_query_avgpool.py; the gallery, the class sweep,
hipGraph replay and the launch trace in this mode; and that supp_aug=1 changes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_utils as gu
import supp_aug_ref as sar
from oneshotdet_amd import spec, synth
from test_gpu_box_head import fixture_proposals, nchw
from test_gpu_query_avgpool import _batch, _check_first_stage, _check_grads, _traced

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
MAPS = [(1, 1), (2, 2), (13, 17), (16, 16)]
CHANNELS = [256, 8, 24]        # the FPN's count; one 16-byte group of bf16; a group count that does not divide the workgroup
A = sar.AUG


def _maps(rows, dt, c, seed=0, values=None):
    """NHWC maps of every size in MAPS; values=16: drawn from 16 distinct values (exact in bf16), so every group has ties"""
    g = torch.Generator().manual_seed(seed)
    if values:
        return [((torch.randint(0, values, (rows, h, w, c), generator=g).float() - 7.0) * 0.25).to(DT[dt]).cuda() for h, w in MAPS]
    return [torch.randn(rows, h, w, c, generator=g).to(DT[dt]).cuda() for h, w in MAPS]


def _np(t):
    return t.float().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("aug", [2, 3])
@pytest.mark.parametrize("groups", [1, 3])
def test_forward_kernels_bitwise_reproducible_and_batch_independent(dt, aug, groups):
    from oneshotdet_amd import ops
    for c in CHANNELS:
        xs = _maps(groups * aug, dt, c, seed=c + aug)
        got = {m: ops.supp_aug_reduce_levels(xs, aug, m) for m in ("avg", "max")}
        for x, y_avg, y_max in zip(xs, got["avg"], got["max"]):
            shape = (groups,) + tuple(x.shape[1:])
            assert tuple(y_avg.shape) == tuple(y_max.shape) == shape and y_avg.dtype == y_max.dtype == x.dtype
            assert y_avg.is_contiguous() and y_max.is_contiguous()
            # max: the exact maximum
            assert torch.equal(y_max, torch.amax(x.view((groups, aug) + tuple(x.shape[1:])), dim=1)), (c, shape)
            # avg: the members added in order in fp32, ONE true division, ONE rounding to the dtype
            ref = sar.avg_closed_form(_np(x), aug)
            if dt == "bf16":
                assert torch.equal(y_avg.cpu(), torch.from_numpy(ref).to(torch.bfloat16)), (c, shape)
            elif aug == 2:
                assert np.array_equal(_np(y_avg), ref), (c, shape)
            else:
                assert sar.within_one_ulp(_np(y_avg), ref), (c, shape)
        for m in ("avg", "max"):
            again = ops.supp_aug_reduce_levels(xs, aug, m)
            assert all(torch.equal(a, b) for a, b in zip(got[m], again)), m
            for i in range(groups):       # group i alone is bit-equal to group i of the batch
                alone = ops.supp_aug_reduce_levels([x[i * aug:(i + 1) * aug] for x in xs], aug, m)
                assert all(torch.equal(a[0], b[i]) for a, b in zip(alone, got[m])), (m, i)


def _call_bwd(xs, dys, dxs, aug, method):
    """osd_supp_aug_reduce_levels_bwd by name, into buffers of the caller"""
    from oneshotdet_amd import _lib, ops
    k = len(xs)
    arr = lambda ts: (C.c_void_p * k)(*[t.data_ptr() for t in ts])      # noqa: E731
    _lib.call("osd_supp_aug_reduce_levels_bwd", k, arr(xs), arr(dys), arr(dxs), (C.c_int32 * k)(*[x.shape[1] * x.shape[2] for x in xs]),
              xs[0].shape[0] // aug, aug, xs[0].shape[-1], ops._dt(xs[0]), ops.SUPP_AUG_METHODS[method], ops._stream())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("aug", [2, 3])
@pytest.mark.parametrize("groups", [1, 3])
def test_max_backward_follows_torch_cpu_tie_rule_and_writes_every_element(dt, aug, groups):
    from oneshotdet_amd import ops
    for c in CHANNELS:
        xs = _maps(groups * aug, dt, c, seed=3 * c + aug, values=16)
        dys = _maps(groups, dt, c, seed=c + 100)
        got = ops.supp_aug_reduce_levels_bwd(xs, dys, aug, "max")
        filled = [torch.full_like(x, float("nan")) for x in xs]
        _call_bwd(xs, dys, filled, aug, "max")
        for x, dy, dx, fl in zip(xs, dys, got, filled):
            xc = x.float().cpu().requires_grad_(True)
            grouped = xc.view((groups, aug) + tuple(x.shape[1:]))
            ties = (grouped == grouped.max(dim=1, keepdim=True)[0]).sum(dim=1)
            assert x.numel() // aug < 256 or int(ties.max()) > 1          # 16 values: a map of 256 positions or more surely has ties
            grouped.max(dim=1)[0].backward(dy.float().cpu())
            assert dx.dtype == x.dtype and dx.shape == x.shape
            assert torch.equal(dx.cpu(), xc.grad.to(x.dtype)), (c, tuple(x.shape))      # bf16: dy or 0, exact in the cast
            assert not bool(torch.isnan(fl).any()) and torch.equal(fl, dx)
        again = ops.supp_aug_reduce_levels_bwd(xs, dys, aug, "max")
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        for i in range(groups):
            alone = ops.supp_aug_reduce_levels_bwd([x[i * aug:(i + 1) * aug] for x in xs], [d[i:i + 1] for d in dys], aug, "max")
            assert all(torch.equal(a, b[i * aug:(i + 1) * aug]) for a, b in zip(alone, got)), i


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("aug", [2, 3])
@pytest.mark.parametrize("groups", [1, 3])
def test_avg_backward_closed_form_and_writes_every_element(dt, aug, groups):
    from oneshotdet_amd import ops
    for c in CHANNELS:
        xs = _maps(groups * aug, dt, c, seed=c)
        dys = _maps(groups, dt, c, seed=c + 200)
        got = ops.supp_aug_reduce_levels_bwd(xs, dys, aug, "avg")
        filled = [torch.full_like(x, float("nan")) for x in xs]
        _call_bwd(xs, dys, filled, aug, "avg")
        for x, dy, dx, fl in zip(xs, dys, got, filled):
            ref = np.repeat((_np(dy) / np.float32(aug)).astype(np.float32), aug, axis=0)       # dy / A to every member, fp32
            assert dx.dtype == x.dtype and dx.shape == x.shape
            if dt == "bf16":
                assert torch.equal(dx.cpu(), torch.from_numpy(ref).to(torch.bfloat16)), (c, tuple(x.shape))
            elif aug == 2:
                assert np.array_equal(_np(dx), ref), (c, tuple(x.shape))
            else:
                assert sar.within_one_ulp(_np(dx), ref), (c, tuple(x.shape))
            assert not bool(torch.isnan(fl).any()) and torch.equal(fl, dx)
        again = ops.supp_aug_reduce_levels_bwd(xs, dys, aug, "avg")
        assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_kernels_refuse_with_the_documented_codes():
    from oneshotdet_amd import _lib, ops
    x12 = torch.zeros(4, 2, 2, 12, device="cuda", dtype=torch.bfloat16)         # 12 bf16 channels: no multiple of 8
    x8 = torch.zeros(4, 2, 2, 8, device="cuda")
    for fn, args, code in ((ops.supp_aug_reduce_levels, ([x12], 2), -2), (ops.supp_aug_reduce_levels_bwd, ([x12], [x12[:2]], 2), -2),
                           (ops.supp_aug_reduce_levels, ([x8], 1), -1), (ops.supp_aug_reduce_levels_bwd, ([x8], [x8], 1), -1),
                           (ops.supp_aug_reduce_levels, ([x8] * 9, 2), -1), (ops.supp_aug_reduce_levels_bwd, ([x8] * 9, [x8[:2]] * 9, 2), -1)):
        for method in ("avg", "max"):
            with pytest.raises(_lib.OsdError) as e:
                fn(*args, method)
            assert e.value.code == code, (fn.__name__, code)
    empty = ops.supp_aug_reduce_levels([x8[:0]], 2, "max")                        # no groups: nothing launched, nothing raised
    assert tuple(empty[0].shape) == (0, 2, 2, 8)


# ------------------------------------------------------------------------------------------------------------- inference
_ENGINES = {}


def _engine(method, shared=False, dt="f32", full=False):
    from oneshotdet_amd import model
    key = (method, shared, dt, full)
    if key not in _ENGINES:
        shapes = spec.full_model_shapes(not shared) if full else spec.hot_path_shapes(not shared)
        _ENGINES[key] = model.HotPathEngine(synth.make_state_dict(shapes), dtype=DT[dt], siamese_backbone=not shared,
                                            supp_aug=A, supp_aug_method=method)
    return _ENGINES[key]


def _inputs(case):
    img, q = sar.case_inputs(case)
    return torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda()


@pytest.mark.parametrize("method,case,shared", sar.FORWARD_CASES)
def test_engine_forward_matches_reference_fixture(method, case, shared):
    B, H, W, S, qh, qw = gu.CASES[case]
    f = gu.load(sar.forward_name(method, case, shared))
    eng = _engine(method, shared)
    img, q = _inputs(case)
    assert q.shape[0] == B * S * A
    out = eng.detect(img, q, cuda_nms=False)
    assert out["query_features"][0].shape[0] == B * S and out["query_features_unmerged"][0].shape[0] == B * S * A
    _check_first_stage(out, f, [(H, W)] * B)
    for lvl in range(5):
        gu.check_against(nchw(out["query_features_unmerged"][lvl]).numpy(), f, "query_features_unmerged.%d" % lvl, 1e-3, 1e-3)
    # the fixture's pooled vectors are the merged maps': the other method misses them
    other = _engine("avg" if method == "max" else "max", shared).forward(img, q)["pooled"][0].cpu().numpy()
    assert not np.allclose(other, f["pooled.0"], rtol=1e-2, atol=1e-3)


def test_second_stage_matches_reference_fixture():
    """box_suppaug_max_small: the reference's full eval forward with roi_heads.  Its proposals through OUR features, OUR merged query
    maps and OUR box head, at test_gpu_box_head's fp32 bars; then detect(second_stage=True) end to end at its end-to-end bars."""
    method, case = sar.BOX_CASE
    B, H, W, S, qh, qw = gu.CASES[case]
    f = gu.load("box_suppaug_%s_%s.npz" % (method, case))
    eng = _engine(method, full=True)
    img, q = _inputs(case)
    feats, qfeats, _, _ = eng.forward_features(img, q)
    assert qfeats[0].shape[0] == B * S
    props = fixture_proposals(f, B)
    out = eng.box_detect(feats, qfeats, (qh, qw), props, None, H, W, shots=S, cuda_nms=False, want_raw=True)
    gu.check_against(nchw(out["pooled"]).numpy(), f, "pooled", 1e-3, 1e-3)
    gu.check_against(nchw(out["query_roi"]).numpy(), f, "supp_roi", 1e-3, 1e-3)
    np.testing.assert_allclose(out["logits"].cpu().numpy(), f["logits"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(out["box_regression"].cpu().numpy(), f["box_regression"], rtol=1e-3, atol=1e-3)
    rb, rs = f["detections.0.boxes"], f["detections.0.scores"]
    k = int(out["counts"][0])
    assert abs(k - len(rb)) <= max(1, len(rb) // 100), (k, len(rb))
    assert gu.match_boxes(rb, rs, out["boxes"][0, :k].cpu().numpy(), out["scores"][0, :k].cpu().numpy()) >= 0.99
    det = eng.detect(img, q, cuda_nms=False, second_stage=True)["detections"]
    k = int(det["counts"][0])
    assert abs(k - len(rb)) <= max(1, len(rb) // 50), (k, len(rb))
    assert gu.match_boxes(rb, rs, det["boxes"][0, :k].cpu().numpy(), det["scores"][0, :k].cpu().numpy()) >= 0.97


@pytest.mark.parametrize("method", ["avg", "max"])
@pytest.mark.parametrize("schedule", ["concurrent", "serial", "lockstep"])
def test_bf16_merged_maps_are_the_kernel_on_the_engines_own_maps(method, schedule, monkeypatch):
    from oneshotdet_amd import model, ops
    eng = _engine(method, dt="bf16")
    img, q = _inputs("shots5")
    monkeypatch.setattr(model, "LOCKSTEP", schedule == "lockstep")
    out = eng.forward(img, q, concurrent=schedule != "serial")
    torch.cuda.synchronize()
    raw, merged = out["query_features_unmerged"], out["query_features"]
    assert raw[0].dtype == torch.bfloat16 and raw[0].shape[0] == q.shape[0] and merged[0].shape[0] == q.shape[0] // A
    again = ops.supp_aug_reduce_levels(raw, A, method)
    assert all(torch.equal(a, b) for a, b in zip(merged, again))
    want = [sar.merge(r.float(), A, method).to(torch.bfloat16) for r in raw]        # avg of two: exact sum, one rounding
    assert all(torch.equal(a, b) for a, b in zip(merged, want))


H, W, QS = 128, 160, 64
SIZES = [(96, 160), (80, 150)]


def _targets(B, seed=0):
    from oneshotdet_amd import layers
    img = torch.from_numpy(synth.make_images("suppaug.target", B, H, W, seed=seed))
    for i, (h, w) in enumerate(SIZES[:B]):
        img[i, :, h:, :] = 0
        img[i, :, :, w:] = 0
    return layers.ImageList(img.cuda(), SIZES[:B])


def _groups(rows, seed=1):
    return sar.aug_queries(torch.from_numpy(synth.make_images("suppaug.query", rows, QS, QS, seed=seed))).cuda()


def _assert_stages_close(got, ref, rows):
    """the bound of test_gpu_gallery / test_gpu_class_sweep: combined rtol 1e-3 + 1e-3 of the absmax, head outputs 1e-3 + 1e-3"""
    for lvl in range(5):
        a, b = got["combined"][lvl], ref["combined"][lvl]
        assert a.shape == b.shape and a.shape[0] == rows
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()))
        for a, b in zip(got["head"][lvl], ref["head"][lvl]):
            torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("method", ["avg", "max"])
def test_enrolled_bank_matches_detect_on_the_same_groups(method):
    """enroll(G*A rows) then detect(bank=, class_ids=) against detect(gathered query groups, classes=K)"""
    eng = _engine(method, full=True)
    B, G, K = 2, 4, 3
    ids = [[2, 0, 3], [1, 1, 0]]
    images, gallery = _targets(B, seed=4), _groups(G, seed=5)
    assert gallery.shape[0] == G * A
    bank = eng.enroll(gallery)
    assert (bank.slots, bank.shots) == (G, 1) and bank.pooled[0].shape[0] == G and bank.q_half.shape[0] == G
    got = eng.detect(images, bank=bank, class_ids=ids, second_stage=True)
    rows = [g * A + a for r in ids for g in r for a in range(A)]
    queries = gallery.index_select(0, torch.tensor(rows, device="cuda")).contiguous()
    ref = eng.detect(images, queries, classes=K, second_stage=True)
    torch.cuda.synchronize()
    assert got["classes"] == K and ref["classes"] == K and ref["query_features"][0].shape[0] == B * K
    assert all(torch.equal(a, b) for a, b in zip(got["features"], ref["features"]))
    _assert_stages_close(got, ref, B * K)
    assert got["detections"]["counts"].shape == (B * K,) and int(got["detections"]["counts"].sum()) > 0
    with pytest.raises(ValueError, match="no multiple of supp_aug"):
        eng.enroll(gallery[:3])


@pytest.mark.parametrize("method", ["avg", "max"])
def test_class_sweep_matches_the_per_pair_calls(method):
    """classes=2 with groups of two against the two per-pair calls, each on its slot's groups"""
    eng = _engine(method, full=True)
    B, K = 2, 2
    images, queries = _targets(B, seed=6), _groups(B * K, seed=7)
    got = eng.detect(images, queries, classes=K, second_stage=True)
    torch.cuda.synchronize()
    assert got["classes"] == K and got["query_features"][0].shape[0] == B * K
    for k in range(K):
        rows = [(b * K + k) * A + a for b in range(B) for a in range(A)]
        ref = eng.detect(images, queries.index_select(0, torch.tensor(rows, device="cuda")).contiguous(), second_stage=True)
        torch.cuda.synchronize()
        sel = {key: [t[k::K] for t in got[key]] for key in ("combined",)}
        sel["head"] = [(c[k::K], r[k::K]) for c, r in got["head"]]
        _assert_stages_close(sel, ref, B)
        assert all(torch.equal(a, b) for a, b in zip(got["features"], ref["features"]))


def test_graphed_detect_equals_eager_bitwise():
    from oneshotdet_amd import model
    eng = _engine("max", dt="bf16")
    img, q = _inputs("shots5")
    g = model.GraphedDetect(eng, img, q)
    for images, queries in ((img, q), (img.flip(-1).contiguous(), q.flip(-2).contiguous())):
        got = g(images, queries)
        torch.cuda.synchronize()
        eager = eng.detect(images, queries)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got["pooled"], eager["pooled"]))
        assert all(torch.equal(a, b) for a, b in zip(got["query_features"], eager["query_features"]))
        for a, b in zip(got["proposals"], eager["proposals"]):
            assert torch.equal(a, b)


def test_unequal_sizes_in_a_group_are_refused_by_name():
    from oneshotdet_amd import layers, train
    eng = _engine("max", full=True)
    img, q = _inputs("small")
    ok = layers.ImageList(q, [(63, 63), (63, 63)])
    bad = layers.ImageList(q, [(63, 63), (60, 63)])
    assert eng.detect(img, ok, second_stage=True)["detections"]["counts"].shape == (1,)
    from oneshotdet_amd import trace
    for call in (lambda: eng.detect(img, bad), lambda: eng.detect(img, bad, second_stage=True), lambda: eng.enroll(bad),
                 lambda: eng.forward(img, bad.tensors, query_sizes=bad.image_sizes)):
        trace.TRACE = []
        try:
            with pytest.raises(ValueError, match=r"query group 0 \(rows 0 \.\. 1\).*different sizes"):
                call()
            assert trace.TRACE == []          # refused before anything was launched
        finally:
            trace.TRACE = None
    t = _train("max", "f32")
    _, _, gtb, cnt = _batch("small")
    with pytest.raises(ValueError, match=r"query group 0 \(rows 0 \.\. 1\).*different sizes"):
        t.forward_backward(img, bad, gtb, cnt)
    with pytest.raises(ValueError, match="no multiple of supp_aug"):
        t.forward_backward(img, torch.cat([q, q[:1]]), gtb, cnt)
    assert isinstance(t, train.TrainEngine)


# ------------------------------------------------------------------------------------------------------------- training
_TRAIN = {}


def _train(method, dt, roialign=True, **kw):
    from oneshotdet_amd import train
    key = (method, dt, roialign) + tuple(sorted(kw.items()))
    if key not in _TRAIN:
        _TRAIN[key] = train.TrainEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=DT[dt], supp_roialign=roialign,
                                        supp_aug=A, supp_aug_method=method, **kw)
    return _TRAIN[key]


def _aug_batch(case):
    img, q, gtb, cnt = _batch(case)
    return img, sar.aug_queries(q), gtb, cnt


@pytest.mark.parametrize("method,case,roialign", sar.TRAIN_CASES)
def test_train_step_fp32_matches_reference_fixture(method, case, roialign):
    """One fp32 forward + backward against train_suppaug_*: the losses and the sampled gradients of both backbones and the head, at
    test_gpu_query_avgpool's bars for the same case.  max_nonsquare's gradients were the reference's own autograd's, torch's max
    backward included (the fixture's oracle gradients were held against them before it was written)."""
    f = gu.load(sar.train_name(method, case))
    eng = _train(method, "f32", roialign)
    losses = eng.forward_backward(*_aug_batch(case)).cpu().numpy()
    print(method, case, "losses", losses, "fixture", f["losses_cuda_formula"], int(f["num_pos"]))
    assert int(losses[3]) == int(f["num_pos"])
    np.testing.assert_allclose(losses[:3], f["losses_cuda_formula"], rtol=1e-4)
    _check_grads(eng.named_grads(), f, "f32", case, False)


@pytest.mark.parametrize("method,case,roialign", sar.TRAIN_CASES)
def test_train_step_bf16_losses_match_reference_fixture(method, case, roialign):
    """bf16: the losses only.  Weight gradients under 'max' are checked in fp32: bf16 storage makes ties between a crop and its flip
    common, and a tie decides which member the gradient goes to."""
    f = gu.load(sar.train_name(method, case))
    eng = _train(method, "bf16", roialign)
    losses = eng.forward_backward(*_aug_batch(case)).cpu().numpy()
    print(method, case, "bf16 losses", losses, "fixture", f["losses_cuda_formula"])
    assert int(losses[3]) == int(f["num_pos"])
    np.testing.assert_allclose(losses[:3], f["losses_cuda_formula"], rtol=3e-2)


@pytest.mark.parametrize("method", ["avg", "max"])
def test_one_merge_launch_per_direction_each_checked_from_its_own_inputs(method):
    """Through the launch trace: a training step makes ONE forward and ONE backward merge launch for all five levels (two backbones
    or one), the inference forward one; every launch is checked from its own recorded operands."""
    from oneshotdet_amd import train
    img, q, gtb, cnt = _aug_batch("shots5")
    for shared in (False, True):
        eng = _train(method, "bf16") if not shared else train.TrainEngine(
            synth.make_state_dict(spec.hot_path_shapes(False)), dtype=torch.bfloat16, siamese_backbone=False, supp_aug=A, supp_aug_method=method)
        eng.forward_backward(img, q, gtb, cnt, with_proposals=False)
        tr = _traced(lambda: eng.forward_backward(img, q, gtb, cnt, with_proposals=False))
        kinds = [k for k, _ in tr]
        assert kinds.count("supp_aug_reduce") == 1 and kinds.count("supp_aug_reduce_bwd") == 1, kinds
        assert kinds.index("supp_aug_reduce") < kinds.index("query_pool") < kinds.index("query_pool_bwd") < kinds.index("supp_aug_reduce_bwd")
        for kind, r in tr:
            if kind == "supp_aug_reduce":
                assert len(r["xs"]) == 5 and r["xs"][0].shape[0] == q.shape[0] and r["aug"] == A and r["method"] == method
                for x, y in zip(r["xs"], r["outs"]):
                    assert torch.equal(y, sar.merge(x.float(), A, method).to(x.dtype))
            elif kind == "supp_aug_reduce_bwd":
                assert len(r["xs"]) == 5 and r["outs"][0].shape[0] == q.shape[0]
                for x, dy, dx in zip(r["xs"], r["dys"], r["outs"]):
                    xc = x.float().cpu().requires_grad_(True)
                    sar.merge(xc, A, method).backward(dy.float().cpu())
                    assert torch.equal(dx.cpu(), xc.grad.to(dx.dtype))       # avg: dy / 2, exact; max: torch's CPU tie rule
        if shared:
            eng.close()
    inf = _traced(lambda: _engine(method, dt="bf16").forward(img, q))
    assert [k for k, _ in inf].count("supp_aug_reduce") == 1


def test_second_stage_gradient_reaches_every_member_through_the_merge():
    """Both stages, fp32, 'avg': the first-stage losses equal the first-stage-only engine's, the box losses are finite, the second
    stage's query gradient joins the merged maps' gradient (the query backbone's gradients differ from the first-stage-only run's), and
    a full train_step stays finite."""
    from oneshotdet_amd import train
    batch = _aug_batch("small")
    both = train.TrainEngine(synth.make_state_dict(spec.full_model_shapes()), dtype=torch.float32, second_stage=True, ordered_wgrad=True,
                             supp_aug=A, supp_aug_method="avg")
    first = _train("avg", "f32", ordered_wgrad=True)
    torch.manual_seed(5)
    l2 = both.forward_backward(*batch).cpu()
    box, g2 = both.box_losses.cpu(), both.named_grads()
    l1 = first.forward_backward(*batch).cpu()
    g1 = first.named_grads()
    assert bool(torch.isfinite(l2).all()) and bool(torch.isfinite(box).all()) and float(box[0]) > 0
    np.testing.assert_allclose(l2[:3].numpy(), l1[:3].numpy(), rtol=1e-4)
    k = "supp_backbone.body.layer4.2.conv3.weight"
    assert float((g2[k] - g1[k]).abs().max()) > 1e-3 * float(g1[k].abs().max())
    torch.manual_seed(6)
    assert bool(torch.isfinite(both.train_step(*batch)).all())
    both.close()


def test_captured_training_step_matches_eager_steps():
    """capture() + replay_step with supp_aug=2 against eager train_steps on changing data, compared as
    tests/test_gpu_train.py::test_captured_training_step_matches_eager_steps compares them."""
    from oneshotdet_amd import train
    np_sd = synth.make_state_dict(spec.hot_path_shapes())
    B, h, w = 2, 128, 160
    q = sar.aug_queries(torch.from_numpy(synth.make_images("cg.q", B, 63, 63, seed=1))).cuda()
    batches = []
    for step in range(3):
        img = torch.from_numpy(synth.make_images("cg.img.%d" % step, B, h, w, seed=step)).cuda()
        gts = synth.make_gt_boxes(B, h, w, seed=60 + step, max_boxes=3)
        gtb = torch.zeros(B, 3, 4)
        for i, g in enumerate(gts):
            gtb[i, :len(g)] = torch.from_numpy(g)
        batches.append((img, gtb.cuda(), torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda()))
    out = {}
    for graphed in (False, True):
        eng = train.TrainEngine(np_sd, dtype=torch.float32, lr=0.002, supp_aug=A, supp_aug_method="max")
        first = eng.train_step(batches[0][0], q, batches[0][1], batches[0][2]).clone()
        if graphed:
            eng.join()
            w0, m0, n0 = eng.flat_w.clone(), eng._sgd["buf"].clone(), eng._sgd["steps"]
            eng.capture(batches[0][0], q, batches[0][1], batches[0][2], warmup=1)
            eng.flat_w.copy_(w0)
            eng._sgd["buf"].copy_(m0)
            eng._sgd["steps"] = n0
            eng.repack()
            losses = [eng.replay_step(img, q, gtb, cnt).clone() for img, gtb, cnt in batches[1:]]
        else:
            losses = [eng.train_step(img, q, gtb, cnt).clone() for img, gtb, cnt in batches[1:]]
        eng.join()
        torch.cuda.synchronize()
        out[graphed] = (torch.stack([first] + losses).cpu(), eng.flat_w.clone().cpu())
        eng.close()
    np.testing.assert_allclose(out[True][0].numpy(), out[False][0].numpy(), rtol=2e-3, atol=1e-6)
    assert float((out[True][1] - out[False][1]).norm() / out[False][1].norm()) < 1e-4


# ------------------------------------------------------------------------------------------------------------- the default
def test_supp_aug_1_launches_no_merge_and_changes_no_bit():
    from oneshotdet_amd import model, train
    img, q, gtb, cnt = _batch("shots5")
    sd = synth.make_state_dict(spec.full_model_shapes())
    plain = model.HotPathEngine(sd, dtype=torch.bfloat16)
    off = model.HotPathEngine(sd, dtype=torch.bfloat16, supp_aug=1, supp_aug_method="max")
    outs = []
    for eng in (plain, off):
        tr = _traced(lambda: outs.append(eng.detect(img, q, second_stage=True)))
        assert not any(k.startswith("supp_aug") for k, _ in tr)
    a, b = outs
    assert sorted(a) == sorted(b) and "query_features_unmerged" not in b
    for key in ("features", "query_features", "pooled", "combined"):
        assert all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    assert all(torch.equal(x, y) for (x, _), (y, _) in zip(a["head"], b["head"])) and all(torch.equal(x, y) for (_, x), (_, y) in zip(a["head"], b["head"]))
    assert all(torch.equal(x, y) for x, y in zip(a["proposals"], b["proposals"]))
    assert all(torch.equal(a["detections"][k], b["detections"][k]) for k in ("boxes", "scores", "counts"))
    kinds, heads = [], []
    for kw in ({}, {"supp_aug": 1, "supp_aug_method": "max"}):
        eng = train.TrainEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=torch.bfloat16, **kw)
        tr = _traced(lambda: eng.forward_backward(img, q, gtb, cnt))
        kinds.append([k for k, _ in tr])
        heads.append([t.clone() for pair in eng.last_head_out for t in pair])
        eng.close()
    # the same launches in the same order, and the forward pass's every output bit for bit
    assert kinds[0] == kinds[1] and not any(k.startswith("supp_aug") for k in kinds[0])
    assert all(torch.equal(x, y) for x, y in zip(heads[0], heads[1]))
