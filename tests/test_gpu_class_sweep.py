"""GPU (-m gpu): the class sweep — K category slots per target image in one pass (detect(..., classes=K)).  The two kernels that
read ONE target pyramid from K rows (osd_correlate_levels_sweep, osd_roi_pool_levels_sweep) against the per-pair entries on K times
replicated maps, bit for bit; the sweep's stages against the per-pair stages on the replicated batch, bit for bit from the same
features; the whole call against the per-pair call on the replicated batch at the project's fp32 bar (the backbones run at other
batch sizes); hipGraph replay; OneShotDetector with nested target_ids; and the refusals that come before any launch."""
import pytest
import torch

from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LEVELS = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 2)]      # odd pixel counts, levels smaller than one slab, the tail iteration
H, W, QS = 96, 160, 64
SIZES = [(96, 160), (80, 150)]                           # true sizes of the two padded targets


def _group():
    from oneshotdet_amd import ops
    return ops.class_sweep_group()


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [64, 256])
def test_sweep_correlation_is_the_per_pair_launch_on_replicated_maps_bit_for_bit(dt, c):
    from oneshotdet_amd import ops
    n, G = 2, _group()
    g = torch.Generator().manual_seed(c)
    xs = [torch.randn(n, h, w, c, generator=g).to(DT[dt]).cuda() for h, w in LEVELS]
    for K in (1, 3, G, G + 1, 2 * G + 1):                # one slot, a short group, a full one, full + 1, two full + 1
        qs = [torch.randn(n * K, c, generator=g).cuda() for _ in LEVELS]
        got = ops.correlate_levels_sweep(xs, qs, K)
        ref = ops.correlate_levels([x.repeat_interleave(K, 0) for x in xs], qs)
        for (h, w), a, b in zip(LEVELS, got, ref):
            assert a.shape == (n * K, h, w, c) and a.dtype == DT[dt]
            assert torch.equal(a, b), (K, h, w)
        if K == 1:
            assert all(torch.equal(a, b) for a, b in zip(got, ops.correlate_levels(xs, qs)))


def test_sweep_correlation_refusals_and_empty_batch():
    from oneshotdet_amd import _lib, ops
    x = torch.zeros(2, 3, 3, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.correlate_levels_sweep([x], [torch.zeros(0, 64, device="cuda")], 0)
    with pytest.raises(_lib.OsdError) as e:               # 12 channels: no multiple of the 16-byte chunk the rule asks for
        ops.correlate_levels_sweep([torch.zeros(2, 3, 3, 12, device="cuda", dtype=torch.bfloat16)], [torch.zeros(6, 12, device="cuda")], 3)
    assert e.value.code == -1
    (y,) = ops.correlate_levels_sweep([x[:0]], [torch.zeros(0, 64, device="cuda")], 3)
    assert y.shape == (0, 3, 3, 64)


def _roi_inputs(dt, c=256):
    """n = 2 images, K = 3: six ROI sets of up to 7 boxes whose sides put them on every pooler level (LevelMapper: sqrt(area) below
    224 -> P3, then one level per doubling) and whose extent leaves the 128 x 160 image on every side"""
    g = torch.Generator().manual_seed(11)
    maps = [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)]
    feats = [torch.randn(2, h, w, c, generator=g).to(DT[dt]).cuda() for h, w in maps]
    sides = torch.tensor([2000.0, 40.0, 300.0, 600.0, 1000.0, 100.0, 500.0])
    centre = torch.rand(6, 7, 2, generator=g) * torch.tensor([160.0, 128.0])
    jitter = 1.0 + 0.2 * torch.rand(6, 7, 2, generator=g)
    half = 0.5 * sides[None, :, None] * jitter
    boxes = torch.cat([centre - half, centre + half], -1).contiguous().cuda()
    counts = torch.tensor([7, 0, 3, 5, 1, 7], dtype=torch.int32).cuda()
    return feats, boxes, counts


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_sweep_roi_pooling_is_the_per_pair_launch_on_replicated_maps_bit_for_bit(dt):
    from oneshotdet_amd import ops
    K = 3
    feats, boxes, counts = _roi_inputs(dt)
    got, lv = ops.roi_pool_levels(feats, spec.POOLER_SCALES, boxes, counts, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO, want_levels=True,
                                  sets_per_image=K)
    ref, lv_ref = ops.roi_pool_levels([f.repeat_interleave(K, 0) for f in feats], spec.POOLER_SCALES, boxes, counts, spec.BOX_POOL,
                                      spec.POOLER_SAMPLING_RATIO, want_levels=True)
    assert got.shape == (6 * 7, spec.BOX_POOL, spec.BOX_POOL, 256) and got.dtype == DT[dt]
    assert torch.equal(got, ref) and torch.equal(lv, lv_ref)
    assert sorted(set(lv.cpu().tolist())) == [-1, 0, 1, 2, 3, 4]          # dead rows and every level
    live = (torch.arange(7, device="cuda")[None] < counts[:, None]).reshape(-1)
    assert bool((got[~live] == 0).all()) and bool((got[live].abs().amax((1, 2, 3)) > 0).all())
    # set j reads image j // K: the sets of image 1 differ from what image 0's maps give
    wrong = ops.roi_pool_levels([f[:1].repeat_interleave(6, 0) for f in feats], spec.POOLER_SCALES, boxes, counts, spec.BOX_POOL,
                                spec.POOLER_SAMPLING_RATIO)
    assert torch.equal(got[:3 * 7], wrong[:3 * 7]) and not torch.equal(got[3 * 7:], wrong[3 * 7:])
    # without counts every row is live
    a = ops.roi_pool_levels(feats, spec.POOLER_SCALES, boxes, None, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO, sets_per_image=K)
    b = ops.roi_pool_levels([f.repeat_interleave(K, 0) for f in feats], spec.POOLER_SCALES, boxes, None, spec.BOX_POOL,
                            spec.POOLER_SAMPLING_RATIO)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="6.*4"):
        ops.roi_pool_levels(feats, spec.POOLER_SCALES, boxes, counts, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO, sets_per_image=4)


# ------------------------------------------------------------------------------------------------------------- engine
_ENGINE = {}


def _engine(dtype=torch.float32):
    from oneshotdet_amd import model
    if dtype not in _ENGINE:
        _ENGINE[dtype] = model.HotPathEngine(synth.make_state_dict(spec.full_model_shapes()), dtype=dtype)
    return _ENGINE[dtype]


def _inputs(B, K, S, seed=0):
    """padded targets with their true sizes (zero outside them, as to_image_list pads) and B*K*S queries"""
    from oneshotdet_amd import layers
    img = torch.from_numpy(synth.make_images("sweep.target", B, H, W, seed=seed))
    sizes = SIZES[:B]
    for i, (h, w) in enumerate(sizes):
        img[i, :, h:, :] = 0
        img[i, :, :, w:] = 0
    q = torch.from_numpy(synth.make_images("sweep.query", B * K * S, QS, QS, seed=seed + 1))
    return layers.ImageList(img.cuda(), sizes), q.cuda()


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("B,K,S", [(2, 3, 1), (1, 2, 5)])
def test_sweep_stages_equal_the_per_pair_stages_on_replicated_features_bit_for_bit(B, K, S):
    """From ONE per-pair forward_features (B-row target features, B*K*S query maps): the per-pair run_correlate / run_head /
    run_proposals / run_box_head on K times replicated features against the sweep forms on the B rows.  Downstream of the two new
    kernels the launches are the same launches on the same shapes, so every stage is exact.  (1, 2, 5): the shots' arg-max."""
    from oneshotdet_amd import box_head, model
    eng = _engine()
    assert eng.box_cls_loss == "ce_loss"
    images, queries = _inputs(B, K, S)
    feats, qfeats, _, _ = eng.forward_features(images.tensors, queries)
    assert feats[0].shape[0] == B and qfeats[0].shape[0] == B * K * S
    pooled = model.run_query_pool(qfeats, [(QS, QS)] * (B * K * S), B * K)
    rep = [f.repeat_interleave(K, 0) for f in feats]
    rows = [s for s in images.image_sizes for _ in range(K)]
    hw = model.image_sizes_dev(rows, feats[0].device)
    old, new = {}, {}
    for out, fs, kw in ((old, rep, {}), (new, feats, dict(classes=K))):
        out["combined"] = model.run_correlate(fs, pooled, **kw)
        out["head"] = model.run_head(eng.head, out["combined"])
        out["proposals"] = model.run_proposals(out["head"], H, W, spec.PRE_NMS_TOP_N_TEST, spec.POST_NMS_TOP_N_TEST, spec.NMS_THRESH,
                                               image_sizes=rows)
        pb, _, pc = out["proposals"]
        out["detections"] = box_head.run_box_head(eng.box_head, fs, qfeats, (QS, QS), pb, pc, H, W, shots=S, img_hw=hw, **kw)
    torch.cuda.synchronize()
    for key in ("combined", "head", "proposals", "detections"):
        assert _same(old[key], new[key]), key
    assert new["combined"][0].shape[0] == B * K and new["detections"]["boxes"].shape[0] == B * K
    assert int(new["proposals"][2].min()) > 0 and int(new["detections"]["counts"].sum()) > 0
    # the K slots of an image are different categories: their combined maps differ
    assert not torch.equal(new["combined"][0][0], new["combined"][0][1])


def test_sweep_detect_matches_detect_on_the_replicated_batch():
    """detect(classes=3) against detect on the 3 times replicated images, fp32, B = 2 padded targets of 96 x 160, 64 x 64 queries.
    The target backbone runs on 2 images here and on 6 there and may take other tiles, so features are held to atol 1e-3 * absmax +
    rtol 1e-3 and head outputs to 1e-3 + 1e-3.  Measured on an MI355X: every compared tensor came out
    bit-equal (worst |difference| 0.0 for the features, the combined maps and the head outputs)."""
    from oneshotdet_amd import layers
    eng = _engine()
    B, K = 2, 3
    images, queries = _inputs(B, K, 1, seed=4)
    got = eng.detect(images, queries, classes=K, second_stage=True)
    rep = layers.ImageList(images.tensors.repeat_interleave(K, 0), [s for s in images.image_sizes for _ in range(K)])
    ref = eng.detect(rep, queries, second_stage=True)
    torch.cuda.synchronize()
    assert got["classes"] == K and "classes" not in ref
    worst = {"features": 0.0, "combined": 0.0, "head": 0.0}
    for lvl in range(5):
        a, b = got["features"][lvl], ref["features"][lvl][::K]
        assert a.shape[0] == B
        worst["features"] = max(worst["features"], float((a - b).abs().max()))
        print("features", lvl, float((a - b).abs().max()), float(b.abs().max()))
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()))
        a, b = got["combined"][lvl], ref["combined"][lvl]
        assert a.shape[0] == B * K
        worst["combined"] = max(worst["combined"], float((a - b).abs().max()))
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()))
        for a, b in zip(got["head"][lvl], ref["head"][lvl]):
            worst["head"] = max(worst["head"], float((a - b).abs().max()))
            torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3)
    print("worst differences:", worst)
    for a, b in zip(got["pooled"], ref["pooled"]):
        assert torch.equal(a, b)                         # the query branch is the same launches on the same rows
    assert got["proposals"][0].shape[0] == B * K and got["detections"]["counts"].shape == (B * K,)


def test_graphed_sweep_replays_equal_eager_bit_for_bit():
    from oneshotdet_amd import model
    eng = _engine(torch.bfloat16)
    B, K = 2, 3
    images, queries = _inputs(B, K, 1, seed=7)
    img = images.tensors
    g = model.GraphedDetect(eng, img, queries, classes=K, second_stage=True)
    for im, q in ((img, queries), (img.flip(-1).contiguous(), queries.flip(-2).contiguous())):
        got = g(im, q)
        torch.cuda.synchronize()
        eager = eng.detect(im, q, classes=K, second_stage=True)
        torch.cuda.synchronize()
        for key in ("features", "pooled", "combined", "head", "proposals", "detections"):
            assert _same(got[key], eager[key]), key
        assert got["combined"][0].shape[0] == B * K and int(got["detections"]["counts"].sum()) > 0


def test_one_shot_detector_with_nested_target_ids_returns_one_boxlist_per_image():
    from oneshotdet_amd import evaluation, layers, modules
    det = modules.OneShotDetector(synth.make_state_dict(spec.full_model_shapes()), dtype=torch.float32)
    B, K = 2, 3
    images, queries = _inputs(B, K, 1, seed=9)
    ids = [[3, 7, 5], [2, 9, 4]]
    res = det(images, queries, target_ids=ids)
    assert len(res) == B
    rep = layers.ImageList(images.tensors.repeat_interleave(K, 0), [s for s in images.image_sizes for _ in range(K)])
    pairs = det(rep, queries, target_ids=[i for row in ids for i in row])      # the per-pair forward: B*K BoxLists
    assert len(pairs) == B * K
    for b, bl in enumerate(res):
        h, w = images.image_sizes[b]
        assert bl.size == (w, h) and len(bl) == sum(len(p) for p in pairs[b * K:(b + 1) * K]) > 0
        s = bl.get_field("scores")
        assert bool((s[:-1] >= s[1:]).all())
        for k in range(K):
            one = pairs[b * K + k]
            sel = bl.get_field("labels") == ids[b][k]
            assert torch.equal(bl.bbox[sel], one.bbox) and torch.equal(s[sel], one.get_field("scores")), (b, k)
    gts = []
    for b, bl in enumerate(res):                          # the best detection of every image as its ground truth
        h, w = images.image_sizes[b]
        gt = modules.BoxList(bl.bbox[:1].clone(), (w, h))
        gt.add_field("labels", bl.get_field("labels")[:1].clone())
        gt.add_field("difficult", torch.zeros(1, dtype=torch.bool, device=bl.bbox.device))
        gts.append(gt)
    ev = evaluation.eval_detection_voc(res, gts)
    assert 0.0 < float(ev["map"]) <= 1.0
    flat = det(images, queries[::K].contiguous(), target_ids=[3, 2])          # a flat target_ids behaves as before
    assert len(flat) == B and int(flat[0].get_field("labels")[0]) == 3


def test_sweep_refusals_come_before_any_launch():
    from oneshotdet_amd import model, trace
    eng = _engine()
    images, queries = _inputs(2, 3, 1)
    one = model.HotPathEngine(synth.make_state_dict(spec.full_model_shapes(box_cls_loss="focal_loss")), dtype=torch.bfloat16,
                              box_cls_loss="focal_loss")
    _, q10 = _inputs(1, 2, 5)
    trace.TRACE = []
    try:
        with pytest.raises(ValueError, match=r"\b7 query rows.*2 x 3 = 6"):
            eng.detect(images, torch.cat([queries, queries[:1]]), classes=3, second_stage=True)
        with pytest.raises(ValueError, match=r"\b6 query rows.*2 x 4 = 8"):
            eng.forward(images.tensors, queries, classes=4)
        with pytest.raises(ValueError, match=r"box_head\.py:246-253"):      # a one-logit loss with S = 5 shots per slot
            one.detect(images.tensors[:1], q10, classes=2, second_stage=True)
        assert trace.TRACE == []
        out = one.detect(images.tensors[:1], q10[::5].contiguous(), classes=2, second_stage=True)       # one shot per slot runs
        assert len(trace.TRACE) > 0
    finally:
        trace.TRACE = None
    torch.cuda.synchronize()
    assert out["detections"]["counts"].shape == (2,)
