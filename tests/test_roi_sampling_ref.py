"""CPU: tests/roi_sampling_ref.py is right before it judges a kernel — against the real reference's recorded ROIAlign vectors
(tests/golden/roialign.npz) and the oracle (oracle/hotpath_ref.py, oracle/box_head_ref.py) — and the inputs of
tests/test_gpu_roi_sampling.py are what they claim: the exact cases are exact (the float32 geometry equals the same statements in
float64, bit for bit), every claimed threshold category is hit (counts printed: run with -s), the random cases keep every sample
at least 1e-3 away from -1 and from the map size."""
import numpy as np
import pytest
import torch

import golden_utils as gu
import roi_sampling_ref as rs
from oracle import box_head_ref as obh
from oracle import hotpath_ref as orc


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(np.asarray(a), (0, 2, 3, 1)))


def _nchw(a):
    return np.transpose(a, (0, 3, 1, 2))


def _golden_cases():
    f = gu.load("roialign.npz")
    for i in range(int(f["n"])):
        scale, ph, pw, sr = f["args.%d" % i]
        yield f["x.%d" % i], f["rois.%d" % i], float(scale), int(ph), int(pw), int(sr), f["y.%d" % i]


def test_forward_reproduces_the_reference_vectors_and_the_oracle():
    for x, rois, scale, ph, pw, sr, y in _golden_cases():
        got = _nchw(rs.forward(_nhwc(x), rois, scale, ph, pw, sr).y)
        np.testing.assert_allclose(got, y, rtol=1e-5, atol=1e-5)
        want = orc.roi_align(torch.from_numpy(x), torch.from_numpy(rois), scale, ph, pw, sr).numpy()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)


def _backward_cases():
    for x, rois, scale, ph, pw, sr, _ in _golden_cases():
        yield x.shape, rois, scale, ph, pw, sr
    yield (2, 5, 9, 12), np.array([[0, -6.0, -4.0, 30.0, 20.0], [1, 50.0, 30.0, 200.0, 100.0], [0, 10.0, 10.0, 10.0, 10.0],
                                   [1, 3.3, 2.2, 70.7, 41.9]], np.float32), 0.125, 3, 2, 2
    yield (2, 5, 9, 12), np.array([[1, 0.0, 0.0, 95.0, 71.0], [0, 7.5, 3.25, 60.0, 50.0]], np.float32), 0.125, 2, 3, 0


def test_backward_equals_the_restated_cuda_kernel_and_autograd():
    rng = np.random.RandomState(7)
    for (b, c, h, w), rois, scale, ph, pw, sr in _backward_cases():
        g = rng.randn(len(rois), c, ph, pw).astype(np.float32)
        got = _nchw(rs.backward(_nhwc(g), rois, (b, h, w, c), scale, ph, pw, sr).gx)
        want = orc.roi_align_backward_cuda(g, rois, scale, ph, pw, b, c, h, w, sr)
        xt = torch.zeros(b, c, h, w, requires_grad=True)
        orc.roi_align(xt, torch.from_numpy(np.asarray(rois, np.float32)), scale, ph, pw, sr).backward(torch.from_numpy(g))
        for ref in (want, xt.grad.numpy()):
            assert np.abs(got - ref).max() <= 1e-5 * max(float(np.abs(ref).max()), 1e-6)
        assert np.abs(want).sum() > 0


def test_backward_is_the_transpose_of_forward_and_counts_its_contributions():
    """<forward(x), gy> = <x, backward(gy)> in float64, A >= |gx|, and m = 0 exactly where nothing arrives."""
    rois = rs.exact_roialign_rois(3, 2, 0)
    b, h, w = rs.ROIALIGN_MAP
    x, gy = rs.data((b, h, w, 6), 3).double().numpy(), rs.data((len(rois), 3, 2, 6), 4).double().numpy()
    f, bw = rs.forward(x, rois, rs.ROIALIGN_SCALE, 3, 2, 0), rs.backward(gy, rois, (b, h, w, 6), rs.ROIALIGN_SCALE, 3, 2, 0)
    assert abs((f.y * gy).sum() - (x * bw.gx).sum()) <= 1e-12 * np.abs(f.y * gy).sum()
    assert (bw.A >= np.abs(bw.gx) - 1e-15).all() and (bw.gx[bw.m == 0] == 0).all() and (bw.m == 0).any()
    assert (f.S >= np.abs(f.y * f.count[:, None, None, None]) - 1e-12).all()
    assert int(bw.m.sum()) == int(f.n.sum())


def test_pooler_composition_equals_the_oracle_pooler():
    feats = [torch.randn(2, 8, h, w, generator=torch.Generator().manual_seed(l)) for l, (h, w) in enumerate(rs.POOL_SIZES)]
    boxes = rs.random_pool_boxes(rs.RANDOM_SEED)
    n, r, _ = boxes.shape
    want = obh.pooler(feats, [torch.from_numpy(boxes[i]) for i in range(n)]).reshape(n * r, 8, 7, 7).numpy()
    f, lv = rs.pool_levels([t.permute(0, 2, 3, 1) for t in feats], rs.POOL_SCALES, boxes, None, 7, 2)
    np.testing.assert_array_equal(lv, obh.map_levels(torch.from_numpy(boxes).reshape(-1, 4)).numpy())
    np.testing.assert_allclose(_nchw(f.y), want, rtol=1e-5, atol=1e-5)
    assert set(lv.tolist()) == {0, 1, 2, 3, 4}
    counts = np.array([r, r - 5], np.int32)
    f2, lv2 = rs.pool_levels([t.permute(0, 2, 3, 1) for t in feats], rs.POOL_SCALES, boxes, counts, 7, 2)
    assert (lv2[-5:] == -1).all() and (f2.y[-5:] == 0).all() and np.array_equal(f2.y[:-5], f.y[:-5])
    # the sweep: set j on image j // K
    f3, _ = rs.pool_levels([t.permute(0, 2, 3, 1)[:1] for t in feats], rs.POOL_SCALES, boxes, None, 7, 2, sets_per_image=2)
    f4, _ = rs.pool_levels([t.permute(0, 2, 3, 1)[:1].repeat(2, 1, 1, 1) for t in feats], rs.POOL_SCALES, boxes, None, 7, 2)
    assert np.array_equal(f3.y, f4.y)
    # backward: the transpose, level by level
    dy = rs.data((n * r, 7, 7, 8), 9).double().numpy()
    bws = rs.pool_levels_bwd(dy, rs.POOL_SIZES, rs.POOL_SCALES, boxes, counts, 7, 2)
    lhs = (f2.y * dy).sum()
    rhs = sum((t.permute(0, 2, 3, 1).double().numpy() * bw.gx).sum() for t, bw in zip(feats, bws))
    assert abs(lhs - rhs) <= 1e-12 * np.abs(f2.y * dy).sum()


def test_query_pooling_composition_equals_the_oracle():
    shots = 3
    rois = rs.exact_query_rois(shots)
    feats = [rs.data((2 * shots, h, w, 8), 20 + l) for l, (h, w) in enumerate(rs.QUERY_SIZES)]
    got = rs.query_pool(feats, rois, rs.POOL_SCALES, 2, 2)
    for x, sc, (y, bound) in zip(feats, rs.POOL_SCALES, got):
        want = orc.roi_align(x.permute(0, 3, 1, 2), torch.from_numpy(rois), sc, 1, 1, 2).view(2, shots, 8).mean(1).numpy()
        np.testing.assert_allclose(y, want, rtol=1e-5, atol=1e-5)
        assert (bound >= 0).all() and bound.max() < 1e-5
    dqs = [rs.data((2, 8), 40 + l) for l in range(5)]
    for dq, x, sc, bw in zip(dqs, feats, rs.POOL_SCALES, rs.query_pool_bwd(dqs, rois, [tuple(f.shape) for f in feats], rs.POOL_SCALES, shots, 2)):
        xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
        (orc.roi_align(xt, torch.from_numpy(rois), sc, 1, 1, 2).view(2, shots, 8).mean(1) * dq).sum().backward()
        ref = xt.grad.permute(0, 2, 3, 1).numpy()
        assert np.abs(bw.gx - ref).max() <= 1e-5 * np.abs(ref).max()


# ---- the inputs of tests/test_gpu_roi_sampling.py
@pytest.mark.parametrize("sampling", [2, 0])
@pytest.mark.parametrize("ph,pw", rs.ROIALIGN_POOLS)
def test_exact_roialign_cases_are_exact_and_hit_every_threshold(ph, pw, sampling):
    rois = rs.exact_roialign_rois(ph, pw, sampling)
    _, h, w = rs.ROIALIGN_MAP
    assert len(rois) <= 24
    for roi in rois:
        assert rs.is_exact(roi, rs.ROIALIGN_SCALE, h, w, ph, pw, sampling), roi
    hits = rs.threshold_hits(rois, rs.ROIALIGN_SCALE, h, w, ph, pw, sampling)
    print("roialign %dx%d sampling %d:" % (ph, pw, sampling), hits)
    for name in rs.ROIALIGN_CLAIMS:
        assert hits[name] > 0, (name, hits)
    f = rs.forward(rs.data((2, h, w, 4), 1), rois, rs.ROIALIGN_SCALE, ph, pw, sampling)
    assert (f.n[-1 if (ph, pw) != (1, 1) else -2] == 0).all()                         # the ROI wholly outside: no live sample
    assert (f.n > 0).any() and (f.n < 4 * f.count[:, None, None]).any()              # cells with skipped samples
    merged = [len({t[0][1] for _, _, t in live} | {t[1][1] for _, _, t in live}) < 2 * len({ix for _, ix, _ in live})
              for roi in rois for live in rs.geometry(roi, rs.ROIALIGN_SCALE, h, w, ph, pw, sampling).cells.values() if live]
    assert sampling != 2 or any(merged)                                                # two samples of a cell share a pixel column
    if sampling == 0:
        grids = {(g.gh, g.gw) for g in (rs.geometry(r, rs.ROIALIGN_SCALE, h, w, ph, pw, 0) for r in rois)}
        assert (4, 4) in grids and (1, 1) in grids


@pytest.mark.parametrize("sampling", [2, 0])
def test_exact_pooler_cases_are_exact_routed_as_built_and_hit_every_threshold(sampling):
    boxes, counts, want = rs.exact_pool_boxes(sampling)
    lv = rs.levels_of(boxes, counts)
    np.testing.assert_array_equal(lv, want)
    assert boxes.shape[0] * boxes.shape[1] <= 24 and all(h <= 16 and w <= 16 for h, w in rs.POOL_SIZES)
    grids = set()
    per_level = {}
    for l, box in zip(lv, boxes.reshape(-1, 4)):
        if l < 0:
            continue
        roi = np.concatenate([[0], box])
        (h, w), sc = rs.POOL_SIZES[l], rs.POOL_SCALES[l]
        assert rs.is_exact(roi, sc, h, w, rs.POOL, rs.POOL, sampling), (l, box)
        g = rs.geometry(roi, sc, h, w, rs.POOL, rs.POOL, sampling)
        grids.add((g.gh, g.gw))
        per_level[l] = rs.add_hits(per_level.get(l, dict.fromkeys(rs.HIT_NAMES, 0)), rs.threshold_hits([roi], sc, h, w, rs.POOL, rs.POOL, sampling))
    for l in range(5):
        print("pooler level %d sampling %d:" % (l, sampling), per_level[l])
        for name in ("on_minus_one", "on_size", "outside", "on_last"):          # on every level
            assert per_level[l][name] > 0, (l, name, per_level[l])
    hits, _ = rs.pool_hits(boxes, counts, rs.POOL, sampling)
    assert all(hits[name] > 0 for name in rs.HIT_NAMES), hits
    if sampling == 0:        # the general branch of the pooler kernels (a grid above 2 x 2) and their merged branch
        assert any(gh > 2 or gw > 2 for gh, gw in grids) and any(gh <= 2 and gw <= 2 for gh, gw in grids), grids
    else:
        assert grids == {(2, 2)}
    assert np.array_equal(boxes[0, 0], boxes[0, 1])                              # duplicates: the atomics accumulate


def test_exact_query_boxes_are_exact_at_every_scale():
    for shots in (1, 3):
        for sampling in (2, 0):
            rois = rs.exact_query_rois(shots, sampling)
            for (h, w), sc in zip(rs.QUERY_SIZES, rs.POOL_SCALES):
                for roi in rois:
                    assert rs.is_exact(roi, sc, h, w, 1, 1, sampling), (roi, sc, sampling)
    hits = dict.fromkeys(rs.HIT_NAMES, 0)
    for (h, w), sc in zip(rs.QUERY_SIZES, rs.POOL_SCALES):
        hits = rs.add_hits(hits, rs.threshold_hits(rs.exact_query_rois(3), sc, h, w, 1, 1, 2))
    print("query boxes, sampling 2:", hits)
    assert hits["on_last"] > 0 and hits["on_pixel"] > 0
    assert np.array_equal(rs.exact_query_rois(3)[1], rs.exact_query_rois(3)[2])


def test_random_cases_keep_their_distance_from_the_thresholds():
    boxes = rs.random_pool_boxes(rs.RANDOM_SEED)
    assert set(rs.levels_of(boxes).tolist()) == {0, 1, 2, 3, 4}
    _, h, w = rs.ROIALIGN_MAP
    for sampling in (2, 0):
        hits, dist = rs.pool_hits(boxes, None, rs.POOL, sampling)
        print("random pooler boxes, sampling %d: distance %.2e" % (sampling, dist), hits)
        assert dist >= 1e-3 and hits["outside"] > 0 and hits["on_last"] > 0
        for ph, pw in rs.ROIALIGN_POOLS:
            rois = rs.random_rois(rs.RANDOM_SEED)
            dist = rs.min_threshold_distance(rois, rs.ROIALIGN_SCALE, h, w, ph, pw, sampling)
            hits = rs.threshold_hits(rois, rs.ROIALIGN_SCALE, h, w, ph, pw, sampling)
            print("random ROIs %dx%d sampling %d: distance %.2e" % (ph, pw, sampling, dist), hits)
            assert dist >= 1e-3 and hits["outside"] > 0


def test_routing_boxes_sit_on_the_level_thresholds():
    b = rs.routing_boxes()[0]
    side = np.sqrt((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1))
    assert side[:10].tolist() == [v for s in rs.ROUTING_SIDES for v in (s, s - 1)]
    assert rs.levels_of(rs.routing_boxes()).tolist() == [0, 0, 1, 0, 2, 1, 3, 2, 4, 3, 0, 4]
    # every one of them reaches its level's map: the backward test needs a non-zero gradient there
    f, lv = rs.pool_levels(rs.pool_feats(8, 50, images=1), rs.POOL_SCALES, rs.routing_boxes(), None, rs.POOL, 2)
    assert (f.n.reshape(12, -1).sum(1) > 0).all()
