"""GPU (-m gpu): the second-stage few-shot ROI box head on the HIP path against the oracle
(oracle/box_head_ref.py) and against the fixtures recorded from the REAL reference's `model.roi_heads`
(tests/golden/box_*.npz, tests/golden/make_golden.py gen_box_case).

Tolerances: fp32 path logits / box deltas atol 1e-3 (BASELINE.json "within 1e-3 fp32"), pooled ROI maps 1e-3 of the
tensor's largest entry; detections: >= 99 % of the reference's (box, score) rows found (a 1e-6 score difference can flip
an NMS tie).  bf16 path: logits atol 0.06, deltas atol 0.03 (8-bit mantissas through the backbone and six more layers).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_utils as gu
from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    from oneshotdet_amd import model
    np_sd = synth.make_state_dict(spec.full_model_shapes())
    return {"f32": model.HotPathEngine(np_sd, dtype=torch.float32),
            "bf16": model.HotPathEngine(np_sd, dtype=torch.bfloat16)}


@pytest.fixture(scope="module")
def sd_full():
    from oracle import hotpath_ref as orc
    return orc.to_torch_state_dict(synth.make_state_dict(spec.full_model_shapes()))


def nchw(t):
    from oneshotdet_amd import ops
    return ops.nhwc_to_nchw_f32(t).cpu()


def fixture_proposals(f, B):
    return torch.stack([torch.from_numpy(f["proposals.%d.boxes" % i]) for i in range(B)], 0).cuda()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_roi_pool_levels_matches_oracle(dt):
    """Level routing bit-exact (int), pooled values against the oracle's Pooler on the same maps; boxes straddling the
    level boundaries, leaving the image, degenerate; ROIs past the per-image count give zero rows."""
    from oneshotdet_amd import ops
    from oracle import box_head_ref as obh
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(11)
    B, C = 2, 64
    sizes = [(40, 48), (20, 24), (10, 12), (5, 6), (3, 3)]
    feats = [torch.randn(B, C, h, w, generator=g) for h, w in sizes]
    if dt == "bf16":
        feats = [f.bfloat16().float() for f in feats]
    R = 37
    xy = torch.rand(B, R, 2, generator=g) * torch.tensor([300.0, 250.0])
    wh = torch.exp(torch.rand(B, R, 2, generator=g) * 6.5)           # 1 .. 665 px: all five levels
    boxes = torch.cat([xy, xy + wh], -1)
    boxes[0, 0] = torch.tensor([0.0, 0.0, 223.0, 223.0])             # sqrt(area) = 224 exactly -> level 4
    boxes[0, 1] = torch.tensor([0.0, 0.0, 222.0, 222.0])
    boxes[0, 2] = torch.tensor([-50.0, -30.0, 20.0, 10.0])
    boxes[0, 3] = torch.tensor([100.0, 100.0, 100.0, 100.0])
    boxes[1, 0] = torch.tensor([380.0, 310.0, 900.0, 700.0])         # outside the maps
    counts = torch.tensor([R, R - 5], dtype=torch.int32)
    dev = [f.permute(0, 2, 3, 1).contiguous().to("cuda", dtype) for f in feats]
    y, lv = ops.roi_pool_levels(dev, spec.POOLER_SCALES, boxes.cuda(), counts.cuda(), 7, 2, want_levels=True)
    ref = obh.pooler(feats, [boxes[0], boxes[1]]).reshape(B * R, C, 7, 7)
    ref_lv = obh.map_levels(boxes.reshape(-1, 4)).to(torch.int32)
    ref_lv[R + R - 5:] = -1
    ref[R + R - 5:] = 0
    assert torch.equal(lv.cpu(), ref_lv)
    got = y.float().cpu().permute(0, 3, 1, 2)
    tol = 1e-5 if dt == "f32" else 2e-2
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=tol, atol=tol)
    if dt == "bf16":         # fp32 arithmetic and one bf16 rounding: within one bf16 ulp of the rounded oracle value, <= 2 % flips
        from oracle import launch_replay as lr
        res = lr.compare(got, ref, dtype)
        assert res["ok"] and res["flips"] <= 0.02, res


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [128, 256, 512])
def test_groupnorm_leaky_rois_matches_aten(dt, c):
    from oneshotdet_amd import ops
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    g = torch.Generator().manual_seed(c)
    R, per, shots = 23, 5, 2                        # 5 ROIs per image, 2 addend maps per image: pick shot 1
    x = (torch.randn(R, 7, 7, c, generator=g) * 2 + 0.5).to(dtype)
    add = torch.randn((R + per - 1) // per * shots, 7, 7, c, generator=g).to(dtype)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    y = ops.groupnorm_act_rois(x.cuda(), gamma.cuda(), beta.cuda(), 32, 1e-5, 0.2, addend=add.cuda(), rois_per_add=per,
                               add_stride=shots, add_offset=1)
    idx = torch.arange(R) // per * shots + 1
    xin = (x.float() + add.float()[idx]).permute(0, 3, 1, 2)
    ref = F.leaky_relu(F.group_norm(xin, 32, gamma, beta, 1e-5), 0.2).permute(0, 2, 3, 1)
    tol = 2e-5 if dt == "f32" else 3e-2
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), rtol=tol, atol=tol)
    # no addend, in place, slope 0 = ReLU; a constant map (variance 0) stays finite
    x2 = x.clone()
    x2[3] = 1.25
    y2 = ops.groupnorm_act_rois(x2.cuda(), gamma.cuda(), beta.cuda(), 32, 1e-5, 0.0)
    ref2 = F.relu(F.group_norm(x2.float().permute(0, 3, 1, 2), 32, gamma, beta, 1e-5)).permute(0, 2, 3, 1)
    np.testing.assert_allclose(y2.float().cpu().numpy(), ref2.numpy(), rtol=tol, atol=tol)
    assert torch.isfinite(y2).all()


@pytest.mark.parametrize("shots", [1, 3])
def test_box_decode_matches_oracle(shots):
    from oneshotdet_amd import ops
    from oracle import box_head_ref as obh
    g = torch.Generator().manual_seed(3 + shots)
    N, R = 2, 50
    pred = torch.randn(shots, N * R, 12, generator=g)
    pred[:, :, 2:10] *= 3.0
    pred[0, 5, 8] = 60.0                                 # dw / 5 beyond log(1000/16): clamped
    xy = torch.rand(N, R, 2, generator=g) * 200
    rois = torch.cat([xy, xy + torch.rand(N, R, 2, generator=g) * 150 + 1], -1)
    counts = torch.tensor([R, 31], dtype=torch.int32)
    scores, boxes, lo, ro = ops.box_decode(pred.cuda(), rois.cuda(), counts.cuda(), spec.BOX_REG_WEIGHTS, 240, 320, 0.0,
                                           want_raw=True)
    tl, tr = pred[:, :, :2], pred[:, :, 2:10]
    idx = torch.argmax(tl, dim=0)
    logits = torch.gather(tl, 0, idx.unsqueeze(0))[0]
    reg = torch.gather(tr, 0, idx[:, :, None].expand(-1, -1, 4).reshape(N * R, 8).unsqueeze(0))[0]
    assert torch.equal(lo.cpu(), logits) and torch.equal(ro.cpu(), reg)
    prob = F.softmax(logits, -1)[:, 1].reshape(N, R)
    dec = obh.decode_boxes(reg, rois.reshape(-1, 4))[:, 4:8].reshape(N, R, 4).clone()
    dec[..., 0::2] = dec[..., 0::2].clamp(0, 319)
    dec[..., 1::2] = dec[..., 1::2].clamp(0, 239)
    prob[1, 31:] = -1
    np.testing.assert_allclose(scores.cpu().numpy(), prob.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(boxes.cpu().numpy(), dec.numpy(), rtol=1e-5, atol=2e-3)


@pytest.mark.parametrize("name", ["small", "nonsquare", "shots5", "tall", "config1"])
def test_fp32_box_head_matches_reference_golden(name, engines):
    """The reference's own proposals (fixture) through OUR backbone features and OUR box head."""
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    f = gu.load("box_%s.npz" % name)
    eng = engines["f32"]
    feats, qfeats, _, _ = eng.forward_features(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda())
    props = fixture_proposals(f, B)
    out = eng.box_detect(feats, qfeats, (qh, qw), props, None, H, W, shots=S, cuda_nms=False, want_raw=True)
    R = props.shape[1]
    gu.check_against(nchw(out["pooled"]).numpy(), f, "pooled", 1e-3, 1e-3)
    gu.check_against(nchw(out["query_roi"]).numpy(), f, "supp_roi", 1e-3, 1e-3)
    np.testing.assert_allclose(out["logits"].cpu().numpy(), f["logits"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(out["box_regression"].cpu().numpy(), f["box_regression"], rtol=1e-3, atol=1e-3)
    for i in range(B):
        k = int(out["counts"][i])
        rb, rs = f["detections.%d.boxes" % i], f["detections.%d.scores" % i]
        assert abs(k - len(rb)) <= max(1, len(rb) // 100), (k, len(rb))
        got_b, got_s = out["boxes"][i, :k].cpu().numpy(), out["scores"][i, :k].cpu().numpy()
        assert np.all(got_s[:-1] >= got_s[1:])
        assert gu.match_boxes(rb, rs, got_b, got_s) >= 0.99


@pytest.mark.parametrize("name", ["small", "shots5", "config1"])
def test_bf16_box_head_close_to_reference_golden(name, engines):
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    f = gu.load("box_%s.npz" % name)
    eng = engines["bf16"]
    feats, qfeats, _, _ = eng.forward_features(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda())
    out = eng.box_detect(feats, qfeats, (qh, qw), fixture_proposals(f, B), None, H, W, shots=S, want_raw=True)
    gu.check_against(nchw(out["pooled"]).numpy(), f, "pooled", 3e-2, 5e-2)
    np.testing.assert_allclose(out["logits"].cpu().numpy(), f["logits"], rtol=0, atol=0.06)
    d = np.abs(out["box_regression"].cpu().numpy() - f["box_regression"])
    if S == 1:
        assert d.max() <= 0.03
    else:
        # the deltas come from the shot with the largest class logit (box_head.py:239-252): where two shots' logits are
        # within bf16 noise of each other the arg-max, and with it the whole delta row, legitimately switches
        assert (d > 0.03).mean() <= 0.05 and d.max() <= 0.5


def test_ragged_counts_and_batch_invariance(engines):
    """What the reference cannot run (poolers.py:80 asserts equal counts): images with different numbers of proposals.
    Every image's detections equal those of a single-image call with just its own proposals, bit for bit."""
    name = "nonsquare"
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    f = gu.load("box_%s.npz" % name)
    eng = engines["f32"]
    images, queries = torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda()
    feats, qfeats, _, _ = eng.forward_features(images, queries)
    props = fixture_proposals(f, B)
    counts = torch.tensor([props.shape[1], 97], dtype=torch.int32).cuda()
    out = eng.box_detect(feats, qfeats, (qh, qw), props, counts, H, W, cuda_nms=False)
    for i in range(B):
        fi, qi, _, _ = eng.forward_features(images[i:i + 1], queries[i:i + 1])
        c = int(counts[i])
        one = eng.box_detect(fi, qi, (qh, qw), props[i:i + 1, :c].contiguous(), None, H, W, cuda_nms=False)
        k = int(one["counts"][0])
        assert int(out["counts"][i]) == k
        assert torch.equal(out["boxes"][i, :k], one["boxes"][0, :k]) and torch.equal(out["scores"][i, :k], one["scores"][0, :k])


def test_end_to_end_detect_with_second_stage(engines):
    """images -> first stage (our proposals) -> second stage, config1: the detections overlap the reference's, which ran
    on the reference's own proposals (the two proposal sets agree to >= 99 %, tests/test_gpu_parity.py)."""
    B, H, W, S, qh, qw = gu.CASES["config1"]
    img, q = gu.case_inputs("config1")
    f = gu.load("box_config1.npz")
    out = engines["f32"].detect(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), cuda_nms=False,
                                second_stage=True)
    det = out["detections"]
    k = int(det["counts"][0])
    rb, rs = f["detections.0.boxes"], f["detections.0.scores"]
    assert abs(k - len(rb)) <= len(rb) // 50
    assert gu.match_boxes(rb, rs, det["boxes"][0, :k].cpu().numpy(), det["scores"][0, :k].cpu().numpy()) >= 0.97


def test_full_size_batch8_second_stage_properties(engines):
    """BASELINE.json configs[1] size (8 x 800x1024, 2000 proposals each) in bf16: identical images give bit-identical
    detections, scores sorted, boxes inside the image, NMS idempotent."""
    from oneshotdet_amd import layers
    eng = engines["bf16"]
    img, q = gu.case_inputs("config1")
    images = torch.from_numpy(img).cuda().expand(8, -1, -1, -1).contiguous()
    queries = torch.from_numpy(q).cuda().expand(8, -1, -1, -1).contiguous()
    det = eng.detect(images, queries, second_stage=True)["detections"]
    k = int(det["counts"][0])
    assert k > 100
    for i in range(1, 8):
        assert int(det["counts"][i]) == k and torch.equal(det["boxes"][i, :k], det["boxes"][0, :k])
        assert torch.equal(det["scores"][i, :k], det["scores"][0, :k])
    s, b = det["scores"][0, :k], det["boxes"][0, :k]
    assert torch.all(s[:-1] >= s[1:]) and s.min() > 0 and s.max() <= 1
    assert b.min() >= 0 and b[:, 2].max() <= 1023 and b[:, 3].max() <= 799
    assert layers.nms(b, s, spec.BOX_NMS_THRESH).numel() == k


def test_checkpoint_round_trip_through_the_engines(tmp_path, engines):
    """TrainEngine.state_dict() -> reference-format .pth -> HotPathEngine: the reloaded engine reproduces the outputs
    bit for bit (oneshotdet_amd/checkpoint.py; utils/checkpoint.py:33-103)."""
    from oneshotdet_amd import checkpoint, model, train
    np_sd = synth.make_state_dict(spec.full_model_shapes())
    tr = train.TrainEngine({k: v for k, v in np_sd.items() if k in spec.hot_path_shapes()}, dtype=torch.float32)
    sd = dict(tr.state_dict())
    sd.update({k: torch.from_numpy(v) for k, v in np_sd.items() if k.startswith("roi_heads.")})
    p = checkpoint.save_checkpoint(str(tmp_path / "model_0000001.pth"), {"module." + k: v for k, v in sd.items()},
                                   iteration=1)
    loaded, extras = checkpoint.load_checkpoint(p)
    assert extras["iteration"] == 1 and list(loaded.keys()) == list(spec.full_model_shapes().keys())
    eng = model.HotPathEngine(loaded, dtype=torch.float32)
    img, q = gu.case_inputs("small")
    a = eng.detect(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), second_stage=True)
    b = engines["f32"].detect(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), second_stage=True)
    k = int(b["detections"]["counts"][0])
    assert int(a["detections"]["counts"][0]) == k and k > 0
    assert torch.equal(a["detections"]["boxes"][0, :k], b["detections"]["boxes"][0, :k])
    assert torch.equal(a["detections"]["scores"][0, :k], b["detections"]["scores"][0, :k])


def test_ragged_batch_of_lists_matches_reference_golden(engines):
    """R0 (to_image_list on lists, structures/image_list.py:52-70): different-size targets and queries are zero-padded
    to a common /32 size by layers.to_image_list; every image is clipped to ITS size, every query's whole-image ROI box
    uses ITS size (pooling and second-stage level routing).  Fixture recorded through the real reference."""
    from oneshotdet_amd import layers
    f = gu.load("case_ragged.npz")
    t_np, q_np = gu.ragged_inputs()
    imgs = layers.to_image_list([torch.from_numpy(a).cuda() for a in t_np], gu.RAGGED["size_divisible"])
    qs = layers.to_image_list([torch.from_numpy(a).cuda() for a in q_np], gu.RAGGED["size_divisible"])
    assert tuple(imgs.tensors.shape) == tuple(f["padded_target"]) and imgs.image_sizes == gu.RAGGED["targets"]
    assert tuple(qs.tensors.shape) == tuple(f["padded_query"]) and qs.image_sizes == gu.RAGGED["queries"]
    eng = engines["f32"]
    out = eng.detect(imgs, qs, cuda_nms=False, second_stage=True)
    logits = [nchw(c)[:, 0:1].numpy() for c, _ in out["head"]]
    ctr = [nchw(c)[:, 1:2].numpy() for c, _ in out["head"]]
    reg = [nchw(r).numpy() for _, r in out["head"]]
    np.testing.assert_allclose(gu.flatten_head(logits, reg, ctr), f["head"], rtol=1e-3, atol=1e-3)
    for lvl in range(5):
        np.testing.assert_allclose(out["pooled"][lvl].cpu().numpy(), f["pooled.%d" % lvl], rtol=1e-4, atol=1e-4)
    ob, os_, oc = out["proposals"]
    for i, (h, w) in enumerate(gu.RAGGED["targets"]):
        k = int(oc[i])
        b = ob[i, :k]
        assert float(b[:, 2].max()) <= w - 1 and float(b[:, 3].max()) <= h - 1 and float(b.min()) >= 0
        rb, rs = f["proposals.%d.boxes" % i], f["proposals.%d.scores" % i]
        assert abs(k - len(rb)) <= 2
        assert gu.match_boxes(rb, rs, b.cpu().numpy(), os_[i, :k].cpu().numpy()) >= 0.99
    # second stage on the reference's own (equal-count) proposals
    props = torch.stack([torch.from_numpy(f["box.proposals.%d" % i]) for i in range(2)], 0).cuda()
    det = eng.box_detect(out["features"], out["query_features"], qs.image_sizes, props, None, 128, 160, cuda_nms=False,
                         want_raw=True, image_sizes=imgs.image_sizes)
    np.testing.assert_allclose(det["logits"].cpu().numpy(), f["box.logits"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(det["box_regression"].cpu().numpy(), f["box.box_regression"], rtol=1e-3, atol=1e-3)
    for i, (h, w) in enumerate(gu.RAGGED["targets"]):
        k = int(det["counts"][i])
        b = det["boxes"][i, :k]
        assert float(b[:, 2].max()) <= w - 1 and float(b[:, 3].max()) <= h - 1
        rb, rs = f["box.detections.%d.boxes" % i], f["box.detections.%d.scores" % i]
        assert abs(k - len(rb)) <= max(1, len(rb) // 100)
        assert gu.match_boxes(rb, rs, b.cpu().numpy(), det["scores"][i, :k].cpu().numpy()) >= 0.99
    # the end-to-end second stage (our proposals, ragged counts) is well formed
    d2 = out["detections"]
    for i, (h, w) in enumerate(gu.RAGGED["targets"]):
        k = int(d2["counts"][i])
        assert k > 0 and float(d2["boxes"][i, :k, 2].max()) <= w - 1 and float(d2["boxes"][i, :k, 3].max()) <= h - 1
