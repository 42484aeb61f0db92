"""GPU (-m gpu): the engines with linear_fusion=True (FEW_SHOT.LINEAR_FUSION) against the fixtures recorded through the REAL
reference (tests/golden/box_*_linear.npz, boxtrain_*_linear.npz; tests/golden/make_golden_linear_fusion.py).  Both dtypes run the
split 3x3 conv (ROI half once for all shots, query half once per query map) + groupnorm_act_rois with the query map as addend.

Tolerances: those tests/test_gpu_box_head.py and tests/test_gpu_box_train.py hold for the same quantities of the default head —
fp32 logits / deltas 1e-3, bf16 logits 0.06 and deltas 0.03 (several shots: the arg-max over shots may switch rows, as there);
fp32 losses rtol 1e-4, parameter gradients 1e-3 x absmax, feature-gradient maps 5e-3 x absmax with cosine >= 0.9999; bf16 losses rtol
3e-2, gradients relative L2 <= 0.35 and cosine >= 0.96.  Measured on an MI355X: fp32 logits 4.4e-6 / deltas 2.3e-6, bf16 logits
1.3e-2 / deltas 9.1e-3 (one shot); fp32 losses within 3e-7 relative, bf16 within 3.7e-3."""
import numpy as np
import pytest
import torch

import golden_utils as gu
from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
P = "roi_heads.box."


@pytest.fixture(scope="module")
def np_sd():
    return synth.make_state_dict(spec.full_model_shapes(linear_fusion=True))


@pytest.fixture(scope="module")
def engines(np_sd):
    from oneshotdet_amd import model
    return {dt: model.HotPathEngine(np_sd, dtype=DT[dt], linear_fusion=True) for dt in DT}


def fixture_proposals(f, B):
    return torch.stack([torch.from_numpy(f["proposals.%d.boxes" % i]) for i in range(B)], 0).cuda()


def test_engines_refuse_the_other_setting_by_name(np_sd):
    from oneshotdet_amd import model, train
    std = synth.make_state_dict(spec.full_model_shapes())
    for cls, kw in ((model.HotPathEngine, {}), (train.TrainEngine, {"second_stage": True})):
        with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION True.*linear_fusion=True"):
            cls(np_sd, dtype=torch.float32, **kw)
        with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION False.*linear_fusion=False"):
            cls(std, dtype=torch.float32, linear_fusion=True, **kw)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["small", "nonsquare", "shots5"])
def test_box_head_matches_the_reference_fixture(name, dt, engines):
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    f = gu.load("box_%s_linear.npz" % name)
    eng = engines[dt]
    assert eng.box_head is not None and eng.box_head.linear_fusion
    feats, qfeats, _, _ = eng.forward_features(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda())
    out = eng.box_detect(feats, qfeats, (qh, qw), fixture_proposals(f, B), None, H, W, shots=S, cuda_nms=False, want_raw=True)
    dl = np.abs(out["logits"].cpu().numpy() - f["logits"])
    dr = np.abs(out["box_regression"].cpu().numpy() - f["box_regression"])
    print("%s %s: logits error %.3e, deltas error %.3e" % (name, dt, dl.max(), dr.max()))
    if dt == "f32":
        np.testing.assert_allclose(out["logits"].cpu().numpy(), f["logits"], rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(out["box_regression"].cpu().numpy(), f["box_regression"], rtol=1e-3, atol=1e-3)
        for i in range(B):
            k = int(out["counts"][i])
            rb, rs = f["detections.%d.boxes" % i], f["detections.%d.scores" % i]
            assert abs(k - len(rb)) <= max(1, len(rb) // 100), (k, len(rb))
            assert gu.match_boxes(rb, rs, out["boxes"][i, :k].cpu().numpy(), out["scores"][i, :k].cpu().numpy()) >= 0.99
    else:
        assert dl.max() <= 0.06
        if S == 1:
            assert dr.max() <= 0.03
        else:       # the deltas come from the shot with the largest class logit: a near-tie legitimately switches the whole row
            assert (dr > 0.03).mean() <= 0.05 and dr.max() <= 0.5


def _train_inputs(name):
    f = gu.load("boxtrain_%s_linear.npz" % name)
    B = gu.CASES[name][0]
    n_props = [int(v) for v in f["n_props"]]
    pmax = max(n_props)
    keys = synth.uniform01("boxtrain.keys." + name, B * pmax, seed=9).reshape(B, pmax).astype(np.float32)
    props = np.zeros((B, pmax, 4), np.float32)
    G = max(len(f["gt.%d" % i]) for i in range(B))
    gt = np.zeros((B, G, 4), np.float32)
    for i in range(B):
        props[i, :n_props[i]] = f["props.%d" % i]
        gt[i, :len(f["gt.%d" % i])] = f["gt.%d" % i]
    gcnt = np.asarray([len(f["gt.%d" % i]) for i in range(B)], np.int32)
    return f, props, np.asarray(n_props, np.int32), gt, gcnt, keys


def _box_train(eng, name):
    f, props, n_props, gt, gcnt, keys = _train_inputs(name)
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    (feats, qfeats), _ = eng.backbones_forward(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda())
    eng.flat_g.zero_()
    proposals = (torch.from_numpy(props).cuda(), None, torch.from_numpy(n_props).cuda())
    out = eng.box_head_forward_backward(feats, qfeats, [(qh, qw)] * (B * S), S, proposals, torch.from_numpy(gt).cuda(),
                                        torch.from_numpy(gcnt).cuda(), keys=torch.from_numpy(keys).cuda(), want_debug=True)
    torch.cuda.synchronize()
    return f, out


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["small", "nonsquare"])
def test_box_head_training_matches_the_reference_fixture(name, dt, np_sd):
    from oneshotdet_amd import train
    B, H, W, S, qh, qw = gu.CASES[name]
    eng = train.TrainEngine(np_sd, dtype=DT[dt], second_stage=True, linear_fusion=True)
    f, (losses, gx, gqs) = _box_train(eng, name)
    for i in range(B):
        assert np.array_equal(eng.last_box["index"][i].cpu().numpy(), f["index.%d" % i])
        assert np.array_equal(eng.last_box["labels"][i].cpu().numpy(), f["labels.%d" % i])
    print("%s %s: losses %s, reference %s" % (name, dt, losses[:2].cpu().numpy(), f["losses"]))
    np.testing.assert_allclose(losses[:2].cpu().numpy(), f["losses"], rtol=1e-4 if dt == "f32" else 3e-2)
    assert int(losses[2]) == B * int(f["n_sampled"])
    grads = eng.named_grads()
    assert not any("compress_dim_conv" in k for k in grads)

    def check(got, ref, scale, what, tier=1e-3):
        err = np.abs(got - ref)
        if not ref.any():
            assert not got.any(), what
        elif dt == "f32":
            cos = float(np.dot(got, ref) / max(np.linalg.norm(got) * np.linalg.norm(ref), 1e-30))
            assert err.max() <= tier * scale and (cos >= 0.9999 or scale <= 1e-12), (what, err.max() / scale, cos)
        else:
            l2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
            cos = float(np.dot(got, ref) / max(np.linalg.norm(got) * np.linalg.norm(ref), 1e-30))
            assert l2 <= 0.35 and cos >= 0.96, (what, l2, cos)
    checked = 0
    for key in f.files:
        if key.startswith("refgrad.") and key.endswith(".samples"):
            k = key[len("refgrad."):-len(".samples")]
            g = grads[k].float().cpu().numpy().reshape(-1)
            assert k != P + "feature_aggreg.0.weight" or tuple(grads[k].shape) == (128, 512, 3, 3)
            idx = gu.sample_indices(g.size, "boxgrad." + k)[:256]
            check(g[idx], f[key], float(f["refgrad.%s.absmax" % k]), k)
            checked += 1
    assert checked == 12
    for lvl in range(5):
        tag = "oracle_only.dfeat.%d" % lvl
        got = gx[lvl].cpu().permute(0, 3, 1, 2).numpy().reshape(-1)
        check(got[gu.sample_indices(got.size, tag)], f[tag + ".samples"], max(float(f[tag + ".absmax"].max()), 1e-12), tag, tier=5e-3)
    for lvl, gq in gqs:
        tag = "oracle_only.dqfeat.%d" % lvl
        got = np.zeros(tuple(f[tag + ".shape"]), np.float32)
        got[::S] = gq.cpu().permute(0, 3, 1, 2).numpy()
        got = got.reshape(-1)
        check(got[gu.sample_indices(got.size, tag)], f[tag + ".samples"], max(float(f[tag + ".absmax"].max()), 1e-12), tag, tier=5e-3)
    others = [lv for lv in range(5) if lv not in [a for a, _ in gqs]]
    assert all(float(f["oracle_only.dqfeat.%d.absmax" % lv].max()) == 0.0 for lv in others)


def test_state_dict_save_and_resume(np_sd, tmp_path):
    """state_dict() of a trained engine has the reference's keys and shapes (ONE 512-channel feature_aggreg.0.weight whose halves are
    the two packed convs); a train_step followed by save / resume reproduces the next step's losses."""
    from oneshotdet_amd import checkpoint, train
    name = "small"
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    gtb = torch.zeros(B, max(len(g) for g in gts), 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    cnt = torch.tensor([len(g) for g in gts], dtype=torch.int32)
    args = (torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), gtb.cuda(), cnt.cuda())
    keys = torch.rand((B, spec.POST_NMS_TOP_N_TRAIN + gtb.shape[1]), generator=torch.Generator().manual_seed(0)).cuda()

    def make(sd):
        e = train.TrainEngine(sd, dtype=torch.bfloat16, second_stage=True, linear_fusion=True)
        e.box_keys = keys
        return e
    eng = make(np_sd)
    sd0 = eng.state_dict()
    shapes = spec.box_head_shapes(linear_fusion=True)
    assert [k for k in sd0 if k.startswith(P)] == list(shapes.keys())
    for key, shape in shapes.items():
        assert tuple(sd0[key].shape) == tuple(shape) and np.array_equal(sd0[key].cpu().numpy(), np_sd[key]), key
    eng.train_step(*args)
    eng.join()
    sd1 = eng.state_dict()
    wa = sd1[P + "feature_aggreg.0.weight"]
    assert tuple(wa.shape) == (128, 512, 3, 3) and (wa != sd0[P + "feature_aggreg.0.weight"]).any()
    for half, lo in (("0x", 0), ("0q", 256)):
        assert torch.equal(eng.convs[P + "feature_aggreg." + half].w.permute(0, 3, 1, 2), wa[:, lo:lo + 256])
    p = checkpoint.save_training_checkpoint(str(tmp_path / "model_0000001.pth"), eng, 1)
    eng.box_keys = keys
    eng.train_step(*args)
    eng.join()
    torch.cuda.synchronize()
    want = torch.cat([eng.box_losses[:2].float().cpu()])
    with pytest.raises(ValueError, match="linear_fusion=True"):
        checkpoint.resume_training(p, make, linear_fusion=False)
    eng2, it = checkpoint.resume_training(p, make, linear_fusion=True)
    assert it == 1 and eng2.linear_fusion
    eng2.train_step(*args)
    eng2.join()
    torch.cuda.synchronize()
    got = eng2.box_losses[:2].float().cpu()
    print("next step's box losses: %s, after save / resume %s" % (want.numpy(), got.numpy()))
    assert torch.isfinite(want).all() and float(want[0]) > 0
    torch.testing.assert_close(got, want, rtol=1e-5, atol=0)
