"""CPU: the second stage with linear_fusion=True (FEW_SHOT.LINEAR_FUSION: one 3x3 conv over cat(x, query), GroupNorm, LeakyReLU in
front of fc6; no compress_dim_conv).  spec's key list against the shapes recorded from the REAL reference model, the refusal of a
state_dict trained with the other setting, the checkpoint field, and the restatement tests/box_linear_fusion_ref.py against the
fixtures tests/golden/make_golden_linear_fusion.py recorded through the reference.

Tolerances: those tests/test_oracle_golden.py holds for the same comparisons of the default head (the oracle's backbone on another
host CPU supplies the features): pooled maps 1e-4, logits / deltas rtol 1e-3 atol 5e-4, losses rtol 1e-3, parameter-gradient samples
2e-3 of the tensor's largest entry; the split form against the concatenated one 1e-12 in float64 (it is exact up to summation order)."""
import os

import numpy as np
import pytest
import torch

from fake_engine import FakeEngine
import box_linear_fusion_ref as blf
import golden_utils as gu
from oneshotdet_amd import checkpoint, spec, synth
from oracle import box_train_ref as obt
from oracle import hotpath_ref as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = "roi_heads.box."


@pytest.fixture(scope="module")
def sd_linear():
    return orc.to_torch_state_dict(synth.make_state_dict(spec.full_model_shapes(linear_fusion=True)))


def test_shapes_equal_the_recorded_reference_model():
    f = gu.load("box_small_linear.npz")
    mine = spec.box_head_shapes(linear_fusion=True)
    assert list(mine.keys()) == [str(k) for k in f["ref_shapes.names"]]
    for (k, s), dims in zip(mine.items(), f["ref_shapes.dims"]):
        assert tuple(s) == tuple(int(d) for d in dims[:len(s)]) and not dims[len(s):].any(), k
    assert mine[P + "feature_aggreg.0.weight"] == (128, 512, 3, 3) and not any("compress_dim_conv" in k for k in mine)
    full = spec.full_model_shapes(linear_fusion=True)
    assert [k for k in full if k.startswith(P)] == list(mine.keys())
    assert [k for k in full if not k.startswith(P)] == list(spec.hot_path_shapes().keys())


def test_default_shapes_are_unchanged():
    import json
    ref = json.load(open(os.path.join(gu.GOLDEN_DIR, "state_dict_keys.json")))
    for mine in (spec.box_head_shapes(), spec.box_head_shapes(linear_fusion=False)):
        assert list(mine.keys()) == list(ref["box_head_shapes"].keys())
        assert all(list(s) == ref["box_head_shapes"][k] for k, s in mine.items())
    assert spec.LINEAR_FUSION is False and spec.full_model_shapes() == spec.full_model_shapes(linear_fusion=False)


def test_a_state_dict_of_the_other_setting_is_refused_by_name():
    lin = {k: torch.zeros(s) for k, s in spec.box_head_shapes(linear_fusion=True).items()}
    std = {k: torch.zeros(s) for k, s in spec.box_head_shapes().items()}
    assert spec.check_linear_fusion(lin, True) is True and spec.check_linear_fusion(std, False) is False
    assert spec.check_linear_fusion(std) is False
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION True.*linear_fusion=True"):
        spec.check_linear_fusion(lin, False)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION False.*linear_fusion=False"):
        spec.check_linear_fusion(std, True)
    mixed = dict(lin)
    mixed[P + "compress_dim_conv.0.weight"] = torch.zeros(512, 512, 1, 1)
    for want in (True, False):
        with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION"):
            spec.check_linear_fusion(mixed, want)
    # the packer refuses before it packs (nothing here touches a GPU), never with a KeyError on compress_dim_conv
    from oneshotdet_amd.box_head import BoxHeadWeights
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION True"):
        BoxHeadWeights(lin, torch.float32)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION False"):
        BoxHeadWeights(std, torch.float32, linear_fusion=True)


def test_checkpoint_round_trip_and_resume_refusal(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.full_model_shapes(linear_fusion=True)).items()}
    p = str(tmp_path / "model_0000010.pth")
    checkpoint.save_training_checkpoint(p, FakeEngine(sd, linear_fusion=True), 10)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert raw["linear_fusion"] is True and not any("compress_dim_conv" in k for k in raw["model"])
    back, extras = checkpoint.load_checkpoint(p, linear_fusion=True)
    assert list(back.keys()) == list(spec.full_model_shapes(linear_fusion=True).keys()) and extras["linear_fusion"] is True
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION True.*linear_fusion=True"):       # not "lacks 8 expected entries"
        checkpoint.load_checkpoint(p)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION True"):
        checkpoint.load_checkpoint(p, second_stage=True, defaults=synth.make_state_dict(spec.full_model_shapes()))
    # a DataParallel file (module. prefix) is recognised too
    p3 = checkpoint.save_checkpoint(str(tmp_path / "dp.pth"), {"module." + k: v for k, v in sd.items()}, tag_last=False)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION True"):
        checkpoint.load_checkpoint(p3)
    assert list(checkpoint.load_checkpoint(p3, linear_fusion=True)[0].keys()) == list(back.keys())
    eng, it = checkpoint.resume_training(p, lambda s: FakeEngine(s, linear_fusion=True), linear_fusion=True)
    assert it == 10 and eng.opt_state["steps"] == 3
    checkpoint.resume_training(p, lambda s: FakeEngine(s, linear_fusion=True))          # the caller need not say it: the file does
    called = []
    with pytest.raises(ValueError) as e:                                   # refused before make_engine, naming both values
        checkpoint.resume_training(p, lambda s: called.append(1), linear_fusion=False)
    assert "linear_fusion=True" in str(e.value) and "linear_fusion=False" in str(e.value) and not called
    with pytest.raises(ValueError, match="make_engine built an engine with linear_fusion=False"):
        checkpoint.resume_training(p, lambda s: FakeEngine(s))
    # the default model: the field is recorded as False, a file without it means False, and loads as before
    sd2 = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.full_model_shapes()).items()}
    p2 = str(tmp_path / "model_old.pth")
    checkpoint.save_training_checkpoint(p2, FakeEngine(sd2), 7)
    raw2 = torch.load(p2, map_location="cpu", weights_only=False)
    assert raw2["linear_fusion"] is False
    del raw2["linear_fusion"]
    torch.save(raw2, p2)
    eng, it = checkpoint.resume_training(p2, lambda s: FakeEngine(s), linear_fusion=False)
    assert it == 7 and list(eng.sd.keys()) == list(spec.full_model_shapes().keys())
    with pytest.raises(ValueError, match="linear_fusion=False.*linear_fusion=True"):
        checkpoint.resume_training(p2, lambda s: FakeEngine(s, linear_fusion=True), linear_fusion=True)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION False.*linear_fusion=False"):
        checkpoint.load_checkpoint(p2, linear_fusion=True)


def test_c2_loader_takes_the_option(tmp_path):
    import pickle
    lin = synth.make_state_dict(spec.full_model_shapes(linear_fusion=True))
    p = str(tmp_path / "r50.pkl")           # the option is checked on `defaults` before the file's blobs are looked at
    with open(p, "wb") as f:
        pickle.dump({"blobs": {}}, f)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION True"):
        checkpoint.load_c2_resnet(p, lin)
    with pytest.raises(ValueError, match=r"FEW_SHOT\.LINEAR_FUSION False"):
        checkpoint.load_c2_resnet(p, synth.make_state_dict(spec.full_model_shapes()), linear_fusion=True)


def test_split_form_equals_the_concatenated_conv():
    """conv3x3(cat(x, q)) = W_x * x + (W_q * q + b) with zero padding on both halves: what the engines compute."""
    g = torch.Generator().manual_seed(0)
    sd = {P + "feature_aggreg.0.weight": torch.randn(128, 512, 3, 3, generator=g, dtype=torch.float64) * 0.05,
          P + "feature_aggreg.0.bias": torch.randn(128, generator=g, dtype=torch.float64),
          P + "feature_aggreg.1.weight": torch.rand(128, generator=g, dtype=torch.float64) + 0.5,
          P + "feature_aggreg.1.bias": torch.randn(128, generator=g, dtype=torch.float64)}
    x = torch.randn(7, 256, 7, 7, generator=g, dtype=torch.float64) + 3
    q = torch.randn(3, 256, 7, 7, generator=g, dtype=torch.float64) + 3
    img = torch.tensor([0, 0, 0, 1, 1, 1, 2])
    a = blf.fuse(x, q[img], sd)
    b = blf.fuse_split(x, q, img, sd)
    assert (a - b).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", ["small", "nonsquare", "shots5"])
def test_restatement_reproduces_the_inference_fixture(name, sd_linear):
    f = gu.load("box_%s_linear.npz" % name)
    B, H, W, S, qh, qw = gu.CASES[name]
    assert int(f["n_shots_outputs"]) == S
    img, q = gu.case_inputs(name)
    with torch.no_grad():
        o = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(q), sd_linear, shots=S)
        props = [torch.from_numpy(f["proposals.%d.boxes" % i]) for i in range(B)]
        r = blf.box_head_forward(o["features"], o["query_features"], props, [(H, W)] * B, [(qh, qw)] * (B * S), sd_linear)
        r64 = blf.box_head_logits(o["features"], o["query_features"], props, [(qh, qw)] * (B * S), sd_linear, double=True)
    R = len(props[0])
    gu.check_against(r["pooled"].reshape(B * R, -1, 7, 7).numpy(), f, "pooled", 1e-4, 1e-4)
    np.testing.assert_allclose(r["logits"].numpy(), f["logits"], rtol=1e-3, atol=5e-4)
    np.testing.assert_allclose(r["box_regression"].numpy(), f["box_regression"], rtol=1e-3, atol=5e-4)
    assert r64[0].dtype == torch.float64
    if S == 1:          # with several shots a near-tie of two shots' logits may pick the other shot's row in float64
        np.testing.assert_allclose(r64[0].numpy(), f["logits"], rtol=1e-3, atol=5e-4)
        np.testing.assert_allclose(r64[1].numpy(), f["box_regression"], rtol=1e-3, atol=5e-4)
    for i in range(B):
        db, ds = r["detections"][i]
        assert abs(len(db) - len(f["detections.%d.boxes" % i])) <= 1
        assert gu.match_boxes(f["detections.%d.boxes" % i], f["detections.%d.scores" % i], db.numpy(), ds.numpy()) >= 0.99
    # the fixture is not the default head's: the two models' logits differ by far more than the bound
    default = gu.load("box_%s.npz" % name)["logits"]
    assert default.shape != f["logits"].shape or np.abs(f["logits"] - default).max() > 0.05


@pytest.mark.parametrize("name", ["small", "nonsquare"])
def test_restatement_reproduces_the_training_fixture(name, sd_linear):
    f = gu.load("boxtrain_%s_linear.npz" % name)
    B, H, W, S, qh, qw = gu.CASES[name]
    n_props = [int(v) for v in f["n_props"]]
    keys = synth.uniform01("boxtrain.keys." + name, B * max(n_props), seed=9).reshape(B, max(n_props)).astype(np.float32)
    img, q = gu.case_inputs(name)
    with torch.no_grad():
        o = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(q), sd_linear, shots=S)
    sd = {k: (v.clone().requires_grad_(True) if k.startswith(P) else v) for k, v in sd_linear.items()}
    samp = [obt.subsample(torch.from_numpy(f["props.%d" % i]), torch.from_numpy(f["gt.%d" % i]),
                          torch.from_numpy(keys[i, :n_props[i]].copy())) for i in range(B)]
    for i in range(B):
        assert np.array_equal(samp[i]["index"].numpy(), f["index.%d" % i]) and np.array_equal(samp[i]["labels"].numpy(), f["labels.%d" % i])
    lc, lb, _, _ = blf.box_train_forward(o["features"], o["query_features"], samp, [(qh, qw)] * (B * S), sd, shots=S)
    np.testing.assert_allclose([lc.item(), lb.item()], f["losses"], rtol=1e-3)
    with torch.no_grad():
        lc64, lb64, _, _ = blf.box_train_forward(o["features"], o["query_features"], samp, [(qh, qw)] * (B * S), sd_linear, shots=S,
                                                 double=True)
    assert lc64.dtype == torch.float64
    np.testing.assert_allclose([lc64.item(), lb64.item()], f["losses"], rtol=1e-3)
    (lc + lb).backward()
    checked = 0
    for key in f.files:
        if key.startswith("refgrad.") and key.endswith(".samples"):
            k = key[len("refgrad."):-len(".samples")]
            assert "compress_dim_conv" not in k
            g = sd[k].grad.numpy().reshape(-1)
            idx = gu.sample_indices(g.size, "boxgrad." + k)[:256]
            assert np.abs(g[idx] - f[key]).max() <= 2e-3 * float(f["refgrad.%s.absmax" % k]), k
            checked += 1
    assert checked == 12


def test_documents_describe_the_option():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "linear_fusion" in open(os.path.join(ROOT, doc)).read(), doc
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "LINEAR_FUSION" in integ
    sentence = integ[integ.index("Still refused by name"):]
    sentence = sentence[:sentence.index("\n\n")]
    for word in ("LOSS_WEIGHTED", "NEG_SUPPORT", "SECOND_STAGE_METHOD", "'rn'", "'matching'", "REVERSE_ORDER", "SUPP_AUG"):
        assert word in sentence, word
    assert "LINEAR_FUSION" not in sentence


def test_examples_take_the_flag():
    for ex in ("train.py", "detect.py"):
        text = open(os.path.join(ROOT, "examples", ex)).read()
        assert "--linear-fusion" in text and "linear_fusion=args.linear_fusion" in text, ex
