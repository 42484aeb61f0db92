"""CPU: the shared-backbone model (FEW_SHOT.SIAMESE_BACKBONE False: the query goes through the target's `backbone`,
generalized_rcnn.py:274-275) — its key set, the oracle with the query backbone TIED to the target's against the fixtures
recorded from the real reference (tests/golden/make_golden_shared.py), checkpoints of either mode into either model, and
the gradient exchange's bucket plan."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fake_engine import FakeEngine
import golden_utils as gu
from oneshotdet_amd import checkpoint, spec, synth
from oracle import hotpath_ref as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sd(shapes):
    return {k: torch.from_numpy(v) for k, v in synth.make_state_dict(shapes).items()}


def tied(sd):
    """The oracle reads `supp_backbone.*` by prefix: the same tensor objects as `backbone.*` make it the shared model."""
    out = dict(sd)
    for k in list(sd):
        if k.startswith("backbone."):
            out["supp_" + k] = sd[k]
    return out


@pytest.fixture(scope="module")
def sd_shared():
    return orc.to_torch_state_dict(synth.make_state_dict(spec.hot_path_shapes(False)))


def test_shared_key_set_matches_reference():
    ref = json.load(open(os.path.join(gu.GOLDEN_DIR, "state_dict_keys_shared.json")))
    mine = spec.hot_path_shapes(siamese_backbone=False)
    assert list(mine.keys()) == list(ref["shapes"].keys())
    for k, s in mine.items():
        assert list(s) == ref["shapes"][k], k
    assert not any(k.startswith("supp_backbone.") for k in mine)
    full = spec.full_model_shapes(siamese_backbone=False)
    assert len(full) == ref["num_all_keys"]
    assert {k: list(v) for k, v in full.items() if k.startswith("roi_heads.")} == ref["box_head_shapes"]
    frozen_params = sorted(k for k in mine if spec.is_frozen(k) and not any(
        k.endswith(b) for b in ("running_mean", "running_var")) and ".bn" not in k and "downsample.1" not in k)
    assert frozen_params == ref["frozen_params"]
    # the default stays the two-backbone key set
    assert list(spec.hot_path_shapes()) == list(spec.hot_path_shapes(True))
    assert set(spec.hot_path_shapes(True)) - set(mine) == {k for k in spec.hot_path_shapes(True) if k.startswith("supp_")}


@pytest.mark.parametrize("name", ["small", "nonsquare"])
def test_tied_oracle_forward_matches_reference(name, sd_shared):
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    f = gu.load("case_shared_%s.npz" % name)
    with torch.no_grad():
        o = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(q), tied(sd_shared), shots=S)
    head = gu.flatten_head(*[[t.numpy() for t in o[k]] for k in ("logits", "bbox_reg", "centerness")])
    np.testing.assert_allclose(head, f["head"], rtol=1e-4, atol=1e-4)       # (test_oracle_golden: 1e-5 across host CPUs)
    for lvl in range(5):
        ref = f["pooled.%d" % lvl]
        np.testing.assert_allclose(o["pooled"][lvl].reshape(B, -1).numpy(), ref, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()))
        gu.check_against(o["features"][lvl].numpy(), f, "features.%d" % lvl, 1e-4, 1e-4)
        gu.check_against(o["query_features"][lvl].numpy(), f, "query_features.%d" % lvl, 1e-4, 1e-4)
        gu.check_against(o["combined"][lvl].numpy(), f, "combined.%d" % lvl, 1e-4, 1e-4)
    # the shared model's query features differ from the two-backbone model's (the synth query backbone has its own weights)
    f2 = gu.load("case_%s.npz" % name)
    assert not np.allclose(f2["query_features.0.samples"], f["query_features.0.samples"])
    np.testing.assert_allclose(f2["features.0.samples"], f["features.0.samples"], rtol=1e-6)


def _oracle_grads(name, sd, tie):
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    leaves = {k: v.clone().requires_grad_(not spec.is_frozen(k)) for k, v in sd.items()}
    if tie:
        d = tied(leaves)
    else:        # untied: the two-backbone model with supp_backbone.* EQUAL to (but not the same tensors as) backbone.*
        d = dict(leaves)
        for k in sd:
            if k.startswith("backbone."):
                d["supp_" + k] = sd[k].clone().requires_grad_(not spec.is_frozen(k))
    o = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(q), d, shots=S)
    c, r, t, info = orc.fcos_loss(o["logits"], o["bbox_reg"], o["centerness"], gts, focal="cuda")
    (c + r + t).backward()
    return (c, r, t), info, gts, {k: v.grad for k, v in d.items() if v.requires_grad and v.grad is not None}


@pytest.mark.parametrize("name", ["small", "nonsquare", "shots5"])
def test_tied_oracle_training_matches_reference(name, sd_shared):
    """Losses and the full gradient (query branch attached) of the tied oracle against train_shared_*; the full gradient of a
    shared parameter is the sum of what the two branches of the untied (two-backbone) oracle give it."""
    f = gu.load("train_shared_%s.npz" % name)
    (c, r, t), info, gts, g = _oracle_grads(name, sd_shared, tie=True)
    np.testing.assert_array_equal(np.concatenate(gts, 0), f["gt_boxes"][:, 1:])
    np.testing.assert_allclose([c.item(), r.item(), t.item()], f["losses_cuda_formula"], rtol=1e-5)
    np.testing.assert_allclose(f["losses_cuda_formula"], f["losses_ref_cpu_formula"], rtol=2e-4)
    assert info["num_pos"] == int(f["num_pos"])
    np.testing.assert_array_equal(info["labels"].numpy().astype(np.int8), f["labels"])
    checked = 0
    for key in f.files:
        if key.startswith("fullgrad_oracle.") and key.endswith(".samples"):
            k = key[len("fullgrad_oracle."):-len(".samples")]
            gg = g[k].numpy().reshape(-1)
            idx = gu.sample_indices(gg.size, "grad." + k)[:256]
            scale = float(f["fullgrad_oracle.%s.absmax" % k])
            np.testing.assert_allclose(gg[idx], f[key], rtol=1e-3, atol=4e-3 * scale, err_msg=k)      # (test_oracle_golden's bars)
            checked += 1
    assert checked == 16
    _, _, _, gu_ = _oracle_grads(name, sd_shared, tie=False)
    for k in sd_shared:
        if k.startswith("backbone.") and k in g:
            np.testing.assert_allclose(g[k].numpy(), (gu_[k] + gu_["supp_" + k]).numpy(), rtol=1e-5,
                                       atol=1e-5 * float(g[k].abs().max()), err_msg=k)
    # the query branch contributes: the full gradient differs from the reference's detached-query one
    k = "backbone.body.layer3.1.conv2.weight"
    assert not np.allclose(f["fullgrad_oracle.%s.samples" % k], f["refgrad_detached.%s.samples" % k], rtol=1e-3)


def test_load_checkpoint_both_modes(tmp_path):
    shared = _sd(spec.full_model_shapes(False))
    siam = _sd(spec.full_model_shapes(True))
    ps, pt = str(tmp_path / "shared.pth"), str(tmp_path / "siamese.pth")
    checkpoint.save_checkpoint(ps, shared, tag_last=False)
    checkpoint.save_checkpoint(pt, siam, tag_last=False)
    assert checkpoint.has_query_backbone(pt) and not checkpoint.has_query_backbone(ps)
    assert checkpoint.has_query_backbone({"module." + k: v for k, v in siam.items()})
    assert not checkpoint.has_query_backbone(shared)
    # shared file -> shared model
    got, _ = checkpoint.load_checkpoint(ps, siamese_backbone=False)
    assert list(got) == list(spec.full_model_shapes(False))
    assert all(torch.equal(got[k], shared[k]) for k in got)
    # siamese file -> shared model: supp_backbone.* ignored, backbone.* is the file's target backbone
    got, _ = checkpoint.load_checkpoint(pt, siamese_backbone=False)
    assert list(got) == list(spec.full_model_shapes(False))
    assert all(torch.equal(got[k], siam[k]) for k in got)
    assert not torch.equal(siam["backbone.body.layer2.0.conv1.weight"], siam["supp_backbone.body.layer2.0.conv1.weight"])
    # shared file -> siamese model: the suffix match fills supp_backbone.* from backbone.* (unchanged behaviour)
    got, _ = checkpoint.load_checkpoint(ps)
    assert list(got) == list(spec.full_model_shapes(True))
    for k in spec.hot_path_shapes(True):
        src = k[len("supp_"):] if k.startswith("supp_backbone.") else k
        assert torch.equal(got[k], shared[src]), k
    # first-stage-only files and the Caffe2 route take the mode too
    got, _ = checkpoint.load_checkpoint(pt, second_stage=False, siamese_backbone=False)
    assert list(got) == list(spec.hot_path_shapes(False))


def test_load_c2_resnet_shared(tmp_path):
    import pickle
    blobs = {"conv1_w": np.ones((64, 3, 7, 7), np.float32), "res_conv1_bn_s": np.full(64, 2.0, np.float32),
             "res_conv1_bn_b": np.zeros(64, np.float32)}
    defaults = _sd(spec.full_model_shapes(False))
    for k, shape in spec.hot_path_shapes(False).items():
        if k.startswith("backbone.body.layer") and not k.endswith(("running_mean", "running_var")):
            blobs[k[len("backbone.body."):]] = np.full(tuple(shape), 0.5, np.float32)     # (no `_`: kept as it is)
    p = str(tmp_path / "r50.pkl")
    with open(p, "wb") as fh:
        pickle.dump({"blobs": blobs}, fh)
    out = checkpoint.load_c2_resnet(p, defaults, siamese_backbone=False)
    assert list(out) == list(spec.full_model_shapes(False))
    assert float(out["backbone.body.stem.conv1.weight"].mean()) == 1.0
    assert float(out["backbone.body.layer3.2.conv2.weight"].mean()) == 0.5
    assert torch.equal(out["rpn.head.cls_logits.bias"], defaults["rpn.head.cls_logits.bias"])


def test_training_checkpoint_round_trip_and_mode_mismatch(tmp_path):
    sd = _sd(spec.hot_path_shapes(False))
    p = str(tmp_path / "model_0000020.pth")
    checkpoint.save_training_checkpoint(p, FakeEngine(sd, siamese_backbone=False), 20)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert raw["siamese_backbone"] is False and raw["iteration"] == 20
    assert not any(k.startswith("supp_backbone.") for k in raw["model"])
    assert not any(k.startswith("supp_backbone.") for k in raw["optimizer"]["momentum_buffer"])
    eng, it = checkpoint.resume_training(p, lambda s: FakeEngine(s, siamese_backbone=False), siamese_backbone=False)
    assert it == 20 and eng.opt_state["steps"] == 3 and list(eng.sd) == list(spec.hot_path_shapes(False))
    assert all(torch.equal(eng.sd[k], sd[k]) for k in sd)
    eng, _ = checkpoint.resume_training(p, lambda s: FakeEngine(s, siamese_backbone=False))        # mode taken from the file
    # a mode mismatch is refused, never silently re-tied / untied
    with pytest.raises(ValueError, match="untie"):
        checkpoint.resume_training(p, lambda s: FakeEngine(s, siamese_backbone=True), siamese_backbone=True)
    with pytest.raises(ValueError, match="shared-backbone"):
        checkpoint.resume_training(p, lambda s: FakeEngine(s, siamese_backbone=True))
    p2 = str(tmp_path / "model_siamese.pth")
    checkpoint.save_training_checkpoint(p2, FakeEngine(_sd(spec.hot_path_shapes(True)), siamese_backbone=True), 5)
    assert torch.load(p2, map_location="cpu", weights_only=False)["siamese_backbone"] is True
    with pytest.raises(ValueError, match="tie"):
        checkpoint.resume_training(p2, lambda s: FakeEngine(s, siamese_backbone=False), siamese_backbone=False)
    # an older training checkpoint without the recorded mode: the key set decides
    raw2 = torch.load(p2, map_location="cpu", weights_only=False)
    del raw2["siamese_backbone"]
    torch.save(raw2, p2)
    with pytest.raises(ValueError):
        checkpoint.resume_training(p2, lambda s: FakeEngine(s, siamese_backbone=False), siamese_backbone=False)
    eng, it = checkpoint.resume_training(p2, lambda s: FakeEngine(s, siamese_backbone=True))
    assert it == 5 and any(k.startswith("supp_backbone.") for k in eng.sd)


def test_shared_bucket_plan_two_ranks():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker_shared.py")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS="1"), cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-1500:]
    assert "RANK 0 SHARED_EXCHANGE=True" in out.stdout and "RANK 1 SHARED_EXCHANGE=True" in out.stdout
