"""CPU: global-average query pooling (supp_roialign=False; FEW_SHOT.SUPP_ROIALIGN False: nn.AdaptiveAvgPool2d((1, 1)) of every
query feature map, generalized_rcnn.py:87-94, 302-303).  The oracle with its pooling restated as that average reproduces the
fixtures recorded through the real reference (tests/golden/make_golden_avgpool.py) in both backbone modes — head outputs, pooled
vectors, losses, and the reference's own gradients of both backbones; training checkpoints record the mode and refuse to resume
in the other; the C-ABI refuses the shapes its kernels cannot handle."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fake_engine import FakeEngine
import golden_utils as gu
from oneshotdet_amd import checkpoint, spec, synth
from oracle import hotpath_ref as orc


def avg_query_pool(query_feats, image_sizes, batch_size):
    """generalized_rcnn.py:87-94, 302-303 + batch_pooling :100-104 (the restatement make_golden_avgpool.py records with)"""
    pooled = []
    for feat in query_feats:
        v = F.adaptive_avg_pool2d(feat, (1, 1))
        D, C = v.shape[:2]
        pooled.append(v.view(batch_size, D // batch_size, C, 1, 1).mean(dim=1))
    return pooled


@pytest.fixture
def avgpool(monkeypatch):
    monkeypatch.setattr(orc, "query_pool", avg_query_pool)


def tied(sd):
    out = dict(sd)
    for k in list(sd):
        if k.startswith("backbone."):
            out["supp_" + k] = sd[k]
    return out


def _sd(shared):
    return orc.to_torch_state_dict(synth.make_state_dict(spec.hot_path_shapes(not shared)))


def _check_forward(o, f, B):
    head = gu.flatten_head(*[[t.numpy() for t in o[k]] for k in ("logits", "bbox_reg", "centerness")])
    np.testing.assert_allclose(head, f["head"], rtol=1e-4, atol=1e-4)          # test_oracle_golden's bars
    for lvl in range(5):
        ref = f["pooled.%d" % lvl]
        np.testing.assert_allclose(o["pooled"][lvl].reshape(B, -1).numpy(), ref, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()))
        for key in ("features", "query_features", "combined"):
            gu.check_against(o[key][lvl].numpy(), f, "%s.%d" % (key, lvl), 1e-4, 1e-4)


@pytest.mark.parametrize("name,shared", [("small", False), ("nonsquare", False), ("shots5", False), ("small", True),
                                         ("nonsquare", True)])
def test_oracle_forward_matches_reference(name, shared, avgpool):
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    f = gu.load("case_%savgpool_%s.npz" % ("shared_" if shared else "", name))
    sd = _sd(shared)
    with torch.no_grad():
        o = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(q), tied(sd) if shared else sd, shots=S)
    _check_forward(o, f, B)
    # a different model from the ROIAlign-pooled one of the same weights and inputs
    f_roi = gu.load("case_%s%s.npz" % ("shared_" if shared else "", name))
    assert not np.allclose(f["pooled.0"], f_roi["pooled.0"], rtol=1e-2, atol=1e-3)
    ref = f_roi["features.0.samples"]          # (the target branch is the same; recorded on another host: 1e-4)
    np.testing.assert_allclose(f["features.0.samples"], ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref).max()))


def test_oracle_ragged_matches_reference_and_the_mean_covers_the_padding(avgpool):
    t_np, q_np = gu.ragged_inputs()
    f = gu.load("case_avgpool_ragged.npz")
    sd = _sd(False)
    img, sizes = orc.to_image_list([torch.from_numpy(a) for a in t_np], gu.RAGGED["size_divisible"])
    q, qsizes = orc.to_image_list([torch.from_numpy(a) for a in q_np], gu.RAGGED["size_divisible"])
    assert tuple(q.shape) == tuple(f["padded_query"]) and qsizes == gu.RAGGED["queries"]
    with torch.no_grad():
        o = orc.hot_path_forward(img, q, sd, shots=1, query_sizes=qsizes)
        alone = avg_query_pool(orc.backbone(torch.from_numpy(q_np[0])[None], sd, "supp_backbone."), None, 1)
    _check_forward(o, f, 2)
    # query 0 (63 x 63) is padded to 96 x 96 in the batch: its vector is NOT the average of its own, unpadded maps
    for lvl in range(5):
        assert not np.allclose(alone[lvl].reshape(-1).numpy(), f["pooled.%d" % lvl][0], rtol=1e-2, atol=1e-3), lvl


def _oracle_training(name, shared):
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    sd = _sd(shared)
    for k in sd:
        if not spec.is_frozen(k):
            sd[k].requires_grad_(True)
    d = tied(sd) if shared else sd
    o = orc.hot_path_forward(torch.from_numpy(img), torch.from_numpy(q), d, shots=S)
    c, r, t, info = orc.fcos_loss(o["logits"], o["bbox_reg"], o["centerness"], gts, focal="cuda")
    (c + r + t).backward()
    return (c, r, t), info, gts, {k: v.grad for k, v in sd.items() if v.grad is not None}


@pytest.mark.parametrize("name,shared", [("small", False), ("nonsquare", False), ("shots5", False), ("small", True),
                                         ("shots5", True)])
def test_oracle_training_matches_reference(name, shared, avgpool):
    """Losses and gradients against train_*avgpool_*: the oracle's full gradient, and the REFERENCE's own (its autograd through
    AdaptiveAvgPool2d; the CPU focal-loss formula, within the same bars) — the query backbone's included."""
    f = gu.load("train_%savgpool_%s.npz" % ("shared_" if shared else "", name))
    (c, r, t), info, gts, g = _oracle_training(name, shared)
    np.testing.assert_array_equal(np.concatenate(gts, 0), f["gt_boxes"][:, 1:])
    np.testing.assert_allclose([c.item(), r.item(), t.item()], f["losses_cuda_formula"], rtol=1e-5)
    np.testing.assert_allclose(f["losses_cuda_formula"], f["losses_ref_cpu_formula"], rtol=2e-4)
    assert info["num_pos"] == int(f["num_pos"])
    np.testing.assert_array_equal(info["labels"].numpy().astype(np.int8), f["labels"])
    checked, query = 0, 0
    for key in f.files:
        for tag in ("fullgrad_oracle.", "refgrad."):
            if key.startswith(tag) and key.endswith(".samples"):
                k = key[len(tag):-len(".samples")]
                gg = g[k].numpy().reshape(-1)
                idx = gu.sample_indices(gg.size, "grad." + k)[:256]
                scale = float(f["%s%s.absmax" % (tag, k)])
                np.testing.assert_allclose(gg[idx], f[key], rtol=1e-3, atol=4e-3 * scale, err_msg=tag + k)
                checked += 1
                query += tag == "refgrad." and k.startswith("supp_backbone.")
    assert checked == 2 * (16 if shared else 19) and query == (0 if shared else 5), (checked, query)


def test_training_checkpoint_records_the_pooling_and_refuses_a_mismatch(tmp_path):
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(spec.hot_path_shapes()).items()}
    p = str(tmp_path / "model_0000010.pth")
    checkpoint.save_training_checkpoint(p, FakeEngine(sd, supp_roialign=False), 10)
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert raw["supp_roialign"] is False and raw["siamese_backbone"] is True
    eng, it = checkpoint.resume_training(p, lambda s: FakeEngine(s, supp_roialign=False), supp_roialign=False)
    assert it == 10 and eng.opt_state["steps"] == 3 and all(torch.equal(eng.sd[k], sd[k]) for k in sd)
    checkpoint.resume_training(p, lambda s: FakeEngine(s, supp_roialign=False))          # the caller need not say it: the file does
    with pytest.raises(ValueError, match="global-average"):
        checkpoint.resume_training(p, lambda s: FakeEngine(s, supp_roialign=True), supp_roialign=True)
    with pytest.raises(ValueError, match="supp_roialign=True"):
        checkpoint.resume_training(p, lambda s: FakeEngine(s, supp_roialign=True))
    # the keys are the same in both modes: load_checkpoint reads either file the same way
    p2 = str(tmp_path / "model_roialign.pth")
    checkpoint.save_training_checkpoint(p2, FakeEngine(sd, supp_roialign=True), 5)
    a, _ = checkpoint.load_checkpoint(p)
    b, _ = checkpoint.load_checkpoint(p2)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    # an engine without the attribute is the default mode; a file without the field resumes as ROIAlign pooling
    p3 = str(tmp_path / "model_old.pth")
    checkpoint.save_training_checkpoint(p3, FakeEngine(sd), 7)
    assert torch.load(p3, map_location="cpu", weights_only=False)["supp_roialign"] is True
    raw3 = torch.load(p3, map_location="cpu", weights_only=False)
    del raw3["supp_roialign"]
    torch.save(raw3, p3)
    eng, it = checkpoint.resume_training(p3, lambda s: FakeEngine(s, supp_roialign=True), supp_roialign=True)
    assert it == 7
    with pytest.raises(ValueError, match="ROIAlign"):
        checkpoint.resume_training(p3, lambda s: FakeEngine(s, supp_roialign=False), supp_roialign=False)
    with pytest.raises(ValueError):
        checkpoint.resume_training(p3, lambda s: FakeEngine(s, supp_roialign=False))


def test_c_abi_workspace_and_refused_shapes():
    """Argument checks run before any launch (no GPU needed): the forward's scratch size, and OSD_ERR_UNSUPPORTED (-2) for a
    channel count the 16-byte kernels cannot take, OSD_ERR_INVALID_ARG (-1) for more than 8 levels."""
    from oneshotdet_amd import _lib
    lib = _lib.load()
    hs, ws = (ctypes.c_int32 * 3)(52, 16, 1), (ctypes.c_int32 * 3)(52, 16, 1)
    # 52 x 52 -> 16 chunks (at most), 16 x 16 -> 4 chunks of 64 pixels, 1 x 1 -> 1: fp32 partials per map and channel
    assert lib.osd_query_avgpool_workspace_bytes(3, hs, ws, 40, 256) == 40 * (16 + 4 + 1) * 256 * 4
    assert lib.osd_query_avgpool_workspace_bytes(3, hs, ws, 40, 12) == -2
    assert lib.osd_query_avgpool_workspace_bytes(9, hs, ws, 40, 256) == -1
    ptrs = (ctypes.c_void_p * 3)(16, 32, 48)
    assert lib.osd_query_avgpool_levels(3, ptrs, hs, ws, 2, 1, 12, ptrs, None, 0, 1, None) == -2
    assert lib.osd_query_avgpool_levels_bwd(3, ptrs, hs, ws, 2, 1, 12, ptrs, 1, None) == -2
    assert b"multiple of 8" in lib.osd_last_error_string()
    assert lib.osd_query_avgpool_levels_bwd(3, ptrs, hs, ws, 2, 0, 256, ptrs, 1, None) == -1
    assert lib.osd_query_avgpool_levels(3, ptrs, hs, ws, 0, 1, 256, ptrs, None, 0, 1, None) == 0     # empty batch: no-op
