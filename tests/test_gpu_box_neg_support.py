"""GPU (-m gpu): the second stage's negative support (neg_support = FEW_SHOT.NEG_SUPPORT.TURN_ON with 'concat' and 'ce_loss') —
osd_box_loss_neg_support against the fixture recorded through the REAL reference (tests/golden/box_neg_support.npz), the two-branch box
head against the end-to-end fixture boxtrain_small_neg.npz (tests/golden/make_golden_box_neg_support.py), and the engine's step.

Tolerances: the bounds tests/test_gpu_box_soft_labels.py holds the same quantities to — kernel losses rtol 1e-5 against the float64
restatement (the fixture's inputs are bf16-exact), kernel gradients rtol 1e-5 / atol 1e-7 (fp32) and rtol 1e-2 / atol 1e-4 (bf16), engine
losses rtol 1e-4 (fp32) / 3e-2 (bf16), parameter gradients 1e-3 x absmax and feature-map gradients 5e-3 x absmax with cosine 0.9999
(fp32), relative L2 0.35 and cosine 0.96 (bf16).  What has to be zero (d_pred_neg outside the active hinges, everything of `nofg`'s
suppress term) is compared exactly."""
import ctypes

import numpy as np
import pytest
import torch

import box_neg_support_ref as bns
import golden_utils as gu
from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LOSS_CASES = ["mixed", "wide", "nofg"]
W = np.array([bns.W_CLS, bns.W_BOX, bns.W_SUPPRESS])


@pytest.fixture(scope="module")
def fx():
    return gu.load("box_neg_support.npz")


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------

def loss_inputs(f, name, stride, dt):
    """-> (pred, pred_neg [M, stride] with the row's 10 columns filled and 9.0 behind them, labels, targets, counts, n, S, valid)"""
    key = "loss.%s." % name
    S = int(f[key + "S"])
    counts = torch.from_numpy(f[key + "counts"])
    M = f[key + "logits"].shape[0]
    pred, neg = torch.full((M, stride), 9.0), torch.full((M, stride), 9.0)
    pred[:, :2], pred[:, 2:10] = torch.from_numpy(f[key + "logits"]), torch.from_numpy(f[key + "deltas"])
    neg[:, :2], neg[:, 2:10] = torch.from_numpy(f[key + "neg_logits"]), torch.from_numpy(f[key + "deltas"]).flip(0)
    valid = np.concatenate([np.arange(S) < int(c) for c in counts])
    return (pred.to(DT[dt]).cuda(), neg.to(DT[dt]).cuda(), torch.from_numpy(f[key + "labels"]).cuda(),
            torch.from_numpy(f[key + "targets"]).cuda(), counts.cuda(), len(counts), S, valid)


def check_loss_outputs(f, name, dt, losses, d, dn, valid):
    key = "loss.%s." % name
    want = f[key + "losses_f64"] * W
    got = losses.cpu().numpy()
    K = int(f[key + "K"])
    d = d.float().cpu().numpy().astype(np.float64)
    dn = dn.float().cpu().numpy().astype(np.float64)
    g_log, g_neg, g_del = (f[key + k].astype(np.float64) for k in ("grad_logits", "grad_neg_logits", "grad_deltas"))
    print("%s %s: losses %r want %r K %d | worst gradient error logits %.3e (float64 closed form %.3e) negative logits %.3e (%.3e) "
          "deltas %.3e" % (name, dt, got.tolist(), want.tolist(), K, np.abs(d[:, :2] - g_log).max(),
                           np.abs(d[:, :2] - f[key + "grad_logits_f64"]).max(), np.abs(dn[:, :2] - g_neg).max(),
                           np.abs(dn[:, :2] - f[key + "grad_neg_logits_f64"]).max(), np.abs(d[:, 2:10] - g_del).max()))
    np.testing.assert_allclose(got[[0, 1, 3]], want, rtol=1e-5)
    assert int(got[2]) == int(valid.sum()) and int(got[4]) == K
    tol = dict(rtol=1e-5, atol=1e-7) if dt == "f32" else dict(rtol=1e-2, atol=1e-4)
    for ref_log, ref_neg in ((g_log, g_neg), (f[key + "grad_logits_f64"], f[key + "grad_neg_logits_f64"])):
        np.testing.assert_allclose(d[:, :2], ref_log, **tol)
        np.testing.assert_allclose(dn[:, :2], ref_neg, **tol)
    np.testing.assert_allclose(d[:, 2:10], g_del, **tol)
    assert not d[:, 10:].any() and not d[~valid].any()
    # d_pred_neg: exactly zero in the delta columns and behind them, and in every row that is invalid, background or has an inactive
    # hinge; non-zero where the hinge is active
    active = f[key + "active"]
    assert not dn[:, 2:].any() and not dn[~active].any() and not (active & ~valid).any()
    assert (np.abs(dn[active, :2]) > 0).all()
    if K == 0:
        assert got[3] == 0.0 and got[4] == 0.0 and not dn.any()
        assert bool(f[key + "reference_nan_without_foreground"]) and np.isnan(f[key + "losses_ref"][2])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", LOSS_CASES)
def test_loss_kernel_matches_the_reference_fixture(fx, name, dt):
    """ops.box_loss_neg_support on the reference's FastRCNNLossComputation.__call__ with neg_class_logits: the three losses against the
    float64 restatement, the valid-row count and K, the reference's autograd and the float64 closed forms w.r.t. both logit sets and
    the deltas.  Rows past the count hold label 1 and the negative logits (-30, 30): counted as foreground they would add hinges of 0.3
    to 1.3 and change K.  `wide` is 1,152 rows (the second trip of the row loop) with one image's count 0; `nofg` has K = 0: the
    reference gives NaN, the kernel its documented (.., 0, 0) and zero hinge gradients.
    Measured on an MI355X (fp32, worst over the cases): losses 9.3e-8 relative, logit gradients within 3.0e-8 absolute of the reference's
    autograd and 3.1e-8 of the float64 closed form (negative branch: 2.2e-8 / 3.2e-9).  The 1e-5 bound holds as it stands."""
    from oneshotdet_amd import ops
    pred, neg, labels, targets, counts, n, S, valid = loss_inputs(fx, name, 10, dt)
    losses, d, dn = ops.box_loss_neg_support(pred, neg, labels, targets, counts, n, S, bns.W_CLS, bns.W_BOX, grad_stride=16)
    torch.cuda.synchronize()
    assert tuple(losses.shape) == (5,) and tuple(d.shape) == tuple(dn.shape) == (n * S, 16)
    check_loss_outputs(fx, name, dt, losses, d, dn, valid)
    # without the gradient: the same losses, bit for bit
    l2, none, none2 = ops.box_loss_neg_support(pred, neg, labels, targets, counts, n, S, bns.W_CLS, bns.W_BOX)
    assert none is None and none2 is None and torch.equal(l2.view(torch.int32), losses.view(torch.int32))
    # the defaults are the reference's margin and weight
    l3, _, _ = ops.box_loss_neg_support(pred, neg, labels, targets, counts, n, S, bns.W_CLS, bns.W_BOX, w_suppress=spec.BOX_SUPPRESS_WEIGHT,
                                        margin=spec.BOX_SUPPRESS_MARGIN)
    assert torch.equal(l3.view(torch.int32), losses.view(torch.int32)) and (spec.BOX_SUPPRESS_WEIGHT, spec.BOX_SUPPRESS_MARGIN) == (2.5, 0.3)


def test_c_entry_with_padded_strides_null_gradients_bad_labels_and_error_codes(fx):
    """osd_box_loss_neg_support called directly: pred_stride 16 and grad_stride 12 (both wider than the row), both gradient buffers
    pre-filled: every row of both is written.  With d_pred null it computes the losses only, bit-equal.  One valid foreground row with
    label 2: losses 0, 1 and 3 come back NaN, K drops by one, the row's gradients are zero in both buffers and every other row's box
    gradient is what it was.  A null pred_neg, one gradient buffer without the other and a stride below 2 + 8 are refused with a
    negative code and a message."""
    from oneshotdet_amd import _lib
    name = "mixed"
    pred, neg, labels, targets, counts, n, S, valid = loss_inputs(fx, name, 16, "f32")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(lab, grads=True, pstride=16, gstride=12, neg_ptr=True, dn_ptr=True):
        losses = torch.full((5,), 7.0, device="cuda")
        d = torch.full((n * S, 12), 7.0, device="cuda")
        dn = torch.full((n * S, 12), 7.0, device="cuda")
        _lib.call("osd_box_loss_neg_support", pred.data_ptr(), neg.data_ptr() if neg_ptr else None, lab.data_ptr(), targets.data_ptr(),
                  counts.data_ptr(), n, S, pstride, bns.W_CLS, bns.W_BOX, bns.MARGIN, bns.W_SUPPRESS, losses.data_ptr(),
                  d.data_ptr() if grads else None, dn.data_ptr() if grads and dn_ptr else None, gstride, _lib.OSD_F32, st)
        torch.cuda.synchronize()
        return losses, d, dn
    losses, d, dn = run(labels)
    check_loss_outputs(fx, name, "f32", losses, d, dn, valid)
    only, d0, dn0 = run(labels, grads=False)
    assert torch.equal(only.view(torch.int32), losses.view(torch.int32)) and bool((d0 == 7.0).all()) and bool((dn0 == 7.0).all())
    bad = labels.clone()
    active = fx["loss.mixed.active"]
    row = int(np.nonzero(active)[0][1])
    bad[row] = 2
    l2, d2, dn2 = run(bad)
    assert torch.isnan(l2[[0, 1, 3]]).all() and int(l2[2]) == int(valid.sum()) and int(l2[4]) == int(fx["loss.mixed.K"]) - 1
    assert not d2[row].any() and not dn2[row].any() and not d2[torch.from_numpy(~valid).cuda()].any()
    others = torch.ones(n * S, dtype=torch.bool, device="cuda")
    others[row] = False
    assert torch.equal(d2[others][:, 2:], d[others][:, 2:])
    for kw in (dict(neg_ptr=False), dict(dn_ptr=False), dict(pstride=9), dict(gstride=9)):
        with pytest.raises(_lib.OsdError, match="box_loss_neg_support") as e:
            run(labels, **kw)
        assert e.value.code < 0, kw


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["mixed", "wide"])
def test_zero_suppress_weight_is_osd_box_loss_bit_for_bit(fx, name, dt):
    """With w_suppress = 0 the first three losses and d_pred are osd_box_loss's, bit for bit, and d_pred_neg is zero."""
    from oneshotdet_amd import ops
    pred, neg, labels, targets, counts, n, S, valid = loss_inputs(fx, name, 12, dt)
    plain, dp = ops.box_loss(pred, labels, targets, counts, n, S, bns.W_CLS, bns.W_BOX, grad_stride=16)
    losses, d, dn = ops.box_loss_neg_support(pred, neg, labels, targets, counts, n, S, bns.W_CLS, bns.W_BOX, w_suppress=0.0, grad_stride=16)
    torch.cuda.synchronize()
    assert torch.equal(losses[:3].view(torch.int32), plain.view(torch.int32)) and float(losses[3]) == 0.0
    assert int(losses[4]) == int(fx["loss.%s.K" % name])
    bits = torch.int32 if dt == "f32" else torch.int16
    assert torch.equal(d.contiguous().view(bits), dp.view(bits)) and not dn.any()


# ---- the engines ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def np_sd():
    return synth.make_state_dict(spec.full_model_shapes())


def _neg_query(f):
    B, H, Wd, S, qh, qw = gu.CASES["small"]
    return synth.make_images(str(f["neg_query.name"]), B * S, qh, qw, int(f["neg_query.seed"]))


def _train_fixture():
    name = "small"
    f = gu.load("boxtrain_small_neg.npz")
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


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_box_head_training_with_a_negative_support_matches_the_reference_fixture(np_sd, dt):
    """tests/test_gpu_box_train.py's comparison of the training box head, on boxtrain_small_neg.npz with a neg_support engine: the
    query backbone runs on (query, negative query) as one batch of 2B rows, the box head on the sampled ROIs against both.  Sampled
    rows and labels exact, the three losses, gradient samples of the 14 box-head parameter tensors (reference autograd: both branches
    add into every one of them), the full gradient maps of the positive and of the negative query at their pooling level, samples of
    the target feature maps' gradients."""
    from oneshotdet_amd import train
    name = "small"
    eng = train.TrainEngine(np_sd, dtype=DT[dt], second_stage=True, neg_support=True)
    f, props, n_props, gt, gcnt, keys = _train_fixture()
    B, H, Wd, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    both = torch.cat([torch.from_numpy(q), torch.from_numpy(_neg_query(f))]).cuda()
    (feats, qall), _ = eng.backbones_forward(torch.from_numpy(img).cuda(), both)
    qfeats, nqfeats, _ = eng._split_neg_rows(qall, B)
    assert all(a.is_contiguous() and b.is_contiguous() and a.shape[0] == b.shape[0] == B for a, b in zip(qfeats, nqfeats))
    eng.flat_g.zero_()
    proposals = (torch.from_numpy(props).cuda(), None, torch.from_numpy(n_props).cuda())
    losses, gx, gqs, gqs_neg = eng.box_head_forward_backward(
        feats, qfeats, [(qh, qw)] * B, S, proposals, torch.from_numpy(gt).cuda(), torch.from_numpy(gcnt).cuda(),
        keys=torch.from_numpy(keys).cuda(), want_debug=True, neg_qfeats=nqfeats, neg_q_sizes=[(qh, qw)] * B)
    torch.cuda.synchronize()
    M = B * spec.BOX_BATCH_PER_IMAGE
    for i in range(B):
        k = len(f["index.%d" % i])
        assert np.array_equal(eng.last_box["index"][i].cpu().numpy()[:k], f["index.%d" % i])
        assert np.array_equal(eng.last_box["labels"][i].cpu().numpy()[:k], f["labels.%d" % i])
    assert eng.last_box["pred"].shape[0] == eng.last_box["pred_neg"].shape[0] == M
    assert not torch.equal(eng.last_box["pred"], eng.last_box["pred_neg"])
    got = losses.cpu().numpy()
    print(dt, "losses", got.tolist(), "reference", f["losses"].tolist())
    np.testing.assert_allclose(got[[0, 1, 3]], f["losses"], rtol=1e-4 if dt == "f32" else 3e-2)
    assert int(got[2]) == B * int(f["n_sampled"]) and int(got[4]) == int(f["n_foreground"])
    grads = eng.named_grads()

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
            assert tuple(grads[k].shape) == tuple(spec.box_head_shapes()[k]), k
            idx = gu.sample_indices(g.size, "boxgrad." + k)[:256]
            check(g[idx], f[key], float(f["refgrad.%s.absmax" % k]), k)
            checked += 1
    assert checked == 14
    for lvl in range(5):
        tag = "oracle_only.dfeat.%d" % lvl
        got = gx[lvl].cpu().permute(0, 3, 1, 2).numpy().reshape(-1)
        check(got[gu.sample_indices(got.size, tag)], f[tag + ".samples"], max(float(f[tag + ".absmax"].max()), 1e-12), tag, tier=5e-3)
    qlvl = int(f["query_level"])
    for what, maps, ref in (("dqfeat_pos", gqs, f["dqfeat_pos"]), ("dqfeat_neg", gqs_neg, f["dqfeat_neg"])):
        assert [lv for lv, _ in maps] == [qlvl]
        got = maps[0][1].cpu().permute(0, 3, 1, 2).numpy()
        assert got.shape == ref.shape
        check(got.reshape(-1), ref.reshape(-1), float(np.abs(ref).max()), what, tier=5e-3)


def _step_inputs():
    name = "small"
    B, H, Wd, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    gts = synth.make_gt_boxes(B, H, Wd, seed=3, max_boxes=3)
    gtb = torch.zeros(B, max(len(g) for g in gts), 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    cnt = torch.tensor([len(g) for g in gts], dtype=torch.int32)
    keys = torch.rand((B, spec.POST_NMS_TOP_N_TRAIN + gtb.shape[1]), generator=torch.Generator().manual_seed(0)).cuda()
    return torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), gtb.cuda(), cnt.cuda(), keys


@pytest.mark.parametrize("siamese", [True, False], ids=["two_backbones", "shared_backbone"])
def test_train_step_with_a_negative_support(siamese):
    """One fp32 train_step with neg_support=True on the `small` geometry, in the two-backbone and in the shared-backbone engine: finite
    losses, box_suppress_loss[1] = the label-1 rows among the step's own sampled rows, the query backbone's trainable weights change.
    A second engine fed the positive query as its negative support: p == q on every foreground row, so the suppress loss is the weight
    times the margin."""
    from oneshotdet_amd import ops, train
    sd = synth.make_state_dict(spec.full_model_shapes(siamese))
    images, queries, gtb, cnt, keys = _step_inputs()
    f = gu.load("boxtrain_small_neg.npz")
    neg = torch.from_numpy(_neg_query(f)).cuda()
    qb = ("supp_backbone." if siamese else "backbone.") + "body.layer2.0.conv1"

    def step(neg_queries):
        eng = train.TrainEngine(sd, dtype=torch.float32, second_stage=True, siamese_backbone=siamese, neg_support=True)
        eng.box_keys = keys
        assert eng.box_suppress_loss is None
        w0 = eng.convs[qb].w.clone()
        losses = eng.train_step(images, queries, gtb, cnt, neg_queries=neg_queries)
        eng.join()
        torch.cuda.synchronize()
        return eng, losses, w0
    eng, losses, w0 = step(neg)
    assert torch.isfinite(losses).all() and torch.isfinite(eng.box_losses).all() and torch.isfinite(eng.box_suppress_loss).all()
    assert tuple(eng.box_losses.shape) == (3,) and tuple(eng.box_suppress_loss.shape) == (2,)
    pb, _, pc = eng.proposals
    S = spec.BOX_BATCH_PER_IMAGE
    _, sl, _, _, sc = ops.box_match_sample(pb, pc, gtb, cnt, keys, S, spec.BOX_POSITIVE_FRACTION, spec.BOX_FG_IOU_THRESH, spec.BOX_REG_WEIGHTS)
    rows = torch.arange(S, device="cuda")[None, :] < sc[:, None]
    K = int(((sl == 1) & rows).sum())
    print("suppress loss %.6f over K = %d foreground rows (%d sampled)" % (float(eng.box_suppress_loss[0]), K, int(eng.box_losses[2])))
    assert K > 0 and int(eng.box_suppress_loss[1]) == K and float(eng.box_suppress_loss[0]) >= 0
    assert not torch.equal(eng.convs[qb].w, w0) and torch.isfinite(eng.convs[qb].w).all()
    same, _, _ = step(queries.clone())
    np.testing.assert_allclose(float(same.box_suppress_loss[0]), bns.W_SUPPRESS * bns.MARGIN, rtol=1e-5)
    assert int(same.box_suppress_loss[1]) == K


def test_padded_batches_with_their_own_true_sizes():
    """Two targets and two queries of different true sizes as layers.ImageList (the `ragged` inputs, padded to a multiple of 32), the
    negative supports the queries in the other order — the same padded shape, other true sizes per row: every whole-image box picks
    its own level, in the negative branch too.  Finite losses and K as sampled; fed the queries themselves (the same true sizes) the
    negative branch must reproduce the positive one, so the suppress loss is the weight times the margin."""
    from oneshotdet_amd import layers, ops, train
    t, q = gu.ragged_inputs()
    div = gu.RAGGED["size_divisible"]
    images = layers.to_image_list([torch.from_numpy(a) for a in t], div).to("cuda")
    queries = layers.to_image_list([torch.from_numpy(a) for a in q], div).to("cuda")
    swapped = layers.to_image_list([torch.from_numpy(a) for a in q[::-1]], div).to("cuda")
    assert swapped.tensors.shape == queries.tensors.shape and swapped.image_sizes == queries.image_sizes[::-1] != queries.image_sizes
    B = len(t)
    gts = synth.make_gt_boxes(B, min(h for h, _ in gu.RAGGED["targets"]), min(w for _, w in gu.RAGGED["targets"]), seed=3, max_boxes=3)
    gtb = torch.zeros(B, max(len(g) for g in gts), 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    gtb, cnt = gtb.cuda(), torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda()
    keys = torch.rand((B, spec.POST_NMS_TOP_N_TRAIN + gtb.shape[1]), generator=torch.Generator().manual_seed(1)).cuda()
    sd = synth.make_state_dict(spec.full_model_shapes())

    def step(neg_queries):
        eng = train.TrainEngine(sd, dtype=torch.float32, second_stage=True, neg_support=True)
        eng.box_keys = keys
        losses = eng.train_step(images, queries, gtb, cnt, neg_queries=neg_queries)
        eng.join()
        torch.cuda.synchronize()
        assert torch.isfinite(losses).all() and torch.isfinite(eng.box_losses).all() and torch.isfinite(eng.box_suppress_loss).all()
        return eng
    eng = step(swapped)
    pb, _, pc = eng.proposals
    S = spec.BOX_BATCH_PER_IMAGE
    _, sl, _, _, sc = ops.box_match_sample(pb, pc, gtb, cnt, keys, S, spec.BOX_POSITIVE_FRACTION, spec.BOX_FG_IOU_THRESH, spec.BOX_REG_WEIGHTS)
    K = int(((sl == 1) & (torch.arange(S, device="cuda")[None, :] < sc[:, None])).sum())
    print("ragged: suppress loss %.6f over K = %d foreground rows" % (float(eng.box_suppress_loss[0]), K))
    assert K > 0 and int(eng.box_suppress_loss[1]) == K
    assert abs(float(eng.box_suppress_loss[0]) - bns.W_SUPPRESS * bns.MARGIN) > 1e-4        # another support: not the margin
    same = step(layers.ImageList(queries.tensors.clone(), queries.image_sizes))
    np.testing.assert_allclose(float(same.box_suppress_loss[0]), bns.W_SUPPRESS * bns.MARGIN, rtol=1e-5)


def test_neg_support_off_makes_the_launches_it_makes_today():
    """neg_support=False is the engine built without the keyword: the launch trace of a forward_backward has the same kinds in the same
    order and the losses are bit-identical; with the option on the trace also has the new loss launch and no plain one."""
    from oneshotdet_amd import trace, train
    sd = synth.make_state_dict(spec.full_model_shapes())
    images, queries, gtb, cnt, keys = _step_inputs()

    def run(neg_queries=None, **kw):
        eng = train.TrainEngine(sd, dtype=torch.bfloat16, second_stage=True, **kw)
        eng.box_keys = keys
        trace.TRACE = []
        try:
            losses = eng.forward_backward(images, queries, gtb, cnt, neg_queries=neg_queries) if kw.get("neg_support") else \
                eng.forward_backward(images, queries, gtb, cnt)
            torch.cuda.synchronize()
            kinds = [k for k, _ in trace.TRACE]
        finally:
            trace.TRACE = None
        return losses.clone(), eng.box_losses.clone(), kinds, eng
    l0, b0, k0, e0 = run()
    l1, b1, k1, e1 = run(neg_support=False)
    assert e1.neg_support is False and e0.neg_support is False and e1.box_suppress_loss is None
    assert k0 == k1 and len(k0) > 10 and "box_loss_neg_support" not in k0
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and torch.equal(b0.view(torch.int32), b1.view(torch.int32))
    l2, b2, k2, e2 = run(neg_queries=queries.flip(-1).contiguous(), neg_support=True)
    assert k2.count("box_loss_neg_support") == 1 and e2.box_suppress_loss is not None
    with pytest.raises(ValueError, match="NEG_SUPPORT"):
        e1.forward_backward(images, queries, gtb, cnt, neg_queries=queries)
    with pytest.raises(ValueError, match="NEG_SUPPORT"):
        e2.forward_backward(images, queries, gtb, cnt)
    with pytest.raises(ValueError, match="NEG_SUPPORT"):
        e2.capture(images, queries, gtb, cnt)
