"""GPU (-m gpu): the second stage's classification-loss modes (box_cls_loss = FEW_SHOT.SECOND_STAGE_CLS_LOSS: 'ce_loss',
'focal_loss', 'mse_loss') — osd_box_loss_opt / osd_box_decode_opt against the fixture recorded through the REAL reference
(tests/golden/box_cls_modes.npz), and the engines in 'focal_loss' against the end-to-end pair box_small_focal.npz /
boxtrain_small_focal.npz (tests/golden/make_golden_box_cls_modes.py).

Tolerances are those tests/test_gpu_box_train.py and tests/test_gpu_box_head.py use for the same quantities: kernel losses rtol 1e-5
(fp32 arithmetic in both dtypes: the fixture's inputs are bf16 numbers, only the stored gradient is rounded), kernel gradients rtol
1e-5 / atol 1e-7 (fp32) and rtol 1e-2 / atol 1e-4 (bf16); decode scores 1e-6, boxes 1e-4 px; engine losses rtol 1e-4 (fp32) / 3e-2
(bf16), parameter gradients 1e-3 x absmax (fp32), relative L2 0.35 and cosine 0.96 (bf16).  The focal loss is held to the float64
restatement with the reference's CUDA formula (the kernel's); the reference's CPU value differs by its log(p + 1e-6)."""
import ctypes

import numpy as np
import pytest
import torch

import box_cls_loss_ref as bcl
import golden_utils as gu
from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LOSS_CASES = ["mixed", "nopos", "allpos", "large"]
ONE_LOGIT = ["focal_loss", "mse_loss"]
W = np.array([bcl.W_CLS, bcl.W_BOX])


@pytest.fixture(scope="module")
def fx():
    return gu.load("box_cls_modes.npz")


def loss_inputs(f, name, mode, stride, dt):
    """-> (pred [M, stride] with the row's L + 8 columns filled and 9.0 behind them, labels, targets, counts, n, S, L, valid)"""
    S = int(f["loss.%s.S" % name])
    counts = torch.from_numpy(f["loss.%s.counts" % name])
    logits = torch.from_numpy(f["loss.%s.%s" % (name, "logits2" if mode == "ce_loss" else "logits1")])
    L = logits.shape[1]
    pred = torch.full((logits.shape[0], stride), 9.0)
    pred[:, :L], pred[:, L:L + 8] = logits, torch.from_numpy(f["loss.%s.deltas" % name])
    valid = np.concatenate([np.arange(S) < int(c) for c in counts])
    return (pred.to(DT[dt]).cuda(), torch.from_numpy(f["loss.%s.labels" % name]).cuda(), torch.from_numpy(f["loss.%s.targets" % name]).cuda(),
            counts.cuda(), len(counts), S, L, valid)


def check_loss_outputs(f, name, mode, dt, losses, d, L, valid):
    key = "loss.%s.%s" % (name, mode)
    want = f[key + ".losses_f64"] * W
    got = losses.cpu().numpy()
    g_log = f[key + (".grad_logits_f64" if mode == "focal_loss" else ".grad_logits")].astype(np.float64)
    g_del = f["loss.%s.grad_deltas" % name].astype(np.float64)
    d = d.float().cpu().numpy().astype(np.float64)
    print("%s %s %s: losses %r want %r rel %.2e %.2e | worst gradient error logits %.3e deltas %.3e"
          % (name, mode, dt, got[:2].tolist(), want.tolist(), abs(got[0] - want[0]) / max(abs(want[0]), 1e-30),
             abs(got[1] - want[1]) / max(abs(want[1]), 1e-30), np.abs(d[:, :L] - g_log).max(), np.abs(d[:, L:L + 8] - g_del).max()))
    np.testing.assert_allclose(got[:2], want, rtol=1e-5)
    assert int(got[2]) == int(valid.sum())
    tol = dict(rtol=1e-5, atol=1e-7) if dt == "f32" else dict(rtol=1e-2, atol=1e-4)
    np.testing.assert_allclose(d[:, :L], g_log, **tol)
    np.testing.assert_allclose(d[:, L:L + 8], g_del, **tol)
    assert not d[:, L + 8:].any() and not d[~valid].any()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", bcl.CLS_LOSSES)
@pytest.mark.parametrize("name", LOSS_CASES)
def test_loss_kernel_matches_the_reference_fixture(fx, name, mode, dt):
    """ops.box_loss in every mode on rows of exactly L + 8 columns: both losses, the valid-row count, the gradient w.r.t. the logits
    and the deltas (class-1 deltas at columns L + 4 .. L + 7), zero rows past the count (which hold label 1 and numbers: a count of
    positives over them, or a read of them, shows), zero columns behind the row.  `large` is M = 1152 rows: the second trip of the
    1024-thread row loop.
    Measured on an MI355X (fp32, worst over the cases): focal loss 1.2e-7 relative, mse 6.6e-8; logit gradients within 3.0e-7
    absolute (`nopos` focal, whose gradients are of order 1: nothing divides them), 4.8e-8 elsewhere.  The fp32 bound holds for
    focal's pow / log chain as it stands."""
    from oneshotdet_amd import ops
    L = bcl.n_logits(mode)
    pred, labels, targets, counts, n, S, L, valid = loss_inputs(fx, name, mode, L + 8, dt)
    losses, d = ops.box_loss(pred, labels, targets, counts, n, S, bcl.W_CLS, bcl.W_BOX, grad_stride=16, cls_loss=mode)
    check_loss_outputs(fx, name, mode, dt, losses, d, L, valid)
    assert int(fx["loss.%s.%s.n_pos" % (name, mode)]) == int((labels.cpu().numpy()[valid] > 0).sum())
    # without the gradient: the same losses, bit for bit
    l2, none = ops.box_loss(pred, labels, targets, counts, n, S, bcl.W_CLS, bcl.W_BOX, cls_loss=mode)
    assert none is None and torch.equal(l2, losses)
    if mode == "focal_loss" and name == "mixed":       # gamma and alpha are arguments
        l3, _ = ops.box_loss(pred, labels, targets, counts, n, S, bcl.W_CLS, bcl.W_BOX, cls_loss=mode, gamma=1.5, alpha=0.4)
        p = pred.float().cpu()
        want = bcl.losses(p[valid][:, :1].double(), p[valid][:, 1:9].double(), labels.cpu()[valid].long(),
                          targets.cpu()[valid].double(), mode, gamma=1.5, alpha=0.4)[0].item()
        np.testing.assert_allclose(float(l3[0]), want, rtol=1e-5)


@pytest.mark.parametrize("mode", ONE_LOGIT)
def test_c_entry_with_padded_strides_bad_labels_and_invalid_rows(fx, mode):
    """osd_box_loss_opt called directly: pred_stride 16 and grad_stride 12 (both wider than the 9-column row), d_pred pre-filled.
    Every row of d_pred is written: gradients in the valid rows, zeros past the count and behind column 8.  Then one valid row gets
    label 2: it has no columns, so both losses come back NaN, its gradient row is zero (nothing was read or written for it beyond
    the zeroing every row gets) and every other row's box gradient is what it was."""
    from oneshotdet_amd import _lib
    name = "mixed"
    pred, labels, targets, counts, n, S, L, valid = loss_inputs(fx, name, mode, 16, "f32")
    code = spec.BOX_CLS_LOSSES.index(mode)

    def run(lab):
        losses = torch.full((3,), 7.0, device="cuda")
        d = torch.full((n * S, 12), 7.0, device="cuda")
        _lib.call("osd_box_loss_opt", pred.data_ptr(), lab.data_ptr(), targets.data_ptr(), counts.data_ptr(), n, S, 16,
                  bcl.W_CLS, bcl.W_BOX, losses.data_ptr(), d.data_ptr(), 12, _lib.OSD_F32, code, bcl.GAMMA, bcl.ALPHA,
                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return losses, d
    losses, d = run(labels)
    check_loss_outputs(fx, name, mode, "f32", losses, d, L, valid)
    bad = labels.clone()
    row = int(np.nonzero(valid & (labels.cpu().numpy() == 1))[0][1])
    bad[row] = 2
    l2, d2 = run(bad)
    assert torch.isnan(l2[:2]).all() and int(l2[2]) == int(valid.sum())
    assert not d2[row].any() and not d2[torch.from_numpy(~valid).cuda()].any()
    others = torch.ones(n * S, dtype=torch.bool, device="cuda")
    others[row] = False
    assert torch.equal(d2[others][:, 1:], d[others][:, 1:])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_old_entries_equal_the_opt_entries_in_ce_mode_bit_for_bit(fx, dt):
    """osd_box_loss / osd_box_decode forward to the _opt entries with OSD_BOX_CLS_CE: the same launch, the same bits."""
    from oneshotdet_amd import _lib, ops
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pred, labels, targets, counts, n, S, L, valid = loss_inputs(fx, "large", "ce_loss", 12, dt)
    l_old, d_old = ops.box_loss(pred, labels, targets, counts, n, S, bcl.W_CLS, bcl.W_BOX, grad_stride=16)
    l_new = torch.empty(3, device="cuda")
    d_new = torch.empty_like(d_old)
    _lib.call("osd_box_loss_opt", pred.data_ptr(), labels.data_ptr(), targets.data_ptr(), counts.data_ptr(), n, S, 12, bcl.W_CLS,
              bcl.W_BOX, l_new.data_ptr(), d_new.data_ptr(), 16, ops._dt(pred), _lib.BOX_CLS_CE, 0.0, 0.0, st)
    assert torch.equal(l_old, l_new) and torch.equal(d_old.view(torch.int16 if dt == "bf16" else torch.int32),
                                                      d_new.view(torch.int16 if dt == "bf16" else torch.int32))
    g = torch.Generator().manual_seed(4)
    N, R, shots = 2, 50, 3
    p = (torch.randn(shots, N * R, 12, generator=g) * 2).to(DT[dt]).cuda()
    xy = torch.rand(N, R, 2, generator=g) * 200
    rois = torch.cat([xy, xy + torch.rand(N, R, 2, generator=g) * 150 + 1], -1).cuda()
    cnt = torch.tensor([R, 31], dtype=torch.int32).cuda()
    old = ops.box_decode(p, rois, cnt, spec.BOX_REG_WEIGHTS, 240, 320, 0.0, want_raw=True)
    new = [torch.empty_like(t) for t in old]
    rw = (ctypes.c_float * 4)(*spec.BOX_REG_WEIGHTS)
    _lib.call("osd_box_decode_opt", p.data_ptr(), rois.data_ptr(), cnt.data_ptr(), new[0].data_ptr(), new[1].data_ptr(),
              new[2].data_ptr(), new[3].data_ptr(), N, R, shots, 12, rw, 240.0, 320.0, None, 0.0, ops._dt(p), _lib.BOX_CLS_CE, st)
    for a, b in zip(old, new):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", bcl.CLS_LOSSES)
def test_decode_kernel_matches_the_reference_fixture(fx, mode, dt):
    """ops.box_decode in every mode on the reference's PostProcessor output (after clip_to_image, before NMS): the class-1 score
    (sigmoid of the one logit / softmax of the two), the box decoded from the class-1 deltas (columns L + 4 .. L + 7), -1 for the
    rows past the count.  The inputs are bf16 numbers, so both dtypes are held to the same bounds."""
    from oneshotdet_amd import ops
    L = bcl.n_logits(mode)
    n, R = fx["decode.rois"].shape[:2]
    pred = torch.full((1, n * R, L + 8), 9.0)
    pred[0, :, :L], pred[0, :, L:] = torch.from_numpy(fx["decode.%s.logits" % mode])[0], torch.from_numpy(fx["decode.deltas"])
    ih, iw = (int(v) for v in fx["decode.image_size"])
    counts = torch.from_numpy(fx["decode.counts"])
    scores, boxes, lo, ro = ops.box_decode(pred.to(DT[dt]).cuda(), torch.from_numpy(fx["decode.rois"]).cuda(), counts.cuda(),
                                           spec.BOX_REG_WEIGHTS, ih, iw, spec.BOX_SCORE_THRESH, want_raw=True, cls_loss=mode)
    live = np.arange(R)[None, :] < counts.numpy()[:, None]
    s, b = scores.cpu().numpy(), boxes.cpu().numpy()
    print(mode, dt, "worst score error %.2e, box error %.2e px" % (np.abs(s[live] - fx["decode.%s.scores" % mode][live]).max(),
                                                                np.abs(b[live] - fx["decode.%s.boxes" % mode][live]).max()))
    assert (s[~live] == -1).all()
    np.testing.assert_allclose(s[live], fx["decode.%s.scores" % mode][live], rtol=0, atol=1e-6)
    np.testing.assert_allclose(b[live], fx["decode.%s.boxes" % mode][live], rtol=0, atol=1e-4)
    assert tuple(lo.shape) == (n * R, L) and torch.equal(lo.cpu(), pred[0, :, :L]) and torch.equal(ro.cpu(), pred[0, :, L:])


# ---- the engines in 'focal_loss' against the end-to-end pair -----------------------------------------------------------------------

def _sd(mode):
    return synth.make_state_dict(spec.full_model_shapes(box_cls_loss=mode))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_focal_box_head_matches_the_reference_golden(dt):
    """tests/test_gpu_box_head.py's comparison of the inference box head, on box_small_focal.npz with a 'focal_loss' engine."""
    from oneshotdet_amd import model, ops
    name = "small"
    B, H, Wd, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    f = gu.load("box_small_focal.npz")
    eng = model.HotPathEngine(_sd("focal_loss"), dtype=DT[dt], box_cls_loss="focal_loss")
    feats, qfeats, _, _ = eng.forward_features(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda())
    props = torch.stack([torch.from_numpy(f["proposals.%d.boxes" % i]) for i in range(B)], 0).cuda()
    out = eng.box_detect(feats, qfeats, (qh, qw), props, None, H, Wd, shots=S, cuda_nms=False, want_raw=True)
    assert tuple(out["logits"].shape) == (B * props.shape[1], 1) == tuple(f["logits"].shape)
    if dt == "f32":
        gu.check_against(ops.nhwc_to_nchw_f32(out["pooled"]).cpu().numpy(), f, "pooled", 1e-3, 1e-3)
        np.testing.assert_allclose(out["logits"].cpu().numpy(), f["logits"], rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(out["box_regression"].cpu().numpy(), f["box_regression"], rtol=1e-3, atol=1e-3)
        for i in range(B):
            k = int(out["counts"][i])
            rb, rs = f["detections.%d.boxes" % i], f["detections.%d.scores" % i]
            assert abs(k - len(rb)) <= max(1, len(rb) // 100), (k, len(rb))
            got_b, got_s = out["boxes"][i, :k].cpu().numpy(), out["scores"][i, :k].cpu().numpy()
            assert np.all(got_s[:-1] >= got_s[1:])
            assert gu.match_boxes(rb, rs, got_b, got_s) >= 0.99
    else:
        np.testing.assert_allclose(out["logits"].cpu().numpy(), f["logits"], rtol=0, atol=0.06)
        assert np.abs(out["box_regression"].cpu().numpy() - f["box_regression"]).max() <= 0.03


def _train_fixture():
    name = "small"
    f = gu.load("boxtrain_small_focal.npz")
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


def _run_box_head(eng):
    name = "small"
    f, props, n_props, gt, gcnt, keys = _train_fixture()
    B, H, Wd, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    (feats, qfeats), _ = eng.backbones_forward(torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda())
    eng.flat_g.zero_()
    proposals = (torch.from_numpy(props).cuda(), None, torch.from_numpy(n_props).cuda())
    losses, gx, gqs = eng.box_head_forward_backward(feats, qfeats, [(qh, qw)] * (B * S), S, proposals, torch.from_numpy(gt).cuda(),
                                                    torch.from_numpy(gcnt).cuda(), keys=torch.from_numpy(keys).cuda(), want_debug=True)
    torch.cuda.synchronize()
    return f, losses, gx, gqs


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_focal_box_head_training_matches_the_reference_fixture(dt):
    """tests/test_gpu_box_train.py's comparison of the training box head, on boxtrain_small_focal.npz with a 'focal_loss' engine:
    sampled rows exact, both losses against the CUDA-formula values AND the reference's CPU-formula ones (they differ by 3e-6
    relative here), gradient samples of the 14 box-head parameter tensors (reference autograd), the feature-gradient maps."""
    from oneshotdet_amd import train
    eng = train.TrainEngine(_sd("focal_loss"), dtype=DT[dt], second_stage=True, box_cls_loss="focal_loss")
    f, losses, gx, gqs = _run_box_head(eng)
    B, S = gu.CASES["small"][0], gu.CASES["small"][3]
    for i in range(B):
        assert np.array_equal(eng.last_box["index"][i].cpu().numpy(), f["index.%d" % i])
        assert np.array_equal(eng.last_box["labels"][i].cpu().numpy(), f["labels.%d" % i])
    assert eng.last_box["pred"].shape[-1] >= 9 and eng.convs["roi_heads.box.pred"].cout == 9
    got = losses[:2].cpu().numpy()
    print(dt, "losses", got.tolist(), "cuda formula", f["losses_cuda_formula"].tolist(), "reference", f["losses"].tolist())
    np.testing.assert_allclose(got, f["losses_cuda_formula"], rtol=1e-4 if dt == "f32" else 3e-2)
    np.testing.assert_allclose(got, f["losses"], rtol=1e-4 if dt == "f32" else 3e-2)
    assert int(losses[2]) == B * int(f["n_sampled"])
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
            assert tuple(grads[k].shape) == tuple(spec.box_head_shapes(box_cls_loss="focal_loss")[k]), k
            idx = gu.sample_indices(g.size, "boxgrad." + k)[:256]
            check(g[idx], f[key], float(f["refgrad.%s.absmax" % k]), k)
            checked += 1
    assert checked == 14
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


def test_mse_train_step_classification_loss_is_the_closed_form():
    """One 'mse_loss' box-head step (fp32): the classification loss equals 5 x the closed form of the reference's [M, M]-broadcast
    mean on the step's OWN logits and labels — and not the row-wise mean.  rtol 1e-5: the kernel's bound."""
    from oneshotdet_amd import train
    eng = train.TrainEngine(_sd("mse_loss"), dtype=torch.float32, second_stage=True, box_cls_loss="mse_loss")
    f, losses, gx, gqs = _run_box_head(eng)
    lb = eng.last_box
    S = spec.BOX_BATCH_PER_IMAGE
    counts = lb["counts"].cpu().numpy()
    valid = torch.from_numpy(np.concatenate([np.arange(S) < int(c) for c in counts]))
    logits = lb["pred"].reshape(valid.numel(), -1)[:, :1].float().cpu()[valid]
    labels = lb["labels"].reshape(-1).cpu()[valid].long()
    assert 0 < int(labels.sum()) < len(labels)
    want = bcl.W_CLS * bcl.mse_loss_closed_form(logits.double(), labels).item()
    rowwise = bcl.W_CLS * ((torch.sigmoid(logits.double().reshape(-1)) - labels.double()) ** 2).mean().item()
    print("mse step: kernel %.7f closed form %.7f row-wise mean %.7f" % (float(losses[0]), want, rowwise))
    np.testing.assert_allclose(float(losses[0]), want, rtol=1e-5)
    assert abs(rowwise - want) > 1e-3 * want
    assert torch.isfinite(eng.named_grads()["roi_heads.box.predictor.cls_score.weight"]).all()


def test_focal_train_step_moves_the_box_head_and_leaves_the_first_stage_alone():
    """train_step in 'focal_loss' (bf16): every roi_heads.box.* parameter changes, the state_dict keeps the mode's shapes, and the
    first stage's three losses equal the default mode's on the same inputs (rtol 1e-5: the same launches on the same numbers)."""
    from oneshotdet_amd import train
    name = "small"
    B, H, Wd, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    gts = synth.make_gt_boxes(B, H, Wd, seed=3, max_boxes=3)
    gtb = torch.zeros(B, max(len(g) for g in gts), 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    cnt = torch.tensor([len(g) for g in gts], dtype=torch.int32)
    args = (torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), gtb.cuda(), cnt.cuda())
    keys = torch.rand((B, spec.POST_NMS_TOP_N_TRAIN + gtb.shape[1]), generator=torch.Generator().manual_seed(0)).cuda()
    foc = train.TrainEngine(_sd("focal_loss"), dtype=torch.bfloat16, second_stage=True, box_cls_loss="focal_loss")
    ce = train.TrainEngine(_sd("ce_loss"), dtype=torch.bfloat16, second_stage=True)
    foc.box_keys, ce.box_keys = keys, keys.clone()
    lf = foc.forward_backward(*args).cpu()
    lc = ce.forward_backward(*args).cpu()
    torch.cuda.synchronize()
    assert torch.isfinite(lf).all() and torch.isfinite(foc.box_losses).all() and float(foc.box_losses[0]) > 0
    torch.testing.assert_close(lf[:3], lc[:3], rtol=1e-5, atol=0)
    assert float(foc.box_losses[0]) != float(ce.box_losses[0])
    sd0 = foc.state_dict()
    shapes = spec.box_head_shapes(box_cls_loss="focal_loss")
    for _ in range(2):
        foc.train_step(*args)
    foc.join()
    torch.cuda.synchronize()
    sd1 = foc.state_dict()
    for key, shape in shapes.items():
        assert tuple(sd1[key].shape) == tuple(shape), key
        assert torch.isfinite(sd1[key]).all() and not torch.equal(sd1[key], sd0[key]), key
    assert sd1["roi_heads.box.predictor.cls_score.weight"].shape == (1, 1024)


def test_engines_refuse_a_cls_score_of_the_other_mode():
    """A 1-row cls_score in a default-mode engine (until now read as two logits, shifting every box delta by a column) and a 2-row
    one in a one-logit engine raise, naming the option; unknown and out-of-scope names raise before anything is built."""
    from oneshotdet_amd import model, modules, train
    one, two = _sd("focal_loss"), _sd("ce_loss")
    with pytest.raises(ValueError, match=r"box_cls_loss='ce_loss'.*'focal_loss' or 'mse_loss'"):
        model.HotPathEngine(one, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"2 row\(s\) but box_cls_loss='mse_loss'"):
        model.HotPathEngine(two, dtype=torch.bfloat16, box_cls_loss="mse_loss")
    with pytest.raises(ValueError, match="box_cls_loss='ce_loss'"):
        train.TrainEngine(one, dtype=torch.bfloat16, second_stage=True)
    with pytest.raises(ValueError, match="box_cls_loss='focal_loss'"):
        train.TrainEngine(two, dtype=torch.bfloat16, second_stage=True, box_cls_loss="focal_loss")
    with pytest.raises(ValueError, match="box_cls_loss='ce_loss'"):
        modules.OneShotDetector(one, dtype=torch.bfloat16)
    for bad in ("l1_loss", "cxe_loss", "hinge"):
        with pytest.raises(ValueError, match="box_cls_loss"):
            model.HotPathEngine(two, box_cls_loss=bad)
        with pytest.raises(ValueError, match="box_cls_loss"):
            train.TrainEngine(two, second_stage=True, box_cls_loss=bad)


def test_multi_shot_detection_in_a_one_logit_mode_raises_before_any_launch():
    """detect(second_stage=True) with 5 shots in 'focal_loss': ValueError citing box_head.py:246-253 (the reference itself raises
    IndexError there), and the launch trace stays empty.  One shot runs; training with 5 shots is unaffected (first query only)."""
    from oneshotdet_amd import model, trace
    B, H, Wd, S, qh, qw = gu.CASES["shots5"]
    assert S == 5
    img, q = gu.case_inputs("shots5")
    eng = model.HotPathEngine(_sd("focal_loss"), dtype=torch.bfloat16, box_cls_loss="focal_loss")
    images, queries = torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda()
    trace.TRACE = []
    try:
        with pytest.raises(ValueError, match=r"box_head\.py:246-253"):
            eng.detect(images, queries, second_stage=True)
        assert trace.TRACE == []
        out = eng.detect(images, queries[::S].contiguous(), second_stage=True)
        assert len(trace.TRACE) > 0
    finally:
        trace.TRACE = None
    torch.cuda.synchronize()
    k = int(out["detections"]["counts"][0])
    s = out["detections"]["scores"][0, :k]
    assert k > 0 and bool((s > 0).all()) and bool((s < 1).all())
