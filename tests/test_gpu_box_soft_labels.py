"""GPU (-m gpu): the second stage's IoU soft labels (soft_labeling / soft_labeling_func = FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC)
and the losses that read them — osd_box_match_sample_soft / osd_box_loss_soft against the fixture recorded through the REAL reference
(tests/golden/box_soft_labels.npz), the decode of the 'l1_loss' / 'cxe_loss' names, and the engines in 'cxe_loss' + 'transLinear'
against the end-to-end fixture boxtrain_small_cxe.npz (tests/golden/make_golden_box_soft_labels.py).

Tolerances.  Sampler: indices, labels and counts exact; soft labels 4.8e-7 absolute = 4 ulp at 1.0 (the values lie in [0, 1], the chain
has at most six float32 roundings and the 4th power is not the reference's pow bit for bit); soft labels of background rows and of
rows past the count exactly 0.  Losses, gradients, decode and engine: the bounds of tests/test_gpu_box_cls_modes.py for the same
quantities — kernel losses rtol 1e-5 against the float64 restatement, kernel gradients rtol 1e-5 / atol 1e-7 (fp32) and rtol 1e-2 / atol
1e-4 (bf16), decode scores 1e-6 and boxes 1e-4 px, engine losses rtol 1e-4 (fp32) / 3e-2 (bf16), parameter gradients 1e-3 x absmax
(fp32), relative L2 0.35 and cosine 0.96 (bf16)."""
import ctypes

import numpy as np
import pytest
import torch

import box_cls_loss_ref as bcl
import box_soft_label_ref as bsl
import golden_utils as gu
from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LOSS_CASES = ["mixed", "nopos", "allpos", "large"]
MATCH_CASES = ["iou", "iou_low", "wide"]
W = np.array([bcl.W_CLS, bcl.W_BOX])
SOFT_ATOL = 4.8e-7
E2E = ("cxe_loss", "transLinear")


@pytest.fixture(scope="module")
def fx():
    return gu.load("box_soft_labels.npz")


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------

def match_inputs(f, name):
    key = "match.%s." % name
    t = {k: torch.from_numpy(f[key + k]).cuda() for k in ("props", "counts", "gt", "gt_count", "keys")}
    return t, float(f[key + "thresh"]), int(f[key + "batch"]), float(f[key + "fraction"])


@pytest.mark.parametrize("func", bsl.FUNCS)
@pytest.mark.parametrize("name", MATCH_CASES)
def test_sampler_matches_the_reference_fixture(fx, name, func):
    """ops.box_match_sample(..., soft_func=func) on the reference's subsample: `iou` / `iou_low` are the 12 hand-made IoUs (1, 0.5,
    0.1, mid-range, below 0.1, 0) at the matcher thresholds 0.5 and 0.05 — the second reaches the middle and 4th-order branches —,
    `wide` has P = 1100 proposals (the second trip of the 1,024-thread proposal loop), different counts and an image without ground
    truth (nothing sampled).
    Measured on an MI355X: 'discrete' / 'linear' bit-equal, 'transLinear' / 'trans4thLinear' within 6.0e-8 (one ulp below 1)."""
    from oneshotdet_amd import ops
    t, thresh, batch, fraction = match_inputs(fx, name)
    sb, sl, st, si, sc, al, am, ss, as_ = ops.box_match_sample(t["props"], t["counts"], t["gt"], t["gt_count"], t["keys"], batch, fraction,
                                                               thresh, spec.BOX_REG_WEIGHTS, want_all=True, soft_func=func)
    torch.cuda.synchronize()
    key = "match.%s.%s." % (name, func)
    assert np.array_equal(sc.cpu().numpy(), fx[key + "count"])
    assert np.array_equal(si.cpu().numpy(), fx[key + "index"]) and np.array_equal(sl.cpu().numpy(), fx[key + "labels"])
    soft, want = ss.cpu().numpy(), fx[key + "soft"]
    all_soft, all_want = as_.cpu().numpy(), fx[key + "all_soft"]
    print("%s %s: worst soft-label error sampled %.3e, all proposals %.3e" % (name, func, np.abs(soft - want).max(), np.abs(all_soft - all_want).max()))
    np.testing.assert_allclose(soft, want, rtol=0, atol=SOFT_ATOL)
    np.testing.assert_allclose(all_soft, all_want, rtol=0, atol=SOFT_ATOL)
    lab = sl.cpu().numpy()
    assert (soft[lab <= 0] == 0).all()                          # background rows and rows past the count: exactly 0
    past = np.arange(all_soft.shape[1])[None, :] >= fx["match.%s.counts" % name][:, None]
    assert (all_soft[past] == 0).all() and (all_soft[al.cpu().numpy() <= 0] == 0).all()
    if func in ("discrete", "linear"):                          # no arithmetic: bit for bit
        assert np.array_equal(soft, want) and np.array_equal(all_soft, all_want)


def test_soft_entry_equals_the_plain_entry_bit_for_bit(fx):
    """osd_box_match_sample_soft called directly on `wide` (P = 1100, three images, one without ground truth): every output it shares
    with osd_box_match_sample is bit-equal to that entry's on the same inputs, with and without the per-proposal outputs."""
    from oneshotdet_amd import _lib, ops
    t, thresh, batch, fraction = match_inputs(fx, "wide")
    plain = ops.box_match_sample(t["props"], t["counts"], t["gt"], t["gt_count"], t["keys"], batch, fraction, thresh,
                                 spec.BOX_REG_WEIGHTS, want_all=True)
    n, p, _ = t["props"].shape
    outs = [torch.full_like(o, 7) for o in plain]
    s_soft = torch.full((n, batch), 7.0, device="cuda")
    all_soft = torch.full((n, p), 7.0, device="cuda")
    rw = (ctypes.c_float * 4)(*spec.BOX_REG_WEIGHTS)
    _lib.call("osd_box_match_sample_soft", t["props"].data_ptr(), t["counts"].data_ptr(), t["gt"].data_ptr(), t["gt_count"].data_ptr(),
              None, t["keys"].data_ptr(), n, p, t["gt"].shape[1], batch, fraction, thresh, rw, *[o.data_ptr() for o in outs],
              _lib.SOFT_LABEL_TRANS_LINEAR, s_soft.data_ptr(), all_soft.data_ptr(),
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for a, b in zip(plain, outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    np.testing.assert_allclose(s_soft.cpu().numpy(), fx["match.wide.transLinear.soft"], rtol=0, atol=SOFT_ATOL)
    np.testing.assert_allclose(all_soft.cpu().numpy(), fx["match.wide.transLinear.all_soft"], rtol=0, atol=SOFT_ATOL)
    # through the wrapper, without the per-proposal outputs: the same sampled rows
    short = ops.box_match_sample(t["props"], t["counts"], t["gt"], t["gt_count"], t["keys"], batch, fraction, thresh,
                                 spec.BOX_REG_WEIGHTS, soft_func="transLinear")
    assert len(short) == 6 and all(torch.equal(a, b) for a, b in zip(short[:5], plain[:5])) and torch.equal(short[5], s_soft)


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------

def loss_inputs(f, name, mode, stride, dt):
    """-> (pred [M, stride] with the row's L + 8 columns filled and 9.0 behind them, labels, soft, targets, counts, n, S, L, valid)"""
    S = int(f["loss.%s.S" % name])
    counts = torch.from_numpy(f["loss.%s.counts" % name])
    logits = torch.from_numpy(f["loss.%s.%s" % (name, "logits2" if mode == "cxe_loss" else "logits1")])
    L = logits.shape[1]
    pred = torch.full((logits.shape[0], stride), 9.0)
    pred[:, :L], pred[:, L:L + 8] = logits, torch.from_numpy(f["loss.%s.deltas" % name])
    valid = np.concatenate([np.arange(S) < int(c) for c in counts])
    return (pred.to(DT[dt]).cuda(), torch.from_numpy(f["loss.%s.labels" % name]).cuda(), torch.from_numpy(f["loss.%s.soft" % name]).cuda(),
            torch.from_numpy(f["loss.%s.targets" % name]).cuda(), counts.cuda(), len(counts), S, L, valid)


def check_loss_outputs(f, name, mode, dt, losses, d, L, valid):
    key = "loss.%s.%s" % (name, mode)
    want = f[key + ".losses_f64"] * W
    got = losses.cpu().numpy()
    g_log = f[key + ".grad_logits"].astype(np.float64)
    g_del = f["loss.%s.grad_deltas" % name].astype(np.float64)
    d = d.float().cpu().numpy().astype(np.float64)
    print("%s %s %s: losses %r want %r rel %.2e %.2e | worst gradient error logits %.3e (float64 closed form %.3e) deltas %.3e"
          % (name, mode, dt, got[:2].tolist(), want.tolist(), abs(got[0] - want[0]) / max(abs(want[0]), 1e-30),
             abs(got[1] - want[1]) / max(abs(want[1]), 1e-30), np.abs(d[:, :L] - g_log).max(),
             np.abs(d[:, :L] - f[key + ".grad_logits_f64"]).max(), np.abs(d[:, L:L + 8] - g_del).max()))
    np.testing.assert_allclose(got[:2], want, rtol=1e-5)
    assert int(got[2]) == int(valid.sum())
    tol = dict(rtol=1e-5, atol=1e-7) if dt == "f32" else dict(rtol=1e-2, atol=1e-4)
    np.testing.assert_allclose(d[:, :L], g_log, **tol)
    np.testing.assert_allclose(d[:, L:L + 8], g_del, **tol)
    assert not d[:, L + 8:].any() and not d[~valid].any()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", bsl.SOFT_LOSSES)
@pytest.mark.parametrize("name", LOSS_CASES)
def test_loss_kernel_matches_the_reference_fixture(fx, name, mode, dt):
    """ops.box_loss(..., soft=) for 'mse_loss' with soft labels, 'l1_loss' and 'cxe_loss': both losses against the float64 restatement of
    the reference's broadcasts, the valid-row count, the reference's autograd w.r.t. the logits and the deltas, zero rows past the count
    (they hold label 1 and soft label 0.7: a read of them as t_j, or a mean over them, shows), zero columns behind the row.  `mixed`
    row 0 is the pair (sigmoid 0.5, soft label 0.5): sign(0) = 0.  `large` is M = 1152 valid rows: the second trip of the row loop
    and, for 'l1_loss', the second tile of 1,024 soft labels (1152^2 pairs).
    Measured on an MI355X (fp32, worst over the cases): losses 8.2e-8 (mse), 8.7e-8 (l1; the 1152^2-pair sum: 1.1e-8), 8.5e-8 (cxe)
    relative; logit gradients within 6.0e-8 absolute of the reference's autograd.  The 1e-5 bound holds as it stands."""
    from oneshotdet_amd import ops
    pred, labels, soft, targets, counts, n, S, L, valid = loss_inputs(fx, name, mode, bsl.n_logits(mode) + 8, dt)
    losses, d = ops.box_loss(pred, labels, targets, counts, n, S, bcl.W_CLS, bcl.W_BOX, grad_stride=16, cls_loss=mode, soft=soft)
    check_loss_outputs(fx, name, mode, dt, losses, d, L, valid)
    # without the gradient: the same losses, bit for bit
    l2, none = ops.box_loss(pred, labels, targets, counts, n, S, bcl.W_CLS, bcl.W_BOX, cls_loss=mode, soft=soft)
    assert none is None and torch.equal(l2, losses)
    # the quirks: the value is not the row-wise mean / not the full soft cross-entropy
    p = pred.float().cpu()[valid]
    row = bcl.W_CLS * bsl.rowwise_value(p[:, :L].double(), soft.cpu()[valid].double(), mode).item()
    if mode == "cxe_loss":
        np.testing.assert_allclose(float(losses[0]), row / 2, rtol=1e-5)
    elif name != "nopos":
        assert abs(float(losses[0]) - row) > 1e-3 * row


@pytest.mark.parametrize("mode", bsl.SOFT_LOSSES)
def test_c_entry_with_padded_strides_bad_labels_and_invalid_rows(fx, mode):
    """osd_box_loss_soft called directly: pred_stride 16 and grad_stride 12 (both wider than the row), d_pred pre-filled.  Every row
    of d_pred is written: gradients in the valid rows, zeros past the count and behind the row.  Then one valid row gets label 2: both
    losses come back NaN, its gradient row is zero and every other row's box gradient is what it was."""
    from oneshotdet_amd import _lib
    name = "mixed"
    pred, labels, soft, targets, counts, n, S, L, valid = loss_inputs(fx, name, mode, 16, "f32")
    code = {"mse_loss": _lib.BOX_CLS_MSE, "l1_loss": _lib.BOX_CLS_L1, "cxe_loss": _lib.BOX_CLS_CXE}[mode]

    def run(lab):
        losses = torch.full((3,), 7.0, device="cuda")
        d = torch.full((n * S, 12), 7.0, device="cuda")
        _lib.call("osd_box_loss_soft", pred.data_ptr(), lab.data_ptr(), targets.data_ptr(), counts.data_ptr(), n, S, 16,
                  bcl.W_CLS, bcl.W_BOX, losses.data_ptr(), d.data_ptr(), 12, _lib.OSD_F32, soft.data_ptr(), code,
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
    assert torch.equal(d2[others][:, L:], d[others][:, L:])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("mode", spec.BOX_CLS_LOSSES_SOFT)
def test_decode_of_the_soft_loss_names_matches_the_reference_fixture(fx, mode, dt):
    """ops.box_decode(..., cls_loss='l1_loss' / 'cxe_loss', soft_labeling=True) on the reference's PostProcessor output: 'l1_loss'
    scores like 'mse_loss' (sigmoid of the one logit), 'cxe_loss' like 'ce_loss' (softmax of the two) — no new kernel."""
    from oneshotdet_amd import ops
    L = bsl.n_logits(mode)
    n, R = fx["decode.rois"].shape[:2]
    pred = torch.full((1, n * R, L + 8), 9.0)
    pred[0, :, :L], pred[0, :, L:] = torch.from_numpy(fx["decode.%s.logits" % mode])[0], torch.from_numpy(fx["decode.deltas"])
    ih, iw = (int(v) for v in fx["decode.image_size"])
    counts = torch.from_numpy(fx["decode.counts"])
    args = (pred.to(DT[dt]).cuda(), torch.from_numpy(fx["decode.rois"]).cuda(), counts.cuda(), spec.BOX_REG_WEIGHTS, ih, iw,
            spec.BOX_SCORE_THRESH)
    scores, boxes, lo, ro = ops.box_decode(*args, want_raw=True, cls_loss=mode, soft_labeling=True)
    live = np.arange(R)[None, :] < counts.numpy()[:, None]
    s, b = scores.cpu().numpy(), boxes.cpu().numpy()
    assert (s[~live] == -1).all()
    np.testing.assert_allclose(s[live], fx["decode.%s.scores" % mode][live], rtol=0, atol=1e-6)
    np.testing.assert_allclose(b[live], fx["decode.%s.boxes" % mode][live], rtol=0, atol=1e-4)
    assert tuple(lo.shape) == (n * R, L) and torch.equal(lo.cpu(), pred[0, :, :L]) and torch.equal(ro.cpu(), pred[0, :, L:])
    same = ops.box_decode(*args, cls_loss=bsl.decode_mode(mode))            # the launch of the mode it maps to
    assert torch.equal(same[0], scores) and torch.equal(same[1], boxes)
    with pytest.raises(ValueError, match="SOFT_LABELING"):
        ops.box_decode(*args, cls_loss=mode)


# ---- the engines ------------------------------------------------------------------------------------------------------------------------

def _sd(mode, soft=True):
    return synth.make_state_dict(spec.full_model_shapes(box_cls_loss=mode, soft_labeling=soft))


def _train_fixture(fname):
    name = "small"
    f = gu.load(fname)
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


def _run_box_head(eng, fname="boxtrain_small_cxe.npz"):
    name = "small"
    f, props, n_props, gt, gcnt, keys = _train_fixture(fname)
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
def test_cxe_translinear_box_head_training_matches_the_reference_fixture(dt):
    """tests/test_gpu_box_train.py's comparison of the training box head, on boxtrain_small_cxe.npz with a 'cxe_loss' + 'transLinear'
    engine: sampled rows and labels exact, the soft labels the sampler handed to the loss (4.8e-7), both losses, gradient samples of
    the 14 box-head parameter tensors (reference autograd), the feature-gradient maps."""
    from oneshotdet_amd import train
    eng = train.TrainEngine(_sd(E2E[0]), dtype=DT[dt], second_stage=True, box_cls_loss=E2E[0], soft_labeling=True,
                            soft_labeling_func=E2E[1])
    f, losses, gx, gqs = _run_box_head(eng)
    B, S = gu.CASES["small"][0], gu.CASES["small"][3]
    for i in range(B):
        k = len(f["index.%d" % i])
        assert np.array_equal(eng.last_box["index"][i].cpu().numpy()[:k], f["index.%d" % i])
        assert np.array_equal(eng.last_box["labels"][i].cpu().numpy()[:k], f["labels.%d" % i])
        np.testing.assert_allclose(eng.last_box["soft"][i].cpu().numpy()[:k], f["soft.%d" % i], rtol=0, atol=SOFT_ATOL)
    assert eng.last_box["pred"].shape[-1] >= 10 and eng.convs["roi_heads.box.pred"].cout == 10
    got = losses[:2].cpu().numpy()
    print(dt, "losses", got.tolist(), "reference", f["losses"].tolist())
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
            assert tuple(grads[k].shape) == tuple(spec.box_head_shapes(box_cls_loss=E2E[0], soft_labeling=True)[k]), k
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


def test_l1_train_step_classification_loss_is_the_pair_mean():
    """One 'l1_loss' box-head step (fp32, 'linear' soft labels): the classification loss equals 5 x the reference's [M, M]-broadcast
    mean of |sigmoid - soft label| on the step's OWN logits and soft labels — and not the row-wise mean.  rtol 1e-5: the kernel's bound."""
    from oneshotdet_amd import train
    eng = train.TrainEngine(_sd("l1_loss"), dtype=torch.float32, second_stage=True, box_cls_loss="l1_loss", soft_labeling=True)
    assert eng.soft_labeling_func == "linear" and eng.convs["roi_heads.box.pred"].cout == 9
    f, losses, gx, gqs = _run_box_head(eng)
    lb = eng.last_box
    S = spec.BOX_BATCH_PER_IMAGE
    counts = lb["counts"].cpu().numpy()
    valid = torch.from_numpy(np.concatenate([np.arange(S) < int(c) for c in counts]))
    logits = lb["pred"].reshape(valid.numel(), -1)[:, :1].float().cpu()[valid]
    soft = lb["soft"].reshape(-1).cpu()[valid]
    labels = lb["labels"].reshape(-1).cpu()[valid]
    assert 0 < int((labels > 0).sum()) < len(labels) and bool((soft[labels > 0] >= 0.5).all()) and bool((soft[labels == 0] == 0).all())
    assert bool((soft[labels > 0] < 1).any())                 # 'linear': the IoU itself, not the hard label
    want = bcl.W_CLS * bsl.cls_loss_value(logits.double(), soft.double(), "l1_loss").item()
    rowwise = bcl.W_CLS * bsl.rowwise_value(logits.double(), soft.double(), "l1_loss").item()
    print("l1 step: kernel %.7f pair mean %.7f row-wise mean %.7f" % (float(losses[0]), want, rowwise))
    np.testing.assert_allclose(float(losses[0]), want, rtol=1e-5)
    # "not the row-wise mean" = the kernel's value fails the same comparison against it, by ten times the bound (most of the step's
    # soft labels are 0, the background rows', so the two means lie within 1e-3 of each other here: 2.8424 / 2.8399)
    assert abs(float(losses[0]) - rowwise) > 10 * 1e-5 * abs(rowwise)
    assert torch.isfinite(eng.named_grads()["roi_heads.box.predictor.cls_score.weight"]).all()


def test_soft_labeling_with_ce_loss_makes_the_default_launches():
    """soft_labeling=True with 'ce_loss' (the reference computes soft labels there and never reads them): the box-head step's losses are
    bit-identical to the default engine's and its launch trace has the same kinds in the same order — no soft launch —, while a
    'cxe_loss' engine's trace has the two soft launches."""
    from oneshotdet_amd import trace, train

    def run(**kw):
        eng = train.TrainEngine(_sd(kw.get("box_cls_loss", "ce_loss"), soft=kw.get("soft_labeling", False)), dtype=torch.bfloat16,
                                second_stage=True, **kw)
        trace.TRACE = []
        try:
            _, losses, _, _ = _run_box_head(eng)
            kinds = [k for k, _ in trace.TRACE]
        finally:
            trace.TRACE = None
        return losses.clone(), kinds, eng
    l0, k0, _ = run()
    l1, k1, e1 = run(soft_labeling=True, soft_labeling_func="trans4thLinear")
    assert e1.soft_labeling is True and e1.soft_labeling_func == "trans4thLinear" and e1.last_box["soft"] is None
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and k0 == k1 and len(k0) > 10
    assert not any(k.endswith("_soft") for k in k0)
    l2, k2, e2 = run(box_cls_loss="cxe_loss", soft_labeling=True)
    assert [k for k in k2 if k.endswith("_soft")] == ["box_match_sample_soft", "box_loss_soft"]
    assert [k for k in k2 if not k.endswith("_soft")] == k0 and float(l2[0]) != float(l0[0])


def test_engines_accept_the_soft_loss_names_with_soft_labeling_only():
    """'l1_loss' / 'cxe_loss' build with soft_labeling=True and raise without it, before anything is built; a 'cxe_loss' detector is the
    'ce_loss' detector of the same weights (inference.py:65-66), bit for bit."""
    from oneshotdet_amd import model, modules, train
    one, two = _sd("l1_loss"), _sd("cxe_loss")
    for bad, sd in (("l1_loss", one), ("cxe_loss", two)):
        with pytest.raises(ValueError, match="SOFT_LABELING"):
            model.HotPathEngine(sd, box_cls_loss=bad)
        with pytest.raises(ValueError, match="SOFT_LABELING"):
            train.TrainEngine(sd, second_stage=True, box_cls_loss=bad)
        with pytest.raises(ValueError, match="SOFT_LABELING"):
            modules.OneShotDetector(sd, box_cls_loss=bad)
    with pytest.raises(ValueError, match="soft_labeling_func must be one of"):
        train.TrainEngine(two, second_stage=True, box_cls_loss="cxe_loss", soft_labeling=True, soft_labeling_func="cubic")
    with pytest.raises(ValueError, match=r"2 row\(s\) but box_cls_loss='l1_loss'"):
        model.HotPathEngine(two, dtype=torch.bfloat16, box_cls_loss="l1_loss", soft_labeling=True)
    B, H, Wd, S, qh, qw = gu.CASES["small"]
    img, q = gu.case_inputs("small")
    images, queries = torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda()
    a = model.HotPathEngine(two, dtype=torch.bfloat16, box_cls_loss="cxe_loss", soft_labeling=True).detect(images, queries, second_stage=True)
    b = model.HotPathEngine(two, dtype=torch.bfloat16).detect(images, queries, second_stage=True)
    torch.cuda.synchronize()
    for k in ("boxes", "scores", "counts"):
        assert torch.equal(a["detections"][k], b["detections"][k]), k
    det = modules.OneShotDetector(one, dtype=torch.bfloat16, box_cls_loss="l1_loss", soft_labeling=True)
    assert det.engine.box_head.box_cls_loss == "l1_loss" and det.second_stage
