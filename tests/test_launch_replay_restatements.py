"""CPU: the launch restatements the option replays stand on (oracle/launch_replay.py; tests/test_gpu_launch_replay_options.py
holds the engines' launches to them), each against something that is not itself:
  fcos_loss_grad_launch in all six (FCOS.CENTER_SAMPLE, FCOS.LOC_LOSS_TYPE) modes against the gradients recorded through the real
      reference (fcos_loss_modes.npz), chained through reg = exp(scale * x) as tests/test_gpu_fcos_loss_modes.py chains them, at the
      bound that test applies to the fp32 kernels (lr.compare, float32); the Scale's raw sum at its 1e-4 x sum |terms|
  the average-pooling and query-augmentation merges against torch autograd of the reference's expressions in float64
  the class sweep's and the gallery's correlation against an explicit loop over (image, class)
and an inventory: every launch kind `ops.py` records has a restatement in tests/launch_replayer.py or a reason not to."""
import os
import re

import numpy as np
import pytest
import torch

import fcos_loss_ref as flr
import golden_utils as gu
import launch_replayer as rpl
import supp_aug_ref as sar
from oracle import launch_replay as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (1.0, 0.75, 1.25, 0.5, 1.5)          # the Scale values tests/test_gpu_fcos_loss_modes.py gives the five levels


# ---------------------------------------------------------------------------------------------------------------- FCOS loss
def _fixture_case(f, name):
    """-> head_out [(cls_ctr [N,h,w,4], reg [N,h,w,4])] per level, gt_boxes [N,G,4], gt_count [N], per_level(flat, c)"""
    hw = [tuple(int(v) for v in r) for r in f[name + ".hw"]]
    gb = f[name + ".gt_boxes"]
    N = int(gb[:, 0].max()) + 1
    gts = [gb[gb[:, 0] == i, 1:] for i in range(N)]
    gtb = torch.zeros(N, max(len(g) for g in gts), 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    cnt = torch.tensor([len(g) for g in gts], dtype=torch.int32)

    def per_level(flat, c):
        t, out, beg = torch.from_numpy(np.asarray(flat)).reshape(-1, c), [], 0
        for h, w in hw:
            out.append(t[beg:beg + N * h * w].reshape(N, h, w, c))
            beg += N * h * w
        assert beg == t.shape[0]
        return out
    lg, ct, rg = per_level(f[name + ".logits"], 1), per_level(f[name + ".centerness"], 1), per_level(f[name + ".bbox_reg"], 4)
    head = [(torch.cat([a, b, torch.zeros_like(a), torch.zeros_like(a)], 3), r) for a, b, r in zip(lg, ct, rg)]
    return head, gtb, cnt, per_level


@pytest.mark.parametrize("name", ["quirks", "random"])
@pytest.mark.parametrize("center_sample,loc_loss_type", flr.MODES)
def test_loss_gradient_launch_reproduces_the_reference_gradients_in_every_mode(center_sample, loc_loss_type, name):
    f = gu.load("fcos_loss_modes.npz")
    head, gtb, cnt, per_level = _fixture_case(f, name)
    nl = len(head)
    outs, raws, raw_abs, losses = lr.fcos_loss_grad_launch(head, gtb, cnt, SCALES[:nl], 2.0, 0.25, center_sample=center_sample,
                                                           loc_loss_type=loc_loss_type)
    key = "%s.cs%d" % (name, center_sample)
    mkey = "%s.%s" % (key, loc_loss_type)
    assert losses[3] == int(f[mkey + ".num_pos"]) == int(f[key + ".labels"].sum()) > 0
    np.testing.assert_allclose(losses[:3], f[mkey + ".losses_cuda_formula"], rtol=1e-5)
    g_logit = per_level(f[key + ".grad_logits_cuda_formula"], 1)
    g_ctr = per_level(f[mkey + ".grad_centerness"], 1)
    g_reg = per_level(f[mkey + ".grad_bbox_reg"], 4)
    for l, (d_cc, d_x) in enumerate(outs):
        assert d_cc.shape == head[l][0].shape[:3] + (2,) and d_x.shape == head[l][1].shape
        ds = g_reg[l] * head[l][1]                                            # chain through reg = exp(scale * x)
        for got, ref, what in ((d_cc[..., 0:1], g_logit[l], "logits"), (d_cc[..., 1:2], g_ctr[l], "centerness"),
                               (d_x, ds * SCALES[l], "bbox conv output")):
            res = lr.compare(got, ref, torch.float32)
            assert res["ok"], (l, what, res)
        terms = ds.double() * head[l][1].double().log()
        assert abs(raws[l] - float(terms.sum())) <= 1e-4 * float(terms.abs().sum()) + 1e-12, (l, raws[l], float(terms.sum()))
        assert abs(raw_abs[l] - float(terms.abs().sum())) <= 1e-4 * float(terms.abs().sum()) + 1e-12
    assert any(a > 0 for a in raw_abs)


def test_loss_gradient_launch_defaults_to_the_mode_of_record():
    f = gu.load("fcos_loss_modes.npz")
    head, gtb, cnt, _ = _fixture_case(f, "random")
    a = lr.fcos_loss_grad_launch(head, gtb, cnt, SCALES, 2.0, 0.25)
    b = lr.fcos_loss_grad_launch(head, gtb, cnt, SCALES, 2.0, 0.25, center_sample=True, loc_loss_type="giou")
    c = lr.fcos_loss_grad_launch(head, gtb, cnt, SCALES, 2.0, 0.25, center_sample=False, loc_loss_type="iou")
    assert a[3] == b[3] and a[1] == b[1] and a[3] != c[3]
    for (x0, y0), (x1, y1) in zip(a[0], b[0]):
        assert torch.equal(x0, x1) and torch.equal(y0, y1)


# ---------------------------------------------------------------------------------------------------------------- pooling / merge
@pytest.mark.parametrize("batch,shots,sizes", [(2, 3, [(5, 7), (3, 4), (1, 1)]), (3, 1, [(2, 3), (1, 1)]), (1, 2, [(1, 1)])])
def test_avgpool_launches_equal_autograd_of_the_two_means(batch, shots, sizes):
    """nn.AdaptiveAvgPool2d((1, 1)) + the mean over the shots (generalized_rcnn.py:87-94, 100-104) and their backward, float64."""
    g = torch.Generator().manual_seed(11)
    c = 8
    xs = [torch.randn(batch * shots, h, w, c, generator=g) for h, w in sizes]
    dqs = [torch.randn(batch, c, generator=g) for _ in sizes]
    leaves = [x.double().requires_grad_(True) for x in xs]
    want = [x.permute(0, 3, 1, 2).mean(dim=(2, 3)).view(batch, shots, c).mean(dim=1) for x in leaves]
    sum((w_ * d.double()).sum() for w_, d in zip(want, dqs)).backward()
    got = lr.query_avgpool_launch(xs, batch)
    grads = lr.query_avgpool_bwd_launch(dqs, [tuple(x.shape) for x in xs], shots)
    for y, w_, gx, x in zip(got, want, grads, leaves):
        assert y.dtype == torch.float32 and tuple(y.shape) == (batch, c) and gx.dtype == torch.float32 and gx.shape == x.shape
        torch.testing.assert_close(y.double(), w_.detach(), rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(gx.double(), x.grad, rtol=1e-6, atol=1e-9)
    # bf16 maps go in as they are stored: the same function of the same values
    xb = [x.bfloat16() for x in xs]
    for a, b in zip(lr.query_avgpool_launch(xb, batch), lr.query_avgpool_launch([x.float() for x in xb], batch)):
        assert torch.equal(a, b)


def _merge_case(aug, groups, sizes, seed):
    g = torch.Generator().manual_seed(seed)
    c = 8
    xs = [torch.randn(groups * aug, h, w, c, generator=g) for h, w in sizes]
    dys = [torch.randn(groups, h, w, c, generator=g) for h, w in sizes]
    return xs, dys


@pytest.mark.parametrize("aug,groups,sizes", [(2, 3, [(4, 5), (1, 1)]), (3, 2, [(2, 3), (1, 1)]), (1, 4, [(3, 2), (1, 1)])])
@pytest.mark.parametrize("method", ["avg", "max"])
def test_supp_aug_launches_equal_autograd_of_the_merge(method, aug, groups, sizes):
    """generalized_rcnn.py:280-288 in float64 through torch autograd (max: torch's CPU max(dim) backward).  Every map carries a
    planted tie in a 'max' group — members 0 and the last equal at the maximum: all of dy goes to member 0."""
    xs, dys = _merge_case(aug, groups, sizes, seed=5)
    for x in xs:                                   # group 1, channel 3 of every pixel: every member holds the same, largest value
        x.view(groups, aug, *x.shape[1:])[1, :, ..., 3] = 9.0
    leaves = [x.double().requires_grad_(True) for x in xs]
    want = [sar.merge(x, aug, method) for x in leaves]
    sum((w_ * d.double()).sum() for w_, d in zip(want, dys)).backward()
    got = lr.supp_aug_reduce_launch(xs, aug, method)
    grads = lr.supp_aug_reduce_bwd_launch(xs, dys, aug, method)
    for x, y, w_, gx, leaf, dy in zip(xs, got, want, grads, leaves, dys):
        assert tuple(y.shape) == (groups,) + tuple(x.shape[1:]) and gx.shape == x.shape
        if method == "max" or aug == 1:
            assert torch.equal(y.double(), w_.detach())
            assert torch.equal(gx.double(), leaf.grad)
        else:
            assert torch.equal(y, torch.from_numpy(sar.avg_closed_form(x.numpy(), aug)))       # member order, one division
            torch.testing.assert_close(y.double(), w_.detach(), rtol=1e-6, atol=1e-7)
            torch.testing.assert_close(gx.double(), leaf.grad, rtol=1e-6, atol=0)
        gg = gx.view(groups, aug, *x.shape[1:])
        if method == "max":                        # the planted tie: member 0 takes it all, the others nothing
            assert torch.equal(gg[1, 0, ..., 3], dy[1, ..., 3])
            assert aug == 1 or float(gg[1, 1:, ..., 3].abs().max()) == 0.0
            assert torch.equal(gg.sum(dim=1), dy)  # every element of dy lands on exactly one member
        if aug == 1:
            assert torch.equal(y, x) and torch.equal(gx, dy)


def test_supp_aug_max_backward_on_rounded_maps_with_many_ties():
    """bf16 storage makes ties common (the tie rule matters): on maps rounded to few distinct values the restatement is still
    torch's CPU max backward, element for element, and 'avg' of two members is exact."""
    xs, dys = _merge_case(2, 4, [(6, 6)], seed=9)
    xs = [(x * 2).round().bfloat16() for x in xs]
    dys = [d.bfloat16() for d in dys]
    x, dy = xs[0], dys[0]
    g = x.float().view(4, 2, 6, 6, 8)
    assert int((g[:, 0] == g[:, 1]).sum()) > 20
    leaf = x.float().requires_grad_(True)
    sar.merge(leaf, 2, "max").backward(dy.float())
    assert torch.equal(lr.supp_aug_reduce_bwd_launch(xs, dys, 2, "max")[0], leaf.grad)
    assert torch.equal(lr.supp_aug_reduce_launch(xs, 2, "max")[0], sar.merge(x.float(), 2, "max"))
    assert torch.equal(lr.supp_aug_reduce_launch(xs, 2, "avg")[0], sar.merge(x.float(), 2, "avg"))
    assert torch.equal(lr.supp_aug_reduce_bwd_launch(xs, dys, 2, "avg")[0].view(4, 2, 6, 6, 8)[:, 1], dy.float() / 2)
    with pytest.raises(ValueError):
        lr.supp_aug_reduce_launch(xs, 2, "conv")


# ---------------------------------------------------------------------------------------------------------------- sweep / gallery
def test_sweep_and_gallery_launches_equal_a_loop_over_image_and_class():
    """row b * K + k = x[b] * q[b * K + k] (sweep) / x[b] * q[slots[b * K + k]] (gallery): K = 9, a table that repeats a slot within
    an image and runs against the row order."""
    g = torch.Generator().manual_seed(3)
    B, K, G, c = 2, 9, 5, 8
    x = torch.randn(B, 3, 4, c, generator=g).bfloat16()
    q = torch.randn(B * K, c, generator=g)
    got = lr.correlate_sweep_launch(x, q, K)
    assert tuple(got.shape) == (B * K, 3, 4, c) and got.dtype == torch.float32
    for b in range(B):
        for k in range(K):
            want = x[b].float() * q[b * K + k][None, None, :]
            assert torch.equal(got[b * K + k], want), (b, k)
    bank = torch.randn(G, c, generator=g)
    slots = torch.tensor([4, 2, 2, 0, 3, 1, 4, 4, 0, 1, 0, 3, 3, 2, 4, 0, 1, 2], dtype=torch.int32)
    assert slots.numel() == B * K and len(set(slots[:K].tolist())) < K and (slots[1:] < slots[:-1]).any()
    got = lr.correlate_gallery_launch(x, bank, slots, K)
    for b in range(B):
        for k in range(K):
            want = x[b].float() * bank[int(slots[b * K + k])][None, None, :]
            assert torch.equal(got[b * K + k], want), (b, k)
    # classes = 1 is the per-pair launch
    assert torch.equal(lr.correlate_sweep_launch(x, q[:B], 1), lr.correlate_launch(x, q[:B]))


# ---------------------------------------------------------------------------------------------------------------- the replayer
# The Replayer's methods on hand-made records (CPU tensors): a record that holds what the restatement gives passes, and each way a
# kernel or the engine's schedule could be subtly wrong is a recorded failure.
BF = torch.bfloat16


def _failed(kind, rec, engine=None):
    rp = rpl.Replayer(engine=engine)
    rp.run([(kind, rec)])
    rp.check_accumulated()
    return [f[0] for f in rp.failures], rp


class _ScaleGradOnly(object):
    """what the Replayer reads of a TrainEngine: the (parameter, gradient) views of the Scale scalars"""

    def __init__(self, grad):
        self.extra = {rpl.SCALES: (torch.ones_like(grad), grad)}


def _loss_record(center_sample, loc_loss_type, dtype=BF):
    f = gu.load("fcos_loss_modes.npz")
    head, gtb, cnt, _ = _fixture_case(f, "quirks")
    head = [(cc.to(dtype), rg.to(dtype)) for cc, rg in head]           # the fixture's inputs are bfloat16 values: nothing is lost
    outs, raws, raw_abs, _ = lr.fcos_loss_grad_launch(head, gtb, cnt, SCALES, 2.0, 0.25, center_sample=center_sample,
                                                      loc_loss_type=loc_loss_type)
    d_cc, d_rg = [], []
    for a, b in outs:                                                  # the engine's buffers: 8 channels, the real ones in front
        d_cc.append(torch.cat([a, torch.zeros(a.shape[:3] + (6,))], 3).to(dtype))
        d_rg.append(torch.cat([b, torch.zeros(b.shape[:3] + (4,))], 3).to(dtype))
    rec = dict(phase=1, head_out=head, gt_boxes=gtb, gt_count=cnt, gamma=2.0, alpha=0.25, sums=None, d_cls_ctrs=d_cc, d_regs=d_rg,
               scale_devs=[torch.tensor([s]) for s in SCALES], d_scale_raws=[torch.tensor([r], dtype=torch.float32) for r in raws],
               center_sample=center_sample, loc_loss_type=loc_loss_type)
    grad = torch.tensor([r / s for r, s in zip(raws, SCALES)], dtype=torch.float32)
    return rec, raw_abs, grad


@pytest.mark.parametrize("center_sample,loc_loss_type", [(True, "giou"), (False, "iou"), (True, "linear_iou")])
def test_replayer_holds_the_loss_launch_to_the_records_mode_and_accounts_for_the_scale_gradient(center_sample, loc_loss_type):
    rec, raw_abs, grad = _loss_record(center_sample, loc_loss_type)
    failed, rp = _failed("fcos_loss", rec, _ScaleGradOnly(grad))
    assert not failed, rp.failures[:3]
    assert rp.counts == {"fcos_loss_grad": 10, "fcos_scale_raw": 5} and rp.loss_info[3] > 0
    assert list(rp.acc) == [grad.data_ptr()] and rp.acc[grad.data_ptr()][1].numel() == 5
    assert not _failed("fcos_loss", dict(rec, phase=0))[1].counts                    # phase 0 writes sums only
    # gradients of ANOTHER mode under this record's mode
    other = (not center_sample, loc_loss_type) if loc_loss_type != "giou" else (True, "iou")
    assert "fcos_loss_grad" in _failed("fcos_loss", dict(rec, center_sample=other[0], loc_loss_type=other[1]))[0]
    # one location of the persistent buffer not rewritten (it keeps an earlier step's value)
    lvl = max(range(5), key=lambda l: float(rec["d_regs"][l].float().abs().max()))
    stale = [t.clone() for t in rec["d_regs"]]
    flat = stale[lvl].view(-1, 8)
    flat[int(flat[:, :4].float().abs().sum(1).argmax()), :4] = 0
    assert "fcos_loss_grad" in _failed("fcos_loss", dict(rec, d_regs=stale))[0]
    # the padding channels are not the launch's to check; a Scale raw sum off by three times its bound is
    lvl = max(range(5), key=lambda l: raw_abs[l])
    raws = [t.clone() for t in rec["d_scale_raws"]]
    raws[lvl] += 3e-4 * raw_abs[lvl]
    assert _failed("fcos_loss", dict(rec, d_scale_raws=raws))[0] == ["fcos_scale_raw"]
    # the finalize launch forgot a level / added into a gradient that was not zero
    bad = grad.clone()
    bad[int(grad.abs().argmax())] *= 1.001
    assert "accumulated gradient" in _failed("fcos_loss", rec, _ScaleGradOnly(bad))[0]


def test_replayer_flags_wrong_pooling_merge_and_correlation_launches():
    g = torch.Generator().manual_seed(21)
    # ---- average pooling: batch 2, shots 2, levels 4 x 3 and 1 x 1
    xs = [torch.randn(4, 4, 3, 8, generator=g).to(BF), torch.randn(4, 1, 1, 8, generator=g).to(BF)]
    rec = dict(xs=xs, batch=2, outs=lr.query_avgpool_launch(xs, 2))
    assert not _failed("query_avgpool", rec)[0]
    no_shots = [x.float().mean(dim=(1, 2))[0::2].contiguous() for x in xs]                      # the first shot only
    assert "query_avgpool" in _failed("query_avgpool", dict(rec, outs=no_shots))[0]
    dqs = [torch.randn(2, 8, generator=g) for _ in xs]
    good = [t.to(BF) for t in lr.query_avgpool_bwd_launch(dqs, [tuple(x.shape) for x in xs], 2)]
    assert not _failed("query_avgpool_bwd", dict(dqs=dqs, shots=2, outs=good))[0]
    assert "query_avgpool_bwd" in _failed("query_avgpool_bwd", dict(dqs=dqs, shots=2, outs=[(t.float() * 2).to(BF) for t in good]))[0]
    swapped = [t.view(2, 2, *t.shape[1:]).flip(0).reshape(t.shape).contiguous() for t in good]   # image 1's gradient in image 0's maps
    assert "query_avgpool_bwd" in _failed("query_avgpool_bwd", dict(dqs=dqs, shots=2, outs=swapped))[0]
    # ---- merge: 3 groups of 2, maps rounded so that members tie
    xs = [(torch.randn(6, 5, 4, 8, generator=g) * 2).round().to(BF), (torch.randn(6, 1, 1, 8, generator=g) * 2).round().to(BF)]
    dys = [torch.randn(3, 5, 4, 8, generator=g).to(BF), torch.randn(3, 1, 1, 8, generator=g).to(BF)]
    for method in ("avg", "max"):
        outs = [t.to(BF) for t in lr.supp_aug_reduce_launch(xs, 2, method)]
        assert not _failed("supp_aug_reduce", dict(xs=xs, aug=2, method=method, outs=outs))[0]
        other = [t.to(BF) for t in lr.supp_aug_reduce_launch(xs, 2, "max" if method == "avg" else "avg")]
        assert "supp_aug_reduce" in _failed("supp_aug_reduce", dict(xs=xs, aug=2, method=method, outs=other))[0]
        dxs = [t.to(BF) for t in lr.supp_aug_reduce_bwd_launch(xs, dys, 2, method)]
        rec = dict(xs=xs, dys=dys, aug=2, method=method, outs=dxs)
        assert not _failed("supp_aug_reduce_bwd", rec)[0]
        unwritten = [t.clone() for t in dxs]
        unwritten[0][5, 4, 3, 7] = 1.0                                                          # the last element of a level left as it was
        assert "supp_aug_reduce_bwd" in _failed("supp_aug_reduce_bwd", dict(rec, outs=unwritten))[0]
    x = xs[0].float().view(3, 2, 5, 4, 8)
    tie = x[:, 0] == x[:, 1]
    assert int(tie.sum()) > 10
    last = torch.where(tie, torch.zeros(()), dxs[0].float().view(3, 2, 5, 4, 8)[:, 0])          # a tie's gradient to the LAST member
    wrong = torch.stack([last, dys[0].float() - last], 1).reshape(6, 5, 4, 8).to(BF)
    assert "supp_aug_reduce_bwd" in _failed("supp_aug_reduce_bwd", dict(rec, outs=[wrong, dxs[1]]))[0]
    # ---- sweep / gallery: 2 images x 3 classes
    x = torch.randn(2, 3, 2, 8, generator=g).to(BF)
    q = torch.randn(6, 8, generator=g)
    good = lr.correlate_sweep_launch(x, q, 3).to(BF)
    assert not _failed("correlate_sweep", dict(x=x, q=q, classes=3, out=good))[0]
    by_mod = lr.correlate_launch(x[torch.arange(6) % 2], q).to(BF)                              # image = row % B, not row // classes
    assert "correlate_sweep" in _failed("correlate_sweep", dict(x=x, q=q, classes=3, out=by_mod))[0]
    slots = torch.tensor([5, 0, 5, 2, 1, 3], dtype=torch.int32)
    good = lr.correlate_gallery_launch(x, q, slots, 3).to(BF)
    assert not _failed("correlate_gallery", dict(x=x, q=q, slots=slots, classes=3, out=good))[0]
    ungathered = lr.correlate_sweep_launch(x, q, 3).to(BF)                                      # q[row], not q[slots[row]]
    assert "correlate_gallery" in _failed("correlate_gallery", dict(x=x, q=q, slots=slots, classes=3, out=ungathered))[0]


# ---------------------------------------------------------------------------------------------------------------- inventory
# Recorded kinds that only a second-stage call records (ops.box_* / the gallery's box-head GroupNorm).  The replays trace with
# second_stage=False; the box head's launches are held to their references by tests/test_gpu_box_*.py and test_gpu_gallery.py.
NOT_REPLAYED = {
    "box_match_sample_soft": "second stage: the soft-label matcher (ops.box_match_sample), tests/test_gpu_box_soft_labels.py",
    "box_loss_soft": "second stage: the soft-label classification losses (ops.box_loss), tests/test_gpu_box_soft_labels.py",
    "box_loss_neg_support": "second stage: the negative-support loss (ops.box_loss_neg_support), tests/test_gpu_box_neg_support.py",
    "groupnorm_act_rois_gallery": "second stage: the box head's GroupNorm through a slot table, tests/test_gpu_gallery.py",
}


def _recorded_kinds():
    kinds = {}
    pkg = os.path.join(ROOT, "oneshotdet_amd")
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py"):
            for kind in re.findall(r"""_rec\(\s*["'](\w+)["']""", open(os.path.join(pkg, fn)).read()):
                kinds.setdefault(kind, fn)
    return kinds


def test_every_recorded_launch_kind_has_a_restatement_or_a_reason():
    kinds = _recorded_kinds()
    assert len(kinds) >= 25 and "conv" in kinds and "correlate_gallery" in kinds, sorted(kinds)
    missing = [k for k in kinds if not hasattr(rpl.Replayer, "do_" + k) and k not in NOT_REPLAYED]
    assert not missing, "launch kinds recorded (%s) without a restatement in tests/launch_replayer.py: %s" % (
        ", ".join(sorted({kinds[k] for k in missing})), missing)
    stale = [k for k in NOT_REPLAYED if k not in kinds or hasattr(rpl.Replayer, "do_" + k)]
    assert not stale, "NOT_REPLAYED rows whose kind is gone or has a restatement now: %s" % stale
    assert all(len(reason) > 20 for reason in NOT_REPLAYED.values())
    # the float64 replayer inherits every method
    assert all(hasattr(rpl.Fp64Replayer, "do_" + k) for k in kinds if k not in NOT_REPLAYED)


def test_a_record_without_a_restatement_fails_the_replay():
    rp = rpl.Replayer()
    with pytest.raises(LookupError, match="no restatement for launch kind 'box_loss_soft'"):
        rp.run([("box_loss_soft", {})])
    assert not rp.counts
