"""GPU (-m gpu): the query gallery — supports enrolled once (HotPathEngine.enroll -> QueryBank), images detected against the bank
(detect(images, bank=bank, class_ids=...)).  The two kernels that read enrolled data through a device slot table
(osd_correlate_levels_gallery, osd_groupnorm_act_rois_gallery) against the existing entries on gathered operands, bit for bit; the
bank's stages against the class sweep's stages on gathered vectors and query maps, bit for bit; the whole call against the sweep call on
gathered queries at the project's fp32 bar (the query branch runs at other batch sizes); hipGraph replay with a rewritten table;
OneShotDetector with a bank; and the refusals that come before any launch."""
import ctypes

import pytest
import torch

from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
LEVELS = [(5, 7), (3, 2), (1, 1)]
H, W, QS = 96, 160, 64
SIZES = [(96, 160), (80, 150)]                           # true sizes of the two padded targets
KEYS = ("features", "pooled", "combined", "head", "proposals", "detections")


def _same(a, b):
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and torch.equal(a, b)


def _slots(rows):
    return torch.tensor([v for r in rows for v in r], dtype=torch.int32, device="cuda")


# ------------------------------------------------------------------------------------------------------------- kernels
# (G, K, per-image slot rows): one full group of 8 plus a group of one, with repeated and descending slots; one slot; the identity
CASES = [
    (11, 9, [[10, 9, 8, 7, 7, 3, 0, 10, 1], [5, 5, 4, 2, 10, 0, 6, 6, 1]]),
    (3, 1, [[2], [0]]),
    (8, 8, [list(range(8)), list(range(8))]),
]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("c", [16, 256])
def test_gallery_correlation_is_the_sweep_launch_on_gathered_vectors_bit_for_bit(dt, c):
    from oneshotdet_amd import ops
    n = 2
    g = torch.Generator().manual_seed(c)
    xs = [torch.randn(n, h, w, c, generator=g).to(DT[dt]).cuda() for h, w in LEVELS]
    for G, K, rows in CASES:
        qs = [torch.randn(G, c, generator=g).cuda() for _ in LEVELS]
        slots = _slots(rows)
        assert ops.class_sweep_group() == 8 and slots.shape == (n * K,)
        got = ops.correlate_levels_gallery(xs, qs, slots, K)
        idx = slots.long()
        ref = ops.correlate_levels_sweep(xs, [q.index_select(0, idx) for q in qs], K)
        for (h, w), x, q, a, b in zip(LEVELS, xs, qs, got, ref):
            assert a.shape == (n * K, h, w, c) and a.dtype == DT[dt]
            assert torch.equal(a, b), (G, K, h, w)
            if dt == "f32":              # one IEEE product per element
                assert torch.equal(a, x.repeat_interleave(K, 0) * q[idx][:, None, None, :]), (G, K, h, w)
    # n = 0: a no-op with the right shapes
    qs = [torch.randn(3, c, generator=g).cuda() for _ in LEVELS]
    got = ops.correlate_levels_gallery([x[:0] for x in xs], qs, torch.zeros(0, dtype=torch.int32, device="cuda"), 2)
    assert [tuple(y.shape) for y in got] == [(0, h, w, c) for h, w in LEVELS]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("offset", [0, 1])
def test_gallery_groupnorm_is_the_existing_entry_on_a_gathered_addend_bit_for_bit(dt, offset):
    """3 ROI sets of 5 ROIs, 7 x 7 maps, 4 slots x 2 shots, index (3, 0, 3).  Channels: the issue names c = 64, which
    osd_groupnorm_act_rois itself refuses (OSD_ERR_UNSUPPORTED: a workgroup is c / 2 threads and must be whole waves), so there is
    nothing to compare at that width: both entries are held to the same refusal there, and the bit-for-bit comparison runs at c = 128,
    the smallest width the existing entry takes."""
    from oneshotdet_amd import _lib, ops
    sets, per, slots, shots = 3, 5, 4, 2
    index = torch.tensor([3, 0, 3], dtype=torch.int32, device="cuda")
    for c in (64, 128):
        g = torch.Generator().manual_seed(c + offset)
        x = (torch.randn(sets * per, 7, 7, c, generator=g) * 2 + 0.5).to(DT[dt]).cuda()
        add = torch.randn(slots * shots, 7, 7, c, generator=g).to(DT[dt]).cuda()
        gamma, beta = (torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.2).cuda()
        gathered = add.index_select(0, index.long() * shots + offset).contiguous()

        def new():
            return ops.groupnorm_act_rois(x, gamma, beta, 32, 1e-5, 0.2, addend=add, rois_per_add=per, add_stride=shots, add_offset=offset,
                                          add_index=index)

        def old():
            return ops.groupnorm_act_rois(x, gamma, beta, 32, 1e-5, 0.2, addend=gathered, rois_per_add=per, add_stride=1, add_offset=0)
        if c == 64:
            for f in (new, old):
                with pytest.raises(_lib.OsdError) as e:
                    f()
                assert e.value.code == -2
            continue
        got, ref = new(), old()
        assert got.shape == x.shape and got.dtype == DT[dt] and bool(torch.isfinite(got.float()).all())
        assert torch.equal(got, ref)
        assert torch.equal(got[:per], got[2 * per:]) is False            # sets 0 and 2 share slot 3 but not their ROIs
        # the index is read: another table gives another result for set 1 only
        other = ops.groupnorm_act_rois(x, gamma, beta, 32, 1e-5, 0.2, addend=add, rois_per_add=per, add_stride=shots, add_offset=offset,
                                       add_index=torch.tensor([3, 1, 3], dtype=torch.int32, device="cuda"))
        assert torch.equal(other[:per], got[:per]) and torch.equal(other[2 * per:], got[2 * per:])
        assert not torch.equal(other[per:2 * per], got[per:2 * per])


def test_gallery_entries_refuse_bad_arguments():
    from oneshotdet_amd import _lib, ops
    lib = _lib.load()
    c = 64
    x = torch.zeros(2, 3, 3, c, device="cuda")
    q = torch.zeros(5, c, device="cuda")
    y = torch.zeros(6, 3, 3, c, device="cuda")
    sl = torch.zeros(6, dtype=torch.int32, device="cuda")
    hws = (ctypes.c_int32 * 1)(9)
    A = lambda t: ops._ptr_array([t])                      # noqa: E731
    s = ops._stream()
    ok = dict(xs=A(x), qs=A(q), slots=sl.data_ptr(), ys=A(y), n=2, classes=3, g=5, c=c, dtype=0)
    for kw in (dict(xs=None), dict(qs=None), dict(slots=None), dict(ys=None), dict(classes=0), dict(g=0), dict(c=62), dict(c=12, dtype=1),
               dict(dtype=3), dict(n=-1)):
        a = dict(ok, **kw)
        with pytest.raises(_lib.OsdError) as e:
            _lib.call("osd_correlate_levels_gallery", 1, a["xs"], a["qs"], a["slots"], a["ys"], hws, a["n"], a["classes"], a["g"], a["c"],
                      a["dtype"], s)
        assert e.value.code == -1, kw
    assert lib.osd_correlate_levels_gallery(1, ok["xs"], ok["qs"], ok["slots"], ok["ys"], hws, 0, 3, 5, c, 0, s) == 0     # n = 0
    c = 128
    gx = torch.zeros(10, 7, 7, c, device="cuda")
    add = torch.zeros(4, 7, 7, c, device="cuda")
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    gam = torch.ones(c, device="cuda")
    out = torch.empty_like(gx)
    ok = dict(x=gx.data_ptr(), addend=add.data_ptr(), index=idx.data_ptr(), gamma=gam.data_ptr(), beta=gam.data_ptr(), y=out.data_ptr(),
              n=10, per=5, stride=2, offset=1, n_add=4, dtype=0)
    for kw in (dict(x=None), dict(addend=None), dict(index=None), dict(gamma=None), dict(beta=None), dict(y=None), dict(n_add=0),
               dict(per=0), dict(stride=0), dict(offset=-1), dict(dtype=2)):
        a = dict(ok, **kw)
        with pytest.raises(_lib.OsdError) as e:
            _lib.call("osd_groupnorm_act_rois_gallery", a["x"], a["addend"], a["index"], a["gamma"], a["beta"], a["y"], a["n"], 49, c, 32,
                      1e-5, 0.2, a["per"], a["stride"], a["offset"], a["n_add"], a["dtype"], s)
        assert e.value.code == -1, kw
    with pytest.raises(ValueError):
        ops.correlate_levels_gallery([x], [q], sl, 0)
    with pytest.raises(ValueError):
        ops.groupnorm_act_rois(gx, gam, gam, add_index=idx)             # an index without an addend
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- engine
_ENGINE = {}


def _engine(dtype=torch.float32):
    from oneshotdet_amd import model
    if dtype not in _ENGINE:
        _ENGINE[dtype] = model.HotPathEngine(synth.make_state_dict(spec.full_model_shapes()), dtype=dtype)
    return _ENGINE[dtype]


def _targets(B, seed=0):
    """padded targets with their true sizes (zero outside them, as to_image_list pads)"""
    from oneshotdet_amd import layers
    img = torch.from_numpy(synth.make_images("gallery.target", B, H, W, seed=seed))
    sizes = SIZES[:B]
    for i, (h, w) in enumerate(sizes):
        img[i, :, h:, :] = 0
        img[i, :, :, w:] = 0
    return layers.ImageList(img.cuda(), sizes)


def _supports(rows, seed=1):
    return torch.from_numpy(synth.make_images("gallery.query", rows, QS, QS, seed=seed)).cuda()


def _gather(gallery, ids, S):
    """the B*K*S query rows detect(classes=K) takes for the table `ids`: row (b*K + k)*S + s = shot s of slot ids[b][k]"""
    rows = [g * S + s for r in ids for g in r for s in range(S)]
    return gallery.index_select(0, torch.tensor(rows, device=gallery.device)).contiguous(), rows


@pytest.mark.parametrize("B,G,K,S,ids", [(2, 4, 3, 1, [[2, 0, 3], [1, 1, 0]]), (1, 2, 2, 5, [[1, 0]])])
def test_bank_stages_equal_the_sweep_stages_on_gathered_vectors_bit_for_bit(B, G, K, S, ids):
    """ONE enrollment of G slots of S shots; one forward_features over the B targets and the same G*S supports gives the target
    features, the query maps and the pooled vectors (the enrollment's launches on the same rows: the same bits, asserted).  The
    sweep forms of run_correlate / run_head / run_proposals / run_box_head on index_select-gathered pooled vectors and query maps
    against the bank forms through the slot table.  (1, 2, 2, 5): the shots' arg-max."""
    from oneshotdet_amd import box_head, model
    eng = _engine()
    assert eng.box_cls_loss == "ce_loss"
    images, gallery = _targets(B), _supports(G * S)
    bank = eng.enroll(gallery, shots=S)
    assert (bank.slots, bank.shots, bank.labels, bank.token) == (G, S, None, eng.pack_token)
    assert [tuple(p.shape) for p in bank.pooled] == [(G, spec.FPN_OUT)] * 5 and bank.pooled[0].dtype == torch.float32
    assert bank.q_half.shape[:3] == (G * S, 7, 7) and bank.query_roi.shape == (G * S, 7, 7, spec.FPN_OUT)
    feats, qfeats, pooled, _ = eng.forward_features(images.tensors, gallery, classes=G // B)     # G*S = B * (G/B) * S query rows
    assert feats[0].shape[0] == B and qfeats[0].shape[0] == G * S
    assert _same(pooled, bank.pooled)
    table = eng.slot_table(bank, B, ids, True)
    assert table.classes == K and table.ids == ids and table.dev.dtype == torch.int32 and table.dev.tolist() == [v for r in ids for v in r]
    idx = table.dev.long()
    qrows = (idx[:, None] * S + torch.arange(S, device="cuda")[None]).reshape(-1)
    pooled_g = [p.index_select(0, idx) for p in pooled]
    qfeats_g = [q.index_select(0, qrows).contiguous() for q in qfeats]
    rows = [s for s in images.image_sizes for _ in range(K)]
    hw = model.image_sizes_dev(rows, feats[0].device)
    old, new = {}, {}
    for out, kw_c, kw_b in ((old, dict(pooled=pooled_g), dict(qfeats=qfeats_g, q_size=(QS, QS))),
                            (new, dict(pooled=None, bank=bank, slots=table.dev), dict(qfeats=None, q_size=None, bank=bank, slots=table.dev))):
        out["combined"] = model.run_correlate(feats, classes=K, **kw_c)
        out["head"] = model.run_head(eng.head, out["combined"])
        out["proposals"] = model.run_proposals(out["head"], H, W, spec.PRE_NMS_TOP_N_TEST, spec.POST_NMS_TOP_N_TEST, spec.NMS_THRESH,
                                               image_sizes=rows)
        pb, _, pc = out["proposals"]
        out["detections"] = box_head.run_box_head(eng.box_head, feats, boxes=pb, counts=pc, img_h=H, img_w=W, shots=S, img_hw=hw,
                                                  classes=K, **kw_b)
    torch.cuda.synchronize()
    for key in ("combined", "head", "proposals", "detections"):
        assert _same(old[key], new[key]), key
    assert new["combined"][0].shape[0] == B * K and new["detections"]["boxes"].shape[0] == B * K
    assert int(new["proposals"][2].min()) > 0 and int(new["detections"]["counts"].sum()) > 0
    # two different slots of one image are different categories: their combined maps differ
    assert ids[0][0] != ids[0][1] and not torch.equal(new["combined"][0][0], new["combined"][0][1])


def test_bank_detect_matches_the_sweep_detect_on_gathered_queries():
    """detect(bank=, class_ids=) against detect(gathered queries, classes=3), fp32, B = 2 padded targets of 96 x 160, K = 3 of G = 4
    slots of 64 x 64 supports.  The target branch is the same launches on the same rows: `features` are bit-equal.  The query branch ran
    on G = 4 rows at the enrollment and on B*K = 6 rows in the sweep call and may take other tiles, so `combined` is held to rtol 1e-3,
    atol 1e-3 * absmax and the head outputs to 1e-3 + 1e-3.  Measured on an MI355X: every compared tensor came out
    bit-equal (worst |difference| 0.0 for the combined maps and the head outputs)."""
    eng = _engine()
    B, G, K = 2, 4, 3
    ids = [[2, 0, 3], [1, 1, 0]]
    images, gallery = _targets(B, seed=4), _supports(G, seed=5)
    bank = eng.enroll(gallery)
    got = eng.detect(images, bank=bank, class_ids=ids, second_stage=True)
    queries, _ = _gather(gallery, ids, 1)
    ref = eng.detect(images, queries, classes=K, second_stage=True)
    torch.cuda.synchronize()
    assert got["classes"] == K and got["class_ids"] == ids and "query_features" not in got and "query_features" in ref
    assert _same(got["features"], ref["features"])
    worst = {"combined": 0.0, "head": 0.0}
    for lvl in range(5):
        a, b = got["combined"][lvl], ref["combined"][lvl]
        assert a.shape == b.shape and a.shape[0] == B * K
        worst["combined"] = max(worst["combined"], float((a - b).abs().max()))
        print("combined", lvl, float((a - b).abs().max()), float(b.abs().max()))
        torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3 * float(b.abs().max()))
        for a, b in zip(got["head"][lvl], ref["head"][lvl]):
            worst["head"] = max(worst["head"], float((a - b).abs().max()))
            torch.testing.assert_close(a, b, rtol=1e-3, atol=1e-3)
    print("worst differences:", worst)
    assert got["proposals"][0].shape[0] == B * K and got["detections"]["counts"].shape == (B * K,)
    assert int(got["detections"]["counts"].sum()) > 0


def test_class_ids_none_is_every_slot_in_order_bit_for_bit():
    eng = _engine()
    B, G = 2, 4
    images = _targets(B, seed=6)
    bank = eng.enroll(_supports(G, seed=7))
    a = eng.detect(images, bank=bank, second_stage=True)
    b = eng.detect(images, bank=bank, class_ids=[list(range(G))] * B, second_stage=True)
    torch.cuda.synchronize()
    assert a["classes"] == b["classes"] == G and a["class_ids"] == b["class_ids"] == [list(range(G))] * B
    for key in KEYS:
        assert _same(a[key], b[key]), key
    assert a["combined"][0].shape[0] == B * G


def test_graphed_bank_replays_equal_eager_and_take_a_new_table():
    from oneshotdet_amd import model
    eng = _engine(torch.bfloat16)
    B, G, K = 2, 4, 3
    ids, other = [[2, 0, 3], [1, 1, 0]], [[0, 1, 2], [3, 3, 2]]
    img = _targets(B, seed=8).tensors
    bank = eng.enroll(_supports(G, seed=9))
    g = model.GraphedDetect(eng, img, None, bank=bank, class_ids=ids, second_stage=True)
    buffer = g.slots.data_ptr()
    for im, table in ((img, None), (img.flip(-1).contiguous(), other)):
        got = g(im, class_ids=table)
        torch.cuda.synchronize()
        want = ids if table is None else table
        eager = eng.detect(im, bank=bank, class_ids=want, second_stage=True)
        torch.cuda.synchronize()
        assert got["class_ids"] == want and g.slots.tolist() == [v for r in want for v in r] and g.slots.data_ptr() == buffer
        for key in KEYS:
            assert _same(got[key], eager[key]), key
        assert got["combined"][0].shape[0] == B * K and int(got["detections"]["counts"].sum()) > 0
    with pytest.raises(ValueError, match="captured with 3"):
        g(img, class_ids=[[0, 1], [2, 3]])
    with pytest.raises(ValueError, match=r"not in \[0, 4\)"):
        g(img, class_ids=[[0, 1, 4], [2, 3, 0]])
    assert g.slots.tolist() == [v for r in other for v in r]             # a refused table leaves the buffer alone


def test_bank_refusals_come_before_any_launch():
    from oneshotdet_amd import model, trace
    eng, eng16 = _engine(), _engine(torch.bfloat16)
    images = _targets(2)
    supports = _supports(4)
    bank, bank16 = eng.enroll(supports), eng16.enroll(supports)
    one = model.HotPathEngine(synth.make_state_dict(spec.full_model_shapes(box_cls_loss="focal_loss")), dtype=torch.bfloat16,
                              box_cls_loss="focal_loss")
    stale = one.enroll(supports)
    one.repack()
    two_shots = one.enroll(supports, shots=2)
    torch.cuda.synchronize()
    trace.TRACE = []
    try:
        with pytest.raises(ValueError, match=r"exactly one of queries and bank.*both"):
            eng.detect(images, supports, bank=bank, second_stage=True)
        with pytest.raises(ValueError, match=r"exactly one of queries and bank.*neither"):
            eng.detect(images, second_stage=True)
        with pytest.raises(ValueError, match=r"ragged class_ids"):
            eng.detect(images, bank=bank, class_ids=[[0, 1], [2]], second_stage=True)
        with pytest.raises(ValueError, match=r"holds slot -1: not in \[0, 4\)"):
            eng.detect(images, bank=bank, class_ids=[[0, -1], [2, 3]])
        with pytest.raises(ValueError, match=r"holds slot 4: not in \[0, 4\)"):
            eng.forward(images.tensors, bank=bank, class_ids=[[0, 1], [4, 3]])
        with pytest.raises(ValueError, match=r"class_ids has 3 rows for 2 images"):
            eng.forward_features(images.tensors, bank=bank, class_ids=[[0], [1], [2]])
        with pytest.raises(ValueError, match=r"stale QueryBank.*repack\(\)"):
            one.detect(images, bank=stale)
        with pytest.raises(ValueError, match=r"another engine"):
            one.detect(images, bank=bank16)
        with pytest.raises(ValueError, match=r"torch\.bfloat16.*torch\.float32"):
            eng.detect(images, bank=bank16, second_stage=True)
        with pytest.raises(ValueError, match=r"box_head\.py:246-253"):      # a one-logit loss with 2 shots per slot
            one.detect(images, bank=two_shots, second_stage=True)
        with pytest.raises(ValueError, match=r"class_ids picks slots of a QueryBank"):
            eng.detect(images, supports[:2], class_ids=[[0], [1]])
        assert trace.TRACE == []
        out = one.detect(images, bank=two_shots, class_ids=[[1], [0]])      # the first stage alone takes the two shots
        kinds = [k for k, _ in trace.TRACE]
        assert "correlate_gallery" in kinds and len(kinds) > 0
        n_bank = len(kinds)
        trace.TRACE = []
        eng.detect(images, bank=bank, class_ids=[[1], [0]], second_stage=True)
        kinds = [k for k, _ in trace.TRACE]
        assert "correlate_gallery" in kinds and "correlate_sweep" not in kinds
        trace.TRACE = []
        eng.detect(images, supports[:2].contiguous(), second_stage=True)    # the per-pair call launches the query branch on top
        assert len(trace.TRACE) > len(kinds) and n_bank > 0
    finally:
        trace.TRACE = None
    torch.cuda.synchronize()
    assert out["proposals"][2].shape == (2,)


def test_one_shot_detector_takes_a_bank_as_images_supp():
    from oneshotdet_amd import model, modules
    det = modules.OneShotDetector(synth.make_state_dict(spec.full_model_shapes()), dtype=torch.float32)
    B, G, K = 2, 4, 3
    images, gallery = _targets(B, seed=10), _supports(G, seed=11)
    labels = [3, 7, 5, 9]
    bank = det.enroll(gallery, labels)
    assert isinstance(bank, model.QueryBank) and bank.labels == labels and bank.slots == G
    ids = [[7, 3, 9], [5, 9, 3]]
    res = det(images, bank, target_ids=ids)
    assert len(res) == B
    queries, _ = _gather(gallery, [[labels.index(v) for v in row] for row in ids], 1)
    sweep = det(images, queries, target_ids=ids)            # the classes=K module call on the gathered supports
    for b, (bl, ref) in enumerate(zip(res, sweep)):
        h, w = images.image_sizes[b]
        assert bl.size == (w, h) and len(bl) == len(ref) > 0
        s = bl.get_field("scores")
        assert bool((s[:-1] >= s[1:]).all()) and set(bl.get_field("labels").tolist()) <= set(ids[b])
        for label in ids[b]:
            sel, rsel = bl.get_field("labels") == label, ref.get_field("labels") == label
            assert torch.equal(bl.bbox[sel], ref.bbox[rsel]) and torch.equal(s[sel], ref.get_field("scores")[rsel]), (b, label)
    every = det(images, bank)                               # target_ids None: all labels, in the bank's order
    assert len(every) == B and set(every[0].get_field("labels").tolist()) <= set(labels)
    assert len(every[0]) >= len(res[0])
    with pytest.raises(ValueError, match=r"label 8, which is not among the bank's labels \[3, 7, 5, 9\]"):
        det(images, bank, target_ids=[[7, 3, 9], [5, 8, 3]])
