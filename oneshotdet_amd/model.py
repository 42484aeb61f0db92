"""Host side of the siamese-FCOS hot path on MI355X: weight packing and kernel sequencing.

Mirrors, function for function, the reference call stack of SURVEY.md §3.1:
  GeneralizedRCNN.forward (modeling/detector/generalized_rcnn.py:226-312)
    backbone / supp_backbone  = Sequential(ResNet body, FPN)   (modeling/backbone/backbone.py:51-72)
    supp_pooling + batch_pooling + correlation                   (generalized_rcnn.py:297-311)
    rpn = FCOSModule: FCOSHead + FCOSPostProcessor               (modeling/rpn/fcos/fcos.py, inference.py)
All tensors between kernels are NHWC; state_dict names and OIHW shapes are the reference's (oneshotdet_amd/spec.py).
"""
import collections
import os

import torch

from . import streams as _streams

from . import ops, spec
from .ops import ACT_EXP_SCALE, ACT_NONE, ACT_RELU, RES_DOWN2X, RES_SAME, RES_UP2X


LOCKSTEP = os.environ.get("OSD_LOCKSTEP", "0") != "0"            # inference engine: both backbones per launch (A/B)
TOWERS_MERGED = os.environ.get("OSD_TOWERS_MERGED", "0") != "0"  # inference engine: both towers per launch (A/B)
SKIP_UNUSED_C2 = os.environ.get("OSD_FULL_C2", "0") == "0"     # A/B switch: compute all of layer1's last block anyway


def _bn(sd, p):
    return (sd[p + ".weight"], sd[p + ".bias"], sd[p + ".running_mean"], sd[p + ".running_var"])


RES_DOWN2X_OK = os.environ.get("OSD_NO_RES_DOWN2X", "0") == "0"      # A/B switch: copy the identity's even pixels instead (the form until round 6)
FPN_OUT_GROUPED = os.environ.get("OSD_NO_FPN_GROUPED", "0") == "0"       # the FPN's P3 + P4 output convs as one launch
FUSE_DOWNSAMPLE = os.environ.get("OSD_NO_FUSE_DS", "0") == "0"      # A/B switch: conv3 + downsample of a stage's first block as one GEMM
C3DS = "conv3+downsample.0"      # that fused conv of a block (pack_conv3_downsample) in the by-name lookups of walk_backbones


def pack_conv3_downsample(sd, p, dtype):
    """The first block of a stage ends in relu(bn3(conv3(out)) + bn_d(downsample(x))) (resnet.py:295-315).  Both are 1x1
    convs onto the same pixels, so they are ONE GEMM over the concatenated input channels [out | x]: FrozenBN folded into
    the rows of either part (batch_norm.py:19-24, no eps), the shifts added.  The 4 x-wide downsample output is then never
    written and never read back as a residual (osd_conv2d_fwd with a second source)."""
    def fold(conv, bn):
        g, b, mean, var = (t.float() for t in _bn(sd, p + bn))
        scale = g * var.rsqrt()
        return sd[p + conv + ".weight"].float() * scale.view(-1, 1, 1, 1), b - mean * scale
    w3, b3 = fold("conv3", "bn3")
    wd, bd = fold("downsample.0", "downsample.1")
    return ops.pack_conv(torch.cat([w3, wd], 1).contiguous(), bias=(b3 + bd).contiguous(), dtype=dtype)


class BackboneWeights(object):
    """Packed weights of one ResNet-50-FPN (resnet.py:80-145, fpn.py:28-41,82-94)."""

    def __init__(self, sd, prefix, dtype):
        b = prefix + "body."
        self.stem = ops.pack_conv(sd[b + "stem.conv1.weight"], bn=_bn(sd, b + "stem.bn1"), dtype=dtype, stem=True)
        self.blocks = []
        self.convs = {"body.stem.conv1": self.stem}      # every packed conv by its name behind the prefix (walk_backbones)
        for si, nblocks in enumerate(spec.STAGE_BLOCKS):
            for bi in range(nblocks):
                p = "%slayer%d.%d." % (b, si + 1, bi)
                blk = {"ds": None}
                if (p + "downsample.0.weight") in sd:
                    blk["ds"] = ops.pack_conv(sd[p + "downsample.0.weight"], bn=_bn(sd, p + "downsample.1"), dtype=dtype)
                    # bf16 only: the exact-fp32 engines stay on the reference's operation order (the fused sum rounds once
                    # instead of twice — enough to flip a ReLU that sits on zero, which the fp32 gradient tests would see)
                    blk["c3ds"] = pack_conv3_downsample(sd, p, dtype) if (FUSE_DOWNSAMPLE and dtype == torch.bfloat16) else None
                for i in (1, 2, 3):
                    blk["c%d" % i] = ops.pack_conv(sd["%sconv%d.weight" % (p, i)], bn=_bn(sd, "%sbn%d" % (p, i)),
                                                   dtype=dtype)
                self.blocks.append(blk)
                for key, name in (("c1", "conv1"), ("c2", "conv2"), ("c3", "conv3"), ("ds", "downsample.0"), ("c3ds", C3DS)):
                    if blk.get(key) is not None:
                        self.convs[p[len(prefix):] + name] = blk[key]
        f = prefix + "fpn."
        self.fpn = {}
        for name in ("fpn_inner2", "fpn_inner3", "fpn_inner4", "fpn_layer2", "fpn_layer3", "fpn_layer4",
                     "top_blocks.p6", "top_blocks.p7"):
            self.convs["fpn." + name] = self.fpn[name] = ops.pack_conv(sd[f + name + ".weight"], bias=sd[f + name + ".bias"], dtype=dtype)


class HeadWeights(object):
    """Packed FCOSHead (fcos.py:27-81).  cls_logits and centerness both read the cls tower (fcos.py:91-92), so they
    are fused into one 2-output conv (stored as 4 channels: logit, centerness, 0, 0)."""

    def __init__(self, sd, dtype, prefix="rpn.head."):
        self.towers = {}
        for tower in ("cls_tower", "bbox_tower"):
            layers = []
            for i in range(spec.NUM_CONVS):
                conv = ops.pack_conv(sd["%s%s.%d.weight" % (prefix, tower, 3 * i)],
                                     bias=sd["%s%s.%d.bias" % (prefix, tower, 3 * i)], dtype=dtype)
                layers.append((conv, sd["%s%s.%d.weight" % (prefix, tower, 3 * i + 1)].float().contiguous(),
                               sd["%s%s.%d.bias" % (prefix, tower, 3 * i + 1)].float().contiguous()))
            self.towers[tower] = layers
        w = torch.cat([sd[prefix + "cls_logits.weight"], sd[prefix + "centerness.weight"]], 0)
        b = torch.cat([sd[prefix + "cls_logits.bias"], sd[prefix + "centerness.bias"]], 0)
        self.pred_cls_ctr = ops.pack_conv(w, bias=b, dtype=dtype)
        self.pred_box = ops.pack_conv(sd[prefix + "bbox_pred.weight"], bias=sd[prefix + "bbox_pred.bias"], dtype=dtype)
        # Scale modules (layers/scale.py): the scalar is folded into the exp epilogue; one host read at pack time
        self.scales = [float(sd["%sscales.%d.scale" % (prefix, i)].item()) for i in range(5)]
        self.scales_dev = torch.cat([sd["%sscales.%d.scale" % (prefix, i)].reshape(1) for i in range(5)]).float().contiguous()


# How a caller wants the R-50-FPN graph walked ("One graph walk, three callers"): data, one instance per caller.
#   fuse_stages       stages whose first block runs conv3 + downsample as one two-source GEMM, where that conv is packed (bf16)
#   down2x_even_only  RES_DOWN2X for layer1's quarter-size last block only where every identity map has even H and W (else a strided copy)
#   p7_relu_in        P7's input ReLU as the conv's prologue, one launch per branch (False: relu(P6) materialised, kept as maps["p6r"])
#   skip_unused_c2, fpn_out_grouped    the OSD_FULL_C2 / OSD_NO_FPN_GROUPED switches as the caller reads them
BackbonePolicy = collections.namedtuple("BackbonePolicy", "fuse_stages down2x_even_only p7_relu_in skip_unused_c2 fpn_out_grouped")


def walk_backbones(conv, inputs, dtype, policy, save=None, after_frozen=None):
    """THE R-50-FPN forward graph (resnet.py:138-145,295-315,332-337; fpn.py:43-75,95-99): stem, max-pool, 16 bottlenecks, top-down
    FPN, P6, P7, for len(inputs) branches in lockstep: every layer is one ops.conv2d_multi launch over the branches (one branch: the
    plain ops.conv2d launch, ops.conv2d_multi forwards it).  conv(j, name) -> the PackedConv of branch j's conv ("body.layer2.0.conv1",
    "fpn.fpn_inner3", a block's C3DS: None where not packed).  save(si, bi, block) gets every bottleneck's per-branch lists (p, s, ds,
    x, o1, o2, y); after_frozen() is called once the stems and layer1 (frozen: resnet.py:127-136) have been enqueued.
    -> ([P3..P7] NHWC per branch, {c3, c4, c5, inner4, inner3, inner2, p5, p6, p6r: per-branch lists})."""
    nb = range(len(inputs))

    def pcs(name):
        return [conv(j, name) for j in nb]
    xs = []
    for j in nb:
        x, hw = ops.stem_input(inputs[j], dtype)
        x = ops.conv2d(x, conv(j, "body.stem.conv1"), act=ACT_RELU, out_hw=hw)
        xs.append(ops.maxpool3x3s2(x))
    stage_out, halved = [], False
    for si, nblocks in enumerate(spec.STAGE_BLOCKS):
        for bi in range(nblocks):
            p = "body.layer%d.%d." % (si + 1, bi)
            s = 2 if (bi == 0 and si > 0) else 1
            if s == 2 and halved:        # the stride already happened in the producer (below)
                s, halved = 1, False
            has_ds = bi == 0             # in_channels != out_channels -> downsample branch (resnet.py:243-251)
            fused = pcs(p + C3DS) if has_ds and si in policy.fuse_stages else [None]
            if fused[0] is not None:     # the 4x-wide downsample map is never written nor re-read as a residual
                o1 = ops.conv2d_multi(xs, pcs(p + "conv1"), stride=s, act=ACT_RELU)
                o2 = ops.conv2d_multi(o1, pcs(p + "conv2"), pad=1, act=ACT_RELU)
                y = [ops.conv2d(o2[j], fused[j], act=ACT_RELU, x2=xs[j], x2_stride=s) for j in nb]
            else:
                identity = ops.conv2d_multi(xs, pcs(p + "downsample.0"), stride=s) if has_ds else xs
                o1 = ops.conv2d_multi(xs, pcs(p + "conv1"), stride=s, act=ACT_RELU)
                rmode = RES_SAME
                # C2 (layer1's output) is read by nothing but layer2.0's two stride-2 1x1 convs (the FPN skips it, fpn.py:33,
                # backbone.py:59): only its even pixels are ever used, so layer1's last block computes just those (its 3x3 at
                # stride 2, its 1x1 + residual on the quarter-size map) and layer2.0 reads them at stride 1
                if policy.skip_unused_c2 and si == 0 and bi == nblocks - 1:
                    o2 = ops.conv2d_multi(o1, pcs(p + "conv2"), stride=2, pad=1, act=ACT_RELU)
                    if RES_DOWN2X_OK and not (policy.down2x_even_only and any(t.shape[1] % 2 or t.shape[2] % 2 for t in identity)):
                        rmode = RES_DOWN2X       # conv3's epilogue reads the identity at (2 ho, 2 wo): no strided copy of a 210 MB map
                    else:
                        identity = [t[:, ::2, ::2].contiguous() for t in identity]
                    halved = True
                else:
                    o2 = ops.conv2d_multi(o1, pcs(p + "conv2"), pad=1, act=ACT_RELU)
                y = ops.conv2d_multi(o2, pcs(p + "conv3"), act=ACT_RELU, residuals=identity, res_mode=rmode)
            if save is not None:
                save(si, bi, dict(p=p, s=s, ds=has_ds, x=xs, o1=o1, o2=o2, y=y))
            xs = y
        stage_out.append(xs)
        if si == 0 and after_frozen is not None:
            after_frozen()
    m = dict(c3=stage_out[1], c4=stage_out[2], c5=stage_out[3])
    m["inner4"] = ops.conv2d_multi(m["c5"], pcs("fpn.fpn_inner4"))
    p5 = m["p5"] = ops.conv2d_multi(m["inner4"], pcs("fpn.fpn_layer4"), pad=1)
    inner3 = m["inner3"] = ops.conv2d_multi(m["c4"], pcs("fpn.fpn_inner3"), residuals=m["inner4"], res_mode=RES_UP2X)
    inner2 = m["inner2"] = ops.conv2d_multi(m["c3"], pcs("fpn.fpn_inner2"), residuals=inner3, res_mode=RES_UP2X)
    if policy.fpn_out_grouped:
        # the P3 and P4 output convs (fpn.py:66-75: same 3x3 256 -> 256 geometry, their own weights) as ONE launch: alone, P3's
        # 400 pixel tiles are 1.56 rounds of the 256 CUs and P4's 100 fill 40 % of one; together 500 tiles are 1.95 rounds
        # (the grouped-launch tuner may still cut it where that measures faster)
        p34 = ops.conv2d_multi(inner2 + inner3, pcs("fpn.fpn_layer2") + pcs("fpn.fpn_layer3"), pad=1)
        p3, p4 = p34[:len(nb)], p34[len(nb):]
    else:
        p4 = ops.conv2d_multi(inner3, pcs("fpn.fpn_layer3"), pad=1)
        p3 = ops.conv2d_multi(inner2, pcs("fpn.fpn_layer2"), pad=1)
    p6 = m["p6"] = ops.conv2d_multi(p5, pcs("fpn.top_blocks.p6"), stride=2, pad=1)
    if policy.p7_relu_in:            # relu prologue (conv2d only): tiny launches
        m["p6r"] = None
        p7 = [ops.conv2d(p6[j], conv(j, "fpn.top_blocks.p7"), stride=2, pad=1, relu_in=True) for j in nb]
    else:                            # relu(P6), materialised: the P7 weight gradient reads it
        m["p6r"] = [ops.add_mask(t, None, t) for t in p6]
        p7 = ops.conv2d_multi(m["p6r"], pcs("fpn.top_blocks.p7"), stride=2, pad=1)
    return [[p3[j], p4[j], p5[j], p6[j], p7[j]] for j in nb], m


def run_backbone(wts, images, dtype):
    """images NCHW fp32 -> [P3, P4, P5, P6, P7] NHWC: walk_backbones with one branch."""
    policy = BackbonePolicy(fuse_stages=(0, 1, 2, 3), down2x_even_only=False, p7_relu_in=True, skip_unused_c2=SKIP_UNUSED_C2,
                            fpn_out_grouped=FPN_OUT_GROUPED)
    return walk_backbones(lambda j, name: wts.convs.get(name), (images,), dtype, policy)[0][0]


def run_backbones(wt, wq, images, queries, dtype):
    """Target and query backbone (BackboneWeights wt / wq: generalized_rcnn.py:270-272, separately parameterised, same
    graph) in LOCKSTEP: every layer is one osd_conv2d_fwd_multi launch over (target, query), so the query branch's
    latency-sized launches ride in the tail of the target's.  -> ([P3..P7] target, [P3..P7] query), NHWC."""
    policy = BackbonePolicy(fuse_stages=(), down2x_even_only=True, p7_relu_in=True, skip_unused_c2=SKIP_UNUSED_C2,
                            fpn_out_grouped=FPN_OUT_GROUPED)
    return walk_backbones(lambda j, name: (wt, wq)[j].convs.get(name), (images, queries), dtype, policy)[0]


_ROI_CACHE = {}


def whole_image_rois(q_sizes, device):
    """[i, 0, 0, h, w] per query — the reference's quirk: the box is built from image_sizes = (h, w) but consumed as
    (x1, y1, x2, y2) (generalized_rcnn.py:257).  Cached per device so no host->device copy happens in steady state
    (and none inside a hipGraph capture)."""
    key = (tuple(q_sizes), str(device))
    if key not in _ROI_CACHE:
        _ROI_CACHE[key] = torch.tensor([[float(i), 0.0, 0.0, float(h), float(w)] for i, (h, w) in enumerate(q_sizes)],
                                       dtype=torch.float32, device=device)
    return _ROI_CACHE[key]


_SIZE_CACHE = {}


def image_sizes_dev(image_sizes, device):
    """[N,2] fp32 (height, width) per image on the device, cached like the ROI table (no copy in steady state)."""
    key = (tuple(tuple(int(v) for v in s) for s in image_sizes), str(device))
    if key not in _SIZE_CACHE:
        _SIZE_CACHE[key] = torch.tensor([[float(h), float(w)] for h, w in key[0]], dtype=torch.float32, device=device)
    return _SIZE_CACHE[key]


def run_query_pool(qfeats, q_sizes, batch, supp_roialign=True):
    """SuppAlignLayer (generalized_rcnn.py:20-52) + batch_pooling (:100-104) -> 5 x [B, C] fp32.  supp_roialign=False
    (FEW_SHOT.SUPP_ROIALIGN False): nn.AdaptiveAvgPool2d((1, 1)) instead (:87-94, 302-303), the mean of each whole map, padding
    included, so q_sizes plays no part."""
    if not supp_roialign:
        return ops.query_avgpool_levels(qfeats, batch)
    rois = whole_image_rois(q_sizes, qfeats[0].device)
    if ops.QUERY_POOL_LEVELS and len(qfeats) <= 8:
        return ops.query_pool_levels(qfeats, rois, spec.POOLER_SCALES, batch, spec.POOLER_SAMPLING_RATIO)
    pooled = []
    for feat, scale in zip(qfeats, spec.POOLER_SCALES):
        v = ops.roi_align(feat, rois, scale, 1, 1, spec.POOLER_SAMPLING_RATIO)
        pooled.append(ops.shot_mean(v.view(v.shape[0], -1), batch))
    return pooled


def run_supp_aug(qfeats, aug, method):
    """FEW_SHOT.SUPP_AUG (generalized_rcnn.py:280-288): every group of `aug` consecutive maps of the query pyramid merged into one
    ('avg' / 'max'), all levels in one launch, directly behind the query backbone: the query pooling, the second stage's query ROI
    pooling and enroll see one map per group.  aug = 1: the maps as they are, nothing launched."""
    return qfeats if aug == 1 else ops.supp_aug_reduce_levels(qfeats, aug, method)


def run_correlate(feats, pooled, classes=1, bank=None, slots=None):
    """generalized_rcnn.py:307-311: all five levels in one launch.  classes = K (the class sweep): pooled has K rows per image of
    feats and the result K maps per image, row b*K + k (ops.correlate_levels_sweep: each map loaded once per group of vectors).
    bank + slots (the query gallery): the K vectors of an image are rows of bank.pooled picked by the device slot table
    (ops.correlate_levels_gallery); `pooled` is not read and no query launch is made."""
    if bank is not None:
        return ops.correlate_levels_gallery(feats, bank.pooled, slots, classes)
    if classes == 1:
        return ops.correlate_levels(feats, pooled)
    return ops.correlate_levels_sweep(feats, pooled, classes)


class QueryBank(object):
    """What HotPathEngine.enroll keeps of G gallery slots of S shots each, so that no later call runs the query branch:
      pooled     5 x [G, C] fp32           the pooled query vectors the correlation multiplies by (run_query_pool)
      q_half     [G*S, 7, 7, 512 | 128]    W_q q + b of the box head's first conv (None without a packed second stage)
      query_roi  [G*S, 7, 7, C]            the pooled query maps behind q_half (box_detect's want_raw)
      shots, slots = G, labels (one per slot, or None), dtype, and the engine + the token of its packed weights the data was computed
    with.  Lives in device memory of this process only: it is refused after engine.repack() and by any other engine."""

    def __init__(self, engine, token, pooled, q_half, query_roi, shots, slots, labels, dtype):
        self.engine, self.token = engine, token
        self.pooled, self.q_half, self.query_roi = pooled, q_half, query_roi
        self.shots, self.slots, self.labels, self.dtype = shots, slots, labels, dtype

    def slots_of(self, target_ids, batch):
        """Labels -> slot numbers (a label's slot is its position in `labels`).  target_ids: None (every slot in order), or one
        sequence of labels per image.  -> class_ids for detect (None, or `batch` lists of slot numbers)."""
        if target_ids is None:
            return None
        if self.labels is None:
            raise ValueError("this QueryBank was enrolled without labels: target_ids cannot name its slots")
        if len(target_ids) != batch or not all(isinstance(t, (list, tuple)) for t in target_ids):
            raise ValueError("target_ids with a QueryBank: one sequence of labels per image, for %d images (got %d entries)"
                             % (batch, len(target_ids)))
        where = {label: i for i, label in enumerate(self.labels)}
        for b, row in enumerate(target_ids):
            for label in row:
                if label not in where:
                    raise ValueError("target_ids[%d] names label %r, which is not among the bank's labels %s" % (b, label, list(self.labels)))
        return [[where[label] for label in row] for row in target_ids]


def check_class_ids(engine, bank, batch, class_ids, second_stage=False):
    """Everything detect(bank=, class_ids=) can refuse, on the host and before anything is launched: the bank (a QueryBank of this
    engine's dtype, of this engine, of its current packed weights; one shot per slot in the one-logit loss modes when the second stage
    runs) and the table (None = every slot in order, or one sequence of K slot numbers in [0, G) per image, the same K for every image;
    repeats allowed).  -> (K, the table as a flat tuple, row b*K + k)."""
    if not isinstance(bank, QueryBank):
        raise ValueError("bank must be a QueryBank made by HotPathEngine.enroll, got %s" % type(bank).__name__)
    if bank.dtype != engine.dtype:
        raise ValueError("the QueryBank holds %s data and this engine computes in %s: enroll the supports with this engine"
                         % (bank.dtype, engine.dtype))
    if bank.engine is not engine:
        raise ValueError("the QueryBank was enrolled by another engine: its vectors come from other weights (enroll the supports with "
                         "this engine)")
    if bank.token != engine.pack_token:
        raise ValueError("stale QueryBank: it was enrolled before repack() (weights token %d, the engine's is %d); enroll the supports "
                         "again" % (bank.token, engine.pack_token))
    if second_stage:
        from .box_head import check_shots
        check_shots(engine.box_cls_loss, bank.shots)
    g = bank.slots
    if class_ids is None:
        return g, tuple(range(g)) * batch
    rows = []
    for r in class_ids:
        r = r.tolist() if hasattr(r, "tolist") else r
        if not isinstance(r, (list, tuple, range)):
            raise ValueError("class_ids must be one sequence of slot numbers per image (nested), got a flat sequence")
        rows.append(list(r))
    if len(rows) != batch:
        raise ValueError("class_ids has %d rows for %d images (one sequence of slot numbers per image)" % (len(rows), batch))
    k = len(rows[0]) if rows else 0
    if any(len(r) != k for r in rows):
        raise ValueError("ragged class_ids: rows of %s slot numbers (the same K for every image)" % sorted(set(len(r) for r in rows)))
    if k < 1:
        raise ValueError("class_ids rows are empty: at least one slot per image")
    for b, r in enumerate(rows):
        for v in r:
            if int(v) != v or not 0 <= int(v) < g:
                raise ValueError("class_ids[%d] holds slot %r: not in [0, %d), the bank's %d slots" % (b, v, g, g))
    return k, tuple(int(v) for r in rows for v in r)


_SLOT_CACHE = {}


def slot_table_dev(flat, device):
    """The slot table on the device (int32 [B*K]), cached by content like the ROI table: no host->device copy in steady state and
    none inside a hipGraph capture."""
    key = (flat, str(device))
    if key not in _SLOT_CACHE:
        _SLOT_CACHE[key] = torch.tensor(flat, dtype=torch.int32, device=device)
    return _SLOT_CACHE[key]


class SlotTable(object):
    """A validated slot table: K, the host rows and the device int32 [B*K] the kernels read.  What check_class_ids + slot_table_dev
    give; GraphedDetect passes one whose device tensor is its own static buffer as `class_ids`."""

    def __init__(self, classes, ids, dev):
        self.classes, self.ids, self.dev = classes, ids, dev


def check_classes(batch, query_rows, classes):
    """The class sweep's row rule, checked before anything is launched: queries holds batch * classes * S rows, row
    (b*classes + k)*S + s = shot s of category slot k of image b.  -> S."""
    classes = int(classes)
    if classes < 1:
        raise ValueError("classes must be at least 1, got %d" % classes)
    if batch * classes == 0 or query_rows == 0 or query_rows % (batch * classes) != 0:
        raise ValueError("%d query rows are no multiple of images x classes = %d x %d = %d (queries holds B*K*S rows: S shots of each "
                         "of K category slots per image)" % (query_rows, batch, classes, batch * classes))
    return query_rows // (batch * classes)


def run_head_tower(hw, feats, tower):
    """One tower + its prediction conv over all levels (fcos.py:89-97): per layer ONE grouped conv launch over the
    levels (they share the weights), then GroupNorm+ReLU of all levels in two launches."""
    t = list(feats)
    for conv, gamma, beta in hw.towers[tower]:
        u = ops.conv2d_grouped(t, conv, pad=1)
        t, _ = ops.groupnorm_relu_levels(u, gamma, beta, spec.GN_GROUPS, spec.GN_EPS)
    if tower == "cls_tower":
        return ops.conv2d_grouped(t, hw.pred_cls_ctr, pad=1)
    return ops.conv2d_grouped(t, hw.pred_box, pad=1, act=ACT_EXP_SCALE,
                              act_scale_devs=[hw.scales_dev[l:l + 1] for l in range(len(t))])


def run_head(hw, feats, streams=None):
    """FCOSHead.forward (fcos.py:83-99).  Per level returns (cls_ctr [N,H,W,4] = (logit, centerness, 0, 0),
    reg [N,H,W,4] = exp(scale_l * bbox_pred)).  The two towers are independent: with `streams` the bbox tower runs on a
    side stream beside the cls tower, so the HBM-bound GroupNorm passes of one tower overlap the MFMA-bound convs of the
    other and the small levels' launch-latency-bound kernels fill the CUs the P3 GEMMs leave idle.  OSD_TOWERS_MERGED=1
    runs each layer of both towers as ONE launch instead (fewer launches, less total kernel time, but measured SLOWER end
    to end: 5.5 vs 4.7 ms per forward step — DESIGN 6b)."""
    if TOWERS_MERGED:
        return run_head_merged(hw, feats)
    if not streams:
        return list(zip(run_head_tower(hw, feats, "cls_tower"), run_head_tower(hw, feats, "bbox_tower")))
    main = _streams.current()
    streams[0].wait_stream(main)
    with _streams.on(streams[0]):
        box_out = run_head_tower(hw, feats, "bbox_tower")
    cls_out = run_head_tower(hw, feats, "cls_tower")
    main.wait_stream(streams[0])
    return list(zip(cls_out, box_out))


def run_head_merged(hw, feats):
    """Both towers per launch: each layer is ONE launch over both towers and all levels (10 pairs, level-major so the
    tuner's large / small split keeps P3 and P4 together), then the GroupNorm+ReLU of a tower's levels in two launches."""
    nl = len(feats)
    towers = ("cls_tower", "bbox_tower")
    t = {tw: list(feats) for tw in towers}
    for i in range(spec.NUM_CONVS):
        xs = [t[tw][l] for l in range(nl) for tw in towers]
        pcs = [hw.towers[tw][i][0] for l in range(nl) for tw in towers]
        us = ops.conv2d_multi(xs, pcs, pad=1)
        for k, tw in enumerate(towers):
            _, gamma, beta = hw.towers[tw][i]
            t[tw], _ = ops.groupnorm_relu_levels(us[k::2], gamma, beta, spec.GN_GROUPS, spec.GN_EPS)
    cls_out = ops.conv2d_grouped(t["cls_tower"], hw.pred_cls_ctr, pad=1)
    box_out = ops.conv2d_grouped(t["bbox_tower"], hw.pred_box, pad=1, act=ACT_EXP_SCALE,
                                 act_scale_devs=[hw.scales_dev[l:l + 1] for l in range(nl)])
    return list(zip(cls_out, box_out))


class ProposalDepth(object):
    """Lagged feedback for the proposal pipeline (osd_proposals_sort_nms_hint): how deep into the score order the greedy
    NMS had to read in recent calls decides how many candidates the next call sorts exactly in its first phase.  The
    depth travels device -> pinned host memory by a non-blocking copy behind the call; the host looks at it only once
    that copy's event has completed (no synchronisation: a step or two of lag), so the pipeline itself never waits."""

    def __init__(self):
        self.hint, self._pending = 0, None

    def before(self, n, device):
        if self._pending is not None and self._pending[1].query():
            host = self._pending[0]
            d = int(host.max())
            # a quarter of headroom over the deepest image, never below the default (0 = let the library decide)
            self.hint = d + d // 4 + 320
            self._pending = None
        return torch.empty((n,), device=device, dtype=torch.int32)

    def after(self, depth_dev):
        if self._pending is None:
            host = torch.empty(depth_dev.shape, dtype=torch.int32, pin_memory=True)
            host.copy_(depth_dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._pending = (host, ev, depth_dev)


def run_proposals(head_out, img_h, img_w, pre_nms_top_n, post_nms_top_n, nms_thresh, cuda_nms=True, workspace=None,
                  image_sizes=None, depth=None):
    """FCOSPostProcessor.forward (fcos/inference.py:251-323).  Boxes are clipped to (img_h, img_w) (the 4-D tensor path of
    to_image_list, structures/image_list.py:44-50) or, for a padded batch, to every image's own image_sizes[i] = (h, w)
    (:52-70).  Everything stays on the device; returns boxes [N, post, 4], scores [N, post] (descending), counts [N]."""
    n = head_out[0][0].shape[0]
    dev = head_out[0][0].device
    sizes = [(c.shape[1], c.shape[2]) for c, _ in head_out]
    total = sum(h * w for h, w in sizes)
    scores = torch.empty((n, total), device=dev, dtype=torch.float32)
    boxes = torch.empty((n, total, 4), device=dev, dtype=torch.float32)
    off = 0
    offs = []
    hw_dev = None if image_sizes is None else image_sizes_dev(image_sizes, dev)
    for (cls_ctr, reg), stride in zip(head_out, spec.FPN_STRIDES):
        ops.fcos_score_decode(cls_ctr, reg, scores, boxes, stride, off, img_h, img_w, hw_dev)
        offs.append(off)
        off += cls_ctr.shape[1] * cls_ctr.shape[2]
    levels = [(lo, h * w) for (h, w), lo in zip(sizes, offs)]
    max_count = sum(min(c, pre_nms_top_n) for _, c in levels)
    if os.environ.get("OSD_PROPOSALS_FULL_SORT"):      # A/B: rank all candidates (two separate calls)
        bs, ss, idx, cnt = ops.rank_sort_gather(scores, boxes, max_count, levels, pre_nms_top_n)
        ob, os_, op, oc = ops.nms_sorted(bs, ss, cnt, nms_thresh, post_nms_top_n, cuda_semantics=cuda_nms,
                                         workspace=workspace)
        return ob, os_, oc
    if depth is None:
        return ops.proposals_sort_nms(scores, boxes, max_count, levels, pre_nms_top_n, nms_thresh, post_nms_top_n,
                                      cuda_semantics=cuda_nms)
    d = depth.before(n, dev)
    out = ops.proposals_sort_nms(scores, boxes, max_count, levels, pre_nms_top_n, nms_thresh, post_nms_top_n,
                                 cuda_semantics=cuda_nms, head_hint=depth.hint, depth_out=d)
    depth.after(d)
    return out


class HotPathEngine(object):
    """Packed weights + forward of the hot path.  state_dict: reference-named fp32 tensors (any device; moved to
    `device`).  dtype: torch.float32 (exact-fp32 MFMA) or torch.bfloat16 (bf16 MFMA, fp32 accumulate).
    siamese_backbone (FEW_SHOT.SIAMESE_BACKBONE): True = the query has a backbone of its own (`supp_backbone.*`); False =
    the query goes through the target's backbone (generalized_rcnn.py:274-275): ONE packed BackboneWeights serves both
    branches (`supp_backbone` is the same object), and `supp_backbone.*` entries of the state_dict are dropped.
    supp_roialign (FEW_SHOT.SUPP_ROIALIGN): True = the query pyramid is pooled by a 1 x 1 ROIAlign of each query's box; False =
    by its global average (run_query_pool).  The pooling has no weights: a state_dict does not tell the two apart.
    box_cls_loss (FEW_SHOT.SECOND_STAGE_CLS_LOSS): "ce_loss" = two class logits and a softmax score; "focal_loss" / "mse_loss" = ONE
    logit and a sigmoid score (roi_box_predictors.py:47-50, inference.py:61-69).  A state_dict whose cls_score has the other mode's
    row count is refused (ValueError naming the option).
    soft_labeling / soft_labeling_func (FEW_SHOT.SOFT_LABELING / SOFT_LABELING_FUNC): how the model was trained; admits "l1_loss"
    (one logit, scored like "mse_loss") and "cxe_loss" (two logits, scored like "ce_loss", inference.py:61-69).  Detection itself
    reads no soft label.
    linear_fusion (FEW_SHOT.LINEAR_FUSION, box_head.py:43,61-72): the second stage's head in front of fc6 is one 3x3 conv over
    cat(x, query), GroupNorm, LeakyReLU; the state_dict has no compress_dim_conv.* and a 512-channel feature_aggreg.0.  A state_dict
    trained with the other setting is refused (ValueError naming the option).
    neg_support (FEW_SHOT.NEG_SUPPORT.TURN_ON): how the model was trained; validated against the combinations the option exists in
    ('ce_loss', no linear_fusion) and changes nothing computed: the reference computes the negative logits in evaluation and discards
    them (box_head.py:156-161,175-177), and the state_dict has the plain 'ce_loss' model's keys and shapes.
    supp_aug / supp_aug_method (FEW_SHOT.SUPP_AUG with NUM_SUPP_AUG = supp_aug - 1, SUPP_AUG_METHOD 'avg' / 'max'): every query is a group
    of supp_aug consecutive rows (a support crop and its augmentations); the query backbone runs on all of them and run_supp_aug merges
    each group into one map per level before anything else reads the query pyramid.  `queries` then holds B*K*S*supp_aug rows (enroll:
    G*shots*supp_aug) and a group's members must have one size.  Ordinary keywords like `shots`: the merge has no weights, and 1 (the
    default) launches nothing."""

    def __init__(self, state_dict, dtype=torch.float32, device="cuda", siamese_backbone=True, supp_roialign=True,
                 box_cls_loss="ce_loss", soft_labeling=False, soft_labeling_func="linear", linear_fusion=False, neg_support=False,
                 supp_aug=1, supp_aug_method="avg"):
        self.supp_aug, self.supp_aug_method = spec.supp_aug_mode(supp_aug, supp_aug_method, neg_support)
        # spec.MODEL_OPTIONS: ValueError by name before anything is built; the rows this engine takes become attributes
        given = spec.options_in(locals())
        options = spec.check_options("the HotPathEngine", True, **given)
        vars(self).update((name, getattr(options, name)) for name in given)
        if not torch.cuda.is_available():
            raise ops._lib.OsdError("HotPathEngine needs an MI355X: no GPU visible and there is no CPU fallback")
        ops._lib.load()
        self.device = torch.device(device)
        self.dtype = dtype
        self.sd = {k: torch.as_tensor(v).to(self.device, torch.float32) for k, v in state_dict.items()
                   if self.siamese_backbone or not spec.is_query_backbone_key(k)}
        missing = [k for k in spec.hot_path_shapes(self.siamese_backbone) if k not in self.sd]
        if missing:
            raise KeyError("state_dict is missing hot-path keys, e.g. %s" % missing[:3])
        self.repack()

    def repack(self):
        self.pack_token = getattr(self, "pack_token", 0) + 1      # a QueryBank enrolled with the weights packed before is stale
        self.backbone = BackboneWeights(self.sd, "backbone.", self.dtype)
        # shared mode: the query branch runs on the target's packed weights (nothing packed, copied or tuned twice)
        self.supp_backbone = BackboneWeights(self.sd, "supp_backbone.", self.dtype) if self.siamese_backbone else self.backbone
        self.head = HeadWeights(self.sd, self.dtype)
        # second stage: packed when the state_dict carries the reference's roi_heads.box.* entries
        self.box_head = None
        if "roi_heads.box.feature_aggreg.0.weight" in self.sd:
            spec.check_linear_fusion(self.sd, self.linear_fusion)      # the other setting's file: refused by name, not passed over
        if all(k in self.sd for k in spec.box_head_shapes(linear_fusion=self.linear_fusion)):
            from .box_head import BoxHeadWeights
            self.box_head = BoxHeadWeights(self.sd, self.dtype, box_cls_loss=self.box_cls_loss, soft_labeling=self.soft_labeling,
                                           linear_fusion=self.linear_fusion, neg_support=self.neg_support)

    def tune(self, images, queries=None, second_stage=False, classes=1, bank=None, class_ids=None):
        """Pick, by measurement on this device, the conv algorithm (kernel generation, ring depth, tile) for every
        distinct conv shape of this input geometry (cached in ops.ALGO_CACHE; a few ms per shape, done once).  classes: as detect's
        (a sweep's head and box head run at B*K rows: other shapes than the per-pair call's); bank / class_ids: as detect's."""
        with ops.tuning():
            self.detect(images, queries, concurrent=False, second_stage=second_stage, classes=classes, bank=bank, class_ids=class_ids)
        torch.cuda.synchronize()

    def enroll(self, queries, shots=1, labels=None):
        """The query branch, once: queries [G*S,3,h,w] (or an ImageList / ops.PackedImages of G*S supports), row g*S + s = shot s of
        gallery slot g -> QueryBank.  With supp_aug = A > 1: G*S*A rows, row (g*S + s)*A + a = member a of that shot's group.  Runs what
        detect runs per call on its queries (the query backbone + FPN, the query pooling, and
        with a packed second stage supproi_pooling and the query half of the box head's first conv), keeps the results, and
        detect(images, bank=bank, class_ids=...) then launches none of them.  labels: one (hashable) label per slot, for
        OneShotDetector's target_ids."""
        from .layers import ImageList
        query_sizes = None
        if isinstance(queries, ops.PackedImages):
            query_sizes = queries.image_sizes
        if isinstance(queries, ImageList):
            queries, query_sizes = queries.tensors, queries.image_sizes
        shots = int(shots)
        aug = self.supp_aug
        q_sizes = spec.group_query_sizes([tuple(queries.shape[-2:])] * queries.shape[0] if query_sizes is None else query_sizes, aug)
        rows = queries.shape[0] // aug
        if shots < 1 or rows == 0 or rows % shots != 0:
            raise ValueError("%d support rows are no multiple of shots = %d (queries holds G*S rows: S shots of each of G gallery slots)"
                             % (rows, shots))
        g = rows // shots
        if labels is not None:
            labels = list(labels)
            if len(labels) != g or len(set(labels)) != g:
                raise ValueError("labels: one distinct label per gallery slot, %d slots (got %d labels, %d distinct)"
                                 % (g, len(labels), len(set(labels))))
        qfeats = run_supp_aug(run_backbone(self.supp_backbone, queries, self.dtype), aug, self.supp_aug_method)
        pooled = run_query_pool(qfeats, q_sizes, g, self.supp_roialign)
        q_half = query_roi = None
        if self.box_head is not None:
            from .box_head import run_query_half
            query_roi, q_half = run_query_half(self.box_head, qfeats, q_sizes if query_sizes is not None else q_sizes[0], self.dtype)
        return QueryBank(self, self.pack_token, pooled, q_half, query_roi, shots, g, labels, self.dtype)

    def slot_table(self, bank, batch, class_ids, second_stage=False):
        """check_class_ids + the cached device table -> SlotTable (a SlotTable passes through: its rows were validated when it was
        made, the bank is checked again)."""
        if isinstance(class_ids, SlotTable):
            check_class_ids(self, bank, batch, None, second_stage)
            if class_ids.dev.shape != (batch * class_ids.classes,):
                raise ValueError("the slot table holds %d entries for %d images x %d slots" % (class_ids.dev.numel(), batch, class_ids.classes))
            return class_ids
        k, flat = check_class_ids(self, bank, batch, class_ids, second_stage)
        return SlotTable(k, [list(flat[b * k:(b + 1) * k]) for b in range(batch)], slot_table_dev(flat, self.device))

    def side_streams(self):
        if getattr(self, "_streams", None) is None:
            self._streams = [torch.cuda.Stream(device=self.device) for _ in range(3)]
        return self._streams

    def forward_features(self, images, queries=None, concurrent=True, query_sizes=None, classes=1, bank=None, class_ids=None):
        """Target backbone on the current stream; the (independent, tiny) query backbone + pooling on a side stream
        (concurrent=False: one after the other on the current stream; OSD_LOCKSTEP=1: both backbones per launch, A/B).
        query_sizes: true (h, w) of every query of a padded batch (default: the tensor's size).
        classes = K (the class sweep): queries holds B*K*S rows; the target backbone runs on the B images once, the query branch pools
        B*K category slots of S shots, and `combined` has B*K rows (b*K + k) from one sweep launch over the B-row features.
        bank (+ class_ids, see detect) instead of queries: only the target backbone runs; `combined` is one gallery launch over the
        bank's pooled vectors, and the query features returned are None.
        supp_aug = A > 1: queries holds B*K*S*A rows; the query features returned are the merged ones (B*K*S rows), the backbone's own
        are kept in self.unmerged_query_features."""
        self.unmerged_query_features = None
        if bank is not None or queries is None:
            table = self._bank_table(images.shape[0], queries, bank, class_ids, classes)
            feats = run_backbone(self.backbone, images, self.dtype)
            return feats, None, bank.pooled, run_correlate(feats, None, table.classes, bank=bank, slots=table.dev)
        if class_ids is not None:
            raise ValueError("class_ids picks slots of a QueryBank: give bank= instead of queries")
        aug, method = self.supp_aug, self.supp_aug_method
        # one size per group, refused (nothing launched yet) where a group's members differ
        q_sizes = spec.group_query_sizes([tuple(queries.shape[-2:])] * queries.shape[0] if query_sizes is None else query_sizes, aug)
        if classes != 1:
            check_classes(images.shape[0], len(q_sizes), classes)
        batch = images.shape[0] * classes
        if concurrent and LOCKSTEP:
            feats, raw = run_backbones(self.backbone, self.supp_backbone, images, queries, self.dtype)
            qfeats = run_supp_aug(raw, aug, method)
            pooled = run_query_pool(qfeats, q_sizes, batch, self.supp_roialign)
        elif concurrent:
            main, side = _streams.current(), self.side_streams()[0]
            side.wait_stream(main)
            with _streams.on(side):
                raw = run_backbone(self.supp_backbone, queries, self.dtype)
                qfeats = run_supp_aug(raw, aug, method)
                pooled = run_query_pool(qfeats, q_sizes, batch, self.supp_roialign)
            feats = run_backbone(self.backbone, images, self.dtype)
            main.wait_stream(side)
        else:
            feats = run_backbone(self.backbone, images, self.dtype)
            raw = run_backbone(self.supp_backbone, queries, self.dtype)
            qfeats = run_supp_aug(raw, aug, method)
            pooled = run_query_pool(qfeats, q_sizes, batch, self.supp_roialign)
        if aug != 1:
            self.unmerged_query_features = raw
        combined = run_correlate(feats, pooled, classes)
        return feats, qfeats, pooled, combined

    def _bank_table(self, batch, queries, bank, class_ids, classes=1, second_stage=False):
        """The bank form's refusals (nothing launched yet) -> SlotTable."""
        if (queries is None) == (bank is None):
            raise ValueError("exactly one of queries and bank must be given (got %s)" % ("both" if bank is not None else "neither"))
        table = self.slot_table(bank, batch, class_ids, second_stage)
        if classes not in (1, table.classes):
            raise ValueError("classes = %d, but class_ids asks for %d slots per image (with a bank, leave classes alone)"
                             % (classes, table.classes))
        return table

    def forward(self, images, queries=None, concurrent=True, query_sizes=None, classes=1, bank=None, class_ids=None):
        """images [B,3,H,W], queries [B*S,3,h,w] NCHW fp32 on the device -> dict of NHWC intermediates.  classes = K: queries
        [B*K*S,3,h,w] (forward_features); `features` keeps B rows, everything per (image, category) has B*K, and out["classes"] = K.
        bank / class_ids: as detect's; out["classes"] = K, out["class_ids"] = the table's rows, and there is no out["query_features"]."""
        if bank is not None or queries is None:
            table = self._bank_table(images.shape[0], queries, bank, class_ids, classes)
            feats, _, pooled, combined = self.forward_features(images, None, concurrent, None, classes, bank, table)
            head = run_head(self.head, combined, self.side_streams() if concurrent else None)
            return dict(features=feats, pooled=pooled, combined=combined, head=head, classes=table.classes, class_ids=table.ids)
        feats, qfeats, pooled, combined = self.forward_features(images, queries, concurrent, query_sizes, classes, None, class_ids)
        head = run_head(self.head, combined, self.side_streams() if concurrent else None)
        out = dict(features=feats, query_features=qfeats, pooled=pooled, combined=combined, head=head)
        if self.supp_aug != 1:         # query_features are the merged maps; the query backbone's own, supp_aug rows per group
            out["query_features_unmerged"] = self.unmerged_query_features
        if classes != 1:
            out["classes"] = classes
        return out

    def detect(self, images, queries=None, training=False, cuda_nms=True, concurrent=True, second_stage=False, classes=1, bank=None,
               class_ids=None):
        """GeneralizedRCNN.forward in eval mode (generalized_rcnn.py:226-332): first stage -> out["proposals"] =
        (boxes [N,P,4], scores [N,P], counts [N]); with second_stage also the few-shot ROI box head ->
        out["detections"] = dict(boxes [N,K,4], scores [N,K] descending, counts [N]).
        classes = K (the class sweep, K category slots per image in one pass): queries holds B*K*S rows, row (b*K + k)*S + s = shot
        s of slot k of image b; the target backbone + FPN run once per image, and every output but out["features"] has N = B*K
        rows in the order b*K + k.  A row count that is no multiple of B*K is a ValueError before anything is launched.
        bank (the query gallery, instead of queries: exactly one of the two): a QueryBank from enroll(); class_ids = one sequence of K
        slot numbers per image (the same K for every image, repeats allowed), None = every slot in order (K = G).  Rows are b*K + k
        as with classes=K, out["classes"] = K, out["class_ids"] the table, no out["query_features"]; no query backbone, query pooling or
        query-half conv is launched.  check_class_ids refuses a bad table or bank (ValueError) before anything is launched."""
        from .layers import ImageList
        image_sizes = query_sizes = None
        if isinstance(images, ImageList):       # padded batch (R0): clip to every image's own size
            images, image_sizes = images.tensors, images.image_sizes
        elif isinstance(images, ops.PackedImages):
            image_sizes = images.image_sizes
        if bank is not None or queries is None:
            table = self._bank_table(images.shape[0], queries, bank, class_ids, classes, second_stage)
            if second_stage and (self.box_head is None or bank.q_half is None):
                raise KeyError("state_dict has no roi_heads.box.* entries: the second stage was not packed")
            if image_sizes is not None:
                image_sizes = [tuple(s) for s in image_sizes for _ in range(table.classes)]
            out = self.forward(images, None, concurrent, None, classes, bank, table)
            h, w = images.shape[-2:]
            pre = spec.PRE_NMS_TOP_N_TRAIN if training else spec.PRE_NMS_TOP_N_TEST
            post = spec.POST_NMS_TOP_N_TRAIN if training else spec.POST_NMS_TOP_N_TEST
            out["proposals"] = run_proposals(out["head"], h, w, pre, post, spec.NMS_THRESH, cuda_nms, image_sizes=image_sizes)
            if second_stage:
                out["detections"] = self.box_detect(out["features"], None, None, out["proposals"][0], out["proposals"][2], h, w,
                                                    cuda_nms=cuda_nms, image_sizes=image_sizes, bank=bank, class_ids=table)
            return out
        if class_ids is not None:
            raise ValueError("class_ids picks slots of a QueryBank: give bank= instead of queries")
        if isinstance(queries, ops.PackedImages):
            query_sizes = queries.image_sizes
        if isinstance(queries, ImageList):
            queries, query_sizes = queries.tensors, queries.image_sizes
        aug = self.supp_aug
        if aug != 1:                            # one size per group for everything behind the merge; unequal members refused here
            grouped = spec.group_query_sizes([tuple(queries.shape[-2:])] * queries.shape[0] if query_sizes is None else query_sizes, aug)
        if classes != 1:                        # the class sweep: the rest of this call runs on B*K rows, each image's true size K times
            check_classes(images.shape[0], queries.shape[0] // aug, classes)
            if image_sizes is not None:
                image_sizes = [tuple(s) for s in image_sizes for _ in range(classes)]
        shots = queries.shape[0] // (images.shape[0] * classes * aug)
        if second_stage:                        # refused before anything is launched
            from .box_head import check_shots
            check_shots(self.box_cls_loss, shots)
        out = self.forward(images, queries, concurrent, query_sizes, classes)
        h, w = images.shape[-2:]
        pre = spec.PRE_NMS_TOP_N_TRAIN if training else spec.PRE_NMS_TOP_N_TEST
        post = spec.POST_NMS_TOP_N_TRAIN if training else spec.POST_NMS_TOP_N_TEST
        out["proposals"] = run_proposals(out["head"], h, w, pre, post, spec.NMS_THRESH, cuda_nms, image_sizes=image_sizes)
        if second_stage:
            q_sizes = query_sizes if query_sizes is not None else tuple(queries.shape[-2:])
            if aug != 1 and query_sizes is not None:
                q_sizes = grouped
            out["detections"] = self.box_detect(out["features"], out["query_features"], q_sizes,
                                                out["proposals"][0], out["proposals"][2], h, w, shots=shots, cuda_nms=cuda_nms,
                                                image_sizes=image_sizes, classes=classes)
        return out

    def box_detect(self, feats, qfeats, q_size, boxes, counts, img_h, img_w, shots=1, cuda_nms=True, want_raw=False,
                   image_sizes=None, classes=1, bank=None, class_ids=None):
        """roi_heads.box on given proposals (boxes [N,R,4] fp32, counts [N] int32 or None).  q_size: (h, w) of all queries
        or a list with every query's true size; image_sizes: true (h, w) per image of a padded batch.
        classes = K (the class sweep): boxes / counts / image_sizes have N = B*K rows (b*K + k), feats B images, qfeats N*shots.
        bank / class_ids (the query gallery, qfeats = q_size = None): N = B*K rows for the table's K, the query halves come from
        the bank through the table and shots is the bank's."""
        if self.box_head is None:
            raise KeyError("state_dict has no roi_heads.box.* entries: the second stage was not packed")
        from .box_head import run_box_head
        if bank is not None or qfeats is None:
            batch = feats[0].shape[0]
            table = self._bank_table(batch, qfeats, bank, class_ids, classes, True)
            if bank.q_half is None:
                raise KeyError("the QueryBank was enrolled without a packed second stage")
            if batch * table.classes != boxes.shape[0]:
                raise ValueError("%d rows of proposals are not images x slots = %d x %d" % (boxes.shape[0], batch, table.classes))
            hw_dev = None if image_sizes is None else image_sizes_dev(image_sizes, boxes.device)
            return run_box_head(self.box_head, feats, None, None, boxes, counts, img_h, img_w, shots=bank.shots, cuda_nms=cuda_nms,
                                want_raw=want_raw, img_hw=hw_dev, classes=table.classes, bank=bank, slots=table.dev)
        hw_dev = None if image_sizes is None else image_sizes_dev(image_sizes, boxes.device)
        if classes != 1 and feats[0].shape[0] * classes != boxes.shape[0]:
            raise ValueError("%d rows of proposals are not images x classes = %d x %d" % (boxes.shape[0], feats[0].shape[0], classes))
        return run_box_head(self.box_head, feats, qfeats, q_size, boxes, counts, img_h, img_w, shots=shots,
                            cuda_nms=cuda_nms, want_raw=want_raw, img_hw=hw_dev, classes=classes)


class GraphedDetect(object):
    """The whole hot-path forward captured once into a hipGraph (static shapes, static HBM buffers) and replayed:
    ~250 kernel launches per step cost one graph launch on the host, and the multi-stream fork/join of
    HotPathEngine.forward becomes parallel branches of the graph."""

    def __init__(self, engine, images, queries=None, warmup=2, **kw):
        self.engine = engine
        self.images = images.clone()
        self.bank = kw.get("bank")
        if self.bank is not None or queries is None:
            # the query gallery: the slot table is a static device buffer of this graph; __call__ rewrites it (device to device, from
            # the content cache) before a replay, so ONE captured graph serves changing per-image category lists
            table = engine._bank_table(images.shape[0], queries, self.bank, kw.get("class_ids"), kw.get("classes", 1),
                                       bool(kw.get("second_stage")))
            self.slots = table.dev.clone()
            self.table = SlotTable(table.classes, table.ids, self.slots)
            self.queries = None
            kw = dict(kw, class_ids=self.table)
            engine.tune(self.images, None, second_stage=bool(kw.get("second_stage")), bank=self.bank, class_ids=self.table)
        else:
            self.queries = queries.clone()
            # classes: a sweep's head and box head run at B*K rows, and those are the shapes to tune
            engine.tune(self.images, self.queries, second_stage=bool(kw.get("second_stage")), classes=kw.get("classes", 1))
        side = torch.cuda.Stream(device=engine.device)
        side.wait_stream(_streams.current())
        with _streams.on(side):
            for _ in range(warmup):
                engine.detect(self.images, self.queries, **kw)
        _streams.current().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = engine.detect(self.images, self.queries, **kw)

    def __call__(self, images=None, queries=None, class_ids=None):
        if class_ids is not None:
            if self.bank is None:
                raise ValueError("class_ids picks slots of a QueryBank: this graph was captured with queries")
            k, flat = check_class_ids(self.engine, self.bank, self.images.shape[0], class_ids)      # on the host, before anything moves
            if k != self.table.classes:
                raise ValueError("class_ids asks for %d slots per image; the graph was captured with %d" % (k, self.table.classes))
            self.slots.copy_(slot_table_dev(flat, self.engine.device), non_blocking=True)
            self.table.ids = [list(flat[b * k:(b + 1) * k]) for b in range(self.images.shape[0])]
            self.out["class_ids"] = self.table.ids
        if images is not None:
            self.images.copy_(images, non_blocking=True)
        if queries is not None:
            if self.queries is None:
                raise ValueError("this graph was captured with a QueryBank: it takes no queries")
            self.queries.copy_(queries, non_blocking=True)
        self.graph.replay()
        return self.out
