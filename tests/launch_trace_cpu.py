"""Launch lists without a GPU.  The `ops` wrappers run on CPU tensors once the library call, the device check and the stream
lookups are stubbed (`stubbed_ops`); with `trace.TRACE = []` they then record every launch they would have made.  `signatures`
turns such a trace into plain data that two versions of the package can be compared on: tests/test_backbone_walker.py holds the
three backbone callers to the lists tests/record_backbone_launches.py recorded from the commit before the walker.

Everything here goes through names both versions have (ops.pack_conv, model.BackboneWeights' stem / blocks / fpn,
model.pack_conv3_downsample, ForwardPass._backbones_forward), so the recorder can import this module on top of either."""
import contextlib
import hashlib
import json
import types

import torch

IMAGE_SHAPES = {"even": ((2, 3, 64, 96), (2, 3, 32, 32)),      # layer1 maps 16x24 and 8x8
                "odd": ((2, 3, 28, 60), (2, 3, 28, 28))}        # layer1 maps 7x15 and 7x7: where the RES_DOWN2X policies differ
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
DRIVERS = ("run_backbone", "run_backbones", "train2", "train_target", "train_query")
SWITCHES = ("SKIP_UNUSED_C2", "RES_DOWN2X_OK", "FPN_OUT_GROUPED", "FUSE_DOWNSAMPLE")
TRAIN_SETTING = {"SKIP_UNUSED_C2": "skip_unused_c2", "FPN_OUT_GROUPED": "fpn_out_grouped"}


@contextlib.contextmanager
def stubbed_ops():
    """ops on CPU tensors: no library call, no device check, no stream.  Restores what it patched, the trace included."""
    from oneshotdet_amd import _lib, ops, trace
    saved = [(_lib, "call", _lib.call), (ops, "_chk_dev", ops._chk_dev), (ops, "_stream", ops._stream),
             (ops, "_stream_handle", ops._stream_handle), (trace, "TRACE", trace.TRACE)]
    _lib.call = lambda *a, **k: None
    ops._chk_dev = lambda *ts: None
    ops._stream = lambda: None
    ops._stream_handle = lambda: 0
    try:
        yield
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(e) for e in v]
    if isinstance(v, torch.dtype):
        return str(v)
    assert v is None or isinstance(v, (bool, int, float, str)), "not a scalar parameter: %r" % (v,)
    return v


def _tensor(t, label):
    return "%s %s %s" % (label, "x".join(str(d) for d in t.shape), str(t.dtype).replace("torch.", ""))


def signatures(records, names, inputs=()):
    """[(kind, {parameter: value})] -> one plain signature per record: [kind, {parameter: value}] with every scalar parameter as it
    is and every tensor operand as "<label> <shape> <dtype>".  The label says what the tensor is: its name in `names` ({data_ptr:
    name}, the packed weights and biases), "in<i>" for inputs[i], "out[k]" for the output of record number k (a record's own output
    included), else "torch": a tensor no record wrote, such as a strided copy.
    Records hold references to their tensors, so data_ptr() is a sound identity while `records` is alive.
    -> (signatures, label(t): the same labels for tensors kept outside the trace)."""
    known = dict(names)
    known.update((t.data_ptr(), "in%d" % i) for i, t in enumerate(inputs))

    def label(t):
        return known.get(t.data_ptr(), "torch")
    sigs = []
    for i, (kind, kw) in enumerate(records):
        if isinstance(kw.get("out"), torch.Tensor):
            known[kw["out"].data_ptr()] = "out[%d]" % i
        sigs.append([kind, {k: _tensor(v, label(v)) if isinstance(v, torch.Tensor) else _plain(v) for k, v in sorted(kw.items())}])
    return sigs, label


def digest(plain, chars=8):
    """A signature (or a labelled ctx) as the fixture keeps it: the first `chars` hex digits of the SHA-256 of its canonical JSON."""
    return hashlib.sha256(json.dumps(plain, sort_keys=True, separators=(",", ":")).encode()).hexdigest()[:chars]


def digests(got):
    """run_case's result as the fixture keeps it: one digest per launch (one string, blank-separated) and one per branch's ctx."""
    return {"launches": " ".join(digest(s) for s in got["launches"]),
            "ctxs": None if got["ctxs"] is None else [digest(c, 16) for c in got["ctxs"]]}


def state_dict():
    """Reference-named tensors of the hot path's shapes.  Ones: nothing here computes with them, and FrozenBN folds without a NaN."""
    from oneshotdet_amd import spec
    return {k: torch.ones(tuple(s)) for k, s in spec.hot_path_shapes().items()}


def weight_names(wts, prefix):
    """{data_ptr: name} of a BackboneWeights' packed tensors, named as the state_dict names their convs."""
    out = {}

    def add(name, pc):
        if pc is not None:
            out[pc.w.data_ptr()], out[pc.bias.data_ptr()] = name + ".w", name + ".b"
    from oneshotdet_amd import spec
    add(prefix + "body.stem.conv1", wts.stem)
    blocks = iter(wts.blocks)
    for si, nblocks in enumerate(spec.STAGE_BLOCKS):
        for bi in range(nblocks):
            blk, p = next(blocks), "%sbody.layer%d.%d." % (prefix, si + 1, bi)
            for key, name in (("c1", "conv1"), ("c2", "conv2"), ("c3", "conv3"), ("ds", "downsample.0"), ("c3ds", "conv3+downsample.0")):
                add(p + name, blk.get(key))
    for name, pc in wts.fpn.items():
        add(prefix + "fpn." + name, pc)
    return out


def train_self(sd, dtype, bbs, fused_l1=True, skip_unused_c2=True, fpn_out_grouped=True):
    """What ForwardPass._backbones_forward reads of a TrainEngine, packed from sd -> (the stand-in, {data_ptr: name})."""
    from oneshotdet_amd import model, ops
    convs, fused, names = {}, {}, {}

    def name(n, pc):
        names[pc.w.data_ptr()], names[pc.bias.data_ptr()] = n + ".w", n + ".b"
        return pc
    for key in sd:
        n = key[:-len(".weight")]
        if not (key.endswith(".weight") and key.startswith(tuple(bbs)) and sd[key].dim() == 4):
            continue
        if ".body." in key:
            bn = n.replace("stem.conv1", "stem.bn1").replace(".conv", ".bn").replace("downsample.0", "downsample.1")
            pc = ops.pack_conv(sd[key], bn=model._bn(sd, bn), dtype=dtype, stem=n.endswith("stem.conv1"))
        else:
            pc = ops.pack_conv(sd[key], bias=sd[n + ".bias"], dtype=dtype)
        convs[n] = types.SimpleNamespace(pc=name(n, pc))
    if fused_l1 and dtype == torch.bfloat16:
        for bb in dict.fromkeys(bbs):
            fused[bb] = name(bb + "body.layer1.0.conv3+downsample.0", model.pack_conv3_downsample(sd, bb + "body.layer1.0.", dtype))
    return types.SimpleNamespace(convs=convs, dtype=dtype, skip_unused_c2=skip_unused_c2, _fused_l1=fused,
                                 fpn_out_grouped=fpn_out_grouped), names


def label_ctx(ctx, label):
    """A training ctx (or any nest of dicts and lists) with every tensor replaced by its label, shape and dtype."""
    if isinstance(ctx, dict):
        return {k: label_ctx(v, label) for k, v in ctx.items()}
    if isinstance(ctx, (list, tuple)):
        return [label_ctx(v, label) for v in ctx]
    return _tensor(ctx, label(ctx)) if isinstance(ctx, torch.Tensor) else _plain(ctx)


def cases():
    """[(case id, dtype name, shape name, driver, options)]: the base grid, then at bf16 and the even shape each switch off in turn,
    the shared-backbone training form and a training call with an after_frozen hook."""
    out = [("%s-%s-%s" % (dt, shape, drv), dt, shape, drv, {}) for dt in DTYPES for shape in IMAGE_SHAPES for drv in DRIVERS]
    out += [("bf16-even-%s-no_%s" % (drv, sw), "bf16", "even", drv, {"off": sw}) for sw in SWITCHES for drv in DRIVERS]
    out.append(("bf16-even-train2-shared", "bf16", "even", "train2", {"shared": True}))
    out.append(("bf16-even-train2-after_frozen", "bf16", "even", "train2", {"after_frozen": True}))
    return out


def run_case(sd, dtype_name, shape_name, driver, options):
    """One driver under the stub -> {"launches": signatures, "ctxs": labelled ctx dicts (training drivers only)}."""
    from oneshotdet_amd import model, trace
    from oneshotdet_amd.train_forward import ForwardPass
    dtype, off = DTYPES[dtype_name], options.get("off")
    images, queries = (torch.zeros(s) for s in IMAGE_SHAPES[shape_name])
    saved = {sw: getattr(model, sw) for sw in SWITCHES}
    with stubbed_ops():
        try:
            if off is not None:
                setattr(model, off, False)
            trace.TRACE = records = []
            ctxs = None
            if driver.startswith("run_"):
                wt, wq = model.BackboneWeights(sd, "backbone.", dtype), model.BackboneWeights(sd, "supp_backbone.", dtype)
                names = weight_names(wt, "backbone.")
                names.update(weight_names(wq, "supp_backbone."))
                inputs = (images,) if driver == "run_backbone" else (images, queries)
                if driver == "run_backbone":
                    model.run_backbone(wt, images, dtype)
                else:
                    model.run_backbones(wt, wq, images, queries, dtype)
            else:
                bbs = ("backbone.", "backbone.") if options.get("shared") else ("backbone.", "supp_backbone.")
                pick = {"train2": slice(0, 2), "train_target": slice(0, 1), "train_query": slice(1, 2)}[driver]
                me, names = train_self(sd, dtype, bbs, fused_l1=off != "FUSE_DOWNSAMPLE",
                                       **{v: off != k for k, v in TRAIN_SETTING.items()})
                inputs = (images, queries)[pick]
                hook = (lambda: trace.rec("marker", name="after_frozen")) if options.get("after_frozen") else None
                _, ctxs = ForwardPass._backbones_forward(me, bbs[pick], inputs, hook)
            sigs, label = signatures(records, names, inputs)
            return {"launches": sigs, "ctxs": None if ctxs is None else label_ctx(ctxs, label)}
        finally:
            for sw, v in saved.items():
                setattr(model, sw, v)
