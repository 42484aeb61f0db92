"""GPU (-m gpu): the MEASURED configuration's arithmetic (bf16 engines) checked LAUNCH BY LAUNCH.

End to end a bf16 pipeline can only be compared loosely with an fp32 reference, and — tests/test_oracle_golden.py shows it
on the CPU — just as loosely with ANY other bf16 implementation of itself: a 1e-6 perturbation of the weights moves the
rounded pipeline's gradients by 0.16-0.25 relative L2, as much as bf16 differs from fp32, because every stored tensor is
re-rounded to 8 bits ~60 times in a row.  So a kernel bug worth 10 % of a gradient tensor could hide under any honest
end-to-end bf16 tolerance.  It cannot hide here: `oneshotdet_amd.trace.TRACE` records every launch of a REAL forward / training
step (same engines, same streams), and each one is recomputed on the CPU by oracle/launch_replay.py FROM THE ENGINE'S OWN
INPUT TENSORS (teacher forcing) in fp32 and rounded once.  Bars, per launch:
  bf16 outputs   every element within ONE bf16 unit in the last place of the restatement (+ 1e-5 x the tensor's absmax for
                 fp32 summation order), i.e. the kernel lands on the nearest or the neighbouring bf16 value, never further;
                 at most 2 % of a tensor's elements on the neighbour
  fp32 outputs   1e-4 relative + 1e-5 x absmax (pooled vectors, query gradients)
  weight / bias / GroupNorm-affine gradients (fp32 accumulations over up to 10^5 pixels): 2e-4 x the tensor's absmax,
                 cosine >= 0.99999
and the chain's coverage is asserted: every conv, GroupNorm, correlation, pooling, loss-gradient and weight-gradient launch
of the step is replayed, and every trainable tensor's gradient is accounted for by the replayed launches."""
import time

import numpy as np
import pytest
import torch

import conv_ref as cr
import golden_utils as gu
from oneshotdet_amd import spec, synth
from oracle import launch_replay as lr

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def cpu(t):
    return None if t is None else t.detach().cpu()


class Replayer(object):
    """Walks a launch trace, recomputes each launch on the CPU from the recorded inputs and checks the recorded output."""

    def __init__(self, flip_cap=0.02):
        self.flip_cap = flip_cap
        self.counts = {}
        self.worst = {}
        self.acc = {}          # data_ptr of an accumulated fp32 gradient tensor -> [engine tensor, replayed sum]
        self.failures = []

    def _check(self, kind, got, ref, what=""):
        res = lr.compare(cpu(got), ref, got.dtype)
        self.counts[kind] = self.counts.get(kind, 0) + 1
        key = "worst_ulp" if got.dtype == torch.bfloat16 else "worst_rel"
        w = self.worst.setdefault(kind, {"worst_ulp": 0.0, "worst_rel": 0.0, "flips": 0.0})
        w[key] = max(w[key], res.get(key, 0.0))
        w["flips"] = max(w["flips"], res["flips"])
        if not res["ok"] or res["flips"] > self.flip_cap:
            self.failures.append((kind, what, tuple(got.shape), res))
        return res

    def _accumulate(self, tensor, value):
        slot = self.acc.setdefault(tensor.data_ptr(), [tensor, torch.zeros(tensor.shape, dtype=torch.float32)])
        slot[1] += value.reshape(tensor.shape)

    def run(self, trace):
        for kind, r in trace:
            getattr(self, "do_" + kind)(r)

    # ---- one method per launch kind
    def do_pack_image(self, r):
        self._check("pack_image", r["out"], lr.pack_image_launch(cpu(r["x"]), tuple(r["out"].shape), r["pad_t"], r["pad_l"]))

    def do_conv(self, r):
        out = r["out"]
        ref = lr.conv_launch(cpu(r["x"]), cpu(r["w"]), cpu(r["bias"]), r["cout"], r["r"], r["s"], stem=r["stem"], stride=r["stride"],
                             pad=r["pad"], act=r["act"], res=cpu(r["res"]), res_mode=r["res_mode"], relu_in=r["relu_in"],
                             act_scale=r["act_scale"], act_scale_dev=cpu(r["act_scale_dev"]), mask=cpu(r["mask"]),
                             x2=cpu(r.get("x2")), x2_stride=r.get("x2_stride", 1), w2=cpu(r.get("w2")),
                             out_hw=tuple(out.shape[1:3]))
        kind = "conv%dx%d%s" % (r["r"], r["s"], "_src2" if r.get("x2") is not None else "")
        self._check(kind, out, ref, "stride %d act %d res %d mask %d" % (r["stride"], r["act"], r["res_mode"], r["mask"] is not None))

    def do_maxpool(self, r):
        self._check("maxpool", r["out"], lr.maxpool_launch(cpu(r["x"])))

    def do_roi_align(self, r):
        self._check("roi_align", r["out"], lr.roi_align_launch(cpu(r["x"]), cpu(r["rois"]), r["scale"], r["ph"], r["pw"],
                                                              r["sampling_ratio"]))

    def do_roi_align_bwd(self, r):
        self._check("roi_align_bwd", r["out"], lr.roi_align_bwd_launch(cpu(r["gy"]), cpu(r["rois"]), tuple(r["out"].shape), r["scale"],
                                                                      r["ph"], r["pw"], r["sampling_ratio"]))

    def do_query_pool(self, r):
        refs = lr.query_pool_launch([cpu(x) for x in r["xs"]], cpu(r["rois"]), r["scales"], r["batch"], r["sampling_ratio"])
        for out, ref in zip(r["outs"], refs):
            self._check("query_pool", out, ref)

    def do_query_pool_bwd(self, r):
        refs = lr.query_pool_bwd_launch([cpu(d) for d in r["dqs"]], cpu(r["rois"]), [tuple(o.shape) for o in r["outs"]], r["scales"],
                                        r["shots"], r["sampling_ratio"])
        for out, ref in zip(r["outs"], refs):
            self._check("query_pool_bwd", out, ref)

    def do_shot_mean(self, r):
        self._check("shot_mean", r["out"], lr.shot_mean_launch(cpu(r["x"]), r["batch"]))

    def do_shot_mean_bwd(self, r):
        self._check("shot_mean_bwd", r["out"], lr.shot_mean_bwd_launch(cpu(r["gy"]), r["shots"]))

    def do_correlate(self, r):
        self._check("correlate", r["out"], lr.correlate_launch(cpu(r["x"]), cpu(r["q"])))

    def do_correlate_bwd_query(self, r):
        self._check("correlate_bwd_query", r["out"], lr.correlate_bwd_query_launch(cpu(r["g"]), cpu(r["feat"])))

    def do_add_mask(self, r):
        self._check("add_mask", r["out"], lr.add_mask_launch(cpu(r["a"]), cpu(r["b"]), cpu(r["mask"])))

    def do_scatter2x(self, r):
        self._check("scatter2x", r["out"], lr.scatter2x_launch(cpu(r["x"]), tuple(r["out"].shape[1:3]), cpu(r["mask"]), cpu(r["addend"])))

    def do_upsample2x_bwd(self, r):
        self._check("upsample2x_bwd", r["out"], lr.upsample2x_bwd_launch(cpu(r["inner"]), cpu(r["prev"])))

    def do_cast(self, r):
        self._check("cast", r["out"], cpu(r["x"]).float())

    def do_gn_relu(self, r):
        self._check("gn_relu", r["out"], lr.gn_relu_launch(cpu(r["x"]), cpu(r["gamma"]), cpu(r["beta"]), r["groups"], r["eps"]))

    def do_gn_relu_bwd(self, r):
        for u, dt, du in zip(r["us"], r["dts"], r["outs"]):
            ref, dg, db = lr.gn_relu_bwd_launch(cpu(u), cpu(dt), cpu(r["gamma"]), cpu(r["beta"]), r["groups"], spec.GN_EPS)
            self._check("gn_relu_bwd", du, ref)
            self._accumulate(r["dgamma"], dg)
            self._accumulate(r["dbeta"], db)
            if r.get("conv_db") is not None:      # the producing conv's bias gradient = sum of du over images and pixels
                self._accumulate(r["conv_db"], ref.double().sum(dim=(0, 1, 2)).float())

    def do_wgrad(self, r):
        self.counts["wgrad"] = self.counts.get("wgrad", 0) + 1
        for it in r["items"]:
            dw, db = lr.wgrad_launch(cpu(it["x"]), cpu(it["dy"]), it["r"], it["s"], it["stride"], it["pad"], it["cout"],
                                     scale=cpu(it["scale"]), want_bias=it["db"] is not None)
            self._accumulate(it["dw"], dw)
            if it["db"] is not None:
                self._accumulate(it["db"], db)

    def do_pred_gather(self, r):
        self._check("pred_gather", r["out"], lr.pred_gather_launch([cpu(t) for t in r["dys"]]))

    def do_pred_dgrad_pack(self, r):
        self._check("pred_dgrad_pack", r["out"], lr.pred_dgrad_pack_launch(cpu(r["w"]), r["cout"], r["cin"]))

    def do_fcos_loss(self, r):
        if r["phase"] != 1:
            return
        outs, raws, _ = lr.fcos_loss_grad_launch([(cpu(c), cpu(g)) for c, g in r["head_out"]], cpu(r["gt_boxes"]), cpu(r["gt_count"]),
                                                 [float(cpu(s).reshape(-1)[0]) for s in r["scale_devs"]], r["gamma"], r["alpha"])
        for lvl, (d_cc, d_x) in enumerate(outs):
            self._check("fcos_loss_grad", r["d_cls_ctrs"][lvl][..., :2], d_cc, "level %d cls/ctr" % lvl)
            self._check("fcos_loss_grad", r["d_regs"][lvl][..., :4], d_x, "level %d reg" % lvl)

    # ---- accumulated fp32 gradients (each is written by the launches of ONE step, from zero)
    def check_accumulated(self, tol=2e-4):
        worst = 0.0
        for ptr, (tensor, ref) in self.acc.items():
            got = cpu(tensor).float().reshape(ref.shape)
            scale = float(ref.abs().max())
            if scale == 0.0:
                assert float(got.abs().max()) == 0.0
                continue
            err = float((got - ref).abs().max()) / scale
            cos = float((got * ref).sum() / (got.norm() * ref.norm()).clamp_min(1e-30))
            worst = max(worst, err)
            if err > tol or cos < 0.99999:
                self.failures.append(("accumulated gradient", tuple(ref.shape), err, cos))
        return worst


def _train_engine(dt, name):
    from oneshotdet_amd import train
    B, H, W, S, qh, qw = gu.CASES[name]
    img, q = gu.case_inputs(name)
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    eng = train.TrainEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=DT[dt])
    G = max(len(g) for g in gts)
    gtb = torch.zeros(B, G, 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    cnt = torch.tensor([len(g) for g in gts], dtype=torch.int32)
    return eng, torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), gtb.cuda(), cnt.cuda()


def _traced(fn):
    from oneshotdet_amd import ops
    from oneshotdet_amd import trace
    trace.TRACE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, trace.TRACE
    finally:
        trace.TRACE = None


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["small", "shots5", "nonsquare"])
def test_every_launch_of_a_training_step_matches_its_cpu_restatement(name, dt):
    """R0-R12 + backward (engine/trainer.py:79-93 up to the optimiser): forward, loss gradient, data gradients, GroupNorm /
    correlation / pooling backward and every weight gradient of one real training step, each launch from its own inputs."""
    eng, img, q, gtb, cnt = _train_engine(dt, name)
    eng.forward_backward(img, q, gtb, cnt, with_proposals=False)      # warm-up: allocations, persistent buffers
    torch.cuda.synchronize()
    _, trace = _traced(lambda: eng.forward_backward(img, q, gtb, cnt, with_proposals=False))
    rp = Replayer()
    rp.run(trace)
    worst_acc = rp.check_accumulated()
    print("\n%s %s: %d launches replayed: %s\n  worst per kind: %s\n  worst accumulated-gradient error %.2e of absmax over %d tensors"
          % (name, dt, len(trace), rp.counts, {k: {a: round(b, 4) for a, b in v.items()} for k, v in rp.worst.items()}, worst_acc,
             len(rp.acc)))
    assert not rp.failures, rp.failures[:6]
    # coverage: the step's launch kinds are all there ...
    for kind in ("pack_image", "conv1x1", "conv3x3", "conv7x1", "maxpool", "query_pool", "correlate", "gn_relu",
                 "fcos_loss_grad", "gn_relu_bwd", "correlate_bwd_query", "query_pool_bwd", "wgrad", "add_mask",
                 "scatter2x", "upsample2x_bwd", "pred_gather", "pred_dgrad_pack"):
        assert rp.counts.get(kind, 0) > 0, "no %s launch in the trace" % kind
    # ... and every trainable conv weight / bias / GroupNorm affine gradient was produced by replayed launches
    flat_lo, flat_hi = eng.flat_g.data_ptr(), eng.flat_g.data_ptr() + eng.flat_g.numel() * 4
    covered = sum(ref.numel() for t, ref in rp.acc.values() if flat_lo <= t.data_ptr() < flat_hi)
    total = sum(int(np.prod(s)) for n_, s in eng._plan if n_ != "rpn.head.scales")
    assert covered == total, (covered, total)


@pytest.mark.parametrize("name", ["small", "shots5"])
def test_every_launch_of_the_inference_forward_matches_its_cpu_restatement(name):
    """HotPathEngine.detect (bf16): the inference engine takes other kernels than the training engine — conv3 + downsample of
    every stage's first block as ONE two-source GEMM, relu(P6) as a conv prologue — replayed the same way."""
    from oneshotdet_amd import model
    img, q = gu.case_inputs(name)
    eng = model.HotPathEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=torch.bfloat16)
    img, q = torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda()
    eng.forward(img, q)
    torch.cuda.synchronize()
    _, trace = _traced(lambda: eng.forward(img, q))
    rp = Replayer()
    rp.run(trace)
    print("\n%s inference bf16: %d launches: %s\n  worst per kind: %s" % (name, len(trace), rp.counts, rp.worst))
    assert not rp.failures, rp.failures[:6]
    assert rp.counts.get("conv1x1_src2", 0) == 8, rp.counts      # 4 stages x 2 backbones


def test_every_launch_at_the_benchmark_geometry_matches_its_cpu_restatement():
    """One 800x1024 target + 127x127 query (BASELINE.json configs[0] geometry = one image of the measured bs=8 step), bf16:
    the kernels the tuner picks at THIS size (256x256 / row-reuse tiles, grouped tower launches, multi-segment weight
    gradients) are the ones replayed.  ~1 TFLOP of CPU convolutions."""
    from oneshotdet_amd import ops
    eng, img, q, gtb, cnt = _train_engine("bf16", "config1")
    with ops.tuning():
        eng.forward_backward(img, q, gtb, cnt, with_proposals=False)
    torch.cuda.synchronize()
    _, trace = _traced(lambda: eng.forward_backward(img, q, gtb, cnt, with_proposals=False))
    rp = Replayer()
    rp.run(trace)
    worst_acc = rp.check_accumulated()
    print("\nconfig1 bf16: %d launches: %s\n  worst per kind: %s\n  worst accumulated-gradient error %.2e"
          % (len(trace), rp.counts, rp.worst, worst_acc))
    assert not rp.failures, rp.failures[:6]


class Fp64Replayer(Replayer):
    """The Replayer with every conv and weight-gradient launch recomputed in float64 ON THE GPU (tests/conv_ref.py: sums of shifted
    matmuls) — the benchmark's batch of eight 800 x 1024 images costs seconds there instead of many minutes of CPU convolutions —
    and each launch's (kind, algorithm) recorded: `by_algo` (kind, algo) -> [launches, worst error], `seen` the (tuner key, algo)
    of every replayed conv / weight-gradient launch.  The other launch kinds keep the CPU restatement.  Accumulated gradients are
    summed in float64 on the GPU."""

    def __init__(self, flip_cap=0.02):
        super().__init__(flip_cap)
        self.by_algo = {}
        self.seen = set()
        self.writers = {}          # data_ptr of an accumulated gradient -> {(kind, algo) of the launches that added into it}

    def _accumulate(self, tensor, value):
        slot = self.acc.setdefault(tensor.data_ptr(), [tensor, torch.zeros(tensor.shape, dtype=torch.float64, device="cuda")])
        slot[1] += value.to("cuda", torch.float64).reshape(tensor.shape)

    def _note(self, kind, algo, err):
        ent = self.by_algo.setdefault((kind, algo), [0, 0.0])
        ent[0] += 1
        ent[1] = max(ent[1], err)

    def do_conv(self, r):
        out = r["out"]
        sc = float(r["act_scale_dev"].float().reshape(-1)[0]) if r["act_scale_dev"] is not None else r["act_scale"]
        if r["stem"]:           # the packed NHWC4 image already carries the padding: 7 x 8 taps, stride 2, cropped to the output
            ref = cr.conv_fwd(r["x"], lr.unpack_weight(r["w"], r["cout"], stem=True), r["bias"], stride=2, act=r["act"],
                              out_hw=tuple(out.shape[1:3]))
        else:
            w = lr.unpack_weight(r["w"], r["cout"])
            x2, w2 = r.get("x2"), None
            if x2 is not None:
                c1, c2 = r["x"].shape[-1], x2.shape[-1]
                w2 = w[:, c1:c1 + c2] if r.get("w2") is None else lr.unpack_weight(r["w2"], r["cout"])[:, :c2]
                w = w[:, :c1]
            ref = cr.conv_fwd(r["x"], w, r["bias"], stride=r["stride"], pad=r["pad"], res=r["res"], res_mode=r["res_mode"],
                              mask=r["mask"], act=r["act"], act_scale=sc, relu_in=r["relu_in"], x2=x2, w2=w2,
                              x2_stride=r.get("x2_stride", 1))
        kind = "conv%dx%d%s" % (r["r"], r["s"], "_src2" if r.get("x2") is not None else "")
        res = self._check(kind, out, ref.float().cpu(), "algo %s stride %d act %d res %d mask %d" % (
            r.get("algo"), r["stride"], r["act"], r["res_mode"], r["mask"] is not None))
        self._note(kind, r.get("algo"), res["worst_ulp"] if out.dtype == torch.bfloat16 else res["worst_rel"])
        self.seen.add((r.get("key"), r.get("algo")))

    def do_wgrad(self, r):
        self.counts["wgrad"] = self.counts.get("wgrad", 0) + 1
        self._note("wgrad", r.get("algo"), 0.0)
        self.seen.add((r.get("key"), r.get("algo")))
        for it in r["items"]:
            dw, db = cr.conv_wgrad(it["x"], it["dy"], it["r"], it["s"], it["stride"], it["pad"], it["cout"], scale=it["scale"],
                                   want_bias=it["db"] is not None)
            self._accumulate(it["dw"], dw)
            self.writers.setdefault(it["dw"].data_ptr(), set()).add(("wgrad", r.get("algo")))
            if it["db"] is not None:
                self._accumulate(it["db"], db)
                self.writers.setdefault(it["db"].data_ptr(), set()).add(("wgrad", r.get("algo")))

    def check_accumulated(self, tol=cr.ACC_TOL):
        """The accumulated-gradient bar of tests/conv_ref.py per tensor; each tensor's error is also charged to the weight-gradient
        launches that wrote it (by_algo)."""
        worst = 0.0
        for ptr, (tensor, ref) in self.acc.items():
            res = cr.check_accumulated(tensor.float(), ref, tol=tol)
            worst = max(worst, res["err"])
            for ka in self.writers.get(ptr, ()):
                self.by_algo[ka][1] = max(self.by_algo[ka][1], res["err"])
            if not res["ok"]:
                self.failures.append(("accumulated gradient", tuple(ref.shape), res))
        return worst


def _bench_batch(dt):
    """bench.py's default training batch: 8 distinct 800 x 1024 targets, their queries and box sets (rank 0's seeds)."""
    from oneshotdet_amd import train
    B = 8
    images = torch.from_numpy(synth.make_images("bench.target", B, 800, 1024, seed=1000)).cuda()
    queries = torch.from_numpy(synth.make_images("bench.query", B, 127, 127, seed=1000)).cuda()
    gts = synth.make_gt_boxes(B, 800, 1024, seed=1000, max_boxes=6)
    gtb = torch.zeros(B, 6, 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    cnt = torch.tensor([len(g) for g in gts], dtype=torch.int32)
    eng = train.TrainEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=DT[dt])
    return eng, images, queries, gtb.cuda(), cnt.cuda()


def test_every_launch_of_the_tuned_batch8_benchmark_step_matches_its_restatement():
    """bench.py's measured configuration: the bf16 training step at bs = 8 (800 x 1024) with the kernels `ops.tuning()` picks for
    THESE shapes (the tuner's choices depend on the pixel count: deep-ring tiles, weight-gradient split targets, team / owner mode and
    the grouped split points differ from bs = 1), the default schedule (streams, one-pass GroupNorm).  One tuned step, then a traced
    step replayed launch by launch with the bars above — conv and weight-gradient launches against their float64 restatement on the
    GPU.  Coverage: every tuner-cache key the step consulted was replayed with the algorithm cached for it, and every trainable
    tensor's gradient is accounted for."""
    from oneshotdet_amd import ops
    t0 = time.time()
    eng, img, q, gtb, cnt = _bench_batch("bf16")
    with ops.tuning():
        eng.forward_backward(img, q, gtb, cnt, with_proposals=False)
    torch.cuda.synchronize()
    t_tune = time.time() - t0
    caches = {"ALGO_CACHE": ops.ALGO_CACHE, "WGRAD_ALGO_CACHE": ops.WGRAD_ALGO_CACHE, "SPLIT_CACHE": ops.SPLIT_CACHE}
    for c in caches.values():
        c.hits = {}
        c.census = True
    try:
        _, trace = _traced(lambda: eng.forward_backward(img, q, gtb, cnt, with_proposals=False))
    finally:
        for c in caches.values():
            c.census = False
    t1 = time.time()
    rp = Fp64Replayer()
    rp.run(trace)
    worst_acc = rp.check_accumulated()
    table = "\n".join("  %-12s algo %-5s %4d launches  worst %s %.3g" % (k, a, n, "ulp" if k != "wgrad" else "acc", w)
                      for (k, a), (n, w) in sorted(rp.by_algo.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))))
    print("\nbs=8 tuned bf16 step: tuning + step %.1f s, replay of %d launches %.1f s\n%s\n  other kinds: %s\n  worst accumulated-gradient "
          "error %.2e of absmax over %d tensors" % (t_tune, len(trace), time.time() - t1, table,
                                                   {k: {a: round(b, 4) for a, b in v.items()} for k, v in rp.worst.items() if not k.startswith("conv")},
                                                   worst_acc, len(rp.acc)))
    assert not rp.failures, rp.failures[:6]
    # coverage: every key the traced step looked up was tuned, and a replayed launch ran the cached algorithm under it
    for name, c in caches.items():
        missing = [k for k in c.hits if k not in c]
        assert not missing, (name, missing[:4])
        if name != "SPLIT_CACHE":       # (a split point shows as the grouped launches it produced: their own keys above)
            unseen = [k for k in c.hits if (k, c[k]) not in rp.seen]
            assert not unseen, (name, unseen[:4])
    assert ops.ALGO_CACHE.hits and ops.WGRAD_ALGO_CACHE.hits
    for kind in ("conv1x1", "conv3x3", "conv7x1", "wgrad", "gn_relu", "gn_relu_bwd", "fcos_loss_grad"):
        assert any(k == kind for k, _ in rp.by_algo) or rp.counts.get(kind, 0) > 0, "no %s launch in the trace" % kind
    flat_lo, flat_hi = eng.flat_g.data_ptr(), eng.flat_g.data_ptr() + eng.flat_g.numel() * 4
    covered = sum(ref.numel() for t, ref in rp.acc.values() if flat_lo <= t.data_ptr() < flat_hi)
    total = sum(int(np.prod(s)) for n_, s in eng._plan if n_ != "rpn.head.scales")
    assert covered == total, (covered, total)
