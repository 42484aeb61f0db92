"""The launch replayers (test helper, imported like conv_ref): walk a trace of `oneshotdet_amd.trace.TRACE`, recompute every
recorded launch from the engine's OWN input tensors by oracle/launch_replay.py, hold what the kernel stored to one rounding of
that restatement, and account for every accumulated gradient.  tests/test_gpu_launch_replay.py states the bars and why the bf16
engines are checked this way; tests/test_gpu_launch_replay_options.py replays the engines' other modes with the same objects.

A record whose kind has no `do_<kind>` method is a failure of the replay (LookupError), never skipped; the inventory in
tests/test_launch_replay_restatements.py holds every kind `ops.py` records to a method here or to a reasoned NOT_REPLAYED entry."""
import numpy as np
import torch

import conv_ref as cr
from oneshotdet_amd import spec
from oracle import launch_replay as lr

SCALES = "rpn.head.scales"            # the five learnable Scale scalars of the head (fcos.py:81), one trainable tensor of the plan
SCALE_RAW_TOL = 1e-4                  # x sum |terms|: the bound tests/test_gpu_fcos_loss_modes.py holds the Scale's raw sum to


def cpu(t):
    return None if t is None else t.detach().cpu()


def _traced(fn):
    from oneshotdet_amd import trace
    trace.TRACE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, trace.TRACE
    finally:
        trace.TRACE = None


class Replayer(object):
    """Walks a launch trace, recomputes each launch on the CPU from the recorded inputs and checks the recorded output.
    engine: the TrainEngine whose step is replayed — its Scale-gradient view (`extra["rpn.head.scales"]`) is what the loss's
    finalize launch adds `raw / scale` into, so with it the Scale gradient joins the accumulated gradients."""

    def __init__(self, flip_cap=0.02, engine=None):
        self.flip_cap = flip_cap
        self.counts = {}
        self.worst = {}
        self.acc = {}          # data_ptr of an accumulated fp32 gradient tensor -> [engine tensor, replayed sum]
        self.failures = []
        self.scale_grad = None if engine is None else engine.extra[SCALES][1]
        self.loss_info = None  # (cls, reg, centerness, num_pos) of the last replayed loss-gradient launch's restatement

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
            do = getattr(self, "do_" + kind, None)
            if do is None:
                raise LookupError("no restatement for launch kind %r" % (kind,))
            do(r)

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

    def do_query_avgpool(self, r):
        refs = lr.query_avgpool_launch([cpu(x) for x in r["xs"]], r["batch"])
        for lvl, (out, ref) in enumerate(zip(r["outs"], refs)):
            self._check("query_avgpool", out, ref, "level %d" % lvl)

    def do_query_avgpool_bwd(self, r):
        refs = lr.query_avgpool_bwd_launch([cpu(d) for d in r["dqs"]], [tuple(o.shape) for o in r["outs"]], r["shots"])
        for lvl, (out, ref) in enumerate(zip(r["outs"], refs)):
            self._check("query_avgpool_bwd", out, ref, "level %d" % lvl)

    def do_supp_aug_reduce(self, r):
        refs = lr.supp_aug_reduce_launch([cpu(x) for x in r["xs"]], r["aug"], r["method"])
        for lvl, (out, ref) in enumerate(zip(r["outs"], refs)):
            self._check("supp_aug_reduce", out, ref, "%s level %d" % (r["method"], lvl))

    def do_supp_aug_reduce_bwd(self, r):
        refs = lr.supp_aug_reduce_bwd_launch([cpu(x) for x in r["xs"]], [cpu(d) for d in r["dys"]], r["aug"], r["method"])
        for lvl, (out, ref) in enumerate(zip(r["outs"], refs)):
            self._check("supp_aug_reduce_bwd", out, ref, "%s level %d" % (r["method"], lvl))

    def do_shot_mean(self, r):
        self._check("shot_mean", r["out"], lr.shot_mean_launch(cpu(r["x"]), r["batch"]))

    def do_shot_mean_bwd(self, r):
        self._check("shot_mean_bwd", r["out"], lr.shot_mean_bwd_launch(cpu(r["gy"]), r["shots"]))

    def do_correlate(self, r):
        self._check("correlate", r["out"], lr.correlate_launch(cpu(r["x"]), cpu(r["q"])))

    def do_correlate_sweep(self, r):
        self._check("correlate_sweep", r["out"], lr.correlate_sweep_launch(cpu(r["x"]), cpu(r["q"]), r["classes"]))

    def do_correlate_gallery(self, r):
        self._check("correlate_gallery", r["out"], lr.correlate_gallery_launch(cpu(r["x"]), cpu(r["q"]), cpu(r["slots"]), r["classes"]))

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
        """Phase 1 (phase 0 writes the loss sums only): the stored gradients in the record's mode, and the Scale parameters' raw
        sums d_scale_raws[l] = sum d/dreg * reg * log(reg) — fp32 atomic adds in any order, held to SCALE_RAW_TOL x sum |terms| of
        the restatement (tests/test_gpu_fcos_loss_modes.py).  The finalize launch that follows (osd_fcos_loss_finalize_scales,
        train_forward.loss_and_grads) adds raw[l] / scale[l] into the engine's Scale gradient: restated from ITS inputs, the raw
        sums the kernel stored, it is accumulated for check_accumulated like every other gradient of the plan."""
        if r["phase"] != 1:
            return
        scales = [float(cpu(s).reshape(-1)[0]) for s in r["scale_devs"]]
        outs, raws, raw_abs, self.loss_info = lr.fcos_loss_grad_launch(
            [(cpu(c), cpu(g)) for c, g in r["head_out"]], cpu(r["gt_boxes"]), cpu(r["gt_count"]), scales, r["gamma"], r["alpha"],
            center_sample=r["center_sample"], loc_loss_type=r["loc_loss_type"])
        for lvl, (d_cc, d_x) in enumerate(outs):
            self._check("fcos_loss_grad", r["d_cls_ctrs"][lvl][..., :2], d_cc, "level %d cls/ctr" % lvl)
            self._check("fcos_loss_grad", r["d_regs"][lvl][..., :4], d_x, "level %d reg" % lvl)
        got = [float(cpu(t).double().reshape(-1)[0]) for t in r["d_scale_raws"]]
        w = self.worst.setdefault("fcos_scale_raw", {"worst_ulp": 0.0, "worst_rel": 0.0, "flips": 0.0})
        for lvl, (g, want, mag) in enumerate(zip(got, raws, raw_abs)):
            self.counts["fcos_scale_raw"] = self.counts.get("fcos_scale_raw", 0) + 1
            err = abs(g - want)
            w["worst_rel"] = max(w["worst_rel"], err / (SCALE_RAW_TOL * mag + 1e-12))       # in units of the bound
            if not np.isfinite(g) or err > SCALE_RAW_TOL * mag + 1e-12:
                self.failures.append(("fcos_scale_raw", "level %d" % lvl, g, want, mag))
        if self.scale_grad is not None:
            value = torch.zeros(self.scale_grad.shape, dtype=torch.float64)
            for lvl, (g, s) in enumerate(zip(got, scales)):
                value[lvl] = g / s
            self._accumulate(self.scale_grad, value)

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


class Fp64Replayer(Replayer):
    """The Replayer with every conv and weight-gradient launch recomputed in float64 ON THE GPU (tests/conv_ref.py: sums of shifted
    matmuls) — the benchmark's batch of eight 800 x 1024 images costs seconds there instead of many minutes of CPU convolutions —
    and each launch's (kind, algorithm) recorded: `by_algo` (kind, algo) -> [launches, worst error], `seen` the (tuner key, algo)
    of every replayed conv / weight-gradient launch.  The other launch kinds keep the CPU restatement.  Accumulated gradients are
    summed in float64 on the GPU.  `writers`: data_ptr of an accumulated gradient -> {(kind, algo)} of the launches that added into
    it; `wgrad_rows`: the same key -> the batch sizes (rows of x) of the weight-gradient items that added into it, in order."""

    def __init__(self, flip_cap=0.02, engine=None):
        super().__init__(flip_cap, engine)
        self.by_algo = {}
        self.seen = set()
        self.writers = {}          # data_ptr of an accumulated gradient -> {(kind, algo) of the launches that added into it}
        self.wgrad_rows = {}

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
            self.wgrad_rows.setdefault(it["dw"].data_ptr(), []).append(int(it["x"].shape[0]))
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


# ---- coverage
# the launch kinds of the default training step (the option steps have them too, but for the query pooling's where the average
# pooling replaces it); "fcos_scale_raw": the Scale parameters' raw sums of the loss-gradient launch
DEFAULT_STEP_KINDS = ("pack_image", "conv1x1", "conv3x3", "conv7x1", "maxpool", "query_pool", "correlate", "gn_relu",
                      "fcos_loss_grad", "fcos_scale_raw", "gn_relu_bwd", "correlate_bwd_query", "query_pool_bwd", "wgrad", "add_mask",
                      "scatter2x", "upsample2x_bwd", "pred_gather", "pred_dgrad_pack")


def assert_kinds_occurred(rp, kinds):
    """these launch kinds were replayed at least once (Fp64Replayer: counted per (kind, algorithm) too)"""
    by_algo = getattr(rp, "by_algo", {})
    for kind in kinds:
        assert rp.counts.get(kind, 0) > 0 or any(k == kind for k, _ in by_algo), "no %s launch in the trace" % kind


def assert_gradients_covered(rp, eng):
    """every trainable tensor of the engine's plan — conv weights and biases, GroupNorm affines, and (a replayer built with
    engine=eng) the Scale parameters — has its gradient accounted for by the replayed launches: the accumulated tensors that lie in
    the flat gradient buffer add up to the plan's size."""
    flat_lo, flat_hi = eng.flat_g.data_ptr(), eng.flat_g.data_ptr() + eng.flat_g.numel() * 4
    covered = sum(ref.numel() for t, ref in rp.acc.values() if flat_lo <= t.data_ptr() < flat_hi)
    total = sum(int(np.prod(s)) for n_, s in eng._plan)
    assert covered == total, (covered, total)
