"""What the class sweep (detect(..., classes=K): K category slots per target image in one pass) buys: bf16, 800x1024 targets,
127x127 queries, K = 20, second stage on, after `tune`, three ways of asking every image of a batch about K categories, interleaved
in ONE process (same box, same clocks, same tuner cache):

    (a) loop       K detect calls on the same images, one category each (all there was before the sweep)
    (b) replicated ONE per-pair detect on the K times replicated batch (B*K images through both backbones)
    (c) sweep      detect(images, queries, classes=K)

    python tools/bench_class_sweep.py [--batches 1,4,8] [--classes 20] [--iters 20] [--warmup 3] [--commit ID] [--out FILE]

Every iteration times (a), (b) and (c) one after the other between device events of their own; reported is the median over the
iterations after warm-up, with the smallest and the largest.  The two new kernels are timed alone as well, `--reps` back-to-back
launches between two events: the sweep correlation against the K osd_correlate_levels launches it replaces and against one launch on
replicated maps, as a share of 8 TB/s under its traffic model of (ceil(K/G) + K) maps (2K for the per-pair launches); the sweep ROI
pooling against the per-pair entry on replicated maps, on the proposals of the batch.  Prints the table as markdown (--out FILE: writes
it there too; profiles/class_sweep.md is such a table with its reading added by hand) and one JSON line last.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oneshotdet_amd import model, ops, spec, synth  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def med(ts):
    a = np.asarray(ts)
    return dict(median_ms=float(np.median(a)), min_ms=float(a.min()), max_ms=float(a.max()), n=int(a.size))


def bench_batch(eng, B, K, H, W, iters, warmup, reps):
    images = torch.from_numpy(synth.make_images("sweep.target", B, H, W, seed=1000)).cuda()
    queries = torch.from_numpy(synth.make_images("sweep.query", B * K, 127, 127, seed=1000)).cuda()      # row b*K + k
    per_slot = [queries[k::K].contiguous() for k in range(K)]
    rep = images.repeat_interleave(K, 0)
    eng.tune(images, per_slot[0], second_stage=True)
    eng.tune(rep, queries, second_stage=True)
    eng.tune(images, queries, second_stage=True, classes=K)

    def loop():
        for k in range(K):
            eng.detect(images, per_slot[k], second_stage=True)
    ways = (("loop", loop),
            ("replicated", lambda: eng.detect(rep, queries, second_stage=True)),
            ("sweep", lambda: eng.detect(images, queries, classes=K, second_stage=True)))
    times = {name: [] for name, _ in ways}
    for it in range(warmup + iters):
        evs = [(name, timed(fn)) for name, fn in ways]
        torch.cuda.synchronize()
        if it >= warmup:
            for name, (a, b) in evs:
                times[name].append(a.elapsed_time(b))
    res = {name: med(ts) for name, ts in times.items()}
    # the two kernels alone, on this batch's own features and proposals
    out = eng.detect(images, queries, classes=K, second_stage=True)
    feats, pooled = out["features"], out["pooled"]
    boxes, counts = out["proposals"][0], out["proposals"][2]
    rep_feats = [f.repeat_interleave(K, 0) for f in feats]
    slot_pooled = [[p[k::K].contiguous() for p in pooled] for k in range(K)]
    pool = lambda fs, **kw: ops.roi_pool_levels(fs, spec.POOLER_SCALES, boxes, counts, spec.BOX_POOL, spec.POOLER_SAMPLING_RATIO, **kw)  # noqa: E731

    def k_launches():
        for k in range(K):
            ops.correlate_levels(feats, slot_pooled[k])
    kernels = (("correlate_sweep", lambda: ops.correlate_levels_sweep(feats, pooled, K)),
               ("correlate_k_launches", k_launches),
               ("correlate_replicated", lambda: ops.correlate_levels(rep_feats, pooled)),
               ("roi_pool_sweep", lambda: pool(feats, sets_per_image=K)),
               ("roi_pool_replicated", lambda: pool(rep_feats)))
    ktimes = {name: [] for name, _ in kernels}
    for it in range(warmup + iters):
        evs = []
        for name, fn in kernels:
            def many(fn=fn):
                for _ in range(reps):
                    fn()
            evs.append((name, timed(many)))
        torch.cuda.synchronize()
        if it >= warmup:
            for name, (a, b) in evs:
                ktimes[name].append(a.elapsed_time(b) / reps)
    res.update({name: med(ts) for name, ts in ktimes.items()})
    G = ops.class_sweep_group()
    map_bytes = sum(f.numel() * f.element_size() for f in feats)          # one pyramid of the whole batch
    res["map_bytes"] = int(map_bytes)
    res["sweep_model_bytes"] = int(((K + G - 1) // G + K) * map_bytes)
    res["pair_model_bytes"] = int(2 * K * map_bytes)
    for name, key in (("correlate_sweep", "sweep_model_bytes"), ("correlate_k_launches", "pair_model_bytes"),
                      ("correlate_replicated", "pair_model_bytes")):
        res[name]["share_of_8TBps"] = res[key] / (res[name]["median_ms"] * 1e-3) / HBM_BYTES_PER_S
    res["proposals_per_row"] = float(counts.float().mean())
    del out, rep_feats
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20, help="timed iterations (the median is reported)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="back-to-back launches per timed window of the kernels alone")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--commit", default="", help="the commit measured (a snapshot without .git cannot tell)")
    ap.add_argument("--out", default="", help="also write the markdown table to this file")
    args = ap.parse_args()
    if args.iters < 20:
        print("note: fewer than 20 timed iterations: a rehearsal, not a measurement")
    K, G = args.classes, ops.class_sweep_group()
    eng = model.HotPathEngine(synth.make_state_dict(spec.full_model_shapes()),
                              dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    result = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "classes": K, "group": G, "dtype": args.dtype,
              "height": args.height, "width": args.width, "iters": args.iters, "warmup": args.warmup, "reps": args.reps, "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        result["batches"][B] = r = bench_batch(eng, B, K, args.height, args.width, args.iters, args.warmup, args.reps)
        print("bs %d: loop %.2f ms, replicated %.2f ms, sweep %.2f ms; correlation sweep %.3f ms vs %d launches %.3f ms; ROI pooling sweep "
              "%.3f ms vs replicated %.3f ms" % (B, r["loop"]["median_ms"], r["replicated"]["median_ms"], r["sweep"]["median_ms"],
                                                 r["correlate_sweep"]["median_ms"], K, r["correlate_k_launches"]["median_ms"],
                                                 r["roi_pool_sweep"]["median_ms"], r["roi_pool_replicated"]["median_ms"]), flush=True)
    lines = ["# Class sweep: classes=K against K per-pair calls", "",
             "`python tools/bench_class_sweep.py` on %s, commit %s: %s, %d x %d targets, 127 x 127 queries, K = %d category slots per "
             "image, second stage on, after `tune`; G = %d query vectors per workgroup of `osd_correlate_levels_sweep`.  Median of %d "
             "iterations after %d of warm-up (smallest .. largest), every iteration timing the three ways one after the other between "
             "device events of their own, in one process."
             % (result["device"], args.commit or "(not given)", args.dtype, args.height, args.width, K, G, args.iters, args.warmup), "",
             "(a) loop = K `detect` calls on the same images; (b) replicated = one per-pair `detect` on the K times replicated batch; "
             "(c) sweep = `detect(images, queries, classes=K)`.", "",
             "| bs | (a) loop ms | (b) replicated ms | (c) sweep ms | (a)/(c) | (b)/(c) | image-categories/s (c) |", "|---|---|---|---|---|---|---|"]
    fmt = lambda m: "%.2f (%.2f .. %.2f)" % (m["median_ms"], m["min_ms"], m["max_ms"])      # noqa: E731
    for B, r in result["batches"].items():
        c = r["sweep"]["median_ms"]
        lines.append("| %d | %s | %s | %s | %.2f | %.2f | %.0f |" % (B, fmt(r["loop"]), fmt(r["replicated"]), fmt(r["sweep"]),
                                                                   r["loop"]["median_ms"] / c, r["replicated"]["median_ms"] / c, B * K / c * 1e3))
    lines += ["", "The two new kernels alone (%d back-to-back launches per timed window, per launch; share of 8 TB/s under the traffic "
              "model: (ceil(K/G) + K) pyramids for the sweep, 2K for the per-pair launches):" % args.reps, "",
              "| bs | pyramid MB | sweep correlation ms (share) | K correlate_levels launches ms (share) | one launch on replicated maps ms (share) "
              "| sweep ROI pooling ms | ROI pooling on replicated maps ms | proposals per row |", "|---|---|---|---|---|---|---|---|"]
    kf = lambda m: "%.3f (%.0f %%)" % (m["median_ms"], 100 * m["share_of_8TBps"])           # noqa: E731
    for B, r in result["batches"].items():
        lines.append("| %d | %.1f | %s | %s | %s | %.3f | %.3f | %.0f |" % (
            B, r["map_bytes"] / 1e6, kf(r["correlate_sweep"]), kf(r["correlate_k_launches"]), kf(r["correlate_replicated"]),
            r["roi_pool_sweep"]["median_ms"], r["roi_pool_replicated"]["median_ms"], r["proposals_per_row"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
