"""What the query gallery (enroll the supports once, detect(images, bank=bank)) buys over the class sweep, which runs the query
branch on B*K*S patches in every call: bf16, 800x1024 targets, 127x127 queries, K = G = 20 (every image is asked about every slot of
the gallery, the reference's fixed-support evaluation), second stage on, after `tune`, interleaved in ONE process (same box, same
clocks, same tuner cache):

    (a) sweep   detect(images, queries, classes=K)       B*K supports through the query backbone, pooling and query-half conv
    (b) bank    detect(images, bank=bank)                 no query launch at all
    (c) enroll  enroll(supports) alone                     what (b) paid once, on G supports

    python tools/bench_query_bank.py [--batches 1,4,8] [--classes 20] [--iters 20] [--warmup 3] [--commit ID] [--out FILE]

Every iteration times (a), (b) and (c) one after the other between device events of their own; reported is the median over the
iterations after warm-up, with the smallest and the largest.  The two new kernels are timed alone as well, `--reps` back-to-back
launches between two events, each against what it replaces: the gallery correlation against the sweep correlation on pre-gathered
vectors (and with the five index_select launches that gather them); the gallery GroupNorm against index_select of the query halves
plus the existing entry (and the existing entry alone on a pre-gathered addend), on the batch's own number of proposals.  Prints the
table as markdown (--out FILE: writes it there too; profiles/query_bank.md is such a table with its reading added by hand) and one JSON
line last.
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
    images = torch.from_numpy(synth.make_images("bank.target", B, H, W, seed=1000)).cuda()
    gallery = torch.from_numpy(synth.make_images("bank.query", K, 127, 127, seed=1000)).cuda()          # G = K slots, one shot each
    queries = gallery.repeat(B, 1, 1, 1).contiguous()                                                      # row b*K + k = slot k
    bank = eng.enroll(gallery)
    eng.tune(images, queries, second_stage=True, classes=K)
    eng.tune(images, second_stage=True, bank=bank)
    with ops.tuning():
        eng.enroll(gallery)
    torch.cuda.synchronize()
    bank = eng.enroll(gallery)                               # with the tuned algorithms, as (c) runs it
    ways = (("sweep", lambda: eng.detect(images, queries, classes=K, second_stage=True)),
            ("bank", lambda: eng.detect(images, bank=bank, second_stage=True)),
            ("enroll", lambda: eng.enroll(gallery)))
    times = {name: [] for name, _ in ways}
    for it in range(warmup + iters):
        evs = [(name, timed(fn)) for name, fn in ways]
        torch.cuda.synchronize()
        if it >= warmup:
            for name, (a, b) in evs:
                times[name].append(a.elapsed_time(b))
    res = {name: med(ts) for name, ts in times.items()}
    # the two kernels alone, on this batch's own features and number of proposals
    out = eng.detect(images, bank=bank, second_stage=True)
    feats = out["features"]
    r = out["proposals"][0].shape[1]
    table = eng.slot_table(bank, B, None, True)
    idx = table.dev.long()
    pre_pooled = [p.index_select(0, idx) for p in bank.pooled]
    pre_half = bank.q_half.index_select(0, idx)
    g0, b0 = eng.box_head.gn[0]
    u0 = torch.randn((B * K * r,) + tuple(bank.q_half.shape[1:]), device="cuda").to(bank.q_half.dtype)
    y = torch.empty_like(u0)
    gn = lambda **kw: ops.groupnorm_act_rois(u0, g0, b0, spec.GN_GROUPS, spec.GN_EPS, spec.BOX_LEAKY_SLOPE, rois_per_add=r, out=y, **kw)  # noqa: E731
    kernels = (("correlate_gallery", lambda: ops.correlate_levels_gallery(feats, bank.pooled, table.dev, K)),
               ("correlate_sweep_pregathered", lambda: ops.correlate_levels_sweep(feats, pre_pooled, K)),
               ("correlate_gather_sweep", lambda: ops.correlate_levels_sweep(feats, [p.index_select(0, idx) for p in bank.pooled], K)),
               ("groupnorm_gallery", lambda: gn(addend=bank.q_half, add_index=table.dev)),
               ("groupnorm_gather_existing", lambda: gn(addend=bank.q_half.index_select(0, idx))),
               ("groupnorm_existing_pregathered", lambda: gn(addend=pre_half)))
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
    res["proposals_per_row"] = int(r)
    res["groupnorm_bytes"] = int(2 * u0.numel() * u0.element_size())
    res["map_bytes"] = int(sum(f.numel() * f.element_size() for f in feats))
    del out, u0, y
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,8")
    ap.add_argument("--classes", type=int, default=20, help="K = G: slots of the gallery, all asked of every image")
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
    K = args.classes
    eng = model.HotPathEngine(synth.make_state_dict(spec.full_model_shapes()),
                              dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    result = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "classes": K, "dtype": args.dtype,
              "height": args.height, "width": args.width, "iters": args.iters, "warmup": args.warmup, "reps": args.reps, "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        result["batches"][B] = r = bench_batch(eng, B, K, args.height, args.width, args.iters, args.warmup, args.reps)
        print("bs %d: sweep %.2f ms, bank %.2f ms, enroll %.2f ms; correlation gallery %.3f ms vs sweep on pre-gathered vectors %.3f ms "
              "(gather + sweep %.3f ms); GroupNorm gallery %.3f ms vs index_select + existing %.3f ms (existing alone %.3f ms)"
              % (B, r["sweep"]["median_ms"], r["bank"]["median_ms"], r["enroll"]["median_ms"], r["correlate_gallery"]["median_ms"],
                 r["correlate_sweep_pregathered"]["median_ms"], r["correlate_gather_sweep"]["median_ms"],
                 r["groupnorm_gallery"]["median_ms"], r["groupnorm_gather_existing"]["median_ms"],
                 r["groupnorm_existing_pregathered"]["median_ms"]), flush=True)
    lines = ["# Query gallery: detect(images, bank=bank) against the class sweep", "",
             "`python tools/bench_query_bank.py` on %s, commit %s: %s, %d x %d targets, 127 x 127 queries, K = G = %d slots (every image "
             "asked about every slot), one shot, second stage on, after `tune`.  Median of %d iterations after %d of warm-up (smallest .. "
             "largest), every iteration timing the three ways one after the other between device events of their own, in one process."
             % (result["device"], args.commit or "(not given)", args.dtype, args.height, args.width, K, args.iters, args.warmup), "",
             "(a) sweep = `detect(images, queries, classes=K)`; (b) bank = `detect(images, bank=bank)`; (c) enroll = `enroll(supports)` "
             "alone, paid once per gallery.", "",
             "| bs | (a) sweep ms | (b) bank ms | (c) enroll ms | (a)/(b) | (a) - (b) ms | image-categories/s (b) |", "|---|---|---|---|---|---|---|"]
    fmt = lambda m: "%.2f (%.2f .. %.2f)" % (m["median_ms"], m["min_ms"], m["max_ms"])      # noqa: E731
    for B, r in result["batches"].items():
        a, b = r["sweep"]["median_ms"], r["bank"]["median_ms"]
        lines.append("| %d | %s | %s | %s | %.2f | %.2f | %.0f |" % (B, fmt(r["sweep"]), fmt(r["bank"]), fmt(r["enroll"]), a / b, a - b,
                                                                   B * K / b * 1e3))
    lines += ["", "The two new kernels alone (%d back-to-back launches per timed window, per launch), each against the entry it replaces "
              "plus its gather:" % args.reps, "",
              "| bs | gallery correlation ms | sweep correlation, pre-gathered vectors ms | 5 index_select + sweep correlation ms | gallery GroupNorm "
              "ms | index_select + existing GroupNorm ms | existing GroupNorm, pre-gathered addend ms | proposals per row |",
              "|---|---|---|---|---|---|---|---|"]
    kf = lambda m: "%.3f (%.3f .. %.3f)" % (m["median_ms"], m["min_ms"], m["max_ms"])       # noqa: E731
    for B, r in result["batches"].items():
        lines.append("| %d | %s | %s | %s | %s | %s | %s | %d |" % (
            B, kf(r["correlate_gallery"]), kf(r["correlate_sweep_pregathered"]), kf(r["correlate_gather_sweep"]), kf(r["groupnorm_gallery"]),
            kf(r["groupnorm_gather_existing"]), kf(r["groupnorm_existing_pregathered"]), r["proposals_per_row"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
