"""What FEW_SHOT.NEG_SUPPORT costs per training step: the bs-8 800x1024 / 127x127 bf16 step with second_stage=True, with
neg_support off and on, two engines alternating in ONE process (same box, same clocks, same tuner cache).

    python tools/bench_neg_support.py [--batch 8] [--blocks 10] [--steps 30] [--warmup 10] [--dtype bf16]

Every block is `--steps` train_steps of one engine between two device synchronisations, timed on the host; the engines take turns
block by block, so drift hits both alike.  Reported: the mean step time of every engine over its blocks, the spread (min / max / standard
deviation of the block means), the difference, and the launch counts of one step by kind (oneshotdet_amd.trace).  The learning rate is
0: the step does all its work (update and repack included) and the model stays what it was — the step time of a model trained for
hundreds of steps on one synthetic batch drifts with its proposals, which would be measured instead of the option.
The negative supports are the positive queries rotated by one image (the rule of examples/train.py).  Prints one JSON line last.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oneshotdet_amd import ops, spec, synth, trace, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=10, help="timed blocks per engine")
    ap.add_argument("--steps", type=int, default=30, help="steps per block")
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps per engine after tuning")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1024)
    args = ap.parse_args()
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    B, H, W = args.batch, args.height, args.width
    sd = synth.make_state_dict(spec.full_model_shapes())
    images = torch.from_numpy(synth.make_images("bench.target", B, H, W, seed=1000)).cuda()
    queries = torch.from_numpy(synth.make_images("bench.query", B, 127, 127, seed=1000)).cuda()
    neg_queries = torch.roll(queries, -1, 0).contiguous()
    gts = synth.make_gt_boxes(B, H, W, seed=1000, max_boxes=6)
    gtb = np.zeros((B, 6, 4), np.float32)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = g
    gtb, cnt = torch.from_numpy(gtb).cuda(), torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda()
    engines = {}
    for name, on in (("off", False), ("on", True)):
        eng = train.TrainEngine(sd, dtype=dtype, lr=0.0, second_stage=True, neg_support=on)
        kw = dict(neg_queries=neg_queries) if on else {}
        with ops.tuning():                      # every conv shape met for the first time is timed over its candidates, untimed here
            eng.forward_backward(images, queries, gtb, cnt, **kw)
        torch.cuda.synchronize()
        eng.defer_join = True
        engines[name] = (eng, kw)
    launches = {}
    for name, (eng, kw) in engines.items():
        for _ in range(args.warmup):
            eng.train_step(images, queries, gtb, cnt, **kw)
        eng.join()
        torch.cuda.synchronize()
        trace.TRACE = []
        try:
            eng.train_step(images, queries, gtb, cnt, **kw)
            eng.join()
            torch.cuda.synchronize()
            kinds = [k for k, _ in trace.TRACE]
        finally:
            trace.TRACE = None
        launches[name] = {k: kinds.count(k) for k in sorted(set(kinds))}
    times = {name: [] for name in engines}
    for _ in range(args.blocks):
        for name, (eng, kw) in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                eng.train_step(images, queries, gtb, cnt, **kw)
            eng.join()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    out = {"batch": B, "height": H, "width": W, "dtype": args.dtype, "blocks": args.blocks, "steps_per_block": args.steps,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        a = np.asarray(ts)
        out[name] = {"step_ms_mean": float(a.mean()), "step_ms_min": float(a.min()), "step_ms_max": float(a.max()),
                     "step_ms_std": float(a.std()), "images_per_s": float(B / a.mean() * 1e3), "timed_steps": args.blocks * args.steps}
        print("neg_support %-3s: %.3f ms per step (blocks: min %.3f, max %.3f, std %.3f; %d timed steps), %.1f images/s"
              % (name, a.mean(), a.min(), a.max(), a.std(), args.blocks * args.steps, B / a.mean() * 1e3))
    d = out["on"]["step_ms_mean"] - out["off"]["step_ms_mean"]
    out["increase_ms"], out["increase_percent"] = d, 100.0 * d / out["off"]["step_ms_mean"]
    print("increase: %.3f ms per step (%.1f %%)" % (d, out["increase_percent"]))
    diff = {k: (launches["off"].get(k, 0), launches["on"].get(k, 0)) for k in sorted(set(launches["off"]) | set(launches["on"]))
            if launches["off"].get(k, 0) != launches["on"].get(k, 0)}
    out["traced_launches"] = {"off": sum(launches["off"].values()), "on": sum(launches["on"].values()), "differ (off, on)": diff}
    print("traced launches per step: off %d, on %d; kinds that differ (off, on): %s"
          % (out["traced_launches"]["off"], out["traced_launches"]["on"], diff))
    eng_on = engines["on"][0]
    out["loss_cls_suppress"], out["foreground_rows"] = float(eng_on.box_suppress_loss[0]), int(eng_on.box_suppress_loss[1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
