"""Same-box interleaved A/B of the training step: the shared-backbone model (siamese_backbone=False) against the two-backbone
model, both at bench.py's default workload (bs = 8, 800x1024 targets, 127x127 queries, bf16, first stage, train_step with the
join deferred as bench.py runs it).  bench.py has no switch for the mode; this builds both engines in ONE process, tunes each
once, then alternates blocks of timed steps between them.

    python tools/shared_backbone_ab.py [--rounds 6] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oneshotdet_amd import ops, spec, synth, train  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    B, H, W = args.batch, 800, 1024
    images = torch.from_numpy(synth.make_images("bench.target", B, H, W, seed=1000)).cuda()
    queries = torch.from_numpy(synth.make_images("bench.query", B, 127, 127, seed=1000)).cuda()
    gts = synth.make_gt_boxes(B, H, W, seed=1000, max_boxes=6)
    gtb = np.zeros((B, 6, 4), np.float32)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = g
    batch = (images, queries, torch.from_numpy(gtb).cuda(), torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda())
    engines = {}
    for label, siamese in (("two_backbones", True), ("shared", False)):
        eng = train.TrainEngine(synth.make_state_dict(spec.hot_path_shapes(siamese)), dtype=torch.bfloat16,
                                siamese_backbone=siamese)
        with ops.tuning():
            eng.forward_backward(*batch)
        torch.cuda.synchronize()
        eng.defer_join = True
        for _ in range(args.warmup):
            eng.train_step(*batch)
        eng.join()
        torch.cuda.synchronize()
        engines[label] = eng
    times = {k: [] for k in engines}
    for r in range(args.rounds):
        for label in (list(engines) if r % 2 == 0 else list(engines)[::-1]):
            eng = engines[label]
            for _ in range(2):
                eng.train_step(*batch)
            eng.join()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                eng.train_step(*batch)
            eng.join()
            t1.record()
            torch.cuda.synchronize()
            times[label].append(t0.elapsed_time(t1) / args.steps)
            print("round %d %-14s %.3f ms/step" % (r, label, times[label][-1]), flush=True)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"ms_per_step_median": med, "ms_per_step_all": times,
                      "shared_over_two_backbones": med["shared"] / med["two_backbones"], "batch": B, "rounds": args.rounds,
                      "steps_per_block": args.steps}))


if __name__ == "__main__":
    main()
