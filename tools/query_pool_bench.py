"""The query branch's pooling, both modes, forward + backward, bf16: the 1 x 1 ROIAlign + shot mean (supp_roialign=True, the
default: osd_query_pool_levels / _bwd) against the global average + shot mean (supp_roialign=False: osd_query_avgpool_levels / _bwd)
on three geometries — bs 8 with one 127 x 127 query each (bench.py's batch), bs 4 with five (BASELINE configs[4]), and bs 8 with
five 416 x 416 supports (real supports padded to /32: P3 is 52 x 52).  Per call: us (device events over back-to-back calls), and
for the average the bytes it must move (every map read once, every gradient map written once) over that time against the
device's measured copy rate.  --step: the bs = 8 bf16 first-stage train_step in avg mode against roialign mode, every measurement
in a fresh process of its own, the modes alternating.

    python tools/query_pool_bench.py [--reps 200] [--step] [--rounds 4] [--steps 50]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oneshotdet_amd import model, ops, spec, synth, train  # noqa: E402

SHAPES = [("bs8_S1_127", 8, 1, 127), ("bs4_S5_127", 4, 5, 127), ("bs8_S5_416", 8, 5, 416)]


def pyramid(q):
    """P3 - P7 sizes of a q x q query: stem conv and max-pool, layer2 - 4 (stride 2 in their first 1 x 1 conv), P6 / P7 (3 x 3,
    stride 2)"""
    s = ops.conv_out(ops.conv_out(q, 7, 2, 3), 3, 2, 1)
    out = []
    for _ in range(3):
        s = ops.conv_out(s, 1, 2, 0)
        out.append(s)
    for _ in range(2):
        s = ops.conv_out(s, 3, 2, 1)
        out.append(s)
    return out


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def copy_rate():
    x = torch.empty(256 << 20, dtype=torch.float32, device="cuda")     # 1 GiB: past the 256 MiB Infinity Cache
    y = torch.empty_like(x)
    us = timed(lambda: y.copy_(x), 20)
    return 2 * x.numel() * 4 / (us * 1e-6) / 1e9


def kernels(reps, gbs):
    dt, c = torch.bfloat16, spec.FPN_OUT
    rows = []
    for label, b, s, q in SHAPES:
        sizes = [(p, p) for p in pyramid(q)]
        g = torch.Generator().manual_seed(0)
        feats = [torch.randn(b * s, h, w, c, generator=g).to(dt).cuda() for h, w in sizes]
        dqs = [torch.randn(b, c, generator=g).cuda() for _ in sizes]
        shapes = [tuple(f.shape) for f in feats]
        rois = model.whole_image_rois([(q, q)] * (b * s), "cuda")
        roi_fwd = timed(lambda: ops.query_pool_levels(feats, rois, spec.POOLER_SCALES, b, spec.POOLER_SAMPLING_RATIO), reps)
        roi_bwd = timed(lambda: ops.query_pool_levels_bwd(dqs, rois, shapes, spec.POOLER_SCALES, s, spec.POOLER_SAMPLING_RATIO, dt), reps)
        avg_fwd = timed(lambda: ops.query_avgpool_levels(feats, b), reps)
        avg_bwd = timed(lambda: ops.query_avgpool_levels_bwd(dqs, shapes, s, dt), reps)
        nbytes = sum(f.numel() * f.element_size() for f in feats)         # read by the forward, written by the backward
        row = dict(shape=label, maps=sizes, MB=round(nbytes / 1e6, 2),
                   roialign_us=dict(fwd=round(roi_fwd, 1), bwd=round(roi_bwd, 1), total=round(roi_fwd + roi_bwd, 1)),
                   avg_us=dict(fwd=round(avg_fwd, 1), bwd=round(avg_bwd, 1), total=round(avg_fwd + avg_bwd, 1)),
                   avg_GBps=dict(fwd=round(nbytes / (avg_fwd * 1e-6) / 1e9, 1), bwd=round(nbytes / (avg_bwd * 1e-6) / 1e9, 1)),
                   avg_of_copy_rate=dict(fwd=round(nbytes / (avg_fwd * 1e-6) / 1e9 / gbs, 3),
                                         bwd=round(nbytes / (avg_bwd * 1e-6) / 1e9 / gbs, 3)))
        print("%-11s P3 %2dx%-2d %7.2f MB | roialign fwd %6.1f bwd %6.1f us | avg fwd %6.1f us (%5.0f GB/s) bwd %6.1f us (%5.0f GB/s)"
              % (label, sizes[0][0], sizes[0][1], nbytes / 1e6, roi_fwd, roi_bwd, avg_fwd, row["avg_GBps"]["fwd"], avg_bwd,
                 row["avg_GBps"]["bwd"]), flush=True)
        rows.append(row)
    return rows


def step_child(mode, steps, warmup):
    """one engine in a process of its own: tune, warm up, time `steps` train_steps (ms per step)"""
    B, H, W = 8, 800, 1024
    images = torch.from_numpy(synth.make_images("bench.target", B, H, W, seed=1000)).cuda()
    queries = torch.from_numpy(synth.make_images("bench.query", B, 127, 127, seed=1000)).cuda()
    gts = synth.make_gt_boxes(B, H, W, seed=1000, max_boxes=6)
    gtb = np.zeros((B, 6, 4), np.float32)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = g
    batch = (images, queries, torch.from_numpy(gtb).cuda(), torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda())
    eng = train.TrainEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=torch.bfloat16, supp_roialign=mode == "roialign")
    with ops.tuning():
        eng.forward_backward(*batch)
    torch.cuda.synchronize()
    eng.defer_join = True
    for _ in range(warmup):
        eng.train_step(*batch)
    eng.join()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        eng.train_step(*batch)
    eng.join()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"mode": mode, "ms_per_step": t0.elapsed_time(t1) / steps}))


def step_ab(rounds, steps, warmup):
    """Each measurement in a FRESH process, the two modes alternating: two engines built in one process are not comparable (the
    one built second measured 0.8 ms per step slower in either order, with 4 hardware queues for both engines' streams)."""
    import subprocess
    times = {"roialign": [], "avg": []}
    for r in range(rounds):
        for mode in (("roialign", "avg") if r % 2 == 0 else ("avg", "roialign")):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-child", mode, "--steps", str(steps),
                                  "--warmup", str(warmup)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError("step child (%s) failed with %d: %s" % (mode, out.returncode, out.stderr[-2000:]))
            ms = json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"]
            times[mode].append(ms)
            print("round %d %-9s %.3f ms/step" % (r, mode, ms), flush=True)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"ms_per_step_median": med, "ms_per_step_all": times, "avg_over_roialign": med["avg"] / med["roialign"],
            "batch": 8, "rounds": rounds, "steps_per_process": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-child", choices=["avg", "roialign"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step_child:
        return step_child(args.step_child, args.steps, args.warmup)
    gbs = copy_rate()
    print("device copy rate %.0f GB/s (1 GiB buffer, read + write)" % gbs, flush=True)
    out = {"copy_GBps": round(gbs, 1), "kernels": kernels(args.reps, gbs)}
    if args.step:
        out["step"] = step_ab(args.rounds, args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
