"""What the colour jitter of support crops (FEW_SHOT.NUM_SUPP_AUG = 3, transforms.color_jitter) costs: ONE call of osd_color_jitter_batch
for the jittered members of a bs-8, one-shot batch — 16 crops of 200 x 300, the jittered crop and the jittered flip of every support —
against what a user has to do for the same rows without it: the four PIL ImageEnhance steps on the host (data/datasets/coco.py:286-294)
and the upload of the results.  ONE process, the two alternating block by block (same box, same clocks).

    python tools/bench_color_jitter.py [--crops 16] [--height 200] [--width 300] [--blocks 10] [--iters 50] [--host-iters 5]

Device side, per block: `--iters` calls of transforms.color_jitter on crops that are already on the device (where DeviceImage.crop leaves
them), between two device events (device time per call, launch gaps included) and, separately, the host time to enqueue them; and
`--host-iters` calls that start from host arrays (upload of the sources included), a host clock around work that ends in a synchronise.
Host side, per block: `--host-iters` times the ImageEnhance chain on all crops plus the upload of the jittered images, the same clock.
Both produce the same bytes, which is checked once before anything is timed.  Prints one JSON line last.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oneshotdet_amd import ops, transforms as T  # noqa: E402


def pil_chain(arrays, factors):
    from PIL import Image, ImageEnhance
    out = []
    for a, f in zip(arrays, factors):
        im = Image.fromarray(a)
        for enh, v in zip((ImageEnhance.Color, ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Sharpness), f):
            im = enh(im).enhance(float(v))
        out.append(np.asarray(im))
    return out


def host_clock(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def device_events(fn, iters):
    """-> (device ms per call between two events, host ms per call to enqueue)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = (time.perf_counter() - t0) / iters * 1e3
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crops", type=int, default=16)
    ap.add_argument("--height", type=int, default=200)
    ap.add_argument("--width", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50, help="device-resident calls per block")
    ap.add_argument("--host-iters", type=int, default=5, help="calls per block of the two candidates that start from host arrays")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_color_jitter needs an MI355X: nothing is measured without one")
    ops._lib.load()
    rng = np.random.RandomState(0)
    arrays = [rng.randint(0, 256, (args.height, args.width, 3)).astype(np.uint8) for _ in range(args.crops)]
    factors = rng.uniform(0.1, 2, (args.crops, 4))
    resident = [T.DeviceImage(a) for a in arrays]
    want = pil_chain(arrays, factors)
    got = T.color_jitter(resident, factors)
    for w, g in zip(want, got):
        assert np.array_equal(w, g.src.cpu().numpy()), "the device jitter and PIL disagree"
    cands = {
        "device.resident": lambda: T.color_jitter(resident, factors),
        "device.from_host": lambda: T.color_jitter(arrays, factors),
        "host.pil_upload": lambda: [T.DeviceImage(o) for o in pil_chain(arrays, factors)],
    }
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in cands}
    enqueue = []
    for _ in range(args.blocks):
        dev, host = device_events(cands["device.resident"], args.iters)
        res["device.resident"].append(dev)
        enqueue.append(host)
        for k in ("device.from_host", "host.pil_upload"):
            res[k].append(host_clock(cands[k], args.host_iters))
    mb = args.crops * args.height * args.width * 3 / 1e6
    out = {"device": torch.cuda.get_device_name(0), "crops": args.crops, "height": args.height, "width": args.width, "image_megabytes": mb,
           "blocks": args.blocks, "iters_per_block": args.iters, "host_iters_per_block": args.host_iters,
           "device.resident.enqueue_ms": float(np.median(enqueue))}
    for k, v in res.items():
        a = np.asarray(v)
        out[k] = {"ms_median": float(np.median(a)), "ms_min": float(a.min()), "ms_max": float(a.max())}
        print("%-18s %.3f ms per call (blocks %.3f .. %.3f)" % (k, np.median(a), a.min(), a.max()))
    print("device.resident: host enqueue %.3f ms per call; %.2f MB of pixels in, as many out" % (out["device.resident.enqueue_ms"], mb))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
