"""GPU box: the backward pass of a prediction conv (cout 2 and 4, cin 256) over the benchmark's five FPN levels at bs = 8: the fused
launch (osd_conv2d_pred_bwd) + its reduce, its two halves, and the gathered sequence it replaces (osd_pred_dy_gather + fill +
osd_conv2d_wgrad_pred_gathered + the K = 64 conv over G), every call on preallocated buffers.  Warm: 20 launches back to back;
cold: one launch behind a 512 MB eviction pass (as tuner._time_launches_cold).  Each figure is the median [min .. max] of --reps
timings, in microseconds; the TB/s are the algorithmic bytes (x read once + dX written once + dy + Wd) over the median.
python tools/pred_bwd_bench.py [--reps 7] [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from oneshotdet_amd import _lib, ops  # noqa: E402

LEVELS = [(8, 100, 128), (8, 50, 64), (8, 25, 32), (8, 13, 16), (8, 7, 8)]
CIN = 256


def timed(fn, reps, warm, flush):
    out = []
    for _ in range(reps):
        n = 20 if warm else 1
        if not warm:
            flush.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / n)
    return dict(median=statistics.median(out), min=min(out), max=max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    flush = torch.zeros(128 * 1024 * 1024, device="cuda")
    lib = _lib.load()
    rows = []
    for cout in (2, 4):
        xs = [torch.randn(n, h, w, CIN, device="cuda", generator=gen).bfloat16() for n, h, w in LEVELS]
        dys = [(torch.randn(n, h, w, 4, device="cuda", generator=gen) * 0.1).bfloat16() for n, h, w in LEVELS]
        for d in dys:
            d[..., cout:] = 0
        k = len(xs)
        tot = sum(n * h * w for n, h, w in LEVELS)
        master = torch.randn(cout, 3, 3, CIN, device="cuda", generator=gen) / 48
        wd = ops.pred_dgrad_pack(master, cout, CIN, torch.bfloat16)
        ent = ops.PackedConv(wd, torch.zeros(CIN, device="cuda"), CIN, CIN, CIN, ops.PRED_G, 1, 1, cin_real=9 * cout)
        dw, db = torch.zeros(cout, 3, 3, CIN, device="cuda"), torch.zeros(cout, device="cuda")
        d = ops._conv_desc(xs[0].shape, ops.OSD_BF16, cout, 3, 3, 1, 1, 4)
        xp = (C.c_void_p * k)(*[t.data_ptr() for t in xs])
        dyp = (C.c_void_p * k)(*[t.data_ptr() for t in dys])
        ns, hs, ws = ((C.c_int32 * k)(*[lv[i] for lv in LEVELS]) for i in range(3))
        st = ops._stream()
        need = int(lib.osd_pred_bwd_workspace_bytes(k, ns, hs, ws, CIN, cout))
        wsp = torch.empty((need // 4 + 1,), device="cuda")
        dx = torch.empty((tot, CIN), device="cuda", dtype=torch.bfloat16)

        def fused(flags):
            return lambda: _lib.call("osd_conv2d_pred_bwd", C.byref(d), k, xp, dyp, ns, hs, ws, wd.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                     db.data_ptr(), wsp.data_ptr(), flags, st)
        g = torch.empty((tot, ops.PRED_G), device="cuda", dtype=torch.bfloat16)
        wsp_old = torch.empty((64 + ops.PRED_G * CIN + 64,), device="cuda")
        dx_old = torch.empty((1, 1, tot, CIN), device="cuda", dtype=torch.bfloat16)
        g4 = g.view(1, 1, tot, ops.PRED_G)

        def gather():
            _lib.call("osd_pred_dy_gather", C.byref(d), k, dyp, ns, hs, ws, g.data_ptr(), st)

        def wgrad_old():
            _lib.call("osd_conv2d_wgrad_pred_gathered", C.byref(d), k, xp, g.data_ptr(), ns, hs, ws, dw.data_ptr(), db.data_ptr(),
                      wsp_old.data_ptr(), st)

        def dgrad_old():
            ops.conv2d(g4, ent, out=dx_old)

        def old():
            gather()
            wgrad_old()
            dgrad_old()
        parts = [("fused + reduce", fused(_lib.PRED_BWD_BOTH)), ("data-gradient half", fused(_lib.PRED_BWD_DGRAD)),
                 ("weight-gradient half + reduce", fused(_lib.PRED_BWD_WGRAD)), ("gathered sequence", old), ("  gather", gather),
                 ("  fill + wgrad over G + scatter", wgrad_old), ("  K = 64 conv over G", dgrad_old)]
        for _, fn in parts:
            fn()
        torch.cuda.synchronize()
        mb = (2 * tot * CIN * 2 + tot * 4 * 2 + CIN * 64 * 2) / 1e6
        for name, fn in parts:
            for mode in ("warm", "cold"):
                t = timed(fn, a.reps, mode == "warm", flush)
                row = dict(cout=cout, what=name.strip(), mode=mode, us=t)
                if name == "fused + reduce":
                    row["algorithmic_MB"], row["TBps"] = round(mb, 1), round(mb / t["median"], 2)
                rows.append(row)
                print("cout %d  %-34s %s  %7.1f us  [%.1f .. %.1f]%s" % (cout, name, mode, t["median"], t["min"], t["max"],
                      "   %.0f MB -> %.2f TB/s" % (mb, mb / t["median"]) if "TBps" in row else ""), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
