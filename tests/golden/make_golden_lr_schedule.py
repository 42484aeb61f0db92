"""Generate tests/golden/lr_schedule.npz from the REAL reference (build container only).

    python tests/golden/make_golden_lr_schedule.py

The reference's solver/lr_scheduler.py is loaded from its file (it imports nothing but bisect and torch) and a real WarmupMultiStepLR
is driven the way engine/trainer.py:93-96 drives it — optimizer.step(), then scheduler.step() — on a torch.optim.SGD with the two
parameter groups of solver/build.py:8-26 (weights at BASE_LR, biases at BASE_LR * BIAS_LR_FACTOR).  Before update k the rates of
both groups are read from optimizer.param_groups, as float64: they are the Python floats the reference's optimiser would use.

Per case <name>:  <name>.k [n] int64 (the sampled update indices), <name>.lr [n][2] float64 (weight group, bias group), and the
schedule's arguments <name>.base_lr, .milestones, .gamma, .warmup_factor, .warmup_iters, .warmup_method.
  record        configs/fcos/2019_10_25_vanilla_siamse_backbone.yaml:50-58 over config/defaults.py; k = 0, 99, 100, 59 999, 60 000,
                89 999, 90 000, 119 999, 120 000, 129 999
  defaults      config/defaults.py's SOLVER.* (linear warmup over 500 iterations, milestone 30 000); every k < 520, then 29 999, 30 000, 39 999
  inside        milestones (3, 7) with warmup_iters 10, linear: both milestones fall inside the warmup; every k < 16
  half          gamma 0.5, milestones (2, 4, 6), constant warmup over 3; every k < 10
  nomilestones  no milestones, linear warmup over 5; every k < 10
  zero          gamma 0.0, milestone (2,), no warmup (warmup_iters 0); every k < 6
  engine        linear warmup over 2 iterations, milestone (3,), gamma 0.1: the engine tests' schedule (tests/test_gpu_solver.py); every k < 8
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh      # noqa: E402

OUT = os.path.join(HERE, "lr_schedule.npz")
BIAS_LR_FACTOR = 2            # config/defaults.py:434
THIRD = 1.0 / 3               # config/defaults.py:444, as written there
CASES = {
    # name: (base_lr, milestones, gamma, warmup_factor, warmup_iters, warmup_method, sampled k)
    "record": (0.0005, (60000, 90000, 120000), 0.1, THIRD, 100, "constant",
               (0, 99, 100, 59999, 60000, 89999, 90000, 119999, 120000, 129999)),
    "defaults": (0.001, (30000,), 0.1, THIRD, 500, "linear", tuple(range(520)) + (29999, 30000, 39999)),
    "inside": (0.002, (3, 7), 0.1, THIRD, 10, "linear", tuple(range(16))),
    "half": (0.01, (2, 4, 6), 0.5, THIRD, 3, "constant", tuple(range(10))),
    "nomilestones": (0.001, (), 0.1, 0.25, 5, "linear", tuple(range(10))),
    "zero": (0.002, (2,), 0.0, THIRD, 0, "linear", tuple(range(6))),
    "engine": (0.002, (3,), 0.1, THIRD, 2, "linear", tuple(range(8))),
}


def reference_scheduler_class():
    path = os.path.join(rh.REFERENCE_ROOT, "maskrcnn_benchmark", "solver", "lr_scheduler.py")
    spec = importlib.util.spec_from_file_location("reference_lr_scheduler", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.WarmupMultiStepLR


def drive(cls, base_lr, milestones, gamma, warmup_factor, warmup_iters, warmup_method, ks):
    w, b = torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([{"params": [w], "lr": base_lr}, {"params": [b], "lr": base_lr * BIAS_LR_FACTOR}], base_lr, momentum=0.9)
    sched = cls(opt, milestones, gamma, warmup_factor=warmup_factor, warmup_iters=warmup_iters, warmup_method=warmup_method)
    want, out = set(ks), {}
    w.grad, b.grad = torch.zeros(1), torch.zeros(1)
    for k in range(max(ks) + 1):
        if k in want:
            out[k] = [float(g["lr"]) for g in opt.param_groups]
        opt.step()
        sched.step()
    return np.array([out[k] for k in ks], dtype=np.float64)


def main():
    if not rh.reference_available():
        raise RuntimeError("the reference is not present at %s" % rh.REFERENCE_ROOT)
    cls = reference_scheduler_class()
    data = {}
    for name, (base_lr, milestones, gamma, wf, wi, wm, ks) in CASES.items():
        data[name + ".k"] = np.array(ks, dtype=np.int64)
        data[name + ".lr"] = drive(cls, base_lr, milestones, gamma, wf, wi, wm, ks)
        data[name + ".base_lr"] = np.float64(base_lr)
        data[name + ".milestones"] = np.array(milestones, dtype=np.int64)
        data[name + ".gamma"] = np.float64(gamma)
        data[name + ".warmup_factor"] = np.float64(wf)
        data[name + ".warmup_iters"] = np.int64(wi)
        data[name + ".warmup_method"] = np.array(wm)
        print(name, data[name + ".lr"][:3].tolist(), "...", data[name + ".lr"][-1].tolist())
    np.savez_compressed(OUT, **data)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
