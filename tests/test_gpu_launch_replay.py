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
  the Scale parameters' raw sums (fp32 atomics over the positives): 1e-4 x sum |terms|, as tests/test_gpu_fcos_loss_modes.py
and the chain's coverage is asserted: every conv, GroupNorm, correlation, pooling, loss-gradient and weight-gradient launch
of the step is replayed, and every trainable tensor's gradient — the Scale parameters' included — is accounted for by the
replayed launches.  The replayers themselves are tests/launch_replayer.py (shared with test_gpu_launch_replay_options.py)."""
import time

import pytest
import torch

import golden_utils as gu
from launch_replayer import DEFAULT_STEP_KINDS, Fp64Replayer, Replayer, _traced, assert_gradients_covered, assert_kinds_occurred
from oneshotdet_amd import spec, synth

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


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


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("name", ["small", "shots5", "nonsquare"])
def test_every_launch_of_a_training_step_matches_its_cpu_restatement(name, dt):
    """R0-R12 + backward (engine/trainer.py:79-93 up to the optimiser): forward, loss gradient, data gradients, GroupNorm /
    correlation / pooling backward and every weight gradient of one real training step, each launch from its own inputs."""
    eng, img, q, gtb, cnt = _train_engine(dt, name)
    eng.forward_backward(img, q, gtb, cnt, with_proposals=False)      # warm-up: allocations, persistent buffers
    torch.cuda.synchronize()
    _, trace = _traced(lambda: eng.forward_backward(img, q, gtb, cnt, with_proposals=False))
    rp = Replayer(engine=eng)
    rp.run(trace)
    worst_acc = rp.check_accumulated()
    print("\n%s %s: %d launches replayed: %s\n  worst per kind: %s\n  worst accumulated-gradient error %.2e of absmax over %d tensors"
          % (name, dt, len(trace), rp.counts, {k: {a: round(b, 4) for a, b in v.items()} for k, v in rp.worst.items()}, worst_acc,
             len(rp.acc)))
    assert not rp.failures, rp.failures[:6]
    # coverage: the step's launch kinds are all there ...
    assert_kinds_occurred(rp, DEFAULT_STEP_KINDS)
    # ... and every trainable conv weight / bias / GroupNorm affine / Scale gradient was produced by replayed launches
    assert_gradients_covered(rp, eng)


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
    rp = Replayer(engine=eng)
    rp.run(trace)
    worst_acc = rp.check_accumulated()
    print("\nconfig1 bf16: %d launches: %s\n  worst per kind: %s\n  worst accumulated-gradient error %.2e"
          % (len(trace), rp.counts, rp.worst, worst_acc))
    assert not rp.failures, rp.failures[:6]


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
    rp = Fp64Replayer(engine=eng)
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
    assert_kinds_occurred(rp, ("conv1x1", "conv3x3", "conv7x1", "wgrad", "gn_relu", "gn_relu_bwd", "fcos_loss_grad", "fcos_scale_raw"))
    assert_gradients_covered(rp, eng)
