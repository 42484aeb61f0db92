"""GPU: osd_solver_set and the `_dev` update entries — the optimiser update with its learning rate in device memory — and the learning-rate
schedule through the training engine (TrainEngine(lr_schedule=), capture / replay_step, checkpoints).

Kernel tests: the small entry tables of tests/test_gpu_support_kernels.py (SGD_ENTRIES: every path of the update kernels — offsets
off a 16-byte boundary, tails, more workgroups than work, packed conv entries whose group of four cannot go out as one store), built
into device tables by tests/support_ref.py (sgd_table, sgd_pack_table), three steps with a DIFFERENT rate each and first_step = 1, 0, 0
over a momentum buffer pre-filled with 5.0.  Bars: `torch.equal` between the `_dev` entries and the by-value entries called with the
same rates (they run one update body); sr.SGD_ATOL / sr.SGD_RTOL against the float64 restatement with per-step rates.

Engine tests: fp32, B = 2, 128 x 160 targets and 63 x 63 queries (the shapes of tests/test_gpu_train.py's capture test) and that
test's bounds for graph against eager: losses rtol 2e-3 / atol 1e-6, weights relative L2 < 1e-4; for a resumed run the bounds of
test_optimizer_state_survives_a_checkpoint, rtol 1e-4 / atol 1e-6.  The rates the engine must use are the reference's own
(tests/golden/lr_schedule.npz, cases `zero` and `engine`)."""
import functools
import os

import numpy as np
import pytest
import torch

import support_ref as sr
import test_gpu_support_kernels as sk
from oneshotdet_amd import ops, spec, synth
from oneshotdet_amd.solver import LRSchedule

pytestmark = pytest.mark.gpu

call, P, ST, DT, DTC, SENT = sk.call, sk.P, sk.ST, sk.DT, sk.DTC, sk.SENT
RATES = (0.05, 0.0125, 0.2)          # a different rate each step (C floats on both routes)
MOM = sk.SGD_MOM
INVALID_ARG = -1                     # OSD_ERR_INVALID_ARG


def new_block():
    """The 8-byte solver block between two sentinels: int64[3], the block is element 1."""
    t = torch.full((3,), 0x7A7A7A7A7A7A7A7A, dtype=torch.int64, device="cuda")
    return t, t[1:2]


def block_words(t):
    return t.cpu().view(torch.int32).tolist()


def f32_bits(x):
    return int(np.float32(x).view(np.int32))


@functools.lru_cache(None)
def reference_f64():
    """sr.sgd_steps with a rate per step: g += wd * p; buf = g on the first step, else momentum * buf + g; p -= lr_k * lr_mult * buf."""
    p0, grads, _, _, _ = sk.sgd_data()
    p, buf = p0.double().clone(), torch.zeros(sk.SGD_N, dtype=torch.float64)
    for k, g in enumerate(grads):
        g = g.double()
        for e in sk.SGD_ENTRIES:
            sl = slice(e["off"], e["off"] + e["numel"])
            d = g[sl] + sr._f32(e["wd"]) * p[sl]
            buf[sl] = d if k == 0 else sr._f32(MOM) * buf[sl] + d
            p[sl] = p[sl] - (sr._f32(RATES[k]) * sr._f32(e["lr_mult"])) * buf[sl]
    return p, buf


def launch(name, table, owner, nb, p, g, buf, sc, packed, dt, zero_grads, rate, first, block):
    """One update launch by entry name: the by-value entries take (rate, first), the `_dev` entries the block (a tensor, or a raw
    address for the refusals)."""
    blk = P(block) if torch.is_tensor(block) else block
    if name == "osd_sgd_momentum_multi":
        call(name, P(table), P(owner), nb, P(p), P(g), P(buf), rate, MOM, first, ST())
    elif name == "osd_sgd_momentum_multi_dev":
        call(name, P(table), P(owner), nb, P(p), P(g), P(buf), blk, MOM, ST())
    elif name == "osd_sgd_momentum_pack_multi":
        call(name, P(table), P(owner), nb, P(p), P(g), P(buf), P(sc), P(packed), DTC[dt], rate, MOM, first, zero_grads, ST())
    else:
        assert name == "osd_sgd_momentum_pack_multi_dev"
        call(name, P(table), P(owner), nb, P(p), P(g), P(buf), P(sc), P(packed), DTC[dt], blk, MOM, zero_grads, ST())


def state(name, dt):
    p0, _, scales, _, _ = sk.sgd_data()
    pack = "pack" in name
    table, owner, nb = (sr.sgd_pack_table if pack else sr.sgd_table)(sk.SGD_ENTRIES, "cuda")
    return dict(table=table, owner=owner, nb=nb, p=p0.clone().cuda(), buf=torch.full((sk.SGD_N,), 5.0, device="cuda"),
                sc=scales.cuda(), packed=sk.sgd_packed_init(DT[dt])[0].cuda() if pack else None)


def run_steps(name, dt=None, zero_grads=0):
    """three steps at RATES with first_step = 1, 0, 0 -> (params, momentum, packed or None, the gradients after each step), on the CPU"""
    grads = sk.sgd_data()[1]
    s = state(name, dt)
    guard, block = new_block()
    after = []
    for k in range(3):
        g = grads[k].clone().cuda()
        if name.endswith("_dev"):
            call("osd_solver_set", P(block), RATES[k], int(k == 0), ST())
        launch(name, s["table"], s["owner"], s["nb"], s["p"], g, s["buf"], s["sc"], s["packed"], dt, zero_grads, RATES[k], int(k == 0), block)
        after.append(g.cpu())
    if name.endswith("_dev"):
        assert block_words(guard) == [0x7A7A7A7A] * 2 + [f32_bits(RATES[2]), 0] + [0x7A7A7A7A] * 2
    return s["p"].cpu(), s["buf"].cpu(), None if s["packed"] is None else s["packed"].cpu(), after


@functools.lru_cache(None)
def by_value(name, dt=None, zero_grads=0):
    return run_steps(name, dt, zero_grads)


# ======================================================================================================== 1. the `_dev` entries
@pytest.mark.parametrize("name,dt,zero_grads", [("osd_sgd_momentum_multi", None, 0), ("osd_sgd_momentum_pack_multi", "f32", 0),
                                                ("osd_sgd_momentum_pack_multi", "f32", 1), ("osd_sgd_momentum_pack_multi", "bf16", 0),
                                                ("osd_sgd_momentum_pack_multi", "bf16", 1)])
def test_dev_entries_match_the_by_value_entries_bit_for_bit(name, dt, zero_grads):
    assert name + "_dev" in ("osd_sgd_momentum_multi_dev", "osd_sgd_momentum_pack_multi_dev")
    p0, grads, _, _, _ = sk.sgd_data()
    want = by_value(name, dt, zero_grads)
    got = run_steps(name + "_dev", dt, zero_grads)
    # bit-identical to the by-value entry called with the same rates: parameters, momentum, packed weights, gradients
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    if dt is not None:
        assert torch.equal(got[2].view(torch.int16 if dt == "bf16" else torch.int32), want[2].view(torch.int16 if dt == "bf16" else torch.int32))
    for k in range(3):
        assert torch.equal(got[3][k], want[3][k])
    # the float64 restatement with per-step rates (a by-value run at ONE of the rates is outside the bar: the rates do arrive)
    ref_p, ref_buf = reference_f64()
    m = sk.sgd_inside()
    worst = {}
    for what, g_, r_ in (("params", got[0], ref_p), ("momentum", got[1], ref_buf)):
        worst[what] = float(((g_.double() - r_)[m].abs() / (sr.SGD_ATOL + sr.SGD_RTOL * r_[m].abs())).max())
    sk.note("%s_dev %s" % (name, dt), **worst)
    assert worst["params"] <= 1.0 and worst["momentum"] <= 1.0, worst
    one_rate = sr.sgd_steps(sk.SGD_ENTRIES, p0, grads, RATES[0], MOM)[0]
    assert float(((got[0].double() - one_rate)[m].abs() / (sr.SGD_ATOL + sr.SGD_RTOL * one_rate[m].abs())).max()) > 100.0
    # nothing outside the table's entries is written
    assert torch.equal(got[0][~m], p0[~m]) and bool((got[1][~m] == 5.0).all())
    if dt is not None:
        init, inside = sk.sgd_packed_init(DT[dt])
        assert bool((got[2][~inside] == SENT).all())
        assert torch.equal(got[2], sr.pack_multi(sk.sgd_pack_entries(), got[0], sk.sgd_data()[2], init, 0))
    for k in range(3):
        if zero_grads:
            assert float(got[3][k][m].abs().max()) == 0.0 and torch.equal(got[3][k][~m], grads[k][~m])
        else:
            assert torch.equal(got[3][k], grads[k])


# ======================================================================================================== 2. the setter
def test_solver_set_writes_its_eight_bytes_and_bad_blocks_are_refused():
    from oneshotdet_amd import _lib
    guard, block = new_block()
    call("osd_solver_set", P(block), 0.125, 1, ST())
    assert block_words(guard) == [0x7A7A7A7A] * 2 + [f32_bits(0.125), 1] + [0x7A7A7A7A] * 2
    ops.solver_set(block, RATES[1], False)
    assert block_words(guard) == [0x7A7A7A7A] * 2 + [f32_bits(RATES[1]), 0] + [0x7A7A7A7A] * 2
    # a second set on the same stream is the one the next launch sees
    p0, grads, _, _, _ = sk.sgd_data()
    outs = {}
    for name in ("osd_sgd_momentum_multi", "osd_sgd_momentum_multi_dev"):
        s = state(name, None)
        g = grads[0].clone().cuda()
        call("osd_solver_set", P(block), RATES[0], 0, ST())
        call("osd_solver_set", P(block), RATES[2], 1, ST())
        if name.endswith("_dev"):
            ops.sgd_momentum_multi_dev(s["table"], s["owner"], s["nb"], s["p"], g, s["buf"], block, MOM)
        else:
            launch(name, s["table"], s["owner"], s["nb"], s["p"], g, s["buf"], None, None, None, 0, RATES[2], 1, None)
        outs[name] = (s["p"].cpu(), s["buf"].cpu())
    assert torch.equal(outs["osd_sgd_momentum_multi"][0], outs["osd_sgd_momentum_multi_dev"][0])
    assert torch.equal(outs["osd_sgd_momentum_multi"][1], outs["osd_sgd_momentum_multi_dev"][1])
    assert not torch.equal(outs["osd_sgd_momentum_multi_dev"][0], p0)
    # a null block and a block at ptr + 4: OSD_ERR_INVALID_ARG with a message, nothing launched
    for bad, word in ((None, "null"), (block.data_ptr() + 4, "aligned")):
        before = block_words(guard)
        with pytest.raises(_lib.OsdError, match=word) as e:
            call("osd_solver_set", bad, 0.5, 1, ST())
        assert e.value.code == INVALID_ARG and block_words(guard) == before
        for name, dt in (("osd_sgd_momentum_multi_dev", None), ("osd_sgd_momentum_pack_multi_dev", "bf16")):
            s = state(name, dt)
            g = grads[0].clone().cuda()
            with pytest.raises(_lib.OsdError, match=word) as e:
                launch(name, s["table"], s["owner"], s["nb"], s["p"], g, s["buf"], s["sc"], s["packed"], dt, 1, 0.0, 0, bad)
            assert e.value.code == INVALID_ARG
            torch.cuda.synchronize()
            assert torch.equal(s["p"].cpu(), p0) and bool((s["buf"] == 5.0).all()) and torch.equal(g.cpu(), grads[0])
            if dt is not None:
                assert torch.equal(s["packed"].cpu(), sk.sgd_packed_init(DT[dt])[0])


# ======================================================================================================== 3. inside a captured graph
def test_one_captured_dev_launch_follows_the_block_across_replays():
    """ONE `_dev` launch captured in a graph (a single stream, no branches), replayed three times with osd_solver_set between the
    replays: the three by-value launches of test 1, bit for bit.  A by-value launch cannot do this: its rate is part of the graph."""
    name, dt, zero_grads = "osd_sgd_momentum_pack_multi_dev", "bf16", 1          # through ops.sgd_momentum_pack_multi_dev
    grads = sk.sgd_data()[1]
    want = by_value("osd_sgd_momentum_pack_multi", dt, zero_grads)
    s = state(name, dt)
    guard, block = new_block()
    g = torch.zeros(sk.SGD_N, device="cuda")
    call("osd_solver_set", P(block), 0.0, 0, ST())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sgd_momentum_pack_multi_dev(s["table"], s["owner"], s["nb"], s["p"], g, s["buf"], s["sc"], s["packed"], block, MOM, zero_grads)
    assert torch.equal(s["p"].cpu(), sk.sgd_data()[0])                  # captured, not run
    for k in range(3):
        g.copy_(grads[k])
        ops.solver_set(block, RATES[k], k == 0)
        graph.replay()
        assert torch.equal(g.cpu(), want[3][k])
    torch.cuda.synchronize()
    assert torch.equal(s["p"].cpu(), want[0]) and torch.equal(s["buf"].cpu(), want[1])
    assert torch.equal(s["packed"].cpu().view(torch.int16), want[2].view(torch.int16))
    assert block_words(guard) == [0x7A7A7A7A] * 2 + [f32_bits(RATES[2]), 0] + [0x7A7A7A7A] * 2


# ======================================================================================================== the engine
B, H, W = 2, 128, 160


@functools.lru_cache(None)
def golden_rates(case):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule.npz"))
    return [float(v) for v in g[case + ".lr"][:, 0]]


def schedule(case):
    if case == "zero":
        return LRSchedule(base_lr=0.002, milestones=(2,), gamma=0.0, warmup_iters=0)
    return LRSchedule(base_lr=0.002, milestones=(3,), gamma=0.1, warmup_factor=1.0 / 3, warmup_iters=2, warmup_method="linear")


@functools.lru_cache(None)
def np_sd():
    return synth.make_state_dict(spec.hot_path_shapes())


@functools.lru_cache(None)
def batches(n=5):
    q = torch.from_numpy(synth.make_images("cg.q", B, 63, 63, seed=1)).cuda()
    out = []
    for step in range(n):
        img = torch.from_numpy(synth.make_images("cg.img.%d" % step, B, H, W, seed=step)).cuda()
        gts = synth.make_gt_boxes(B, H, W, seed=60 + step, max_boxes=3)
        gtb = torch.zeros(B, 3, 4)
        for i, g in enumerate(gts):
            gtb[i, :len(g)] = torch.from_numpy(g)
        out.append((img, q, gtb.cuda(), torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda()))
    return out


def engine(lr_schedule=None, lr=0.002, sd=None):
    from oneshotdet_amd import train
    return train.TrainEngine(np_sd() if sd is None else sd, dtype=torch.float32, lr=lr, lr_schedule=lr_schedule)


def capture_after_first_step(eng):
    """As tests/test_gpu_train.py's capture test: capture() runs training steps itself, so restore the state after step 1."""
    eng.join()
    w0, m0, n0 = eng.flat_w.clone(), eng._sgd["buf"].clone(), eng._sgd["steps"]
    eng.capture(*batches()[0], warmup=1)
    assert eng.iteration == n0 + 1              # the warm-up step counts, the captured update (which has not run) does not
    eng.flat_w.copy_(w0)
    eng._sgd["buf"].copy_(m0)
    eng._sgd["steps"] = n0
    eng.repack()


def test_a_rate_of_zero_freezes_the_weights_of_replayed_steps_and_not_the_momentum():
    rates = golden_rates("zero")
    eng = engine(schedule("zero"))
    try:
        assert eng.iteration == 0
        eng.train_step(*batches()[0])
        assert eng.lr == rates[0] and eng.iteration == 1
        capture_after_first_step(eng)
        for k, batch in enumerate(batches()[1:], start=1):
            torch.cuda.synchronize()
            w, m = eng.flat_w.clone(), eng._sgd["buf"].clone()
            eng.replay_step(*batch)
            torch.cuda.synchronize()
            assert eng.lr == rates[k] and eng.iteration == k + 1
            assert not torch.equal(eng._sgd["buf"], m), k
            if k < 2:
                assert rates[k] == 0.002 and not torch.equal(eng.flat_w, w), k
            else:
                assert rates[k] == 0.0 and torch.equal(eng.flat_w, w), k          # p - 0 * buf == p
        assert bool(torch.isfinite(eng._sgd["buf"]).all())
    finally:
        eng.close()


def test_replayed_scheduled_steps_match_eager_scheduled_steps_and_hand_set_rates():
    rates = golden_rates("engine")
    assert len(set(rates[:5])) == 4 and rates[3] == rates[4]          # warmup 0, 1; full rate 2; the milestone at 3
    out = {}
    for mode in ("eager", "graph", "by hand"):
        eng = engine(None if mode == "by hand" else schedule("engine"))
        try:
            losses = []
            for k, batch in enumerate(batches()):
                if mode == "by hand":
                    eng.lr = rates[k]
                if mode == "graph" and k == 1:
                    capture_after_first_step(eng)
                losses.append((eng.replay_step if mode == "graph" and k >= 1 else eng.train_step)(*batch).clone())
                assert eng.lr == rates[k] and eng.iteration == k + 1, (mode, k)
            eng.join()
            torch.cuda.synchronize()
            out[mode] = (torch.stack(losses).cpu(), eng.flat_w.clone().cpu())
        finally:
            eng.close()
    for mode in ("graph", "by hand"):
        dl = float(((out[mode][0] - out["eager"][0]).abs() / (1e-6 + 2e-3 * out["eager"][0].abs())).max())
        dw = float((out[mode][1] - out["eager"][1]).norm() / out["eager"][1].norm())
        sk.note("scheduled steps, %s against eager" % mode, losses_over_bar=dl, weights_rel_l2=dw)
        np.testing.assert_allclose(out[mode][0].numpy(), out["eager"][0].numpy(), rtol=2e-3, atol=1e-6, err_msg=mode)
        assert dw < 1e-4, (mode, dw)


def test_a_resumed_run_continues_the_schedule_at_the_restored_iteration(tmp_path):
    from oneshotdet_amd import checkpoint
    rates = golden_rates("engine")
    eng = engine(schedule("engine"))
    eng2 = None
    try:
        for batch in batches()[:2]:
            eng.train_step(*batch)
        path = checkpoint.save_training_checkpoint(str(tmp_path / "model_0000002.pth"), eng, 2)
        saved = torch.load(path, map_location="cpu", weights_only=False)["scheduler"]
        assert saved == schedule("engine").state_dict(last_epoch=2)
        eng2, it = checkpoint.resume_training(path, lambda sd: engine(schedule("engine"), sd=sd))
        assert it == 2 and eng2.iteration == 2
        la, lb = eng.train_step(*batches()[2]).clone(), eng2.train_step(*batches()[2]).clone()
        assert eng.lr == eng2.lr == rates[2] != rates[0] and eng2.iteration == 3
        eng.join(), eng2.join()
        torch.cuda.synchronize()
        dl = float(((la - lb).abs() / (1e-6 + 1e-4 * la.abs())).max())
        sk.note("resumed third step", losses_over_bar=dl, weights_rel_l2=float((eng.flat_w - eng2.flat_w).norm() / eng.flat_w.norm()))
        torch.testing.assert_close(lb, la, rtol=1e-4, atol=1e-6)
        a, b = eng.state_dict(), eng2.state_dict()
        for k in a:
            torch.testing.assert_close(a[k], b[k], rtol=1e-4, atol=1e-6, msg=lambda m, k=k: "%s: %s" % (k, m))
        with pytest.raises(ValueError, match="gamma"):
            checkpoint.resume_training(path, lambda sd: engine(LRSchedule(0.002, (3,), 0.5, 1.0 / 3, 2, "linear"), sd=sd))
    finally:
        eng.close()
        if eng2 is not None:
            eng2.close()


def test_entry_points_by_phase_with_and_without_a_schedule(monkeypatch):
    """Without a schedule no step, eager or captured, reaches osd_solver_set or a `_dev` entry; with one the `_dev` entries are
    enqueued only while capture() captures the update, and a replay adds exactly one osd_solver_set."""
    from oneshotdet_amd import _lib
    NEW = {"osd_solver_set", "osd_sgd_momentum_multi_dev", "osd_sgd_momentum_pack_multi_dev"}
    BY_VALUE = {"osd_sgd_momentum_multi", "osd_sgd_momentum_pack_multi"}
    seen, phase, real = {}, ["eager"], _lib.call

    def recording(name, *args):
        seen.setdefault(phase[0], []).append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)
    for scheduled in (False, True):
        seen.clear()
        eng = engine(schedule("engine") if scheduled else None)
        try:
            phase[0] = "eager"
            eng.train_step(*batches()[0])
            eng.join()
            phase[0] = "capture"
            eng.capture(*batches()[0], warmup=1)
            phase[0] = "replay"
            eng.replay_step(*batches()[1])
            eng.replay_step(*batches()[2])
            phase[0] = "eager again"
            eng.train_step(*batches()[3])
            eng.join()
            torch.cuda.synchronize()
        finally:
            eng.close()
        for ph in ("eager", "eager again"):
            assert BY_VALUE & set(seen[ph]) and not NEW & set(seen[ph]), (scheduled, ph)
        assert not BY_VALUE & set(seen.get("replay", []))
        if scheduled:
            n_buckets = len([n for n in seen["eager"] if n in BY_VALUE])
            assert len([n for n in seen["capture"] if n.endswith("_dev")]) == n_buckets
            assert seen["capture"].count("osd_solver_set") == 0 and seen["replay"].count("osd_solver_set") == 2
            assert [n for n in seen["replay"] if n in NEW] == ["osd_solver_set"] * 2
        else:
            assert not NEW & set(sum(seen.values(), []))
