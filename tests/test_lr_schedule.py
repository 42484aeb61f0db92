"""CPU: solver.LRSchedule against the rates a real WarmupMultiStepLR of the reference gave (tests/golden/lr_schedule.npz, written by
tests/golden/make_golden_lr_schedule.py), and the `scheduler` field of a training checkpoint through save_training_checkpoint /
resume_training with a stand-in engine.

Bars.  The weight group's rate is the same Python arithmetic in the same order: bit-equal doubles.  The bias group's rate is formed
on the device as float32(lr) * 2.0f: one rounding to fp32 (relative 2^-24), then an exact doubling; the reference's own bias-group
double differs from twice the weight group's by a few ulps of a double (2^-52), which the bar 2^-23 swallows."""
import os

import numpy as np
import pytest
import torch

from fake_engine import FakeEngine
from oneshotdet_amd import checkpoint, spec
from oneshotdet_amd.solver import LRSchedule

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule.npz")
CASES = ("record", "defaults", "inside", "half", "nomilestones", "zero", "engine")      # the issue's six and the engine tests' own


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def schedule_of(golden, name):
    g = lambda f: golden["%s.%s" % (name, f)]      # noqa: E731
    return LRSchedule(float(g("base_lr")), tuple(int(m) for m in g("milestones")), float(g("gamma")), float(g("warmup_factor")),
                      int(g("warmup_iters")), str(g("warmup_method")))


def test_the_fixture_holds_the_cases_of_the_issue(golden):
    assert sorted(k.split(".")[0] for k in golden if k.endswith(".lr")) == sorted(CASES)
    assert golden["record.k"].tolist() == [0, 99, 100, 59999, 60000, 89999, 90000, 119999, 120000, 129999]
    assert golden["defaults.k"].tolist()[:520] == list(range(520)) and str(golden["defaults.warmup_method"]) == "linear"
    assert golden["inside.milestones"].tolist() == [3, 7] and int(golden["inside.warmup_iters"]) == 10
    assert float(golden["half.gamma"]) == 0.5 and golden["nomilestones.milestones"].size == 0 and float(golden["zero.gamma"]) == 0.0
    for name in CASES:
        assert golden[name + ".lr"].dtype == np.float64 and golden[name + ".lr"].shape == (len(golden[name + ".k"]), 2)
    assert os.path.getsize(GOLDEN) < 64 * 1024


@pytest.mark.parametrize("name", CASES)
def test_lr_at_is_bit_equal_to_the_reference_and_the_bias_rate_within_one_fp32_rounding(golden, name):
    s = schedule_of(golden, name)
    for k, (w, b) in zip(golden[name + ".k"].tolist(), golden[name + ".lr"].tolist()):
        got = s.lr_at(k)
        assert type(got) is float and got == w and np.float64(got).tobytes() == np.float64(w).tobytes(), (name, k, got, w)
        bias = float(np.float32(2.0) * np.float32(got))            # what the kernel forms: lr (a C float) * lr_mult
        assert abs(bias - b) <= 2.0 ** -23 * abs(b), (name, k, bias, b)


def test_defaults_and_the_schedule_of_record(golden):
    d = LRSchedule()
    assert (d.base_lr, d.milestones, d.gamma, d.warmup_factor, d.warmup_iters, d.warmup_method) == (0.001, (30000,), 0.1, 1.0 / 3, 500, "linear")
    assert d.state_dict() == schedule_of(golden, "defaults").state_dict()
    r = LRSchedule.of_record()
    assert r.state_dict() == schedule_of(golden, "record").state_dict()
    assert r.lr_at(0) == 0.0005 * (1.0 / 3) and r.lr_at(100) == 0.0005 and r.lr_at(60000) == 0.0005 * 1 * 0.1 ** 1
    # a rate of exactly zero (gamma 0.0 past the milestone): the engine test's frozen weights rest on it
    z = schedule_of(golden, "zero")
    assert z.lr_at(1) == 0.002 and z.lr_at(2) == 0.0 and z.lr_at(5) == 0.0


def test_the_references_two_value_errors():
    with pytest.raises(ValueError, match="[Mm]ilestones"):
        LRSchedule(milestones=(7, 3))
    with pytest.raises(ValueError, match="warmup_method"):
        LRSchedule(warmup_method="exponential")
    LRSchedule(milestones=(3, 3, 7), warmup_method="constant")          # sorted, not strictly increasing: accepted, as the reference


def test_state_dict_uses_the_reference_schedulers_attribute_names_and_round_trips():
    s = LRSchedule(0.002, (3, 7), 0.5, 0.25, 10, "constant")
    st = s.state_dict(last_epoch=5)
    assert st == {"milestones": [3, 7], "gamma": 0.5, "warmup_factor": 0.25, "warmup_iters": 10, "warmup_method": "constant",
                  "base_lrs": [0.002, 0.004], "last_epoch": 5}
    t = LRSchedule()
    assert t.load_state_dict(st) == 5
    assert t.state_dict(5) == st and all(t.lr_at(k) == s.lr_at(k) for k in range(12))
    assert s.differences(st) == [] and s.differences(dict(st, last_epoch=9)) == []
    assert t.differences(dict(st, gamma=0.1)) == [("gamma", 0.5, 0.1)]
    with pytest.raises(ValueError):
        t.load_state_dict(dict(st, milestones=[7, 3]))


# ------------------------------------------------------------------------------------------------------------ checkpoints
class _Engine(FakeEngine):
    """FakeEngine with the update count the checkpoint code reads from an engine that has a schedule."""

    def __init__(self, sd, steps=0, **kw):
        FakeEngine.__init__(self, sd, **kw)
        self.steps = steps

    @property
    def iteration(self):
        return self.steps

    def optimizer_state_dict(self):
        return {"momentum_buffer": {}, "steps": self.steps, "lr": 0.01, "momentum": 0.9, "weight_decay": 1e-4}

    def load_optimizer_state_dict(self, st):
        FakeEngine.load_optimizer_state_dict(self, st)
        self.steps = int(st["steps"])


def _sd():
    return {k: torch.zeros(()).expand(s) for k, s in spec.full_model_shapes().items()}


SCHEDULE = dict(base_lr=0.002, milestones=(3, 7), gamma=0.5, warmup_factor=0.25, warmup_iters=10, warmup_method="linear")


def _file(tmp_path, schedule, steps=6):
    eng = _Engine(_sd(), steps=steps) if schedule is None else _Engine(_sd(), steps=steps, lr_schedule=schedule)
    return checkpoint.save_training_checkpoint(str(tmp_path / "model.pth"), eng, steps)


def test_the_scheduler_field_is_written_only_by_an_engine_with_a_schedule(tmp_path):
    p = _file(tmp_path, LRSchedule(**SCHEDULE))
    raw = torch.load(p, map_location="cpu", weights_only=False)
    assert set(raw) == {"model", "optimizer", "iteration", "scheduler"} | set(spec.MODEL_OPTIONS)
    assert raw["scheduler"] == LRSchedule(**SCHEDULE).state_dict(last_epoch=6) and raw["scheduler"]["last_epoch"] == 6
    p = _file(tmp_path, None)
    assert "scheduler" not in torch.load(p, map_location="cpu", weights_only=False)
    import inspect
    assert "lr_schedule" not in inspect.signature(checkpoint.resume_training).parameters and "lr_schedule" not in spec.MODEL_OPTIONS


@pytest.mark.parametrize("in_file", [True, False])
@pytest.mark.parametrize("in_engine", [True, False])
def test_the_four_combinations_of_file_and_engine(tmp_path, in_file, in_engine):
    p = _file(tmp_path, LRSchedule(**SCHEDULE) if in_file else None)
    mine = LRSchedule(**SCHEDULE) if in_engine else None
    eng, it = checkpoint.resume_training(p, lambda sd: _Engine(sd, lr_schedule=mine) if in_engine else _Engine(sd))
    assert it == 6 and eng.iteration == 6 and eng.opt_state["lr"] == 0.01          # the count and the optimiser state are restored
    if in_engine:       # the engine's schedule goes on at the restored count (no second warmup)
        assert eng.lr_schedule is mine and mine.lr_at(eng.iteration) == LRSchedule(**SCHEDULE).lr_at(6) != mine.lr_at(0)
    else:
        assert getattr(eng, "lr_schedule", None) is None


@pytest.mark.parametrize("field,other", [("base_lr", 0.004), ("milestones", (3, 8)), ("gamma", 0.1), ("warmup_factor", 0.5),
                                         ("warmup_iters", 11), ("warmup_method", "constant")])
def test_a_mismatch_names_the_field_and_both_values(tmp_path, field, other):
    p = _file(tmp_path, LRSchedule(**SCHEDULE))
    built = LRSchedule(**dict(SCHEDULE, **{field: other}))
    name = "base_lrs" if field == "base_lr" else field
    with pytest.raises(ValueError) as e:
        checkpoint.resume_training(p, lambda sd: _Engine(sd, lr_schedule=built))
    msg = str(e.value)
    assert name in msg and repr(LRSchedule(**SCHEDULE).state_dict()[name]) in msg and repr(built.state_dict()[name]) in msg, msg
    # last_epoch is not compared: the same schedule resumes from any count
    eng, _ = checkpoint.resume_training(p, lambda sd: _Engine(sd, steps=99, lr_schedule=LRSchedule(**SCHEDULE)))
    assert eng.iteration == 6
