"""model.run_backbone, model.run_backbones and ForwardPass._backbones_forward are three thin callers of ONE graph walk
(model.walk_backbones).  Each must issue exactly the launches the three hand-written copies issued before the walker existed: same
order, same operands, same parameters and tuner keys, and for training the same saved context.  The expected lists were recorded
from the parent commit (tests/record_backbone_launches.py; the hash is in the fixture), on the CPU with the library call stubbed
(tests/launch_trace_cpu.py), and so are the lists compared here.  The fixture keeps one digest per launch signature and per
ctx (launch_trace_cpu.digest), compared entry for entry; the recorder writes the full lists on request.  No GPU."""
import json
import os

import pytest

import launch_trace_cpu as lt

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launch_lists", "backbone_launches.json")
CASES = lt.cases()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def state_dict():
    return lt.state_dict()


def test_every_case_is_recorded(recorded):
    assert len(recorded["parent"]) == 40
    assert sorted(recorded["cases"]) == sorted(c[0] for c in CASES) and len(CASES) == 42


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launches_equal_the_parent_commits(case, recorded, state_dict):
    cid, dt, shape, driver, options = case
    want = recorded["cases"][cid]
    full = lt.run_case(state_dict, dt, shape, driver, options)
    got = lt.digests(full)
    want_launches, got_launches = want["launches"].split(), got["launches"].split()
    assert len(got_launches) == len(want_launches)
    for i, (g, w) in enumerate(zip(got_launches, want_launches)):      # the fixture keeps digests: show the launch itself
        assert g == w, "launch %d of %s is not the parent's: %s" % (i, cid, json.dumps(full["launches"][i]))
    assert driver.startswith("train") == (want["ctxs"] is not None)
    assert got["ctxs"] == want["ctxs"]


# What the digests cannot show a reader: launches, and RES_DOWN2X convs among them, per walk as counted on the parent commit.
# Drivers: run_backbone, run_backbones, training with two branches, training with the target alone.
COUNTS = {("fp32", "even"): ((63, 1), (126, 2), (128, 2), (64, 1)), ("bf16", "even"): ((59, 1), (126, 2), (126, 2), (63, 1)),
          ("fp32", "odd"): ((63, 1), (126, 0), (128, 0), (64, 0)), ("bf16", "odd"): ((59, 1), (126, 0), (126, 0), (63, 0))}


@pytest.mark.parametrize("dt,shape", sorted(COUNTS))
def test_launch_counts(dt, shape, state_dict):
    from oneshotdet_amd.ops import RES_DOWN2X
    for driver, (launches, down2x) in zip(lt.DRIVERS, COUNTS[dt, shape]):
        sigs = lt.run_case(state_dict, dt, shape, driver, {})["launches"]
        assert (len(sigs), sum(kw.get("res_mode") == RES_DOWN2X for _, kw in sigs)) == (launches, down2x), driver


def test_stub_restores_what_it_patched():
    from oneshotdet_amd import _lib, ops, trace
    before = (_lib.call, ops._chk_dev, ops._stream, ops._stream_handle, trace.TRACE)
    with lt.stubbed_ops():
        trace.TRACE = []
        assert ops._stream() is None
    assert (_lib.call, ops._chk_dev, ops._stream, ops._stream_handle, trace.TRACE) == before
