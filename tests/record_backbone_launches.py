"""Writes tests/launch_lists/backbone_launches.json: the launch lists and training contexts of model.run_backbone, model.run_backbones
and ForwardPass._backbones_forward AS THE COMMIT BEFORE THE WALKER ISSUED THEM, for every case of launch_trace_cpu.cases().

    git worktree add /tmp/parent <hash of the parent commit>
    python tests/record_backbone_launches.py /tmp/parent [full lists as JSON, to read or diff by hand]

The package is imported from that checkout, never from this tree: the fixture is measured on the parent, not on the code under
test.  No GPU and no built library are needed (launch_trace_cpu.stubbed_ops).

File format: {"parent": hash, "cases": {id: {"launches": "digest of launch 0's signature, of launch 1's, ..., blank-separated",
"ctxs": [digest of branch 0's labelled ctx, ...] or null}}} with launch_trace_cpu.digest: the full lists are half a megabyte of near-repeats that
nobody reads, while one short digest per launch still compares entry for entry and names the first launch that differs."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "launch_lists", "backbone_launches.json")


def main(parent, dump=None):
    parent = os.path.abspath(parent)
    sys.path.insert(0, parent)
    sys.path.insert(1, HERE)
    import oneshotdet_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(oneshotdet_amd.__file__))) == parent, "the package must come from the parent checkout"
    import launch_trace_cpu as lt
    commit = subprocess.check_output(["git", "-C", parent, "rev-parse", "HEAD"]).decode().strip()
    sd = lt.state_dict()
    full = {cid: lt.run_case(sd, dt, shape, driver, options) for cid, dt, shape, driver, options in lt.cases()}
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    with open(FIXTURE, "w") as f:
        f.write('{"parent": "%s", "cases": {\n' % commit)
        f.write(",\n".join('"%s": %s' % (cid, json.dumps(lt.digests(got))) for cid, got in full.items()))
        f.write("\n}}\n")
    if dump:
        with open(dump, "w") as f:
            json.dump(full, f, indent=1)
    print("%s: %d cases, %d launches, %d bytes" % (FIXTURE, len(full), sum(len(g["launches"]) for g in full.values()), os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main(*sys.argv[1:3])
