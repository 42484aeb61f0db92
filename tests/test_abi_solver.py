"""CPU: include/oneshotdet_hip_solver.h under the rules tests/test_abi.py, tests/test_abi_coverage.py, tests/test_abi_box_modes.py,
tests/test_abi_soft_labels.py and tests/test_abi_neg_support.py hold the other four headers to — the functions it declares are exactly
the ones the binding's fifth table (_lib.SIGNATURES_SOLVER) lists and the library exports, and each names a GPU test that exists and
calls it."""
import ctypes
import os
import re

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GPU = "test_gpu_solver.py"
HEADER = "oneshotdet_hip_solver.h"
OTHER_HEADERS = ("oneshotdet_hip.h", "oneshotdet_hip_box_modes.h", "oneshotdet_hip_soft_labels.h", "oneshotdet_hip_neg_support.h")
ENTRIES = ["osd_sgd_momentum_multi_dev", "osd_sgd_momentum_pack_multi_dev", "osd_solver_set"]

# function -> the test of GPU that calls it by name through _lib.call and checks what it computed
COVERED = {
    "osd_solver_set": "test_solver_set_writes_its_eight_bytes_and_bad_blocks_are_refused",
    "osd_sgd_momentum_multi_dev": "test_dev_entries_match_the_by_value_entries_bit_for_bit",
    "osd_sgd_momentum_pack_multi_dev": "test_dev_entries_match_the_by_value_entries_bit_for_bit",
}
# function -> the `ops` wrapper that reaches it
THROUGH_OPS = {
    "osd_solver_set": "solver_set",
    "osd_sgd_momentum_multi_dev": "sgd_momentum_multi_dev",
    "osd_sgd_momentum_pack_multi_dev": "sgd_momentum_pack_multi_dev",
}


def declared(header):
    """the regex of tests/test_abi.py"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(osd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    from oneshotdet_amd import build
    return build.build_library(verbose=False)


def test_header_and_fifth_binding_table_agree():
    from oneshotdet_amd import _lib
    names = declared(HEADER)
    assert names == sorted(_lib.SIGNATURES_SOLVER.keys()) == ENTRIES
    # the five tables are disjoint, and the new header adds nothing to the other four's inventories
    tables = (_lib.SIGNATURES, _lib.SIGNATURES_BOX_MODES, _lib.SIGNATURES_SOFT_LABELS, _lib.SIGNATURES_NEG_SUPPORT, _lib.SIGNATURES_SOLVER)
    assert sum(len(t) for t in tables) == len(set().union(*tables))
    others = set().union(*tables[:4])
    for h in OTHER_HEADERS:
        others |= set(declared(h))
    assert not set(names) & others
    assert declared("oneshotdet_hip_box_modes.h") == ["osd_box_decode_opt", "osd_box_loss_opt"]
    assert declared("oneshotdet_hip_soft_labels.h") == ["osd_box_loss_soft", "osd_box_match_sample_soft"]
    assert declared("oneshotdet_hip_neg_support.h") == ["osd_box_loss_neg_support"]
    # the by-value entries' arguments with (float lr, int first_step) replaced by one pointer
    for name in ("osd_sgd_momentum_multi", "osd_sgd_momentum_pack_multi"):
        new, old = _lib.SIGNATURES_SOLVER[name + "_dev"], _lib.SIGNATURES[name]
        assert new[0] is old[0] and len(new[1]) == len(old[1]) - 1
        want = list(old[1])
        want.remove(ctypes.c_float), want.remove(ctypes.c_int), want.append(ctypes.c_void_p)
        assert sorted(map(str, new[1])) == sorted(map(str, want)), name
    assert _lib.SIGNATURES_SOLVER["osd_solver_set"][1] == [ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    # the prototypes have as many parameters as the table, and the block replaces lr and first_step
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, args) in _lib.SIGNATURES_SOLVER.items():
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(params.split(",")) == len(args), name
        if name.endswith("_dev"):
            assert re.search(r"\bconst void\* solver_block\b", params) and not re.search(r"\b(lr|first_step)\b", params), name
    # the build depends on the header, and the ABI version is not part of this change
    from oneshotdet_amd import build
    assert HEADER in open(build.__file__).read()
    assert _lib.ABI_VERSION == 4
    # the header states the block's layout
    assert "struct { float lr; int32_t first_step; }" in text and "8 bytes" in text and "8-byte aligned" in text


def test_library_exports_and_binds_the_new_entries(lib_path):
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    raw = ctypes.CDLL(lib_path)
    for name in declared(HEADER):
        assert hasattr(raw, name), name
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_SOLVER.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.osd_abi_version() == _lib.ABI_VERSION == 4


def test_every_new_entry_names_a_gpu_test_that_calls_it():
    assert sorted(COVERED) == sorted(THROUGH_OPS) == declared(HEADER)
    src = open(os.path.join(TESTS, GPU)).read()
    assert "pytestmark = pytest.mark.gpu" in src
    ops_src = open(os.path.join(ROOT, "oneshotdet_amd", "ops.py")).read()

    def body(test):
        m = re.search(r"^def %s\(.*?(?=^def |^@pytest|\Z)" % re.escape(test), src, flags=re.S | re.M)
        assert m, test
        return m.group(0)
    for fn, test in COVERED.items():
        assert '"%s"' % fn in body(test), (fn, test)                    # called by name through _lib.call
    for fn, wrapper in THROUGH_OPS.items():
        wbody = re.search(r"^def %s\(.*?(?=^def |\Z)" % wrapper, ops_src, flags=re.S | re.M).group(0)
        assert '"%s"' % fn in wbody, (fn, wrapper)
        assert "ops.%s(" % wrapper in src, (fn, wrapper)                # and the wrapper is exercised on the GPU too
