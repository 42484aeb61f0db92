"""CPU: include/oneshotdet_hip_box_modes.h under the two rules tests/test_abi.py and tests/test_abi_coverage.py hold
include/oneshotdet_hip.h to — the functions it declares are exactly the ones the binding's second table
(_lib.SIGNATURES_BOX_MODES) lists and the library exports, and every one of them names a GPU test that exists and calls it."""
import ctypes
import os
import re

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GPU = "test_gpu_box_cls_modes.py"

# function -> (test file, test function) that runs it on the GPU and checks what it computed
COVERED = {
    "osd_box_loss_opt": (GPU, "test_c_entry_with_padded_strides_bad_labels_and_invalid_rows"),
    "osd_box_decode_opt": (GPU, "test_old_entries_equal_the_opt_entries_in_ce_mode_bit_for_bit"),
}
# the `ops` wrapper that reaches the function in the one-logit modes -> a test that calls it against the reference fixture
THROUGH_OPS = {
    "osd_box_loss_opt": ("box_loss", "test_loss_kernel_matches_the_reference_fixture"),
    "osd_box_decode_opt": ("box_decode", "test_decode_kernel_matches_the_reference_fixture"),
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


def test_header_and_second_binding_table_agree():
    from oneshotdet_amd import _lib
    names = declared("oneshotdet_hip_box_modes.h")
    assert names == sorted(_lib.SIGNATURES_BOX_MODES.keys()) == ["osd_box_decode_opt", "osd_box_loss_opt"]
    # the two tables are disjoint, and the new header adds nothing to the main one's inventory
    assert not set(names) & set(_lib.SIGNATURES) and not set(names) & set(declared("oneshotdet_hip.h"))
    # one argument more than the entry it extends (+ gamma, alpha for the loss)
    assert len(_lib.SIGNATURES_BOX_MODES["osd_box_loss_opt"][1]) == len(_lib.SIGNATURES["osd_box_loss"][1]) + 3
    assert len(_lib.SIGNATURES_BOX_MODES["osd_box_decode_opt"][1]) == len(_lib.SIGNATURES["osd_box_decode"][1]) + 1
    # the build depends on the header
    from oneshotdet_amd import build
    assert "oneshotdet_hip_box_modes.h" in [os.path.basename(h) for h in build.HEADERS]


def test_library_exports_and_binds_the_new_entries(lib_path):
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    raw = ctypes.CDLL(lib_path)
    for name in declared("oneshotdet_hip_box_modes.h"):
        assert hasattr(raw, name), name
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_BOX_MODES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.osd_abi_version() == _lib.ABI_VERSION == 4


def test_every_new_entry_names_a_gpu_test_that_calls_it():
    assert sorted(COVERED) == sorted(THROUGH_OPS) == declared("oneshotdet_hip_box_modes.h")
    for fn, (path, test) in COVERED.items():
        src = open(os.path.join(TESTS, path)).read()
        m = re.search(r"^def %s\(.*?(?=^def |^@pytest|\Z)" % re.escape(test), src, flags=re.S | re.M)
        assert m, (fn, test)
        assert '"%s"' % fn in m.group(0), (fn, test)                    # called by name through _lib.call
        assert "pytestmark = pytest.mark.gpu" in src
    for fn, (wrapper, test) in THROUGH_OPS.items():
        src = open(os.path.join(TESTS, GPU)).read()
        m = re.search(r"^def %s\(.*?(?=^def |^@pytest|\Z)" % re.escape(test), src, flags=re.S | re.M)
        assert m and "ops.%s(" % wrapper in m.group(0) and "cls_loss=mode" in m.group(0), (fn, test)
        ops_src = open(os.path.join(ROOT, "oneshotdet_amd", "ops.py")).read()
        body = re.search(r"^def %s\(.*?(?=^def |\Z)" % wrapper, ops_src, flags=re.S | re.M).group(0)
        assert '"%s"' % fn in body, (fn, wrapper)
