"""CPU: include/oneshotdet_hip_soft_labels.h under the rules tests/test_abi.py, tests/test_abi_coverage.py and
tests/test_abi_box_modes.py hold the other two headers to — the functions it declares are exactly the ones the binding's third table
(_lib.SIGNATURES_SOFT_LABELS) lists and the library exports, and every one of them names a GPU test that exists and calls it."""
import ctypes
import os
import re

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GPU = "test_gpu_box_soft_labels.py"
HEADER = "oneshotdet_hip_soft_labels.h"

# function -> the test of GPU that calls it by name through _lib.call and checks what it computed
COVERED = {
    "osd_box_match_sample_soft": "test_soft_entry_equals_the_plain_entry_bit_for_bit",
    "osd_box_loss_soft": "test_c_entry_with_padded_strides_bad_labels_and_invalid_rows",
}
# the `ops` wrapper that reaches the function -> a test that calls it against the reference fixture
THROUGH_OPS = {
    "osd_box_match_sample_soft": ("box_match_sample", "soft_func=", "test_sampler_matches_the_reference_fixture"),
    "osd_box_loss_soft": ("box_loss", "soft=", "test_loss_kernel_matches_the_reference_fixture"),
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


def test_header_and_third_binding_table_agree():
    from oneshotdet_amd import _lib
    names = declared(HEADER)
    assert names == sorted(_lib.SIGNATURES_SOFT_LABELS.keys()) == ["osd_box_loss_soft", "osd_box_match_sample_soft"]
    # the three tables are disjoint, and the new header adds nothing to the other two's inventories
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_BOX_MODES) | set(declared("oneshotdet_hip.h")) | set(declared("oneshotdet_hip_box_modes.h"))
    assert not set(names) & others
    assert declared("oneshotdet_hip_box_modes.h") == ["osd_box_decode_opt", "osd_box_loss_opt"]
    # the arguments of the entry each extends + (soft_func, s_soft, all_soft) / (soft, cls_loss)
    assert len(_lib.SIGNATURES_SOFT_LABELS["osd_box_match_sample_soft"][1]) == len(_lib.SIGNATURES["osd_box_match_sample"][1]) + 3
    assert len(_lib.SIGNATURES_SOFT_LABELS["osd_box_loss_soft"][1]) == len(_lib.SIGNATURES["osd_box_loss"][1]) + 2
    assert _lib.SIGNATURES_SOFT_LABELS["osd_box_match_sample_soft"][1][:20] == _lib.SIGNATURES["osd_box_match_sample"][1][:20]
    assert _lib.SIGNATURES_SOFT_LABELS["osd_box_loss_soft"][1][:13] == _lib.SIGNATURES["osd_box_loss"][1][:13]
    # the prototypes have as many parameters as the table
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    for name, (_, args) in _lib.SIGNATURES_SOFT_LABELS.items():
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(params.split(",")) == len(args), name
    # the build depends on the header, and the ABI version is not part of this change
    from oneshotdet_amd import build
    assert HEADER in [os.path.basename(h) for h in build.HEADERS]
    assert _lib.ABI_VERSION == 4


def test_library_exports_and_binds_the_new_entries(lib_path):
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    raw = ctypes.CDLL(lib_path)
    for name in declared(HEADER):
        assert hasattr(raw, name), name
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_SOFT_LABELS.items():
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
    for fn, (wrapper, kw, test) in THROUGH_OPS.items():
        assert "ops.%s(" % wrapper in body(test) and kw in body(test), (fn, test)
        wbody = re.search(r"^def %s\(.*?(?=^def |\Z)" % wrapper, ops_src, flags=re.S | re.M).group(0)
        assert '"%s"' % fn in wbody, (fn, wrapper)
