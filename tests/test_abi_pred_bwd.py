"""CPU: include/oneshotdet_hip_pred_bwd.h under the rules tests/test_abi.py and the other add-on headers' tests hold theirs to — the
functions it declares are exactly the ones the binding's eighth table (_lib.SIGNATURES_PRED_BWD) lists and the library exports, and
each names a GPU test that exists and calls it."""
import ctypes
import os
import re

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
GPU = "test_gpu_pred_bwd.py"
HEADER = "oneshotdet_hip_pred_bwd.h"
OTHER_HEADERS = ("oneshotdet_hip.h", "oneshotdet_hip_box_modes.h", "oneshotdet_hip_soft_labels.h", "oneshotdet_hip_neg_support.h",
                 "oneshotdet_hip_solver.h", "oneshotdet_hip_class_sweep.h", "oneshotdet_hip_gallery.h")
ENTRIES = ["osd_conv2d_pred_bwd", "osd_pred_bwd_workspace_bytes"]

# function -> the test of GPU that reaches it (by name through ctypes, or through ops.pred_bwd_fused) and checks what it computed
COVERED = {
    "osd_conv2d_pred_bwd": "test_unsupported_shapes_return_the_documented_codes",
    "osd_pred_bwd_workspace_bytes": "test_unsupported_shapes_return_the_documented_codes",
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


def test_header_and_eighth_binding_table_agree():
    from oneshotdet_amd import _lib
    names = declared(HEADER)
    assert names == sorted(_lib.SIGNATURES_PRED_BWD.keys()) == ENTRIES
    others = (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_BOX_MODES) | set(_lib.SIGNATURES_SOFT_LABELS) | set(_lib.SIGNATURES_NEG_SUPPORT)
              | set(_lib.SIGNATURES_SOLVER) | set(_lib.SIGNATURES_CLASS_SWEEP) | set(_lib.SIGNATURES_GALLERY))
    for h in OTHER_HEADERS:
        others |= set(declared(h))
    assert not set(names) & others
    # the prototype has as many parameters as the table
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    for name, (_, args) in _lib.SIGNATURES_PRED_BWD.items():
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(params.split(",")) == len(args), name
    # osd_conv2d_wgrad_pred's arguments + (wd_packed, dx, flags)
    new, old = _lib.SIGNATURES_PRED_BWD["osd_conv2d_pred_bwd"], _lib.SIGNATURES["osd_conv2d_wgrad_pred"]
    assert new[0] is old[0] and len(new[1]) == len(old[1]) + 3
    assert (_lib.PRED_BWD_BOTH, _lib.PRED_BWD_DGRAD, _lib.PRED_BWD_WGRAD) == tuple(
        int(re.search(r"#define OSD_PRED_BWD_%s (\d+)" % n, src).group(1)) for n in ("BOTH", "DGRAD", "WGRAD"))
    # the build depends on the header and compiles the kernel's source; the ABI version is not part of this change
    from oneshotdet_amd import build
    assert HEADER in open(build.__file__).read() and "conv_pred_bwd.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 4


def test_library_exports_and_binds_the_new_entries(lib_path):
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    raw = ctypes.CDLL(lib_path)
    for name in declared(HEADER):
        assert hasattr(raw, name), name
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_PRED_BWD.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.osd_abi_version() == _lib.ABI_VERSION == 4
    # the size query is host code: 8 workgroups of 272 pixels for the GPU tests' 2,134 pixels, 9 * cout rows of 256 fp32 values each
    ns, hs, ws = (ctypes.c_int32 * 2)(2, 2), (ctypes.c_int32 * 2)(25, 13), (ctypes.c_int32 * 2)(32, 16)
    assert lib.osd_pred_bwd_workspace_bytes(2, ns, hs, ws, 256, 4) == 8 * 36 * 256 * 4 + 8 * 16 + 256
    assert lib.osd_pred_bwd_workspace_bytes(2, ns, hs, ws, 192, 4) == 0 and lib.osd_pred_bwd_workspace_bytes(2, ns, hs, ws, 256, 5) == 0


def test_the_new_entries_name_a_gpu_test_that_calls_them():
    assert sorted(COVERED) == declared(HEADER)
    src = open(os.path.join(TESTS, GPU)).read()
    assert "pytestmark = pytest.mark.gpu" in src
    for fn, test in COVERED.items():
        m = re.search(r"^def %s\(.*?(?=^def |^@pytest|\Z)" % re.escape(test), src, flags=re.S | re.M)
        assert m and fn in m.group(0), (fn, test)
    ops_src = open(os.path.join(ROOT, "oneshotdet_amd", "ops.py")).read()
    wbody = re.search(r"^def pred_bwd_fused\(.*?(?=^def |\Z)", ops_src, flags=re.S | re.M).group(0)
    assert all('"%s"' % fn in wbody or "osd_pred_bwd_workspace_bytes(" in wbody for fn in COVERED)
    assert "ops().pred_bwd_fused(" in src or "o.pred_bwd_fused(" in src
