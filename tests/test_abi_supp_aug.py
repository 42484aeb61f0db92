"""CPU: include/oneshotdet_hip_supp_aug.h under the rules tests/test_abi.py and tests/test_abi_soft_labels.py hold the other headers to
— the functions it declares are exactly the ones the binding's fourth table (_lib.SIGNATURES_SUPP_AUG) lists and the library exports —
and the entries' argument checks, which need no GPU: they return before anything is launched."""
import ctypes
import os
import re

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
HEADER = "oneshotdet_hip_supp_aug.h"
NAMES = ["osd_supp_aug_reduce_levels", "osd_supp_aug_reduce_levels_bwd"]
INVALID, UNSUPPORTED = -1, -2


def declared(header):
    """the regex of tests/test_abi.py"""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(osd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib_path():
    from oneshotdet_amd import build
    return build.build_library(verbose=False)


def test_header_and_fourth_binding_table_agree():
    from oneshotdet_amd import _lib, build
    assert declared(HEADER) == sorted(_lib.SIGNATURES_SUPP_AUG) == NAMES
    # the tables are disjoint, and the main header (which tests/test_abi.py holds to SIGNATURES exactly) declares neither name
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_BOX_MODES) | set(_lib.SIGNATURES_SOFT_LABELS)
    for h in ("oneshotdet_hip.h", "oneshotdet_hip_box_modes.h", "oneshotdet_hip_soft_labels.h"):
        others |= set(declared(h))
    assert not set(NAMES) & others
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, (res, args) in _lib.SIGNATURES_SUPP_AUG.items():
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(params.split(",")) == len(args), name
        assert res is ctypes.c_int
    # (n_levels, x, y, hw, groups, aug, c, dtype, method, stream); the backward takes dy as well
    assert len(_lib.SIGNATURES_SUPP_AUG[NAMES[0]][1]) == 10 and len(_lib.SIGNATURES_SUPP_AUG[NAMES[1]][1]) == 11
    # each prototype cites the reference lines it restates, and the method codes are the binding's
    for name in NAMES:
        comment = raw[:raw.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "generalized_rcnn.py:280-288" in comment, name
    assert re.search(r"#define OSD_SUPP_AUG_AVG 0\b", raw) and re.search(r"#define OSD_SUPP_AUG_MAX 1\b", raw)
    assert (_lib.SUPP_AUG_AVG, _lib.SUPP_AUG_MAX) == (0, 1)
    # the build compiles the translation unit and depends on the header; the ABI version is not part of this change
    assert "supp_aug.hip" in build.SOURCES
    assert HEADER in [os.path.basename(h) for h in build.HEADERS]
    assert _lib.ABI_VERSION == 4


def test_library_exports_and_binds_the_new_entries(lib_path):
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    raw = ctypes.CDLL(lib_path)
    for name in NAMES:
        assert hasattr(raw, name), name
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_SUPP_AUG.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.osd_abi_version() == _lib.ABI_VERSION == 4


def _call(lib, bwd, n_levels=2, x=True, y=True, dy=True, hw=True, groups=3, aug=2, c=8, dtype=1, method=0, level_ptr=4096):
    """either entry with made-up, 16-byte aligned, never dereferenced addresses: every check returns before a launch"""
    ptrs = (ctypes.c_void_p * 9)(*([level_ptr] * 9))
    sizes = (ctypes.c_int32 * 9)(*([4] * 9))
    a = lambda on, v: v if on else None      # noqa: E731
    if bwd:
        return lib.osd_supp_aug_reduce_levels_bwd(n_levels, a(x, ptrs), a(dy, ptrs), a(y, ptrs), a(hw, sizes), groups, aug, c, dtype,
                                                  method, None)
    return lib.osd_supp_aug_reduce_levels(n_levels, a(x, ptrs), a(y, ptrs), a(hw, sizes), groups, aug, c, dtype, method, None)


@pytest.mark.parametrize("bwd", [False, True])
def test_argument_checks_return_before_any_launch(lib_path, bwd):
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for kw in (dict(x=False), dict(y=False), dict(hw=False), dict(aug=1), dict(aug=0), dict(aug=9), dict(n_levels=9), dict(n_levels=0),
               dict(dtype=2), dict(method=2), dict(method=-1), dict(groups=-1), dict(level_ptr=0)):
        assert _call(lib, bwd, **kw) == INVALID, kw
        assert lib.osd_last_error_string()
    if bwd:
        assert _call(lib, True, dy=False) == INVALID
    # one 16-byte group is 8 bf16 or 4 fp32 channels
    for kw in (dict(c=12, dtype=1), dict(c=4, dtype=1), dict(c=6, dtype=0), dict(level_ptr=4100), dict(groups=1 << 27, c=8)):
        assert _call(lib, bwd, **kw) == UNSUPPORTED, kw
    assert _call(lib, bwd, c=12, dtype=0, groups=0) == 0 and _call(lib, bwd, c=24, dtype=1, groups=0, aug=8, n_levels=8) == 0
    # the order of the header: a bad group size is an invalid argument even where the channel count is unsupported too
    assert _call(lib, bwd, aug=1, c=12) == INVALID


def test_ops_refuse_an_unknown_method_before_touching_tensors():
    from oneshotdet_amd import ops
    for fn, args in ((ops.supp_aug_reduce_levels, (None, 2)), (ops.supp_aug_reduce_levels_bwd, (None, None, 2))):
        for method in ("conv", "mean", None, 0):
            with pytest.raises(ValueError, match="SUPP_AUG_METHOD"):
                fn(*args, method)
