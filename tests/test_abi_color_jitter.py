"""CPU: include/oneshotdet_hip_color_jitter.h under the rules tests/test_abi.py and tests/test_abi_supp_aug.py hold the other headers to —
the functions it declares are exactly the ones the binding's fifth table (_lib.SIGNATURES_COLOR_JITTER) lists and the library exports —
and the entries' argument checks, which need no GPU: they return before anything is launched."""
import ctypes
import os
import re

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
HEADER = "oneshotdet_hip_color_jitter.h"
NAMES = ["osd_color_jitter_batch", "osd_color_jitter_workspace_bytes"]
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


def test_header_and_fifth_binding_table_agree():
    from oneshotdet_amd import _lib, build
    assert declared(HEADER) == sorted(_lib.SIGNATURES_COLOR_JITTER) == NAMES
    # the tables are disjoint, and no other header declares either name
    others = set(_lib.SIGNATURES) | set(_lib.SIGNATURES_BOX_MODES) | set(_lib.SIGNATURES_SOFT_LABELS) | set(_lib.SIGNATURES_SUPP_AUG)
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != HEADER:
            others |= set(declared(h))
    assert not set(NAMES) & others
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, (res, args) in _lib.SIGNATURES_COLOR_JITTER.items():
        params = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(params.split(",")) == len(args), name
    # (n_images, hs, ws) -> int64; (n_images, srcs, hs, ws, factors, dsts, workspace, stream) -> int
    assert _lib.SIGNATURES_COLOR_JITTER["osd_color_jitter_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SIGNATURES_COLOR_JITTER["osd_color_jitter_batch"] == (ctypes.c_int, [ctypes.c_int] + [ctypes.c_void_p] * 7)
    assert re.search(r"int64_t\s+osd_color_jitter_workspace_bytes\(", src) and re.search(r"\bint\s+osd_color_jitter_batch\(", src)
    # each prototype cites the reference lines it restates; the chunk size is the binding's
    for name in NAMES:
        comment = raw[:raw.index(" %s(" % name)].rsplit("/*", 1)[1]
        assert "coco.py:286-294" in comment, name
    assert re.search(r"#define OSD_COLOR_JITTER_MAX_IMAGES %d\b" % _lib.COLOR_JITTER_MAX_IMAGES, raw)
    # the build compiles the translation unit and depends on the header; the ABI version is not part of this change
    assert "color_jitter.hip" in build.SOURCES
    assert HEADER in [os.path.basename(h) for h in build.HEADERS]
    assert _lib.ABI_VERSION == 4
    # plain C++ on vector memory instructions: no inline assembly in the translation unit
    hip = open(os.path.join(ROOT, "oneshotdet_amd", "csrc", "color_jitter.hip")).read()
    assert not re.search(r"\b(__)?asm(__)?\b", hip)
    # every float step is rounded on its own: contraction is off for the whole file, ahead of the first function, and the product and
    # the sum are not written with hipcc's __fmul_rn / __fadd_rn (plain operators compiled under the header's contraction mode: they fuse)
    code = re.sub(r"//.*", "", hip)
    assert "#pragma clang fp contract(off)" in code and code.index("#pragma clang fp contract(off)") < code.index("__device__")
    assert "__fmul_rn" not in code and "__fadd_rn" not in code


def test_library_exports_and_binds_the_new_entries(lib_path):
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    raw = ctypes.CDLL(lib_path)
    for name in NAMES:
        assert hasattr(raw, name), name
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES_COLOR_JITTER.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.osd_abi_version() == _lib.ABI_VERSION == 4


def _call(lib, n=2, srcs=True, hs=True, ws=True, factors=True, dsts=True, workspace=8192, h=(5, 7), w=(6, 3), f=None, src_ptr=(4096, 4096 + 256),
          dst_ptr=(16384, 16384 + 256)):
    """the entry with made-up, never dereferenced device addresses: every check returns before a launch"""
    k = max(len(h), 1)
    s = (ctypes.c_void_p * k)(*src_ptr[:k])
    d = (ctypes.c_void_p * k)(*dst_ptr[:k])
    hh, ww = (ctypes.c_int32 * k)(*h), (ctypes.c_int32 * k)(*w)
    ff = (ctypes.c_float * (4 * k))(*(f if f is not None else [1.5, 0.5, 1.0, 2.0] * k))
    a = lambda on, v: v if on else None      # noqa: E731
    return lib.osd_color_jitter_batch(n, a(srcs, s), a(hs, hh), a(ws, ww), a(factors, ff), a(dsts, d), workspace or None, None)


def test_argument_checks_return_before_any_launch(lib_path):
    from oneshotdet_amd import _lib
    lib = _lib.load()
    nan, inf = float("nan"), float("inf")
    good = [1.5, 0.5, 1.0, 2.0]
    for kw in (dict(srcs=False), dict(hs=False), dict(ws=False), dict(factors=False), dict(dsts=False), dict(workspace=0),      # a null table
               dict(n=-1),
               dict(src_ptr=(4096, 0)), dict(dst_ptr=(0, 16384)),                                                                # a null image
               dict(h=(5, 0)), dict(w=(-3, 3)), dict(h=(0, 0)),                                                                  # a non-positive size
               dict(f=good + [1.0, nan, 1.0, 1.0]), dict(f=[-0.25] + good[1:] + good), dict(f=good + [1.0, 1.0, 1.0, -1e-30]),
               dict(f=[nan] * 8), dict(f=good + good[:3] + [inf]),                                                               # a bad factor
               dict(dst_ptr=(16384, 4096 + 256)), dict(src_ptr=(16384, 4096 + 256)),                                             # in place
               dict(workspace=8196)):
        assert _call(lib, **kw) == INVALID, kw
        assert lib.osd_last_error_string()
    # the first image of a long list is checked like the last: the whole list before the first chunk is launched
    k = _lib.COLOR_JITTER_MAX_IMAGES + 1
    long = dict(n=k, h=(4,) * k, w=(4,) * k, src_ptr=tuple(4096 + 64 * i for i in range(k)), dst_ptr=tuple(65536 + 64 * i for i in range(k)))
    assert _call(lib, f=good * (k - 1) + [1.0, 1.0, nan, 1.0], **long) == INVALID
    assert _call(lib, **dict(long, dst_ptr=long["dst_ptr"][:-1] + (long["src_ptr"][-1],))) == INVALID
    assert _call(lib, h=(65536, 7), w=(32768, 3)) == UNSUPPORTED                       # 2^31 pixels
    # nothing to do: 0, and nothing is launched (the tables are not looked at)
    assert _call(lib, n=0) == 0 and _call(lib, n=0, h=(0, 0), src_ptr=(0, 0)) == 0


def test_workspace_bytes(lib_path):
    from oneshotdet_amd import _lib
    lib = _lib.load()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    one = lib.osd_color_jitter_workspace_bytes(1, arr(200), arr(300))
    assert one > 0 and one % 256 == 0
    # image by image, so a list's need is the sum of its images'
    assert lib.osd_color_jitter_workspace_bytes(3, arr(200, 1, 37), arr(300, 1, 53)) == one + 2 * lib.osd_color_jitter_workspace_bytes(1, arr(1), arr(1))
    assert lib.osd_color_jitter_workspace_bytes(1, arr(4000), arr(4000)) > one
    for bad in ((0, arr(1), arr(1)), (-1, arr(1), arr(1)), (1, None, arr(1)), (1, arr(1), None), (1, arr(0), arr(5)), (2, arr(3, 3), arr(3, -1))):
        assert lib.osd_color_jitter_workspace_bytes(*bad) == 0
