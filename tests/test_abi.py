"""CPU: include/oneshotdet_hip.h declares exactly the functions _lib.SIGNATURES lists, with as many parameters, and the built library
exports and binds every one of them (no compute calls without a GPU).  The entries that extend another entry are held to the
relation their comments state.  (The loss-mode and soft-label headers have tables and tests of their own: tests/test_abi_box_modes.py,
tests/test_abi_soft_labels.py.)"""
import ctypes
import os
import re

import pytest

from abi_utils import HEADER, code, declared, section_of

_p, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float

# entry -> (the entry it extends, arguments more, (types removed, types added) where the added types are pinned exactly)
EXTENDS = {
    "osd_box_loss_neg_support": ("osd_box_loss", 4, ([], [_p, _p, _f, _f])),          # + pred_neg, d_pred_neg, margin, w_suppress
    "osd_sgd_momentum_multi_dev": ("osd_sgd_momentum_multi", -1, ([_f, _i], [_p])),   # (lr, first_step) -> solver_block
    "osd_sgd_momentum_pack_multi_dev": ("osd_sgd_momentum_pack_multi", -1, ([_f, _i], [_p])),
    "osd_roi_pool_levels_sweep": ("osd_roi_pool_levels", 1, None),                    # + sets_per_image
    "osd_correlate_levels_sweep": ("osd_correlate_levels", 1, None),                  # + classes
    "osd_correlate_levels_gallery": ("osd_correlate_levels_sweep", 2, None),          # + slots, n_gallery
    "osd_groupnorm_act_rois_gallery": ("osd_groupnorm_act_rois", 2, None),            # + add_index, n_add
    "osd_conv2d_pred_bwd": ("osd_conv2d_wgrad_pred", 3, None),                        # + wd_packed, dx, flags
}
# entries whose table row is pinned as it stands
EXACT = {"osd_solver_set": (_i, [_p, _f, _i, _p])}
# parameter names a prototype must have, and must not have
PARAMS = {
    "osd_box_loss_neg_support": (("pred_neg", "d_pred_neg", "margin", "w_suppress"), ()),
    "osd_sgd_momentum_multi_dev": (("const void* solver_block",), ("lr", "first_step")),
    "osd_sgd_momentum_pack_multi_dev": (("const void* solver_block",), ("lr", "first_step")),
}


def prototype_params(name):
    """the text between the parentheses of `name`'s prototype"""
    return re.search(r"\b%s\s*\((.*?)\)\s*;" % name, code(open(HEADER).read()), flags=re.S).group(1)


@pytest.fixture(scope="module")
def lib_path():
    from oneshotdet_amd import build
    return build.build_library(verbose=False)


def test_header_and_binding_agree():
    from oneshotdet_amd import _lib
    names = declared()
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)   # no name is declared twice
    assert names == list(_lib.SIGNATURES)            # the same functions, the table in the header's order
    assert set(EXTENDS) | set(EXACT) | {"osd_class_sweep_group", "osd_pred_bwd_workspace_bytes"} <= set(names)
    assert _lib.ABI_VERSION == 4


def test_every_prototype_has_as_many_parameters_as_its_table_row():
    from oneshotdet_amd import _lib
    for name, (_, args) in _lib.SIGNATURES.items():
        params = [p for p in prototype_params(name).split(",") if p.strip() != "void"]
        assert len(params) == len(args), name
    for name, (have, have_not) in PARAMS.items():
        params = prototype_params(name)
        for word in have:
            assert re.search(r"\b%s\b" % re.escape(word), params), (name, word)
        for word in have_not:
            assert not re.search(r"\b%s\b" % word, params), (name, word)


def test_entries_that_extend_another_entry_differ_from_it_as_stated():
    from oneshotdet_amd import _lib
    for name, (base, more, exact) in EXTENDS.items():
        new, old = _lib.SIGNATURES[name], _lib.SIGNATURES[base]
        assert new[0] is old[0] and len(new[1]) == len(old[1]) + more, name
        if exact:
            want = list(old[1])
            for t in exact[0]:
                want.remove(t)
            assert sorted(map(str, new[1])) == sorted(map(str, want + exact[1])), name
    for name, row in EXACT.items():
        assert _lib.SIGNATURES[name] == row, name
    src = open(HEADER).read()
    assert (_lib.PRED_BWD_BOTH, _lib.PRED_BWD_DGRAD, _lib.PRED_BWD_WGRAD) == tuple(
        int(re.search(r"#define OSD_PRED_BWD_%s (\d+)" % n, src).group(1)) for n in ("BOTH", "DGRAD", "WGRAD"))


def test_sections_state_what_their_entries_replace_and_answer():
    """each text is looked for in the section that declares the function concerned, not anywhere in the header"""
    neg = section_of("osd_box_loss_neg_support")
    assert "K == 0" in neg and "NaN" in neg                   # the kernel's answer where the reference has none
    for name in ("osd_solver_set", "osd_sgd_momentum_multi_dev", "osd_sgd_momentum_pack_multi_dev"):
        text = section_of(name)                               # the solver block's layout
        assert "struct { float lr; int32_t first_step; }" in text and "8 bytes" in text and "8-byte aligned" in text, name
    # what each class-sweep and gallery entry replaces or stands in for
    assert "generalized_rcnn.py:307-311" in section_of("osd_correlate_levels_sweep")
    assert "poolers.py:93-124" in section_of("osd_roi_pool_levels_sweep")
    assert "generalized_rcnn.py:307-311" in section_of("osd_correlate_levels_gallery")
    assert "box_head.py:43-66" in section_of("osd_groupnorm_act_rois_gallery")


def test_build_depends_on_the_header_and_compiles_the_kernel_sources():
    from oneshotdet_amd import build
    assert os.path.realpath(HEADER) in [os.path.realpath(h) for h in build.HEADERS]
    for src in ("class_sweep.hip", "gallery.hip", "conv_pred_bwd.hip"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src)), src


def test_library_exports_every_declared_symbol(lib_path):
    import torch  # noqa: F401  resolves libamdhip64.so.7 to the runtime torch ships
    lib = ctypes.CDLL(lib_path)
    for name in declared():
        assert hasattr(lib, name), name
    lib.osd_abi_version.restype = ctypes.c_int
    from oneshotdet_amd import _lib
    assert lib.osd_abi_version() == _lib.ABI_VERSION == 4


def test_load_binds_every_function_with_the_tables_types(lib_path):
    from oneshotdet_amd import _lib
    lib = _lib.load()
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.osd_abi_version() == _lib.ABI_VERSION == 4
    group = lib.osd_class_sweep_group()
    m = re.search(r"#define OSD_CLASS_SWEEP_GROUP (\d+)", open(HEADER).read())
    assert group == int(m.group(1)) and group >= 2
    # the size query is host code: 8 workgroups of 272 pixels for the GPU tests' 2,134 pixels, 9 * cout rows of 256 fp32 values each
    ns, hs, ws = (ctypes.c_int32 * 2)(2, 2), (ctypes.c_int32 * 2)(25, 13), (ctypes.c_int32 * 2)(32, 16)
    assert lib.osd_pred_bwd_workspace_bytes(2, ns, hs, ws, 256, 4) == 8 * 36 * 256 * 4 + 8 * 16 + 256
    assert lib.osd_pred_bwd_workspace_bytes(2, ns, hs, ws, 192, 4) == 0 and lib.osd_pred_bwd_workspace_bytes(2, ns, hs, ws, 256, 5) == 0


def test_ops_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from oneshotdet_amd import _lib, model, ops, spec, synth
    with pytest.raises(_lib.OsdError):
        model.HotPathEngine(synth.make_state_dict(spec.hot_path_shapes()))
    with pytest.raises(_lib.OsdError):
        ops.correlate(torch.zeros(1, 2, 2, 8), torch.zeros(1, 8))


def test_invalid_arguments_return_error_codes(lib_path):
    """Error behaviour of the boundary: negative return code + message, never a crash (no GPU needed: argument checks
    run before any launch)."""
    from oneshotdet_amd import _lib
    lib = _lib.load()
    d = _lib.ConvDesc()
    d.cout = 3
    rc = lib.osd_conv2d_fwd(ctypes.byref(d), None, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"null" in lib.osd_last_error_string()
    rc = lib.osd_correlate_fwd(None, None, None, 1, 1, 8, 0, None)
    assert rc == -1
    assert lib.osd_correlate_fwd(None, None, None, 0, 1, 8, 0, None) == 0     # empty batch: no-op
    assert lib.osd_nms_workspace_bytes(2, 130) == 2 * 192 * 3 * 8 + (1 + 8) * 8      # mask rows padded to 64 + per-image flags
