"""GPU: osd_color_jitter_batch (csrc/color_jitter.hip), transforms.color_jitter / DeviceImage.jittered and the dataset's num_supp_aug=3
against tests/color_jitter_ref.py (the numpy restatement that tests/test_color_jitter.py holds to Pillow and to the reference) and
tests/golden/color_jitter.npz (recorded through the reference's COCODataset.color_jitter).  Every comparison is exact equality: the
result is bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_jitter_ref as cj
import golden_utils as gu
from color_jitter_ref import CASES, NumpyJitter

pytestmark = pytest.mark.gpu
GUARD = 64
MIXED = [(1, 1), (2, 5), (5, 2), (3, 3), (3, 40), (40, 3), (37, 53), (127, 131)]


@pytest.fixture(scope="module")
def fixture():
    return gu.load("color_jitter.npz")


def raw_call(arrays, factors, fill=None):
    """osd_color_jitter_batch through the binding, on buffers of this test's own: every destination is followed by GUARD bytes of 0xA5,
    the workspace is filled with `fill` first.  -> (outputs, guards intact, sources intact)"""
    from oneshotdet_amd import _lib, ops
    n = len(arrays)
    srcs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    dsts = [torch.full((a.size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for a in arrays]
    hs = (C.c_int32 * n)(*[a.shape[0] for a in arrays])
    ws = (C.c_int32 * n)(*[a.shape[1] for a in arrays])
    need = int(_lib.load().osd_color_jitter_workspace_bytes(n, hs, ws))
    assert need > 0 and need % 8 == 0
    wsp = torch.empty((need // 8,), dtype=torch.int64, device="cuda")
    if fill is not None:
        wsp.view(torch.uint8).fill_(fill)
    f32 = np.ascontiguousarray(np.asarray(factors, dtype=np.float64).astype(np.float32).reshape(n, 4))
    _lib.call("osd_color_jitter_batch", n, (C.c_void_p * n)(*[s.data_ptr() for s in srcs]), hs, ws, f32.ctypes.data_as(C.c_void_p),
              (C.c_void_p * n)(*[d.data_ptr() for d in dsts]), ops._ptr(wsp), ops._stream())
    torch.cuda.synchronize()
    outs = [d[:a.size].cpu().numpy().reshape(a.shape) for a, d in zip(arrays, dsts)]
    guards = all(bool((d[a.size:] == 0xA5).all()) for a, d in zip(arrays, dsts))
    same = all(np.array_equal(s.cpu().numpy(), a) for a, s in zip(arrays, srcs))
    return outs, guards, same


def test_every_fixture_case_through_the_c_entry_and_the_wrapper(fixture):
    from oneshotdet_amd import transforms as T
    arrays = [fixture[n + ".src"] for n in CASES]
    factors = [fixture[n + ".factors"] for n in CASES]
    outs, guards, same = raw_call(arrays, factors)
    assert guards and same
    imgs = T.color_jitter(arrays, factors)
    assert all(isinstance(im, T.DeviceImage) for im in imgs)
    for name, a, f, o, im in zip(CASES, arrays, factors, outs, imgs):
        np.testing.assert_array_equal(o, fixture[name + ".out"], err_msg=name)
        np.testing.assert_array_equal(im.src.cpu().numpy(), fixture[name + ".out"], err_msg=name)
        assert im.size == (a.shape[1], a.shape[0])
        single, g1, s1 = raw_call([a], [f])                      # alone, the image gets the same bytes
        assert g1 and s1
        np.testing.assert_array_equal(single[0], fixture[name + ".out"], err_msg=name)
        np.testing.assert_array_equal(T.DeviceImage(a).jittered(f).src.cpu().numpy(), fixture[name + ".out"], err_msg=name)


def test_mixed_sizes_across_a_chunk_boundary():
    from oneshotdet_amd import _lib
    rng = np.random.RandomState(3)
    sizes = list(MIXED)
    while len(sizes) < _lib.COLOR_JITTER_MAX_IMAGES + 1:         # one more image than the kernarg table holds
        sizes.append((int(rng.randint(1, 50)), int(rng.randint(1, 70))))
    sizes.append((127, 131))                                     # and a many-tile image in the second chunk
    arrays = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    factors = rng.uniform(0.1, 2, (len(arrays), 4))
    outs, guards, same = raw_call(arrays, factors, fill=0xFF)
    assert guards and same
    for a, f, o in zip(arrays, factors, outs):
        ref = cj.color_jitter(a, f)
        np.testing.assert_array_equal(o, ref, err_msg=str(a.shape))
        single, g1, s1 = raw_call([a], [f])
        assert g1 and s1
        np.testing.assert_array_equal(single[0], ref, err_msg=str(a.shape))


def test_factors_at_both_branch_edges_in_every_step():
    """0.1, 1.0 and 2.0, one factor in (0, 1) and one in (1, 2), at each of the four steps, the other three steps drawn"""
    rng = np.random.RandomState(8)
    arrays, factors = [], []
    for step in range(4):
        for v in (0.1, 1.0, 2.0, 0.37, 1.63):
            f = rng.uniform(0.1, 2, 4)
            f[step] = v
            factors.append(f)
            arrays.append(rng.randint(0, 256, (int(rng.randint(3, 20)), int(rng.randint(3, 45)), 3)).astype(np.uint8))
    for v in (0.1, 1.0, 2.0, 0.0):                               # and all four at once
        factors.append(np.full(4, v))
        arrays.append(rng.randint(0, 256, (11, 35, 3)).astype(np.uint8))
    outs, guards, same = raw_call(arrays, factors)
    assert guards and same
    for a, f, o in zip(arrays, factors, outs):
        np.testing.assert_array_equal(o, cj.color_jitter(a, f), err_msg="%s %r" % (a.shape, f))
    np.testing.assert_array_equal(outs[-3], arrays[-3])          # all factors 1.0: the image itself


def test_short_decimal_factors_where_a_fused_multiply_add_would_show():
    """With factors like 0.8 or 1.1 the product f * (x - d) lands within one float32 rounding of an integer for many bytes, so the byte
    depends on the product and the sum being rounded separately, as ImagingBlend does.  (Measured on an MI355X with the two fused into
    v_fma_f32: 26 of 1056 bytes of the first image off by 1 or 2, while every test with drawn factors passed.)"""
    rng = np.random.RandomState(0)
    a = rng.randint(0, 256, (20, 30, 3)).astype(np.uint8)
    arrays = [np.ascontiguousarray(a[2:18, 3:25]), a]
    factors = [[1.2, 0.8, 1.1, 0.9], [1.2, 0.8, 1.1, 0.9]]
    grid = np.round(np.arange(0.1, 2.05, 0.1), 1)
    for _ in range(10):
        arrays.append(rng.randint(0, 256, (int(rng.randint(8, 30)), int(rng.randint(8, 50)), 3)).astype(np.uint8))
        factors.append(list(rng.choice(grid, 4)))
    outs, guards, same = raw_call(arrays, factors)
    assert guards and same
    for a, f, o in zip(arrays, factors, outs):
        np.testing.assert_array_equal(o, cj.color_jitter(a, f), err_msg="%s %r" % (a.shape, f))


def test_flat_and_saturated_images_at_factor_two():
    arrays = [np.full((9, 35, 3), 77, np.uint8), np.full((12, 33, 3), 255, np.uint8), np.full((5, 5, 3), 0, np.uint8),
              np.tile(np.array([[[250, 3, 128]]], np.uint8), (10, 40, 1))]
    factors = [np.full(4, 2.0)] * len(arrays)
    outs, guards, same = raw_call(arrays, factors)
    assert guards and same
    for a, f, o in zip(arrays, factors, outs):
        np.testing.assert_array_equal(o, cj.color_jitter(a, f), err_msg=str(a.shape))
    np.testing.assert_array_equal(outs[1], arrays[1])            # all 255 stays all 255: every step clips


def test_result_does_not_depend_on_the_workspace_and_repeats(fixture):
    rng = np.random.RandomState(21)
    arrays = [fixture["gradient127x131.src"], fixture["lowcontrast.src"], rng.randint(0, 256, (70, 90, 3)).astype(np.uint8)]
    factors = rng.uniform(0.1, 2, (3, 4))
    first, g1, s1 = raw_call(arrays, factors, fill=0xFF)
    second, g2, s2 = raw_call(arrays, factors, fill=0xFF)
    third, g3, s3 = raw_call(arrays, factors, fill=0x00)
    assert g1 and g2 and g3 and s1 and s2 and s3
    for a, f, x, y, z in zip(arrays, factors, first, second, third):
        ref = cj.color_jitter(a, f)
        np.testing.assert_array_equal(x, ref)
        np.testing.assert_array_equal(y, ref)
        np.testing.assert_array_equal(z, ref)


def test_wrapper_refuses_transformed_images_and_bad_factors():
    from oneshotdet_amd import _lib, transforms as T
    a = np.random.RandomState(0).randint(0, 256, (20, 30, 3)).astype(np.uint8)
    im = T.DeviceImage(a)
    f = [1.2, 0.8, 1.1, 0.9]
    for bad in (im.resized((10, 15)), im.flipped(), im.flipped().resized((40, 60))):
        with pytest.raises(ValueError, match="untransformed"):
            bad.jittered(f)
        with pytest.raises(ValueError, match="untransformed"):
            T.color_jitter([im, bad], [f, f])
    for factors in ([f], [f, f, f], [[1.0, 1.0, 1.0]] * 2):
        with pytest.raises(ValueError, match="four factors"):
            T.color_jitter([im, a], factors)
    with pytest.raises(_lib.OsdError, match="factor"):
        im.jittered([1.0, -0.5, 1.0, 1.0])
    assert T.color_jitter([], []) == []
    # a crop is an untransformed image; tensors and DeviceImages mix with arrays
    crop = im.crop((3, 2, 25, 18))
    outs = T.color_jitter([crop, torch.from_numpy(a), im], [f, f, f])
    np.testing.assert_array_equal(outs[0].src.cpu().numpy(), cj.color_jitter(a[2:18, 3:25], f))
    np.testing.assert_array_equal(outs[1].src.cpu().numpy(), cj.color_jitter(a, f))
    np.testing.assert_array_equal(outs[2].src.cpu().numpy(), outs[1].src.cpu().numpy())
    np.testing.assert_array_equal(im.src.cpu().numpy(), a)


def test_jittered_image_goes_through_resize_and_collate():
    from oneshotdet_amd import transforms as T
    rng = np.random.RandomState(4)
    a = rng.randint(0, 256, (45, 61, 3)).astype(np.uint8)
    f = [1.4, 0.7, 1.3, 1.8]
    ref = cj.color_jitter(a, f)
    imgs = []
    for im in (T.DeviceImage(a).jittered(f), T.DeviceImage(ref)):        # the device's bytes, and the restatement's uploaded
        im, _ = T.Resize(64, 96)(im, None)
        imgs.append(im.flipped())
    batch = T.collate(imgs, 32)
    assert batch.tensors.shape[0] == 2 and batch.image_sizes[0] == batch.image_sizes[1]
    assert torch.equal(batch.tensors[0], batch.tensors[1])
    packed = T.collate(imgs, 32, stem_dtype=torch.bfloat16)
    assert torch.equal(packed.tensor[0], packed.tensor[1])


def test_dataset_item_with_the_device_jitter_equals_the_numpy_stand_in():
    from oneshotdet_amd import dataset, transforms as T
    coco, pix = gu.dataset_inputs()
    kw = dict(is_train=True, shot=2, supp_area_threshold=60.0, num_supp_aug=3)
    dev = dataset.FewShotCocoDataset(coco, lambda info: pix[info["id"]], **kw)
    host = dataset.FewShotCocoDataset(coco, lambda info: pix[info["id"]], jitter=NumpyJitter(), **kw)
    for idx in range(3):
        a, b = dev[idx]["img_supp"], host[idx]["img_supp"]
        assert len(a) == len(b) == 8
        for k, (x, y) in enumerate(zip(a, b)):
            if k % 4 < 2:
                assert isinstance(x, np.ndarray)
                np.testing.assert_array_equal(x, y)
            else:
                assert isinstance(x, T.DeviceImage) and x.size == (y.shape[1], y.shape[0])
                np.testing.assert_array_equal(x.src.cpu().numpy(), y)
    # the support transforms take the mixed list
    tf = T.build_transforms(supp_min_size=32, supp_max_size=64, is_train=False)[1]
    ds = dataset.FewShotCocoDataset(coco, lambda info: pix[info["id"]], supp_transforms=T.Compose(tf.transforms[:2]), **dict(kw, shot=1))
    supp = ds[0]["img_supp"]
    assert len(supp) == 4 and all(isinstance(s, T.DeviceImage) for s in supp) and len({s.out_hw for s in supp}) == 1
