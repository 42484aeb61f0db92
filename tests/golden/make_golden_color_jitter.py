"""Generate the colour-jitter fixture (FEW_SHOT.NUM_SUPP_AUG = 3) from the REAL reference (build container only).

    python tests/golden/make_golden_color_jitter.py

Per case: `np.random.seed(seed)`, then the reference's own `COCODataset.color_jitter` (data/datasets/coco.py:286-294: four
`np.random.uniform(0.1, 2)` draws from numpy's global stream, each feeding one PIL ImageEnhance step) on a PIL RGB image, imported through
ref_harness's shims as make_golden.gen_dataset does.  The method does not touch `self`, so it is called unbound.  The factors are
recorded by re-seeding and drawing the same four numbers, and checked against a run of the four ImageEnhance steps with exactly those.

tests/golden/color_jitter.npz holds, per case `name`: `name.src` (uint8 [H, W, 3]), `name.seed` (int64), `name.factors` (float64 [4],
as drawn, in the order Color, Brightness, Contrast, Sharpness), `name.out` (uint8 [H, W, 3]); `names` lists the cases.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_harness as rh                 # noqa: E402


def cases():
    """(name, source image): the sizes where the smoothing has no interior (a side < 3), the smallest with one, odd sizes past one
    32 x 8 tile, and the images on which the Contrast mean and the clipping matter (flat, low contrast, a wide gradient)."""
    rng = np.random.RandomState(20241)
    out = []
    for h, w in ((1, 1), (2, 5), (5, 2), (3, 3), (3, 40), (37, 53)):
        out.append(("r%dx%d" % (h, w), rng.randint(0, 256, (h, w, 3)).astype(np.uint8)))
    out.append(("flat", np.full((9, 11, 3), 77, dtype=np.uint8)))
    out.append(("lowcontrast", (112 + rng.randint(0, 32, (23, 29, 3))).astype(np.uint8)))
    yy, xx = np.mgrid[0:127, 0:131]
    grad = np.stack([xx * 255.0 / 130, yy * 255.0 / 126, (xx + yy) * 255.0 / 256], axis=2)
    out.append(("gradient127x131", np.clip(grad + rng.normal(0, 12, grad.shape), 0, 255).astype(np.uint8)))
    return out


def main():
    from PIL import Image, ImageEnhance
    rh.load_reference()
    rh.install_coco_shims()
    from maskrcnn_benchmark.data.datasets import coco as rc
    out, names = {}, []
    for k, (name, src) in enumerate(cases()):
        seed = 1000 + k
        np.random.seed(seed)
        res = np.asarray(rc.COCODataset.color_jitter(None, Image.fromarray(src)))
        np.random.seed(seed)
        factors = np.asarray([np.random.uniform(0.1, 2) for _ in range(4)], dtype=np.float64)
        im = Image.fromarray(src)
        for enh, f in zip((ImageEnhance.Color, ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Sharpness), factors):
            im = enh(im).enhance(f)
        assert res.dtype == np.uint8 and res.shape == src.shape and np.array_equal(res, np.asarray(im)), name
        out[name + ".src"], out[name + ".seed"], out[name + ".factors"], out[name + ".out"] = src, np.int64(seed), factors, res
        names.append(name)
        print("colour-jitter fixture %s: %s, factors %s, %d of %d bytes changed" % (name, src.shape, factors, int((res != src).sum()), src.size))
    out["names"] = np.asarray(names)
    path = os.path.join(HERE, "color_jitter.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 256 * 1024
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
