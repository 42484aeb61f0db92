"""The reference's colour jitter (data/datasets/coco.py:286-294), restated in numpy: four PIL ImageEnhance steps — Color, Brightness,
Contrast, Sharpness — each `Image.blend(degenerate, image, factor)` with a factor drawn from `np.random.uniform(0.1, 2)`.  Every step is
integer or float32 arithmetic on bytes (Pillow: Convert.c rgb2l, Blend.c ImagingBlend, ImageStat mean, Filter.c ImagingFilter3x3 with
ImageFilter.SMOOTH), so the restatement is exact: tests/test_color_jitter.py holds it byte for byte to the fixture recorded through the
reference's own method and to the installed Pillow.  It is what osd_color_jitter_batch (csrc/color_jitter.hip) is compared with.

Input uint8 RGB a[H, W, 3]; factors f[4] float64 as drawn, each converted to float32 once, in the order Color, Brightness, Contrast,
Sharpness.  Every step yields a uint8 image that the next step reads.
"""
import numpy as np

F32 = np.float32
CASES = ["r1x1", "r2x5", "r5x2", "r3x3", "r3x40", "r37x53", "flat", "lowcontrast", "gradient127x131"]      # of tests/golden/color_jitter.npz


def draw_factors(rng):
    """four factors in the reference's order of draws; `rng` is anything with .uniform (np.random itself in the reference)"""
    return np.asarray([rng.uniform(0.1, 2) for _ in range(4)], dtype=np.float64)


def luma(a):
    """PIL convert("L"): (R*19595 + G*38470 + B*7471 + 0x8000) >> 16"""
    a = a.astype(np.int64)
    return ((a[..., 0] * 19595 + a[..., 1] * 38470 + a[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, x, f):
    """ImagingBlend(d, x, f) per byte: t = float32(d) + float32(f * float32(x - d)), product and sum each rounded to float32;
    0 <= f <= 1 truncates, any other factor clips to 0..255 first."""
    f = F32(f)
    d = np.broadcast_to(np.asarray(d), np.shape(x)).astype(np.int32)
    x = np.asarray(x).astype(np.int32)
    prod = (f * (x - d).astype(F32)).astype(F32)
    t = (d.astype(F32) + prod).astype(F32)
    if F32(0) <= f <= F32(1):
        return np.trunc(t).astype(np.int32).astype(np.uint8)
    out = np.trunc(np.clip(t, F32(0), F32(255))).astype(np.int32)
    out[t <= 0] = 0
    out[t >= 255] = 255
    return out.astype(np.uint8)


def smooth(a):
    """ImageFilter.SMOOTH: the 3x3 kernel (1 1 1 / 1 5 1 / 1 1 1) / 13 with float32 weights, + 0.5, truncated and clipped, on the interior;
    border pixels are copies.  An image with H < 3 or W < 3 has no interior."""
    h, w = a.shape[:2]
    out = a.copy()
    if h < 3 or w < 3:
        return out
    k, kc = F32(1) / F32(13), F32(5) / F32(13)
    acc = np.full((h - 2, w - 2, a.shape[2]), F32(0.5), dtype=F32)
    for dy in range(3):
        for dx in range(3):
            acc = (acc + (a[dy:dy + h - 2, dx:dx + w - 2].astype(F32) * (kc if dy == dx == 1 else k)).astype(F32)).astype(F32)
    out[1:h - 1, 1:w - 1] = np.clip(np.trunc(acc), 0, 255).astype(np.uint8)
    return out


def color_jitter(a, factors):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3
    f = [F32(v) for v in np.asarray(factors, dtype=np.float64)]
    b1 = blend(luma(a)[..., None], a, f[0])                                  # Color: towards the grey image
    b2 = blend(0, b1, f[1])                                                  # Brightness: towards black
    n = a.shape[0] * a.shape[1]
    m = (2 * int(luma(b2).astype(np.int64).sum()) + n) // (2 * n)            # Contrast: towards int(mean(L) + 0.5)
    b3 = blend(m, b2, f[2])
    return blend(smooth(b3), b3, f[3])                                       # Sharpness: towards the smoothed image


class NumpyJitter(object):
    """A stand-in for transforms.color_jitter as the dataset's `jitter`: this restatement on host arrays; remembers its calls."""

    def __init__(self):
        self.calls = []

    def __call__(self, arrays, factors):
        self.calls.append(([np.array(a) for a in arrays], np.array(factors)))
        return [color_jitter(a, f) for a, f in zip(arrays, factors)]
