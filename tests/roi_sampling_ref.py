"""One plain reference for the bilinear ROI sampling family (osd_roialign_fwd / _bwd, osd_query_pool_levels / _bwd,
osd_roi_pool_levels / _sweep / _bwd), and the inputs of tests/test_roi_sampling_ref.py (CPU) and tests/test_gpu_roi_sampling.py.

Geometry (`geometry`): csrc/cuda/ROIAlign_cuda.cu:11-122 / csrc/cpu/ROIAlign_cpu.cpp:44-219 in np.float32 in the reference's
operation order, as oracle/hotpath_ref.py roi_align + _bilinear_taps: per ROI and cell the live samples (iy, ix, 4 x (row, col,
weight)) and the sample count.  With ft=np.float64 the same statements run in float64 (the exactness check of the exact cases).
Values (`forward`, `backward`): float64 sums over that tap list, with the sums of magnitudes the derived bounds need:
    forward   |got - ref| <= (n + 2) x 2^-24 x S / count     n = 4 x live samples of the cell: n product roundings, n additions
                                                              (3 inside a sample's expression + 1 into the cell sum) of partial sums
                                                              <= S, one division; a fused multiply-add only removes roundings
    backward  |got - ref| <= (m + 2) x 2^-24 x A              m contributions to the element: <= 3 roundings each (dy / shots, x hy,
                                                              x hx; dy / count is exact: the counts of the exact cases are powers of
                                                              two) and m - 1 atomic additions of partial sums <= A
Loops over ROI, cell and sample are explicit; only the channels are vectorised."""
import math
from collections import namedtuple

import numpy as np
import torch

from oracle import box_head_ref as obh

U = 2.0 ** -24                     # unit roundoff of float32
Geometry = namedtuple("Geometry", "image gh gw count ys xs cells inter")
Forward = namedtuple("Forward", "y S n count")
Backward = namedtuple("Backward", "gx A m")
HIT_NAMES = ("on_minus_one", "on_size", "outside", "on_pixel", "on_last")


def _f64(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def _taps(y, x, height, width, ft):
    """ROIAlign_cpu.cpp:44-104 / ROIAlign_cuda.cu:11-60, one sample: None (skipped) or 4 x (row, col, weight)."""
    if y < -1.0 or y > height or x < -1.0 or x > width:
        return None
    y, x = max(y, ft(0.0)), max(x, ft(0.0))
    y_low, x_low = int(y), int(x)
    if y_low >= height - 1:
        y_high = y_low = height - 1
        y = ft(y_low)
    else:
        y_high = y_low + 1
    if x_low >= width - 1:
        x_high = x_low = width - 1
        x = ft(x_low)
    else:
        x_high = x_low + 1
    ly, lx = ft(y) - ft(y_low), ft(x) - ft(x_low)
    hy, hx = ft(1.0) - ly, ft(1.0) - lx
    return ((y_low, x_low, hy * hx), (y_low, x_high, hy * lx), (y_high, x_low, ly * hx), (y_high, x_high, ly * lx))


def geometry(roi, scale, height, width, ph, pw, sampling, ft=np.float32):
    """roi = (image, x1, y1, x2, y2) float32.  -> Geometry: ys [ph][gh] / xs [pw][gw] the sample positions, cells[(i, j)] = the live
    samples [(iy, ix, taps)], inter = every intermediate (the exactness check compares them between float32 and float64)."""
    r = np.asarray(roi, np.float32)
    s = ft(np.float32(scale))
    rsw, rsh, rew, reh = ft(r[1]) * s, ft(r[2]) * s, ft(r[3]) * s, ft(r[4]) * s
    roi_w, roi_h = max(rew - rsw, ft(1.0)), max(reh - rsh, ft(1.0))
    bin_h, bin_w = ft(roi_h) / ft(ph), ft(roi_w) / ft(pw)
    gh = sampling if sampling > 0 else int(math.ceil(ft(roi_h) / ft(ph)))
    gw = sampling if sampling > 0 else int(math.ceil(ft(roi_w) / ft(pw)))
    inter = [rsw, rsh, rew, reh, roi_w, roi_h, bin_h, bin_w]
    ys = [[None] * gh for _ in range(ph)]
    xs = [[None] * gw for _ in range(pw)]
    for i in range(ph):
        for iy in range(gh):
            a, b = ft(i) * bin_h, ft(iy + 0.5) * bin_h
            ys[i][iy] = rsh + a + b / ft(gh)
            inter += [a, b, rsh + a, b / ft(gh)]
    for j in range(pw):
        for ix in range(gw):
            a, b = ft(j) * bin_w, ft(ix + 0.5) * bin_w
            xs[j][ix] = rsw + a + b / ft(gw)
            inter += [a, b, rsw + a, b / ft(gw)]
    cells = {}
    for i in range(ph):
        for j in range(pw):
            live = []
            for iy in range(gh):
                for ix in range(gw):
                    t = _taps(ys[i][iy], xs[j][ix], height, width, ft)
                    if t is not None:
                        live.append((iy, ix, t))
                        inter += [w for (_, _, w) in t]
            cells[(i, j)] = live
    return Geometry(int(r[0]), gh, gw, gh * gw, ys, xs, cells, [float(v) for v in inter] + [float(v) for row in ys + xs for v in row])


def is_exact(roi, scale, height, width, ph, pw, sampling):
    """Every intermediate of the float32 geometry equals the same statement in float64, bit for bit, and so do the taps."""
    a = geometry(roi, scale, height, width, ph, pw, sampling, np.float32)
    b = geometry(roi, scale, height, width, ph, pw, sampling, np.float64)
    def pixels(g):
        return {k: [(iy, ix, [(r, c) for r, c, _ in t]) for iy, ix, t in live] for k, live in g.cells.items()}
    return (a.gh, a.gw) == (b.gh, b.gw) and a.inter == b.inter and pixels(a) == pixels(b)


def forward(x, rois, scale, ph, pw, sampling):
    """x [B, H, W, C] (NHWC), rois [R, 5] -> Forward(y, S [R, ph, pw, C] float64, n [R, ph, pw] tap products, count [R])."""
    x = _f64(x)
    rois = np.asarray(_f64(rois), np.float32)
    _, H, W, C = x.shape
    R = len(rois)
    y, S = np.zeros((R, ph, pw, C)), np.zeros((R, ph, pw, C))
    n, count = np.zeros((R, ph, pw), np.int64), np.zeros((R,), np.int64)
    for r in range(R):
        g = geometry(rois[r], scale, H, W, ph, pw, sampling)
        count[r] = g.count
        for (i, j), live in g.cells.items():
            for (_, _, taps) in live:
                for (ty, tx, wgt) in taps:
                    term = float(wgt) * x[g.image, ty, tx]
                    y[r, i, j] += term
                    S[r, i, j] += np.abs(term)
                n[r, i, j] += 4
        y[r] /= g.count
    return Forward(y, S, n, count)


def forward_bound(f):
    """(n + 2) x 2^-24 x S / count, per element."""
    return (f.n[..., None] + 2) * U * f.S / f.count[:, None, None, None]


def backward(gy, rois, x_shape, scale, ph, pw, sampling):
    """gy [R, ph, pw, C], x_shape (B, H, W, C) -> Backward(gx, A [B, H, W, C] float64, m [B, H, W] contributions per element)."""
    gy = _f64(gy)
    rois = np.asarray(_f64(rois), np.float32)
    B, H, W, C = x_shape
    gx, A, m = np.zeros((B, H, W, C)), np.zeros((B, H, W, C)), np.zeros((B, H, W), np.int64)
    for r in range(len(rois)):
        g = geometry(rois[r], scale, H, W, ph, pw, sampling)
        for (i, j), live in g.cells.items():
            top = gy[r, i, j] / g.count
            for (_, _, taps) in live:
                for (ty, tx, wgt) in taps:
                    term = top * float(wgt)
                    gx[g.image, ty, tx] += term
                    A[g.image, ty, tx] += np.abs(term)
                    m[g.image, ty, tx] += 1
    return Backward(gx, A, m)


def backward_bound(b):
    """(m + 2) x 2^-24 x A, per element; 0 where nothing contributes."""
    return np.where(b.m[..., None] > 0, (b.m[..., None] + 2) * U * b.A, 0.0)


# ---- compositions
def query_pool(feats, rois, scales, batch, sampling):
    """1 x 1 ROIAlign of every query's box + the mean over the shots of a target image, per level -> [(y [batch, C], bound)].
    bound: each shot's cell within forward_bound, then `shots` additions and one division on sums <= sum of S / count."""
    out = []
    for x, sc in zip(feats, scales):
        f = forward(x, rois, sc, 1, 1, sampling)
        R, C = f.y.shape[0], f.y.shape[-1]
        shots = R // batch
        y = f.y.reshape(batch, shots, C).mean(1)
        mag = (f.S.reshape(R, C) / f.count[:, None]).reshape(batch, shots, C).sum(1) / shots
        bound = forward_bound(f).reshape(batch, shots, C).sum(1) / shots + (shots + 1) * U * mag
        out.append((y, bound))
    return out


def query_pool_bwd(dqs, rois, shapes, scales, shots, sampling):
    """dqs[l] [batch, C] -> per level Backward of gy[r] = dq[r // shots] / shots through the 1 x 1 ROIAlign."""
    out = []
    for dq, sh, sc in zip(dqs, shapes, scales):
        gy = np.repeat(_f64(dq) / shots, shots, axis=0)[:, None, None, :]
        out.append(backward(gy, rois, tuple(sh), sc, 1, 1, sampling))
    return out


def levels_of(boxes, counts=None):
    """boxes [N, R, 4] -> int64 [N * R]: oracle.box_head_ref.map_levels, -1 past counts[image]."""
    b = torch.as_tensor(np.asarray(boxes, np.float32))
    n, r, _ = b.shape
    lv = obh.map_levels(b.reshape(-1, 4)).numpy().copy()
    if counts is not None:
        for i in range(n):
            lv[i * r + int(counts[i]):(i + 1) * r] = -1
    return lv


def _level_rois(boxes, counts, sets_per_image):
    b = np.asarray(boxes, np.float32)
    n, r, _ = b.shape
    lv = levels_of(b, counts)
    rois = np.concatenate([np.repeat(np.arange(n) // sets_per_image, r)[:, None].astype(np.float32), b.reshape(-1, 4)], 1)
    return lv, rois


def pool_levels(feats, scales, boxes, counts, pool, sampling, sets_per_image=1):
    """The multi-level pooler (modeling/poolers.py:93-124): feats NHWC per level, boxes [N, R, 4]; ROI set j reads image
    j // sets_per_image.  -> (Forward over the N * R rows (rows past counts zero), levels [N * R])."""
    lv, rois = _level_rois(boxes, counts, sets_per_image)
    C = feats[0].shape[-1]
    T = len(rois)
    y, S = np.zeros((T, pool, pool, C)), np.zeros((T, pool, pool, C))
    n, count = np.zeros((T, pool, pool), np.int64), np.ones((T,), np.int64)
    for l, (x, sc) in enumerate(zip(feats, scales)):
        idx = np.nonzero(lv == l)[0]
        if len(idx):
            f = forward(x, rois[idx], sc, pool, pool, sampling)
            y[idx], S[idx], n[idx], count[idx] = f.y, f.S, f.n, f.count
    return Forward(y, S, n, count), lv


def pool_levels_bwd(dy, shapes, scales, boxes, counts, pool, sampling):
    """dy [N * R, pool, pool, C], shapes [(h, w)] per level -> per level Backward on [N, h, w, C]."""
    lv, rois = _level_rois(boxes, counts, 1)
    dy = _f64(dy)
    n_img, C = np.asarray(boxes).shape[0], dy.shape[-1]
    out = []
    for l, ((h, w), sc) in enumerate(zip(shapes, scales)):
        idx = np.nonzero(lv == l)[0]
        out.append(backward(dy[idx], rois[idx], (n_img, h, w, C), sc, pool, pool, sampling))
    return out


# ---- where the samples lie
def _positions(rois, scale, height, width, ph, pw, sampling):
    for roi in np.asarray(rois, np.float32):
        g = geometry(roi, scale, height, width, ph, pw, sampling)
        yield [float(v) for row in g.ys for v in row], height
        yield [float(v) for row in g.xs for v in row], width


def threshold_hits(rois, scale, height, width, ph, pw, sampling):
    """Per-axis sample positions of all ROIs, counted: exactly on -1, exactly on the map size, strictly outside [-1, size],
    exactly on an integer pixel 0 .. size - 1, and on the last row / column (>= size - 1, inside: the two taps collapse)."""
    hits = dict.fromkeys(HIT_NAMES, 0)
    for pos, size in _positions(rois, scale, height, width, ph, pw, sampling):
        for v in pos:
            hits["on_minus_one"] += v == -1.0
            hits["on_size"] += v == size
            hits["outside"] += v < -1.0 or v > size
            hits["on_pixel"] += 0 <= v <= size - 1 and v == int(v)
            hits["on_last"] += size - 1 <= v <= size
    return hits


def min_threshold_distance(rois, scale, height, width, ph, pw, sampling):
    """The smallest distance of any sample position from -1 and from the map size."""
    d = float("inf")
    for pos, size in _positions(rois, scale, height, width, ph, pw, sampling):
        for v in pos:
            d = min(d, abs(v + 1.0), abs(v - size))
    return d


def add_hits(a, b):
    return {k: a[k] + b[k] for k in HIT_NAMES}


# ---- the inputs of the GPU tests (built here so that the CPU test can assert their conditions)
def data(shape, seed, bf16=False):
    """N(0, 1) values, NHWC float32 torch; bf16: rounded to bfloat16 (what a bf16 kernel is handed)."""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    return t.bfloat16().float() if bf16 else t


def _grid(b, sampling):
    return sampling if sampling > 0 else int(math.ceil(b))


def _start(kind, size, P, b, gg):
    """Start of the ROI on one axis, in map units, so that its samples start + b x (p + (i + .5) / gg) lie as `kind` says."""
    off, eps = b / (2 * gg), 2.0 ** -10
    return {"low": -1 - off,                         # first sample exactly on -1 (kept, clamped to pixel 0)
            "below": -1 - off - eps,                 # first sample 2^-10 below -1 (skipped)
            "high": size - P * b + off,              # last sample exactly on the map size (kept, on the last row)
            "above": size - P * b + off + eps,       # last sample 2^-10 above the map size (skipped)
            "int": 1 - off,                          # first sample on pixel 1: the samples with an integer spacing stay on pixels
            "pair": 1.25 - off,                      # samples .25 / .5 apart: the two of a cell share a pixel pair
            "inside": 0.375 - off,
            "outside": size + 2.0}[kind]             # every sample beyond the map


def exact_box(size_h, size_w, scale, ph, pw, sampling, ky, by, kx, bx):
    """(x1, y1, x2, y2) in image units of the ROI with bins (by, bx) map pixels and sample positions (ky, kx): dyadic throughout."""
    sy = _start(ky, size_h, ph, by, _grid(by, sampling))
    sx = _start(kx, size_w, pw, bx, _grid(bx, sampling))
    return [sx / scale, sy / scale, (sx + pw * bx) / scale, (sy + ph * by) / scale]


ROIALIGN_MAP = (2, 13, 11)        # images, rows, columns of the one map of the osd_roialign_fwd / _bwd cases
ROIALIGN_SCALE = 1.0 / 16
ROIALIGN_KINDS = [("low", 4, "low", 4), ("below", 4, "inside", 2), ("inside", 2, "below", 4), ("high", 4, "high", 1),
                  ("above", 1, "above", 4), ("int", 2, "int", 4), ("pair", 0.5, "pair", 1), ("high", 0.5, "low", 0.5),
                  ("low", 1, "high", 2), ("outside", 2, "inside", 2), ("inside", 1, "outside", 4), ("int", 1, "pair", 0.5)]
ROIALIGN_CLAIMS = HIT_NAMES       # every category, in every (pool, sampling) configuration
ROIALIGN_POOLS = [(1, 1), (7, 7), (3, 2)]


def exact_roialign_rois(ph, pw, sampling):
    """[R, 5] float32: ROIALIGN_KINDS alternating between the two images, a ROI wholly outside the map, the first and fourth ROI
    again on their own images (their gradients add up), and a degenerate ROI (x2 = x1, y2 = y1: roi_w / roi_h clamped to 1) where
    the clamped bin 1 / pool is a power of two on both axes (pool 1 x 1)."""
    _, h, w = ROIALIGN_MAP
    rois = [[i % 2] + exact_box(h, w, ROIALIGN_SCALE, ph, pw, sampling, *k) for i, k in enumerate(ROIALIGN_KINDS)]
    rois += [list(rois[0]), list(rois[3]), [1] + exact_box(h, w, ROIALIGN_SCALE, ph, pw, sampling, "outside", 1, "outside", 1)]
    if (ph, pw) == (1, 1):
        rois.append([0, 40.0, 72.0, 40.0, 72.0])
    return np.asarray(rois, np.float32)


POOL_SCALES = (0.125, 0.0625, 0.03125, 0.015625, 0.0078125)
POOL_SIZES = [(16, 15), (13, 11), (9, 10), (6, 7), (5, 4)]
POOL = 7
# per level four ROIs; their bins give a sqrt(area) that routes them to the level whose scale makes them dyadic:
# 56 x 2^l x sqrt(by x bx) + 1 lies in [112, 224) x 2^l for by x bx in {4, 8}; level 0 also takes smaller bins, level 4 larger ones
_POOL_KINDS = [("low", 4, "high", 1), ("high", 2, "low", 2), ("below", 1, "above", 4), ("int", 4, "pair", 1)]
_POOL_KINDS_0 = [("low", 4, "pair", 0.5), ("high", 0.5, "low", 0.5), ("below", 1, "above", 4), ("int", 4, "high", 1)]
_POOL_KINDS_4 = [("low", 4, "high", 1), ("high", 2, "low", 2), ("below", 1, "above", 4), ("low", 4, "high", 4)]


def exact_pool_boxes(sampling):
    """-> boxes [2, 12, 4] float32, counts [2] int32 (ragged: 12, 10), want [2 * 12] the level every live ROI is built for.
    22 live ROIs: four per level, one wholly outside its map, one duplicate (same image as its twin); the two dead rows are copies."""
    flat, want = [], []
    for l, (h, w) in enumerate(POOL_SIZES):
        for k in (_POOL_KINDS_0 if l == 0 else _POOL_KINDS_4 if l == 4 else _POOL_KINDS):
            flat.append(exact_box(h, w, POOL_SCALES[l], POOL, POOL, sampling, *k))
            want.append(l)
    flat.append(exact_box(*POOL_SIZES[1], POOL_SCALES[1], POOL, POOL, sampling, "outside", 2, "inside", 2))
    want.append(1)
    flat.insert(1, list(flat[0]))          # the duplicate: rows 0 and 1 of image 0
    want.insert(1, 0)
    flat += [list(flat[4]), list(flat[9])]
    want += [-1, -1]
    return np.asarray(flat, np.float32).reshape(2, 12, 4), np.asarray([12, 10], np.int32), np.asarray(want)


def pool_feats(c, seed, bf16=False, images=2):
    return [data((images, h, w, c), seed + l, bf16) for l, (h, w) in enumerate(POOL_SIZES)]


QUERY_SIZES = [(16, 16), (8, 8), (4, 5), (2, 3), (1, 1)]


def exact_query_rois(shots, sampling=2):
    """Whole-image query boxes (0, 0, w, h), 2 x shots of them.  sampling 2: any integer size is exact at every pooler scale for
    the 1 x 1 pooling; adaptive sampling: sizes whose grid ceil(size x scale) is a power of two at every scale (powers of two, and
    sizes <= 8, whose extent is clamped to one map pixel).  (128, 1) / (128, 3): degenerate, roi_h clamped to 1 at every scale.
    With more than one shot the last two of image 0 are the same box ON the same map (roi[0] equal: their gradients add up)."""
    r = 2 * shots
    sizes = ([(128, 128), (96, 64), (127, 67), (33, 128), (64, 100), (128, 1)] if sampling > 0 else
             [(128, 128), (64, 128), (128, 32), (16, 64), (7, 128), (128, 3)])
    rois = [[i, 0.0, 0.0, float(sizes[i % 6][0]), float(sizes[i % 6][1])] for i in range(r)]
    if shots > 1:
        rois[shots - 1] = list(rois[shots - 2])
    return np.asarray(rois, np.float32)


def random_pool_boxes(seed, n=2, r=12):
    """Random float boxes of every level (sqrt(area) from 16 to 2,500 pixels), some hanging over the borders of the 128-pixel image
    the POOL_SIZES maps stand for, one degenerate."""
    g = torch.Generator().manual_seed(seed)
    side = torch.exp(torch.rand(n, r, 1, generator=g) * math.log(2500.0 / 16)) * 16
    ar = torch.exp((torch.rand(n, r, 1, generator=g) - 0.5) * 1.2)
    wh = torch.cat([side * ar, side / ar], -1)
    ctr = torch.rand(n, r, 2, generator=g) * 160 - 16
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], -1)
    boxes[0, 0] = torch.tensor([37.3, 41.9, 37.3, 41.9])
    return boxes.numpy().astype(np.float32)


def random_rois(seed, r=14):
    """Random float ROIs on the ROIALIGN_MAP (scale 1 / 16: 208 x 176 pixels), some over the borders, one degenerate."""
    g = torch.Generator().manual_seed(seed)
    wh = torch.rand(r, 2, generator=g) * 150 + 4
    xy = torch.rand(r, 2, generator=g) * 220 - 40
    rois = torch.cat([(torch.arange(r) % 2).float()[:, None], xy, xy + wh], 1)
    rois[1, 3:] = rois[1, 1:3]
    return rois.numpy().astype(np.float32)


RANDOM_SEED = 1          # tests/test_roi_sampling_ref.py asserts min_threshold_distance >= 1e-3 for this seed, on the CPU


def pool_hits(boxes, counts, pool, sampling):
    """threshold_hits / min_threshold_distance of the live ROIs of a pooler input, each on its routed level."""
    lv, rois = _level_rois(boxes, counts, 1)
    hits, dist = dict.fromkeys(HIT_NAMES, 0), float("inf")
    for l, ((h, w), sc) in enumerate(zip(POOL_SIZES, POOL_SCALES)):
        sel = rois[lv == l]
        hits = add_hits(hits, threshold_hits(sel, sc, h, w, pool, pool, sampling))
        dist = min(dist, min_threshold_distance(sel, sc, h, w, pool, pool, sampling))
    return hits, dist


ROUTING_SIDES = (112, 224, 448, 896, 1792)


def routing_boxes():
    """[1, 12, 4]: squares whose sqrt(area) ('+1' area) is exactly 112 .. 1792 and one pixel less, one far below k_min, one far
    above k_max."""
    b = []
    for s in ROUTING_SIDES:
        b += [[8.0, 8.0, 8.0 + s - 1, 8.0 + s - 1], [8.0, 8.0, 8.0 + s - 2, 8.0 + s - 2]]
    b += [[20.0, 24.0, 23.0, 26.0], [-3000.0, -2000.0, 5000.0, 6000.0]]
    return np.asarray(b, np.float32)[None]
