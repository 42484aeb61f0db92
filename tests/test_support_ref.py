"""CPU: tests/support_ref.py — the restatements the support-kernel tests (tests/test_gpu_support_kernels.py) compare with — pinned
to independent statements of the same operations: float64 autograd, torch.optim.SGD, a stable sort, the FCOS post-processing
restatement of oracle/hotpath_ref.py, and the struct layouts the header documents."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr
import support_ref as sr
from oracle import hotpath_ref as orc
from oracle import launch_replay as lr


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def autograd_dx(x_shape_nchw, w, dy_nchw, stride, pad):
    x = torch.zeros(x_shape_nchw, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, stride=stride, padding=pad).backward(dy_nchw)
    return x.grad


DGRAD_CASES = [
    # n, cin, h, w, cout, k, stride, pad
    (2, 8, 9, 11, 12, 3, 2, 1),
    (1, 8, 8, 6, 16, 3, 2, 1),       # even sizes: the last input row / column gets no gradient from a 3x3 / 2 / 1 conv
    (2, 4, 5, 7, 8, 1, 2, 0),
    (1, 8, 7, 5, 4, 3, 1, 1),
]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_dgrad_naive_equals_float64_autograd(case):
    n, cin, h, w, cout, k, st, p = case
    ho, wo = (h + 2 * p - k) // st + 1, (w + 2 * p - k) // st + 1
    wt, dy = rnd(cout, cin, k, k, seed=1), rnd(n, cout + 4, ho, wo, seed=2)        # dy stores more channels than cout
    ref = autograd_dx((n, cin, h, w), wt, dy[:, :cout].contiguous(), st, p)
    got = sr.dgrad_naive(nhwc(dy), wt, (n, h, w, cin), st, p)
    assert got.dtype == torch.float64
    torch.testing.assert_close(nchw(got), ref, rtol=1e-12, atol=1e-12)
    # the order: mask first, addend after (a masked-out position still receives the addend)
    mask, add = rnd(n, cin, h, w, seed=3), rnd(n, cin, h, w, seed=4)
    both = sr.dgrad_naive(nhwc(dy), wt, (n, h, w, cin), st, p, mask=nhwc(mask), addend=nhwc(add))
    torch.testing.assert_close(nchw(both), torch.where(mask > 0, ref, torch.zeros_like(ref)) + add, rtol=1e-12, atol=1e-12)
    other = torch.where(mask > 0, ref + add, torch.zeros_like(ref))
    assert float((nchw(both) - other).abs().max()) > 1e-3


PACK_SHAPES = [(6, 10, 3, 3), (16, 8, 1, 1), (4, 12, 7, 7)]     # cout, cin, r, s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", PACK_SHAPES)
def test_pack_references_round_trip_through_unpack_weight(shape, dtype):
    cout, cin, r, s = shape
    w_oihw = rnd(cout, cin, r, s, seed=1).float()
    w_orsi = w_oihw.permute(0, 2, 3, 1).contiguous()
    scale = rnd(cout, seed=2).float()
    for sc in (None, scale):
        want = w_oihw if sc is None else w_oihw * sc.view(-1, 1, 1, 1)
        want = want.to(dtype).float()
        rows, kpad = cout + 3, cin + 6
        fw = sr.pack_fwd(w_orsi, sc, rows, kpad, dtype)
        assert fw.shape == (rows, r, s, kpad) and fw.dtype == dtype
        back = lr.unpack_weight(fw, cout)                                  # [cout, kpad, r, s]
        assert torch.equal(back[:, :cin], want)
        assert float(fw[cout:].float().abs().max()) == 0.0 and float(fw[..., cin:].float().abs().max()) == 0.0
        rows, kpad = cin + 5, cout + 2
        dg = sr.pack_dgrad(w_orsi, sc, rows, kpad, dtype)
        assert dg.shape == (rows, r, s, kpad) and dg.dtype == dtype
        back = lr.unpack_weight(dg, cin)                                   # [cin, kpad, r, s]: Wd[ci][co][r'][s'] = w[co][ci][R-1-r'][S-1-s']
        assert torch.equal(back[:, :cout], want.flip(2, 3).transpose(0, 1))
        assert float(dg[cin:].float().abs().max()) == 0.0 and float(dg[..., cout:].float().abs().max()) == 0.0


@pytest.mark.parametrize("k,pad", [(3, 1), (1, 0), (3, 0), (7, 3)])
def test_dgrad_pack_used_as_conv_weights_reproduces_the_input_gradient(k, pad):
    """The data gradient of a stride-1 conv = a forward conv of dy with the data-gradient pack and pad' = r - 1 - pad."""
    n, cin, h, w, cout = 2, 6, 9, 8, 10
    ho, wo = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    wt, dy = rnd(cout, cin, k, k, seed=1).float(), rnd(n, cout, ho, wo, seed=2)
    scale = rnd(cout, seed=3).float()
    ref = autograd_dx((n, cin, h, w), (wt * scale.view(-1, 1, 1, 1)).double(), dy, 1, pad)
    wd = sr.pack_dgrad(wt.permute(0, 2, 3, 1).contiguous(), scale, cin + 2, cout + 6, torch.float32)
    got = cr.conv_fwd(nhwc(dy), lr.unpack_weight(wd, cin)[:, :cout], stride=1, pad=k - 1 - pad)
    assert got.shape == (n, h, w, cin)
    torch.testing.assert_close(nchw(got), ref, rtol=1e-12, atol=1e-12)


def test_pack_multi_reference_places_every_entry_and_nothing_else():
    entries = [dict(src_off=3, dst_off=8, scale_off=-1, cout=2, cin=3, r=1, s=1, rows=3, kpad=4, n_blocks=1),
               dict(src_off=9, dst_off=24, scale_off=1, cout=3, cin=2, r=1, s=2, rows=4, kpad=4, n_blocks=2)]
    src, scales = rnd(32, seed=1).float(), rnd(8, seed=2).float()
    dst = torch.full((64,), 7.0)
    out = sr.pack_multi(entries, src, scales, dst, dgrad=0)
    assert torch.equal(out[8:20].view(3, 1, 1, 4), sr.pack_fwd(src[3:9].view(2, 1, 1, 3), None, 3, 4, torch.float32))
    assert torch.equal(out[24:56].view(4, 1, 2, 4), sr.pack_fwd(src[9:21].view(3, 1, 2, 2), scales[1:4], 4, 4, torch.float32))
    untouched = torch.ones(64, dtype=torch.bool)
    untouched[8:20] = False
    untouched[24:56] = False
    assert bool((out[untouched] == 7.0).all()) and torch.equal(dst, torch.full((64,), 7.0))


def test_tables_follow_the_documented_struct_layouts():
    """The header: PackEntry { int64 src_off, dst_off, scale_off; int32 cout, cin, r, s, rows, kpad, first_block, n_blocks } (56 bytes),
    SgdEntry { int64 off, numel; float lr_mult, wd; int32 first_block, n_blocks } (32), SgdPackEntry { ... ; int64 dst_off, scale_off;
    int32 cin, rs, kpad, pad } (64)."""
    i8, i4, f4 = "<i8", "<i4", "<f4"
    pe = np.dtype([(k, i8) for k in ("src_off", "dst_off", "scale_off")] +
                  [(k, i4) for k in ("cout", "cin", "r", "s", "rows", "kpad", "first_block", "n_blocks")])
    se = np.dtype([("off", i8), ("numel", i8), ("lr_mult", f4), ("wd", f4), ("first_block", i4), ("n_blocks", i4)])
    spe = np.dtype(se.descr + [("dst_off", i8), ("scale_off", i8), ("cin", i4), ("rs", i4), ("kpad", i4), ("pad", i4)])
    assert (pe.itemsize, se.itemsize, spe.itemsize) == (56, 32, 64)
    ents = [dict(src_off=5, dst_off=64, scale_off=-1, cout=2, cin=3, r=1, s=1, rows=16, kpad=4, n_blocks=2),
            dict(src_off=11, dst_off=128, scale_off=7, cout=4, cin=8, r=3, s=3, rows=16, kpad=16, n_blocks=3)]
    t, owner, nb = sr.pack_table(ents)
    a = np.frombuffer(t.numpy().tobytes(), dtype=pe)
    assert nb == 5 and owner.tolist() == [0, 0, 1, 1, 1] and owner.dtype == torch.int32
    assert a["src_off"].tolist() == [5, 11] and a["scale_off"].tolist() == [-1, 7] and a["kpad"].tolist() == [4, 16]
    assert a["first_block"].tolist() == [0, 2] and a["n_blocks"].tolist() == [2, 3] and a["rows"].tolist() == [16, 16]
    ents = [dict(off=1, numel=5, lr_mult=2.0, wd=0.0, n_blocks=1),
            dict(off=8, numel=24, lr_mult=1.0, wd=0.5, n_blocks=3, dst_off=32, scale_off=-1, cin=4, rs=3, kpad=8)]
    t, owner, nb = sr.sgd_table(ents)
    a = np.frombuffer(t.numpy().tobytes(), dtype=se)
    assert nb == 4 and owner.tolist() == [0, 1, 1, 1]
    assert a["off"].tolist() == [1, 8] and a["numel"].tolist() == [5, 24] and a["lr_mult"].tolist() == [2.0, 1.0]
    assert a["wd"].tolist() == [0.0, 0.5] and a["first_block"].tolist() == [0, 1] and a["n_blocks"].tolist() == [1, 3]
    t, owner, nb = sr.sgd_pack_table(ents)
    a = np.frombuffer(t.numpy().tobytes(), dtype=spe)
    assert a["off"].tolist() == [1, 8] and a["dst_off"].tolist() == [-1, 32] and a["scale_off"].tolist() == [-1, -1]
    assert a["cin"].tolist() == [0, 4] and a["rs"].tolist() == [0, 3] and a["kpad"].tolist() == [0, 8] and a["n_blocks"].tolist() == [1, 3]


def test_sgd_reference_equals_torch_optim_sgd():
    lr_, mom = 0.05, 0.9
    entries = [dict(off=0, numel=1, lr_mult=2.0, wd=0.0, n_blocks=1), dict(off=1, numel=5, lr_mult=1.0, wd=1e-2, n_blocks=1),
               dict(off=9, numel=12, lr_mult=0.5, wd=1e-4, n_blocks=2)]
    total = 24
    p0 = rnd(total, seed=1)
    grads = [rnd(total, seed=10 + k) for k in range(3)]
    params = [torch.nn.Parameter(p0[e["off"]:e["off"] + e["numel"]].clone()) for e in entries]
    opt = torch.optim.SGD([{"params": [q], "lr": sr._f32(lr_) * sr._f32(e["lr_mult"]), "weight_decay": sr._f32(e["wd"])}
                           for q, e in zip(params, entries)], lr=lr_, momentum=sr._f32(mom))
    for k in range(3):
        for q, e in zip(params, entries):
            q.grad = grads[k][e["off"]:e["off"] + e["numel"]].clone()
        opt.step()
        p, buf = sr.sgd_steps(entries, p0, grads, lr_, mom, n_steps=k + 1)
        for q, e in zip(params, entries):
            sl = slice(e["off"], e["off"] + e["numel"])
            torch.testing.assert_close(p[sl], q.detach(), rtol=1e-13, atol=1e-13)
            torch.testing.assert_close(buf[sl], opt.state[q]["momentum_buffer"], rtol=1e-13, atol=1e-13)
    gaps = torch.ones(total, dtype=torch.bool)
    for e in entries:
        gaps[e["off"]:e["off"] + e["numel"]] = False
    assert torch.equal(p[gaps], p0[gaps])


@pytest.mark.parametrize("cnt,topn", [(1, 1), (37, 5), (300, 100), (300, 300), (300, 305), (1100, 1)])
def test_level_topk_reference_equals_a_stable_sort(cnt, topn):
    g = torch.Generator().manual_seed(cnt + topn)
    total, lo = cnt + 50, 13
    keys = torch.randint(0, 6, (2, total), generator=g).float() / 4      # heavy ties
    keys[torch.rand(2, total, generator=g) < 0.1] = -1.0                 # already dropped
    got = sr.level_topk(keys, lo, cnt, topn)
    for img in range(2):
        k = keys[img, lo:lo + cnt]
        order = torch.sort(k, descending=True, stable=True).indices      # (key descending, index ascending)
        want = torch.full_like(k, -1.0)
        keep = order[:topn]
        want[keep] = k[keep]
        want[k < 0] = -1.0
        assert torch.equal(got[img, lo:lo + cnt], want)
    outside = torch.ones(total, dtype=torch.bool)
    outside[lo:lo + cnt] = False
    assert torch.equal(got[:, outside], keys[:, outside])


def test_score_decode_reference_equals_the_fcos_postprocessing_restatement():
    """oracle.hotpath_ref.fcos_postprocess (fcos/inference.py:46-137) with the top-n cut, NMS and the post-NMS cut switched off keeps
    every candidate (sigmoid(logit) > 0) of every level in location order: the same scores and clipped boxes."""
    g = torch.Generator().manual_seed(5)
    level_hw, strides, n = [(5, 7), (3, 4)], orc.FPN_STRIDES[:2], 2
    sizes = [(33, 50), (40, 41)]                                          # true (height, width) per image
    logits = [torch.randn(n, 1, h, w, generator=g) * 3 for h, w in level_hw]
    ctrs = [torch.randn(n, 1, h, w, generator=g) * 3 for h, w in level_hw]
    regs = [torch.rand(n, 4, h, w, generator=g) * 40 for h, w in level_hw]
    logits[0][0, 0, 1, 2] = -200.0                                        # the sigmoid underflows: not a candidate
    logits[1][1, 0, 2, 3] = -200.0
    want = orc.fcos_postprocess(logits, regs, ctrs, sizes, pre_nms_top_n=10 ** 6, post_nms_top_n=0, nms_thresh=2.0)
    per_image = [([], []) for _ in range(n)]
    n_dropped = 0
    for lg, ct, rg, st in zip(logits, ctrs, regs, strides):
        cc = torch.cat([nhwc(lg), nhwc(ct), torch.zeros_like(nhwc(lg))], -1)        # a wider pixel stride than the two values read
        img_hw = torch.tensor(sizes, dtype=torch.float32)
        scores, dropped, boxes = sr.score_decode(cc, nhwc(rg), st, 0.0, 0.0, img_hw=img_hw)
        assert scores.dtype == torch.float64 and boxes.dtype == torch.float32
        assert bool((scores[dropped] == -1.0).all())
        n_dropped += int(dropped.sum())
        for i in range(n):
            per_image[i][0].append(boxes[i][~dropped[i]])
            per_image[i][1].append(scores[i][~dropped[i]])
    assert n_dropped == 2
    for i in range(n):
        b, s = torch.cat(per_image[i][0]), torch.cat(per_image[i][1])
        assert torch.equal(b, want[i][0])
        torch.testing.assert_close(s.float(), want[i][1], rtol=1e-5, atol=1e-7)
    # one size for the whole batch = the same size given per image
    a = sr.score_decode(cc, nhwc(rg), st, 33.0, 50.0)
    b = sr.score_decode(cc, nhwc(rg), st, 0.0, 0.0, img_hw=torch.tensor([[33.0, 50.0]] * n))
    assert torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])


def test_small_references():
    x = rnd(2, 3, 4, 16, seed=1).float()                                   # NHWC, pixel stride 16
    assert torch.equal(sr.nhwc_to_nchw(x, c0=3, c=5), x[..., 3:8].permute(0, 3, 1, 2))
    y = rnd(2, 5, 3, 7, seed=2).float()
    assert torch.equal(sr.nchw_to_nhwc(y, torch.bfloat16), y.permute(0, 2, 3, 1).bfloat16())
    assert torch.equal(sr.nhwc_to_nchw(sr.nchw_to_nhwc(y.bfloat16().float(), torch.bfloat16)), y.bfloat16().float())
    dy = rnd(7, 8, seed=3)
    torch.testing.assert_close(sr.bias_grad(dy, 5, torch.ones(5)), dy[:, :5].sum(0) + 1.0, rtol=1e-14, atol=1e-14)
    inner, prev = rnd(2, 6, 4, 3, seed=4), rnd(2, 3, 2, 3, seed=5)
    up = F.interpolate(nchw(prev), scale_factor=2, mode="nearest").requires_grad_(False)
    t = nchw(prev).clone().requires_grad_(True)
    (F.interpolate(t, scale_factor=2, mode="nearest") * nchw(inner)).sum().backward()       # d/dt = the 2 x 2 sums of inner
    torch.testing.assert_close(nchw(sr.upsample2x_bwd(inner, prev)), t.grad + nchw(prev), rtol=1e-13, atol=1e-13)
    assert up.shape[-2:] == inner.shape[1:3]
    dw, sc, g0 = rnd(5, 3, 3, 7, seed=6).float(), rnd(5, seed=7).float(), rnd(5, 7, 3, 3, seed=8).float()
    assert torch.equal(sr.unpack_wgrad(dw, None), dw.permute(0, 3, 1, 2))
    assert torch.equal(sr.unpack_wgrad(dw, sc, g0), g0 + dw.permute(0, 3, 1, 2) * sc.view(-1, 1, 1, 1))
    d0, raw, scl = rnd(6, seed=9).float(), rnd(6, seed=10).float(), rnd(6, seed=11).float().abs() + 0.5
    out = sr.finalize_scales(d0, raw, scl, 5)
    torch.testing.assert_close(out[:5], d0[:5].double() + raw[:5].double() / scl[:5].double(), rtol=0, atol=0)
    assert float(out[5]) == float(d0[5])


def test_upsample2x_bwd_wrapper_refuses_an_odd_sized_gradient():
    """The kernel reads `inner` as exactly [n][2h][2w][c]: a halved odd size would address the wrong pixels without any error."""
    from oneshotdet_amd import ops
    for shape in [(1, 5, 4, 8), (1, 4, 5, 8), (2, 7, 3, 8)]:
        with pytest.raises(ValueError):
            ops.upsample2x_bwd(torch.zeros(shape))
