"""CPU: tests/conv_ref.py — the float64 conv / weight-gradient reference and the bounds the kernel tests use — pinned.

(i) The reference equals float64 F.conv2d / autograd: stride 2, odd sizes, 1x1 / 3x3 / the stem's 7x8 taps, every residual mode,
mask, ReLU / exp-scale, relu_in, the two-source 1x1 conv, the FrozenBN scale of the weight gradient and the bias gradient.
(ii) The bounds accept what a correct kernel produces (fp32 accumulation in another order, one rounding) and reject the subtle
mistakes a kernel can make: one pixel dropped from the pixel axis, one 16-pixel block summed twice, a zeroed channel tail, a
residual epilogue that rounds twice."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("case", [
    # n, cin, h, w, cout, r, s, stride, pad
    (2, 8, 9, 11, 12, 3, 3, 1, 1),
    (1, 16, 13, 7, 8, 3, 3, 2, 1),
    (3, 8, 5, 6, 4, 1, 1, 1, 0),
    (2, 16, 11, 9, 8, 1, 1, 2, 0),
    (1, 4, 15, 22, 8, 7, 8, 2, 0),      # the stem's packed form: 7 filter rows x 8 pixels, stride 2, no padding
])
def test_forward_equals_float64_conv2d(case):
    n, cin, h, w, cout, r, s, st, p = case
    x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, r, s, seed=2), rnd(cout, seed=3)
    ref = F.conv2d(x, wt, b, stride=st, padding=p)
    y = cr.conv_fwd(nhwc(x), wt, b, stride=st, pad=p)
    assert y.dtype == torch.float64
    torch.testing.assert_close(nchw(y), ref, rtol=1e-12, atol=1e-12)
    # relu_in, exp-scale, ReLU
    torch.testing.assert_close(nchw(cr.conv_fwd(nhwc(x), wt, b, stride=st, pad=p, relu_in=True)), F.conv2d(F.relu(x), wt, b, stride=st, padding=p),
                               rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(nchw(cr.conv_fwd(nhwc(x), wt * 0.1, b * 0.1, stride=st, pad=p, act=cr.ACT_EXP_SCALE, act_scale=0.7)),
                               torch.exp(0.7 * F.conv2d(x, wt * 0.1, b * 0.1, stride=st, padding=p)), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(nchw(cr.conv_fwd(nhwc(x), wt, b, stride=st, pad=p, act=cr.ACT_RELU)), F.relu(ref), rtol=1e-12, atol=1e-12)
    # extra input channels past the weights' are ignored (the kernels' K padding), a crop of the output (the stem's out_hw)
    xp = torch.cat([x, rnd(n, 4, h, w, seed=9)], 1)
    torch.testing.assert_close(nchw(cr.conv_fwd(nhwc(xp), wt, b, stride=st, pad=p)), ref, rtol=1e-12, atol=1e-12)
    ho, wo = ref.shape[2], ref.shape[3]
    if ho > 1 and wo > 1:
        torch.testing.assert_close(nchw(cr.conv_fwd(nhwc(x), wt, b, stride=st, pad=p, out_hw=(ho - 1, wo - 1))), ref[:, :, :ho - 1, :wo - 1],
                                   rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("hw", [(10, 14), (9, 13)])
def test_forward_residual_modes_and_mask(hw):
    h, w = hw
    n, cin, cout = 2, 8, 12
    x, wt, b = rnd(n, cin, h, w, seed=1), rnd(cout, cin, 3, 3, seed=2), rnd(cout, seed=3)
    lin = F.conv2d(x, wt, b, padding=1)
    same, mask = rnd(n, cout + 4, h, w, seed=4), rnd(n, cout, h, w, seed=5)
    up = rnd(n, cout, (h + 1) // 2, (w + 1) // 2, seed=6)
    down = rnd(n, cout, 2 * h - 1, 2 * w - 1, seed=7)
    cases = [
        (dict(res=nhwc(same), res_mode=cr.RES_SAME), lin + same[:, :cout]),
        (dict(res=nhwc(up), res_mode=cr.RES_UP2X), lin + F.interpolate(up, scale_factor=2, mode="nearest")[:, :, :h, :w]),
        (dict(res=nhwc(down), res_mode=cr.RES_DOWN2X), lin + down[:, :, ::2, ::2]),
        (dict(res=nhwc(same), res_mode=cr.RES_SAME, mask=nhwc(mask), act=cr.ACT_RELU),
         F.relu(torch.where(mask > 0, lin + same[:, :cout], torch.zeros_like(lin)))),
    ]
    for kw, ref in cases:
        torch.testing.assert_close(nchw(cr.conv_fwd(nhwc(x), wt, b, pad=1, **kw)), ref, rtol=1e-12, atol=1e-12, msg=str(sorted(kw)))


@pytest.mark.parametrize("stride", [1, 2])
def test_forward_two_sources(stride):
    """conv3 + downsample of a bottleneck's first block as one 1x1 GEMM over two pixel sources."""
    n, c1, c2, cout, h, w = 2, 8, 16, 12, 5, 7
    x1 = rnd(n, c1, h, w, seed=1)
    x2 = rnd(n, c2, (h - 1) * stride + 1 + (stride - 1), (w - 1) * stride + 1, seed=2)
    w1, w2, b = rnd(cout, c1, 1, 1, seed=3), rnd(cout, c2, 1, 1, seed=4), rnd(cout, seed=5)
    ref = F.conv2d(x1, w1, b) + F.conv2d(x2, w2, stride=stride)
    y = cr.conv_fwd(nhwc(x1), w1, b, x2=nhwc(x2), w2=w2, x2_stride=stride, act=cr.ACT_RELU)
    torch.testing.assert_close(nchw(y), F.relu(ref), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case", [(2, 8, 9, 11, 12, 3, 1, 1), (1, 16, 13, 7, 8, 3, 2, 1), (3, 8, 5, 6, 4, 1, 1, 0), (2, 16, 11, 9, 8, 1, 2, 0)])
def test_weight_gradient_equals_float64_autograd(case):
    n, cin, h, w, cout, k, st, p = case
    x = rnd(n, cin, h, w, seed=1)
    wt = rnd(cout, cin, k, k, seed=2).requires_grad_(True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    scale = rnd(cout, seed=4).abs() + 0.5
    y = F.conv2d(x, wt * scale.view(-1, 1, 1, 1), b, stride=st, padding=p)
    dy = rnd(*y.shape, seed=3)
    (y * dy).sum().backward()
    dyp = torch.cat([dy, rnd(n, 4, y.shape[2], y.shape[3], seed=5)], 1)       # dy stored with more channels than cout
    dw, db = cr.conv_wgrad(nhwc(x), nhwc(dyp), k, k, st, p, cout, scale=scale, want_bias=True)
    torch.testing.assert_close(dw, wt.grad.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(db, b.grad, rtol=1e-12, atol=1e-12)


def _bf16(t):
    return t.to(torch.bfloat16).double()


def test_bounds_accept_fp32_accumulation_and_reject_kernel_mistakes_in_the_weight_gradient():
    """dW of a (2, 64, 20, 24) -> 64 3x3 conv on bf16-rounded operands (960 output pixels).  Accepted: the fp32 sum in two different
    orders.  Rejected: one pixel dropped, one 16-pixel block summed twice, the last 8 input channels zeroed, the last 4 output
    channels zeroed; and for db one dropped pixel."""
    n, cin, h, w, cout = 2, 64, 20, 24, 64
    x, dy = _bf16(rnd(n, h, w, cin, seed=1)), _bf16(rnd(n, h, w, cout, seed=2))
    ref, refb = cr.conv_wgrad(x, dy, 3, 3, 1, 1, cout, want_bias=True)
    xf, dyf = x.float(), dy.float()
    # fp32, autograd's order and the taps' GEMMs in fp32
    f32 = torch.nn.grad.conv2d_weight(nchw(xf), (cout, cin, 3, 3), nchw(dyf), padding=1).permute(0, 2, 3, 1)
    assert cr.check_accumulated(f32, ref)["ok"]
    f32b, f32bb = cr.conv_wgrad(xf, dyf, 3, 3, 1, 1, cout, want_bias=True)
    assert cr.check_accumulated(f32b.float(), ref)["ok"] and cr.check_accumulated(dyf.reshape(-1, cout).sum(0), refb)["ok"]
    # one pixel missing from the pixel axis (a tail the kernel does not reach)
    keep = torch.ones(n, h, w, 1, dtype=torch.float64)
    keep[1, h - 1, w - 1] = 0.0
    drop, dropb = cr.conv_wgrad(x, dy * keep, 3, 3, 1, 1, cout, want_bias=True)
    assert not cr.check_accumulated(drop, ref)["ok"]
    assert not cr.check_accumulated(dropb, refb)["ok"]
    # one 16-pixel block of the flattened pixel axis counted twice (a split boundary walked by two workgroups)
    m0 = 7 * w + 3
    flat = dy.reshape(-1, cout).clone()
    twice = torch.zeros_like(flat)
    twice[m0:m0 + 16] = flat[m0:m0 + 16]
    dup, _ = cr.conv_wgrad(x, (flat + twice).view(dy.shape), 3, 3, 1, 1, cout)
    assert not cr.check_accumulated(dup, ref)["ok"]
    # channel tails
    tail = ref.clone()
    tail[..., cin - 8:] = 0.0
    assert not cr.check_accumulated(tail, ref)["ok"]
    tail = ref.clone()
    tail[cout - 4:] = 0.0
    assert not cr.check_accumulated(tail, ref)["ok"]


def test_one_dropped_pixel_is_rejected_at_a_large_pixel_count():
    """M = 25,600 output pixels (the (8, 256, 50, 64) case of the kernel tests, scaled down in channels): 1/sqrt(M) of the signal
    is still far above the bound."""
    n, cin, h, w, cout = 8, 32, 50, 64, 32
    x, dy = _bf16(rnd(n, h, w, cin, seed=11)), _bf16(rnd(n, h, w, cout, seed=12))
    ref, _ = cr.conv_wgrad(x, dy, 3, 3, 1, 1, cout)
    f32 = torch.nn.grad.conv2d_weight(nchw(x.float()), (cout, cin, 3, 3), nchw(dy.float()), padding=1).permute(0, 2, 3, 1)
    ok = cr.check_accumulated(f32, ref)
    assert ok["ok"] and ok["err"] < 1e-5, ok
    keep = torch.ones(n, h, w, 1, dtype=torch.float64)
    keep[5, 17, 40] = 0.0
    drop, _ = cr.conv_wgrad(x, dy * keep, 3, 3, 1, 1, cout)
    bad = cr.check_accumulated(drop, ref)
    assert not bad["ok"] and bad["err"] > 10 * cr.ACC_TOL, bad


def test_bounds_accept_one_rounding_and_reject_forward_kernel_mistakes():
    """bf16 forward conv + bias + residual + ReLU on bf16 operands (K = 576).  Accepted: fp32 accumulation + one rounding.  Rejected:
    the residual added after a bf16 store of the conv (two roundings), the bias added in bf16, one pixel of the output left as the
    conv of a dropped input pixel, a zeroed channel tail; fp32: a dropped tap row."""
    n, cin, h, w, cout = 2, 64, 12, 16, 64
    x, wt = _bf16(rnd(n, h, w, cin, seed=1)), _bf16(rnd(cout, cin, 3, 3, seed=2) / 24)
    b, res = rnd(cout, seed=3).float().double(), _bf16(rnd(n, h, w, cout, seed=4))
    ref = cr.conv_fwd(x, wt, b, pad=1, res=res, res_mode=cr.RES_SAME, act=cr.ACT_RELU)
    # a correct kernel: fp32 accumulate, fp32 epilogue, one rounding
    acc = nhwc(F.conv2d(nchw(x.float()), wt.float(), b.float(), padding=1))
    good = F.relu(acc + res.float()).to(torch.bfloat16)
    r = cr.check_output(good, ref)
    assert r["ok"], r
    # the residual added after the conv's bf16 store
    twice = F.relu(acc.to(torch.bfloat16).float() + res.float()).to(torch.bfloat16)
    r = cr.check_output(twice, ref)
    assert not r["ok"], r
    # the bias added in bf16 (to the rounded accumulator)
    acc_nb = nhwc(F.conv2d(nchw(x.float()), wt.float(), None, padding=1))
    bias16 = F.relu((acc_nb.to(torch.bfloat16) + b.float().to(torch.bfloat16)).float() + res.float()).to(torch.bfloat16)
    assert not cr.check_output(bias16, ref)["ok"]
    # a zeroed channel tail
    tail = good.clone()
    tail[..., cout - 4:] = 0
    assert not cr.check_output(tail, ref)["ok"]
    # one input pixel dropped from the implicit GEMM's A operand (a tile edge read as zero)
    xd = x.clone()
    xd[1, 5, 15] = 0.0
    dropped = F.relu(nhwc(F.conv2d(nchw(xd.float()), wt.float(), b.float(), padding=1)) + res.float()).to(torch.bfloat16)
    assert not cr.check_output(dropped, ref)["ok"]
    # fp32 outputs
    ref32 = cr.conv_fwd(x, wt, b, pad=1)
    assert cr.check_output(acc, ref32)["ok"]
    assert not cr.check_output(nhwc(F.conv2d(nchw(xd.float()), wt.float(), b.float(), padding=1)), ref32)["ok"]
