"""GPU (-m gpu): non-dense operand strides through the C-ABI (osd_conv_desc.in_stride_n / _h / _w, out_stride, res_stride).

ops.py always passes dense strides, so only a direct caller of the library meets these.  The descriptor is built the way
ops._build_conv_desc / ops._conv_desc build it, then one stride is changed by hand:
  slice   the input is a channel slice of a wider tensor (in_stride_w > cin)
  rows    padded rows (in_stride_h > w * in_stride_w)
  gaps    gaps between images (in_stride_n > h * in_stride_h)
  out     out_stride > cout, a sentinel in the channels the call must not write
  res     res_stride > cout (a RES_SAME residual that is a channel slice)
Every call of osd_conv2d_fwd (algo 0 and every candidate the tuner may pick) and of osd_conv2d_wgrad (every variant x split
target, and the filter-row kernel) either matches the float64 reference under the bounds of tests/conv_ref.py or returns
OSD_ERR_UNSUPPORTED — never wrong values, never a store outside its slice (the bytes between the pixels keep their sentinel,
and so does a guard region behind every buffer).  All buffers are allocated for the strides they are described with."""
import ctypes as C

import pytest
import torch

import conv_ref as cr
from oracle import launch_replay as lr

pytestmark = pytest.mark.gpu

OSD_ERR_UNSUPPORTED = -2
GUARD = 4096                 # elements of sentinel behind every buffer
GAP_FILL = 64.0              # what the bytes outside an input's slice hold: a kernel that reads them gets visibly wrong values
OUT_FILL = -777.0            # the output's sentinel

STRIDE_MODES = ["dense", "slice", "rows", "gaps", "out", "res"]
# dtype, n, cin, h, w, cout, k, stride, pad: conv_sp's padded-image width (64) and general width, the prediction-conv kernel's
# skinny output, a 1x1 (conv_px), stride 2 and fp32
FWD_CASES = [
    ("bf16", 3, 64, 5, 64, 256, 3, 1, 1),
    ("bf16", 2, 128, 7, 13, 128, 3, 1, 1),
    ("bf16", 2, 256, 9, 11, 4, 3, 1, 1),
    ("bf16", 2, 64, 6, 10, 256, 1, 1, 0),
    ("bf16", 2, 64, 9, 11, 64, 3, 2, 1),
    ("f32", 2, 32, 9, 11, 64, 3, 1, 1),
]


def ops():
    from oneshotdet_amd import ops as o
    return o


def _dt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _strided_input(x, mode, fill=GAP_FILL):
    """x dense NHWC on the GPU -> (flat buffer, element offset of pixel 0, (sN, sH, sW)) for the stride mode; everything outside the
    described slice holds `fill`."""
    n, h, w, c = x.shape
    epc = 8 if x.dtype == torch.bfloat16 else 4
    sw = c + (64 if mode == "slice" else 0)
    sh = w * sw + (3 * epc if mode == "rows" else 0)
    sn = h * sh + (5 * epc if mode == "gaps" else 0)
    off = 32 if mode == "slice" else 0                 # the slice starts 32 channels into the wider tensor
    buf = torch.full((off + n * sn + GUARD,), fill, dtype=x.dtype, device=x.device)
    view = torch.as_strided(buf, (n, h, w, c), (sn, sh, sw, 1), off)
    view.copy_(x)
    return buf, off, (sn, sh, sw)


def _desc(dtype, x_shape, cout, w_rows, k, stride, pad, strides):
    o = ops()
    n, h, w, c = x_shape
    d = o.ConvDesc()
    d.dtype = o.OSD_BF16 if dtype == torch.bfloat16 else o.OSD_F32
    d.n, d.h, d.w, d.cin = n, h, w, c
    d.in_stride_n, d.in_stride_h, d.in_stride_w = strides
    d.ho, d.wo = o.conv_out(h, k, stride, pad), o.conv_out(w, k, stride, pad)
    d.cout, d.r, d.s, d.w_rows = cout, k, k, w_rows
    d.stride_h = d.stride_w = stride
    d.pad_h = d.pad_w = pad
    d.out_stride = cout
    d.res_mode = o.RES_NONE
    return d


def _addr(buf, off=0):
    return buf.data_ptr() + off * buf.element_size()


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "%s-%dx%dx%dx%d-%d-k%ds%d" % (c[0], c[1], c[3], c[4], c[2], c[5], c[6], c[7]))
def test_conv_fwd_with_strided_operands_matches_or_is_refused(case):
    o = ops()
    from oneshotdet_amd import _lib
    lib = _lib.load()
    dname, n, cin, h, w, cout, k, stride, pad = case
    T = _dt(dname)
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(n, h, w, cin, generator=g)).to(T).cuda()
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    pc = o.pack_conv(wt.cuda(), bias=torch.randn(cout, generator=g).cuda(), dtype=T)
    cs = pc.cout_store
    w_ref = lr.unpack_weight(pc.w, cs).cuda()                       # the kernel's own (rounded) operands
    ho, wo = o.conv_out(h, k, stride, pad), o.conv_out(w, k, stride, pad)
    res = torch.randn(n, ho, wo, cs, generator=g).to(T).cuda()
    cands = [0] + sorted(set(o.conv_algo_candidates(cs, False, pixels=n * ho * wo) + [1 + 16 + 6, o.CONV_ALGO_PX, o.CONV_ALGO_PX_WIDE]))
    table = {}
    bad = []
    for mode in STRIDE_MODES:
        xbuf, xoff, strides = _strided_input(x, "dense" if mode in ("out", "res") else mode)
        d = _desc(T, x.shape, cs, pc.w_rows, k, stride, pad, strides)
        ostride = cs + (64 if mode == "out" else 0)
        d.out_stride = ostride
        rbuf = None
        if mode == "res":
            d.res_mode, d.res_h, d.res_w, d.res_stride = o.RES_SAME, ho, wo, cs + 32
            rbuf = torch.full((n * ho * wo * (cs + 32) + GUARD,), GAP_FILL, dtype=T, device="cuda")
            torch.as_strided(rbuf, res.shape, (ho * wo * (cs + 32), wo * (cs + 32), cs + 32, 1), 0).copy_(res)
        ref = cr.conv_fwd(x, w_ref, pc.bias, stride=stride, pad=pad, res=res if mode == "res" else None,
                          res_mode=o.RES_SAME if mode == "res" else o.RES_NONE)
        for algo in cands:
            d.algo = algo
            ybuf = torch.full((n * ho * wo * ostride + GUARD,), OUT_FILL, dtype=T, device="cuda")
            rc = lib.osd_conv2d_fwd(C.byref(d), _addr(xbuf, xoff), pc.w.data_ptr(), pc.bias.data_ptr(),
                                    None if rbuf is None else rbuf.data_ptr(), None, None, None, ybuf.data_ptr(), None)
            torch.cuda.synchronize()
            body = ybuf[:n * ho * wo * ostride].view(n, ho, wo, ostride)
            untouched = bool((ybuf[n * ho * wo * ostride:] == OUT_FILL).all()) and bool((body[..., cs:] == OUT_FILL).all())
            if rc == OSD_ERR_UNSUPPORTED:
                table.setdefault(mode, {})[algo] = "unsupported"
                if not bool((body == OUT_FILL).all()) or not untouched:
                    bad.append((mode, algo, "refused, but wrote its output"))
                continue
            if rc != 0:
                bad.append((mode, algo, "rc %d: %s" % (rc, lib.osd_last_error_string())))
                continue
            got = body[..., :cs]
            r = cr.check_output(got, ref)
            table.setdefault(mode, {})[algo] = "ok" if r["ok"] else "WRONG"
            if not r["ok"] or not untouched:
                bad.append((mode, algo, "untouched sentinel %s" % untouched, {kk: v for kk, v in r.items() if kk != "ok"}))
    print("\n%s: %s" % (case, {m: " ".join("%d:%s" % (a, s[0]) for a, s in sorted(v.items())) for m, v in table.items()}))
    assert not bad, bad[:8]
    # every mode ran on at least the library's default kernel
    assert all(table[m].get(0) == "ok" for m in STRIDE_MODES), table


WGRAD_CASES = [
    # dtype, n, cin, h, w, cout, k, stride, pad
    ("bf16", 3, 256, 6, 32, 256, 3, 1, 1),
    ("bf16", 2, 128, 7, 13, 128, 1, 2, 0),
    ("f32", 2, 64, 9, 11, 64, 3, 1, 1),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "%s-%dx%dx%dx%d-%d-k%ds%d" % (c[0], c[1], c[3], c[4], c[2], c[5], c[6], c[7]))
def test_conv_wgrad_with_strided_input_matches_or_is_refused(case):
    """osd_conv2d_wgrad: x with a channel slice, padded rows or gaps between images (dy stored with more channels than cout in the
    `out` mode) -> dW and db match the float64 reference under the accumulated-gradient bound, or the call is refused; a refused
    call leaves dW and db alone."""
    o = ops()
    from oneshotdet_amd import _lib
    lib = _lib.load()
    dname, n, cin, h, w, cout, k, stride, pad = case
    T = _dt(dname)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, h, w, cin, generator=g).to(T).cuda()
    ho, wo = o.conv_out(h, k, stride, pad), o.conv_out(w, k, stride, pad)
    dy = torch.randn(n, ho, wo, cout, generator=g).to(T).cuda()
    scale = (torch.rand(cout, generator=g) + 0.5).cuda()
    cands = [0] + o.wgrad_algo_candidates(o.OSD_BF16 if T == torch.bfloat16 else o.OSD_F32, cout, cin)
    cands += o.wgrad_xr_candidates(o.OSD_BF16 if T == torch.bfloat16 else o.OSD_F32, cout, cin, k, k, stride, pad, [w])
    ref_dw, ref_db = cr.conv_wgrad(x, dy, k, k, stride, pad, cout, scale=scale, want_bias=True)
    table, bad = {}, []
    for mode in ("dense", "slice", "rows", "gaps", "out"):
        xbuf, xoff, strides = _strided_input(x, "dense" if mode == "out" else mode)
        d = o._conv_desc(x.shape, o.OSD_BF16 if T == torch.bfloat16 else o.OSD_F32, cout, k, k, stride, pad, cout)
        d.in_stride_n, d.in_stride_h, d.in_stride_w = strides
        dyv = dy
        if mode == "out":                                # dy stored with 64 more channels per pixel than cout
            dyv = torch.full((n, ho, wo, cout + 64), GAP_FILL, dtype=T, device="cuda")
            dyv[..., :cout] = dy
            d.out_stride = cout + 64
        for algo in cands:
            d.algo = algo
            dw = torch.zeros(cout * k * k * cin + GUARD, device="cuda")
            db = torch.zeros(cout + GUARD, device="cuda")
            rc = lib.osd_conv2d_wgrad(C.byref(d), _addr(xbuf, xoff), dyv.data_ptr(), scale.data_ptr(), dw.data_ptr(), db.data_ptr(), None)
            torch.cuda.synchronize()
            guards = bool((dw[cout * k * k * cin:] == 0).all()) and bool((db[cout:] == 0).all())
            if rc == OSD_ERR_UNSUPPORTED:
                table.setdefault(mode, {})[algo] = "unsupported"
                if bool(dw.abs().max() > 0) or bool(db.abs().max() > 0):
                    bad.append((mode, algo, "refused, but wrote dW / db"))
                continue
            if rc != 0:
                bad.append((mode, algo, "rc %d: %s" % (rc, lib.osd_last_error_string())))
                continue
            rw = cr.check_accumulated(dw[:cout * k * k * cin].view(cout, k, k, cin), ref_dw)
            rb = cr.check_accumulated(db[:cout], ref_db)
            table.setdefault(mode, {})[algo] = "ok" if rw["ok"] and rb["ok"] else "WRONG"
            if not (rw["ok"] and rb["ok"] and guards):
                bad.append((mode, algo, "guards %s" % guards, rw, rb))
    print("\n%s: %s" % (case, {m: "%d ok, %d unsupported, %d wrong" % tuple(sum(1 for s in v.values() if s == t) for t in ("ok", "unsupported", "WRONG"))
                               for m, v in table.items()}))
    assert not bad, bad[:8]
    assert table["dense"].get(0) == "ok" and table["out"].get(0) == "ok", table
