"""GPU: every exported support kernel that the engine reaches only at the model's own shapes (or not at all), called directly and
compared with its restatement in tests/support_ref.py at the smallest shapes that reach each code path of the kernel.

Bars (the project's existing ones, tests/conv_ref.py): `torch.equal` for copies, roundings and single IEEE operations;
`assert_output` for rounded outputs (one bf16 ulp, FLIP_CAP; fp32 1e-4 |ref| + 1e-5 absmax); `assert_accumulated` for fp32 sums;
rtol 1e-6 / atol 1e-7 for parameters after SGD steps.  Every test prints its worst error in units of its bar (MI355X: SGD
parameters 0.13, momentum 0.17; bias_grad <= 0.03; dgrad_naive fp32 <= 0.03, bf16 <= 0.89 ulp; upsample2x_bwd fp32 0.003, bf16 0;
scores 0.002; Scale gradient 0.03; everything else is exact).

What these tests found: left to the compiler's contraction, the SGD kernels fused two lanes of every group of four and not the other
two, and their one-value path fused all — a tensor's update depended on its alignment, and osd_sgd_momentum_multi and
osd_sgd_momentum_pack_multi differed in the last bit wherever they chose different paths (cin % 4 != 0).  The kernels now spell the
three fused multiply-adds out (test_sgd_momentum_pack_multi_update_packed_weights_and_consumed_gradients)."""
import functools

import pytest
import torch

import conv_ref as cr
import support_ref as sr
from oracle import launch_replay as lr

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
DTC = {"f32": 0, "bf16": 1}          # OSD_F32, OSD_BF16
EP = {"f32": 4, "bf16": 8}           # elements of one 16-byte chunk
SENT = 7.0                           # sentinel (exact in bf16) for memory a kernel must not write
BOTH = pytest.mark.parametrize("dt", ["f32", "bf16"])


def ops():
    from oneshotdet_amd import ops as o
    return o


def call(name, *args):
    from oneshotdet_amd import _lib
    _lib.call(name, *args)


def P(t):
    return None if t is None else t.data_ptr()


def ST():
    return ops()._stream()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def note(what, **figures):
    print("\nBAR %s: %s" % (what, ", ".join("%s %.3g" % kv for kv in sorted(figures.items()))))


def worst_of(res):
    return res.get("worst_ulp", res.get("worst_rel", 0.0))


def ru(x, m):
    return (x + m - 1) // m * m


# =============================================================================================================== weight packers
# cout, cin, r, s, scale, n_blocks, floats of an unrelated tensor in front (-> src_off % 4), data-gradient kpad
PACK_SHAPES = [
    (64, 64, 3, 3, False, 3, 0, 64),      # forward: 16 bytes per lane; data gradient: whole 64 x 64 tiles
    (80, 72, 1, 1, True, 2, 0, 128),      # rows and columns of padding; data gradient: a partial 64-tile in both directions
    (4, 256, 3, 3, True, 1, 0, 16),       # data gradient: kpad = 16 -> the 32 x 32 transpose
    (6, 10, 3, 3, True, 2, 0, 16),        # cin % 4 != 0: one value per lane in both forms
    (16, 64, 7, 7, True, 4, 0, 64),
    (8, 16, 1, 1, True, 1, 3, 64),        # behind a 3-float tensor: src_off % 4 == 3 -> the scalar forward path, the 32 x 32 transpose
    (12, 8, 1, 3, False, 1, 0, 16),
    (16, 64, 1, 1, True, 2, 0, 64),       # dst_off % 4 == 2 (see pack_case): no 16-byte stores, the one-value paths of both forms
]


@functools.lru_cache(None)
def pack_case(dt):
    kmult = 16 if dt == "f32" else 64
    fwd, dg = [], []
    src_off = scale_off = fwd_off = dg_off = 0
    for cout, cin, r, s, scaled, nb, front, dg_kpad in PACK_SHAPES:
        src_off = ru(src_off, 4) + front
        geo = dict(src_off=src_off, scale_off=scale_off if scaled else -1, cout=cout, cin=cin, r=r, s=s, n_blocks=nb)
        rows = ru(cout, 16) + (16 if cin == 72 else 0)
        shift = 2 if (cout, cin, r, s) == (16, 64, 1, 1) else 0
        fwd_off = ru(fwd_off, 64) + 64 + shift          # 64 sentinel elements (at least) in front of and between the entries
        fwd.append(dict(geo, dst_off=fwd_off, rows=rows, kpad=ru(cin, kmult)))
        fwd_off += rows * r * s * ru(cin, kmult)
        dg_off = ru(dg_off, 64) + 64 + shift
        dg.append(dict(geo, dst_off=dg_off, rows=ru(cin, 16), kpad=dg_kpad))
        dg_off += ru(cin, 16) * r * s * dg_kpad
        src_off += cout * r * s * cin
        scale_off += cout if scaled else 0
        scale_off += 1                                  # scale vectors do not start on multiples of four either
    src = rnd(src_off + 5, seed=11)
    scales = rnd(scale_off + 3, seed=12) * 0.5 + 1.5
    return dict(src=src, scales=scales, fwd=(fwd, fwd_off + 64), dg=(dg, dg_off + 64))


def entry_weight(c, e):
    n = e["cout"] * e["r"] * e["s"] * e["cin"]
    w = c["src"][e["src_off"]:e["src_off"] + n].view(e["cout"], e["r"], e["s"], e["cin"])
    sc = None if e["scale_off"] < 0 else c["scales"][e["scale_off"]:e["scale_off"] + e["cout"]]
    return w, sc


@BOTH
@pytest.mark.parametrize("form", ["forward", "dgrad"])
def test_single_conv_packers_are_one_multiplication_and_one_rounding(form, dt):
    """osd_pack_conv_weight_ex / osd_pack_conv_weight_dgrad, both source orders, at every shape of the table: exact, padding zero."""
    c = pack_case(dt)
    entries = c["fwd" if form == "forward" else "dg"][0]
    name = "osd_pack_conv_weight_ex" if form == "forward" else "osd_pack_conv_weight_dgrad"
    ref_fn = sr.pack_fwd if form == "forward" else sr.pack_dgrad
    for e in entries:
        w, sc = entry_weight(c, e)
        want = ref_fn(w, sc, e["rows"], e["kpad"], DT[dt])
        scd = None if sc is None else sc.cuda()
        for orsi in (1, 0):
            wsrc = (w if orsi else w.permute(0, 3, 1, 2)).contiguous().cuda()
            got = torch.full((e["rows"] * e["r"] * e["s"] * e["kpad"] + 16,), SENT, dtype=DT[dt], device="cuda")
            call(name, P(wsrc), P(scd), P(got), e["cout"], e["cin"], e["r"], e["s"], e["rows"], e["kpad"], orsi, DTC[dt], ST())
            got = got.cpu()
            assert torch.equal(got[:-16].view(want.shape), want), (form, e, orsi)
            assert bool((got[-16:] == SENT).all())
    # the wrappers (their own padded geometry)
    e = entries[3]
    w, sc = entry_weight(c, e)
    kmult = 16 if dt == "f32" else 64
    if form == "forward":
        got = ops().pack_conv_master(w.cuda(), sc.cuda(), DT[dt])
        want = sr.pack_fwd(w, sc, ru(e["cout"], 16), ru(e["cin"], kmult), DT[dt])
    else:
        got = ops().pack_conv_master_dgrad(w.cuda(), sc.cuda(), DT[dt])
        want = sr.pack_dgrad(w, sc, ru(e["cin"], 16), ru(e["cout"], kmult), DT[dt])
    assert got.shape == want.shape and torch.equal(got.cpu(), want)


@BOTH
@pytest.mark.parametrize("dgrad", [0, 1])
def test_pack_multi_every_path_is_exact_and_equals_the_single_conv_packer(dgrad, dt):
    """osd_pack_multi over one table that reaches the four code paths of its kernel (forward 16-byte / scalar, data-gradient
    64 x 64 / 32 x 32 transpose): the value is w * scale in fp32, rounded once; padding is zero; nothing outside the entries is
    written; every entry is bit-identical to the single-conv packer of the same form."""
    c = pack_case(dt)
    entries, numel = c["dg" if dgrad else "fwd"]
    src, scales = c["src"].cuda(), c["scales"].cuda()
    dst = torch.full((numel,), SENT, dtype=DT[dt], device="cuda")
    table, owner, nb = sr.pack_table(entries, "cuda")
    assert nb == sum(e["n_blocks"] for e in entries)
    call("osd_pack_multi", P(table), P(owner), nb, P(src), P(scales), P(dst), dgrad, DTC[dt], ST())
    want = sr.pack_multi(entries, c["src"], c["scales"], torch.full((numel,), SENT, dtype=DT[dt]), dgrad)
    got = dst.cpu()
    inside = torch.zeros(numel, dtype=torch.bool)
    for e in entries:
        n = e["rows"] * e["r"] * e["s"] * e["kpad"]
        sl = slice(e["dst_off"], e["dst_off"] + n)
        inside[sl] = True
        assert torch.equal(got[sl], want[sl]), e
        g = got[sl].view(e["rows"], e["r"], e["s"], e["kpad"]).float()
        real_rows, real_k = (e["cin"], e["cout"]) if dgrad else (e["cout"], e["cin"])
        assert float(g[real_rows:].abs().sum()) == 0.0 and float(g[..., real_k:].abs().sum()) == 0.0, e       # padding
        one = torch.empty(n, dtype=DT[dt], device="cuda")
        wv = src[e["src_off"]:]
        sv = None if e["scale_off"] < 0 else scales[e["scale_off"]:]
        call("osd_pack_conv_weight_dgrad" if dgrad else "osd_pack_conv_weight_ex", P(wv), P(sv), P(one), e["cout"], e["cin"], e["r"],
             e["s"], e["rows"], e["kpad"], 1, DTC[dt], ST())
        assert torch.equal(one.cpu(), got[sl]), e
    assert bool((got[~inside] == SENT).all()) and int((~inside).sum()) >= 64 * (len(entries) + 1)


# =============================================================================================================== SGD
SGD_LR, SGD_MOM = 0.05, 0.9
SGD_N = 4120
SGD_ENTRIES = [
    dict(off=0, numel=1, lr_mult=2.0, wd=0.0, n_blocks=1),
    dict(off=1, numel=3, lr_mult=1.0, wd=1e-4, n_blocks=1),              # off % 4 == 1: one value per lane
    dict(off=4, numel=4, lr_mult=1.0, wd=1e-2, n_blocks=1),
    dict(off=8, numel=5, lr_mult=0.5, wd=1e-4, n_blocks=1),              # one 16-byte group and a tail of one
    dict(off=13, numel=5, lr_mult=2.0, wd=0.0, n_blocks=3),              # more workgroups than work
    dict(off=20, numel=1027, lr_mult=1.0, wd=1e-4, n_blocks=3),          # several trips of three workgroups, a tail of three
    dict(off=1049, numel=1027, lr_mult=1.0, wd=5e-3, n_blocks=1),        # off % 4 == 1
    # conv weights [cout][rs][cin] (the pack form also writes [rows][rs][kpad]); plain tensors for osd_sgd_momentum_multi
    dict(off=2080, numel=8 * 9 * 16, lr_mult=1.0, wd=1e-4, n_blocks=3, cout=8, rs=9, cin=16, kpad=24, rows=10, dst_off=16, scale_off=2),
    dict(off=3232, numel=6 * 9 * 10, lr_mult=1.0, wd=1e-4, n_blocks=1, cout=6, rs=9, cin=10, kpad=16, rows=8, dst_off=2192, scale_off=-1),
    dict(off=3773, numel=4 * 1 * 8, lr_mult=1.0, wd=1e-2, n_blocks=1, cout=4, rs=1, cin=8, kpad=8, rows=4, dst_off=3360, scale_off=11),
    dict(off=3808, numel=5 * 4 * 12, lr_mult=0.5, wd=1e-4, n_blocks=2, cout=5, rs=4, cin=12, kpad=12, rows=5, dst_off=3408, scale_off=-1),
    dict(off=4048, numel=6, lr_mult=2.0, wd=0.0, n_blocks=1),
    # dst_off % 4 == 2 and kpad % 4 == 2: the packed group of four cannot go out as one store -> one value per lane
    dict(off=4064, numel=3 * 2 * 8, lr_mult=1.0, wd=1e-4, n_blocks=1, cout=3, rs=2, cin=8, kpad=10, rows=3, dst_off=3666, scale_off=-1),
]
SGD_PACKED_N = 3744


def sgd_inside():
    m = torch.zeros(SGD_N, dtype=torch.bool)
    for e in SGD_ENTRIES:
        assert not bool(m[e["off"]:e["off"] + e["numel"]].any()) and e["off"] + e["numel"] <= SGD_N
        m[e["off"]:e["off"] + e["numel"]] = True
    return m


def sgd_pack_entries():
    """the conv entries as osd_pack_multi (forward form) entries: [cout][rs][cin] masters are [cout][r = rs][s = 1][cin]"""
    return [dict(src_off=e["off"], dst_off=e["dst_off"], scale_off=e["scale_off"], cout=e["cout"], cin=e["cin"], r=e["rs"], s=1,
                 rows=e["rows"], kpad=e["kpad"], n_blocks=2) for e in SGD_ENTRIES if "dst_off" in e]


def sgd_packed_init(dtype):
    packed = torch.full((SGD_PACKED_N,), SENT, dtype=dtype)
    inside = torch.zeros(SGD_PACKED_N, dtype=torch.bool)
    for e in sgd_pack_entries():
        sl = slice(e["dst_off"], e["dst_off"] + e["rows"] * e["r"] * e["kpad"])
        assert not bool(inside[sl].any()) and sl.stop <= SGD_PACKED_N
        inside[sl] = True
    packed[inside] = 0.0                                    # the padding is zero from an initial pack and is never written
    return packed, inside


@functools.lru_cache(None)
def sgd_data():
    p0 = rnd(SGD_N, seed=21)
    grads = [rnd(SGD_N, seed=22 + k, scale=0.1) for k in range(3)]
    scales = rnd(16, seed=25) * 0.5 + 1.5
    ref_p, ref_buf = sr.sgd_steps(SGD_ENTRIES, p0, grads, SGD_LR, SGD_MOM)
    return p0, grads, scales, ref_p, ref_buf


def run_sgd(dt=None, zero_grads=0):
    """three steps (first_step = 1, 0, 0); dt None: osd_sgd_momentum_multi, else osd_sgd_momentum_pack_multi writing `dt`"""
    p0, grads, scales, _, _ = sgd_data()
    p, buf = p0.clone().cuda(), torch.full((SGD_N,), 5.0, device="cuda")        # the first step must not read the momentum
    sc = scales.cuda()
    packed = None
    if dt is None:
        table, owner, nb = sr.sgd_table(SGD_ENTRIES, "cuda")
    else:
        table, owner, nb = sr.sgd_pack_table(SGD_ENTRIES, "cuda")
        packed = sgd_packed_init(DT[dt])[0].cuda()
    after = []
    for k in range(3):
        g = grads[k].clone().cuda()
        if dt is None:
            call("osd_sgd_momentum_multi", P(table), P(owner), nb, P(p), P(g), P(buf), SGD_LR, SGD_MOM, int(k == 0), ST())
        else:
            call("osd_sgd_momentum_pack_multi", P(table), P(owner), nb, P(p), P(g), P(buf), P(sc), P(packed), DTC[dt], SGD_LR, SGD_MOM,
                 int(k == 0), zero_grads, ST())
        after.append(g.cpu())
    return p.cpu(), buf.cpu(), None if packed is None else packed.cpu(), after


def check_sgd_against_float64(p, buf, what):
    p0, _, _, ref_p, ref_buf = sgd_data()
    m = sgd_inside()
    worst = {}
    for name, got, ref in (("params", p, ref_p), ("momentum", buf, ref_buf)):
        err = (got.double() - ref)[m].abs() / (sr.SGD_ATOL + sr.SGD_RTOL * ref[m].abs())
        worst[name] = float(err.max())
    note(what, **worst)
    assert worst["params"] <= 1.0 and worst["momentum"] <= 1.0, worst
    assert torch.equal(p[~m], p0[~m]) and bool((buf[~m] == 5.0).all())         # nothing outside the table's entries is written


def test_sgd_momentum_multi_matches_the_float64_update():
    p, buf, _, after = run_sgd()
    check_sgd_against_float64(p, buf, "sgd_momentum_multi")
    for k, g in enumerate(after):
        assert torch.equal(g, sgd_data()[1][k])


@BOTH
@pytest.mark.parametrize("zero_grads", [0, 1])
def test_sgd_momentum_pack_multi_update_packed_weights_and_consumed_gradients(zero_grads, dt):
    p0, grads, scales, _, _ = sgd_data()
    p, buf, packed, after = run_sgd(dt, zero_grads)
    check_sgd_against_float64(p, buf, "sgd_momentum_pack_multi %s" % dt)
    # the two entry points run the same update: bit-identical parameters and momentum
    p1, buf1, _, _ = run_sgd()
    assert torch.equal(p, p1) and torch.equal(buf, buf1)
    # packed = round(the kernel's OWN updated fp32 master * scale), padding still zero, sentinel outside
    init, inside = sgd_packed_init(DT[dt])
    want = sr.pack_multi(sgd_pack_entries(), p, scales, init, 0)
    assert torch.equal(packed, want)
    assert bool((packed[~inside] == SENT).all())
    # ... which is what osd_pack_multi (forward form) writes from those masters
    ents = sgd_pack_entries()
    table, owner, nb = sr.pack_table(ents, "cuda")
    dst, pc, sc = init.clone().cuda(), p.cuda(), scales.cuda()
    call("osd_pack_multi", P(table), P(owner), nb, P(pc), P(sc), P(dst), 0, DTC[dt], ST())
    assert torch.equal(dst.cpu(), packed)
    # zero_grads: exactly the elements of the table's entries are zeroed; otherwise the gradients are left bit-identical
    m = sgd_inside()
    for k, g in enumerate(after):
        if zero_grads:
            assert float(g[m].abs().max()) == 0.0 and torch.equal(g[~m], grads[k][~m])
        else:
            assert torch.equal(g, grads[k])


# =============================================================================================================== gradients
@pytest.mark.parametrize("shape", [(5, 7, 3, 3), (64, 32, 1, 1)])
def test_unpack_wgrad_writes_and_accumulates_exactly(shape):
    cout, cin, r, s = shape
    dw = rnd(cout, r, s, cin, seed=31)
    scale = rnd(cout, seed=32) * 0.5 + 1.5
    n = cout * cin * r * s
    dwd = dw.cuda()
    for sc in (None, scale):
        scd = None if sc is None else sc.cuda()
        out = torch.full((n + 8,), SENT, device="cuda")
        call("osd_unpack_wgrad", P(dwd), P(scd), P(out), cout, cin, r, s, 0, ST())
        want = sr.unpack_wgrad(dw, sc)
        assert torch.equal(out[:n].cpu().view(cout, cin, r, s), want) and bool((out[n:] == SENT).all())
        g = rnd(cout, cin, r, s, seed=33)
        acc = g.clone().cuda()
        for _ in range(2):
            ops().unpack_wgrad(dwd, scd, out=acc, accumulate=True)
            g = sr.unpack_wgrad(dw, sc, g)
        assert torch.equal(acc.cpu(), g)
        assert torch.equal(ops().unpack_wgrad(dwd, scd).cpu(), want)


@BOTH
@pytest.mark.parametrize("m,c,stride", [(1, 1, 8), (513, 257, 264), (65537, 4, 8)])
def test_bias_grad_accumulates_the_column_sums(m, c, stride, dt):
    """one row block and two, a second channel block, the 2048-row variant (m > 65536); db accumulates; columns past c are not summed"""
    dy = rnd(m, stride, seed=41).to(DT[dt])
    dy[:, c:] = 1000.0
    db0 = torch.cat([rnd(c, seed=42) * 3, torch.full((4,), SENT)])
    db = db0.clone().cuda()
    ops().bias_grad(dy.cuda().view(1, 1, m, stride), db, c)
    res = cr.assert_accumulated(db[:c].cpu(), sr.bias_grad(dy, c, db0[:c]), what="bias_grad %s" % ((m, c, stride),))
    note("bias_grad %s %s" % ((m, c, stride), dt), err_over_tol=res["err"] / cr.ACC_TOL)
    assert bool((db[c:] == SENT).all())


DGRAD_CASES = [
    # n, cin, h, w, cout, k, stride, pad
    (2, 64, 9, 11, 64, 3, 2, 1),
    (1, 64, 8, 6, 128, 3, 2, 1),
    (2, 64, 5, 7, 64, 1, 2, 0),
    (1, 64, 7, 5, 64, 3, 1, 1),
]


@BOTH
@pytest.mark.parametrize("case", DGRAD_CASES)
def test_conv2d_dgrad_naive_masks_then_adds(case, dt):
    """float64 data gradient from the packed (rounded) weights, the ReLU mask applied BEFORE the addend; dy stored with a pixel
    stride wider than cout."""
    n, cin, h, w, cout, k, st, pad = case
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    wt = rnd(cout, cin, k, k, seed=51) / (3.0 * k)
    pc = ops().pack_conv(wt.cuda(), dtype=DT[dt])
    assert pc.cin_k == cin                                     # the kernel indexes the packed rows with cin: cin_pad == cin
    w_oihw = lr.unpack_weight(pc.w.cpu(), cout)[:, :cin]
    dy = rnd(n, ho, wo, cout + 8, seed=52).to(DT[dt])
    mask = rnd(n, h, w, cin, seed=53)
    mask[rnd(n, h, w, cin, seed=54) > 0.8] = 0.0               # exact zeros and negative values: both switch the gradient off
    mask, addend = mask.to(DT[dt]), rnd(n, h, w, cin, seed=55).to(DT[dt])
    worst = 0.0
    for m, a in ((None, None), (mask, None), (None, addend), (mask, addend)):
        dx = ops().conv2d_dgrad_naive(dy.cuda(), pc.w, (n, h, w, cin), k, k, st, pad, cout, mask=None if m is None else m.cuda(),
                                      addend=None if a is None else a.cuda())
        ref = sr.dgrad_naive(dy, w_oihw, (n, h, w, cin), st, pad, mask=m, addend=a)
        res = cr.assert_output(dx, ref, what="dgrad_naive %s mask %s addend %s" % (case, m is not None, a is not None))
        worst = max(worst, worst_of(res))
    note("dgrad_naive %s %s" % (case, dt), worst=worst)


# =============================================================================================================== element-wise
def chans(dt):
    return [EP[dt], 264]


def masks_like(shape, seed, dtype):
    m = rnd(*shape, seed=seed)
    m[rnd(*shape, seed=seed + 1) > 0.8] = 0.0
    return m.to(dtype)


@BOTH
@pytest.mark.parametrize("geo", [(9, 11, 5, 6), (8, 6, 4, 3)])
def test_scatter2x_adds_then_masks(geo, dt):
    h, w, ho, wo = geo
    n = 3
    for c in chans(dt):
        src = rnd(n, ho, wo, c, seed=61).to(DT[dt])
        mask, addend = masks_like((n, h, w, c), 62, DT[dt]), rnd(n, h, w, c, seed=64).to(DT[dt])
        for m, a in ((None, None), (mask, None), (None, addend), (mask, addend)):
            got = ops().scatter2x(src.cuda(), (h, w), mask=None if m is None else m.cuda(), addend=None if a is None else a.cuda())
            want = sr.round_dtype(sr.scatter2x(src, (h, w), mask=m, addend=a), DT[dt])
            assert torch.equal(got.cpu(), want), (geo, c, m is not None, a is not None)


@BOTH
def test_add_mask_every_operand_combination_in_place_and_past_the_grid(dt):
    for c in chans(dt):
        a, b, mask = rnd(3, 5, 7, c, seed=71).to(DT[dt]), rnd(3, 5, 7, c, seed=72).to(DT[dt]), masks_like((3, 5, 7, c), 73, DT[dt])
        for bb, mm in ((None, None), (b, None), (None, mask), (b, mask)):
            want = sr.round_dtype(sr.add_mask(a, bb, mm), DT[dt])
            bd, md = None if bb is None else bb.cuda(), None if mm is None else mm.cuda()
            assert torch.equal(ops().add_mask(a.cuda(), bd, md).cpu(), want)
            ad = a.clone().cuda()
            assert ops().add_mask(ad, bd, md, out=ad) is ad and torch.equal(ad.cpu(), want)        # out aliases a
    # more 16-byte chunks than 2048 workgroups x 256 lanes: the grid-stride loop takes a second trip
    numel = (2048 * 256 + 1000) * EP[dt]
    a, b, mask = rnd(numel, seed=75).to(DT[dt]), rnd(numel, seed=76).to(DT[dt]), masks_like((numel,), 77, DT[dt])
    got = ops().add_mask(a.cuda(), b.cuda(), mask.cuda())
    assert torch.equal(got.cpu(), sr.round_dtype(sr.add_mask(a, b, mask), DT[dt]))


@BOTH
@pytest.mark.parametrize("hw", [(1, 1), (7, 5)])
def test_upsample2x_bwd_sums_the_2x2_block(hw, dt):
    h, w = hw
    n, worst = 3, 0.0
    for c in chans(dt):
        inner, prev = rnd(n, 2 * h, 2 * w, c, seed=81).to(DT[dt]), rnd(n, h, w, c, seed=82).to(DT[dt])
        for pv in (None, prev):
            got = ops().upsample2x_bwd(inner.cuda(), None if pv is None else pv.cuda())
            assert got.shape == (n, h, w, c)
            worst = max(worst, worst_of(cr.assert_output(got, sr.upsample2x_bwd(inner, pv), what="upsample2x_bwd %s c %d" % (hw, c))))
    note("upsample2x_bwd %s %s" % (hw, dt), worst=worst)


# =============================================================================================================== layouts
@BOTH
@pytest.mark.parametrize("shape", [(2, 5, 3, 7), (1, 264, 9, 4)])
def test_layout_changes_are_a_rounding_and_a_copy(shape, dt):
    n, c, h, w = shape
    x = rnd(n, c, h, w, seed=91)
    y = ops().nchw_f32_to_nhwc(x.cuda(), DT[dt])
    assert y.shape == (n, h, w, c) and torch.equal(y.cpu(), sr.nchw_to_nhwc(x, DT[dt]))
    back = ops().nhwc_to_nchw_f32(y)
    assert back.dtype == torch.float32 and torch.equal(back.cpu(), sr.nhwc_to_nchw(y.cpu()))
    assert torch.equal(back.cpu(), x.to(DT[dt]).float())                       # the round trip of representable data is the identity
    # a channel slice of a wider tensor: c0 = 3, c = 5 of pixel stride 16
    wide = rnd(n, h, w, 16, seed=92).to(DT[dt])
    got = ops().nhwc_to_nchw_f32(wide.cuda(), c0=3, c=5)
    assert got.shape == (n, 5, h, w) and torch.equal(got.cpu(), sr.nhwc_to_nchw(wide, 3, 5))


# =============================================================================================================== proposals
SD_LEVELS = [(5, 7, 8), (37, 29, 16)]           # h, w, stride; the second has more than 1024 locations
SD_PAD_HW = (592.0, 464.0)
SD_TRUE_HW = [[500.0, 400.0], [333.0, 461.0]]


@functools.lru_cache(None)
def sd_case(dt):
    n, out = 2, []
    for l, (h, w, st) in enumerate(SD_LEVELS):
        cc = rnd(n, h, w, 4, seed=101 + l, scale=4.0).clamp_min(-80.0)
        flat = cc.view(-1, 4)
        flat[0::7, 0] = -200.0                                      # the sigmoid underflows: not a candidate, score -1
        flat[3::11, 0] = 60.0                                       # sigmoid == 1
        flat[5::13, 1] = 90.0
        flat[2::9, 0] = -80.0
        reg = rnd(n, h, w, 8, seed=111 + l, scale=60.0).abs()
        rf = reg.view(-1, 8)
        for side in range(4):
            rf[side::5, side] = 1000.0                              # far outside the image on that side
        rf[4::17, :4] *= -1.0                                       # a negative distance is decoded like any other
        out.append((cc.to(DT[dt]), reg.to(DT[dt])))
    return out


@BOTH
@pytest.mark.parametrize("sizes", ["one", "per_image"])
def test_fcos_score_decode_two_levels_into_one_buffer(sizes, dt):
    n = 2
    offs, total = [], 5
    for h, w, _ in SD_LEVELS:
        offs.append(total)
        total += h * w + 3
    img_hw = torch.tensor(SD_TRUE_HW) if sizes == "per_image" else None
    scores = torch.full((n, total), -SENT, device="cuda")
    boxes = torch.full((n, total, 4), -SENT, device="cuda")
    scores2, boxes2 = scores.clone(), boxes.clone()
    ihw = None if img_hw is None else img_hw.cuda()
    for (cc, reg), (h, w, st), lo in zip(sd_case(dt), SD_LEVELS, offs):
        ccd, regd = cc.cuda(), reg.cuda()
        call("osd_fcos_score_decode_sizes", P(ccd), P(regd), P(scores), P(boxes), n, h, w, 4, 8, st, lo, total, SD_PAD_HW[0], SD_PAD_HW[1],
             P(ihw), DTC[dt], ST())
        if img_hw is None:
            call("osd_fcos_score_decode", P(ccd), P(regd), P(scores2), P(boxes2), n, h, w, 4, 8, st, lo, total, SD_PAD_HW[0], SD_PAD_HW[1],
                 DTC[dt], ST())
    scores, boxes = scores.cpu(), boxes.cpu()
    if img_hw is None:
        assert torch.equal(scores2.cpu(), scores) and torch.equal(boxes2.cpu(), boxes)      # the two entry points agree bit for bit
    written = torch.zeros(total, dtype=torch.bool)
    worst, n_dropped, clipped = 0.0, 0, set()
    for (cc, reg), (h, w, st), lo in zip(sd_case(dt), SD_LEVELS, offs):
        ref_s, dropped, ref_b = sr.score_decode(cc, reg, st, SD_PAD_HW[0], SD_PAD_HW[1], img_hw=img_hw)
        sl = slice(lo, lo + h * w)
        written[sl] = True
        assert torch.equal(boxes[:, sl], ref_b), (h, w)
        got = scores[:, sl]
        assert bool((got[dropped] == -1.0).all()) and bool((got[~dropped] >= 0.0).all())
        worst = max(worst, worst_of(cr.assert_output(got[~dropped], ref_s[~dropped], what="scores %s" % ((h, w),))))
        n_dropped += int(dropped.sum())
        for i in range(n):
            hh, ww = SD_TRUE_HW[i] if img_hw is not None else SD_PAD_HW
            b = ref_b[i]
            clipped |= {k for k, hit in (("l", (b[:, 0] == 0).any()), ("t", (b[:, 1] == 0).any()), ("r", (b[:, 2] == ww - 1).any()),
                                         ("b", (b[:, 3] == hh - 1).any())) if bool(hit)}
    assert n_dropped > 0 and clipped == {"l", "t", "r", "b"}
    assert bool((scores[:, ~written] == -SENT).all()) and bool((boxes[:, ~written] == -SENT).all())
    note("fcos_score_decode %s %s" % (sizes, dt), worst=worst)


def topk_keys(kind, n, total, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "ties":
        return torch.randint(0, 5, (n, total), generator=g).float() / 4
    keys = torch.rand(n, total, generator=g)
    if kind == "dropped":
        keys[torch.rand(n, total, generator=g) < 0.3] = -1.0
    return keys


@pytest.mark.parametrize("cnt", [1, 255, 256, 257, 1025, 3000])
def test_level_topk_keeps_the_topn_by_key_then_index(cnt):
    n, total, lo = 2, 4000, 37
    for kind in ("ties", "dropped", "random"):
        keys = topk_keys(kind, n, total, seed=cnt)
        for topn in (1, 100, cnt, cnt + 5):
            want = sr.level_topk(keys, lo, cnt, topn)
            assert torch.equal(want[:, :lo], keys[:, :lo]) and torch.equal(want[:, lo + cnt:], keys[:, lo + cnt:])
            kin = keys.cuda()
            out = torch.full((n, total), SENT, device="cuda")
            call("osd_level_topk", P(kin), P(out), n, total, lo, cnt, topn, ST())
            out = out.cpu()
            assert torch.equal(out[:, lo:lo + cnt], want[:, lo:lo + cnt]), (kind, topn)
            assert bool((out[:, :lo] == SENT).all()) and bool((out[:, lo + cnt:] == SENT).all()) and torch.equal(kin.cpu(), keys)
            ops().level_topk(kin, lo, cnt, topn)                       # keys_in == keys_out: the header promises aliasing
            assert torch.equal(kin.cpu(), want), (kind, topn, "aliased")


# =============================================================================================================== loss, algorithms
@pytest.mark.parametrize("n_levels", [1, 5])
def test_fcos_loss_finalize_scales_is_finalize_plus_the_scale_gradient(n_levels):
    for sums in ([37.0, 29.5, 11.25, 17.5, 21.75, 0, 0, 0], [37.0, 0.0, 11.25, 17.5, 21.75, 0, 0, 0], [0.0, 0.0, 3.5, 0.0, 0.0, 0, 0, 0]):
        sums = torch.tensor(sums, device="cuda")
        raw, scales = rnd(8, seed=121), rnd(8, seed=122).abs() + 0.5
        d0 = rnd(8, seed=123)
        a, b = torch.full((4,), SENT, device="cuda"), torch.full((4,), SENT, device="cuda")
        d, rawd, scd = d0.clone().cuda(), raw.cuda(), scales.cuda()
        call("osd_fcos_loss_finalize", P(sums), P(a), 2, ST())
        call("osd_fcos_loss_finalize_scales", P(sums), P(b), 2, P(rawd), P(scd), P(d), n_levels, ST())
        assert torch.equal(a.cpu(), b.cpu()) and bool(torch.isfinite(a).all())
        want = sr.finalize_scales(d0, raw, scales, n_levels)
        mag = d0.double().abs() + (raw.double() / scales.double()).abs()
        err = (d.cpu().double() - want)[:n_levels].abs() / (1e-6 * mag[:n_levels])
        note("fcos_loss_finalize_scales %d" % n_levels, worst=float(err.max()))
        assert float(err.max()) <= 1.0
        assert torch.equal(d.cpu()[n_levels:], d0[n_levels:])


def test_conv_algo_count_bounds_the_selectable_algorithms():
    from oneshotdet_amd import _lib
    count = _lib.load().osd_conv_algo_count()
    assert count > 0
    x = rnd(1, 4, 4, 64, seed=131).cuda()
    pc = ops().pack_conv((rnd(64, 64, 1, 1, seed=132) / 8).cuda(), dtype=torch.float32)
    ops().conv2d(x, pc)                                            # the plain 1x1 conv itself runs
    from oneshotdet_amd import tuner
    assert all(1 <= a <= count for a in tuner.conv_algo_candidates(64, False, pixels=16))
    for algo in list(range(count + 1, count + 66)) + [1000, 2 ** 20, 2 ** 31 - 1]:
        with pytest.raises(_lib.OsdError) as ei:
            ops().conv2d(x, pc, algo=algo)
        assert ei.value.code < 0, algo


# =============================================================================================================== forwarding entries
@BOTH
def test_plain_groupnorm_level_entries_are_the_fused_entries_with_no_fused_level(dt):
    """osd_groupnorm_relu_fwd_levels / _bwd_levels (the wrappers call the _fused forms with fused_mask = 0): outputs, saved
    statistics and input gradients bit-identical to those, d gamma / d beta (atomic adds) equal to the accumulation bar; fp32 also
    against autograd at the bar of test_groupnorm_relu_backward_with_zero_negative_and_tiny_scales (2e-4 of absmax)."""
    import ctypes as C
    import torch.nn.functional as F
    o = ops()
    n, c, groups, eps, sizes = 2, 256, 32, 1e-5, [(5, 7), (3, 4)]
    k = len(sizes)
    gamma, beta = rnd(c, seed=141).abs() + 0.5, rnd(c, seed=142)
    xs = [(rnd(n, h, w, c, seed=143 + i, scale=2.0) + 0.3).to(DT[dt]) for i, (h, w) in enumerate(sizes)]
    dts = [rnd(n, h, w, c, seed=147 + i).to(DT[dt]) for i, (h, w) in enumerate(sizes)]
    xd, dd, gd, bd = [x.cuda() for x in xs], [d.cuda() for d in dts], gamma.cuda(), beta.cuda()
    hws = (C.c_int32 * k)(*[h * w for h, w in sizes])
    pa = o._ptr_array

    def forward(fused):
        ys = [torch.empty_like(x) for x in xd]
        ab = torch.empty((k, 4, n, c), device="cuda")
        ws = torch.empty(k * n * 64 * groups * 2, device="cuda")
        args = (k, pa(xd), pa(ys), hws, P(gd), P(bd), P(ab), P(ws), n, c, groups, eps, DTC[dt])
        if fused:
            call("osd_groupnorm_relu_fwd_levels_fused", *args, 0, ST())
        else:
            call("osd_groupnorm_relu_fwd_levels", *args, ST())
        return ys, ab

    def backward(fused, ab):
        dus = [torch.empty_like(x) for x in xd]
        dg, db = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda")
        ws = torch.empty(k * n * 64 * (groups * 2 + 2 * c), device="cuda")
        args = (k, pa(xd), pa(dd), pa(dus), hws, P(ab), P(gd), P(bd), P(ws), P(dg), P(db), n, c, groups, DTC[dt])
        if fused:
            call("osd_groupnorm_relu_bwd_levels_fused", *args, 0, ST())
        else:
            call("osd_groupnorm_relu_bwd_levels", *args, ST())
        return dus, dg, db

    (y0, ab0), (y1, ab1) = forward(False), forward(True)
    assert torch.equal(ab0, ab1) and all(torch.equal(a, b) for a, b in zip(y0, y1))
    (du0, dg0, db0), (du1, dg1, db1) = backward(False, ab0), backward(True, ab0)
    assert all(torch.equal(a, b) for a, b in zip(du0, du1))
    cr.assert_accumulated(dg0, dg1.double(), what="d gamma")
    cr.assert_accumulated(db0, db1.double(), what="d beta")
    if dt == "f32":
        g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        for x, d, y, du in zip(xs, dts, y0, du0):
            xx = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
            ref = F.relu(F.group_norm(xx, groups, g, b, eps=eps))
            (ref * d.permute(0, 3, 1, 2)).sum().backward()
            assert float((y.cpu().permute(0, 3, 1, 2) - ref.detach()).abs().max()) <= 2e-4 * float(ref.abs().max())
            assert float((du.cpu().permute(0, 3, 1, 2) - xx.grad).abs().max()) <= 2e-4 * float(xx.grad.abs().max())
        assert float((dg0.cpu() - g.grad).abs().max()) <= 2e-4 * float(g.grad.abs().max())
        assert float((db0.cpu() - b.grad).abs().max()) <= 2e-4 * float(b.grad.abs().max())
