"""GPU: the prediction convs' fused backward launch (osd_conv2d_pred_bwd, include/oneshotdet_hip.h; ops.pred_bwd_fused):
data gradient + weight / bias gradient of a 3x3 conv with 2 or 4 outputs over all FPN levels in one launch that keeps the gathered
dy matrix G in LDS.  Bars: tests/conv_ref.py (one bf16 rounding of the float64 result for dX, ACC_TOL for the accumulated dW / db)."""
import ctypes as C

import pytest
import torch

import conv_ref as cr
import golden_utils as gu
from oracle import launch_replay as lr

pytestmark = pytest.mark.gpu

# levels down to 1 x 1 and 1 x 3 (every tap crosses the border), a level (7 x 8, two images) whose images end inside a 128-pixel tile,
# level boundaries inside a tile; 2,134 pixels = 8 workgroups of 272 pixels (two whole tiles and a 16-pixel one), the last with 230: its
# second tile ends inside an X stage and holds the end of level 1, levels 2, 3 and 4
SIZES = [(2, 25, 32), (2, 13, 16), (2, 7, 8), (1, 1, 3), (3, 1, 1)]
CASES = [(2, 256), (4, 256), (4, 512)]


def ops():
    from oneshotdet_amd import ops as o
    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


_CACHE = {}


def case(cout, cin):
    """inputs, today's path and the float64 references of one (cout, cin), computed once and left unchanged"""
    key = (cout, cin)
    if key in _CACHE:
        return _CACHE[key]
    o = ops()
    bf = torch.bfloat16
    dys, xs = [], []
    for i, (n, h, w) in enumerate(SIZES):
        d = rnd(n, h, w, 4, seed=10 + i)
        d[..., cout:] = 0.0                      # the channels past cout are stored as zeros by the loss kernel
        dys.append(d.to(bf).cuda())
        xs.append(rnd(n, h, w, cin, seed=20 + i).to(bf).cuda())
    master = (rnd(cout, 3, 3, cin, seed=1) / 48).cuda()          # [cout][3][3][cin] fp32
    wd = o.pred_dgrad_pack(master, cout, cin, bf)
    ent = o.PackedConv(wd, torch.zeros(cin, device="cuda"), cin, cin, cin, 64, 1, 1, cin_real=9 * cout)
    g = o.pred_dy_gather(dys, cout, cin)
    tot = g.shape[0]
    ref_dx = cr.conv_fwd(g.view(1, 1, tot, 64), lr.unpack_weight(wd, cin), None)          # float64, [1][1][tot][cin]
    ref_dw = torch.zeros((cout, 3, 3, cin), dtype=torch.float64, device="cuda")
    ref_db = torch.zeros((cout,), dtype=torch.float64, device="cuda")
    for x, d in zip(xs, dys):
        a, b = cr.conv_wgrad(x, d, 3, 3, 1, 1, cout, want_bias=True)
        ref_dw += a
        ref_db += b
    dw0 = rnd(cout, 3, 3, cin, seed=5).cuda()                       # non-zero start: the launch ADDS into dw / db
    db0 = rnd(cout, seed=6).cuda()
    # today's path: G in memory, the 1x1 conv over it, the weight gradient from it
    old_dx = o.conv2d(g.view(1, 1, tot, 64), ent).view(tot, cin)
    old_dw, old_db = dw0.clone(), db0.clone()
    o.conv2d_wgrad_grouped(list(zip(xs, dys)), old_dw, 3, 3, 1, 1, cout, db=old_db, g=g)
    _CACHE[key] = dict(xs=xs, dys=dys, ent=ent, tot=tot, ref_dx=ref_dx, ref_dw=ref_dw, ref_db=ref_db, dw0=dw0, db0=db0,
                       old_dx=old_dx, old_dw=old_dw, old_db=old_db)
    return _CACHE[key]


def run(c, cout, flags=0):
    o = ops()
    dw, db = c["dw0"].clone(), c["db0"].clone()
    dx = o.pred_bwd_fused(c["xs"], c["dys"], c["ent"], dw, db, cout, flags=flags)
    torch.cuda.synchronize()
    return dx, dw, db


def flat(dx):
    return torch.cat([t.reshape(-1, t.shape[-1]) for t in dx])


@pytest.mark.parametrize("cout,cin", CASES)
def test_fused_launch_against_float64(cout, cin):
    """dX: one bf16 rounding of the float64 1x1 conv over the G that osd_pred_dy_gather builds, with the unpacked Wd; dw / db: the
    float64 weight and bias gradient summed over the levels, added to a non-zero start."""
    c = case(cout, cin)
    dx, dw, db = run(c, cout)
    assert [tuple(t.shape) for t in dx] == [(n, h, w, cin) for n, h, w in SIZES]
    assert dx[0].data_ptr() + dx[0].numel() * 2 == dx[1].data_ptr()           # views of one buffer, the levels one after the other
    cr.assert_output(flat(dx).view(1, 1, c["tot"], cin), c["ref_dx"], what="fused dX")
    cr.assert_accumulated(dw - c["dw0"], c["ref_dw"], "fused dW")
    cr.assert_accumulated(db - c["db0"], c["ref_db"], "fused db")
    # the start values are still there: dw0 + gradient, not the gradient alone
    cr.assert_accumulated(dw, c["ref_dw"] + c["dw0"].double(), "fused dW + start")
    cr.assert_accumulated(db, c["ref_db"] + c["db0"].double(), "fused db + start")


@pytest.mark.parametrize("cout,cin", CASES)
def test_each_half_alone_gives_the_fused_launchs_bits_and_two_runs_are_equal(cout, cin):
    from oneshotdet_amd import _lib
    c = case(cout, cin)
    dx, dw, db = run(c, cout)
    dx2, dw2, db2 = run(c, cout)
    assert torch.equal(flat(dx), flat(dx2)) and torch.equal(dw, dw2) and torch.equal(db, db2)          # no atomics: same bits every run
    dxd, dwd, dbd = run(c, cout, _lib.PRED_BWD_DGRAD)
    assert torch.equal(flat(dxd), flat(dx))
    assert torch.equal(dwd, c["dw0"]) and torch.equal(dbd, c["db0"])          # the data-gradient half leaves dw / db alone
    dxw, dww, dbw = run(c, cout, _lib.PRED_BWD_WGRAD)
    assert dxw is None and torch.equal(dww, dw) and torch.equal(dbw, db)


def bf16_ulp(v):
    """the spacing of bf16 values at |v| (8 significant bits)"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -120))
    return torch.ldexp(torch.ones_like(v), e - 8)


@pytest.mark.parametrize("cout,cin", CASES)
def test_against_the_gathered_path(cout, cin):
    """The launches this one replaces (osd_pred_dy_gather + the K = 64 conv + osd_conv2d_wgrad_pred_gathered): dX within one bf16 ulp
    element by element (the same operands in the same K order: equality expected, the count of differing elements is printed), dw / db
    within the accumulated-gradient bar of each other."""
    c = case(cout, cin)
    dx, dw, db = run(c, cout)
    a, b = flat(dx).float(), c["old_dx"].float()
    diff = (a - b).abs()
    print("\ncout %d cin %d: %d of %d dX elements differ from the gathered path, worst %.3g ulp"
          % (cout, cin, int((diff > 0).sum()), a.numel(), float((diff / bf16_ulp(torch.maximum(a.abs(), b.abs()))).max())))
    assert bool((diff <= bf16_ulp(torch.maximum(a.abs(), b.abs()))).all())
    cr.assert_accumulated(dw - c["dw0"], (c["old_dw"] - c["dw0"]).double(), "dW against the gathered path")
    cr.assert_accumulated(db - c["db0"], (c["old_db"] - c["db0"]).double(), "db against the gathered path")


def test_unsupported_shapes_return_the_documented_codes():
    """fp32 and cin % 256 != 0 and cout > 4: OSD_ERR_UNSUPPORTED (-2); more than six levels: OSD_ERR_INVALID_ARG (-1).  Nothing is
    launched (dw stays as it was), through ctypes."""
    from oneshotdet_amd import _lib
    o = ops()
    lib = _lib.load()

    def call(dtype, cin, cout, k):
        x = torch.zeros((1, 4, 4, cin), device="cuda", dtype=dtype)
        dy = torch.zeros((1, 4, 4, 8), device="cuda", dtype=dtype)
        wd = torch.zeros((cin, 64), device="cuda", dtype=dtype)
        dx = torch.zeros((16 * k, cin), device="cuda", dtype=dtype)
        dw = torch.ones((cout, 3, 3, cin), device="cuda")
        wsp = torch.zeros((1 << 20,), device="cuda")
        d = o._conv_desc(x.shape, o._dt(x), cout, 3, 3, 1, 1, dy.shape[-1])
        xs = (C.c_void_p * k)(*[x.data_ptr()] * k)
        dys = (C.c_void_p * k)(*[dy.data_ptr()] * k)
        ns, hs, ws = (C.c_int32 * k)(*[1] * k), (C.c_int32 * k)(*[4] * k), (C.c_int32 * k)(*[4] * k)
        rc = lib.osd_conv2d_pred_bwd(C.byref(d), k, xs, dys, ns, hs, ws, wd.data_ptr(), dx.data_ptr(), dw.data_ptr(), None,
                                     wsp.data_ptr(), 0, None)
        torch.cuda.synchronize()
        assert rc == 0 or bool((dw == 1).all())
        return rc
    assert call(torch.bfloat16, 256, 4, 2) == 0
    assert call(torch.float32, 256, 4, 2) == -2
    assert call(torch.bfloat16, 192, 4, 2) == -2
    assert call(torch.bfloat16, 256, 5, 2) == -2
    assert call(torch.bfloat16, 256, 4, 7) == -1
    assert lib.osd_last_error_string()
    assert lib.osd_pred_bwd_workspace_bytes(7, None, None, None, 256, 4) == 0
    assert not o.pred_bwd_fused_ok(torch.float32, 4, 3, 3, 1, 1, 256, 5) and o.pred_bwd_fused_ok(torch.bfloat16, 2, 3, 3, 1, 1, 256, 5)


def test_training_step_with_the_fused_launch_equals_the_gathered_step(monkeypatch):
    """TrainEngine.pred_bwd_fused (OSD_PRED_BWD_FUSED, read when the engine is built): one bf16 forward_backward of the `small` golden
    case on the gathered path, then on the fused launch, in fresh engines.  The forward pass is the same; the backward differs by the
    weight gradients' summation order and at most single-ulp roundings of the prediction convs' data gradient, re-rounded by the
    layers behind it.  Bars: those of test_gpu_train.py:898-901 for two bf16 backward passes that differ in this way (losses rtol
    1e-5; relative L2 per gradient bucket: head <= 1e-4, every bucket <= 1e-2)."""
    import numpy as np
    from oneshotdet_amd import _lib, spec, synth, train
    B, H, W, S, qh, qw = gu.CASES["small"]
    img, q = gu.case_inputs("small")
    gts = synth.make_gt_boxes(B, H, W, seed=3, max_boxes=3)
    gtb = torch.zeros(B, max(len(g) for g in gts), 4)
    for i, g in enumerate(gts):
        gtb[i, :len(g)] = torch.from_numpy(g)
    cnt = torch.tensor([len(g) for g in gts], dtype=torch.int32).cuda()
    img, q, gtb = torch.from_numpy(img).cuda(), torch.from_numpy(q).cuda(), gtb.cuda()
    out = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("OSD_PRED_BWD_FUSED", fused)
        eng = train.TrainEngine(synth.make_state_dict(spec.hot_path_shapes()), dtype=torch.bfloat16)
        assert eng.pred_bwd_fused == (fused == "1")
        calls = []
        real = _lib.call

        def spy(name, *a):
            calls.append(name)
            return real(name, *a)
        _lib.call = spy
        try:
            losses = eng.forward_backward(img, q, gtb, cnt).clone()
        finally:
            _lib.call = real
        torch.cuda.synchronize()
        assert calls.count("osd_conv2d_pred_bwd") == (2 if fused == "1" else 0)           # one launch per tower
        assert calls.count("osd_pred_dy_gather") == (0 if fused == "1" else 2)            # outside a trace no G is built
        out[fused] = (losses, eng.flat_g.clone(), dict(eng.exchange.ranges))
    torch.testing.assert_close(out["1"][0], out["0"][0], rtol=1e-5, atol=0)
    g0, g1 = out["0"][1], out["1"][1]
    errs = {name: float((g1[lo:hi] - g0[lo:hi]).norm() / g0[lo:hi].norm()) for name, (lo, hi) in out["0"][2].items()}
    print("\nfused vs gathered prediction-conv backward, relative L2 per gradient bucket:", {k: "%.1e" % v for k, v in errs.items()})
    assert np.isfinite(list(errs.values())).all()
    assert errs["head"] <= 1e-4 and max(errs.values()) <= 1e-2, errs
