"""float64 reference of one convolution / weight-gradient launch, and the bounds the kernel tests hold the kernels to.

Every conv kernel of the library multiplies operands that are already rounded to its dtype and accumulates in fp32, so the
only legitimate differences from an exact result are fp32 summation order and ONE final rounding to the output dtype.  The
reference below computes the same expression exactly enough to stand for "exact" (float64: 29 more bits than fp32) and is
written as a sum over the filter taps of shifted `torch.matmul` calls, so that it runs on the GPU as well (there are no
float64 convolutions there; float64 GEMMs are always there): the benchmark-sized launches take seconds instead of minutes.

Layouts are the kernels' own: activations NHWC, weights OIHW as `oracle.launch_replay.unpack_weight` returns them from the
packed tensor (FrozenBN already folded in, already rounded to the kernel's dtype), weight gradients [cout][r][s][cin].

Bounds (one definition for every test):
  outputs (bf16 and fp32)      `check_output`: oracle.launch_replay.compare, the launch replay's bar — bf16: every element within
                               one bf16 ulp of the rounded reference + 1e-5 x absmax, at most FLIP_CAP of the elements on the
                               neighbouring value; fp32: 1e-4 |ref| + 1e-5 x absmax
  accumulated gradients        `check_accumulated`: max |got - ref| <= ACC_TOL x absmax(ref) and cosine >= ACC_COS (dW, db: fp32
                               sums over up to 4 x 10^5 pixels; fp32 summation order alone differs from float64 by ~2e-6 of absmax,
                               one pixel dropped from 4 x 10^5 by ~4e-4)."""
import torch
import torch.nn.functional as F

from oracle import launch_replay as lr

ACT_NONE, ACT_RELU, ACT_EXP_SCALE = lr.ACT_NONE, lr.ACT_RELU, lr.ACT_EXP_SCALE
RES_NONE, RES_SAME, RES_UP2X, RES_DOWN2X = lr.RES_NONE, lr.RES_SAME, lr.RES_UP2X, lr.RES_DOWN2X

FLIP_CAP = 0.02         # bf16 outputs: at most this fraction of the elements on the neighbouring bf16 value
ACC_TOL = 2e-5          # accumulated fp32 gradients: max |got - ref| / absmax(ref) (MI355X: <= 1.8e-6 over every weight-gradient
                        # variant at 409,600 pixels and over the bs = 8 training step)
ACC_COS = 0.99999


def _out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def _taps(x, r, s, stride, pad, ho, wo):
    """x NHWC float64 -> [(i, j, the [n, ho, wo, c] input pixels that filter tap (i, j) of every output pixel reads)]."""
    if pad:
        x = F.pad(x, (0, 0, pad, pad, pad, pad))
    for i in range(r):
        for j in range(s):
            yield i, j, x[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride, :]


def conv_fwd(x, w, bias=None, stride=1, pad=0, res=None, res_mode=RES_NONE, mask=None, act=ACT_NONE, act_scale=1.0, relu_in=False,
             x2=None, w2=None, x2_stride=1, out_hw=None):
    """One forward-conv launch in float64 (osd_conv2d_fwd and its grouped / multi forms, forward or data-gradient use alike):
    act(mask > 0 ? x (*) w + bias + residual : 0).  x NHWC (channels past w's input channels are ignored), w OIHW [cout, cin, r, s]
    (cin <= x's channels), bias [>= cout], res NHWC (RES_SAME: the output's size; RES_UP2X: half of it, nearest 2x; RES_DOWN2X:
    read at (2 ho, 2 wo)), mask NHWC (the output's geometry), relu_in: ReLU on x first.  x2 / w2 (1x1 convs): a second pixel source
    read at (ho * x2_stride, wo * x2_stride) with its own weights [cout, cin2, 1, 1].  out_hw crops the output (the stem, whose
    packed image is wider than its output needs).  Returns NHWC float64 [n, ho, wo, cout] before any rounding."""
    dev = x.device
    xd = x.double()
    if relu_in:
        xd = xd.clamp_min(0.0)
    cout, cin, r, s = w.shape
    xd = xd[..., :cin]
    n, h, wd, _ = xd.shape
    ho, wo = _out_size(h, r, stride, pad), _out_size(wd, s, stride, pad)
    if out_hw is not None:
        ho, wo = out_hw
    wk = w.to(dev).double()
    y = torch.zeros((n, ho, wo, cout), dtype=torch.float64, device=dev)
    for i, j, xs in _taps(xd, r, s, stride, pad, ho, wo):
        y += torch.matmul(xs[:, :ho, :wo], wk[:, :, i, j].t())
    if x2 is not None:
        c2 = w2.shape[1]
        xs2 = x2.double()[:, ::x2_stride, ::x2_stride, :c2][:, :ho, :wo]
        y += torch.matmul(xs2, w2.to(dev).double()[:, :, 0, 0].t())
    if bias is not None:
        y += bias.to(dev).double()[:cout]
    if res_mode == RES_SAME:
        y += res.double()[..., :cout]
    elif res_mode == RES_UP2X:
        y += res.double()[..., :cout].repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :ho, :wo]
    elif res_mode == RES_DOWN2X:
        y += res.double()[:, ::2, ::2, :cout][:, :ho, :wo]
    if mask is not None:
        y = torch.where(mask[..., :cout] > 0, y, torch.zeros_like(y))
    if act == ACT_RELU:
        y = y.clamp_min(0.0)
    elif act == ACT_EXP_SCALE:
        y = torch.exp(y * float(act_scale))
    return y


def conv_wgrad(x, dy, r, s, stride, pad, cout, scale=None, want_bias=False):
    """The weight gradient of conv(x; w * scale) w.r.t. w in float64 (osd_conv2d_wgrad and its grouped / batched / multi / mixed
    forms, per (x, dy) pair): dW[co][i][j][ci] = scale[co] * sum over output pixels m of dy[m][co] * x[m @ tap (i, j)][ci];
    db[co] = sum over m of dy[m][co].  x, dy NHWC (dy may store more than cout channels).  -> (dW [cout, r, s, cin], db or None)."""
    dev = x.device
    xd = x.double()
    n, h, wd, cin = xd.shape
    ho, wo = _out_size(h, r, stride, pad), _out_size(wd, s, stride, pad)
    g = dy.to(dev).double()[..., :cout].reshape(-1, cout)
    dw = torch.zeros((cout, r, s, cin), dtype=torch.float64, device=dev)
    for i, j, xs in _taps(xd, r, s, stride, pad, ho, wo):
        dw[:, i, j, :] = torch.matmul(g.t(), xs.reshape(-1, cin))
    if scale is not None:
        dw *= scale.to(dev).double()[:cout].view(-1, 1, 1, 1)
    return dw, (g.sum(0) if want_bias else None)


def check_output(got, ref, dtype=None, flip_cap=FLIP_CAP):
    """got: what a kernel stored (any layout, any float dtype); ref: the exact result (float64) in the same layout.  -> the dict of
    oracle.launch_replay.compare, `ok` also requiring at most `flip_cap` of a bf16 tensor's elements on the neighbouring value."""
    dtype = got.dtype if dtype is None else dtype
    res = lr.compare(got.detach().float().cpu(), ref.detach().float().cpu(), dtype)
    res["ok"] = bool(res["ok"]) and res["flips"] <= flip_cap
    return res


def assert_output(got, ref, dtype=None, what=""):
    res = check_output(got, ref, dtype)
    assert res["ok"], (what, {k: v for k, v in res.items()})
    return res


def check_accumulated(got, ref, tol=ACC_TOL, cos_min=ACC_COS):
    """got: an accumulated fp32 gradient (dW or db) a launch wrote; ref: the float64 sum.  -> dict(ok, err = max |got - ref| /
    absmax(ref), cos)."""
    g, r = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    scale = float(r.abs().max()) if r.numel() else 0.0
    if scale == 0.0:
        return dict(ok=float(g.abs().max()) == 0.0 if g.numel() else True, err=0.0, cos=1.0)
    if not bool(torch.isfinite(g).all()):
        return dict(ok=False, err=float("inf"), cos=0.0)
    err = float((g - r).abs().max()) / scale
    cos = float((g * r).sum() / (g.norm() * r.norm()).clamp_min(1e-300))
    return dict(ok=err <= tol and cos >= cos_min, err=err, cos=cos)


def assert_accumulated(got, ref, what="", tol=ACC_TOL):
    res = check_accumulated(got, ref, tol=tol)
    assert res["ok"], (what, res)
    return res
