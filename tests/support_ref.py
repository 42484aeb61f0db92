"""High-precision restatements of the support kernels behind include/oneshotdet_hip.h: weight packers, the table-driven SGD
update, the strided data gradient, the element-wise backward kernels, layout changes, proposal scoring and the per-level top-k.

Style of tests/conv_ref.py: plain torch, runnable on the CPU and on the GPU.  Where an operation is ONE fp32 operation and one
rounding (the packers, scatter / add / mask, box decode, layout changes) the restatement does that operation in fp32 and is meant
to be compared with `torch.equal`; where sums or transcendental functions are involved (the data gradient, column sums, the SGD
recurrence, sigmoid scores) it computes in float64 and the caller applies conv_ref's bounds.

The device tables of the table-driven entry points are written here from the struct layouts documented in the header comment
(not from the training engine's own table builder): the tests check the ABI as it is documented.
"""
import struct

import numpy as np
import torch

from oracle import launch_replay as lr

# re-exported: these launches already have a restatement in the launch replay
scatter2x = lr.scatter2x_launch            # (src, (h, w), mask=None, addend=None): add first, then mask
add_mask = lr.add_mask_launch              # (a, b=None, mask=None)
unpack_weight = lr.unpack_weight

SGD_RTOL, SGD_ATOL = 1e-6, 1e-7            # parameters / momentum after SGD steps (the bar of test_fused_sgd_matches_torch_optim)


def round_dtype(t, dtype):
    """One round-to-nearest-even of an fp32 tensor to `dtype` (identity for float32)."""
    return t.float().to(dtype)


# ------------------------------------------------------------------------------------------------------------ device tables
PACK_ENTRY = struct.Struct("<qqq8i")       # int64 src_off, dst_off, scale_off; int32 cout, cin, r, s, rows, kpad, first_block, n_blocks
SGD_ENTRY = struct.Struct("<qqff2i")       # int64 off, numel; float lr_mult, wd; int32 first_block, n_blocks
SGD_PACK_ENTRY = struct.Struct("<qqff2iqq4i")   # ... ; int64 dst_off, scale_off; int32 cin, rs, kpad, pad
assert (PACK_ENTRY.size, SGD_ENTRY.size, SGD_PACK_ENTRY.size) == (56, 32, 64)


def _blocks(entries):
    """entries: dicts with `n_blocks` -> (first_block per entry, block_entry list): workgroup b serves entry block_entry[b]."""
    first, owner = [], []
    for i, e in enumerate(entries):
        first.append(len(owner))
        owner += [i] * int(e["n_blocks"])
    return first, owner


def _table(raw, owner, device):
    t = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).to(device)
    return t, torch.tensor(owner, dtype=torch.int32, device=device), len(owner)


def pack_table(entries, device="cpu"):
    """PackEntry table of osd_pack_multi.  entries: dicts src_off, dst_off, scale_off, cout, cin, r, s, rows, kpad, n_blocks.
    -> (table uint8 tensor, block_entry int32 tensor, n_blocks)."""
    first, owner = _blocks(entries)
    raw = b"".join(PACK_ENTRY.pack(e["src_off"], e["dst_off"], e["scale_off"], e["cout"], e["cin"], e["r"], e["s"], e["rows"], e["kpad"],
                                   f, e["n_blocks"]) for e, f in zip(entries, first))
    return _table(raw, owner, device)


def sgd_table(entries, device="cpu"):
    """SgdEntry table of osd_sgd_momentum_multi.  entries: dicts off, numel, lr_mult, wd, n_blocks."""
    first, owner = _blocks(entries)
    raw = b"".join(SGD_ENTRY.pack(e["off"], e["numel"], e["lr_mult"], e["wd"], f, e["n_blocks"]) for e, f in zip(entries, first))
    return _table(raw, owner, device)


def sgd_pack_table(entries, device="cpu"):
    """SgdPackEntry table of osd_sgd_momentum_pack_multi.  entries: as sgd_table plus dst_off (-1: update only), scale_off (-1: none),
    cin, rs, kpad (ignored when dst_off < 0)."""
    first, owner = _blocks(entries)
    raw = b"".join(SGD_PACK_ENTRY.pack(e["off"], e["numel"], e["lr_mult"], e["wd"], f, e["n_blocks"], e.get("dst_off", -1),
                                       e.get("scale_off", -1), e.get("cin", 0), e.get("rs", 0), e.get("kpad", 0), 0)
                   for e, f in zip(entries, first))
    return _table(raw, owner, device)


# ------------------------------------------------------------------------------------------------------------ weight packers
def _scaled(w_orsi, scale):
    w = w_orsi.float()
    return w if scale is None else w * scale.float().view(-1, 1, 1, 1)        # ONE fp32 multiplication


def pack_fwd(w_orsi, scale, rows, kpad, dtype):
    """osd_pack_conv_weight_ex (src_orsi = 1) / osd_pack_multi (dgrad = 0): master [cout][r][s][cin] fp32 (x per-cout scale) ->
    [rows >= cout][r][s][kpad >= cin] of `dtype`, zero padded."""
    cout, r, s, cin = w_orsi.shape
    out = torch.zeros((rows, r, s, kpad), dtype=dtype, device=w_orsi.device)
    out[:cout, :, :, :cin] = round_dtype(_scaled(w_orsi, scale), dtype)
    return out


def pack_dgrad(w_orsi, scale, rows, kpad, dtype):
    """osd_pack_conv_weight_dgrad (src_orsi = 1) / osd_pack_multi (dgrad = 1): Wd[ci][r'][s'][co] = w[co][R-1-r'][S-1-s'][ci] * scale[co],
    [rows >= cin][r][s][kpad >= cout] of `dtype`, zero padded."""
    cout, r, s, cin = w_orsi.shape
    out = torch.zeros((rows, r, s, kpad), dtype=dtype, device=w_orsi.device)
    out[:cin, :, :, :cout] = round_dtype(_scaled(w_orsi, scale).flip(1, 2).permute(3, 1, 2, 0), dtype)
    return out


def pack_multi(entries, src, scales, dst, dgrad):
    """osd_pack_multi on flat buffers: writes every entry's packed tensor into (a copy of) `dst` and returns it."""
    out = dst.clone()
    for e in entries:
        numel = e["cout"] * e["r"] * e["s"] * e["cin"]
        w = src[e["src_off"]:e["src_off"] + numel].view(e["cout"], e["r"], e["s"], e["cin"])
        sc = None if e["scale_off"] < 0 else scales[e["scale_off"]:e["scale_off"] + e["cout"]]
        p = (pack_dgrad if dgrad else pack_fwd)(w, sc, e["rows"], e["kpad"], dst.dtype)
        out[e["dst_off"]:e["dst_off"] + p.numel()] = p.reshape(-1)
    return out


def unpack_wgrad(dw_packed, scale, grad_oihw=None):
    """osd_unpack_wgrad: packed fp32 dW [cout][r][s][cin] -> OIHW, times scale[co] (one fp32 multiplication), added to grad_oihw
    (one fp32 addition) when given."""
    v = dw_packed.float().permute(0, 3, 1, 2).contiguous()
    if scale is not None:
        v = v * scale.float().view(-1, 1, 1, 1)
    return v if grad_oihw is None else grad_oihw.float() + v


# ------------------------------------------------------------------------------------------------------------ SGD
def _f32(x):
    return float(np.float32(x))         # the ABI passes lr, momentum, lr_mult and wd as C floats


def sgd_steps(entries, params, grads, lr, momentum, n_steps=None):
    """The header's update rule in float64 over flat buffers: g += wd * p; buf = g on the first step, else momentum * buf + g;
    p -= lr * lr_mult * buf.  grads: one flat gradient per step.  Elements outside every entry are left alone.
    -> (params, momentum) float64 after the steps (momentum starts undefined: the first step overwrites it)."""
    p = params.double().clone()
    buf = torch.zeros_like(p)
    for k, g in enumerate(grads[:n_steps]):
        g = g.double()
        for e in entries:
            sl = slice(e["off"], e["off"] + e["numel"])
            d = g[sl] + _f32(e["wd"]) * p[sl]
            buf[sl] = d if k == 0 else _f32(momentum) * buf[sl] + d
            p[sl] = p[sl] - (_f32(lr) * _f32(e["lr_mult"])) * buf[sl]
    return p, buf


# ------------------------------------------------------------------------------------------------------------ gradients
def bias_grad(dy, c, db0=None):
    """osd_bias_grad: db[ch] (+)= sum over rows of dy[m][ch], ch < c; dy [m][stride >= c].  float64."""
    s = dy.double()[:, :c].sum(0)
    return s if db0 is None else s + db0.double()


def dgrad_naive(dy, w_oihw, x_shape, stride, pad, mask=None, addend=None):
    """osd_conv2d_dgrad_naive in float64: the gradient of conv(x; w, stride, pad) w.r.t. x given dy, THEN the ReLU mask
    (mask > 0 ? . : 0), THEN the addend.  dy NHWC [n][ho][wo][>= cout], w OIHW [cout][cin][r][s], x_shape (n, h, w, cin)."""
    n, h, wd, cin = x_shape
    cout, _, r, s = w_oihw.shape
    g = dy.double()[..., :cout]
    ho, wo = g.shape[1], g.shape[2]
    wk = w_oihw.to(g.device).double()
    hp, wp = max(h + 2 * pad, stride * (ho - 1) + r), max(wd + 2 * pad, stride * (wo - 1) + s)
    dx = torch.zeros((n, hp, wp, cin), dtype=torch.float64, device=g.device)
    for i in range(r):
        for j in range(s):
            dx[:, i:i + stride * (ho - 1) + 1:stride, j:j + stride * (wo - 1) + 1:stride, :] += torch.matmul(g, wk[:, :, i, j])
    dx = dx[:, pad:pad + h, pad:pad + wd, :]
    if mask is not None:
        dx = torch.where(mask.to(g.device).double() > 0, dx, torch.zeros_like(dx))
    if addend is not None:
        dx = dx + addend.to(g.device).double()
    return dx


def upsample2x_bwd(inner, prev=None):
    """osd_upsample2x_bwd in float64: top[n, y, x] = prev[n, y, x] + the 2 x 2 sum of inner[n, 2y.., 2x..]; inner exactly twice top's size."""
    t = inner.double()
    assert t.shape[1] % 2 == 0 and t.shape[2] % 2 == 0
    y = t[:, 0::2, 0::2] + t[:, 0::2, 1::2] + t[:, 1::2, 0::2] + t[:, 1::2, 1::2]
    return y if prev is None else y + prev.double()


# ------------------------------------------------------------------------------------------------------------ layouts
def nhwc_to_nchw(x, c0=0, c=None):
    """osd_nhwc_to_nchw_f32: channels [c0, c0 + c) of an NHWC tensor -> NCHW fp32 (a copy: bf16 -> fp32 is exact)."""
    c = x.shape[-1] - c0 if c is None else c
    return x[..., c0:c0 + c].float().permute(0, 3, 1, 2).contiguous()


def nchw_to_nhwc(x, dtype):
    """osd_nchw_f32_to_nhwc: NCHW fp32 -> dense NHWC `dtype` (one rounding)."""
    return round_dtype(x.permute(0, 2, 3, 1).contiguous(), dtype)


# ------------------------------------------------------------------------------------------------------------ proposals
def score_decode(cls_ctr, reg, stride, img_h, img_w, img_hw=None):
    """osd_fcos_score_decode(_sizes) for one level, from the header comment: score = sigmoid(logit) * sigmoid(centerness), -1 where
    the fp32 sigmoid of the logit is not > 0 (the candidate test); location (x, y) = (j * stride + stride // 2, i * stride +
    stride // 2); box = (x - l, y - t, x + r, y + b), each coordinate clipped to [0, width - 1] / [0, height - 1] of its image
    (img_hw [n][2] = (height, width) per image, else img_h / img_w).  cls_ctr [n][h][w][>= 2], reg [n][h][w][>= 4].
    -> (scores float64 [n][h * w], dropped bool [n][h * w], boxes fp32 [n][h * w][4])."""
    n, h, w, _ = cls_ctr.shape
    dev = cls_ctr.device
    lg, ct = cls_ctr[..., 0].reshape(n, -1), cls_ctr[..., 1].reshape(n, -1)
    dropped = ~(torch.sigmoid(lg.float()) > 0)
    scores = torch.sigmoid(lg.double()) * torch.sigmoid(ct.double())
    scores = torch.where(dropped, torch.full_like(scores, -1.0), scores)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    lx = (xs * stride + stride // 2).float().reshape(1, -1)
    ly = (ys * stride + stride // 2).float().reshape(1, -1)
    d = reg[..., :4].float().reshape(n, -1, 4)
    if img_hw is None:
        hh = torch.full((n, 1), float(img_h), dtype=torch.float32, device=dev)
        ww = torch.full((n, 1), float(img_w), dtype=torch.float32, device=dev)
    else:
        hh, ww = img_hw.float()[:, 0:1].to(dev), img_hw.float()[:, 1:2].to(dev)

    def clip(v, hi):
        return torch.minimum(v.clamp_min(0.0), hi - 1.0)
    boxes = torch.stack([clip(lx - d[..., 0], ww), clip(ly - d[..., 1], hh), clip(lx + d[..., 2], ww), clip(ly + d[..., 3], hh)], dim=-1)
    return scores, dropped, boxes


def level_topk(keys, lo, cnt, topn):
    """osd_level_topk: within keys[img][lo, lo + cnt) the `topn` largest (ties: lower index first) keep their key, the rest get -1;
    an entry that is already negative stays dropped.  keys [n][total] fp32 -> a new tensor."""
    out = keys.clone()
    for img in range(keys.shape[0]):
        k = keys[img, lo:lo + cnt]
        rank = torch.zeros(cnt, dtype=torch.int64, device=keys.device)
        for i0 in range(0, cnt, 512):           # rank[i] = number of j before i: k[j] > k[i], or equal and j < i
            ki = k[i0:i0 + 512, None]
            idx = torch.arange(i0, min(cnt, i0 + 512), device=keys.device)[:, None]
            j = torch.arange(cnt, device=keys.device)[None, :]
            rank[i0:i0 + 512] = ((k[None, :] > ki) | ((k[None, :] == ki) & (j < idx))).sum(1)
        keep = (rank < topn) & (k >= 0)
        out[img, lo:lo + cnt] = torch.where(keep, k, torch.full_like(k, -1.0))
    return out


# ------------------------------------------------------------------------------------------------------------ loss
def finalize_scales(d_scales0, d_scale_raw, scales, n_levels):
    """osd_fcos_loss_finalize_scales: d_scales[l] = d_scales0[l] + d_scale_raw[l] / scales[l] for l < n_levels.  float64."""
    out = d_scales0.double().clone()
    out[:n_levels] += d_scale_raw.double()[:n_levels] / scales.double()[:n_levels]
    return out
