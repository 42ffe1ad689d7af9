"""Torch constructions, float64 oracles and derived bounds for the
Deconvolution layer and its depth-to-space GPU route.  Shared by
test_deconv.py (CPU) and test_deconv_gpu.py (GPU).

Notation (ops/csrc/d2s.hip): x[N][Ci][H][W], caffe weight Wd[Ci][Co][R][S],
stride st, R' = ceil(R/st), S' = ceil(S/st), H' = H+R'-1, W' = W+S'-1.

Bounds, in the notation of _bf16_bounds.py (u = 2^-8, e = 2^-24); none is
taken from a kernel's output.

 y, dx  bf16 x bf16 products are exact in fp32.  An output stored as
        bf16(fp32 sum of K terms + bias) is within (u + 2(K+2)e)*T of the
        float64 value, T = sum|a||w| + |b|.  The factor 2 on the
        accumulation term allows for an MFMA accumulate that is not
        round-to-nearest; it stays far below u for these K.  ReLU is
        1-Lipschitz, so the bound holds after it.
 col2im The fallback rounds three times instead of once: every tap's
        partial sum to bf16 (the dcol matrix), their fp32 sum to bf16
        (col2im), and that plus the bf16-rounded bias to bf16 again.  Each
        rounding is relative to a quantity bounded by (1+u)^2 T, and the
        bias rounding adds u|b| <= uT: (4u + 3u^2 + 2(K+2)e)*T with K the
        per-tap depth plus the taps summed.
 dW, db fp32 outputs of fp32 accumulations: 2(K+2)e*T, K = N*H*W terms for
        dW (T = sum|x||dy|) and N*Ho*Wo for db (T = sum|dy|).
"""

import torch
import torch.nn.functional as F

U = 2.0 ** -8
E32 = 2.0 ** -24
BF = torch.bfloat16


def pad32(k):
    return (k + 31) // 32 * 32


def pad128(k):
    return (k + 127) // 128 * 128


def d2s_dims(R, S, st, Ci):
    Rp, Sp = -(-R // st), -(-S // st)
    return Rp, Sp, Rp * Sp * Ci, max(64, pad32(Rp * Sp * Ci))


def out_dim(h, k, st, p, dil=1):
    return st * (h - 1) + dil * (k - 1) + 1 - 2 * p


def pack_weight(wd, st, rows=None, kpad=None):
    """wrD[(py*st+px)*Co + co][(r'*S'+s')*Ci + ci] =
    Wd[ci][co][py + st*(R'-1-r')][px + st*(S'-1-s')], zero for a phantom
    tap; optionally embedded in a zero [rows][kpad] buffer."""
    Ci, Co, R, S = wd.shape
    Rp, Sp, kcol, _ = d2s_dims(R, S, st, Ci)
    wp = torch.zeros(Ci, Co, Rp * st, Sp * st, dtype=wd.dtype)
    wp[:, :, :R, :S] = wd
    # r = j*st + py with j = R'-1-r': flip the j axes
    v = wp.reshape(Ci, Co, Rp, st, Sp, st).flip(2, 4)
    live = v.permute(3, 5, 1, 2, 4, 0).reshape(st * st * Co, kcol)
    if rows is None:
        return live
    out = torch.zeros(rows, kpad, dtype=wd.dtype)
    out[:st * st * Co, :kcol] = live
    return out


def pack_weight_brute(wd, st):
    """The definition, element by element."""
    Ci, Co, R, S = wd.shape
    Rp, Sp, kcol, _ = d2s_dims(R, S, st, Ci)
    out = torch.zeros(st * st * Co, kcol, dtype=wd.dtype)
    for py in range(st):
        for px in range(st):
            for co in range(Co):
                for rp in range(Rp):
                    for sp in range(Sp):
                        r = py + st * (Rp - 1 - rp)
                        s = px + st * (Sp - 1 - sp)
                        if r >= R or s >= S:
                            continue
                        for ci in range(Ci):
                            out[(py * st + px) * Co + co,
                                (rp * Sp + sp) * Ci + ci] = wd[ci, co, r, s]
    return out


def unpack(z, Co, st, ph, pw, Ho, Wo):
    """y[n][co][oh][ow] = Z[n][(oh+ph)/st][(ow+pw)/st]
    [(((oh+ph)%st)*st + (ow+pw)%st)*Co + co]; z is [N][H'][W'][st*st*Co]."""
    N, Hp, Wp, _ = z.shape
    full = z.reshape(N, Hp, Wp, st, st, Co).permute(0, 5, 1, 3, 2, 4) \
        .reshape(N, Co, Hp * st, Wp * st)
    return full[:, :, ph:ph + Ho, pw:pw + Wo]


def d2s_route(x, wd, b, st, ph, pw):
    """pack -> stride-1 F.conv2d -> unpack, in x's dtype."""
    N, Ci, H, W = x.shape
    _, Co, R, S = wd.shape
    Rp, Sp, _, _ = d2s_dims(R, S, st, Ci)
    wr = pack_weight(wd, st).reshape(st * st * Co, Rp, Sp, Ci) \
        .permute(0, 3, 1, 2)
    z = F.conv2d(x, wr, None if b is None else b.repeat(st * st),
                 padding=(Rp - 1, Sp - 1))
    return unpack(z.permute(0, 2, 3, 1).contiguous(), Co, st, ph, pw,
                  out_dim(H, R, st, ph), out_dim(W, S, st, pw))


def as_pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def make_inputs(N, Ci, Co, H, W, k, s, p, seed, groups=1, dil=1, bias=True):
    """bf16-rounded x, Wd, dy and the fp32 bias of one deconvolution."""
    g = torch.Generator().manual_seed(seed)
    R, S = as_pair(k)
    sh, sw = as_pair(s)
    ph, pw = as_pair(p)
    x = torch.randn(N, Ci, H, W, generator=g).to(BF)
    w = (torch.randn(Ci, Co // groups, R, S, generator=g) * 0.25).to(BF)
    b = torch.randn(Co, generator=g) if bias else None
    Ho, Wo = out_dim(H, R, sh, ph, dil), out_dim(W, S, sw, pw, dil)
    dy = torch.randn(N, Co, Ho, Wo, generator=g).to(BF)
    return dict(x=x, w=w, b=b, dy=dy, stride=(sh, sw), pad=(ph, pw),
                dilation=(dil, dil), groups=groups)


def forward_oracle(inp, relu, route):
    """float64 y and its bound; route "d2s" or "col2im"."""
    x, w = inp["x"].double(), inp["w"].double()
    b = inp["b"].double() if inp["b"] is not None else None
    kw = dict(stride=inp["stride"], padding=inp["pad"],
              dilation=inp["dilation"], groups=inp["groups"])
    y = F.conv_transpose2d(x, w, b, **kw)
    t = F.conv_transpose2d(x.abs(), w.abs(), None if b is None else b.abs(),
                           **kw)
    Ci, Cog, R, S = w.shape
    cig = Ci // inp["groups"]
    if route == "d2s":
        st = inp["stride"][0]
        K = -(-R // st) * -(-S // st) * Ci
        tol = (U + 2 * (K + 2) * E32) * t
    else:
        K = cig + R * S
        tol = (4 * U + 3 * U * U + 2 * (K + 2) * E32) * t
    if relu:
        y = y.clamp_min(0)
    return y, tol


def backward_oracle(inp):
    """float64 (dx, dW, db) with bounds.  dx is the bf16 output of a
    convolution over dy with K = R*S*Co/G terms."""
    x, w, dy = inp["x"].double(), inp["w"].double(), inp["dy"].double()
    kw = dict(stride=inp["stride"], padding=inp["pad"],
              dilation=inp["dilation"], groups=inp["groups"])
    Ci, Cog, R, S = w.shape
    dx = F.conv2d(dy, w, None, **kw)
    tdx = F.conv2d(dy.abs(), w.abs(), None, **kw)
    dw = torch.nn.grad.conv2d_weight(dy, list(w.shape), x, **kw)
    tdw = torch.nn.grad.conv2d_weight(dy.abs(), list(w.shape), x.abs(), **kw)
    db = dy.sum(dim=(0, 2, 3))
    tdb = dy.abs().sum(dim=(0, 2, 3))
    N, _, H, W = x.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    Kdx = R * S * Cog
    return {"dx": (dx, (U + 2 * (Kdx + 2) * E32) * tdx),
            "dw": (dw, 2 * (N * H * W + 2) * E32 * tdw),
            "db": (db, 2 * (N * Ho * Wo + 2) * E32 * tdb)}


# (N, Ci, Co, H, W, k, s, p): the depth-to-space forward cases
D2S_CASES = {
    "partial_m_tile": (2, 8, 8, 5, 7, 4, 2, 1),
    "three_m_tiles": (3, 16, 16, 9, 11, 4, 2, 1),
    "second_n_tile": (1, 8, 40, 4, 4, 4, 2, 1),
    "phantom_nonsquare": (1, 8, 6, 4, 3, (5, 3), 2, (0, 1)),
    "single_k_tile": (1, 8, 8, 6, 6, 2, 2, 0),
    "stride3": (1, 8, 8, 4, 4, 7, 3, 2),
    "fcn_stride8": (1, 8, 8, 3, 3, 16, 8, 4),
}

# name -> make_inputs keyword arguments: shapes the fallback serves
FALLBACK_CASES = {
    "stride1": dict(N=2, Ci=8, Co=8, H=5, W=6, k=3, s=1, p=1),
    # flipped-weight implicit GEMM with R*S*Ci = 32 and 24: one real K tile
    "stride1_k2": dict(N=4, Ci=8, Co=8, H=8, W=9, k=2, s=1, p=0),
    "stride1_1x3": dict(N=2, Ci=8, Co=8, H=5, W=6, k=(1, 3), s=1, p=(0, 1)),
    "groups2": dict(N=2, Ci=8, Co=8, H=4, W=5, k=4, s=2, p=1, groups=2),
    "depthwise": dict(N=1, Ci=6, Co=6, H=4, W=4, k=4, s=2, p=1, groups=6),
    "dilation2": dict(N=1, Ci=8, Co=8, H=4, W=5, k=3, s=2, p=1, dil=2),
    "ci3": dict(N=2, Ci=3, Co=4, H=4, W=5, k=4, s=2, p=1),
    "sh_ne_sw": dict(N=1, Ci=8, Co=8, H=4, W=4, k=4, s=(2, 3), p=1),
}


def bilinear_kernel(k):
    """Closed form of the `bilinear` filler for a k x k filter."""
    f = -(-k // 2)
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    a = 1 - (torch.arange(k, dtype=torch.float64) / f - c).abs()
    return a[:, None] * a[None, :]


NET_TEXT = """
layer { name: "d" type: "MemoryData" top: "x" top: "t"
        memory_data_param { batch_size: 4 channels: 8 height: 8 width: 8 } }
layer { name: "conv" type: "Convolution" bottom: "x" top: "c"
        convolution_param { num_output: 8 kernel_size: 3 stride: 2 pad: 1
          weight_filler { type: "gaussian" std: 0.2 } } }
layer { name: "relu" type: "ReLU" bottom: "c" top: "c" }
layer { name: "up" type: "Deconvolution" bottom: "c" top: "u"
        convolution_param { num_output: 3 kernel_size: 4 stride: 2 pad: 1
          weight_filler { type: "gaussian" std: 0.2 }
          bias_filler { type: "constant" value: 0.1 } } }
layer { name: "l" type: "SoftmaxWithLoss" bottom: "u" bottom: "t"
        top: "loss" }
"""


def net_batch(seed=5):
    """A fixed batch for NET_TEXT: the label of a pixel is the arg-max of
    three fixed 2x2-smoothed channel mixes, so it is learnable."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(4, 8, 8, 8, generator=g)
    mix = torch.randn(3, 8, 1, 1, generator=g)
    s = F.avg_pool2d(F.conv2d(x, mix), 2, stride=1, padding=1)[:, :, :8, :8]
    return x, s.argmax(dim=1, keepdim=True).float()
