"""Float64 oracles, derived error bounds, CPU emulations and mutants for the
non-GEMM bf16 kernels (pool.hip, lrn.hip, batchnorm.hip and the softmax-loss,
ReLU, embed, LSTM-unit and SGD kernels of elementwise.hip).  Shared by
test_aux_kernel_bounds.py (CPU) and test_gpu_aux_kernels.py (GPU).

Every oracle takes the same bf16-rounded tensors the kernel gets, computes in
float64 and returns {output name: (want, tol)}; tol None means bit-exact.
The bounds are derived from the kernels' arithmetic, never from what a
kernel returned.

Notation.  u = 2^-8 is the bf16 unit roundoff (8 significand bits, round to
nearest), e = 2^-24 the fp32 one.

 B1  An output stored as bf16(fp32 expression) may differ from the float64
     value by u*T, T being the sum of the ABSOLUTE values of the
     expression's terms in float64.  T >= |value|, so the bound also holds
     where the terms cancel (LRN dx, BN dx).  Where the expression is a
     single product (no cancellation) T is |value|.
 B2  Each intermediate the kernel itself rounds to bf16 adds one further u
     on the terms it enters.
 B3  An fp32 accumulation of K terms, in any order, adds K*e*sum|terms|.
     Single fp32 operations add e each; they are folded into K (+2..+4).
 B4  Fast intrinsics.  The HIP math documentation is not installed with
     the toolchain, so: a relative I = 2^-16 for __logf, __powf,
     __frsqrt_rn, __fsqrt_rn and tanhf, and (1+|a|)*2^-20 for __expf(a)
     (its argument is scaled by log2(e) in fp32 first, so the error grows
     with |a|).  Where a result can underflow an absolute 2^-126 (smallest
     normal fp32) is added.  I is u/256: it cannot hide a bf16-level
     mistake.  Products of two roundings (u*u = I) are charged to the same
     slack, so bounds carry a small multiple of I.

Per op (n = local_size, m = rows = N*H*W):

 MAX pool   forward bit-exact (a selection); first maximum in window order
            (r*kw+s), found here with unfold + argmax.  Backward sums the
            routed dy in fp32 then rounds: (u + kh*kw*e) * sum|routed dy|.
 AVE pool   y = bf16(sum/size), size = window clipped at the PADDED
            boundary: (u + (K+2)e) * sum|x|/size, K = kh*kw.  Backward the
            same with sum|dy|/size over the windows holding the pixel.
 LRN        scale (fp32) = k + alpha/n*sum x^2, all terms positive:
            (n+4)e*scale.  y = bf16(x*scale^-beta): (u + 4I)|y|.
            dx = bf16(dy*scale^-beta - rc*x*sum_win(ratio)),
            ratio = bf16(dy*y/scale) built from the bf16 y:
            T = |dy|scale^-beta + rc|x|sum_win|ratio|; B1 gives u*T, the
            rounded ratio and the rounded y one u each on the second term
            (B2), together <= 3u*T; plus 4I*T.  A CPU emulation of the
            rounding points stays below 0.99u|y| and 1.47u*T.
 Softmax    a = x - max.  __expf(a) carries d = (1+|a|)2^-20; the row sum
            then carries D = sum(p*d) + C*e, so prob (fp32) is within
            p*(d + D + (C+4)e) + 2*2^-126.  Row loss -(x_l - max - log s):
            3e(|x_l|+|max|+|log s|) + I|log s| + D + (C+4)e; the fixed
            order sum adds rows*e*sum|rowloss|.  dx = bf16((p-1_l)*scale):
            (u+4e)|dx| + tol_p*scale + 2^-126, relative per element; an
            ignored row is exactly 0.
 BatchNorm  mean = s0/m: (m+2)e*mean|x|.  var = s1/m - mean^2:
            (m+3)e*mean(x^2) + 2|mean|tol_mean + 3e*mean^2, the absolute
            terms of the E[x^2]-mean^2 form.  invstd follows from var by
            the exact one-sided change of (var+eps)^-1/2.  y = bf16((x -
            mean)*invstd): the subtraction is fp32 of exact inputs, so
            (u+I)|y| + tol_mean*invstd + |x-mean|tol_invstd
            + 2e(|x|+|mean|)invstd.  Backward takes xhat (bf16) and invstd
            (fp32) as INPUTS, the oracle reads the same tensors, so xhat's
            rounding is not charged: T = invstd(|dy| + sum|dy|/m
            + |xhat|sum|dy*xhat|/m), tol (u + (m+6)e)T.  Global-stats mode:
            (u+8e)|value|.
 ReLU       bf16(x*slope): exact for a power-of-two slope; otherwise
            (u+4e)|y| (under one bf16 ulp).  Fused bias gradient: fp32 sum
            of m terms onto the prior content: (m+2)e(|db0| + sum|dx|).
 Embed      forward a copy (exact); dw fp32 atomics: (K+1)e*sum|dy| over
            the K rows that hit the word.
 LSTM unit  sigmoid s = 1/(1+__expf(-x)): s*(d + 3e).  tanhf: (I+e)|t|.
            1-s, 1-t^2 inherit absolute errors (they cancel near
            saturation).  Products propagate sum_k tol_k*prod_{j!=k}(|f_j|
            + tol_j).  c and act are fp32, h and dgates bf16 (+u*T).
 SGD        fp32 FMA chain, checked at rtol 1e-5 / atol 1e-6.

The whole-sequence LSTM routes are bounded in _lstm_seq_cases.py by the same
rules, one step at a time from the state the route itself emitted:

 LSTM seq   forward pre = xg + h_in @ W^T: (H+4)e(|xg| + |h_in| @ |W|^T),
 forward    then the LSTM-unit gate, c and h bounds; h_in[t] ==
            bf16(h[t-1] cont[t]) bit-exact.
 LSTM seq   dh_rec = cont (dxg[t+1] @ W): (4H+4)e(|dxg| @ |W|), plus u on
 backward   the loop route, which stores it as bf16; dc carried in float64
            with cont*gf*(tol + 4e*mag); dxg as the LSTM-unit dgates; dwhc
            (TN+4)e(|dxg|^T @ |h_in|).

The fused whole-arena solver updates are bounded in _solver_update_cases.py
(rules B1 and B3; no fast-math flag in the build, so sqrtf and the fp32
divide are correctly rounded and cost one e each, not the I of B4):

 Updates    every element with the lr / wd of the segment that owns it
            (torch.bucketize on the offsets), gg = g + wd p; c e T with c
            the roundings on a term's longest path plus one:
            SGD v' = mu v + lr gg: 5e(mu|v| + lr(|g| + wd|p|)) = 5e T_v;
            p' = p - v': 6e(|p| + T_v).  Nesterov v' as SGD;
            p' = p - ((1+mu)v' - mu v): 9e(|p| + (1+mu)T_v + mu|v|).
            Adam m' = b1 m + (1-b1)gg: 6e T_m, T_m = b1|m| + (1-b1)(|g| +
            wd|p|); v' = b2 v + (1-b2)gg^2: 9e(b2 v + (1-b2)(|g| + wd|p|)^2);
            p' = p - lr m'/(sqrt(v') + eps): the exact one-sided change of
            the root under tol_v, 8e on the quotient's T and 2e(|p| + Tq),
            about 16.5e(|p| + lr T_m/(sqrt(v') + eps)) in all.  A frozen
            segment (lr == 0) keeps p, v, m and the shadow bit for bit;
            elsewhere the shadow == bf16(p') of the p' the kernel wrote.
"""

import torch
import torch.nn.functional as F

U = 2.0 ** -8
E32 = 2.0 ** -24
INTR = 2.0 ** -16
TINY = 2.0 ** -126
BF = torch.bfloat16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf16(t):
    return t.to(BF)


def rb(t):
    """fp32 value rounded through bf16: the kernels' stbf()."""
    return t.to(BF).float()


# ------------------------------------------------------------- comparison

def violations(out, orc):
    """Messages for every output of `out` outside its bound in `orc`."""
    bad = []
    for name, got in out.items():
        want, tol = orc[name]
        if not isinstance(want, torch.Tensor):
            if got != want:
                bad.append(f"{name}: {got} != {want}")
            continue
        g = got.detach().cpu()
        if tuple(g.shape) != tuple(want.shape):
            bad.append(f"{name}: shape {tuple(g.shape)} vs "
                       f"{tuple(want.shape)}")
            continue
        if tol is None:
            if g.dtype != want.dtype or not torch.equal(g, want):
                nd = int((g.double() != want.double()).sum())
                bad.append(f"{name}: not bit-exact ({nd} differ)")
            continue
        err = (g.double() - want).abs()
        over = ~(err <= tol)
        if over.any():
            worst = (err - tol)[over].max().item()
            bad.append(f"{name}: {int(over.sum())}/{over.numel()} beyond "
                       f"the bound, worst excess {worst:.3e}")
    return bad


def report(out, orc, what):
    """One line per bounded output: how much of the bound was used."""
    for name, got in out.items():
        want, tol = orc[name]
        if not isinstance(want, torch.Tensor) or tol is None:
            continue
        g = got.detach().cpu()
        if tuple(g.shape) != tuple(want.shape):
            continue
        err = (g.double() - want).abs()
        used = (err / torch.as_tensor(tol).clamp_min(1e-300)).max().item()
        print(f"{what} {name}: max err {err.max().item():.3e}, "
              f"max err/bound {used:.3f}")


def assert_within(out, orc, what):
    report(out, orc, what)
    bad = violations(out, orc)
    assert not bad, f"{what}: " + "; ".join(bad)


# ---------------------------------------------------------------- pooling

def pool_out(h, k, s, p, floor_mode=False):
    """Caffe output size: ceil mode, last window must start inside the
    image or its left/top padding."""
    if floor_mode:
        return (h + 2 * p - k) // s + 1
    o = -(-(h + 2 * p - k) // s) + 1
    if p > 0 and (o - 1) * s >= h + p:
        o -= 1
    return o


# (H, W, kernel, stride, pad)
POOL_GEOMS = [
    (12, 12, (3, 3), (2, 2), (0, 0)),    # ceil overhang, last window clipped
    (7, 7, (3, 3), (1, 1), (1, 1)),      # inception pool
    (5, 5, (2, 2), (2, 2), (1, 1)),      # pool_out clamp fires: 4 -> 3
    (9, 14, (3, 2), (2, 1), (1, 0)),     # non-square everything
    (11, 11, (2, 2), (3, 3), (0, 0)),    # stride > kernel
]
# (C, geometry); C=16 runs the 8-wide kernels, C=20 the scalar ones
MAXPOOL_CASES = [(c, g) for g in POOL_GEOMS for c in (16, 20)] + [
    (8, (13, 13, (11, 11), (1, 1), (0, 0))),     # rs up to 120: int8 top
    (8, (12, 12, (12, 12), (1, 1), (0, 0))),     # global, int32 argmax
    (12, (12, 12, (12, 12), (1, 1), (0, 0))),
    (8, (7, 7, (7, 7), (1, 1), (0, 0))),         # global, int8 argmax
]
AVGPOOL_CASES = [(c, g) for g in POOL_GEOMS for c in (16, 20)]
GLOBAL_AVG_CASES = [(32, 7, 7), (20, 7, 7)]


def pool_inputs(c, geom, seed, ties, n=2):
    h, w, k, s, p = geom
    g = gen(seed)
    if ties:    # multiples of 0.5 in [-2, 2]: most windows hold ties
        x = torch.randint(-4, 5, (n, c, h, w), generator=g).float() * 0.5
    else:
        x = torch.randn(n, c, h, w, generator=g)
    po, qo = pool_out(h, k[0], s[0], p[0]), pool_out(w, k[1], s[1], p[1])
    dy = torch.randn(n, c, po, qo, generator=g)
    return dict(x=bf16(x), dy=bf16(dy), kernel=k, stride=s, pad=p)


def _windows(x, k, s, p, po, qo, fill):
    """[N, C, kh*kw, po*qo] window taps in (r*kw+s) order, `fill` outside."""
    n, c, h, w = x.shape
    hp, wp = (po - 1) * s[0] + k[0], (qo - 1) * s[1] + k[1]
    xp = torch.full((n, c, max(hp, h + p[0]), max(wp, w + p[1])), fill,
                    dtype=x.dtype)
    xp[:, :, p[0]:p[0] + h, p[1]:p[1] + w] = x
    cols = F.unfold(xp[:, :, :hp, :wp], k, stride=s)
    return cols.reshape(n, c, k[0] * k[1], po * qo)


def _route(rs, dy, shape, k, s, p):
    """Scatter-add dy [N,C,P,Q] to the pixel each window-relative argmax
    rs [N,C,P*Q] names."""
    n, c, h, w = shape
    po, qo = dy.shape[2], dy.shape[3]
    pp = torch.arange(po).repeat_interleave(qo)
    qq = torch.arange(qo).repeat(po)
    hh = pp * s[0] - p[0] + rs // k[1]
    ww = qq * s[1] - p[1] + rs % k[1]
    dx = torch.zeros(n, c, h * w, dtype=dy.dtype)
    dx.scatter_add_(2, hh * w + ww, dy.reshape(n, c, -1))
    return dx.reshape(n, c, h, w)


def maxpool_oracle(inp):
    x, dy = inp["x"].double(), inp["dy"].double()
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    po, qo = dy.shape[2], dy.shape[3]
    win = _windows(x, k, s, p, po, qo, float("-inf"))
    rs = torch.argmax(win, dim=2)            # first maximum
    y = win.gather(2, rs.unsqueeze(2)).reshape(x.shape[0], x.shape[1], po, qo)
    dx = _route(rs, dy, x.shape, k, s, p)
    t = _route(rs, dy.abs(), x.shape, k, s, p)
    return {"y": (bf16(y), None),
            "dx": (dx, (U + k[0] * k[1] * E32) * t)}


def maxpool_emulate(inp, tie_last=False, floor_mode=False):
    """The kernel's own loop: strict > keeps the first maximum."""
    x, dy = inp["x"].float(), inp["dy"].float()
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    n, c, h, w = x.shape
    po = pool_out(h, k[0], s[0], p[0], floor_mode)
    qo = pool_out(w, k[1], s[1], p[1], floor_mode)
    win = _windows(x, k, s, p, po, qo, float("-inf"))
    best = torch.full((n, c, po * qo), -3.4e38)
    brs = torch.zeros((n, c, po * qo), dtype=torch.long)
    for t in range(k[0] * k[1]):
        v = win[:, :, t]
        upd = (v >= best) if tie_last else (v > best)
        upd &= torch.isfinite(v)
        best = torch.where(upd, v, best)
        brs = torch.where(upd, torch.full_like(brs, t), brs)
    out = {"y": bf16(best.reshape(n, c, po, qo))}
    if (po, qo) == tuple(dy.shape[2:]):
        out["dx"] = bf16(_route(brs, dy, x.shape, k, s, p))
    return out


def _avg_geometry(h, w, k, s, p, po, qo, divisor):
    for pi in range(po):
        h0 = pi * s[0] - p[0]
        he = min(h0 + k[0], h + p[0])
        for qi in range(qo):
            w0 = qi * s[1] - p[1]
            we = min(w0 + k[1], w + p[1])
            hs, ws = slice(max(h0, 0), min(he, h)), slice(max(w0, 0),
                                                          min(we, w))
            if divisor == "caffe":
                size = (he - h0) * (we - w0)
            elif divisor == "full":
                size = k[0] * k[1]
            else:   # "image": clipped at the image, not the padded boundary
                size = (hs.stop - hs.start) * (ws.stop - ws.start)
            yield pi, qi, hs, ws, size


def _avgpool(x, dy, k, s, p, po, qo, divisor="caffe"):
    n, c, h, w = x.shape
    y = torch.zeros(n, c, po, qo, dtype=x.dtype)
    dx = torch.zeros_like(x) if dy is not None else None
    for pi, qi, hs, ws, size in _avg_geometry(h, w, k, s, p, po, qo,
                                              divisor):
        y[:, :, pi, qi] = x[:, :, hs, ws].sum(dim=(2, 3)) / size
        if dx is not None:
            dx[:, :, hs, ws] += (dy[:, :, pi, qi] / size)[:, :, None, None]
    return y, dx


def avgpool_oracle(inp):
    x, dy = inp["x"].double(), inp["dy"].double()
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    po, qo = dy.shape[2], dy.shape[3]
    y, dx = _avgpool(x, dy, k, s, p, po, qo)
    ty, tdx = _avgpool(x.abs(), dy.abs(), k, s, p, po, qo)
    r = U + (k[0] * k[1] + 2) * E32
    return {"y": (y, r * ty), "dx": (dx, r * tdx)}


def avgpool_emulate(inp, divisor="caffe", floor_mode=False):
    x, dy = inp["x"].float(), inp["dy"].float()
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    h, w = x.shape[2], x.shape[3]
    po = pool_out(h, k[0], s[0], p[0], floor_mode)
    qo = pool_out(w, k[1], s[1], p[1], floor_mode)
    same = (po, qo) == tuple(dy.shape[2:])
    y, dx = _avgpool(x, dy if same else None, k, s, p, po, qo, divisor)
    out = {"y": bf16(y)}
    if same:
        out["dx"] = bf16(dx)
    return out


def global_avg_inputs(c, h, w, seed, n=2):
    g = gen(seed)
    return dict(x=bf16(torch.randn(n, c, h, w, generator=g)),
                dy=bf16(torch.randn(n, c, 1, 1, generator=g)),
                kernel=(h, w), stride=(1, 1), pad=(0, 0))


MAXPOOL_MUTANTS = {
    "tie_last": lambda i: maxpool_emulate(i, tie_last=True),
    "floor_mode": lambda i: maxpool_emulate(i, floor_mode=True),
}
AVGPOOL_MUTANTS = {
    "divisor_full": lambda i: avgpool_emulate(i, divisor="full"),
    "divisor_image": lambda i: avgpool_emulate(i, divisor="image"),
    "floor_mode": lambda i: avgpool_emulate(i, floor_mode=True),
}


# -------------------------------------------------------------------- LRN

# (C, local_size, alpha, beta, k, input scale)
LRN_CASES = [
    (8, 5, 1.0, 0.75, 1.0, 1.0),      # one octet, both edges zero-padded
    (16, 5, 1.0, 0.75, 1.0, 1.0),     # two octets, no interior octet
    (24, 9, 0.5, 0.5, 2.0, 1.0),      # maximum radius, rsqrt path
    (40, 3, 2.0, 0.6, 1.0, 1.0),      # generic __powf
    (96, 5, 1e-4, 0.75, 1.0, 60.0),   # AlexNet's, activation-sized input
]


def lrn_inputs(case, seed, n=2, hw=3):
    c, ls, alpha, beta, k, xs = case
    g = gen(seed)
    return dict(x=bf16(torch.randn(n, c, hw, hw, generator=g) * xs),
                dy=bf16(torch.randn(n, c, hw, hw, generator=g)),
                local_size=ls, alpha=alpha, beta=beta, k=k)


def _chan_window(t, n, circular=False):
    """Sum over the n-wide channel window centred on each channel."""
    half, c = n // 2, t.shape[1]
    if circular:
        return sum(torch.roll(t, j, dims=1) for j in range(-half, half + 1))
    tp = F.pad(t, (0, 0, 0, 0, half, half))
    return sum(tp[:, j:j + c] for j in range(n))


def lrn_oracle(inp):
    x, dy = inp["x"].double(), inp["dy"].double()
    n, alpha, beta, k = (inp["local_size"], inp["alpha"], inp["beta"],
                         inp["k"])
    scale = k + alpha / n * _chan_window(x * x, n)
    pw = scale ** -beta
    y = x * pw
    ratio = dy * y / scale
    rc = 2.0 * alpha * beta / n
    t1 = dy * pw
    dx = t1 - rc * x * _chan_window(ratio, n)
    t = t1.abs() + rc * x.abs() * _chan_window(ratio.abs(), n)
    return {"scale": (scale, (n + 4) * E32 * scale),
            "y": (y, (U + 4 * INTR) * y.abs()),
            "dx": (dx, (3 * U + 4 * INTR) * t)}


def lrn_emulate(inp, radius_delta=0, circular=False, second_term=True,
                identity=False):
    """fp32 arithmetic, bf16 at the kernel's three rounding points (y,
    ratio, dx).  Outputs as NCHW; scale is NCHW here, NHWC in the pack."""
    x, dy = inp["x"].float(), inp["dy"].float()
    n, beta = inp["local_size"], inp["beta"]
    if identity:
        return {"scale": torch.ones_like(x), "y": bf16(x), "dx": bf16(dy)}
    nw = n + 2 * radius_delta
    a_over_n = torch.tensor(inp["alpha"], dtype=torch.float32) / n
    scale = inp["k"] + a_over_n * _chan_window(x * x, nw, circular)
    pw = scale.pow(-beta)
    y = rb(x * pw)
    ratio = rb(dy * y / scale)
    rc = torch.tensor(2.0 * inp["alpha"] * beta / n, dtype=torch.float32)
    dx = dy * pw
    if second_term:
        dx = dx - rc * x * _chan_window(ratio, nw, circular)
    return {"scale": scale, "y": bf16(y), "dx": bf16(dx)}


LRN_MUTANTS = {
    "radius_minus_1": lambda i: lrn_emulate(i, radius_delta=-1),
    "circular_window": lambda i: lrn_emulate(i, circular=True),
    "no_second_term": lambda i: lrn_emulate(i, second_term=False),
    "identity": lambda i: lrn_emulate(i, identity=True),
}


# ----------------------------------------------------------- softmax loss

def _softmax_case(shape, axis, seed, ignore_label=None, ignore_every=0,
                  special=False):
    g = gen(seed)
    x = torch.randn(shape, generator=g) * 20
    c = shape[axis]
    lshape = [d for i, d in enumerate(shape) if i != axis]
    lab = torch.randint(0, c, lshape, generator=g).float()
    if special:
        # rows 0, 1: +-200 alternating (inf without the max subtraction),
        # label once on a +200 and once on a -200 entry; row 2: constant
        alt = torch.tensor([200.0, -200.0]).repeat(c)[:c]
        x[0], x[1], x[2] = alt, alt, 3.0
        lab[0], lab[1] = 2.0, 1.0
    if ignore_every:
        flat = lab.reshape(-1)
        flat[::ignore_every] = float(ignore_label)
        lab = flat.reshape(lshape)
    return dict(x=bf16(x), label=lab, ignore_label=ignore_label, axis=axis)


def softmax_cases():
    """name -> inputs.  rows x C, logits x20."""
    cases = {}
    for i, (rows, c) in enumerate([(5, 1), (3, 63), (3, 64), (3, 65),
                                   (6, 1000), (2, 8801), (300, 11)]):
        cases[f"{rows}x{c}"] = _softmax_case((rows, c), 1, 100 + i)
    cases["special_4x65"] = _softmax_case((4, 65), 1, 120, special=True)
    cases["ignore_32x11"] = _softmax_case((32, 11), 1, 121, -1, 4)
    cases["ignore_axis2_3x4x11"] = _softmax_case((3, 4, 11), 2, 122, -1, 3)
    cases["ignore_axis1_2x5x3x2"] = _softmax_case((2, 5, 3, 2), 1, 123, -1, 5)
    return cases


def _softmax_rows(inp, dtype):
    x, axis = inp["x"].to(dtype), inp["axis"]
    xm = x.movedim(axis, -1)
    lab = inp["label"].reshape(-1).long()
    ig = inp["ignore_label"]
    valid = (lab != ig) if ig is not None else torch.ones_like(lab,
                                                               dtype=torch.bool)
    return xm.reshape(-1, xm.shape[-1]), tuple(xm.shape), lab, valid


def softmax_oracle(inp):
    x2, mshape, lab, valid = _softmax_rows(inp, torch.float64)
    rows, c = x2.shape
    vd = valid.double().unsqueeze(1)
    mx = x2.max(dim=1, keepdim=True).values
    a = x2 - mx
    ex = a.exp()
    s = ex.sum(dim=1, keepdim=True)
    p = ex / s
    d = (1.0 + a.abs()) * 2.0 ** -20
    dsum = (p * d).sum(dim=1, keepdim=True)
    tol_p = p * (d + dsum + (c + 4) * E32) + 2 * TINY
    safe = torch.where(valid, lab, torch.zeros_like(lab)).unsqueeze(1)
    xl, ls = x2.gather(1, safe), s.log()
    rowloss = -(xl - mx - ls) * vd
    tol_row = (3 * E32 * (xl.abs() + mx.abs() + ls.abs()) + INTR * ls.abs()
               + dsum + (c + 4) * E32) * vd
    loss = rowloss.sum()
    tol_loss = tol_row.sum() + (rows + 1) * E32 * rowloss.abs().sum()
    count = int(valid.sum())
    scale = 1.0 / count
    onehot = torch.zeros_like(p).scatter_(1, safe, 1.0)
    dx = (p - onehot) * scale * vd
    tol_dx = ((U + 4 * E32) * dx.abs() + tol_p * scale + TINY) * vd
    back = lambda t: t.reshape(mshape).movedim(-1, inp["axis"])  # noqa: E731
    return {"loss": (loss, tol_loss), "count": (count, None),
            "prob": (p, tol_p), "dx": (back(dx), back(tol_dx))}


def softmax_emulate(inp, zero_off_label=False, no_ignore=False,
                    no_max=False):
    x2, mshape, lab, valid = _softmax_rows(inp, torch.float32)
    if no_ignore:
        valid = torch.ones_like(valid)
    vf = valid.float().unsqueeze(1)
    mx = x2.max(dim=1, keepdim=True).values
    if no_max:
        mx = torch.zeros_like(mx)
    ex = (x2 - mx).exp()
    s = ex.sum(dim=1, keepdim=True)
    p = ex * (1.0 / s)
    safe = lab.clamp_min(0).unsqueeze(1)
    rowloss = -(x2.gather(1, safe) - mx - s.log()) * vf
    count = int(valid.sum())
    scale = torch.tensor(1.0 / count, dtype=torch.float32)
    onehot = torch.zeros_like(p).scatter_(1, safe, 1.0)
    onehot = onehot * (lab >= 0).float().unsqueeze(1)
    dx = rb((p - onehot) * scale) * vf
    if zero_off_label:
        dx = dx * onehot
    return {"loss": rowloss.sum(), "count": count, "prob": p,
            "dx": bf16(dx.reshape(mshape).movedim(-1, inp["axis"]))}


SOFTMAX_MUTANTS = {
    "zero_off_label": lambda i: softmax_emulate(i, zero_off_label=True),
    "no_ignore": lambda i: softmax_emulate(i, no_ignore=True),
    "no_max_subtraction": lambda i: softmax_emulate(i, no_max=True),
}


# -------------------------------------------------------------- batchnorm

BN_EPS = 1e-5
# (N, C, H, W), shift, spread
BN_CASES = [
    ((1, 8, 1, 3), 0.0, 1.0),       # rows < row-groups
    ((2, 24, 23, 23), 0.0, 1.0),    # bx=3, 255 threads, multi-block atomics
    ((2, 56, 5, 5), 0.0, 1.0),      # bx=7, 252 threads
    ((2, 264, 3, 3), 0.0, 1.0),     # second column pass, one live group
    ((2, 24, 9, 9), 8.0, 0.5),      # shifted: E[x^2] - mean^2 cancels
]


def bn_inputs(case, seed):
    shape, shift, spread = case
    g = gen(seed)
    c = shape[1]
    return dict(x=bf16(torch.randn(shape, generator=g) * spread + shift),
                dy=bf16(torch.randn(shape, generator=g)),
                gmean=torch.randn(c, generator=g) + shift,
                gvar=torch.rand(c, generator=g) + 0.5, eps=BN_EPS)


def _pc(v):
    return v.reshape(1, -1, 1, 1)


def bn_train_oracle(inp):
    x, eps = inp["x"].double(), inp["eps"]
    m = x.numel() // x.shape[1]
    dims = (0, 2, 3)
    mean = x.mean(dim=dims)
    m2 = (x * x).mean(dim=dims)
    var = ((x - _pc(mean)) ** 2).mean(dim=dims)
    tol_mean = (m + 2) * E32 * x.abs().mean(dim=dims)
    tol_var = ((m + 3) * E32 * m2 + 2 * mean.abs() * tol_mean
               + 3 * E32 * mean * mean)
    invstd = (var + eps) ** -0.5
    tol_inv = ((var + eps - tol_var).clamp_min(1e-30) ** -0.5 - invstd
               + 4 * E32 * invstd)
    xc = x - _pc(mean)
    y = xc * _pc(invstd)
    tol_y = ((U + INTR) * y.abs() + _pc(tol_mean * invstd)
             + xc.abs() * _pc(tol_inv)
             + 2 * E32 * (x.abs() + _pc(mean.abs())) * _pc(invstd))
    return {"mean": (mean, tol_mean), "var": (var, tol_var),
            "invstd": (invstd, tol_inv), "y": (y, tol_y)}


def bn_infer_oracle(inp):
    x = inp["x"].double()
    mean, var = inp["gmean"].double(), inp["gvar"].double()
    invstd = (var + inp["eps"]) ** -0.5
    y = (x - _pc(mean)) * _pc(invstd)
    tol_y = (U * y.abs()
             + 8 * E32 * (x.abs() + _pc(mean.abs())) * _pc(invstd))
    return {"invstd": (invstd, 4 * E32 * invstd), "y": (y, tol_y)}


def bn_backward_oracle(xhat, dy, invstd, train):
    """xhat (bf16) and invstd (fp32) are the tensors handed to the kernel."""
    xh, d, inv = xhat.double(), dy.double(), _pc(invstd.double())
    if not train:
        dx = d * inv
        return {"dx": (dx, (U + 8 * E32) * dx.abs())}
    m = d.numel() // d.shape[1]
    dims = (0, 2, 3)
    s1, s2 = _pc(d.sum(dim=dims)), _pc((d * xh).sum(dim=dims))
    a1, a2 = _pc(d.abs().sum(dim=dims)), _pc((d * xh).abs().sum(dim=dims))
    dx = inv * (d - s1 / m - xh * s2 / m)
    t = inv * (d.abs() + a1 / m + xh.abs() * a2 / m)
    return {"dx": (dx, (U + (m + 6) * E32) * t)}


def bn_train_emulate(inp):
    x = inp["x"].float()
    m = x.numel() // x.shape[1]
    mean = x.sum(dim=(0, 2, 3)) / m
    var = ((x * x).sum(dim=(0, 2, 3)) / m - mean * mean).clamp_min(0)
    invstd = (var + inp["eps"]).rsqrt()
    y = bf16((x - _pc(mean)) * _pc(invstd))
    return {"mean": mean, "var": var, "invstd": invstd, "y": y}


def bn_infer_emulate(inp):
    invstd = (inp["gvar"] + inp["eps"]).rsqrt()
    y = bf16((inp["x"].float() - _pc(inp["gmean"])) * _pc(invstd))
    return {"invstd": invstd, "y": y}


def bn_backward_emulate(xhat, dy, invstd, train, s2_term=True):
    xh, d, inv = xhat.float(), dy.float(), _pc(invstd.float())
    if not train:
        return {"dx": bf16(inv * d)}
    inv_m = 1.0 / (d.numel() // d.shape[1])
    s1 = _pc(d.sum(dim=(0, 2, 3)))
    s2 = _pc((d * xh).sum(dim=(0, 2, 3)))
    if not s2_term:
        s2 = torch.zeros_like(s2)
    return {"dx": bf16(inv * (d - s1 * inv_m - xh * s2 * inv_m))}


BN_BACKWARD_MUTANTS = {
    "no_s2_term": lambda xh, dy, inv: bn_backward_emulate(
        xh, dy, inv, True, s2_term=False),
}


# ------------------------------------------------------------------- ReLU

RELU_SIZES = (7, 8, 2295)
RELU_SLOPES = (0.25, 0.1)


def relu_inputs(n, seed):
    g = gen(seed)
    return dict(x=bf16(torch.randn(n, generator=g)),
                dy=bf16(torch.randn(n, generator=g)))


def _relu_bound(v, slope):
    pow2 = slope == 0.0 or (slope > 0 and
                            torch.tensor(slope).log2().frac().item() == 0.0)
    if pow2:
        return (bf16(v), None)
    return (v, (U + 4 * E32) * v.abs())


def relu_oracle(inp, slope):
    """The kernel multiplies by the fp32 slope."""
    x, dy = inp["x"].double(), inp["dy"].double()
    sl = float(torch.tensor(slope, dtype=torch.float32))
    y = torch.where(x > 0, x, x * sl)
    dx = torch.where(x > 0, dy, dy * sl)    # sign(y) == sign(x), slope > 0
    return {"y": _relu_bound(y, slope), "dx": _relu_bound(dx, slope)}


def relu_emulate(inp, slope):
    x, dy = inp["x"].float(), inp["dy"].float()
    sl = torch.tensor(slope, dtype=torch.float32)
    y = bf16(torch.where(x > 0, x, x * sl))
    dx = bf16(torch.where(y.float() > 0, dy, dy * sl))
    return {"y": y, "dx": dx}


def relu_window_inputs(c, seed, n=2, h=3, w=5, ctot=24, off=8):
    """y and dy as channel windows [off, off+c) of channels-last buffers
    with row stride ctot; db0 a nonzero prior bias gradient."""
    g = gen(seed)
    cl = torch.channels_last
    ybuf = bf16(torch.randn(n, ctot, h, w, generator=g)).contiguous(
        memory_format=cl)
    dbuf = bf16(torch.randn(n, ctot, h, w, generator=g)).contiguous(
        memory_format=cl)
    return dict(ybuf=ybuf, dybuf=dbuf, off=off, c=c,
                db0=torch.randn(c, generator=g) * 3 + 1)


def relu_fused_oracle(y, dy, db0, slope):
    """dx and the bias gradient accumulated onto db0, y/dy any 2-D or 4-D
    (channel dim 1) tensors of equal shape."""
    yd, dd = y.double(), dy.double()
    sl = float(torch.tensor(slope, dtype=torch.float32))
    dx = torch.where(yd > 0, dd, dd * sl)
    dims = (0,) if yd.dim() == 2 else (0, 2, 3)
    m = yd.numel() // yd.shape[1]
    db = db0.double() + dx.sum(dim=dims)
    tol_db = (m + 2) * E32 * (db0.double().abs() + dx.abs().sum(dim=dims))
    return {"dx": _relu_bound(dx, slope), "db": (db, tol_db)}


def relu_fused_emulate(y, dy, db0, slope):
    yf, df = y.float(), dy.float()
    g = torch.where(yf > 0, df, df * torch.tensor(slope))
    dims = (0,) if yf.dim() == 2 else (0, 2, 3)
    return {"dx": bf16(g), "db": db0.float() + g.sum(dim=dims)}


# ------------------------------------------------------------------ embed

EMBED_V, EMBED_E = 50, 5


def embed_inputs(seed):
    g = gen(seed)
    idx = torch.randint(0, EMBED_V, (7, 3), generator=g)
    idx[0, 0], idx[0, 1], idx[1, 0] = 0, EMBED_V - 1, EMBED_V - 1
    idx[2] = 17                                  # repeats
    return dict(idx=idx.float(),
                w=torch.randn(EMBED_V, EMBED_E, generator=g) * 0.1,
                dy=bf16(torch.randn(7, 3, EMBED_E, generator=g)))


def embed_oracle(inp):
    idx = inp["idx"].long().reshape(-1)
    wb = bf16(inp["w"])
    dy = inp["dy"].double().reshape(-1, EMBED_E)
    dw = torch.zeros(EMBED_V, EMBED_E, dtype=torch.float64)
    dw.index_add_(0, idx, dy)
    t = torch.zeros_like(dw).index_add_(0, idx, dy.abs())
    hits = torch.zeros(EMBED_V, dtype=torch.float64).index_add_(
        0, idx, torch.ones(idx.numel(), dtype=torch.float64))
    n = idx.numel()
    return {"y": (wb[idx].reshape(7, 3, EMBED_E), None),
            "dw": (dw, (hits.unsqueeze(1) + 1) * E32 * t),
            "db": (dy.sum(0), (n + 1) * E32 * dy.abs().sum(0))}


def embed_emulate(inp):
    idx = inp["idx"].long().reshape(-1)
    dy = inp["dy"].float().reshape(-1, EMBED_E)
    dw = torch.zeros(EMBED_V, EMBED_E).index_add_(0, idx, dy)
    return {"y": bf16(inp["w"])[idx].reshape(7, 3, EMBED_E), "dw": dw,
            "db": dy.sum(0)}


# -------------------------------------------------------------- LSTM unit

def lstm_inputs(seed, n=12, h=20):
    g = gen(seed)
    cont = torch.ones(n)
    cont[::3] = 0
    return dict(c_prev=torch.randn(n, h, generator=g),
                gates=bf16(torch.randn(n, 4 * h, generator=g) * 4),
                cont=cont, dc_next=torch.randn(n, h, generator=g),
                dh=bf16(torch.randn(n, h, generator=g)))


def _ptol(*factors):
    """Error of a product of (magnitude, tol) factors."""
    total = 0.0
    for i, (_, ti) in enumerate(factors):
        term = ti
        for j, (mj, tj) in enumerate(factors):
            if j != i:
                term = term * (mj + tj)
        total = total + term
    return total


def _exact(v):
    return (v.abs(), torch.zeros_like(v))


def lstm_oracle(inp):
    n, h4 = inp["gates"].shape
    h = h4 // 4
    gx = inp["gates"].double().reshape(n, 4, h)
    cp, ct = inp["c_prev"].double(), inp["cont"].double().reshape(n, 1)
    dcn, dh = inp["dc_next"].double(), inp["dh"].double()

    def sig(x):
        s = torch.sigmoid(x)
        return s, s * ((1.0 + x.abs()) * 2.0 ** -20 + 3 * E32)

    (gi, ti), (gf, tf), (go, to) = sig(gx[:, 0]), sig(gx[:, 1]), sig(gx[:, 2])
    gg = torch.tanh(gx[:, 3])
    tg = (INTR + E32) * gg.abs()
    cpc = cp * ct
    c = gf * cpc + gi * gg
    tol_c = (_ptol((gf, tf), _exact(cpc)) + _ptol((gi, ti), (gg.abs(), tg))
             + 4 * E32 * ((gf * cpc).abs() + (gi * gg).abs()))
    tc = torch.tanh(c)
    ttc = (INTR + E32) * tc.abs() + (1 - tc * tc) * tol_c + E32
    hh = go * tc
    tol_h = U * hh.abs() + _ptol((go, to), (tc.abs(), ttc)) \
        + 2 * E32 * hh.abs()
    act = torch.stack([gi, gf, go, gg], dim=1)
    tol_act = torch.stack([ti, tf, to, tg], dim=1)

    one_m = lambda s, ts: (1 - s, ts + E32)                 # noqa: E731
    one_m2 = lambda t, tt: (1 - t * t, 2 * t.abs() * tt + 2 * E32)  # noqa
    f_tc2 = one_m2(tc, ttc)
    dc = dcn + dh * go * f_tc2[0]
    t_dc = dcn.abs() + dh.abs() * go * f_tc2[0]
    tol_dc = _ptol(_exact(dh), (go, to), f_tc2) + 3 * E32 * t_dc
    fdc = (t_dc, tol_dc)

    def out(value, *factors):
        mag = 1.0
        for mf, _ in factors:
            mag = mag * mf
        return value, mag, _ptol(*factors) + 4 * E32 * mag

    dcp, _, tol_dcp = out(dc * gf * ct, fdc, (gf, tf),
                          _exact(ct.expand_as(gf)))
    outs = [out(dc * gg * gi * (1 - gi), fdc, (gg.abs(), tg), (gi, ti),
                one_m(gi, ti)),
            out(dc * cpc * gf * (1 - gf), fdc, _exact(cpc), (gf, tf),
                one_m(gf, tf)),
            out(dh * tc * go * (1 - go), _exact(dh), (tc.abs(), ttc),
                (go, to), one_m(go, to)),
            out(dc * gi * (1 - gg * gg), fdc, (gi, ti), one_m2(gg, tg))]
    dg = torch.stack([o[0] for o in outs], dim=1).reshape(n, h4)
    tol_dg = torch.stack([U * o[1] + o[2] for o in outs],
                         dim=1).reshape(n, h4)
    return {"c": (c, tol_c + E32 * c.abs()), "h": (hh, tol_h),
            "act": (act, tol_act), "dc_prev": (dcp, tol_dcp),
            "dgates": (dg, tol_dg)}


def lstm_emulate(inp):
    n, h4 = inp["gates"].shape
    h = h4 // 4
    gx = inp["gates"].float().reshape(n, 4, h)
    cp, ct = inp["c_prev"].float(), inp["cont"].float().reshape(n, 1)
    gi, gf, go = (1.0 / (1.0 + torch.exp(-gx[:, j])) for j in range(3))
    gg = torch.tanh(gx[:, 3])
    c = gf * cp * ct + gi * gg
    tc = torch.tanh(c)
    dhv = inp["dh"].float()
    dc = inp["dc_next"].float() + dhv * go * (1.0 - tc * tc)
    dg = torch.stack([dc * gg * gi * (1.0 - gi),
                      dc * cp * ct * gf * (1.0 - gf),
                      dhv * tc * go * (1.0 - go),
                      dc * gi * (1.0 - gg * gg)], dim=1)
    return {"c": c, "h": bf16(go * tc),
            "act": torch.stack([gi, gf, go, gg], dim=1),
            "dc_prev": dc * gf * ct, "dgates": bf16(dg.reshape(n, h4))}


# -------------------------------------------------------------------- SGD

SGD_SIZES = (1, 3, 4, 5)
SGD_HYPER = (0.1, 0.9, 0.005)          # lr, momentum, weight decay


def sgd_inputs(n, seed):
    g = gen(seed)
    return dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g),
                v=torch.randn(n, generator=g))


def sgd_oracle(inp):
    lr, mu, wd = SGD_HYPER
    p, g, v = inp["p"].double(), inp["g"].double(), inp["v"].double()
    v1 = mu * v + lr * (g + wd * p)
    p1 = p - v1
    return {"p": (p1, 1e-5 * p1.abs() + 1e-6),
            "v": (v1, 1e-5 * v1.abs() + 1e-6)}


def sgd_emulate(inp):
    lr, mu, wd = SGD_HYPER
    p, g, v = inp["p"].clone(), inp["g"], inp["v"].clone()
    v = mu * v + lr * (g + wd * p)
    return {"p": p - v, "v": v}
