"""Float64 oracle, derived bounds, CPU emulation and mutants for the fused
LSTM decode-step kernel (csrc/lstm_step.hip).  Shared by the CPU proof and
the GPU test in test_lstm_step_gpu.py; notation and rules B1-B4 are those of
_bf16_bounds.py.

The kernel computes, per stream n and hidden unit j,

    pre[g] = b[gH+j] + x[n].W_xc[gH+j] + (cont_n h_prev[n]).W_hc[gH+j]
             + x_static[n].W_xsc[gH+j]                  g = i, f, o, g

in fp32 from bf16 operands, then the LSTM unit of elementwise.hip:
c = cont*f*c_prev + i*g (fp32), h = bf16(o*tanh(c)).

 pre    a bf16 x bf16 product is exact in fp32 (16 significand bits), so
        only the accumulation rounds: rule B3 with K the total dot length,
        (K+4) e T, T = |b| + sum|terms| (the +4 covers the bias add and the
        cross-lane tree).  cont is 0 or 1, so cont*h_prev is exact.
 gates  sigmoid is 1/4-Lipschitz and tanh 1-Lipschitz: the pre-activation
        bound enters the gate bounds of the LSTM-unit oracle scaled by 1/4
        and 1, next to the intrinsic terms (s*(d+3e), (I+e)|t|).
 c, h   as the LSTM-unit oracle: products propagate through _ptol; tanh(c)
        takes tol_c whole (1-Lipschitz); h additionally gets U|h|.

The oracle reads the same bf16 tensors the kernel gets.
"""

import torch

from _bf16_bounds import BF, E32, INTR, U, _ptol, gen

# (N, D, H, Ds); Ds = 0: no static segment
CASES = [
    (1, 8, 8, 0),          # one chunk per row; fewer units than waves
    (3, 520, 24, 0),       # one full 64-lane x 8 pass plus a one-chunk tail
    (16, 64, 136, 8),      # several blocks, a partial last block, all three
                           # segments, full N
    (2, 1000, 1000, 1000),  # one LRCN step
]


def inputs(N, D, H, Ds, seed=0):
    g = gen(seed + 7919 * N + D + H + Ds)
    K = D + H + Ds
    # pre-activations of std ~1.6: they reach about +-4
    sw = 1.6 / (D + H / 3.0 + Ds) ** 0.5

    def w(cols):
        return (torch.randn(4 * H, cols, generator=g) * sw).to(BF)

    cont = torch.ones(N)
    cont[1::3] = 0                    # streams 1, 4, 7, ... restart
    inp = dict(
        x=torch.randn(N, D, generator=g).to(BF),
        # non-zero previous state everywhere, so a missed gate shows
        h_prev=(torch.rand(N, H, generator=g) * 1.6 - 0.8).to(BF),
        c_prev=torch.randn(N, H, generator=g) * 1.5,
        cont=cont, w_xc=w(D), w_hc=w(H),
        b=(torch.randn(4 * H, generator=g) * 0.5).to(BF),
        xs=None, w_xsc=None, K=K)
    if Ds:
        inp["xs"] = torch.randn(N, Ds, generator=g).to(BF)
        inp["w_xsc"] = w(Ds)
    return inp


def _segments(inp, dtype, use_cont=True):
    ct = inp["cont"].to(dtype).reshape(-1, 1)
    h_in = inp["h_prev"].to(dtype) * (ct if use_cont else 1.0)
    segs = [(inp["x"].to(dtype), inp["w_xc"].to(dtype)),
            (h_in, inp["w_hc"].to(dtype))]
    if inp["xs"] is not None:
        segs.append((inp["xs"].to(dtype), inp["w_xsc"].to(dtype)))
    return segs


def _exact(v):
    return (v.abs(), torch.zeros_like(v))


def oracle(inp):
    """{"c": (want, tol), "h": (want, tol)} in float64."""
    f64 = torch.float64
    N, H = inp["h_prev"].shape
    b = inp["b"].to(f64)
    pre = b.reshape(1, 4 * H).expand(N, 4 * H).clone()
    mag = b.abs().reshape(1, 4 * H).expand(N, 4 * H).clone()
    for a, w in _segments(inp, f64):
        pre += a @ w.t()
        mag += a.abs() @ w.abs().t()
    tol_pre = (inp["K"] + 4) * E32 * mag
    pre = pre.reshape(N, 4, H)
    tol_pre = tol_pre.reshape(N, 4, H)

    def sig(x, tx):
        s = torch.sigmoid(x)
        return s, s * ((1.0 + x.abs()) * 2.0 ** -20 + 3 * E32) + 0.25 * tx

    (gi, ti), (gf, tf), (go, to) = (sig(pre[:, k], tol_pre[:, k])
                                    for k in range(3))
    gg = torch.tanh(pre[:, 3])
    tg = (INTR + E32) * gg.abs() + tol_pre[:, 3]
    cpc = inp["c_prev"].to(f64) * inp["cont"].to(f64).reshape(N, 1)
    c = gf * cpc + gi * gg
    tol_c = (_ptol((gf, tf), _exact(cpc)) + _ptol((gi, ti), (gg.abs(), tg))
             + 4 * E32 * ((gf * cpc).abs() + (gi * gg).abs()))
    tc = torch.tanh(c)
    ttc = (INTR + E32) * tc.abs() + tol_c + E32
    hh = go * tc
    tol_h = U * hh.abs() + _ptol((go, to), (tc.abs(), ttc)) \
        + 2 * E32 * hh.abs()
    return {"c": (c, tol_c + E32 * c.abs()), "h": (hh, tol_h)}


def emulate(inp, round_pre=False, ignore_cont=False):
    """The kernel's arithmetic in fp32 on the CPU.  round_pre and
    ignore_cont are the mutants: pre-activations rounded to bf16 (what the
    unrolled route does), and h_prev / c_prev taken ungated."""
    f32 = torch.float32
    N, H = inp["h_prev"].shape
    pre = inp["b"].to(f32).reshape(1, 4 * H).expand(N, 4 * H).clone()
    for a, w in _segments(inp, f32, use_cont=not ignore_cont):
        pre += a @ w.t()
    if round_pre:
        pre = pre.to(BF).to(f32)
    pre = pre.reshape(N, 4, H)
    gi, gf, go = (1.0 / (1.0 + torch.exp(-pre[:, k])) for k in range(3))
    gg = torch.tanh(pre[:, 3])
    ct = 1.0 if ignore_cont else inp["cont"].reshape(N, 1)
    c = gf * inp["c_prev"] * ct + gi * gg
    return {"c": c, "h": (go * torch.tanh(c)).to(BF)}
