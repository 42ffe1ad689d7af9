"""Cases, the float64 per-step loop and the derived bf16 bounds of the RNN
tests (test_rnn_layer.py on the CPU, test_rnn_seq_gpu.py on the GPU).

Every input is bf16-representable, so the float64 loop and the kernels read
the same numbers.  W_hh and W_ho have row AND column absolute sums <= 0.5
(backward contracts over the other index); b_o ~ 1.5 N(0,1) takes the output
stage's z into tanh's nonlinear range.  u = 2^-8 (bf16), e = 2^-24 (fp32),
I = 2^-16 (tanhf, rule B4 of _bf16_bounds).

Forward, end to end.  h_t = bf16(tanh(pre_t)), pre_t = W_hh (cont_t h_{t-1})
+ xg_t in fp32; cont is 0 or 1, so cont_t h_{t-1} is exact.  tanh is
1-Lipschitz and the row sums give e_t <= r + 0.5 e_{t-1}, so e_t <= 2r with
r the sum of
  u * 1                       the stored |h| < 1 rounded to bf16,
  nx * u * XG                 the roundings of xg to bf16: nx = 1, or 3 with
                              x_static (two products and their sum); XG =
                              max(|x| |W_xh|^T + |b_h| + |xs| |W_xsh|^T),
  (K + 8) e (XG + 0.5) + I    fp32 accumulation over K = H (+ D + Ds for xg)
                              terms of absolute sum <= XG + 0.5, and tanhf.
o = bf16(tanh(bf16(W_ho h + b_o))): 0.5 * 2r + r1 (|h||W_ho|^T + |b_o|) + I +
u per element, r1 = u + (H+4)e being a bf16 result of an H-term fp32 sum.

Backward.  dpre_t = bf16(dh_t (1 - h_t^2)), dh_t = dho_t + cont_{t+1}
(dpre_{t+1} W_hh).  The kernel's h is off by 2r, so 1 - h^2 by c1 = 4r(1+r).
With DE_t the bound of dh_t's error, G_t of dpre_t's follows t = T-1 .. 0:
  DE_t = E_dho_t + cont_{t+1} ((G_{t+1} + (H+4)e (|dpre_{t+1}| + G_{t+1}))
         |W_hh|),
  G_t  = DE_t (1 + c1 + u) + (c1 + 4e)|dh_t| + u |dpre_t|,
|dh|, |dpre| from the float64 loop; the expression at t = 0 bounds dh_0 =
cont_0 (dpre_0 W_hh).  For the op dho is an input (E_dho = 0).

The layer's backward is held stage by stage, each against float64 of the
tensors the layer itself produced before it, so no bound carries a worst case
over T N rows: dz = bf16(do (1 - o^2)): (u + 4e)|dz|; dpre as above from dho =
dz W_ho, E_dho = r1 |dz||W_ho|; GEMM gradients A^T B over K rows (fp32 out):
(K+4)e |A|^T|B|; dx = bf16(dpre W_xh): r1 |dpre||W_xh|; d_static = bf16(sum_t
dpre_t) is off by ES = (u + (T+4)e) sum_t |dpre_t|, which enters its products.
"""

import torch

from _bf16_bounds import E32, INTR, U, rb

F64 = torch.float64

# T, N, H, D, Ds (0: no x_static), expose, cont reset, COS_RNN_SEQ, GPU route
CASES = [
    (1, 3, 32, 8, 0, False, False, None, "resident"),
    (5, 17, 96, 24, 8, False, True, None, "resident"),
    (4, 16, 64, 16, 0, True, False, None, "resident"),
    (3, 2, 40, 5, 0, False, False, None, "loop"),
    (5, 17, 96, 24, 8, False, True, "0", "loop"),
]
BLOBS = {False: ["W_xh", "b_h", "W_hh", "W_ho", "b_o"],
         True: ["W_xh", "b_h", "W_xsh", "W_hh", "W_ho", "b_o"]}


def case_id(c):
    return f"T{c[0]}N{c[1]}H{c[2]}Ds{c[4]}" + ("_env0" if c[7] else "")


def _half_sums(w):
    """Scale w so its bf16 image has row and column abs sums <= 0.5."""
    w = rb(w * (0.49 / max(w.abs().sum(0).max(), w.abs().sum(1).max())))
    assert max(w.abs().sum(0).max(), w.abs().sum(1).max()) <= 0.5
    return w


def inputs(case):
    T, N, H, D, Ds, expose, reset = case[:7]
    g = torch.Generator().manual_seed(1000 * T + N + H)
    rn = lambda *s: torch.randn(*s, generator=g)            # noqa: E731
    cont = torch.ones(T, N)
    cont[0] = 0 if not expose else 1
    if reset:
        cont[2, ::3] = 0
    inp = dict(x=rb(rn(T, N, D)), cont=cont, do=rb(rn(T, N, H)),
               W_xh=rb(rn(H, D) * 0.5 / D), b_h=rb(rn(H) * 0.1),
               W_hh=_half_sums(rn(H, H)), W_ho=_half_sums(rn(H, H)),
               b_o=rb(rn(H) * 1.5))
    if Ds:
        inp.update(xs=rb(rn(N, Ds)), W_xsh=rb(rn(H, Ds) * 0.5 / Ds))
    if expose:
        inp.update(h0=rb(rn(N, H).clamp(-0.9, 0.9)), dhT=rb(rn(N, H)))
    return inp


def f64(d):
    return {k: v.to(F64) for k, v in d.items()}


def xg64(p):
    """x W_xh^T + b_h [+ xs W_xsh^T] as [T, N, H]."""
    T, N = p["cont"].shape
    xg = (p["x"].reshape(T * N, -1) @ p["W_xh"].t() + p["b_h"]).reshape(
        T, N, -1)
    return xg + (p["xs"] @ p["W_xsh"].t()).unsqueeze(0) if "xs" in p else xg


def forward64(p, xg=None):
    """The plain per-step loop in float64 from a dict of float64 tensors;
    with xg given, the recurrence alone (o is None).  Returns o and the
    lists over t of h_t, hc_t = cont_t h_{t-1} and pre_t."""
    whole = xg is None
    xg = xg64(p) if whole else xg
    h = p["h0"] if "h0" in p else torch.zeros_like(xg[0])
    hs, hc, pre = [], [], []
    for t, xg_t in enumerate(xg):
        hc.append(h * p["cont"][t].unsqueeze(1))
        pre.append(hc[t] @ p["W_hh"].t() + xg_t)
        h = torch.tanh(pre[t])
        hs.append(h)
    o = torch.tanh(torch.stack(hs) @ p["W_ho"].t() + p["b_o"]) if whole \
        else None
    return o, hs, hc, pre


def loss64(p, o, hs):
    """L = sum(do * o) + sum(dhT * h_T); the recurrence alone has hs for o."""
    loss = (p["do"] * (torch.stack(hs) if o is None else o)).sum()
    return loss + (p["dhT"] * hs[-1]).sum() if "dhT" in p else loss


def loop64(inp, xg=None):
    """forward64 and the gradients of loss64 by autograd: dpre, dh (all of
    the gradient reaching h_t) and grad[name] of every input."""
    p = {k: v.requires_grad_(k != "cont") for k, v in f64(inp).items()}
    o, hs, hc, pre = forward64(p, None if xg is None else xg.to(F64))
    for t in pre + hs:
        t.retain_grad()
    loss64(p, o, hs).backward()
    st = lambda ts: torch.stack([t.detach() for t in ts])   # noqa: E731
    return dict(o=None if o is None else o.detach(), hs=st(hs), hc=st(hc),
                dpre=st([t.grad for t in pre]), dh=st([t.grad for t in hs]),
                grad={k: v.grad for k, v in p.items() if v.grad is not None})


def r_fwd(H, XG, nx=1, kx=0):
    return U + nx * U * XG + (H + kx + 8) * E32 * (XG + 0.5) + INTR


def dpre_bound(ref, inp, H, r, e_dho=None):
    """Elementwise bound G [T, N, H] of dpre's error and [N, H] of dh_0's,
    by the backward sweep of the module docstring; e_dho bounds dho's."""
    W, cont = inp["W_hh"].to(F64).abs(), inp["cont"].to(F64)
    c1, acc = 4 * r * (1 + r), (H + 4) * E32
    dpre, dh = ref["dpre"].abs(), ref["dh"].abs()
    G, rec = [None] * len(dpre), torch.zeros_like(dpre[0])
    for t in reversed(range(len(dpre))):
        de = rec if e_dho is None else rec + e_dho[t]
        G[t] = de * (1 + c1 + U) + (c1 + 4 * E32) * dh[t] + U * dpre[t]
        rec = cont[t].unsqueeze(1) * ((G[t] + acc * (dpre[t] + G[t])) @ W)
    return torch.stack(G), rec


def seq_xg(inp):
    """The recurrence's input: the layer's xg rounded to bf16."""
    return rb(xg64(f64(inp)).float())


def seq_oracle(case, inp, xg):
    """{name: (float64 value, bound)} of the recurrence alone."""
    ref = loop64(inp, xg)
    r = r_fwd(case[2], float(xg.abs().max()))
    g, g0 = dpre_bound(ref, inp, case[2], r)
    orc = dict(hs=(ref["hs"], 2 * r), hc=(ref["hc"], 2 * r),
               dpre=(ref["dpre"], g))
    if "h0" in inp:
        orc["dh0"] = (ref["grad"]["h0"], g0)
    return orc


def emulate_seq(xg, w_hh, cont, h0, dho, dhT):
    """The kernels' arithmetic on the CPU: fp32 with bf16 stores."""
    T, N, H = xg.shape
    h = torch.zeros(N, H) if h0 is None else h0
    hs, hc = [], []
    for t in range(T):
        hc.append(rb(h * cont[t].unsqueeze(1)))
        h = rb(torch.tanh(hc[t] @ w_hh.t() + xg[t]))
        hs.append(h)
    dpre = [None] * T
    carry = torch.zeros(N, H) if dhT is None else dhT
    for t in reversed(range(T)):
        dpre[t] = rb((dho[t] + carry) * (1 - hs[t] * hs[t]))
        carry = (dpre[t] @ w_hh) * cont[t].unsqueeze(1)
    out = dict(hs=torch.stack(hs), hc=torch.stack(hc), dpre=torch.stack(dpre))
    return dict(out, dh0=carry) if h0 is not None else out


# ------------------------------------------------------------------ the layer

def run_layer(case, inp, device=None, dtype=torch.float32):
    """A one-layer net on `device`: forward, then the layer's backward from
    do (and dhT).  Returns (tops, gradients and the layer's own stage
    tensors hs, hc, dz, dpre by name, the layer)."""
    from caffeonspark_amd.core.net import Net
    from caffeonspark_amd.proto import caffe_pb, text_format

    T, N, H, D, Ds, expose = case[:6]
    bots = ["x", "cont"] + (["xs"] if Ds else []) + (["h0"] if expose else [])
    shapes = dict(x=(T, N, D), cont=(T, N), xs=(N, Ds), h0=(1, N, H))
    dims = lambda b: " ".join(f"dim: {d}" for d in shapes[b])  # noqa: E731
    text = "".join(f'input: "{b}" input_shape {{ {dims(b)} }}\n'
                   for b in bots) + 'layer { name: "rnn" type: "RNN" ' \
        + " ".join(f'bottom: "{b}"' for b in bots) + ' top: "o" ' \
        + ('top: "hT" ' if expose else "") + "recurrent_param { " \
        + f"num_output: {H} expose_hidden: {str(expose).lower()} }} }}"
    net = Net(text_format.parse(text, caffe_pb.NetParameter),
              caffe_pb.NetState(phase=caffe_pb.Phase.TRAIN), device=device,
              dtype=dtype, seed=1)
    layer = net.layers[-1]
    # blob order and shapes: W_xh, b_h, [W_xsh], W_hh, W_ho, b_o
    assert [(b.name, tuple(b.data.shape)) for b in layer.blobs] == \
        [("rnn_" + k.replace("_", ""), tuple(inp[k].shape))
         for k in BLOBS[bool(Ds)]]
    for b, k in zip(layer.blobs, BLOBS[bool(Ds)]):
        b.data.copy_(inp[k])
        b.zero_diff()
    for b in bots:
        net.blob_by_name(b).data = inp[b].reshape(shapes[b]).to(
            device, torch.float32 if b == "cont" else dtype)
    net.forward()
    fwd_route = layer.seq_route
    tops, bottoms = net.layer_tops[-1], net.layer_bottoms[-1]
    tops[0].diff = inp["do"].to(device, dtype)
    if expose:
        tops[1].diff = inp["dhT"].reshape(1, N, H).to(device, dtype)
    state = layer._backward_state(tops)
    layer._backward_grads(*state, [b != "cont" for b in bots], bottoms)
    assert layer.seq_route == fwd_route
    out = dict(o=tops[0].data, dx=bottoms[0].diff, hs=layer._cache[1],
               hc=layer._cache[3][2], dz=state[0].reshape(T, N, H),
               dpre=state[2])
    if expose:
        out.update(hT=tops[1].data[0], dh0=bottoms[-1].diff[0])
    if Ds:
        out["dxs"] = bottoms[2].diff
    out.update({k: b.diff for b, k in zip(layer.blobs, BLOBS[bool(Ds)])})
    return {k: v.detach().float().cpu() for k, v in out.items()}, layer


def layer_oracle(case, inp, out):
    """{name: (float64 value, bound)} for run_layer's outputs `out` on the
    bf16 path, by the staging of the module docstring."""
    T, N, H, D, Ds, expose = case[:6]
    p, k = f64(inp), f64(out)
    ref = loop64(inp)
    XG = float((xg64({n: v.abs() for n, v in p.items()})).max())
    e_h = 2 * r_fwd(H, XG, 3 if Ds else 1, D + Ds)
    r1 = U + (H + 4) * E32
    who, wxh = p["W_ho"].abs(), p["W_xh"].abs()
    orc = dict(hs=(ref["hs"], e_h), hc=(ref["hc"], e_h),
               o=(ref["o"], 0.5 * e_h + INTR + U + r1 * (
                   ref["hs"].abs() @ who.t() + p["b_o"].abs())))
    dz = p["do"] * (1 - k["o"] ** 2)
    orc["dz"] = (dz, (U + 4 * E32) * dz.abs())
    # the recurrence backward from the layer's own dz
    back = loop64(dict(inp, do=k["dz"] @ p["W_ho"]), xg64(p))
    g, g0 = dpre_bound(back, inp, H, e_h / 2, r1 * (k["dz"].abs() @ who))
    orc["dpre"] = (back["dpre"], g)
    # GEMMs of the layer's own operands, K = T N rows
    f2 = lambda t: t.reshape(T * N, -1)                     # noqa: E731

    def gemm(A, B, K=T * N):
        return A.t() @ B, (K + 4) * E32 * (A.abs().t() @ B.abs())
    dpre, ones = f2(k["dpre"]), torch.ones(T * N, 1, dtype=F64)
    orc.update(W_ho=gemm(f2(k["dz"]), f2(k["hs"])),
               b_o=tuple(v[:, 0] for v in gemm(f2(k["dz"]), ones)),
               W_hh=gemm(dpre, f2(k["hc"])), W_xh=gemm(dpre, f2(p["x"])),
               b_h=tuple(v[:, 0] for v in gemm(dpre, ones)),
               dx=((dpre @ p["W_xh"]).reshape(T, N, D),
                   (r1 * (dpre.abs() @ wxh)).reshape(T, N, D)))
    if expose:
        orc.update(hT=(ref["hs"][-1], e_h),
                   dh0=(back["grad"]["h0"], g0 + U * back["grad"]["h0"].abs()))
    if Ds:
        ds, wxs = k["dpre"].sum(0), p["W_xsh"].abs()
        es = (U + (T + 4) * E32) * k["dpre"].abs().sum(0)
        w, tw = gemm(ds, p["xs"], N)
        orc.update(W_xsh=(w, tw + es.t() @ p["xs"].abs()),
                   dxs=(ds @ p["W_xsh"],
                        es @ wxs + r1 * ((ds.abs() + es) @ wxs)))
    return orc
