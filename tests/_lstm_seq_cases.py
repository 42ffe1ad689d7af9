"""Float64 oracle, derived bounds, CPU emulation and mutants for the two
whole-sequence LSTM routes behind ops.gpu.lstm_seq_forward / _backward:

 persist  csrc/lstm_persist.hip: one kernel for all T steps, recurrent
          weights stationary in MFMA fragments, c / dc / dh in LDS.
 loop     csrc/lstm_seq.hip: per step a rowscale kernel, a split-K atomic
          GEMM into fp32 and lstm_unit2_*.

Shared by test_lstm_seq_bounds.py (CPU) and test_lstm_seq_gpu.py (GPU).
Notation and rules B1-B4 are those of _bf16_bounds.py; the gate, c and h
bounds are those of _lstm_step_cases.py.

A bound compounded over T steps would be too wide to catch anything, so the
oracle is STEP-WISE and fed the route's own emitted state: both routes hand
out per-step h, c, act and h_in in the cache tuple and dxg from the
backward.  What a step reads from them is an exact input, as xhat and
invstd are for the BatchNorm backward oracle.

Forward, step t.  Inputs h_in[t] (bf16) and c[t-1] (fp32) as emitted.

 pre    xg[t] + h_in[t] @ W_hc^T.  bf16 x bf16 products are exact in fp32,
        only the accumulation (MFMA chain, cross-wave LDS reduce or split-K
        atomics, the xg add) rounds: rule B3, (H+4) e (|xg| + |h_in| @
        |W|^T).
 gates, c, h, act   as the oracle of _lstm_step_cases.py; cont[t] c[t-1] is
        exact (cont is 0 or 1).

Forward linkage, bit-exact: h_in[0] == 0 and h_in[t] == bf16(h[t-1] cont[t])
of the route's own h (the product is exact, so both routes' rounding points
give the same bits).  With the step-wise bound this covers the whole
recurrence by induction.

Backward, step t.  act[t], c[t], c[t-1] as emitted are inputs: the gate
tolerances are zero, tanh(c[t]) carries (I+e)|t|.

 dh_rec cont[t+1] (dxg[t+1] @ W_hc) of the route's own bf16 dxg[t+1]:
        (4H+4) e (|dxg| @ |W|).  The loop route stores it as bf16
        (rowscale_f32_kernel): one further u on the computed value, u
        (|dh_rec| + the accumulation bound).  The persistent route keeps it
        in fp32 in LDS and adds nothing.
 dhv    dy[t] + dh_rec, one fp32 add: e (|dy| + |dh_rec|).
 dc     is not emitted.  It is carried in float64 with a magnitude (sum of
        absolute terms) and a tolerance: dc[t] = carry + dhv go (1 - tc^2)
        gets the carry's tolerance, the _ptol of the product and 3e of the
        magnitude; the carry into t-1 is cont gf dc[t] with tolerance
        cont gf (tol_dc + 4e mag).  gf <= 1, so the carried tolerance grows
        by addition only.
 dxg    per gate u T + _ptol(...) + 4e T, T the product of the factors'
        magnitudes, as the dgates of lstm_oracle.

Weight gradient: dwhc against dxg^T @ h_in of the route's own emitted
tensors, (T N + 4) e (|dxg|^T @ |h_in|).
"""

import torch

from _bf16_bounds import BF, E32, INTR, U, _exact, _ptol, gen, rb

# (T, N, H), the route taken when nothing is set in the environment
CASES = [
    ((1, 1, 24), "persist"),     # smallest eligible: 2 blocks, 8-column
                                 # last slice, waves 1-3 all-zero K window
    ((3, 5, 40), "persist"),     # ragged slice, K-window tail in wave 1
    ((4, 64, 64), "persist"),    # every row fragment full
    ((3, 17, 136), "persist"),   # 2 k-steps, tail in wave 2, 9 blocks
    ((3, 3, 1000), "persist"),   # LRCN width: 63 blocks, tail in wave 3
    ((2, 2, 1024), "persist"),   # full 8 and 32 k-step windows
    ((3, 65, 24), "loop"),       # N > 64
    ((3, 4, 16), "loop"),        # one block only
    ((3, 4, 20), "loop"),        # H % 8 != 0
    ((2, 2, 1032), "loop"),      # H > 1024
]

# every persist-eligible case also runs on the loop route
RUNS = [(shape, route, forced)
        for shape, route in CASES
        for forced in ((False, True) if route == "persist" else (False,))]


def run_route(route, forced):
    return "loop" if forced else route


def run_id(run):
    (T, N, H), route, forced = run
    return f"T{T}-N{N}-H{H}-{run_route(route, forced)}"


def inputs(T, N, H, seed=0):
    g = gen(seed + 7919 * T + 131 * N + H)
    sw = 1.6 / (H / 3.0) ** 0.5
    cont = torch.ones(T, N)
    cont[0] = 0
    if T >= 3:
        cont[2, 1::3] = 0           # streams 1, 4, 7, ... restart at t = 2
    return dict(
        w_hc=(torch.randn(4 * H, H, generator=g) * sw).to(BF),
        xg=(torch.randn(T, N, 4 * H, generator=g) * 1.2).to(BF),
        dy=torch.randn(T, N, H, generator=g).to(BF),
        cont=cont)


def _sig(x, tx):
    s = torch.sigmoid(x)
    return s, s * ((1.0 + x.abs()) * 2.0 ** -20 + 3 * E32) + 0.25 * tx


def oracle(inp, em, route):
    """{"h", "c", "act", "h_in", "dxg", "dwhc": (want, tol)} in float64.
    em holds the route's own emitted h, c, act, h_in and dxg."""
    f64 = torch.float64
    T, N, H4 = inp["xg"].shape
    H = H4 // 4
    W = inp["w_hc"].to(f64)
    aW = W.abs()
    xg, dy = inp["xg"].to(f64), inp["dy"].to(f64)
    cont = inp["cont"].to(f64).reshape(T, N, 1)
    h_in = em["h_in"].detach().cpu().to(f64)
    c_em = em["c"].detach().cpu().to(f64)
    h_em = em["h"].detach().cpu()
    zero = torch.zeros(N, H, dtype=f64)

    # ---- forward, one step at a time from the emitted h_in[t], c[t-1]
    hs, cs, acts = [], [], []
    for t in range(T):
        a = h_in[t]
        pre = xg[t] + a @ W.t()
        mag = xg[t].abs() + a.abs() @ aW.t()
        tol_pre = ((H + 4) * E32 * mag).reshape(N, 4, H)
        pre = pre.reshape(N, 4, H)
        (gi, ti), (gf, tf), (go, to) = (_sig(pre[:, k], tol_pre[:, k])
                                        for k in range(3))
        gg = torch.tanh(pre[:, 3])
        tg = (INTR + E32) * gg.abs() + tol_pre[:, 3]
        cpc = (c_em[t - 1] if t else zero) * cont[t]
        c = gf * cpc + gi * gg
        tol_c = (_ptol((gf, tf), _exact(cpc))
                 + _ptol((gi, ti), (gg.abs(), tg))
                 + 4 * E32 * ((gf * cpc).abs() + (gi * gg).abs()))
        tc = torch.tanh(c)
        ttc = (INTR + E32) * tc.abs() + tol_c + E32
        hh = go * tc
        tol_h = U * hh.abs() + _ptol((go, to), (tc.abs(), ttc)) \
            + 2 * E32 * hh.abs()
        hs.append((hh, tol_h))
        cs.append((c, tol_c + E32 * c.abs()))
        acts.append((torch.stack([gi, gf, go, gg], 1).reshape(N, H4),
                     torch.stack([ti, tf, to, tg], 1).reshape(N, H4)))

    # ---- linkage: h_in from the route's own h, bit for bit
    want_h_in = torch.zeros(T, N, H, dtype=BF)
    if T > 1:
        want_h_in[1:] = (h_em[:-1].float()
                         * inp["cont"][1:].reshape(T - 1, N, 1)).to(BF)

    # ---- backward, from the emitted act, c and dxg[t+1]
    act = em["act"].detach().cpu().to(f64).reshape(T, N, 4, H)
    dxg_em = em["dxg"].detach().cpu().to(f64)
    carry, mag_carry, tol_carry = zero, zero, zero
    dxgs = [None] * T
    for t in range(T - 1, -1, -1):
        gi, gf, go, gg = act[t].unbind(1)
        if t + 1 < T:
            d = dxg_em[t + 1]
            dh = cont[t + 1] * (d @ W)
            tol_dh = (4 * H + 4) * E32 * cont[t + 1] * (d.abs() @ aW)
            if route == "loop":
                tol_dh = tol_dh + U * (dh.abs() + tol_dh)
        else:
            dh, tol_dh = zero, zero
        dhv = dy[t] + dh
        mag_dhv = dy[t].abs() + dh.abs()
        fdhv = (mag_dhv, tol_dh + E32 * mag_dhv)
        tc = torch.tanh(c_em[t])
        ftc = (tc.abs(), (INTR + E32) * tc.abs())
        f_tc2 = (1 - tc * tc, 2 * tc.abs() * ftc[1] + 2 * E32)
        dc = carry + dhv * go * f_tc2[0]
        mag_dc = mag_carry + mag_dhv * go * f_tc2[0]
        tol_dc = tol_carry + _ptol(fdhv, _exact(go), f_tc2) + 3 * E32 * mag_dc
        fdc = (mag_dc, tol_dc)
        cpc = (c_em[t - 1] if t else zero) * cont[t]

        def out(value, *factors):
            mag = 1.0
            for mf, _ in factors:
                mag = mag * mf
            return value, U * mag + _ptol(*factors) + 4 * E32 * mag

        one_m = lambda s: (1 - s, E32 + torch.zeros_like(s))    # noqa: E731
        outs = [out(dc * gg * gi * (1 - gi), fdc, _exact(gg), _exact(gi),
                    one_m(gi)),
                out(dc * cpc * gf * (1 - gf), fdc, _exact(cpc), _exact(gf),
                    one_m(gf)),
                out(dhv * tc * go * (1 - go), fdhv, ftc, _exact(go),
                    one_m(go)),
                out(dc * gi * (1 - gg * gg), fdc, _exact(gi),
                    (1 - gg * gg, 2 * E32 + torch.zeros_like(gg)))]
        dxgs[t] = (torch.stack([o[0] for o in outs], 1).reshape(N, H4),
                   torch.stack([o[1] for o in outs], 1).reshape(N, H4))
        carry = dc * gf * cont[t]
        mag_carry = mag_dc * gf * cont[t]
        tol_carry = cont[t] * gf * (tol_dc + 4 * E32 * mag_dc)

    # ---- weight gradient of the emitted dxg and h_in
    dflat, hflat = dxg_em.reshape(T * N, H4), h_in.reshape(T * N, H)
    dw = dflat.t() @ hflat
    tol_dw = (T * N + 4) * E32 * (dflat.abs().t() @ hflat.abs())

    def cat(pairs):
        return (torch.stack([p[0] for p in pairs]),
                torch.stack([p[1] for p in pairs]))

    return {"h": cat(hs), "c": cat(cs), "act": cat(acts),
            "h_in": (want_h_in, None), "dxg": cat(dxgs),
            "dwhc": (dw, tol_dw)}


MUTANTS = ("cont_prev", "no_c_gate", "no_dh_gate", "dc_drop", "round_pre",
           "k_tail_dropped", "slice_tail_dropped")
FIRST_FIVE = MUTANTS[:5]


def tail_is_empty(mutant, H):
    """True where the mutant's dropped tail holds nothing at this H."""
    return (mutant == "k_tail_dropped" and H % 32 == 0) or \
        (mutant == "slice_tail_dropped" and H % 16 == 0)


def emulate(inp, route, mutant=None):
    """Both routes' arithmetic in fp32 on the CPU, bf16 at their rounding
    points (h, h_in, dxg; the loop route's dh_rec).  Returns what the
    routes emit.  Mutants:

     cont_prev           h_in[t] gated with cont[t-1]
     no_c_gate           c[t-1] enters c[t] ungated
     no_dh_gate          dh into step t ungated by cont[t+1]
     dc_drop             the carried dc is lost once, into step T-2
     round_pre           pre-activations rounded to bf16
     k_tail_dropped      the recurrent dot stops at floor(H/32)*32
     slice_tail_dropped  columns >= floor(H/16)*16 are never written and
                         keep their previous value (zero here)
    """
    assert mutant is None or mutant in MUTANTS
    T, N, H4 = inp["xg"].shape
    H = H4 // 4
    W, xg, dy = inp["w_hc"].float(), inp["xg"].float(), inp["dy"].float()
    cont = inp["cont"].float().reshape(T, N, 1)
    kd = (H // 32) * 32 if mutant == "k_tail_dropped" else H
    js = (H // 16) * 16 if mutant == "slice_tail_dropped" else H

    h = torch.zeros(T, N, H)
    c = torch.zeros(T, N, H)
    act = torch.zeros(T, N, 4, H)
    h_in = torch.zeros(T, N, H)
    for t in range(T):
        if t:
            gate = cont[t - 1] if mutant == "cont_prev" else cont[t]
            h_in[t, :, :js] = rb(h[t - 1] * gate)[:, :js]
        pre = xg[t] + h_in[t][:, :kd] @ W[:, :kd].t()
        if mutant == "round_pre":
            pre = rb(pre)
        pre = pre.reshape(N, 4, H)
        gi, gf, go = (1.0 / (1.0 + torch.exp(-pre[:, k])) for k in range(3))
        gg = torch.tanh(pre[:, 3])
        cp = c[t - 1] if t else torch.zeros(N, H)
        ct = 1.0 if mutant == "no_c_gate" else cont[t]
        cv = gf * cp * ct + gi * gg
        c[t, :, :js] = cv[:, :js]
        h[t, :, :js] = rb(go * torch.tanh(cv))[:, :js]
        act[t, :, :, :js] = torch.stack([gi, gf, go, gg], 1)[:, :, :js]

    dxg = torch.zeros(T, N, 4, H)
    dc_next = torch.zeros(N, H)
    for t in range(T - 1, -1, -1):
        gi, gf, go, gg = act[t].unbind(1)
        tc = torch.tanh(c[t])
        if t + 1 < T:
            dh = dxg[t + 1].reshape(N, H4) @ W
            if mutant != "no_dh_gate":
                dh = dh * cont[t + 1]
            if route == "loop":
                dh = rb(dh)
        else:
            dh = torch.zeros(N, H)
        dhv = dy[t] + dh
        if mutant == "dc_drop" and t == T - 2:
            dc_next = torch.zeros(N, H)
        dc = dc_next + dhv * go * (1.0 - tc * tc)
        cp = c[t - 1] if t else torch.zeros(N, H)
        dg = torch.stack([dc * gg * gi * (1.0 - gi),
                          dc * cp * cont[t] * gf * (1.0 - gf),
                          dhv * tc * go * (1.0 - go),
                          dc * gi * (1.0 - gg * gg)], 1)
        dxg[t, :, :, :js] = rb(dg)[:, :, :js]
        dc_next = dc * gf * cont[t]
    dxg = dxg.reshape(T, N, H4)
    dwhc = dxg.reshape(T * N, H4).t() @ h_in.reshape(T * N, H)
    return {"h": h.to(BF), "c": c, "act": act.reshape(T, N, H4),
            "h_in": h_in.to(BF), "dxg": dxg.to(BF), "dwhc": dwhc}
