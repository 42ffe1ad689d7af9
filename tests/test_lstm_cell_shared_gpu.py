"""One LSTM cell behind every route: the whole-sequence routes
(csrc/lstm_persist.hip, csrc/lstm_seq.hip) and the fused decode step
(csrc/lstm_step.hip) give the very bits of the unit op
(csrc/elementwise.hip) wherever their pre-activations are exactly the
unit op's gates.  All four call csrc/lstm_cell.h; a cell edited in one
kernel only, or contracted differently in two of them, fails here."""

import pytest
import torch

import _lstm_seq_cases as C
from _bf16_bounds import BF, gen
from caffeonspark_amd import ops

gpu = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _settle(route):
    """A watchdog abort of the persistent kernel fails this test, not the
    one after it."""
    from caffeonspark_amd.ops import gpu as g

    torch.cuda.synchronize()
    if route == "persist":
        g._persist_check_pending(force=True)


def same_bits(a, b):
    ints = {2: torch.int16, 4: torch.int32}
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.view(ints[a.element_size()]), b.view(ints[b.element_size()]))


# T = 1: h_in[0] == 0, so the recurrent term is exactly zero on both routes
# whatever the accumulation order, and the pre-activations are xg[0].
SEQ = [
    ((1, 5, 40), False, "persist"),   # ragged last slice, 3 blocks
    ((1, 5, 40), True, "loop"),
    ((1, 3, 20), False, "loop"),      # H % 8 != 0: the persistent kernel
                                      # declines it
]


@gpu
@pytest.mark.parametrize("shape,forced,route", SEQ,
                         ids=[f"N{s[1]}-H{s[2]}-{r}" for s, _, r in SEQ])
def test_seq_routes_give_the_unit_ops_bits_at_T1(shape, forced, route,
                                                 monkeypatch):
    monkeypatch.delenv("COS_LSTM_PERSIST", raising=False)
    if forced:
        monkeypatch.setenv("COS_LSTM_PERSIST", "0")
    T, N, H = shape
    inp = C.inputs(*shape)
    d = dev()
    cont = torch.zeros(T, N)
    cont[0, ::2] = 1                  # a mix of 0 and 1
    xg, w, dy, cont = (t.to(d) for t in (inp["xg"], inp["w_hc"], inp["dy"],
                                         cont))

    fctx, bctx = {}, {}
    h, cache = ops.gpu_op("lstm_seq_forward")(xg, w, cont, fctx)
    _settle(fctx["route"])
    dxg, _ = ops.gpu_op("lstm_seq_backward")(dy, w, cache, bctx)
    _settle(bctx["route"])
    assert (fctx["route"], bctx["route"]) == (route, route)
    c, act = cache[2], cache[3]

    zero = torch.zeros(N, H, device=d)
    c_u, h_u, ucache = ops.gpu_op("lstm_unit_forward")(zero, xg[0], cont[0])
    _, dg_u = ops.gpu_op("lstm_unit_backward")(zero, ucache, zero, dy[0])
    torch.cuda.synchronize()
    assert same_bits(h[0], h_u)
    assert same_bits(c[0], c_u)
    assert same_bits(act[0], ucache[2].reshape(N, 4 * H))
    assert same_bits(dxg[0], dg_u)


@gpu
def test_fused_step_gives_the_unit_ops_bits():
    """x = 0 and h_prev = 0: the pre-activations are exactly the bias, and
    c_prev * cont goes through the shared cell with a non-zero c_prev."""
    N, D, H = 3, 8, 24
    g = gen(24)
    d = dev()
    w_xc = torch.randn(4 * H, D, generator=g).to(BF).to(d)
    w_hc = torch.randn(4 * H, H, generator=g).to(BF).to(d)
    b = (torch.randn(4 * H, generator=g) * 1.5).to(BF).to(d)
    c_prev = torch.randn(N, H, generator=g).to(d)
    cont = torch.tensor([1.0, 0.0, 1.0], device=d)
    x = torch.zeros(N, D, dtype=BF, device=d)
    h_prev = torch.zeros(N, H, dtype=BF, device=d)
    assert ops.gpu_op("lstm_step_ok")(N, D, H, 0,
                                      [x, h_prev, w_xc, w_hc, b])
    h, c = ops.gpu_op("lstm_step")(x, h_prev, c_prev, cont, w_xc, b, w_hc)
    c_u, h_u, _ = ops.gpu_op("lstm_unit_forward")(
        c_prev, b.reshape(1, 4 * H).expand(N, 4 * H), cont)
    torch.cuda.synchronize()
    assert same_bits(h, h_u)
    assert same_bits(c, c_u)
