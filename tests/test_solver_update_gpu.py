"""The fused whole-arena solver updates on the GPU against the float64
bounds of _solver_update_cases.py (shown sound on the CPU by
test_solver_update_bounds.py): the three kernels called directly on every
layout with and without the bf16 shadow, the arena wrappers at the LDS
table's capacity and one segment past it, the single-tensor sgd_update on
views that start off a 16-byte boundary, and a real Solver per type on a
net whose blobs start at odd offsets."""

import types

import pytest
import torch

import _bf16_bounds as B
import _solver_update_cases as S

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G


def dev():
    return torch.device("cuda:0")


def d(t):
    return t.to(dev())


def ext():
    assert ops.native_available(), "HIP extension not loaded"
    return G._ext


def check(case, out, sh, what):
    """p, v (, m) against the oracle; the shadow against bf16 of the p the
    kernel itself wrote (sentinel where frozen); nothing left behind."""
    B.assert_within(out, S.oracle(case), what)
    if sh is not None:
        B.assert_within({"sh": sh}, S.shadow_expect(case, out["p"]), what)
    missed = S.missed_elements(case, out)
    assert not missed, f"{what}: never updated {missed[:16]}"
    frozen = ~S.trainable(case)
    for name, t in out.items():
        assert torch.equal(t.cpu()[frozen], case[name][frozen]), \
            f"{what}: frozen {name} touched"


# ------------------------------------------------- direct kernel calls

def launch(case, shadow):
    e = ext()
    solver = case["solver"]
    out = {n: d(case[n]) for n in ("p", "v")}
    if solver == "adam":
        out["m"] = d(case["m"])
    sh = d(case["sh0"]) if shadow else None
    seg = (d(case["off"]), d(case["seg_lr"]), d(case["seg_wd"]))
    assert int(case["off"][-1]) == out["p"].numel()
    assert case["seg_lr"].numel() <= S.MAX_SEG
    g = d(case["g"])
    if solver == "sgd":
        e.sgd_update_multi(out["p"], g, out["v"], *seg, S.MU, sh)
    elif solver == "nesterov":
        e.nesterov_update_multi(out["p"], g, out["v"], *seg, S.MU, sh)
    else:
        e.adam_update_multi(out["p"], g, out["m"], out["v"], *seg,
                            S.B1, S.B2, S.EPS, sh)
    torch.cuda.synchronize()
    return out, sh


DIRECT = [(layout, shadow) for layout in S.SMALL_LAYOUTS
          for shadow in (True, False)] + [("grid_stride", True)]


@pytest.mark.parametrize("solver", S.SOLVERS)
@pytest.mark.parametrize("layout,shadow", DIRECT,
                         ids=[f"{n}-{'sh' if s else 'nosh'}"
                              for n, s in DIRECT])
def test_update_multi_kernel(layout, shadow, solver):
    case = S.make_case(layout, solver)
    out, sh = launch(case, shadow)
    check(case, out, sh, f"{solver} {layout} shadow={shadow}")


# ------------------------------------------------------- arena wrappers

def arena(table, solver):
    sizes, lrm, dm = table
    case = S.build_case(sizes, lrm, dm, solver, 4900 + len(sizes))
    off = case["off"].tolist()
    adam = solver == "adam"
    ns = types.SimpleNamespace(
        flat_w=d(case["p"]), flat_g=d(case["g"]),
        flat_m=d(case["m"] if adam else case["v"]),
        flat_m2=d(case["v"]) if adam else None,
        flat_wb=d(case["sh0"]), device=dev(),
        segments=[(off[i], sizes[i], lrm[i], dm[i])
                  for i in range(len(sizes))])
    return case, ns


def arena_update(ns, solver):
    if solver == "sgd":
        G.sgd_update_multi_arena(ns, S.RATE, S.MU, S.WD)
        return True
    if solver == "nesterov":
        return G.nesterov_update_multi_arena(ns, S.RATE, S.MU, S.WD)
    return G.adam_update_multi_arena(ns, S.RATE, S.B1, S.B2, S.EPS, S.WD,
                                     S.ADAM_T)


def arena_out(ns, solver):
    if solver == "adam":
        return {"p": ns.flat_w, "m": ns.flat_m, "v": ns.flat_m2}
    return {"p": ns.flat_w, "v": ns.flat_m}


@pytest.mark.parametrize("solver", S.SOLVERS)
def test_arena_at_table_capacity(solver):
    """512 segments fill the LDS table: the fused kernel runs, writes the
    shadow and says so."""
    ext()
    case, ns = arena(S.LAYOUTS["table_full"], solver)
    assert len(ns.segments) == S.MAX_SEG
    assert arena_update(ns, solver) is True
    torch.cuda.synchronize()
    assert ns._shadow_synced is True
    check(case, arena_out(ns, solver), ns.flat_wb, f"{solver} arena 512")


def test_sgd_arena_past_table_capacity():
    """513 segments: per-segment sgd_update on views at odd offsets, same
    bounds; the shadow is not written and not declared current."""
    ext()
    case, ns = arena(S.TABLE_OVER, "sgd")
    assert len(ns.segments) == S.MAX_SEG + 1
    arena_update(ns, "sgd")
    torch.cuda.synchronize()
    assert not getattr(ns, "_shadow_synced", False)
    assert torch.equal(ns.flat_wb.cpu(), case["sh0"])
    check(case, arena_out(ns, "sgd"), None, "sgd arena 513")


@pytest.mark.parametrize("solver", ("nesterov", "adam"))
def test_fused_arena_declines_past_table_capacity(solver):
    ext()
    case, ns = arena(S.TABLE_OVER, solver)
    assert arena_update(ns, solver) is False
    torch.cuda.synchronize()
    assert not getattr(ns, "_shadow_synced", False)
    for name, t in arena_out(ns, solver).items():
        assert torch.equal(t.cpu(), case[name]), name
    assert torch.equal(ns.flat_wb.cpu(), case["sh0"])
    assert torch.equal(ns.flat_g.cpu(), case["g"])


# ------------------------------------- single-tensor update on odd views

@pytest.mark.parametrize("n", (1, 4, 7, 9))
@pytest.mark.parametrize("start", (1, 2, 3))
def test_sgd_update_unaligned_view(start, n):
    """What the per-blob route passes: a narrow() view of the arena that
    starts 4, 8 or 12 bytes past a 16-byte boundary."""
    ext()
    total = start + n + 6
    inp = B.sgd_inputs(total, 700 + 10 * start + n)
    buf = {k: d(inp[k]) for k in "pgv"}
    ops.sgd_update(buf["p"].narrow(0, start, n), buf["g"].narrow(0, start, n),
                   buf["v"].narrow(0, start, n), *B.SGD_HYPER)
    torch.cuda.synchronize()
    inside = slice(start, start + n)
    orc = B.sgd_oracle({k: inp[k][inside] for k in "pgv"})
    B.assert_within({"p": buf["p"][inside], "v": buf["v"][inside]}, orc,
                    f"sgd view start={start} n={n}")
    outside = torch.ones(total, dtype=torch.bool)
    outside[inside] = False
    for k in "pgv":
        assert torch.equal(buf[k].cpu()[outside], inp[k][outside]), k
    assert torch.equal(buf["g"].cpu(), inp["g"])


# ------------------------------------------------------- a real Solver

NET = """
  layer { name: "d" type: "MemoryData" top: "x" top: "t"
          memory_data_param { batch_size: 4 channels: 5 height: 1
                              width: 1 } }
  layer { name: "ip1" type: "InnerProduct" bottom: "x" top: "a"
          param { lr_mult: 1 decay_mult: 1 }
          param { lr_mult: 2 decay_mult: 0 }
          inner_product_param { num_output: 3
            weight_filler { type: "gaussian" std: 0.1 } } }
  layer { name: "ip2" type: "InnerProduct" bottom: "a" top: "b"
          param { lr_mult: 1 decay_mult: 1 }
          param { lr_mult: 2 decay_mult: 0 }
          inner_product_param { num_output: 2
            weight_filler { type: "gaussian" std: 0.1 } } }
  layer { name: "ip3" type: "InnerProduct" bottom: "b" top: "c"
          param { lr_mult: 0 decay_mult: 1 }
          param { lr_mult: 0 decay_mult: 0 }
          inner_product_param { num_output: 3
            weight_filler { type: "gaussian" std: 0.1 } } }
  layer { name: "ip4" type: "InnerProduct" bottom: "c" top: "z"
          param { lr_mult: 1 decay_mult: 1 }
          param { lr_mult: 2 decay_mult: 0 }
          inner_product_param { num_output: 1
            weight_filler { type: "gaussian" std: 0.1 } } }
  layer { name: "l" type: "SoftmaxWithLoss" bottom: "z" bottom: "t"
          top: "loss" }
"""
NET_OFFSETS = [0, 15, 18, 24, 26, 32, 35, 38]       # blobs 15 3 6 2 6 3 3 1
NET_TOTAL = 39
NET_FROZEN = slice(26, 35)                          # ip3's two blobs


@pytest.mark.parametrize("stype", ("SGD", "Nesterov", "Adam"))
def test_solver_steps_per_element(stype):
    """Three apply_update calls on injected fp32 gradients, each checked
    per element against the float64 oracle started from the state the GPU
    itself held before the step."""
    from caffeonspark_amd.core.solver import Solver
    from caffeonspark_amd.proto import caffe_pb, text_format

    ext()
    sp = caffe_pb.SolverParameter(
        net_param=text_format.parse(NET, caffe_pb.NetParameter),
        base_lr=S.RATE, momentum=S.MU, momentum2=S.B2, delta=S.EPS,
        weight_decay=S.WD, lr_policy="fixed", max_iter=8, random_seed=6,
        display=0, type=stype)
    s = Solver(sp, device=dev(), dtype=torch.bfloat16)
    assert s.param_offsets == NET_OFFSETS
    assert int(s.flat_w.numel()) == NET_TOTAL
    kind = stype.lower()
    sizes = [seg[1] for seg in s.segments]
    off = S.offsets(sizes)
    assert off.tolist()[:-1] == [seg[0] for seg in s.segments]
    assert any(o % 2 for o in off.tolist())
    w0 = s.flat_w.cpu().clone()
    gen = B.gen(77)
    for step in range(3):
        grads = torch.randn(NET_TOTAL, generator=gen) * 0.1
        case = dict(solver=kind, off=off, n=NET_TOTAL, g=grads,
                    p=s.flat_w.cpu().clone(), sh0=s.flat_wb.cpu().clone())
        if kind == "adam":
            case["m"] = s.flat_m.cpu().clone()
            case["v"] = s.flat_m2.cpu().clone()
        else:
            case["v"] = s.flat_m.cpu().clone()
        s.flat_g.copy_(d(grads))
        s.apply_update()
        torch.cuda.synchronize()
        # the tensors the wrapper handed to the kernel, formed the same way
        scale = s.get_lr()
        if kind == "adam":
            scale = scale * S.adam_correction(s.iter + 1, sp.momentum,
                                              sp.momentum2)
        case["seg_lr"] = (s._seg_lrm * scale).cpu()
        case["seg_wd"] = (s._seg_dm * sp.weight_decay).cpu()
        assert S._f32(sp.momentum) == S._f32(S.MU)
        assert S._f32(sp.momentum2) == S._f32(S.B2)
        assert S._f32(sp.delta) == S._f32(S.EPS)
        out = {"p": s.flat_w, "v": s.flat_m}
        if kind == "adam":
            out = {"p": s.flat_w, "m": s.flat_m, "v": s.flat_m2}
        check(case, out, s.flat_wb, f"{stype} step {step}")
        s.iter += 1
    assert s._shadow_synced is True
    assert torch.equal(s.flat_wb, s.flat_w.to(torch.bfloat16))
    moved = s.flat_w.cpu() != w0
    assert not moved[NET_FROZEN].any()
    moved[NET_FROZEN] = True
    assert moved.all(), f"never trained: {(~moved).nonzero().reshape(-1)}"
