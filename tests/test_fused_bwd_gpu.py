"""The fused backward kernels on the GPU against the bounds of
_fused_bwd_cases.py (shown sound on the CPU by test_fused_bwd_bounds.py):
relu_db_dense and maxpool_bwd8_relu_db with 1, 2 and 3 forced blocks (the
grid-stride loop, its tail and the multi-block reduction on tiny data), the
shapes that must decline the fused pool route, and a tiny net that takes
the fused routes by default and the separate kernels with COS_RELU_DB=0."""

import pytest
import torch

import _bf16_bounds as B
import _fused_bwd_cases as F

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops
from caffeonspark_amd.ops import gpu as G


def dev():
    return torch.device("cuda:0")


def d(t):
    return t.to(dev())


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------- ReLU + db

@pytest.mark.parametrize("blocks", F.FORCED_BLOCKS)
@pytest.mark.parametrize("slope", F.RELU_DB_SLOPES)
@pytest.mark.parametrize("shape", F.RELU_DB_SHAPES,
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_relu_db_dense(shape, slope, blocks):
    inp = F.relu_db_inputs(*shape, 900 + shape[0])
    orc = F.relu_db_oracle(inp, slope)
    db = d(inp["db0"]).clone()
    dx, done = ops.relu_backward(d(inp["y"]), d(inp["dy"]), slope,
                                 db_out=db, db_blocks=blocks)
    assert done is True
    B.assert_within({"dx": dx, "db": db}, orc,
                    f"relu+db {shape} slope={slope} blocks={blocks}")


_big = {}


@pytest.mark.parametrize("blocks", [0, 3])
def test_relu_db_dense_big_activation(blocks):
    """2^22 elements and more run 1024-thread blocks (85 row groups of 12
    octets at C = 96): launcher-sized grid and a forced 3-block one."""
    rows, c = 43701, 96
    assert rows * c >= 1 << 22
    if not _big:
        inp = F.relu_db_inputs(rows, c, 990)
        _big.update(inp=inp, orc=F.relu_db_oracle(inp, 0.0),
                    y=d(inp["y"]), dy=d(inp["dy"]))
    db = d(_big["inp"]["db0"]).clone()
    dx, done = ops.relu_backward(_big["y"], _big["dy"], 0.0, db_out=db,
                                 db_blocks=blocks)
    assert done is True
    B.assert_within({"dx": dx, "db": db}, _big["orc"],
                    f"relu+db {rows}x{c} blocks={blocks}")


def test_relu_db_dense_channels_last_auto_grid():
    """4-D dense channels-last input through the same route, launcher-
    sized grid."""
    g = B.gen(930)
    cl = torch.channels_last
    y = B.bf16(torch.randn(3, 24, 7, 5, generator=g)).contiguous(
        memory_format=cl)
    dy = B.bf16(torch.randn(3, 24, 7, 5, generator=g)).contiguous(
        memory_format=cl)
    db0 = torch.randn(24, generator=g) * 3 + 1
    db = d(db0).clone()
    dx, done = ops.relu_backward(d(y), d(dy), 0.0, db_out=db)
    assert done is True
    B.assert_within({"dx": dx, "db": db},
                    B.relu_fused_oracle(y, dy, db0, 0.0), "relu+db 4-D")


# ------------------------------------------------------ pool + ReLU + db

_pool_ref = {}


def _pool_case(case):
    """Inputs, oracle and the unfused pair's dx, computed once per case."""
    if case not in _pool_ref:
        c, geom = case
        inp = F.pool_relu_inputs(c, geom, 940 + c)
        x = cl(d(inp["x"]))
        y, pack = ops.maxpool_forward(x, inp["kernel"], inp["stride"],
                                      inp["pad"])
        plain = ops.maxpool_backward(list(x.shape), pack, d(inp["dy"]))
        pair = ops.relu_backward(x, plain, 0.0)
        _pool_ref[case] = (inp, F.pool_relu_oracle(inp), pack, pair.cpu())
    return _pool_ref[case]


@pytest.mark.parametrize("blocks", F.FORCED_BLOCKS)
@pytest.mark.parametrize("case", F.POOL_CASES, ids=F.case_id)
def test_maxpool_bwd_relu_db(case, blocks):
    inp, orc, pack, pair = _pool_case(case)
    db = d(inp["db0"]).clone()
    dx = G.maxpool_backward_relu_db(pack, d(inp["dy"]), db, blocks=blocks)
    assert dx is not None, "fused route declined a supported shape"
    what = f"pool+relu+db {F.case_id(case)} blocks={blocks}"
    assert torch.equal(dx.cpu(), pair), what + ": dx != unfused pair"
    B.assert_within({"dx": dx, "db": db}, orc, what)
    unc = F.uncovered(inp)
    if unc.any():
        assert not dx.cpu()[:, :, unc].any()


@pytest.mark.parametrize("case", F.POOL_DECLINE_CASES, ids=F.case_id)
def test_maxpool_bwd_relu_db_declines(case):
    c, geom = case
    inp = F.pool_relu_inputs(c, geom, 980 + c)
    x = cl(d(inp["x"]))
    y, pack = ops.maxpool_forward(x, inp["kernel"], inp["stride"],
                                  inp["pad"])
    db = d(inp["db0"]).clone()
    assert G.maxpool_backward_relu_db(pack, d(inp["dy"]), db) is None
    assert torch.equal(db.cpu(), inp["db0"])        # nothing written
    # the separate kernels still give the right answer for this shape
    plain = ops.maxpool_backward(list(x.shape), pack, d(inp["dy"]))
    dx, done = ops.relu_backward(x, plain, 0.0, db_out=db)
    orc = F.pool_relu_oracle(inp)
    out = {"dx": dx}
    if done:
        out["db"] = db
    B.assert_within(out, orc, f"declined {F.case_id(case)}")


# --------------------------------------------------------------- net level

NET_TEXT = """
  layer { name: "d" type: "MemoryData" top: "x" top: "t"
          memory_data_param { batch_size: 8 channels: 8 height: 13
                              width: 13 } }
  layer { name: "c1" type: "Convolution" bottom: "x" top: "c1"
          convolution_param { num_output: 8 kernel_size: 3 pad: 1
            weight_filler { type: "gaussian" std: 0.2 } } }
  layer { name: "r1" type: "ReLU" bottom: "c1" top: "c1" }
  layer { name: "p1" type: "Pooling" bottom: "c1" top: "p1"
          pooling_param { pool: MAX kernel_size: 3 stride: 2 } }
  layer { name: "c2" type: "Convolution" bottom: "p1" top: "c2"
          convolution_param { num_output: 16 kernel_size: 3 pad: 1
            weight_filler { type: "gaussian" std: 0.2 } } }
  layer { name: "r2" type: "ReLU" bottom: "c2" top: "c2" }
  %s
  layer { name: "ip" type: "InnerProduct" bottom: "c2" top: "z"
          inner_product_param { num_output: 5
            weight_filler { type: "gaussian" std: 0.1 } } }
  layer { name: "l" type: "SoftmaxWithLoss" bottom: "z" bottom: "t"
          top: "loss" }
"""
# a second reader of the rectified conv1 blob
SECOND_CONSUMER = """
  layer { name: "p1b" type: "Pooling" bottom: "c1" top: "p1b"
          pooling_param { pool: AVE kernel_size: 3 stride: 2 } }
  layer { name: "sil" type: "Silence" bottom: "p1b" }
"""


def _one_step(monkeypatch, relu_db, extra=""):
    """One solver step from a fixed seed; returns (gradients, weights,
    routes of the pool and the two ReLU layers)."""
    from caffeonspark_amd.core.solver import Solver
    from caffeonspark_amd.proto import caffe_pb, text_format
    if relu_db is None:
        monkeypatch.delenv("COS_RELU_DB", raising=False)
    else:
        monkeypatch.setenv("COS_RELU_DB", relu_db)
    sp = caffe_pb.SolverParameter(
        net_param=text_format.parse(NET_TEXT % extra,
                                    caffe_pb.NetParameter),
        base_lr=0.1, momentum=0.9, lr_policy="fixed", max_iter=4,
        random_seed=3, display=0)
    s = Solver(sp, device=dev(), dtype=torch.bfloat16)
    g = B.gen(77)
    x = B.bf16(torch.randn(8, 8, 13, 13, generator=g))
    t = torch.randint(0, 5, (8,), generator=g).float()
    s.net.data_layers()[0].reset(d(x), d(t))
    s._step_one()
    routes = {n: getattr(s.net.layer_by_name(n), "_route", None)
              for n in ("p1", "r1", "r2")}
    # per-channel sum|dy| into each conv (what its bias gradient sums)
    # and the row count, for the oracle bound on a regrouped fp32 sum
    sums = []
    for n in ("c1", "c2"):
        dy = s.net.blob_by_name(n).diff.double()
        sums.append((dy.numel() // dy.shape[1],
                     dy.abs().sum(dim=(0, 2, 3)).max().item()))
    return s.flat_g.cpu().clone(), s.flat_w.cpu().clone(), routes, sums


def test_net_step_fused_matches_unfused(monkeypatch):
    g_a, w_a, r_a, sums = _one_step(monkeypatch, "0")
    g_b, w_b, r_b, _ = _one_step(monkeypatch, "0")
    g_f, w_f, r_f, _ = _one_step(monkeypatch, None)     # default: fused
    assert r_a == r_b == {"p1": "plain", "r1": "plain", "r2": "plain"}
    assert r_f == {"p1": "relu_db", "r1": "mask_done", "r2": "relu_db"}
    # Oracle bound for a deterministic unfused build: the fused dx is
    # bit-identical, so only the two conv bias gradients can differ, each
    # an fp32 sum of the same m terms in another grouping.  B3 on both
    # sides: 2(m+2)e*sum|dy|.  The weights move by lr * gradient (lr 0.1,
    # first step) and round once in fp32.
    tol_g = max(2 * (m + 2) * B.E32 * t for m, t in sums)
    tol_w = tol_g + 2 * B.E32 * w_a.abs().max().item()
    for name, a, b, f, tol in (("grad", g_a, g_b, g_f, tol_g),
                               ("weight", w_a, w_b, w_f, tol_w)):
        noise = (a - b).abs().max().item()
        diff = (f - a).abs().max().item()
        print(f"{name}: unfused run-to-run {noise:.3e}, fused vs unfused "
              f"{diff:.3e}, oracle bound {tol:.3e}")
        if noise > 0:
            assert diff <= 4 * noise, name
        else:
            assert diff <= tol, f"{name}: {diff} > {tol}"


def test_net_second_consumer_disables_pool_fusion(monkeypatch):
    _, _, routes, _ = _one_step(monkeypatch, None, SECOND_CONSUMER)
    assert routes["p1"] == "plain"
    assert routes["r1"] == "relu_db"    # ReLU' + db still fuses for conv1
    assert routes["r2"] == "relu_db"
