"""gemm_kernel's DMA-pipelined path at the shortest K it takes: pipelined_loop
peels its last tile and waits for it with vmcnt(0), so with K of two tiles
the loop body runs once and with three twice.  Whole 128x128 tiles with
8-aligned leading dimensions take that path; M = N = 128 runs the 8-wave
kernel, 384 the 4-wave one.  Checked like test_gemm_bf16_gpu.py."""

import pytest

import _gemm_bounds as GB
from test_gemm_bf16_gpu import CLASSES, _run

pytestmark = pytest.mark.gpu

TAIL_CASES = {
    "w8_k64": GB.gcase(128, 128, 64),
    "w8_k96": GB.gcase(128, 128, 96, bias=True, relu=True),
    "w4_k64": GB.gcase(384, 384, 64),
    "w4_k96": GB.gcase(384, 384, 96, bias=True),
}


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(TAIL_CASES))
def test_gemm_pipelined_tail(name, cls):
    seed = 900 + 2 * list(TAIL_CASES).index(name) + CLASSES.index(cls)
    _run(TAIL_CASES[name], cls, seed, f"{name}/{cls}")
