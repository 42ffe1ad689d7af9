"""gemm_kernel (all four ta/tb combinations, store modes 0-3, 4- and 8-wave)
and gemm_wide_tt_kernel<., BGuarded> through _ext.gemm, against the float64
oracles of _gemm_bounds.py: bit-exact on the exact input class, inside the
derived bound on the rounded one.  Every operand sits in a NaN-poisoned
buffer and C in a sentinel buffer (see _gemm_bounds.gemm_layout), so a read
outside the operands, an unwritten output or a write outside the view
shows.  Kernel variants are chosen by shape: the COS_GEMM_W8 override is
cached at first use, so the tests never set it.

k_begin % 8 != 0 in gemm_kernel's fast-path test cannot be reached through
the host: split_k() makes every split a multiple of 32."""

import pytest
import torch

import _gemm_bounds as GB

pytestmark = pytest.mark.gpu

from caffeonspark_amd import ops

CLASSES = ("exact", "rounded")
TABLE = dict(GB.GEMM_CASES, **GB.WIDE_CASES)


def dev():
    return torch.device("cuda:0")


def _run(c, cls, seed, what):
    inp = GB.gemm_inputs(c, cls, seed)
    orc, peak = GB.gemm_oracle(c, inp)
    if cls == "exact":
        assert peak <= 256, "exact-class precondition"
    lay = GB.gemm_layout(c, inp)
    A, B, C = (lay[k].to(dev()) for k in ("A", "B", "C"))
    bias = None
    db_flat = None
    if GB.is_wide(c):
        if inp["db0"] is not None:
            # the wide branch's bias slot is the fused db output
            db_flat, _, _ = GB.out_buf(1, c["M"], torch.float32,
                                       inp["db0"].view(1, -1), ld_x=0)
            db_flat = db_flat.to(dev())
            bias = db_flat[GB.PADEL:]
    elif inp["bias"] is not None:
        bias = inp["bias"].to(dev())
    ops.native().gemm(A[GB.PADEL:], B[GB.PADEL:], C[GB.PADEL:], bias,
                      c["M"], c["N"], c["K"], lay["lda"], lay["ldb"],
                      lay["ldc"], c["ta"], c["tb"], c["store"], c["splitk"],
                      c["relu"], inp["alpha"], c["m_alloc"], c["n_alloc"])
    torch.cuda.synchronize()
    Cc = C.cpu()
    M, N, ldc = c["M"], c["N"], lay["ldc"]
    out = {"C": Cc[GB.PADEL:GB.PADEL + M * ldc].view(M, ldc)[:, :N]}
    assert GB.outside_untouched(Cc, M, N, ldc), \
        "wrote outside the C view"
    if db_flat is not None:
        dbc = db_flat.cpu()
        out["db"] = dbc[GB.PADEL:GB.PADEL + M]
        assert GB.outside_untouched(dbc, 1, M, M), "wrote outside db"
    GB.within(out, orc, what)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("name", list(TABLE))
def test_gemm(name, cls):
    seed = 100 + 2 * list(TABLE).index(name) + CLASSES.index(cls)
    _run(TABLE[name], cls, seed, f"{name}/{cls}")


@pytest.mark.parametrize("name", list(GB.RAISES_CASES))
def test_split_k_refuses_fused_bias_and_relu(name):
    """Every split-K block runs the fp32 epilogue, so a bias would be added
    once per split and the ReLU applied to partial sums: the host throws
    before any launch and C is untouched."""
    c = GB.RAISES_CASES[name]
    inp = GB.gemm_inputs(c, "exact", 7)
    lay = GB.gemm_layout(c, inp)
    A, B, C = (lay[k].to(dev()) for k in ("A", "B", "C"))
    before = C.clone()
    bias = inp["bias"].to(dev()) if inp["bias"] is not None else None
    with pytest.raises(RuntimeError, match="split-K"):
        ops.native().gemm(A[GB.PADEL:], B[GB.PADEL:], C[GB.PADEL:], bias,
                          c["M"], c["N"], c["K"], lay["lda"], lay["ldb"],
                          lay["ldc"], c["ta"], c["tb"], c["store"],
                          c["splitk"], c["relu"], inp["alpha"],
                          c["m_alloc"], c["n_alloc"])
    torch.cuda.synchronize()
    assert torch.equal(C, before)


def test_split_k_refuses_plain_store():
    c = GB.gcase(130, 70, 1030, store=1, splitk=3)
    inp = GB.gemm_inputs(c, "exact", 7)
    lay = GB.gemm_layout(c, inp)
    A, B, C = (lay[k].to(dev()) for k in ("A", "B", "C"))
    with pytest.raises(RuntimeError, match="split-K"):
        ops.native().gemm(A[GB.PADEL:], B[GB.PADEL:], C[GB.PADEL:], None,
                          c["M"], c["N"], c["K"], lay["lda"], lay["ldb"],
                          lay["ldc"], False, False, 1, 3, False, 1.0,
                          c["m_alloc"], c["n_alloc"])
