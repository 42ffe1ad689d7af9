"""Case tables, input builders, float64 oracles with derived bounds, CPU
emulations and mutants for the bf16 GEMM kernels of gemm.hip (gemm_kernel,
gemm_wide_tt_kernel, the implicit / small-C / space-to-depth convolution
routes) and the column and glue kernels around them (im2col, col2im,
im2col_t, transpose, colsum, bias_act_cast) and for the Winograd pipeline of
winograd.hip (its section below).  Shared by test_gemm_bounds.py
(CPU) and test_gemm_bf16_gpu.py, test_conv_gemm_gpu.py,
test_col_kernels_gpu.py (GPU).  Same conventions as _bf16_bounds.py: every
oracle takes the tensors the kernel gets, computes in float64 and returns
{output name: (want, tol)}, tol None meaning bit-exact; no bound is derived
from what a kernel returned.

Two input classes are run through every GEMM-shaped case.

 exact    A-side values are integers in {-1, 0, 1}, B-side values integers in
          {-3 .. 3}, bias and prior output content small integers, alpha 1
          or -2.  Every product and partial sum is an integer below 2^24, so
          the fp32 accumulation is exact in any order (split-K atomics
          included) and the output must be BIT-exact: the float64 sum as
          fp32, or bf16(sum).  Precondition, asserted on the oracle:
          max|result| <= 256 for every bf16 value on the way, so each is a
          bf16 integer and any wrong, missing or doubled non-zero term
          changes the output.
 rounded  randn plus an offset, rounded to bf16.  bf16 x bf16 products are
          exact in fp32 (8 + 8 significand bits); the roundings are the fp32
          accumulation, alpha, bias, the atomic adds and the final bf16
          store.  With T = |alpha| (|A| |B|^T) + |bias| + |C0| in float64,
          rule B3 of _bf16_bounds.py gives for an fp32 output
              tol_acc = (K + splits + 4) e T
          and for a bf16 output (rule B1 on top)
              tol = tol_acc + u (|want| + tol_acc).
          ReLU is 1-Lipschitz, so both survive it.

Layouts are poisoned (gemm_layout): operands sit inside NaN-filled buffers,
the gap between rows is NaN where ld exceeds the row, rows M..m_alloc-1 are
NaN (they exist: every buffer is as large as the m_alloc / n_alloc passed),
and C is a view with ldc > N of a buffer whose every other element holds a
sentinel that must survive.  Plain-store modes start from a NaN C, modes 2
and 3 from a known non-zero C0 the oracle includes.

Convolution bounds (K the reduction length of the GEMM that produces the
output, T the same convolution on absolute values):
 y            bf16-output form, K = R S Cg (padding adds exact zeros)
 dx implicit  one GEMM: bf16-output form, K = R S Kg (+ |dx0| when the
              epilogue accumulates onto dx0)
 dx 1x1       one GEMM: bf16-output form, K = Kout
 dx fallback  bf16 dcol, col2im sums <= R S of them in fp32, bf16 store:
              (2u + (Kg + R S + 8) e) T + I T
 dw           (NPQ + splits + 4) e T
 db           (2 NPQ + 4) e sum|dy|
Column kernels: im2col, im2col_t and transpose are copies (bit-exact);
col2im (u + (R S + 2) e) sum|taps|; colsum (2 rows + 4) e (|out0| + sum|x|);
bias_act_cast (u + 4 e)(|in| + |bias|).
"""

import torch
import torch.nn.functional as F

from _bf16_bounds import (U, E32, INTR, BF, gen, bf16, rb,  # noqa: F401
                          violations, report, assert_within)

NAN = float("nan")
SENT = -7.5         # sentinel around every output view
PADEL = 64          # poison elements on either side of every buffer
BK = 32


def f32(v):
    """The float32 value a Python float becomes when handed to a kernel."""
    return float(torch.tensor(v, dtype=torch.float32))


def trunc_bf16(t):
    """fp32 -> bf16 by truncation (the mutant of round-to-nearest)."""
    bits = t.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(BF)


def split_k(k, splitk):
    """(ksplit, zblocks) of split_k() in gemm.hip."""
    ks = -(-k // max(1, splitk))
    ks = -(-ks // BK) * BK
    return ks, -(-k // ks)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _rnd(shape, g, off, scale=1.0):
    return rb(torch.randn(shape, generator=g) * scale + off)


def within(out, orc, what):
    """assert_within plus: no NaN / inf reached a bit-exact output."""
    for name, got in out.items():
        assert torch.isfinite(got.float()).all(), \
            f"{what} {name}: NaN/inf reached the output"
    assert_within(out, orc, what)


# ===================================================================== GEMM

def gcase(M, N, K, ta=False, tb=False, store=0, splitk=1, bias=False,
          relu=False, alpha=1.0, lda_x=0, ldb_x=0, m_alloc=0, n_alloc=0,
          db=False):
    return dict(M=M, N=N, K=K, ta=ta, tb=tb, store=store, splitk=splitk,
                bias=bias, relu=relu, alpha=alpha, lda_x=lda_x, ldb_x=ldb_x,
                m_alloc=max(m_alloc, M), n_alloc=max(n_alloc, N), db=db)


def is_wide(c):
    """The gemm_wide_tt_kernel branch of gemm_bf16_batched."""
    return c["ta"] and c["tb"] and c["store"] >= 1 and c["N"] > 128


# gemm_kernel: 8 waves when M <= 256 or N <= 256 (NN only), else 4 waves;
# every transposed combination runs the 4-wave kernel
GEMM_CASES = {
    # single tile, everything guarded
    "nn_1x1x1": gcase(1, 1, 1),
    "nn_33x17x5": gcase(33, 17, 5),
    # pipelined fast path, exactly 2 and 3 K tiles (8-wave)
    "nn_fast_k64": gcase(128, 128, 64),
    "nn_fast_k96": gcase(128, 128, 96),
    # 4-wave: 3x3 tiles, 1-row / 1-column edge tiles staged from alloc rows
    "nn_w4_fast_k64": gcase(257, 257, 64, m_alloc=384, n_alloc=384),
    "nn_w4_guarded_k41": gcase(257, 257, 41),
    # K = 32 exactly: fast staging in the non-pipelined loop
    "nn_fast_k32": gcase(128, 128, 32),
    # K tails: K % 32 != 0 sends the whole split down the guarded path
    "nn_tail_130x70x41": gcase(130, 70, 41),
    "nn_tail_128x128x72": gcase(128, 128, 72),
    # A fast / B guarded and the reverse
    "nn_afast_bguard": gcase(128, 70, 64),
    "nn_aguard_bfast": gcase(70, 128, 64),
    # m_alloc > M: junk (NaN) rows staged by the DMA, outputs masked
    "nn_malloc_256": gcase(130, 128, 64, m_alloc=256),
    "nn_nalloc_256": gcase(128, 130, 96, n_alloc=256),
    # lda % 8 != 0 / ldb % 8 != 0: scalar guarded fill, NaN gap
    "nn_ld_odd": gcase(130, 70, 41, lda_x=3, ldb_x=3),
    "nn_ld_odd_k64": gcase(128, 128, 64, lda_x=3, ldb_x=5),
    # transposed staging, vector path (ld % 8 == 0, rows % 8 == 0)
    "tn_vec": gcase(136, 72, 41, ta=True),
    "nt_vec": gcase(136, 72, 41, tb=True),
    "tt_vec": gcase(136, 72, 41, ta=True, tb=True),
    "tt_vec_store1": gcase(136, 72, 70, ta=True, tb=True, store=1),
    # transposed staging, scalar path (ld = rows + 3, rows % 8 != 0)
    "tn_scalar": gcase(130, 70, 41, ta=True, lda_x=3),
    "nt_scalar": gcase(130, 70, 41, tb=True, ldb_x=3),
    "tt_scalar": gcase(130, 70, 41, ta=True, tb=True, lda_x=3, ldb_x=3),
    # A fast, B transposed
    "nt_afast": gcase(128, 72, 64, tb=True),
    # store modes
    "nn_store1": gcase(130, 70, 41, store=1),
    "nn_store2_c0": gcase(130, 70, 41, store=2),
    "nn_store3_c0": gcase(130, 70, 41, store=3),
    "nn_store3_fast": gcase(128, 128, 64, store=3),
    # bias, ReLU, alpha
    "nn_bias_relu_alpha": gcase(200, 130, 96, bias=True, relu=True,
                                alpha=-0.37),
    "nn_bias_alpha_store1": gcase(200, 130, 96, store=1, bias=True,
                                  alpha=-0.37),
    "nn_bias_relu_store1": gcase(200, 130, 96, store=1, bias=True,
                                 relu=True),
    "nn_bias_store3": gcase(130, 70, 41, store=3, bias=True, relu=True,
                            alpha=-0.37),
    "tn_bias_relu": gcase(130, 70, 41, ta=True, bias=True, relu=True,
                          lda_x=3),
    # split-K, store 2: last split shorter (352/352/326), single-tile
    # splits (33 of them, 6 elements in the last), tail in the last split
    "nn_split3_k1030": gcase(130, 70, 1030, store=2, splitk=3),
    "nn_split33_k1030": gcase(130, 70, 1030, store=2, splitk=33),
    # fast splits: 352/352/320 pipelined; 32 fast single tiles + a tail
    "nn_split3_fast_k1024": gcase(128, 128, 1024, store=2, splitk=3),
    "nn_split33_fast_k1030": gcase(128, 128, 1030, store=2, splitk=33),
    "nn_split3_alpha": gcase(130, 70, 200, store=2, splitk=3, alpha=-0.37),
    "tt_split3_narrow": gcase(96, 72, 98, ta=True, tb=True, store=2,
                              splitk=3),
}

# gemm_wide_tt_kernel<., BGuarded>: ta and tb, store >= 1, N > 128.  N = 160
# is one 256-block with 96 dead columns, 288 two n-blocks; M = 96 one partial
# m-tile, 192 a second half valid; K = 98 four tiles with a 2-row tail, two
# splits of 64 / 34 (splitk 3) or four single-tile splits (splitk 4).
WIDE_CASES = {
    "wide_96x160": gcase(96, 160, 98, ta=True, tb=True, store=1),
    "wide_192x288_db": gcase(192, 288, 98, ta=True, tb=True, store=1,
                             db=True),
    "wide_96x160_split3_db": gcase(96, 160, 98, ta=True, tb=True, store=2,
                                   splitk=3, db=True),
    "wide_192x288_split4_db": gcase(192, 288, 98, ta=True, tb=True, store=2,
                                    splitk=4, db=True),
    "wide_store2_single": gcase(96, 160, 98, ta=True, tb=True, store=2),
    "wide_alpha": gcase(96, 160, 98, ta=True, tb=True, store=1,
                        alpha=-0.37),
    "wide_alpha_split3": gcase(192, 288, 98, ta=True, tb=True, store=2,
                               splitk=3, alpha=-0.37, db=True),
    # M % 8 != 0 and lda % 8 != 0: the scalar trans path on both operands
    "wide_scalar": gcase(100, 163, 98, ta=True, tb=True, store=1, lda_x=3,
                         ldb_x=2, db=True),
    "wide_scalar_split3": gcase(100, 163, 98, ta=True, tb=True, store=2,
                                splitk=3, lda_x=3, ldb_x=2, db=True),
}

# split-K with a fused bias or ReLU on the non-wide branch: every split
# would run the epilogue, so the host refuses.  The CPU file still runs the
# bias case through the oracle to show what a per-split bias would cost.
RAISES_CASES = {
    "split3_bias": gcase(130, 70, 1030, store=2, splitk=3, bias=True),
    "split3_relu": gcase(130, 70, 1030, store=2, splitk=3, relu=True),
    "split3_bias_tn": gcase(130, 70, 1030, ta=True, store=2, splitk=3,
                            bias=True),
}


def gemm_alpha(c, cls):
    if c["alpha"] == 1.0:
        return 1.0
    return -2.0 if cls == "exact" else f32(c["alpha"])


def gemm_inputs(c, cls, seed):
    """Logical operands: A [M, K], B [N, K], bias [N], C0 [M, N], db0 [M]."""
    g = gen(seed)
    M, N, K = c["M"], c["N"], c["K"]
    if cls == "exact":
        A, B = _ints((M, K), -1, 1, g), _ints((N, K), -3, 3, g)
        bias, C0, db0 = (_ints((N,), -4, 4, g), _ints((M, N), -8, 8, g),
                         _ints((M,), -8, 8, g))
    else:
        A, B = _rnd((M, K), g, 0.25), _rnd((N, K), g, -0.125, 0.5)
        bias = torch.randn(N, generator=g) * 2 + 0.5
        C0 = torch.randn(M, N, generator=g) * 3 + 1
        db0 = torch.randn(M, generator=g) * 3 + 1
    if c["store"] == 3:
        C0 = rb(C0)
    return dict(A=A, B=B, bias=bias if c["bias"] else None,
                C0=C0 if c["store"] >= 2 else None,
                db0=db0 if c["db"] else None, alpha=gemm_alpha(c, cls),
                cls=cls)


def _operand_buf(mat, trans, alloc_rows, ld_x):
    """[rows][K] logical `mat` in the kernel's global layout inside a NaN
    buffer: ([K][rows] when trans).  Returns (flat buffer, ld)."""
    rows, k = mat.shape
    src = mat.t() if trans else mat
    nrows = k if trans else alloc_rows
    ld = src.shape[1] + ld_x
    flat = torch.full((PADEL + nrows * ld + PADEL,), NAN, dtype=BF)
    view = flat[PADEL:PADEL + nrows * ld].view(nrows, ld)
    view[:src.shape[0], :src.shape[1]] = src.to(BF)
    return flat, ld


def out_buf(rows, cols, dtype, fill, ld_x=3):
    """A [rows, cols] view with ld = cols + ld_x inside a sentinel buffer.
    Returns (flat buffer, view, ld)."""
    ld = cols + ld_x
    flat = torch.full((PADEL + rows * ld + PADEL,), SENT, dtype=dtype)
    view = flat[PADEL:PADEL + rows * ld].view(rows, ld)[:, :cols]
    if isinstance(fill, torch.Tensor):
        view.copy_(fill)
    else:
        view.fill_(fill)
    return flat, view, ld


def outside_untouched(flat, rows, cols, ld):
    """Every element of an out_buf buffer outside the view still holds the
    sentinel."""
    f = flat.detach().cpu().float().clone()
    f[PADEL:PADEL + rows * ld].view(rows, ld)[:, :cols] = SENT
    return bool((f == SENT).all())


def gemm_layout(c, inp):
    A_flat, lda = _operand_buf(inp["A"], c["ta"], c["m_alloc"], c["lda_x"])
    B_flat, ldb = _operand_buf(inp["B"], c["tb"], c["n_alloc"], c["ldb_x"])
    cdt = BF if c["store"] in (0, 3) else torch.float32
    fill = inp["C0"] if c["store"] >= 2 else NAN
    C_flat, _, ldc = out_buf(c["M"], c["N"], cdt, fill)
    return dict(A=A_flat, B=B_flat, C=C_flat, lda=lda, ldb=ldb, ldc=ldc)


def layout_operands(c, lay):
    """Logical A [M, K] and B [N, K] read back through the leading
    dimensions, as the kernel addresses them."""
    def read(flat, ld, trans, rows, alloc):
        nrows = c["K"] if trans else alloc
        v = flat[PADEL:PADEL + nrows * ld].view(nrows, ld)
        return v[:c["K"], :rows].t() if trans else v[:rows, :c["K"]]
    return (read(lay["A"], lay["lda"], c["ta"], c["M"], c["m_alloc"]),
            read(lay["B"], lay["ldb"], c["tb"], c["N"], c["n_alloc"]))


def gemm_oracle(c, inp):
    """relu(alpha A B^T + bias) + C0, and db0 + colsum for the fused db."""
    A, B = inp["A"].double(), inp["B"].double()
    K, alpha = c["K"], inp["alpha"]
    _, splits = split_k(K, c["splitk"])
    s = alpha * (A @ B.t())
    t = abs(alpha) * (A.abs() @ B.abs().t())
    stages = [s]
    if inp["bias"] is not None:
        s = s + inp["bias"].double()
        t = t + inp["bias"].double().abs()
        stages.append(s)
    if c["relu"]:
        s = s.clamp_min(0)
    if inp["C0"] is not None:
        s = s + inp["C0"].double()
        t = t + inp["C0"].double().abs()
        stages.append(s)
    out_bf16 = c["store"] in (0, 3)
    peak = max(v.abs().max().item() for v in stages)
    if inp["cls"] == "exact":
        orc = {"C": (s.to(BF) if out_bf16 else s.float(), None)}
    else:
        tol = (K + splits + 4) * E32 * t
        if out_bf16:
            tol = tol + U * (s.abs() + tol)
        orc = {"C": (s, tol)}
    if inp["db0"] is not None:
        db0 = inp["db0"].double()
        db = db0 + A.sum(dim=1)
        if inp["cls"] == "exact":
            orc["db"] = (db.float(), None)
        else:
            orc["db"] = (db, (K + splits + 2) * E32
                         * (db0.abs() + A.abs().sum(dim=1)))
        peak = max(peak, db.abs().max().item())
    return orc, peak


def gemm_emulate(c, inp, A=None, B=None, mutant=None):
    """fp32 arithmetic with the kernel's rounding points: one fp32 partial
    per split, alpha / bias / ReLU in the epilogue, partials summed in fp32
    onto C0, bf16 where the kernel stores bf16."""
    A = (inp["A"] if A is None else A).float()
    B = (inp["B"] if B is None else B).float()
    M, N, K = c["M"], c["N"], c["K"]
    alpha = torch.tensor(inp["alpha"], dtype=torch.float32)
    ksplit, splits = split_k(K, c["splitk"])
    wide = is_wide(c)
    out_bf16 = c["store"] in (0, 3)
    acc = torch.zeros(M, N)
    if inp["C0"] is not None and mutant != "c0_dropped":
        acc = inp["C0"].float().clone()
    db = inp["db0"].float().clone() if inp["db0"] is not None else None
    nblocks = -(-N // 256)
    for sp in range(splits):
        ks, ke = sp * ksplit, min(K, (sp + 1) * ksplit)
        if ke == K and mutant == "drop_last_k":
            ke = K - 1
        if ke == K and mutant == "drop_tail_tile":
            ke = K - (K % BK or BK)
        part = A[:, ks:ke] @ B[:, ks:ke].t() if ke > ks else \
            torch.zeros(M, N)
        bias = None
        if inp["bias"] is not None and not wide and \
                (sp == 0 or mutant == "bias_per_split"):
            bias = inp["bias"].float()
        if mutant == "alpha_after_bias" and bias is not None:
            v = (part + bias) * alpha
        elif mutant == "relu_before_bias" and c["relu"]:
            v = (part * alpha).clamp_min(0)
            if bias is not None:
                v = v + bias
        else:
            v = part * alpha
            if bias is not None:
                v = v + bias
        if c["relu"] and not wide and mutant != "relu_before_bias":
            v = v.clamp_min(0)
        acc = acc + v
        if db is not None:
            reps = nblocks if mutant == "db_per_nblock" else 1
            for _ in range(reps):
                db = db + A[:, ks:ke].sum(dim=1)
    if out_bf16:
        out = {"C": trunc_bf16(acc) if mutant == "truncate" else bf16(acc)}
    else:
        out = {"C": acc}
    if db is not None:
        out["db"] = db
    return out


GEMM_MUTANTS = ["drop_last_k", "drop_tail_tile", "bias_per_split",
                "relu_before_bias", "truncate", "alpha_after_bias",
                "c0_dropped"]
WIDE_MUTANTS = ["drop_last_k", "drop_tail_tile", "c0_dropped",
                "db_per_nblock"]


# ============================================================== convolution

def ccase(n, c, h, w, k, r, s=None, stride=1, pad=0, dil=1, groups=1,
          bias=True, relu=False, route="implicit", dx="implicit",
          dx_acc=False, density=1.0):
    return dict(n=n, c=c, h=h, w=w, k=k, r=r, s=r if s is None else s,
                stride=stride, pad=pad, dil=dil, groups=groups, bias=bias,
                relu=relu, route=route, dx=dx, dx_acc=dx_acc,
                density=density)


# route: the ctx flag that must be set (implicit, implicit_sc, s2d, is_1x1,
# or "col" for the materialised-col fallback).  dx: which data-gradient
# sequence the shape takes (implicit: one GEMM over the flipped weights;
# 1x1: one GEMM; col2im: dcol GEMM + col2im).  The gates are those of
# conv2d_forward: implicit needs C % 8 == Cg % 8 == 0 and not 1x1; its
# kernel is <8,4> when (NPQ <= 256 or Kg <= 256) and 128 <= Kpad <= 1152,
# <8,2> when 8-wave otherwise, <4,2> when NPQ >= 257 and Kg >= 257;
# Kpad = max(64, pad32(R S Cg)).  Implicit dx needs stride 1, Kg % 8 == 0
# and pad <= dil (R - 1).
CONV_CASES = {
    # <8,2>: Kpad 64 (2x3 taps of 8 channels + a zero tile) and 96
    "imp82_k64": ccase(2, 8, 8, 9, 16, 2, 3),
    "imp82_k96_npq98": ccase(2, 8, 9, 9, 16, 3),
    "imp82_k96_npq288": ccase(2, 8, 12, 12, 16, 3, pad=1, relu=True),
    "imp82_k96_dil2": ccase(2, 8, 11, 11, 16, 3, dil=2, pad=2),
    # <8,4>: Kpad 128 (lower edge), 288, 1152 (upper edge); 1248 is <8,2>
    "imp84_k128": ccase(2, 8, 10, 10, 16, 4),
    "imp84_k288": ccase(2, 32, 9, 9, 24, 3, pad=1, relu=True),
    "imp84_k1152": ccase(1, 128, 7, 7, 16, 3, pad=1),
    "imp82_k1248": ccase(1, 136, 7, 7, 16, 3, pad=1),
    # <4,2>: NPQ 288, Kg 264 (ragged N: 8 live rows in the third n-tile)
    "imp42_k264": ccase(2, 8, 12, 12, 264, 3, pad=1, density=0.25),
    # ragged N = 24: the edge tile reads wrb's zero pad rows
    "imp_n24": ccase(2, 16, 7, 7, 24, 3, pad=1),
    # groups: wrb group slice, y2[:, g*Kg:] written with ldc = Kout
    "imp_g2": ccase(2, 32, 8, 8, 48, 3, pad=1, groups=2),
    "imp_g4": ccase(2, 32, 8, 8, 32, 3, pad=1, groups=4, relu=True),
    # geometry
    "imp_stride2": ccase(2, 16, 13, 13, 16, 3, stride=2, pad=1,
                         dx="col2im"),
    "imp_fullpad": ccase(2, 8, 7, 6, 16, 3, pad=2),
    "imp_nonsquare_7x5": ccase(2, 8, 9, 7, 16, 3),
    # implicit dx with fan-in: the epilogue accumulates onto dx0
    "imp_dx_acc": ccase(2, 16, 8, 8, 24, 3, pad=1, dx_acc=True),
    "imp_g2_dx_acc": ccase(2, 32, 8, 8, 48, 3, pad=1, groups=2,
                           dx_acc=True),
    # small-C kernels (C % 8 != 0, stride 1): 10x10 taps of 3 channels;
    # pad 0 is the all-interior fast path (the last column has
    # w0 C + S C == W C, the last row h + R == H), pad > 0 the edge path
    "sc_c3_pad0": ccase(2, 3, 14, 13, 16, 10, route="implicit_sc",
                        dx="col2im"),
    "sc_c3_pad2": ccase(2, 3, 12, 11, 16, 10, pad=2, relu=True,
                        route="implicit_sc", dx="col2im"),
    "sc_c4_9x9": ccase(2, 4, 12, 12, 24, 9, pad=1, route="implicit_sc",
                       dx="col2im"),
    # space-to-depth route (from test_conv_s2d.py's table)
    "s2d_c4_9x9_s2": ccase(2, 4, 21, 21, 16, 9, stride=2, pad=4,
                           route="s2d", dx="col2im"),
    # materialised-col fallback: Cg % 8 != 0, grouped (Kpad 56, narrow dw)
    # and C = 20 (Kpad 184: the wide trans/trans dw over col)
    "col_g2_cg6": ccase(2, 12, 8, 8, 16, 3, pad=1, groups=2, route="col",
                        dx="col2im"),
    "col_c20": ccase(2, 20, 8, 8, 16, 3, pad=1, relu=True, route="col",
                     dx="col2im"),
    "col_c20_stride2_dil2": ccase(2, 20, 11, 11, 16, 3, stride=2, pad=2,
                                  dil=2, route="col", dx="col2im"),
    # 1x1 route, with its store-3 dx
    "1x1_8x8": ccase(2, 32, 8, 8, 24, 1, route="is_1x1", dx="1x1"),
    "1x1_9x9_acc": ccase(2, 32, 9, 9, 24, 1, route="is_1x1", dx="1x1",
                         dx_acc=True),
}


def conv_dims(c):
    eff_r, eff_s = (c["r"] - 1) * c["dil"] + 1, (c["s"] - 1) * c["dil"] + 1
    p = (c["h"] + 2 * c["pad"] - eff_r) // c["stride"] + 1
    q = (c["w"] + 2 * c["pad"] - eff_s) // c["stride"] + 1
    return p, q


def _thin(t, density, g):
    if density >= 1.0:
        return t
    return t * (torch.rand(t.shape, generator=g) < density).float()


def conv_inputs(c, cls, seed):
    """x, dy, dx0 bf16-representable fp32; w fp32 holding bf16 values (the
    repack rounds nothing); b fp32.  Every group gets its own data."""
    g = gen(seed)
    p, q = conv_dims(c)
    cg = c["c"] // c["groups"]
    xs, ws = (c["n"], c["c"], c["h"], c["w"]), (c["k"], cg, c["r"], c["s"])
    ys = (c["n"], c["k"], p, q)
    if cls == "exact":
        d = c["density"]
        x = _thin(_ints(xs, -1, 1, g), d, g)
        w = _ints(ws, -3, 3, g)
        b = _ints((c["k"],), -4, 4, g)
        dy = _thin(_ints(ys, -1, 1, g), d, g)
        dx0 = _ints(xs, -8, 8, g)
    else:
        x, w = _rnd(xs, g, 0.25), _rnd(ws, g, -0.0625, 0.25)
        b = torch.randn(c["k"], generator=g) + 0.5
        dy, dx0 = _rnd(ys, g, 0.125), _rnd(xs, g, 1.0, 3.0)
    return dict(x=x, w=w, b=b if c["bias"] else None, dy=dy,
                dx0=dx0 if c["dx_acc"] else None, cls=cls)


def _conv_args(c):
    return dict(stride=c["stride"], padding=c["pad"], dilation=c["dil"],
                groups=c["groups"])


def _conv_dx64(c, w, dy):
    from torch.nn import grad as G
    st, pd, dl = (c["stride"],) * 2, (c["pad"],) * 2, (c["dil"],) * 2
    return G.conv2d_input((c["n"], c["c"], c["h"], c["w"]), w, dy, st, pd,
                          dl, c["groups"])


def _conv_dw64(c, x, dy):
    from torch.nn import grad as G
    cg = c["c"] // c["groups"]
    st, pd, dl = (c["stride"],) * 2, (c["pad"],) * 2, (c["dil"],) * 2
    return G.conv2d_weight(x, (c["k"], cg, c["r"], c["s"]), dy, st, pd, dl,
                           c["groups"])


def conv_geometry_ok(c):
    """A padded case has zero-filled and in-image taps on every border."""
    p, q = conv_dims(c)
    if p < 1 or q < 1:
        return False
    if c["pad"] == 0:
        return True
    for size, outs, taps in ((c["h"], p, c["r"]), (c["w"], q, c["s"])):
        first = [-c["pad"] + t * c["dil"] for t in range(taps)]
        last = [(outs - 1) * c["stride"] + f for f in first]
        if not (any(v < 0 for v in first) and any(v >= size for v in last)
                and any(0 <= v < size for v in first)
                and any(0 <= v < size for v in last)):
            return False
    return True


def conv_oracle(c, inp, splits_dw=1):
    x, w, dy = inp["x"].double(), inp["w"].double(), inp["dy"].double()
    b = inp["b"].double() if inp["b"] is not None else None
    exact = inp["cls"] == "exact"
    kw = _conv_args(c)
    cg, kg = c["c"] // c["groups"], c["k"] // c["groups"]
    rs = c["r"] * c["s"]
    p, q = conv_dims(c)
    npq = c["n"] * p * q

    def bf_form(want, t, k):
        tol = (k + 1 + 4) * E32 * t
        return tol + U * (want.abs() + tol)

    y = F.conv2d(x, w, b, **kw)
    ty = F.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), **kw)
    peak = y.abs().max().item()
    if c["relu"]:
        y = y.clamp_min(0)
    dx = _conv_dx64(c, w, dy)
    tdx = _conv_dx64(c, w.abs(), dy.abs())
    peak = max(peak, dx.abs().max().item())
    if c["dx"] == "col2im":
        tol_dx = (2 * U + (kg + rs + 8) * E32 + INTR) * tdx
    else:
        k_dx = c["k"] if c["dx"] == "1x1" else rs * kg
        if inp["dx0"] is not None:
            dx = dx + inp["dx0"].double()
            tdx = tdx + inp["dx0"].double().abs()
            peak = max(peak, dx.abs().max().item())
        tol_dx = bf_form(dx, tdx, k_dx)
    dw = _conv_dw64(c, x, dy)
    tdw = _conv_dw64(c, x.abs(), dy.abs())
    db = dy.sum(dim=(0, 2, 3))
    if exact:
        return {"y": (y.to(BF), None), "dx": (dx.to(BF), None),
                "dw": (dw.float(), None), "db": (db.float(), None)}, peak
    return {"y": (y, bf_form(y, ty, rs * cg)), "dx": (dx, tol_dx),
            "dw": (dw, (npq + splits_dw + 4) * E32 * tdw),
            "db": (db, (2 * npq + 4) * E32
                   * dy.abs().sum(dim=(0, 2, 3)))}, peak


def _unfold_cols(x, c, padding_mode="zeros"):
    """[N, groups, Cg, R*S, P*Q] taps of x."""
    r, s, pad = c["r"], c["s"], c["pad"]
    if padding_mode == "clamp" and pad > 0:
        x = F.pad(x, (pad,) * 4, mode="replicate")
        pad = 0
    cols = F.unfold(x, (r, s), dilation=c["dil"], padding=pad,
                    stride=c["stride"])
    cg = c["c"] // c["groups"]
    return cols.view(c["n"], c["groups"], cg, r * s, -1)


def conv_emulate(c, inp, mutant=None):
    """fp32 arithmetic, bf16 where the route stores bf16 (y, dx, and dcol
    on the col2im route)."""
    x, w, dy = inp["x"].float(), inp["w"].float(), inp["dy"].float()
    b = inp["b"]
    kw = _conv_args(c)
    g = c["groups"]
    cg, kg = c["c"] // g, c["k"] // g
    wf, xf = w, x
    if mutant == "rs_swapped":
        wf = w.transpose(2, 3).reshape(w.shape)
    if mutant == "group_window_off":
        xf = torch.roll(x, -cg, dims=1)
    if mutant == "pad_clamped" and c["pad"] > 0:
        xp = F.pad(xf, (c["pad"],) * 4, mode="replicate")
        y = F.conv2d(xp, wf, b, stride=c["stride"], dilation=c["dil"],
                     groups=g)
    else:
        y = F.conv2d(xf, wf, b, **kw)
    if c["relu"]:
        y = y.clamp_min(0)
    wd = w.flip(2, 3) if mutant == "dx_not_flipped" else w
    if c["dx"] == "col2im":
        # dcol[n, g, cg, rs, pq] = sum_kg dy * w, bf16; fold in fp32
        p, q = conv_dims(c)
        dyg = dy.view(c["n"], g, kg, p * q)
        wg = wd.view(g, kg, cg, c["r"] * c["s"])
        dcol = rb(torch.einsum("ngkp,gkcr->ngcrp", dyg, wg))
        dx = F.fold(dcol.reshape(c["n"], c["c"] * c["r"] * c["s"], p * q),
                    (c["h"], c["w"]), (c["r"], c["s"]), dilation=c["dil"],
                    padding=c["pad"], stride=c["stride"])
    else:
        dx = _conv_dx64(c, wd, dy)
        if inp["dx0"] is not None and mutant != "c0_dropped":
            dx = dx + inp["dx0"].float()
    dw = _conv_dw64(c, xf, dy)
    out = {"y": bf16(y), "dx": bf16(dx), "dw": dw,
           "db": dy.sum(dim=(0, 2, 3))}
    if mutant == "truncate":
        out["y"], out["dx"] = trunc_bf16(y), trunc_bf16(dx)
    return out


CONV_MUTANTS = ["pad_clamped", "rs_swapped", "group_window_off",
                "dx_not_flipped", "c0_dropped", "truncate"]


# direct gemm_conv_fwd calls on a poisoned input: NaN before and after x
# and in every channel outside the group window
FWD_DIRECT_CASES = {
    "g2_second_window": ccase(2, 32, 8, 8, 48, 3, pad=1, groups=2),
    "g4_stride2_dil2": ccase(2, 32, 11, 11, 32, 3, stride=2, pad=2, dil=2,
                             groups=4, relu=True),
    "g1_k64_nopad": ccase(2, 8, 8, 9, 16, 2, 3),
}


def kpad_dma(k):
    return max(64, -(-k // 32) * 32)


# =========================================================== column kernels

def colcase(n, h, w, c, r, s=None, stride=1, pad=0, dil=1, c0=0, ct=None,
            kpad=None):
    s = r if s is None else s
    ct = c if ct is None else ct
    kcol = r * s * ct
    return dict(n=n, h=h, w=w, c=c, r=r, s=s, stride=stride, pad=pad,
                dil=dil, c0=c0, ct=ct, groups=1, kcol=kcol,
                kpad=kpad or -(-kcol // 8) * 8)


# im2col_nhwc: the LUT kernel when Kpad <= 2560 and the packed fields fit
# (runs8: Ct % 8 == 0; runfast: pad 0, dil 1, full channels, S C >= 8;
# LUT scalar otherwise), the generic kernel beyond
IM2COL_CASES = {
    "runs8_c16": colcase(2, 7, 6, 16, 3, pad=1),
    "runs8_kpad_dma": colcase(2, 6, 6, 8, 2, 3, kpad=64),
    "runs8_stride2_dil2": colcase(2, 11, 9, 8, 3, stride=2, pad=2, dil=2),
    "runs8_window": colcase(2, 7, 6, 32, 3, pad=1, c0=8, ct=16),
    # C = 3, 5 taps wide: S C = 15, slots straddle a filter-row boundary,
    # also on the last image row
    "runfast_c3": colcase(2, 9, 8, 3, 5),
    "runfast_c3_10x10": colcase(1, 11, 10, 3, 10),
    "lut_scalar_pad": colcase(2, 9, 8, 3, 5, pad=2),
    "lut_scalar_5x1": colcase(2, 9, 8, 1, 5, 1),          # S C = 1 < 8
    "lut_scalar_window": colcase(2, 7, 6, 12, 3, pad=1, c0=6, ct=6),
    "generic_c296": colcase(1, 5, 5, 296, 3, pad=1),      # Kpad 2664
    "generic_ct_odd": colcase(1, 5, 4, 300, 3, pad=1, c0=3, ct=291),
    # LUT field width: channel offsets >= 1024 must not carry into dw
    "lutwidth_c1032": colcase(1, 3, 3, 1032, 1, stride=2),
    "lutwidth_c2056": colcase(1, 3, 3, 2056, 1, stride=2),
    "lutwidth_c1032_pad": colcase(1, 4, 4, 1032, 1, pad=1),
    "lutwidth_c1100_1x2": colcase(1, 3, 4, 1100, 1, 2, ct=1096, c0=4),
}

COL2IM_CASES = {
    "s1_pad0": colcase(2, 7, 6, 16, 3),
    "s1_padmax": colcase(2, 7, 6, 16, 3, pad=2),
    "s1_window": colcase(2, 6, 5, 32, 2, 3, pad=1, c0=8, ct=16),
    "generic_stride2": colcase(2, 9, 8, 16, 3, stride=2, pad=1),
    "generic_dil2": colcase(2, 9, 8, 8, 3, pad=2, dil=2),
    "generic_ct_odd_window": colcase(2, 7, 6, 12, 3, pad=1, c0=6, ct=6),
    "generic_stride2_dil2_odd": colcase(2, 11, 10, 10, 3, stride=2, pad=2,
                                        dil=2, c0=3, ct=5),
}

# NPQ = 2*7*7 = 98: a tail of 2 under the 8-wide slot, rows start at k*98
IM2COL_T_CASES = {
    "npq98": colcase(2, 9, 9, 8, 3),
    "npq98_window_pad": colcase(2, 7, 7, 12, 3, pad=1, c0=4, ct=4),
    "npq330_stride2": colcase(3, 21, 19, 3, 3, stride=2, pad=1),
}


def col_inputs(c, cls, seed):
    g = gen(seed)
    p, q = conv_dims(c)
    npq = c["n"] * p * q
    xs = (c["n"], c["c"], c["h"], c["w"])
    if cls == "exact":
        x = _ints(xs, -3, 3, g)
        dcol = _ints((npq, c["kcol"]), -3, 3, g)
    else:
        x, dcol = _rnd(xs, g, 0.25), _rnd((npq, c["kcol"]), g, 0.125)
    return dict(x=x, dcol=dcol, cls=cls)


def im2col_want(c, x, mutant=None):
    """[NPQ, Kpad] with column (r S + s) Ct + ch, pad columns zero."""
    p, q = conv_dims(c)
    xw = x[:, c["c0"]:c["c0"] + c["ct"]]
    cc = dict(c, c=c["ct"])
    cols = _unfold_cols(xw, cc)[:, 0]               # [N, Ct, RS, PQ]
    if mutant == "lut_carry" and c["ct"] > 1024:
        # channel offset >= 1024 decoded as (dw + 1, ch - 1024): the tap
        # one pixel to the right, zero outside the image
        xs = torch.zeros_like(x)
        xs[..., :-1] = x[..., 1:]
        xw2 = xs[:, c["c0"]:c["c0"] + c["ct"]]
        alt = _unfold_cols(xw2, cc)[:, 0]
        cols = cols.clone()
        cols[:, 1024:] = alt[:, :c["ct"] - 1024]
    col = cols.permute(0, 3, 2, 1).reshape(c["n"] * p * q, c["kcol"])
    out = torch.zeros(c["n"] * p * q, c["kpad"], dtype=x.dtype)
    out[:, :c["kcol"]] = col
    return out


def col2im_oracle(c, inp):
    """dx over the window channels [N, Ct, H, W]."""
    p, q = conv_dims(c)
    rs = c["r"] * c["s"]

    def fold(d):
        cols = d.view(c["n"], p * q, rs, c["ct"]).permute(0, 3, 2, 1) \
            .reshape(c["n"], c["ct"] * rs, p * q)
        return F.fold(cols, (c["h"], c["w"]), (c["r"], c["s"]),
                      dilation=c["dil"], padding=c["pad"],
                      stride=c["stride"])
    d = inp["dcol"].double()
    want, t = fold(d), fold(d.abs())
    if inp["cls"] == "exact":
        return {"dx": (want.to(BF), None)}, want.abs().max().item()
    return {"dx": (want, (U + (rs + 2) * E32) * t)}, 0.0


def col2im_emulate(c, inp, mutant=None):
    p, q = conv_dims(c)
    rs = c["r"] * c["s"]
    d = inp["dcol"].float()
    cols = d.view(c["n"], p * q, rs, c["ct"])
    if mutant == "rs_swapped" and c["r"] == c["s"]:
        cols = cols.view(c["n"], p * q, c["r"], c["s"], c["ct"]) \
            .transpose(2, 3).reshape(c["n"], p * q, rs, c["ct"])
    cols = cols.permute(0, 3, 2, 1).reshape(c["n"], c["ct"] * rs, p * q)
    dx = F.fold(cols, (c["h"], c["w"]), (c["r"], c["s"]), dilation=c["dil"],
                padding=c["pad"], stride=c["stride"])
    return {"dx": trunc_bf16(dx) if mutant == "truncate" else bf16(dx)}


TRANSPOSE_SHAPES = [(1, 1), (127, 63), (128, 64), (130, 70), (257, 129)]
# (rows, cols, ld - cols)
COLSUM_CASES = [(1, 1, 3), (98, 8, 8), (98, 20, 4), (3000, 20, 0),
                (98, 264, 8), (3000, 264, 0), (1, 264, 8)]
BIAS_ACT_SHAPES = [(1, 1), (5, 77), (64, 4096)]


def colsum_inputs(rows, cols, cls, seed):
    g = gen(seed)
    if cls == "exact":
        return dict(x=_ints((rows, cols), -3, 3, g),
                    out0=_ints((cols,), -8, 8, g), cls=cls)
    return dict(x=_rnd((rows, cols), g, 0.25),
                out0=torch.randn(cols, generator=g) * 3 + 1, cls=cls)


def colsum_oracle(inp):
    x, o = inp["x"].double(), inp["out0"].double()
    want = o + x.sum(dim=0)
    if inp["cls"] == "exact":
        return {"out": (want.float(), None)}
    rows = x.shape[0]
    return {"out": (want, (2 * rows + 4) * E32
                    * (o.abs() + x.abs().sum(dim=0)))}


def colsum_emulate(inp, mutant=None):
    x = inp["x"].float()
    if mutant == "drop_last_row":
        x = x[:-1]
    s = x.sum(dim=0)
    return {"out": s if mutant == "out0_dropped" else inp["out0"].float() + s}


def bias_act_inputs(rows, cols, cls, seed):
    g = gen(seed)
    if cls == "exact":
        return dict(x=_ints((rows, cols), -200, 200, g),
                    bias=_ints((cols,), -8, 8, g), cls=cls)
    return dict(x=torch.randn(rows, cols, generator=g) * 3 + 0.25,
                bias=torch.randn(cols, generator=g) + 0.5, cls=cls)


def bias_act_oracle(inp, bias, relu):
    x = inp["x"].double()
    t = x.abs()
    if bias:
        x = x + inp["bias"].double()
        t = t + inp["bias"].double().abs()
    if relu:
        x = x.clamp_min(0)
    if inp["cls"] == "exact":
        return {"out": (x.to(BF), None)}
    return {"out": (x, (U + 4 * E32) * t)}


def bias_act_emulate(inp, bias, relu, mutant=None):
    x = inp["x"].float()
    if mutant == "relu_before_bias" and relu:
        x = x.clamp_min(0)
    if bias:
        x = x + inp["bias"].float()
    if relu and mutant != "relu_before_bias":
        x = x.clamp_min(0)
    return {"out": trunc_bf16(x) if mutant == "truncate" else bf16(x)}


# ================================================================= Winograd
# F(2x2, 3x3), winograd.hip.  Rounding points, read from the kernels: U =
# G w G^T, V = B^T d B and M = sum_c V U (gemm_kernel store 0, batch 16)
# are each stored as bf16, and so is y = A^T M A + b: four roundings, the
# transforms and the reduction over Cin in fp32 between them.  With
# Ubar = |G||w||G^T|, Vbar = |B^T||d||B|, Mbar = sum_c Vbar Ubar and
# Ybar = |A^T| Mbar |A| + |b| (all >= the magnitudes they bound, so
# cancellation in the transforms is covered):
#     tol = (4u + 8I + (Cin + 16) e) Ybar
# 4u the roundings, 8I their cross terms (u*u = I, six pairs, rounded up),
# (Cin + 16) e the fp32 reduction and the transforms' additions.  The data
# gradient (flip) is the same pipeline over dy with the filter rotated 180
# degrees and K, C swapped, so Cin is the forward K there.
# Exact class: G holds halves, so the weights are multiples of 4; U, V, M
# and y must all stay integers <= 256 (asserted on the oracle).

WINO_G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]
WINO_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
WINO_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def wcase(n, h, w, c, k, bias=False, relu=False):
    return dict(n=n, h=h, w=w, c=c, k=k, bias=bias, relu=relu)


WINO_CASES = {
    "13x13_c8_k8": wcase(2, 13, 13, 8, 8),              # ragged both ways
    "6x8_c8_k8": wcase(2, 6, 8, 8, 8),                  # no ragged tile
    "13x12_c8_k16_bias_relu": wcase(2, 13, 12, 8, 16, bias=True, relu=True),
    # U has zero pad rows (256 allocated for 136 / 32 live)
    "13x13_c32_k136": wcase(1, 13, 13, 32, 136),
    "7x9_c32_k136_bias_relu": wcase(2, 7, 9, 32, 136, bias=True, relu=True),
}


def wino_inputs(c, cls, seed):
    g = gen(seed)
    xs, ws = (c["n"], c["c"], c["h"], c["w"]), (c["k"], c["c"], 3, 3)
    ys = (c["n"], c["k"], c["h"], c["w"])
    if cls == "exact":
        x, w = _ints(xs, -1, 1, g), 4 * _ints(ws, -1, 1, g)
        b, dy = _ints((c["k"],), -4, 4, g), _ints(ys, -1, 1, g)
        if c["k"] > 64:         # keep the K-long dgrad sums under 256
            dy = _thin(dy, 0.25, g)
    else:
        x, w = _rnd(xs, g, 0.25), _rnd(ws, g, -0.0625, 0.25)
        b, dy = torch.randn(c["k"], generator=g) + 0.5, _rnd(ys, g, 0.125)
    return dict(x=x, w=w, b=b if c["bias"] else None, dy=dy, cls=cls)


def _wino_pipeline(x, w_eff, dtype, rnd, absolute=False):
    """[N, Kout, 2 th, 2 tw] output tiles (uncropped, no bias) and the
    largest |U|, |V|, |M| on the way."""
    def mat(m):
        t = torch.tensor(m, dtype=dtype)
        return t.abs() if absolute else t
    g, bt, at = mat(WINO_G), mat(WINO_BT), mat(WINO_AT)
    n, cin, h, w = x.shape
    kout = w_eff.shape[0]
    th, tw = (h + 1) // 2, (w + 1) // 2
    xp = F.pad(x.to(dtype), (1, 2 * tw + 1 - w, 1, 2 * th + 1 - h))
    tiles = F.unfold(xp, 4, stride=2).view(n, cin, 4, 4, th * tw)
    v = rnd(torch.einsum("ia,ncabt,jb->ncijt", bt, tiles, bt))
    u = rnd(torch.einsum("ia,kcab,jb->kcij", g, w_eff.to(dtype), g))
    m = rnd(torch.einsum("ncijt,kcij->nkijt", v, u))
    y = torch.einsum("pi,nkijt,qj->nkpqt", at, m, at)
    y = y.reshape(n, kout, 2, 2, th, tw).permute(0, 1, 4, 2, 5, 3) \
        .reshape(n, kout, 2 * th, 2 * tw)
    peak = max(t.abs().max().item() for t in (u, v, m))
    return y, peak


def _wino_operands(inp, flip):
    if flip:
        return inp["dy"], inp["w"].flip(2, 3).transpose(0, 1), None
    return inp["x"], inp["w"], inp["b"]


def wino_oracle(c, inp, flip):
    x, w_eff, b = _wino_operands(inp, flip)
    h, w = c["h"], c["w"]
    b64 = b.double() if b is not None else None
    want = F.conv2d(x.double(), w_eff.double(), b64, padding=1)
    relu = c["relu"] and not flip
    name = "dx" if flip else "y"
    if inp["cls"] == "exact":
        _, peak = _wino_pipeline(x, w_eff, torch.float64, lambda t: t)
        peak = max(peak, want.abs().max().item())
        if relu:
            want = want.clamp_min(0)
        return {name: (want.to(BF), None)}, peak
    if relu:
        want = want.clamp_min(0)
    ybar, _ = _wino_pipeline(x.abs(), w_eff.abs(), torch.float64,
                             lambda t: t, absolute=True)
    ybar = ybar[:, :, :h, :w]
    if b64 is not None:
        ybar = ybar + b64.abs().view(1, -1, 1, 1)
    cin = w_eff.shape[1]
    return {name: (want, (4 * U + 8 * INTR + (cin + 16) * E32) * ybar)}, 0.0


def wino_emulate(c, inp, flip, mutant=None):
    x, w_eff, b = _wino_operands(inp, flip)
    h, w = c["h"], c["w"]
    y, _ = _wino_pipeline(x, w_eff, torch.float32, rb)
    if b is not None:
        y = y + b.float().view(1, -1, 1, 1)
    if c["relu"] and not flip:
        y = y.clamp_min(0)
    out = y[:, :, :h, :w].contiguous()
    if mutant == "no_ragged_guard":
        # NHWC stores past q = Q-1 / p = P-1 land on the next row / image
        n, k = out.shape[:2]
        flat = torch.zeros(n * h * w + 2 * (w + 2), k)
        flat[:n * h * w] = out.permute(0, 2, 3, 1).reshape(-1, k)
        for p in range(y.shape[2]):
            for q in range(y.shape[3]):
                if p < h and q < w:
                    continue
                for ni in range(n):
                    flat[(ni * h + p) * w + q] = y[ni, :, p, q]
        out = flat[:n * h * w].view(n, h, w, k).permute(0, 3, 1, 2)
    return {"dx" if flip else "y": bf16(out)}
