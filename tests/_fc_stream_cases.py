"""Cases, inputs, float64 oracle, fp32 emulation and mutants for the
weight-streaming InnerProduct GEMM (gemm_fc_kernel + fc_slab_finalize in
gemm.hip / elementwise.hip).  Shared by test_fc_stream_bounds.py (CPU) and
test_fc_stream_gpu.py (GPU).  Conventions of _gemm_bounds.py: the oracle
takes the tensors the kernel gets, computes in float64 and returns
{name: (want, tol)}, tol None meaning bit-exact; no bound comes from what a
kernel returned.

The product is out[M, N] = act(A[M, K] Bp[N, K]^T + bias) stored as bf16.
kind "fwd" keeps Bp as it is (W [N][K]); kind "dx" stores it transposed
(W [K][N]): the values are the same, only the layout the kernel reads.

Split-K by slabs: split s accumulates k in [s ksplit, min(K, (s+1) ksplit))
in ascending order into an fp32 partial (slab s); the finalize adds the slabs
in ascending s, then the bias, applies ReLU and rounds once to bf16.

Bound (rounded class), T = |A| |Bp|^T + |bias| in float64: every slab is an
fp32 accumulation of its K_s products (exact in fp32: 8 + 8 significand
bits), the finalize adds `splits` partials and one bias; rule B3 of
_bf16_bounds.py gives tol_acc = (K + splits + 4) e T, and the bf16 store
(rule B1) tol = tol_acc + u (|want| + tol_acc).  ReLU is 1-Lipschitz.
The exact class (A in {-1, 0, 1}, Bp in {-2 .. 2}, integer bias: every
partial sum is an integer far below 2^24, so fp32 is exact in any order)
must come out bit-exact; precondition, asserted by the tests on the
oracle's `peak`: |result| <= 256, so that it is a bf16 integer.
"""

import torch

from _bf16_bounds import U, E32, BF, gen, bf16, rb
from _gemm_bounds import split_k, BK

FC_BN = 128          # the kernel's N tile

MS = (1, 64, 130, 256)
NS = (16, 72, 200, 264)
KS = (64, 104, 328, 1000)
SKS = (1, 2, 3, 7)


def fcase(M, N, K, sk, bias, relu):
    return dict(M=M, N=N, K=K, sk=sk, bias=bias, relu=relu)


def _table():
    """Every (M, N) pair once; K and sk each run through all four values
    along every row and column (two Latin squares)."""
    t = {}
    for a, M in enumerate(MS):
        for b, N in enumerate(NS):
            K = KS[(a + b) % 4]
            sk = SKS[(a - b) % 4]
            c = fcase(M, N, K, sk, bias=(a + b) % 2 == 0, relu=b % 2 == 0)
            t[f"m{M}_n{N}_k{K}_sk{sk}"] = c
    # the ragged last split and the one-tile split with everything on
    t["m256_n264_k1000_sk7_br"] = fcase(256, 264, 1000, 7, True, True)
    t["m130_n200_k64_sk7_br"] = fcase(130, 200, 64, 7, True, True)
    t["m64_n72_k104_sk3_b"] = fcase(64, 72, 104, 3, True, False)
    return t


FC_CASES = _table()
# output widths that are no multiple of 8 (forward only: the data gradient
# needs whole 8-column octets of W and keeps the legacy route): the
# element-wise bf16 store, the 16-byte slab store with the scalar finalize
# (N % 4 == 0), and the element-wise slab store
FC_CASES["m64_n10_k800_sk1_br"] = fcase(64, 10, 800, 1, True, True)
FC_CASES["m64_n500_k800_sk3_br"] = fcase(64, 500, 800, 3, True, True)
FC_CASES["m130_n10_k64_sk2_b"] = fcase(130, 10, 64, 2, True, False)
KINDS = ("fwd", "dx")
CLASSES = ("exact", "rounded")


def fc_inputs(c, cls, seed):
    g = gen(seed)
    M, N, K = c["M"], c["N"], c["K"]
    if cls == "exact":
        A = torch.randint(-1, 2, (M, K), generator=g).float()
        Bp = torch.randint(-2, 3, (N, K), generator=g).float()
        bias = torch.randint(-4, 5, (N,), generator=g).float()
    else:
        A = rb(torch.randn((M, K), generator=g) + 0.25)
        Bp = rb(torch.randn((N, K), generator=g) * 0.5 + 0.1)
        bias = torch.randn((N,), generator=g)
    return dict(A=A, Bp=Bp, bias=bias if c["bias"] else None, cls=cls)


def fc_oracle(c, inp):
    A, B = inp["A"].double(), inp["Bp"].double()
    _, splits = split_k(c["K"], c["sk"])
    s = A @ B.t()
    t = A.abs() @ B.abs().t()
    if inp["bias"] is not None:
        s = s + inp["bias"].double()
        t = t + inp["bias"].double().abs()
    peak = s.abs().max().item()
    if c["relu"]:
        s = s.clamp_min(0)
    if inp["cls"] == "exact":
        return {"out": (s.to(BF), None)}, peak
    tol = (c["K"] + splits + 4) * E32 * t
    tol = tol + U * (s.abs() + tol)
    return {"out": (s, tol)}, peak


FC_MUTANTS = ["drop_last_split", "drop_tail_tile", "bias_per_slab",
              "relu_per_slab", "ntail_from_neighbour", "rows_128_dropped"]


def fc_emulate(c, inp, mutant=None):
    """fp32 with the kernel's rounding points."""
    A, B = inp["A"].float(), inp["Bp"].float()
    M, N, K = c["M"], c["N"], c["K"]
    ksplit, splits = split_k(K, c["sk"])
    bias = inp["bias"].float() if inp["bias"] is not None else None
    slabs = []
    for s in range(splits):
        ks, ke = s * ksplit, min(K, (s + 1) * ksplit)
        if s == splits - 1 and mutant == "drop_tail_tile":
            ke = K - (K % BK or BK)
        acc = torch.zeros(M, N)
        for k in range(ks, ke):                  # ascending k, fp32
            acc = acc + A[:, k:k + 1] * B[:, k].unsqueeze(0)
        if mutant == "bias_per_slab" and bias is not None:
            acc = acc + bias
        if mutant == "relu_per_slab" and c["relu"]:
            acc = acc.clamp_min(0)
        slabs.append(acc)
    if mutant == "drop_last_split" and splits > 1:
        slabs = slabs[:-1]
    v = torch.zeros(M, N)
    for acc in slabs:                            # ascending s
        v = v + acc
    if bias is not None and mutant != "bias_per_slab":
        v = v + bias
    if c["relu"]:
        v = v.clamp_min(0)
    if mutant == "ntail_from_neighbour" and N % FC_BN and N > FC_BN:
        n0 = N // FC_BN * FC_BN
        v = v.clone()
        v[:, n0:] = v[:, n0 - FC_BN:N - FC_BN]
    if mutant == "rows_128_dropped" and M > 128:
        v = v.clone()
        v[128:] = 0
    return {"out": bf16(v)}
