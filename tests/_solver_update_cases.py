"""Layouts, inputs, float64 oracles, fp32 emulations and mutants for the
three fused whole-arena solver updates (sgd_update_multi_kernel,
nesterov_update_multi_kernel, adam_update_multi_kernel in elementwise.hip).
Shared by test_solver_update_bounds.py (CPU) and test_solver_update_gpu.py
(GPU).  Conventions of _bf16_bounds.py: an oracle takes the tensors the
kernel gets, computes in float64 and returns {name: (want, tol)}; no bound
comes from what a kernel returned.

The arena is a packed run of segments, segment s being elements
[off[s], off[s+1]) with its own fp32 lr[s] and wd[s].  Every element is
updated with the parameters of the segment that owns it, wherever the
segment starts; a segment with lr == 0 is frozen.  The kernels take one
quad (4 elements) per thread and iteration, so the layouts put segment
boundaries at every position inside a quad.

The oracle reads the same fp32 seg_lr and seg_wd tensors the kernel is
handed, and mu, b1, b2, eps rounded to fp32 as the launcher's float
arguments are; the owner of an element comes from torch.bucketize on the
offsets.  With gg = g + wd p:

 SGD       v' = mu v + lr gg,  p' = p - v'
 Nesterov  v' = mu v + lr gg,  p' = p - ((1 + mu) v' - mu v)
 Adam      m' = b1 m + (1 - b1) gg,  v' = b2 v + (1 - b2) gg^2,
           p' = p - lr m' / (sqrt(v') + eps), the bias correction being
           folded into lr by the caller

Bounds (e = 2^-24; rules B1 and B3 of _bf16_bounds.py): c e T, T the sum of
the absolute values of the expression's terms in float64 and c the number
of fp32 roundings on the longest path a term takes to the output, plus one
(every rounding adds at most e times the terms that pass through it, and
T carries the factors applied afterwards; contraction into FMAs only
removes roundings).  The extension is built with -O3 alone (setup.py; the
loader adds no flag): no fast-math flag, and hipcc's default for HIP code
keeps the fp32 divide and sqrtf correctly rounded, so each is charged one
e, not the INTR of rule B4.

 SGD v'       wd p, + g, lr *, + mu v: 4 roundings, c = 5,
              T = mu |v| + lr (|g| + wd |p|)
 SGD p'       one more subtraction: c = 6, T = |p| + T_v
 Nesterov v'  as SGD: c = 5
 Nesterov p'  v' (4), the constant 1 + mu, its product, - mu v, p -:
              8 roundings, c = 9, T = |p| + (1 + mu) T_v + mu |v|
 Adam m'      wd p, + g, the constant 1 - b1, its product, + b1 m:
              5 roundings, c = 6, T = b1 |m| + (1 - b1)(|g| + wd |p|)
 Adam v'      gg enters squared, so its 2 roundings count twice; the
              constant 1 - b2, two products, + b2 v: 8 roundings, c = 9,
              T = b2 v + (1 - b2)(|g| + wd |p|)^2
 Adam p'      with D = sqrt(v') + eps and Tq = lr T_m / D:
              tol_D = sqrt(v') - sqrt(max(v' - tol_v, 0)) + 2 e D (the
              exact one-sided change of the root, then sqrtf and + eps),
              tol_q = Tq (c_m + 2) e + Tq tol_D / (D - tol_D)   (m', lr *, /)
              tol_p = tol_q + 2 e (|p| + Tq)                    (p -)
              Where v' has no cancellation tol_D / D is about 6.5 e and the
              whole is about 16.5 e (|p| + Tq).

A frozen segment keeps p, v (and m) bit for bit: want is the input and the
bound is 0 there.  The bf16 shadow is checked apart from the bound on p:
it equals bf16(p') of the p' the route ITSELF produced, bit for bit, and
keeps its previous content in frozen segments (shadow_expect).
"""

import functools

import torch

from _bf16_bounds import U, E32, BF, gen, bf16    # noqa: F401

SOLVERS = ("sgd", "nesterov", "adam")
MAX_SEG = 512                       # COS_SGD_MAX_SEG, the LDS table capacity
SWEEP = 2048 * 256 * 4              # launcher's block cap x one quad a thread

# the existing solver tests' hyper-parameters
RATE, MU, WD = 0.05, 0.9, 0.001
B1, B2, EPS = 0.9, 0.999, 1e-8
ADAM_T = 3                          # iteration whose correction is folded in
SENTINEL = -7.0                     # shadow content before the update

LENET_SIZES = [500, 20, 25000, 50, 400000, 500, 5000, 10]
LENET_OFFSETS = [0, 500, 520, 25520, 25570, 425570, 426070, 431070, 431080]
LENET_QUAD_OWNER_MISSES = [25570, 25571, 425570, 425571, 426070, 426071,
                           431070, 431071]


def _alt(n, a, b):
    return [a if i % 2 == 0 else b for i in range(n)]


def _grid_stride():
    """A little over one sweep of the capped grid.  An odd boundary in the
    first sweep; ten tiny segments ending two elements before the sweep
    boundary, so that thread 0's cursor jumps twelve segments between its
    two iterations and the quad before the boundary straddles; an odd
    boundary in the second sweep."""
    tiny = [1, 2, 3, 1, 2, 3, 1, 2, 3, 1]
    first = 1_000_001
    second = SWEEP - 2 - sum(tiny) - first
    sizes = [first, second] + tiny + [2 + 1001, 3075 - 1001]
    lrm = _alt(len(sizes), 1.0, 2.0)
    lrm[5] = 0.0                                    # one frozen tiny segment
    return sizes, lrm, _alt(len(sizes), 1.0, 0.0)


def _table(nseg):
    sizes = [(1, 2, 3, 5)[i % 4] for i in range(nseg)]
    lrm = [(1.0, 2.0, 1.0, 0.0, 2.0)[i % 5] for i in range(nseg)]
    return sizes, lrm, _alt(nseg, 1.0, 0.0)


# name -> (segment sizes, lr_mult per segment, decay_mult per segment)
LAYOUTS = {
    "aligned": ([8, 4, 12], [1.0, 2.0, 1.0], [1.0, 0.0, 1.0]),
    "straddle": ([5, 1, 2, 7, 3], [1.0, 2.0, 1.0, 0.0, 1.0],
                 [1.0, 0.0, 1.0, 1.0, 0.0]),
    "three_in_a_quad": ([4, 1, 1, 1, 5], [1.0, 2.0, 1.0, 2.0, 1.0],
                        [1.0, 0.0, 1.0, 0.0, 1.0]),
    "frozen_edges": ([3, 6, 5, 7, 2], [0.0, 1.0, 2.0, 1.0, 0.0],
                     [1.0, 0.0, 1.0, 0.0, 1.0]),
    "single1": ([1], [1.0], [1.0]),
    "single3": ([3], [2.0], [1.0]),
    "single4": ([4], [1.0], [0.0]),
    "single5": ([5], [2.0], [1.0]),
    "lenet": (LENET_SIZES, _alt(8, 1.0, 2.0), _alt(8, 1.0, 0.0)),
    "table_full": _table(MAX_SEG),
    "grid_stride": _grid_stride(),
}
# one segment past the LDS table: the arena wrappers must not launch the
# fused kernels on it (not a layout of the direct kernel calls)
TABLE_OVER = _table(MAX_SEG + 1)

SMALL_LAYOUTS = [n for n in LAYOUTS if n != "grid_stride"]
FOLLOWS_REFERENCE = ("single1", "single3", "single4", "single5", "aligned")
QUAD_OWNER_CAUGHT = ("straddle", "three_in_a_quad", "frozen_edges", "lenet",
                     "grid_stride")

assert sum(LAYOUTS["straddle"][0]) == 18
assert sum(LAYOUTS["grid_stride"][0]) == SWEEP + 3075
assert max(sum(LAYOUTS[n][0]) for n in SMALL_LAYOUTS) < 432 * 1024


def offsets(sizes):
    return torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0)


assert offsets(LENET_SIZES).tolist() == LENET_OFFSETS


def adam_correction(t, b1=B1, b2=B2):
    return (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t)


def seg_params(lrm, dm, solver, rate=RATE, wd=WD, t=ADAM_T):
    """fp32 seg_lr and seg_wd as the arena wrappers of ops/gpu.py form
    them: an fp32 tensor of multipliers times a Python scalar."""
    scale = rate * adam_correction(t) if solver == "adam" else rate
    return (torch.tensor(lrm, dtype=torch.float32) * scale,
            torch.tensor(dm, dtype=torch.float32) * wd)


def build_case(sizes, lrm, dm, solver, seed):
    off = offsets(sizes)
    n = int(off[-1])
    g = gen(seed)
    case = dict(solver=solver, off=off, n=n,
                p=torch.randn(n, generator=g),
                g=torch.randn(n, generator=g) * 0.1,
                v=torch.randn(n, generator=g))
    if solver == "adam":
        case["m"] = case["v"]
        case["v"] = torch.randn(n, generator=g).square()   # second moment
    # a division by eps alone (Adam): no gradient, no second moment
    for k in range(0, n, 7 if n < 4096 else 4099):
        case["g"][k] = 0.0
        case["v"][k] = 0.0
    case["seg_lr"], case["seg_wd"] = seg_params(lrm, dm, solver)
    case["sh0"] = torch.full((n,), SENTINEL, dtype=BF)
    return case


@functools.lru_cache(maxsize=None)
def make_case(layout, solver):
    """Shared by the tests and read-only: nothing may write into it."""
    sizes, lrm, dm = LAYOUTS[layout]
    seed = 4000 + 10 * sorted(LAYOUTS).index(layout) + SOLVERS.index(solver)
    return build_case(sizes, lrm, dm, solver, seed)


def owner(off, n):
    """Segment that owns each element: the count of boundaries <= k."""
    k = torch.arange(n, dtype=torch.int64)
    return torch.bucketize(k, off[1:].contiguous(), right=True).clamp_max(
        off.numel() - 2)


def _f32(x):
    """A Python float as the launcher's float argument, back in float64."""
    return float(torch.tensor(x, dtype=torch.float32))


def trainable(case):
    return case["seg_lr"][owner(case["off"], case["n"])] != 0


# ---------------------------------------------------------------- oracles

def oracle(case):
    seg = owner(case["off"], case["n"])
    lr, wd = case["seg_lr"].double()[seg], case["seg_wd"].double()[seg]
    live = lr != 0
    p, g, v = case["p"].double(), case["g"].double(), case["v"].double()
    gg, gga = g + wd * p, g.abs() + wd * p.abs()
    solver = case["solver"]

    def pick(new, tol, old):
        return (torch.where(live, new, old),
                torch.where(live, tol, torch.zeros_like(tol)))

    if solver in ("sgd", "nesterov"):
        mu = _f32(MU)
        v1 = mu * v + lr * gg
        t_v = mu * v.abs() + lr * gga
        if solver == "sgd":
            p1, t_p, c_p = p - v1, p.abs() + t_v, 6
        else:
            p1 = p - ((1.0 + mu) * v1 - mu * v)
            t_p, c_p = p.abs() + (1.0 + mu) * t_v + mu * v.abs(), 9
        return {"p": pick(p1, c_p * E32 * t_p, p),
                "v": pick(v1, 5 * E32 * t_v, v)}

    b1, b2, eps = _f32(B1), _f32(B2), _f32(EPS)
    m = case["m"].double()
    m1 = b1 * m + (1.0 - b1) * gg
    t_m = b1 * m.abs() + (1.0 - b1) * gga
    v1 = b2 * v + (1.0 - b2) * gg * gg
    tol_v = 9 * E32 * (b2 * v + (1.0 - b2) * gga * gga)
    root = v1.sqrt()
    den = root + eps
    tol_den = root - (v1 - tol_v).clamp_min(0.0).sqrt() + 2 * E32 * den
    p1 = p - lr * m1 / den
    t_q = lr * t_m / den
    tol_q = t_q * (6 + 2) * E32 \
        + t_q * tol_den / (den - tol_den).clamp_min(1e-300)
    tol_p = tol_q + 2 * E32 * (p.abs() + t_q)
    return {"p": pick(p1, tol_p, p), "m": pick(m1, 6 * E32 * t_m, m),
            "v": pick(v1, tol_v, v)}


def magnitude(case):
    """T of the p' expression: what its bound is relative to."""
    seg = owner(case["off"], case["n"])
    lr, wd = case["seg_lr"].double()[seg], case["seg_wd"].double()[seg]
    p, g, v = case["p"].double(), case["g"].double(), case["v"].double()
    gg, gga = g + wd * p, g.abs() + wd * p.abs()
    if case["solver"] == "adam":
        b1, b2, eps = _f32(B1), _f32(B2), _f32(EPS)
        t_m = b1 * case["m"].double().abs() + (1.0 - b1) * gga
        den = (b2 * v + (1.0 - b2) * gg * gg).sqrt() + eps
        return p.abs() + lr * t_m / den
    mu = _f32(MU)
    t_v = mu * v.abs() + lr * gga
    if case["solver"] == "sgd":
        return p.abs() + t_v
    return p.abs() + (1.0 + mu) * t_v + mu * v.abs()


def shadow_expect(case, p_out):
    """{"sh": (want, None)}: bf16 of the p' the route produced where the
    owner trains, the previous shadow content where it is frozen."""
    want = torch.where(trainable(case), bf16(p_out.detach().cpu()),
                       case["sh0"])
    return {"sh": (want, None)}


# -------------------------------------------------- emulation and mutants

def emulate(case, mutant=None):
    """The kernels' arithmetic in fp32, vectorised, every element with its
    owner's parameters.  `mutant` names one deliberate mistake."""
    off, n, solver = case["off"], case["n"], case["solver"]
    nseg = off.numel() - 1
    k = torch.arange(n, dtype=torch.int64)
    seg = owner(off, n)
    pseg = seg                                  # whose parameters are used
    if mutant == "last_table_entry_dropped":
        pseg = seg.clamp_max(MAX_SEG - 2)
    qseg = seg[(k // 4) * 4]                    # owner of the quad's start
    if mutant == "neighbour_params":
        pseg = torch.where(qseg != seg, (seg - 1).clamp_min(0), seg)
    seg_lr, seg_wd = case["seg_lr"], case["seg_wd"]
    if mutant == "no_decay":
        seg_wd = torch.zeros_like(seg_wd)
    if mutant == "unfolded_correction":
        seg_lr = seg_lr / torch.tensor(adam_correction(ADAM_T),
                                       dtype=torch.float32)
    lr, wd = seg_lr[pseg], seg_wd[pseg]
    live = lr != 0
    if mutant == "quad_owner":
        live = (k < off[(qseg + 1).clamp_max(nseg)]) & (seg_lr[qseg] != 0)
    p, g, v = case["p"], case["g"], case["v"]
    late = mutant == "decay_after_lr"           # decay not scaled by lr
    gg = g if late else g + wd * p
    extra = wd * p if late else torch.zeros_like(p)
    out = {}
    if solver in ("sgd", "nesterov"):
        mu = torch.tensor(MU, dtype=torch.float32)
        v1 = mu * v + lr * gg + extra
        if solver == "sgd" or mutant == "plain_momentum":
            p1 = p - v1
        else:
            p1 = p - ((1.0 + mu) * v1 - mu * v)
        frozen_v = {"v": mu * v}
    else:
        b1, b2, eps = (torch.tensor(x, dtype=torch.float32)
                       for x in (B1, B2, EPS))
        m = case["m"]
        m1 = b1 * m + (1.0 - b1) * gg
        v1 = b2 * v + (1.0 - b2) * gg * gg
        den = (v1 + eps).sqrt() if mutant == "eps_inside_sqrt" \
            else v1.sqrt() + eps
        p1 = p - lr * m1 / den - extra
        out["m"] = torch.where(live, m1, m)
        frozen_v = {"v": b2 * v, "m": b1 * m}
    out["p"] = torch.where(live, p1, p)
    out["v"] = torch.where(live, v1, v)
    if mutant == "frozen_touched":
        for name, decayed in frozen_v.items():
            out[name] = torch.where(live, out[name], decayed)
    src = p if mutant == "stale_shadow" else out["p"]
    out["sh"] = torch.where(live, bf16(src), case["sh0"])
    return out


COMMON_MUTANTS = ("quad_owner", "neighbour_params", "frozen_touched",
                  "no_decay", "decay_after_lr", "stale_shadow",
                  "last_table_entry_dropped")
MUTANTS = {
    "sgd": COMMON_MUTANTS,
    "nesterov": COMMON_MUTANTS + ("plain_momentum",),
    "adam": COMMON_MUTANTS + ("eps_inside_sqrt", "unfolded_correction"),
}


def all_violations(case, out):
    """Bound violations of p, v (, m) and of the shadow against the p' that
    `out` itself holds."""
    from _bf16_bounds import violations
    state = {n: t for n, t in out.items() if n != "sh"}
    bad = violations(state, oracle(case))
    if "sh" in out:
        bad += violations({"sh": out["sh"]}, shadow_expect(case, out["p"]))
    return bad


def missed_elements(case, out):
    """Elements `out` left at their initial p where staying there is
    outside the bound (a step below the bound, such as g == 0 and v == 0
    without decay, may round to no step at all)."""
    want, tol = oracle(case)["p"]
    far = (want - case["p"].double()).abs() > tol
    same = (out["p"].detach().cpu() == case["p"]) & far
    return torch.nonzero(same).reshape(-1).tolist()
