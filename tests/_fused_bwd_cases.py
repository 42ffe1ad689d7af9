"""Cases, float64 oracles, CPU emulations and mutants for the two fused
backward kernels: relu_db_dense (ReLU' + bias gradient in one pass) and
maxpool_bwd8_relu_db (max-pool backward + ReLU mask + bias gradient).
Shared by test_fused_bwd_bounds.py (CPU) and test_fused_bwd_gpu.py (GPU);
the pooling and ReLU pieces come from _bf16_bounds.py.

Bounds (u = 2^-8, e = 2^-24, see _bf16_bounds.py for B1..B3):

 ReLU + db   dx as _relu_bound; db as relu_fused_oracle:
             (m+2)e(|db0| + sum|dx|), m = rows.  The kernel sums the fp32 g
             the dx rounding sees, in any grouping (registers, LDS, one
             atomic per block), which B3 covers.
 pool+ReLU   dx = sum of the dy routed to the pixel by first-maximum
             argmax, over the windows whose pooled output is > 0; every
             such window has top == y[pixel], so that is (y > 0) * routed
             sum.  tol_dx = (u + kh*kw*e) * sum|routed dy| on the pixels
             with y > 0 and exactly 0 elsewhere (masked pixels and pixels
             no window covers are stored as 0).
             db sums the ROUNDED dx (what a separate column sum would
             read): against db0 + sum(exact dx) that is
             sum(tol_dx) + (m+2)e(|db0| + sum|dx|), m = N*H*W.
"""

import torch

import _bf16_bounds as B

FORCED_BLOCKS = (1, 2, 3)

# rows x C: three octets; fewer rows than row groups; odd row count and
# more than one unrolled trip; 2-D wide (column strips on grid.x)
RELU_DB_SHAPES = [(37, 24), (5, 384), (1001, 96), (3, 4096)]
RELU_DB_SLOPES = (0.0, 0.25)

POOL_GEOMS = [B.POOL_GEOMS[0], B.POOL_GEOMS[1], B.POOL_GEOMS[4]]
assert POOL_GEOMS[0] == (12, 12, (3, 3), (2, 2), (0, 0))
assert POOL_GEOMS[1] == (7, 7, (3, 3), (1, 1), (1, 1))
assert POOL_GEOMS[2] == (11, 11, (2, 2), (3, 3), (0, 0))
POOL_CS = (8, 24, 48)
POOL_CASES = [(c, g) for g in POOL_GEOMS for c in POOL_CS]
# must decline the fused route: scalar pooling kernels, int32 argmax
POOL_DECLINE_CASES = [(20, POOL_GEOMS[0]),
                      (8, (12, 12, (12, 12), (1, 1), (0, 0)))]


def case_id(case):
    c, (h, w, k, s, p) = case
    return f"C{c}-{h}x{w}-k{k[0]}s{s[0]}p{p[0]}"


# ------------------------------------------------------------- ReLU + db

def relu_db_inputs(rows, c, seed):
    g = B.gen(seed)
    return dict(y=B.bf16(torch.randn(rows, c, generator=g)),
                dy=B.bf16(torch.randn(rows, c, generator=g)),
                db0=torch.randn(c, generator=g) * 3 + 1)


def two_level_sum(vals, db0, nblocks, seed):
    """fp32 column sums of vals [m, C] as the kernels form them: each of
    nblocks blocks sums its rows (grid-stride: rows b, b+nblocks, ...) in
    fp32, then the block partials land on db0 in a shuffled (atomic)
    order."""
    parts = [vals[b::nblocks].float().sum(dim=0, dtype=torch.float32)
             for b in range(nblocks)]
    order = torch.randperm(nblocks, generator=B.gen(seed)).tolist()
    db = db0.float().clone()
    for b in order:
        db = db + parts[b]
    return db


def relu_db_emulate(inp, slope, nblocks=3, seed=0, mask="y",
                    db_unmasked=False):
    y, dy = inp["y"].float(), inp["dy"].float()
    sl = torch.tensor(slope, dtype=torch.float32)
    if mask == "y":
        keep = y > 0
    elif mask == "none":
        keep = torch.ones_like(y, dtype=torch.bool)
    else:                                   # "dy": sign of the gradient
        keep = dy > 0
    g = torch.where(keep, dy, dy * sl)
    return {"dx": B.bf16(g),
            "db": two_level_sum(dy if db_unmasked else g, inp["db0"],
                                nblocks, seed)}


def relu_db_oracle(inp, slope):
    return B.relu_fused_oracle(inp["y"], inp["dy"], inp["db0"], slope)


RELU_DB_MUTANTS = {
    "mask_ignored": lambda i, s: relu_db_emulate(i, s, mask="none"),
    "mask_from_dy": lambda i, s: relu_db_emulate(i, s, mask="dy"),
    "db_unmasked": lambda i, s: relu_db_emulate(i, s, db_unmasked=True),
}


# ------------------------------------------------------ pool + ReLU + db

def pool_relu_inputs(c, geom, seed, n=2):
    """x is the conv's rectified output: relu(multiples of 0.5 in [-2, 2]),
    so 5/9 of it is exactly 0 (windows whose maximum is 0) and positive
    ties are common."""
    h, w, k, s, p = geom
    g = B.gen(seed)
    x = torch.relu(torch.randint(-4, 5, (n, c, h, w), generator=g).float()
                   * 0.5)
    po, qo = B.pool_out(h, k[0], s[0], p[0]), B.pool_out(w, k[1], s[1], p[1])
    dy = torch.randn(n, c, po, qo, generator=g)
    return dict(x=B.bf16(x), dy=B.bf16(dy), kernel=k, stride=s, pad=p,
                db0=torch.randn(c, generator=g) * 3 + 1)


def _argmax_first(inp, dtype):
    x = inp["x"].to(dtype)
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    po, qo = inp["dy"].shape[2], inp["dy"].shape[3]
    win = B._windows(x, k, s, p, po, qo, float("-inf"))
    rs = torch.argmax(win, dim=2)
    top = win.gather(2, rs.unsqueeze(2)).squeeze(2)      # [N, C, P*Q]
    return rs, top.reshape(x.shape[0], x.shape[1], po, qo)


def pool_data_facts(inp):
    """(windows whose maximum is exactly 0 with a non-zero dy,
        pixels that are the argmax of two or more windows)."""
    rs, top = _argmax_first(inp, torch.float64)
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    zero_win = int(((top == 0) & (inp["dy"].double() != 0)).sum())
    hits = B._route(rs, torch.ones_like(inp["dy"].double()),
                    inp["x"].shape, k, s, p)
    return zero_win, int((hits >= 2).sum())


def uncovered(inp):
    """Pixels no window holds (stride > kernel, or past the last window)."""
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    n, c, h, w = inp["x"].shape
    po, qo = inp["dy"].shape[2], inp["dy"].shape[3]
    cov = torch.zeros(h, w, dtype=torch.bool)
    for pi in range(po):
        for qi in range(qo):
            h0, w0 = pi * s[0] - p[0], qi * s[1] - p[1]
            cov[max(h0, 0):min(h0 + k[0], h),
                max(w0, 0):min(w0 + k[1], w)] = True
    return ~cov


def pool_relu_oracle(inp):
    x, dy = inp["x"].double(), inp["dy"].double()
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    rs, _ = _argmax_first(inp, torch.float64)
    keep = (x > 0).double()
    dx = B._route(rs, dy, x.shape, k, s, p) * keep
    t = B._route(rs, dy.abs(), x.shape, k, s, p) * keep
    tol_dx = (B.U + k[0] * k[1] * B.E32) * t
    m = x.numel() // x.shape[1]
    db0 = inp["db0"].double()
    db = db0 + dx.sum(dim=(0, 2, 3))
    tol_db = tol_dx.sum(dim=(0, 2, 3)) + (m + 2) * B.E32 * (
        db0.abs() + dx.abs().sum(dim=(0, 2, 3)))
    return {"dx": (dx, tol_dx), "db": (db, tol_db)}


def pool_relu_emulate(inp, nblocks=3, seed=0, mask="top", db_unmasked=False,
                      tie_last=False):
    """The kernel's arithmetic: first-maximum argmax (strict >), fp32 sum
    of the routed dy over the windows with top > 0, one bf16 rounding, db
    from the rounded values in a two-level order."""
    k, s, p = inp["kernel"], inp["stride"], inp["pad"]
    x, dy = inp["x"].float(), inp["dy"].float()
    n, c, h, w = x.shape
    po, qo = dy.shape[2], dy.shape[3]
    win = B._windows(x, k, s, p, po, qo, float("-inf"))
    best = torch.full((n, c, po * qo), -3.4e38)
    brs = torch.zeros((n, c, po * qo), dtype=torch.long)
    for t in range(k[0] * k[1]):
        v = win[:, :, t]
        upd = (v >= best) if tie_last else (v > best)
        upd &= torch.isfinite(v)
        best = torch.where(upd, v, best)
        brs = torch.where(upd, torch.full_like(brs, t), brs)
    top = best.reshape(n, c, po, qo)
    plain = B._route(brs, dy, x.shape, k, s, p)
    if mask == "top":
        g = B._route(brs, dy * (top > 0).float(), x.shape, k, s, p)
    elif mask == "none":
        g = plain
    else:                                   # "dy": sign of the pixel's sum
        g = plain * (plain > 0).float()
    dx = B.bf16(g)
    src = B.bf16(plain) if db_unmasked else dx
    rows = src.float().permute(0, 2, 3, 1).reshape(-1, c)
    return {"dx": dx, "db": two_level_sum(rows, inp["db0"], nblocks, seed)}


POOL_RELU_MUTANTS = {
    "mask_ignored": lambda i: pool_relu_emulate(i, mask="none"),
    "mask_from_dy": lambda i: pool_relu_emulate(i, mask="dy"),
    "db_unmasked": lambda i: pool_relu_emulate(i, db_unmasked=True),
    "tie_last": lambda i: pool_relu_emulate(i, tie_last=True),
}
