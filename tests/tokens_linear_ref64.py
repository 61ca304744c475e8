"""fp64 restatement of gd_tokens_linear (csrc/tokens_linear.hip) with a per-element bound on |kernel - fp64| derived from the kernel's operation
order, the case table and input families the host and GPU tests share, and the mutants the host test shows to break the bound.  u = 2^-24 is fp32's
unit round-off; gamma_n = n u / (1 - n u) bounds a sum of n terms IN ANY ORDER, so the bound knows neither the tile nor how K is split.

linear64 takes `mutant=`: None for the kernel's arithmetic, or the name of one deliberate mistake (MUTANTS)."""
import math

import torch

from rows_ref64 import gamma_n, gen
from rowwise_ref64 import SECOND, U

MUTANTS = ("last_k_chunk_dropped", "one_k_part_dropped", "neighbour_bias", "residual_before_gelu", "accumulate_ignored", "edge_row_repeated",
           "edge_column_skipped")
# the kernel's constants (csrc/tokens_linear.hip): a workgroup owns a TILE_M x TILE_N output (TILE_M = 64 once the grid of 64 x 32 tiles has
# TALL_MIN_WGS workgroups), its WAVES waves take the K_STEP-wide steps of K in turn, PREFETCH steps per pass of a wave's loop (TALL_PREFETCH on the
# tall tiles), and their partial sums meet in MERGES additions
TILE_M, TILE_N, K_STEP, WAVES, PREFETCH, TALL_TILE_M, TALL_PREFETCH, TALL_MIN_WGS = 32, 32, 16, 4, 3, 64, 2, 512
MERGES = WAVES - 1


def _c(M, N, K, bias=True, gelu=False, residual=False, accumulate=False, pads=(0, 0, 0)):
    """pads: elements beyond K in the rows of x and w, beyond N (rounded up to a multiple of 4) in the rows of y."""
    return dict(M=M, N=N, K=K, bias=bias, gelu=gelu, residual=residual, accumulate=accumulate, pads=pads)


# The smallest shapes that straddle those constants.  K: 4 and 12 (one step, one and three live lane groups), 16, 60 / 64 / 68 (four steps with a
# tail, exactly one per wave, a second step for wave 0), 128 (two steps per wave: a pass of the loop that is two thirds full), 388 (25 steps: wave 0
# alone has a seventh, a third pass), 384 (two full passes), 1536 (eight).
# M and N: 1, 31 / 32 / 33, 65 (three row tiles), 130 in rows of 132 (N % 4 != 0: the element-by-element piece), 600.
# The last two go beyond the issue's table: no bias at all, and a grid of 17 x 32 = 544 >= TALL_MIN_WGS tall tiles (bias + residual).
CASES = [
    _c(1, 1, 4),
    _c(9, 36, 12, pads=(4, 0, 0)),
    _c(31, 31, 16),                                                           # ldy 32
    _c(32, 32, 60, pads=(0, 8, 4)),
    _c(33, 33, 64),                                                           # ldy 36
    _c(65, 4, 68, pads=(4, 4, 0)),
    _c(40, 130, 388),                                                         # ldy 132: the flow head and the input transform in one
    _c(128, 96, 384, gelu=True),                                              # fc1
    _c(50, 96, 1536, residual=True, accumulate=True, pads=(0, 0, 8)),         # fc2 of a last block, onto the saved input tokens
    _c(600, 128, 128, gelu=True, residual=True),                              # ffeat_updater at teacher rows
    _c(17, 20, 24, bias=False, pads=(8, 0, 4)),
    _c(1025, 1021, 20, residual=True),                                        # out_proj's form on 64 x 32 tiles
]
IDS = [f"{i}-M{c['M']}-N{c['N']}-K{c['K']}" for i, c in enumerate(CASES)]


def tall_tiles(c):
    """Whether the kernel serves the case on 64 x 32 tiles."""
    return -(-c["M"] // TALL_TILE_M) * -(-c["N"] // TILE_N) >= TALL_MIN_WGS


def inputs(c, seed=0):
    """x [M, K], w [N, K], bias [N], residual [M, N], y0 [M, N] (the accumulate target) or None, on the host.  Families: x and w standard normal, except
    the last min(8, K) columns, which are positive and about 4 in both (the last chunk of K weighs in with products that do not cancel); bias,
    residual and y0 64 x normal, so that a wrong column's bias or a skipped addition moves the result by far more than the accumulation bound."""
    M, N, K = c["M"], c["N"], c["K"]
    g = gen(5000 + 7 * M + 13 * K + 17 * N + seed)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    t = min(8, K)
    x[:, K - t:] = 4.0 + 0.5 * torch.randn(M, t, generator=g).abs()
    w[:, K - t:] = 4.0 + torch.randn(N, t, generator=g).abs()
    big = lambda *s: 64 * torch.randn(*s, generator=g)
    return dict(x=x, w=w, bias=big(N) if c["bias"] else None, residual=big(M, N) if c["residual"] else None, y0=big(M, N) if c["accumulate"] else None)


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def linear64(x, w, bias=None, residual=None, y0=None, gelu=False, accumulate=False, mutant=None, dtype=torch.float64):
    """-> (y, bound) [M, N].  dtype=torch.float32 evaluates the same expression in fp32 (the host test's check that fp32 stays inside the bound).

    The bound, term by term (absacc = sum_k |x_k w_k|):
      accumulation  gamma_(K + MERGES) absacc: K fused multiply-adds (the f32 MFMA is a k-ordered fmaf chain) and the MERGES additions of the four
                    waves' partial sums, in whatever order;
      bias          one addition: u |v|;
      GELU          as rows_ref64.linear64: what v carried passes through |GELU'| <= 1.13, + 4 u |v| + 3 u |g|;
      residual      one addition: u |v|;
      accumulate    one addition: u |v|."""
    xd, wd = x.to(dtype), w.to(dtype)
    M, K = xd.shape
    N = wd.shape[0]
    if mutant == "last_k_chunk_dropped":
        xd = xd.clone()
        xd[:, K - 4:] = 0
    if mutant == "one_k_part_dropped":                                      # wave 1's steps: k in [16 s, 16 s + 16) for s = 1, 5, 9, ...
        xd = xd.clone()
        for s in range(1, -(-K // K_STEP), WAVES):
            xd[:, s * K_STEP:(s + 1) * K_STEP] = 0
    v = xd @ wd.T
    e = gamma_n(K + MERGES) * (xd.abs().double() @ wd.abs().double().T)
    if bias is not None:
        b = bias.to(dtype)
        if mutant == "neighbour_bias":
            b = torch.cat([b[1:], b[N - 2:N - 1]]) if N > 1 else torch.zeros_like(b)
        v = v + b
        e = e + U * v.abs().double()
    r = residual.to(dtype) if residual is not None else None
    if mutant == "residual_before_gelu" and r is not None and gelu:
        v, r = v + r, None
    if gelu:
        gv = _gelu(v)
        e = 1.13 * e + 4 * U * v.abs().double() + 3 * U * gv.abs().double()
        v = gv
    if r is not None:
        v = v + r
        e = e + U * v.abs().double()
    if accumulate and mutant != "accumulate_ignored":
        v = v + y0.to(dtype)
        e = e + U * v.abs().double()
    if mutant == "edge_row_repeated" and M % TILE_M and M > 1:               # the last row of a partial row tile takes its neighbour's result
        v = v.clone()
        v[M - 1] = v[M - 2]
    if mutant == "edge_column_skipped" and N % TILE_N:                       # the last column of a partial column tile keeps what y held
        v = v.clone()
        v[:, N - 1] = y0[:, N - 1].to(dtype) if accumulate else 0
    return v, e * SECOND + 1e-300


def mutant_applies(c, m):
    """Whether mutant m changes anything on case c."""
    steps = -(-c["K"] // K_STEP)
    return {"last_k_chunk_dropped": True, "one_k_part_dropped": steps >= 2, "neighbour_bias": c["bias"], "residual_before_gelu": c["residual"] and c["gelu"],
            "accumulate_ignored": c["accumulate"], "edge_row_repeated": c["M"] % TILE_M != 0 and c["M"] > 1, "edge_column_skipped": c["N"] % TILE_N != 0}[m]
