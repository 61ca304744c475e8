"""fp64 restatements of the row kernels (csrc/norm.hip: LayerNorm, L2 norm; csrc/elementwise.hip: tap mean, the refine-conv layout kernels,
clip + AdamW) and the per-element error bounds tests/test_gpu_rowwise_paths.py holds the kernels to.  Plain torch, no autograd in a checked
formula; every function works on whatever device its inputs live on.  A test helper, not a test module.

Notation of the bound derivations: u = 2^-24 (fp32 unit roundoff); an fp32 operation returns the exact result times (1 + d), |d| <= u; a
fused multiply-add rounds once, so counting its product and its sum separately over-counts and stays valid.  First-order bounds carry a
factor (1 + 2^-10) for the dropped second-order terms.  A wave sums a row as: each lane adds its own elements in order (`lane_terms(D)` of
them at most), then wave_sum adds the 64 lane sums in a tree of depth 6 — every element passes through at most lane_terms(D) + 6 additions."""
import math

import torch

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
PREC = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}          # significand bits
EMIN = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}    # exponent of the smallest normal number


def half_ulp(v, dtype):
    """Half the spacing of `dtype` at |v|: the error of ONE round-to-nearest of v, exactly (between 2^-p |v| / 2 and 2^-p |v|; half the subnormal
    spacing below the normal range)."""
    _, e = torch.frexp(v.abs().double())                                   # |v| = m 2^e, m in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype]), torch.clamp(e - 1, min=EMIN[dtype]))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - PREC[dtype])


def f16_sat(v):
    """The library's fp32 -> fp16 store: round to nearest, saturate at +-65504, NaN stays NaN."""
    return v.float().clamp(-65504.0, 65504.0).half()


def lane_terms(D, vec=4):
    """Most elements one lane of a row kernel adds up before the wave reduction: 4 per 256-column slab (the 16-byte bf16 kernels: 8 per 512
    columns — never more than this count plus 4)."""
    return vec * ((D + 64 * vec - 1) // (64 * vec)) + 4


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_stats64(x, eps):
    x = x.double()
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    return mean, var, (var + eps) ** -0.5


def ln_fwd64(x, gamma, beta, eps):
    """-> (y, mean, rstd) in fp64; var is the biased one (nn.LayerNorm)."""
    mean, _, rstd = ln_stats64(x, eps)
    y = (x.double() - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()
    return y, mean, rstd


def ln_fwd_bound(x, gamma, beta, eps, out_dtype):
    """-> (by [M, D], bmean [M], brstd [M]): bounds on |kernel - fp64| for y (AFTER its store in out_dtype; for fp16 compare against the
    reference clamped to +-65504), mean and rstd.

    mean = wave_sum(x) / D: (lane_terms + 6) additions and one division -> e_mu = (lane_terms + 7) u mean|x|.
    var: with m the exact mean, sum (x - mu)^2 = sum (x - m)^2 + D (mu - m)^2 exactly, so the mean's error enters squared; each term costs a
    subtraction (relative 2 u after squaring) and a product, the sum lane_terms + 6 additions, then / D and + eps: relative
    (lane_terms + 11) u + e_mu^2 / (var + eps).  rstd = rsqrtf(.) halves that and adds the instruction's own 1 ulp = 2 u.
    y = ((x - mu) rstd) gamma + beta.  d = x - mu carries e_mu + u |d|; with t = d rstd gamma the two products add 2 u |t|, rstd its own
    relative error, and the final sum u (|t| + |beta|):
        |dy| <= |gamma| rstd e_mu + |t| (d_rstd + 3 u) + u (|t| + |beta|)
    The first term is the conditioning term: rstd e_mu ~ (lane_terms + 7) u (1 + |mean| / std), an fp32 mean is only good to ~u |mean|.
    A store narrower than fp32 adds one rounding of the stored value (half_ulp)."""
    xd, g, b = x.double(), gamma.double(), beta.double()
    D = xd.shape[-1]
    mean, var, rstd = ln_stats64(xd, eps)
    n = lane_terms(D)
    e_mu = (n + 7) * U * xd.abs().mean(-1)
    rel_var = (n + 11) * U + e_mu ** 2 / (var + eps)
    d_rs = 0.5 * rel_var + 2 * U
    t = (xd - mean[:, None]) * rstd[:, None] * g
    by = (g.abs() * (rstd * e_mu)[:, None] + t.abs() * (d_rs[:, None] + 3 * U) + U * (t.abs() + b.abs())) * SECOND
    if out_dtype != torch.float32:
        by = by + half_ulp((t + b).abs() + by, out_dtype)
    return by, e_mu * SECOND, rstd * d_rs * SECOND


def ln_bwd64(dy, x, gamma, eps, dyscale=1.0, dres=None, dres2=None):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)) + dres + dres2,  g = dy dyscale gamma — the closed form of the kernel's comment, statistics
    recomputed in fp64."""
    mean, _, rstd = ln_stats64(x, eps)
    xh = (x.double() - mean[:, None]) * rstd[:, None]
    g = dy.double() * dyscale * gamma.double()
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    for r in (dres, dres2):
        if r is not None:
            dx = dx + r.double()
    return dx


def ln_bwd_bound(dy, x, gamma, eps, dyscale, dres, dres2, out_dtype, mean_err=U, rstd_err=U):
    """Bound on |kernel dx - ln_bwd64| per element, for a kernel handed mean / rstd with relative errors mean_err / rstd_err (fp64 statistics
    rounded to fp32: u each).

    xhat = (x - mu) rstd:  e_xh = rstd (mean_err |mu| + u |d|) + |xhat| (rstd_err + u)       (again the conditioning term, through mu)
    g = dy dyscale gamma (and the device-side dy scale): 3 u |g|
    s1 = wave_sum(g) / D:       e1 = (lane_terms + 10) u mean|g|
    s2 = wave_sum(g xhat) / D:  e2 = mean(|g| e_xh) + (lane_terms + 11) u mean|g xhat|
    inner = g - s1 - xhat s2:   3 u |g| + e1 + e_xh |s2| + |xhat| e2 + u |xhat s2| + 2 u (|g| + |s1| + |xhat s2|)
    dx = rstd inner:            rstd times that, + (rstd_err + u) |rstd inner|
    each residual added:        u times the running magnitude;  a narrower store: half_ulp.
    Every term scales with |g|, not with |dx|: where g is parallel to xhat, dx cancels to zero and the bound does not."""
    xd = x.double()
    D = xd.shape[-1]
    mean, _, rstd = ln_stats64(xd, eps)
    rs = rstd[:, None]
    d = xd - mean[:, None]
    xh = d * rs
    g = dy.double() * dyscale * gamma.double()
    n = lane_terms(D)
    e_xh = rs * (mean_err * mean.abs()[:, None] + U * d.abs()) + xh.abs() * (rstd_err + U)
    s1 = g.mean(-1, keepdim=True)
    s2 = (g * xh).mean(-1, keepdim=True)
    e1 = (n + 10) * U * g.abs().mean(-1, keepdim=True)
    e2 = (g.abs() * e_xh).mean(-1, keepdim=True) + (n + 11) * U * (g * xh).abs().mean(-1, keepdim=True)
    inner = g - s1 - xh * s2
    e_in = 3 * U * g.abs() + e1 + e_xh * s2.abs() + xh.abs() * e2 + U * (xh * s2).abs() + 2 * U * (g.abs() + s1.abs() + (xh * s2).abs())
    dx = rs * inner
    run = dx.abs()
    b = rs * e_in + (rstd_err + U) * run
    for r in (dres, dres2):
        if r is not None:
            dx = dx + r.double()
            run = run + r.double().abs()
            b = b + U * run
    b = b * SECOND
    if out_dtype != torch.float32:
        b = b + half_ulp(dx.abs() + b, out_dtype)      # one rounding of the value actually stored
    return b


# ------------------------------------------------------------------------------------------------ L2 norm
def l2_fwd64(x, eps):
    """-> (y, inv): y = x / max(||x||, eps), inv = 1 / max(||x||, eps)  (F.normalize)."""
    xd = x.double()
    inv = 1.0 / torch.clamp(xd.norm(dim=-1), min=eps)
    return xd * inv[:, None], inv


def l2_bwd64(y, dy, inv):
    """dx = (dy - y (y . dy)) inv, from the forward's stored y and inv (the kernel's inputs)."""
    y, dy = y.double(), dy.double()
    return (dy - y * (y * dy).sum(-1, keepdim=True)) * inv.double()[:, None]


def l2_inv_rel_bound(D, vec=1):
    """Relative bound on inv = 1 / max(sqrt(sum x^2), eps): the sum of squares is positive, so its relative error is one product plus
    per_lane + 6 additions; sqrtf (correctly rounded) halves it and adds u, the clamp is 1-Lipschitz, the division adds u."""
    per_lane = vec * ((D + 64 * vec - 1) // (64 * vec))
    return (0.5 * (per_lane + 7) + 2) * U * SECOND


def l2_fwd_bound(x, eps):
    """-> (by, binv): y = x inv costs one more product."""
    y, inv = l2_fwd64(x, eps)
    r = l2_inv_rel_bound(x.shape[-1])
    return y.abs() * (r + U * SECOND), inv * r


def l2_bwd_bound(y, dy, inv):
    """s = wave_sum(y dy): (per_lane + 7) u sum|y dy|;  dx = (dy - y s) inv: e_s |y| + 3 u (|dy| + |y s|), all times inv."""
    y, dy = y.double(), dy.double()
    D = y.shape[-1]
    per_lane = (D + 63) // 64
    e_s = (per_lane + 7) * U * (y * dy).abs().sum(-1, keepdim=True)
    s = (y * dy).sum(-1, keepdim=True)
    return (e_s * y.abs() + 3 * U * (dy.abs() + (y * s).abs())) * inv.double().abs()[:, None] * SECOND


# ------------------------------------------------------------------------------------------------ tap mean
def tap_mean64(grids, prefix):
    """mean of the taps [B, prefix + hw, D] with the prefix rows dropped -> [B, hw, D] fp64."""
    return sum(g.double()[:, prefix:] for g in grids) / len(grids)


def tap_mean_bound(grids, prefix, out_dtype):
    """ngrid u of the sum of the taps' absolute values (the kernel adds the ngrid taps in order and multiplies by fl(1 / ngrid): ngrid - 1
    additions, the constant's rounding and the product, each at most u of the running sum), plus one rounding of the stored type."""
    n = len(grids)
    sa = sum(g.double()[:, prefix:].abs() for g in grids)
    b = n * U * sa
    return b + half_ulp(tap_mean64(grids, prefix).abs() + b, out_dtype)


def tap_mean_bwd64(dout, ngrid, prefix):
    """every tap's gradient: dout / ngrid under `prefix` zero rows -> [B, prefix + hw, D] fp64."""
    B, hw, D = dout.shape
    dg = torch.zeros(B, prefix + hw, D, dtype=torch.float64, device=dout.device)
    dg[:, prefix:] = dout.double() / ngrid
    return dg


def tap_mean_bwd_bound(dout, ngrid, prefix, dtype):
    """dout fl(1 / ngrid), rounded once to the tap dtype.  A power-of-two ngrid only moves the exponent: the bound is ZERO (bit equality, in
    both dtypes).  Otherwise (ngrid = 3): u |v| for the constant, u |v| for the fp32 product, and the store's rounding."""
    v = tap_mean_bwd64(dout, ngrid, prefix).abs()
    if ngrid & (ngrid - 1) == 0:
        return torch.zeros_like(v)
    b = 2 * U * v
    return b + half_ulp(v + b, dtype) * (v > 0)


# ------------------------------------------------------------------------------------------------ refine-conv layout kernels (index only)
def grid_of(src, B, gh, gw, D, prefix=None):
    """The [B, gh, gw, D] grid a layout kernel reads: from tokens [B, prefix + gh gw, D] (prefix given) or a pitched grid [B, gh, gw + 1, D]."""
    if prefix is not None:
        return src[:, prefix:].reshape(B, gh, gw, D)
    return src.reshape(B, gh, gw + 1, D)[:, :, :gw]


def stack3_rows_ref(grid, dtype):
    """gd_stack3_rows: buf [B gh (gw + 1) + 2, 3 D].  Row R = r + 1 (one zero guard row in front, one behind) holds, for the pitched position
    r = (b, y, x) with x in [0, gw], the slots (grid[b, y - 1, x], grid[b, y, x], grid[b, y + 1, x]); zeros outside the image and in the
    separator column x == gw."""
    B, gh, gw, D = grid.shape
    pad = torch.zeros(B, gh + 2, gw + 1, D, dtype=dtype, device=grid.device)
    pad[:, 1:gh + 1, :gw] = grid.to(dtype)
    body = torch.stack([pad[:, s:s + gh] for s in range(3)], dim=3).reshape(B * gh * (gw + 1), 3 * D)
    z = torch.zeros(1, 3 * D, dtype=dtype, device=grid.device)
    return torch.cat([z, body, z], 0)


def unpitch_tokens_ref(src, B, gh, gw, D, prefix):
    """gd_unpitch_tokens: pitched [B, gh, gw + 1, D] -> [B, prefix + gh gw, D], prefix rows zero, separator column dropped."""
    out = torch.zeros(B, prefix + gh * gw, D, dtype=src.dtype, device=src.device)
    out[:, prefix:] = src.reshape(B, gh, gw + 1, D)[:, :, :gw].reshape(B, gh * gw, D)
    return out


def conv_weight_pack_ref(w, dtype):
    """ops.conv_weight_pack of W[n, c, ky, kx]: wk[n, (ky, kx, c)];  wt[c, (kx', ky', n)] = W[n, c, 2 - ky', 2 - kx'];  wu = wk^T."""
    D = w.shape[0]
    wk = w.permute(0, 2, 3, 1).reshape(D, 9 * D)
    wt = w.flip(2, 3).permute(1, 3, 2, 0).reshape(D, 9 * D)
    return wk.to(dtype).contiguous(), wt.to(dtype).contiguous(), wk.t().to(dtype).contiguous()


def stacked_view_weight(w):
    """The weight the overlapping-row view of a stack3 buffer multiplies: K order (kx, ky, c) -> [n, 9 D]."""
    return w.permute(0, 3, 2, 1).reshape(w.shape[0], -1)


def im2col3x3_ref(grid):
    """gd_im2col3x3: col[(b, y, x), (ky, kx, c)] = grid[b, y + ky - 1, x + kx - 1, c], zero outside."""
    B, gh, gw, D = grid.shape
    pad = torch.zeros(B, gh + 2, gw + 2, D, dtype=grid.dtype, device=grid.device)
    pad[:, 1:gh + 1, 1:gw + 1] = grid
    taps = [pad[:, ky:ky + gh, kx:kx + gw] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, dim=3).reshape(B * gh * gw, 9 * D)


def col2im3x3_ref(dcol, B, gh, gw, D):
    """gd_col2im3x3 (the adjoint): dx[b, y, x, c] = sum_taps dcol[(b, y - ky + 1, x - kx + 1), (ky, kx, c)] -> [B, gh, gw, D] fp64."""
    dc = dcol.double().reshape(B, gh, gw, 3, 3, D)
    pad = torch.zeros(B, gh + 2, gw + 2, D, dtype=torch.float64, device=dcol.device)
    for ky in range(3):
        for kx in range(3):
            pad[:, ky:ky + gh, kx:kx + gw] += dc[:, :, :, ky, kx]
    return pad[:, 1:gh + 1, 1:gw + 1]


# ------------------------------------------------------------------------------------------------ clip + AdamW
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def adamw64(p, g, m, v, step, lr=1e-5, wd=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, grad_scale=1.0, ranges=None):
    """Global-norm clip + AdamW of gd_clip_adamw_step / _ranges in fp64 -> (p, m, v, norm), new tensors.  The hyper-parameters are the fp32
    values the C ABI receives.  norm = ||g|| grad_scale over the WHOLE buffer; coef = min(max_norm / (norm + 1e-6), 1) (1 when
    max_norm <= 0) times grad_scale; the update touches only `ranges` [(a, b), ...] (everything when None)."""
    lr, wd, b1, b2, eps, max_norm, gs = (_f32(t) for t in (lr, wd, betas[0], betas[1], eps, max_norm, grad_scale))
    p, g, m, v = (t.double().clone() for t in (p, g, m, v))
    norm = g.pow(2).sum().sqrt() * gs
    coef = (min(max_norm / (float(norm) + _f32(1e-6)), 1.0) if max_norm > 0 else 1.0) * gs
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    for a, b in (ranges or [(0, p.numel())]):
        gi = g[a:b] * coef
        m[a:b] = b1 * m[a:b] + (1 - b1) * gi
        v[a:b] = b2 * v[a:b] + (1 - b2) * gi * gi
        p[a:b] = p[a:b] * (1 - lr * wd) - (lr / bc1) * m[a:b] / (v[a:b].sqrt() / math.sqrt(bc2) + eps)
    return p, m, v, norm


def adamw_bound(p, g, m, v, step, lr=1e-5, wd=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, grad_scale=1.0):
    """-> (bdp, bm, bv, bnorm_rel): bounds on |kernel - adamw64| for the update p_new - p_old, the moments, and the norm (relative), per
    element, from adamw_kernel's fp32 operations.

    norm = (float) sqrt(sum in fp64) * grad_scale: 2 u.  coef: exactly grad_scale when the clip is inactive or off, else + 1e-6, the
    division, the product: d_coef = 5 u.  gi = g coef: d_coef + u.
    m' = b1 m + (1 - b1) gi:    bm = 2 u |b1 m| + (d_coef + 3 u) |(1 - b1) gi|
    v' = b2 v + (1 - b2) gi^2:  bv = 2 u b2 v + (2 d_coef + 5 u) (1 - b2) gi^2
    Bias corrections, on the host in fp32: bc = 1 - powf(b, step).  The subtraction is exact (Sterbenz); powf is exact at step 1 and within
    1 ulp = 2 u otherwise, which the cancellation magnifies: d_bc = 2 u b^step / (1 - b^step) — 500 u for b2 at step 2.
    upd = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps):
        numerator:   (lr / bc1) bm + |lr / bc1 m'| (d_bc1 + 2 u)
        denominator: relative bv / (2 v') + d_bc2 / 2 + 4 u      (two square roots, the division, + eps; every term positive)
        |d upd| <= numerator / den + |upd| (denominator + u)
    p' = p (1 - lr wd) - upd: 1 - lr wd, the product and the difference round at u |p| each — the only terms that scale with |p| (the
    stored parameter cannot be better than its own half ulp); the rest is relative to |upd| <= lr.
        bdp = 3 u |p| + u |upd| + |d upd|"""
    lr, wd, b1, b2, eps, max_norm, gs = (_f32(t) for t in (lr, wd, betas[0], betas[1], eps, max_norm, grad_scale))
    p, g, m, v = (t.double() for t in (p, g, m, v))
    norm = float(g.pow(2).sum().sqrt()) * gs
    active = max_norm > 0 and max_norm / (norm + 1e-6) < 1.0
    d_coef = 5 * U if active else 0.0
    coef = (min(max_norm / (norm + _f32(1e-6)), 1.0) if max_norm > 0 else 1.0) * gs
    gi = g * coef
    m1 = b1 * m + (1 - b1) * gi
    v1 = b2 * v + (1 - b2) * gi * gi
    bm = 2 * U * (b1 * m).abs() + (d_coef + 3 * U) * ((1 - b1) * gi).abs()
    bv = 2 * U * b2 * v + (2 * d_coef + 5 * U) * (1 - b2) * gi * gi
    pw = 0.0 if step == 1 else 2 * U
    d_bc1 = pw * b1 ** step / (1 - b1 ** step)
    d_bc2 = pw * b2 ** step / (1 - b2 ** step)
    A = lr / (1 - b1 ** step)
    den = v1.sqrt() / math.sqrt(1 - b2 ** step) + eps
    upd = A * m1 / den
    rel_den = bv / (2 * v1).clamp_min(1e-300) + 0.5 * d_bc2 + 4 * U
    d_upd = (A * bm + (A * m1).abs() * (d_bc1 + 2 * U)) / den + upd.abs() * (rel_den + U)
    bdp = (3 * U * p.abs() + U * upd.abs() + d_upd) * SECOND
    return bdp, bm * SECOND, bv * SECOND, 2 * U * SECOND
