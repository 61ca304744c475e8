"""fp64 restatement of what csrc/vggt_track.hip computes — the FUSED formulation of the tracker's correlation sampling (integer window, zero mask,
one shared fractional part, the reference's transposed window order, repeated pooling) and of the small kernels around it — with the derived error
bounds the GPU tests hold the kernels to.  tests/test_teacher_tracker_host.py holds this restatement to the layout's correlation class
(tracker_layout.CorrPyramid, the reference's form: full volume + grid_sample) in fp64.

U = 2^-24 is fp32's unit roundoff (half an ulp, relative)."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126


# ----------------------------------------------------------------------------------------------------------------------------------
# pyramid
# ----------------------------------------------------------------------------------------------------------------------------------
def pool2_64(m):
    """m [F, H, W, C] -> fp64 [F, H // 2, W // 2, C]: 2 x 2 mean, stride 2, an odd last row / column dropped."""
    m = m.double()
    H2, W2 = m.shape[1] // 2 * 2, m.shape[2] // 2 * 2
    m = m[:, :H2, :W2]
    return (m[:, 0::2, 0::2] + m[:, 0::2, 1::2] + m[:, 1::2, 0::2] + m[:, 1::2, 1::2]) / 4


def pool2_bound(m):
    """Per output of the fp32 kernel ((a + b) + (c + d)) * 0.25: three roundings, each at most U times a partial sum of |inputs| <= 4 mean|inputs|,
    the quarter exact: |err| <= 3 U mean|inputs|."""
    return 3 * U * pool2_64(m.abs())


def pyramid32(fmap, levels):
    """fmap [F, H, W, C] fp32 -> [levels] fp32 maps, each the fp64 mean of the PREVIOUS fp32 level rounded once (the reference pools repeatedly in fp32)."""
    out = [fmap.float()]
    for _ in range(levels - 1):
        out.append(pool2_64(out[-1]).float())
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# correlation window sampling
# ----------------------------------------------------------------------------------------------------------------------------------
def corr_sample64(pyramid, targets, coords, radius):
    """pyramid: [levels] maps [B * S, H_l, W_l, C]; targets [B, S, N, C]; coords [B, S, N, 2] (level-0 cells) -> (out, A), both fp64
    [B, S, N, levels * (2r+1)^2]: out the fused formulation, A the same blend and mask applied to sum_c |t_c f_c| / sqrt(C)."""
    B, S, N, C = targets.shape
    r, side, win = radius, 2 * radius + 2, 2 * radius + 1
    t = targets.double().reshape(B * S, N, 1, 1, C)
    outs, As = [], []
    k = torch.arange(side)
    f_idx = torch.arange(B * S).view(B * S, 1, 1, 1)
    for l, m in enumerate(pyramid):
        m = m.double()
        H, W = m.shape[1:3]
        xy = coords.double().reshape(B * S, N, 2) / 2 ** l
        x0, y0 = xy[..., 0].floor(), xy[..., 1].floor()
        fx, fy = (xy[..., 0] - x0)[..., None, None], (xy[..., 1] - y0)[..., None, None]
        ix = (x0.long()[..., None] - r + k)[:, :, None, :].expand(B * S, N, side, side)             # [F, N, i (y), j (x)]
        iy = (y0.long()[..., None] - r + k)[:, :, :, None].expand(B * S, N, side, side)
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        cells = m[f_idx, iy.clamp(0, H - 1), ix.clamp(0, W - 1)]                                    # [F, N, side, side, C]
        prod = cells * t
        d = prod.sum(-1) / math.sqrt(C) * inside
        a = prod.abs().sum(-1) / math.sqrt(C) * inside

        def blend(v):
            v = v.transpose(2, 3)                     # [F, N, x index, y index]: entry (a, b) of the window is the sample at (x + a - r, y + b - r)
            return ((1 - fy) * ((1 - fx) * v[:, :, :-1, :-1] + fx * v[:, :, 1:, :-1]) + fy * ((1 - fx) * v[:, :, :-1, 1:] + fx * v[:, :, 1:, 1:])).reshape(B * S, N, win * win)
        outs.append(blend(d))
        As.append(blend(a))
    return torch.cat(outs, -1).view(B, S, N, -1), torch.cat(As, -1).view(B, S, N, -1)


def corr_bound(A, C=128):
    """(C + 8) U A + 2^-126.  The kernel's dot product is 8 fmas per lane and a 4-step tree (12 roundings on the path of any term, against C allowed),
    the 1 / sqrt(C) factor costs 2 (the constant and the product), the blend 5 ((1 - f) twice, a product and a sum per stage): within C + 8."""
    return (C + 8) * U * A + TINY


# ----------------------------------------------------------------------------------------------------------------------------------
# point sampling, position embedding, input assembly
# ----------------------------------------------------------------------------------------------------------------------------------
def _clamped(v, n):
    v = v.double().clamp(0, n - 1)
    v0 = v.floor()
    return v0, (v0 + 1).clamp(max=n - 1), v - v0


def points_bilinear64(fmap, pts):
    """fmap [B, H, W, C] (the sampled frame of every batch entry), pts [B, N, 2] -> (out fp64 [B, N, C], mag: the same blend of |values|)."""
    B, H, W, C = fmap.shape
    m = fmap.double()
    x0, x1, fx = _clamped(pts[..., 0], W)
    y0, y1, fy = _clamped(pts[..., 1], H)
    b = torch.arange(B).view(B, 1)
    fx, fy = fx[..., None], fy[..., None]

    def blend(g):
        return (1 - fy) * ((1 - fx) * g(y0, x0) + fx * g(y0, x1)) + fy * ((1 - fx) * g(y1, x0) + fx * g(y1, x1))
    return blend(lambda y, x: m[b, y.long(), x.long()]), blend(lambda y, x: m[b, y.long(), x.long()].abs())


def trig_bound(arg):
    """|sinf(a32) - sin(a)| with a32 the fp32 product of two fp32 factors, one of them a rounded constant: the argument is off by at most 2 U |a|
    (|sin'| <= 1) and sinf / cosf by two ulp of a value <= 1: 2^-22 |a| + 2^-22 allows twice the first."""
    return 2.0 ** -22 * arg.abs() + 2.0 ** -22


def pos_embed64(pts, H, W, D):
    """pts [M, 2] -> (out fp64 [M, D], bound [M, D]): the sampled position table, and per channel the trig bound blended with the sample's weights
    (nothing more: the blend's own three roundings, at most 3 U of a magnitude <= 1, fit in what the trig bound leaves over the kernel's arithmetic)."""
    q = D // 4
    omega = 1.0 / 10000 ** (torch.arange(q, dtype=torch.float64) / q)
    outs, bounds = [], []
    for comp, n in ((pts[:, 0], W), (pts[:, 1], H)):
        p0, p1, fr = _clamped(comp, n)
        a0, a1, fr = p0[:, None] * omega, p1[:, None] * omega, fr[:, None]
        for fn in (torch.sin, torch.cos):
            outs.append((1 - fr) * fn(a0) + fr * fn(a1))
            bounds.append((1 - fr) * trig_bound(a0) + fr * trig_bound(a1))
    return torch.cat(outs, 1), torch.cat(bounds, 1)


def assemble64(coords, corr, feats, pos, ref_token, max_scale):
    """coords [B, N, S, 2], corr [B, S, N, C], feats [B, N, S, C], pos [B * N, 3C + 4], ref_token [2, 3C + 4] -> (x fp64 [B, N, S, 3C + 4], bound).
    Bound: the trig bound on the embedding channels (argument flow * div, the flow's own rounding U |flow| included in the allowance of 2 U |a|), and on
    every channel 4 ulp of the summed magnitudes of its three terms (two additions, a subtraction and a quotient on the flow channels).  On the
    embedding channels that second term goes beyond the trig rule alone: the kernel's output there is not the sine but the sum sine + position + token,
    two more fp32 additions of terms that are not bounded by 1, whose roundings the trig bound of the first term cannot cover."""
    B, N, S, C = feats.shape
    c = coords.double()
    flow = c - c[:, :, :1]
    div = (torch.arange(0, C // 2, 2, dtype=torch.float32) * (1000.0 / (C // 2))).double()
    emb, eb = [], []
    for comp in (flow[..., 0:1], flow[..., 1:2]):
        a = comp * div
        emb.append(torch.stack([a.sin(), a.cos()], -1).flatten(-2))
        eb.append(torch.stack([trig_bound(a), trig_bound(a)], -1).flatten(-2))
    fl = flow / max_scale
    first = torch.cat(emb + [fl, fl, corr.double().permute(0, 2, 1, 3), feats.double()], -1)
    tb = torch.cat(eb + [torch.zeros_like(first[..., C:])], -1)
    p = pos.double().view(B, N, 1, -1)
    tok = torch.cat([ref_token.double()[:1], ref_token.double()[1:2].expand(S - 1, -1)], 0).view(1, 1, S, -1)
    x = first + p + tok
    return x, tb + 4 * 2.0 ** -23 * (first.abs() + p.abs() + tok.abs())


def nchw_to_cl(fmaps):
    """[B, S, C, H, W] -> [B * S, H, W, C] contiguous."""
    B, S, C, H, W = fmaps.shape
    return fmaps.permute(0, 1, 3, 4, 2).reshape(B * S, H, W, C).contiguous()


def pitched(m, poison=3.0e4):
    """[F, H, W, C] -> [F, H, W + 1, C] with the separator column holding a large finite value: a kernel that reads it shows."""
    F, H, W, C = m.shape
    out = torch.full((F, H, W + 1, C), poison, dtype=m.dtype, device=m.device)
    out[:, :, :W] = m
    return out
