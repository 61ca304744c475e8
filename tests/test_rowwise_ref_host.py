"""CPU checks of tests/rowwise_ref64.py: the fp64 restatements the GPU row-kernel tests compare against are themselves held to torch's own
operators (fp64, autograd or direct calls) and to the oracle's clip + AdamW; the bound functions are held to a plain fp32 evaluation of the
same formulas (a bound an fp32 torch evaluation already breaks would be a wrong derivation, not a kernel bug)."""
import pytest
import torch
import torch.nn.functional as F

import gd_oracle as O
import rowwise_ref64 as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("M,D", [(1, 4), (5, 260), (3, 2048)])
def test_layernorm_refs_match_torch_autograd(M, D):
    g = _gen(1)
    x = torch.randn(M, D, generator=g, dtype=torch.float64) * 2 + 3
    gm, bt = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    dy, r1, r2 = (torch.randn(M, D, generator=g, dtype=torch.float64) for _ in range(3))
    y, mean, rstd = R.ln_fwd64(x, gm, bt, 1e-6)
    xr = x.clone().requires_grad_(True)
    yr = F.layer_norm(xr, (D,), gm, bt, 1e-6)
    assert torch.allclose(y, yr, rtol=1e-12, atol=1e-12)
    assert torch.allclose(mean, x.mean(-1), rtol=1e-13, atol=0) and torch.allclose(rstd, (x.var(-1, unbiased=False) + 1e-6).rsqrt(), rtol=1e-12, atol=0)
    yr.backward(dy * 0.25)
    assert torch.allclose(R.ln_bwd64(dy, x, gm, 1e-6, 0.25, r1, r2), xr.grad + r1 + r2, rtol=1e-10, atol=1e-11)
    assert torch.allclose(R.ln_bwd64(dy, x, gm, 1e-6, 0.25), xr.grad, rtol=1e-10, atol=1e-11)


@pytest.mark.parametrize("M,D", [(1, 1), (5, 65), (2, 200)])
def test_l2_refs_match_normalize(M, D):
    g = _gen(2)
    x = torch.randn(M, D, generator=g, dtype=torch.float64)
    x[0] = 0.0
    w = torch.randn(M, D, generator=g, dtype=torch.float64)
    y, inv = R.l2_fwd64(x, 1e-12)
    xr = x.clone().requires_grad_(True)
    yr = F.normalize(xr, dim=-1, eps=1e-12)
    assert torch.allclose(y, yr, rtol=1e-13, atol=0) and float(inv[0]) == 1e12
    (yr * w).sum().backward()
    # the zero row: autograd of the clamp gives dy / eps; the closed form gives (dy - 0) inv, the same
    assert torch.allclose(R.l2_bwd64(y, w, inv), xr.grad, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("ng,prefix", [(1, 0), (3, 5), (4, 1)])
def test_tap_mean_refs_match_autograd(ng, prefix):
    g = _gen(3)
    taps = [torch.randn(2, prefix + 7, 8, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(ng)]
    out = R.tap_mean64([t.detach() for t in taps], prefix)
    ref = torch.stack([t[:, prefix:] for t in taps]).mean(0)
    assert torch.allclose(out, ref, rtol=1e-14, atol=0)
    dout = torch.randn(2, 7, 8, generator=g, dtype=torch.float64)
    (ref * dout).sum().backward()
    dg = R.tap_mean_bwd64(dout, ng, prefix)
    for t in taps:
        assert torch.allclose(dg, t.grad, rtol=1e-14, atol=0)
    assert prefix == 0 or float(dg[:, :prefix].abs().max()) == 0.0


@pytest.mark.parametrize("B,gh,gw,D", [(1, 1, 1, 8), (2, 1, 4, 8), (1, 3, 1, 8), (3, 5, 7, 16)])
def test_layout_refs_match_conv2d_and_unfold(B, gh, gw, D):
    g = _gen(4)
    grid = torch.randint(-8, 9, (B, gh, gw, D), generator=g).double()
    w = torch.randint(-4, 5, (D, D, 3, 3), generator=g).double()
    x = grid.permute(0, 3, 1, 2).clone().requires_grad_(True)
    conv = F.conv2d(x, w, padding=1)                                                                     # [B, n, gh, gw]
    want = conv.detach().permute(0, 2, 3, 1).reshape(B * gh * gw, D)
    # im2col + wk
    col = R.im2col3x3_ref(grid)
    unf = F.unfold(grid.permute(0, 3, 1, 2), 3, padding=1)                                                # [B, (c, ky, kx), L]
    assert torch.equal(col.view(B, gh * gw, 9, D), unf.view(B, D, 9, gh * gw).permute(0, 3, 2, 1))
    wk, wt, wu = R.conv_weight_pack_ref(w, torch.float64)
    assert torch.equal(col @ wk.t(), want) and torch.equal(wu, wk.t())
    # the stacked buffer's overlapping-row view against the (kx, ky, c) weight: the conv on the pitched grid
    buf = R.stack3_rows_ref(grid, torch.float64)
    rows, pitch = B * gh * (gw + 1), gw + 1
    view = torch.as_strided(buf, (rows, 9 * D), (3 * D, 1))
    out = (view @ R.stacked_view_weight(w).t()).view(B, gh, pitch, D)
    assert torch.equal(out[:, :, :gw].reshape(-1, D), want)
    assert float(buf[0].abs().max()) == 0.0 and float(buf[-1].abs().max()) == 0.0
    assert float(buf[1:-1].view(B, gh, pitch, 3 * D)[:, :, gw].abs().max()) == 0.0
    # the transposed conv: the same view of a stacked dY (separator column zero) against wt, then unpitch = autograd's input gradient
    dy = torch.randint(-4, 5, (B, gh, gw, D), generator=g).double()
    conv.backward(dy.permute(0, 3, 1, 2))
    dyp = torch.zeros(B, gh, pitch, D, dtype=torch.float64)
    dyp[:, :, :gw] = dy
    sview = torch.as_strided(R.stack3_rows_ref(R.grid_of(dyp, B, gh, gw, D), torch.float64), (rows, 9 * D), (3 * D, 1))
    dx = R.unpitch_tokens_ref(sview @ wt.t(), B, gh, gw, D, 2)
    assert torch.equal(dx[:, 2:].reshape(B, gh, gw, D), x.grad.permute(0, 2, 3, 1)) and float(dx[:, :2].abs().max()) == 0.0
    # col2im = F.fold of the (c, ky, kx)-ordered columns
    dcol = torch.randint(-4, 5, (B * gh * gw, 9 * D), generator=g).double()
    fold = F.fold(dcol.view(B, gh * gw, 9, D).permute(0, 3, 2, 1).reshape(B, D * 9, gh * gw), (gh, gw), 3, padding=1)
    assert torch.equal(R.col2im3x3_ref(dcol, B, gh, gw, D), fold.permute(0, 2, 3, 1))


@pytest.mark.parametrize("max_norm,gmag", [(1.0, 1.0), (1.0, 1e-4), (0.0, 1.0)])
def test_adamw_ref_matches_the_oracle(max_norm, gmag):
    g = _gen(5)
    n = 257
    p = torch.randn(n, generator=g, dtype=torch.float64) * 0.02
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    po, st = p.clone(), [(m.clone(), v.clone())]
    hp = dict(lr=R._f32(1e-5), wd=R._f32(1e-4), betas=(R._f32(0.9), R._f32(0.999)), eps=R._f32(1e-8))
    for step in (1, 2, 3):
        gr = torch.randn(n, generator=g, dtype=torch.float64) * gmag
        p, m, v, norm = R.adamw64(p, gr * 2.0, m, v, step, max_norm=max_norm, grad_scale=0.5)
        if max_norm > 0:
            rn = O.clip_and_adamw([po], [gr], st, step, max_norm=max_norm, **hp)
            assert abs(float(norm) - float(rn)) < 1e-6 * float(rn)          # (the oracle returns its norm as fp32)
            # the oracle keeps its clip coefficient from that fp32 norm: 1e-7 relative on the step
            assert torch.allclose(p, po, rtol=0, atol=2e-7 * 1e-5 + 1e-15)
        else:                                                              # no clip: the oracle with a norm it can never reach
            O.clip_and_adamw([po], [gr], st, step, max_norm=1e30, **hp)
            assert torch.allclose(p, po, rtol=0, atol=1e-7 * 1e-5 + 1e-15)
        assert torch.allclose(m, st[0][0], rtol=0, atol=1e-6 * float(m.abs().max())) and torch.allclose(v, st[0][1], rtol=0, atol=1e-6 * float(v.max()))
    # ranges: the rest untouched, the norm global
    p2, m2, v2, norm2 = R.adamw64(p, gr, m, v, 4, ranges=[(0, 4), (8, 20)])
    keep = torch.ones(n, dtype=torch.bool)
    keep[0:4] = False
    keep[8:20] = False
    assert torch.equal(p2[keep], p[keep]) and torch.equal(m2[keep], m[keep]) and torch.equal(v2[keep], v[keep])
    full = R.adamw64(p, gr, m, v, 4)
    assert torch.equal(p2[~keep], full[0][~keep]) and float(norm2) == float(full[3])


def test_half_ulp_and_f16_sat():
    v = torch.tensor([1.0, 1.5, 1.9999, 2.0, 3e-40, 0.0, 70000.0])
    assert R.half_ulp(v, torch.bfloat16)[:4].tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7]
    assert R.half_ulp(v, torch.float32)[0] == 2.0 ** -24 and R.half_ulp(v, torch.float32)[4] == 2.0 ** -150 and R.half_ulp(v, torch.float16)[5] == 2.0 ** -25
    for dt in (torch.bfloat16, torch.float16):
        x = torch.randn(4096, generator=_gen(6), dtype=torch.float64)
        assert bool(((x.to(dt).double() - x).abs() <= R.half_ulp(x, dt)).all())
    s = R.f16_sat(torch.tensor([70000.0, -1e9, 65519.0, 1.0, float("nan")]))
    assert s[:4].tolist() == [65504.0, -65504.0, 65504.0, 1.0] and bool(torch.isnan(s[4]))


def _rows(M, D, g):
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    x[0] = x[0] * 0.01 + 10.0                  # |mean| = 1e3 std
    return x


@pytest.mark.parametrize("D", [4, 260, 768, 2048])
def test_an_fp32_torch_evaluation_stays_inside_the_bounds(D):
    """The derivations allow for any fp32 evaluation order of the same formulas; torch's own fp32 operators are one."""
    g = _gen(7)
    M, eps = 9, R._f32(1e-6)
    x, gm, bt = _rows(M, D, g), torch.randn(D, generator=g), torch.randn(D, generator=g)
    dy, r1 = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    y64, mean64, rstd64 = R.ln_fwd64(x, gm, bt, eps)
    by, bmean, brstd = R.ln_fwd_bound(x, gm, bt, eps, torch.float32)
    mu = x.mean(-1)
    rs = ((x - mu[:, None]) ** 2).mean(-1).add(eps).rsqrt()
    y = (x - mu[:, None]) * rs[:, None] * gm + bt
    assert bool(((y.double() - y64).abs() <= by).all()) and bool(((mu.double() - mean64).abs() <= bmean).all())
    assert bool(((rs.double() - rstd64).abs() <= brstd).all())
    mu, rs = mean64.float(), rstd64.float()
    xh = (x - mu[:, None]) * rs[:, None]
    gg = dy * 0.25 * gm
    dx = rs[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True)) + r1
    bd = R.ln_bwd_bound(dy, x, gm, eps, 0.25, r1, None, torch.float32)
    assert bool(((dx.double() - R.ln_bwd64(dy, x, gm, eps, 0.25, r1)).abs() <= bd).all())
    # L2
    y64, inv64 = R.l2_fwd64(x, 1e-12)
    inv = 1.0 / x.norm(dim=-1).clamp_min(1e-12)
    byl, binv = R.l2_fwd_bound(x, 1e-12)
    assert bool((((x * inv[:, None]).double() - y64).abs() <= byl).all()) and bool(((inv.double() - inv64).abs() <= binv).all())


def test_the_oracle_fp32_adamw_stays_inside_the_bound():
    g = _gen(8)
    n = 4099
    p, gr = torch.randn(n, generator=g) * 0.02, torch.randn(n, generator=g) * 0.01
    m, v = torch.randn(n, generator=g) * 0.01, torch.rand(n, generator=g) * 1e-4
    for step in (1, 2, 1000):
        p64, m64, v64, _ = R.adamw64(p, gr, m, v, step)
        bdp, bm, bv, _ = R.adamw_bound(p, gr, m, v, step)
        po, st = p.clone(), [(m.clone(), v.clone())]
        # (the oracle takes 1 - beta in Python floats: hand it the fp32 values the C ABI receives, as adamw64 uses them)
        O.clip_and_adamw([po], [gr], st, step, lr=R._f32(1e-5), wd=R._f32(1e-4), betas=(R._f32(0.9), R._f32(0.999)), eps=R._f32(1e-8))
        assert bool((((po.double() - p.double()) - (p64 - p.double())).abs() <= bdp).all())
        assert bool(((st[0][0].double() - m64).abs() <= bm).all()) and bool(((st[0][1].double() - v64).abs() <= bv).all())
