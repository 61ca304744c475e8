"""The row kernels around the GEMM paths — LayerNorm, L2 norm, tap mean, the refine-conv layout kernels, cast, clip + AdamW (csrc/norm.hip,
csrc/elementwise.hip) — PER ELEMENT against the fp64 restatements of tests/rowwise_ref64.py: |got - ref64| <= bound(element), the bound
derived there from the kernel's operation order, never measured.  A failure reports the worst err / bound and its index.  Layout kernels
are held to bit equality.  With GD_ROWWISE_ERRORS=<file> the worst ratio of every group is written there (profiles/rowwise_errors.txt).

Template instantiations named by the launch sites and the case that reaches each (profiles/rowwise_path_coverage.txt has the full table):
  ln_fwd_kernel<T, TO, NV>   test_layernorm_forward[<pair>-D]: NV 1 (D 4, 64, 252), 2 (260, 512), 3 (516, 520, 768), 4 (1016, 1020, 1024), 6 (1028, 1536), 8 (1792, 2044, 2048),
                             pairs bf16->bf16 (narrow), bf16->f32, f32->f32, f32->bf16, f32->f16
  ln_fwd8_kernel<1 | 2>      test_layernorm_forward[bf16_wide-64, -512 | bf16_wide-520, -768, -1016, -1024]
  ln_bwd_kernel<T, TD, NV>   test_layernorm_backward[<variant>-D]: <bf16, bf16> bf16_narrow / bf16_ld4, <bf16, float> bf16_f32dy, <float, float> f32 /
                             cast / ex_f32, <float, f16> ex_f16; the same D -> NV map
  ln_bwd8_kernel<1 | 2>      test_layernorm_backward[bf16_wide-64, -512 | bf16_wide-520, -768, -1016, -1024]
  tap_mean_fwd_kernel, tap_mean_norm_fwd_kernel, tap_mean_bwd_kernel <float | bf16>      test_tap_mean[f32 | bf16 - ...]
  stack3_kernel <float, float>, <float, bf16>, <bf16, bf16>      test_stack3_rows;      unpitch_kernel <float | bf16>      test_unpitch_tokens
  conv_weight_pack_kernel <float | bf16>      test_conv_weight_pack;      cast_kernel (four pairs)      test_cast"""
import os

import pytest
import torch
import torch.nn.functional as F

import rowwise_ref64 as R

pytestmark = pytest.mark.gpu

BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
EPS = R._f32(1e-6)
# the requested sizes, plus: 1020 (nothing else fell into the NV = 4 bucket); 512, 1024 (the 16-byte kernels with lane 63 live in the last slab),
# 520, 1016 (their ragged second slab); 1792 (nv_ = 7 runs as NV = 8 with a wholly empty last slab)
LN_D = [4, 64, 252, 260, 512, 516, 520, 768, 1016, 1020, 1024, 1028, 1536, 1792, 2044, 2048]
LN_M = [1, 3, 5, 9]
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GD_ROWWISE_ERRORS")
    if path and _WORST:
        with open(path, "w") as f:
            for k in sorted(_WORST):
                f.write(f"{_WORST[k][0]:8.4f}  {k:28s} worst at {_WORST[k][1]}\n")


def _g(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _check(group, got, ref, bound, what):
    """Every element: |got - ref| <= bound (bound 0: equality; a NaN anywhere fails)."""
    got = got.detach()
    err = (got.double() - ref.double()).abs()
    bound = bound.double().expand_as(err)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max())
    i = int(ratio.argmax())
    idx = tuple(int(t) for t in torch.unravel_index(torch.tensor(i), ratio.shape))
    if worst > _WORST.get(group, (-1.0, ""))[0]:
        _WORST[group] = (worst, f"{what} {idx}")
    assert worst <= 1.0, (f"{group} / {what}: worst err / bound = {worst:.3f} at {idx}: got {float(got.double().reshape(-1)[i])!r}, "
                          f"ref {float(ref.double().reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i]):.3e}")


def _knob(name, value):
    from gd_amd._lib import check, lib
    old = lib().gd_debug_get(name.encode())
    check(lib().gd_debug_set(name.encode(), value), "gd_debug_set")
    return old


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


CONST = -2.5     # the constant row: D * 2.5 and every partial sum are exact in fp32, so mean == CONST and x - mean == 0 exactly


def _ln_rows(M, D, dtype, seed, shift):
    """Row kinds, cycling from `shift`: randn; |mean| = 1e3 std; constant; magnitude 1e-4; magnitude 1e4; zero but one element; randn."""
    g = _g(seed)
    x = torch.randn(M, D, generator=g, device="cuda") * 2 + 0.5
    kinds = []
    for i in range(M):
        k = (i + shift) % 7
        kinds.append(k)
        if k == 1:
            x[i] = torch.randn(D, generator=g, device="cuda") * 0.02 + 20.0
        elif k == 2:
            x[i] = CONST
        elif k == 3:
            x[i] *= 1e-4
        elif k == 4:
            x[i] *= 1e4
        elif k == 5:
            x[i] = 0.0
            x[i, (7 * i + 3) % D] = 3.0
    return x.to(dtype), kinds


def _gamma_beta(D, seed):
    g = _g(seed)
    gm = (0.5 + torch.rand(D, generator=g, device="cuda")) * torch.where(torch.rand(D, generator=g, device="cuda") < 0.5, -1.0, 1.0)
    return gm, torch.randn(D, generator=g, device="cuda")


def _ln_fwd(x, gm, bt, eps, out_dtype, pad, save_stats):
    """gd_layernorm_fwd on slices of wider, NaN-poisoned buffers (row strides D + pad); the padding must come back untouched."""
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    M, D = x.shape
    xb = torch.full((M, D + pad), float("nan"), dtype=x.dtype, device="cuda")
    xb[:, :D] = x
    yb = torch.full((M, D + pad), float("nan"), dtype=out_dtype, device="cuda")
    before = _bits(yb).clone()
    mean = torch.full((M,), float("nan"), device="cuda") if save_stats else None
    rstd = torch.full((M,), float("nan"), device="cuda") if save_stats else None
    check(lib().gd_layernorm_fwd(ptr(xb), ptr(gm), ptr(bt), ptr(yb), ptr(mean), ptr(rstd), M, D, D + pad, D + pad, float(eps), dtype_code(xb),
                                 dtype_code(yb), stream()), "gd_layernorm_fwd")
    assert torch.equal(_bits(yb)[:, D:], before[:, D:]), "the output padding was written"
    return yb[:, :D], mean, rstd


# name -> (x dtype, y dtype, ln_16b, pad).  pad 8 keeps the row strides multiples of 8 (the 16-byte kernel's condition), pad 4 breaks it
# (ld % 8 == 4 whenever D % 8 == 0); D % 8 == 4 falls to the narrow kernel whatever the stride.
FWD = {"bf16_wide": (BF, BF, 1, 8), "bf16_narrow": (BF, BF, 0, 8), "bf16_ld4": (BF, BF, 1, 4), "bf16_f32": (BF, F32, 1, 8),
       "f32_f32": (F32, F32, 1, 4), "f32_bf16": (F32, BF, 1, 8), "f32_f16": (F32, F16, 1, 4)}


@pytest.mark.parametrize("D", LN_D)
@pytest.mark.parametrize("variant", list(FWD))
def test_layernorm_forward(variant, D):
    tx, ty, knob, pad = FWD[variant]
    gm, bt = _gamma_beta(D, 100 + D)
    if ty == F16 and D >= 8:
        bt[1], bt[2] = 7e4, -7e4                       # past fp16's range: the store saturates at +-65504
    old = _knob("ln_16b", knob)
    try:
        for M in LN_M:
            x, kinds = _ln_rows(M, D, tx, 7 * D + M, (D // 4 + M) % 7)
            y64, mean64, rstd64 = R.ln_fwd64(x, gm, bt, EPS)
            by, bmean, brstd = R.ln_fwd_bound(x, gm, bt, EPS, ty)
            ref = y64.clamp(-65504.0, 65504.0) if ty == F16 else y64
            y, mean, rstd = _ln_fwd(x, gm, bt, EPS, ty, pad, True)
            y0, m0, r0 = _ln_fwd(x, gm, bt, EPS, ty, pad, False)
            assert m0 is None and r0 is None and torch.equal(_bits(y0.contiguous()), _bits(y.contiguous())), "save_stats changes y"
            _check(f"ln_fwd y {variant}", y, ref, by, f"D={D} M={M}")
            _check("ln_fwd mean", mean, mean64, bmean, f"{variant} D={D} M={M}")
            _check("ln_fwd rstd", rstd, rstd64, brstd, f"{variant} D={D} M={M}")
            for i, k in enumerate(kinds):
                if k == 2:      # the constant row: y == beta (as stored) exactly, rstd == rsqrt(eps) to 1 ulp
                    want = R.f16_sat(bt) if ty == F16 else bt.to(ty)
                    assert float(mean[i]) == CONST and torch.equal(y[i], want), (variant, D, M, i)
                    assert abs(float(rstd[i]) - EPS ** -0.5) <= 2.0 ** -23 * EPS ** -0.5
    finally:
        _knob("ln_16b", old)


@pytest.mark.parametrize("D", LN_D)
@pytest.mark.parametrize("tx", [F32, BF], ids=["f32", "bf16"])
def test_layernorm_forward_exactness_probe(tx, D):
    """Small integers whose mean (i - 2 in row i) and variance (5) are exact, gamma a power of two, beta an integer, eps = 11 so that
    var + eps = 16 = 4^2: every fp32 operation of the kernel is exact, and its fp32 output must EQUAL fp64 — statistics included."""
    M = 5
    c = torch.arange(D, device="cuda")
    x = (torch.tensor([-3.0, -1.0, 1.0, 3.0], device="cuda")[c % 4][None] + (torch.arange(M, device="cuda") - 2.0)[:, None]).to(tx)
    gm, bt = torch.ldexp(torch.ones(D, device="cuda"), (c % 5 - 2).int()), (c % 7 - 3.0).float()
    y64, mean64, rstd64 = R.ln_fwd64(x, gm, bt, 11.0)
    assert torch.equal(rstd64, torch.full_like(rstd64, 0.25)) and torch.equal(y64, y64.float().double())
    y, mean, rstd = _ln_fwd(x, gm, bt, 11.0, F32, 4, True)
    assert torch.equal(mean.double(), mean64) and torch.equal(rstd.double(), rstd64) and torch.equal(y.double(), y64)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
# name -> (x dtype, dy dtype, ln_16b, dy pad, entry)
BWD = {"bf16_wide": (BF, BF, 1, 8, "bwd"), "bf16_narrow": (BF, BF, 0, 8, "bwd"), "bf16_ld4": (BF, BF, 1, 4, "bwd"), "bf16_f32dy": (BF, F32, 1, 4, "bwd"),
       "f32": (F32, F32, 1, 4, "bwd"), "cast": (F32, F32, 1, 4, "cast"), "ex_f32": (F32, F32, 1, 4, "ex"), "ex_f16": (F32, F16, 1, 4, "ex")}


def _dy_rows(x, gm, seed):
    """Row i % 3: 0 randn; 1 g = dy gamma orthogonal to xhat with zero mean (dx = rstd g up to rounding); 2 g parallel to xhat (dx cancels
    to zero).  fp64, before the rounding to the kernel's dy type."""
    M, D = x.shape
    mean, _, rstd = R.ln_stats64(x, EPS)
    xh = (x.double() - mean[:, None]) * rstd[:, None]
    g = torch.randn(M, D, generator=_g(seed), device="cuda", dtype=torch.float64)
    for i in range(M):
        if i % 3 == 1:
            one = torch.ones(D, device="cuda", dtype=torch.float64) / D ** 0.5
            g[i] -= one * (g[i] @ one)
            xo = xh[i] - one * (xh[i] @ one)
            if float(xo.norm()) > 0:
                g[i] -= xo * (g[i] @ xo) / (xo @ xo)
        elif i % 3 == 2:
            g[i] = 1.5 * xh[i]
    return g / gm.double()


@pytest.mark.parametrize("D", LN_D)
@pytest.mark.parametrize("variant", list(BWD))
def test_layernorm_backward(variant, D):
    from gd_amd import ops
    from gd_amd._lib import check, lib, ptr, stream
    tx, td, knob, pad, entry = BWD[variant]
    gm, _ = _gamma_beta(D, 200 + D)
    old = _knob("ln_16b", knob)
    try:
        for M in LN_M:
            x, _ = _ln_rows(M, D, tx, 11 * D + M, (D // 4 + M + 3) % 7)
            mean64, _, rstd64 = R.ln_stats64(x, EPS)
            mean, rstd = mean64.float(), rstd64.float()                  # the statistics the kernel is handed: fp64, rounded once
            dy64 = _dy_rows(x, gm, 13 * D + M)
            dys = None
            if td == F16:                                                # an fp16 dy under a power-of-two scale the device-side dy_scale undoes
                dyv, dys, dy_eff = (dy64 * 256.0).half(), torch.tensor([2.0 ** -8], device="cuda"), None
                dy_eff = dyv.double() * 2.0 ** -8
            else:
                dyv = dy64.to(td)
                dy_eff = dyv.double()
            dyb = torch.full((M, D + pad), float("nan"), dtype=dyv.dtype, device="cuda")
            dyb[:, :D] = dyv
            dy = dyb[:, :D]                                              # strided dy: the wrapper allows it on every path
            r1 = torch.randn(M, D, generator=_g(17 * D + M), device="cuda").to(tx)
            r2 = (torch.randn(M, D, generator=_g(19 * D + M), device="cuda") * 3).to(tx)
            if entry != "bwd":
                r1[M - 1, 0] = 1e5      # the fp16 copy saturates here; the LAST row carries max |dx|: the row the waves past M recompute
            for nres, (a, b) in enumerate([(None, None), (r1, None), (r1, r2)]):
                for dyscale in (1.0, 0.25, 2.0 ** -12):
                    what = f"D={D} M={M} dres={nres} dyscale={dyscale}"
                    ref = R.ln_bwd64(dy_eff, x, gm, EPS, dyscale, a, b)
                    bound = R.ln_bwd_bound(dy_eff, x, gm, EPS, dyscale, a, b, tx)
                    if entry == "bwd":
                        dx = ops.layernorm_bwd(dy, x, gm, mean, rstd, dres=a, dyscale=dyscale, dres2=b)
                    else:
                        sc = torch.tensor([8.0 if nres else 0.75], device="cuda")      # (0.75: a scale that is no power of two)
                        dx = torch.full((M, D), float("nan"), device="cuda")
                        dx16 = torch.full((M, D), float("nan"), dtype=F16, device="cuda")
                        slots = torch.zeros(256, dtype=torch.int32, device="cuda")
                        if entry == "cast":
                            check(lib().gd_layernorm_bwd_cast(ptr(dy), ptr(x), ptr(gm), ptr(mean), ptr(rstd), ptr(a), ptr(b), ptr(dx), ptr(dx16), ptr(sc),
                                                              M, D, dy.stride(0), D, dyscale, stream()), "gd_layernorm_bwd_cast")
                        else:
                            check(lib().gd_layernorm_bwd_ex(ptr(dy), 3 if td == F16 else 0, ptr(dys), ptr(x), ptr(gm), ptr(mean), ptr(rstd), ptr(a), ptr(b),
                                                            ptr(dx), ptr(dx16), ptr(sc), ptr(slots), None, M, D, dy.stride(0), D, dyscale, stream()),
                                  "gd_layernorm_bwd_ex")
                            # one slot holds max |dx| bit for bit: the waves past M (M % 4 != 0) recompute row M - 1 and change nothing
                            assert int(slots.max()) == int(_bits(dx.abs().max().reshape(1))), what
                            if nres == 2 and dyscale == 1.0:             # the wrapper's form of the same launch
                                w32, w16 = ops.layernorm_bwd(dy, x, gm, mean, rstd, dres=a, dres2=b, cast_scale=sc, dy_scale=dys, want_amax=True)
                                assert torch.equal(w32, dx) and torch.equal(w16, dx16) and ops.amax_take(w32) is not None
                        assert torch.equal(dx16, R.f16_sat(dx * sc)), what + ": dx16 != f16_sat(dx * s)"
                    assert dx.dtype == tx
                    _check(f"ln_bwd {variant}", dx, ref, bound, what)
    finally:
        _knob("ln_16b", old)


# ------------------------------------------------------------------------------------------------ L2 norm
L2_EPS = R._f32(1e-12)


def _l2(x, dy):
    from gd_amd._lib import check, lib, ptr, stream
    M, D = x.shape
    y, dx = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    inv = torch.full((M,), float("nan"), device="cuda")
    check(lib().gd_l2norm_fwd(ptr(x), ptr(y), ptr(inv), M, D, L2_EPS, stream()), "gd_l2norm_fwd")
    check(lib().gd_l2norm_bwd(ptr(y), ptr(dy), ptr(inv), ptr(dx), M, D, stream()), "gd_l2norm_bwd")
    return y, inv, dx


@pytest.mark.parametrize("D", [1, 3, 63, 64, 65, 96, 200])
def test_l2norm(D):
    """Rows: randn; zero (y == 0, inv == 1 / eps, finite dx); 1e-20 (its squares are fp32 subnormals or flush to zero: under the clamp either
    way, y = x / eps); 1e18 (squares of 1e36 still fit fp32 at these D: an ordinary row); randn * 3.  M = 5 takes them together, M = 1 each
    alone.  The backward is checked on the forward's stored y and inv."""
    from gd_amd import ops
    g = _g(300 + D)
    x5 = torch.randn(5, D, generator=g, device="cuda")
    x5[1] = 0.0
    x5[2] *= 1e-20
    x5[3] = torch.where(x5[3] < 0, -1e18, 1e18) * (1 + 0.25 * torch.rand(D, generator=g, device="cuda"))
    x5[4] *= 3.0
    dy5 = torch.randn(5, D, generator=g, device="cuda")
    for x, dy in [(x5, dy5)] + [(x5[i:i + 1].clone(), dy5[i:i + 1].clone()) for i in range(4)]:
        y, inv, dx = _l2(x, dy)
        y64, inv64 = R.l2_fwd64(x, L2_EPS)
        by, binv = R.l2_fwd_bound(x, L2_EPS)
        _check("l2 fwd y", y, y64, by, f"D={D} M={x.shape[0]}")
        _check("l2 fwd inv", inv, inv64, binv, f"D={D} M={x.shape[0]}")
        _check("l2 bwd", dx, R.l2_bwd64(y, dy, inv), R.l2_bwd_bound(y, dy, inv), f"D={D} M={x.shape[0]}")
        assert bool(torch.isfinite(dx).all())
    y, inv, dx = _l2(x5, dy5)
    assert float(y[1].abs().max()) == 0.0 and float(inv[1]) == float(torch.tensor(1.0) / torch.tensor(L2_EPS, dtype=F32))
    # the autograd wrapper runs the same two kernels
    xa = x5.clone().requires_grad_(True)
    ya = ops.l2_normalize(xa)
    ya.backward(dy5)
    assert torch.equal(ya.detach(), y) and torch.equal(xa.grad, dx)


def test_l2norm_rows_whose_squares_overflow_fp32():
    """|x| = 3e19: every square (9e38) is past fp32's largest number.  What the kernel does: the sum is +Inf, sqrt(Inf) = Inf, inv = 1 / Inf = 0,
    so y = 0, inv = 0 and dx = 0 — finite everywhere, no Inf or NaN.  F.normalize in fp32 does the same (its fp32 norm overflows and x / Inf = 0):
    parity with the operator this kernel replaces, not the unit vector fp64 would give."""
    D = 96
    x = torch.where(torch.randn(2, D, generator=_g(330), device="cuda") < 0, -3e19, 3e19)
    y, inv, dx = _l2(x, torch.randn(2, D, generator=_g(331), device="cuda"))
    assert float(y.abs().max()) == 0.0 and float(inv.abs().max()) == 0.0 and float(dx.abs().max()) == 0.0
    cpu = F.normalize(x.cpu(), dim=-1)
    assert bool(torch.isfinite(cpu).all()) and float(cpu.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ tap mean
@pytest.mark.parametrize("ngrid", [1, 2, 3, 4])
@pytest.mark.parametrize("D", [8, 72, 768])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_tap_mean(dtype, D, ngrid):
    from gd_amd import ops
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    V = 4 if dtype == F32 else 8
    seed = 400
    for prefix in (0, 1, 5):
        for hw in (1, 7, 50):
            for B in (1, 3):
                seed += 1
                what = f"D={D} ngrid={ngrid} prefix={prefix} hw={hw} B={B}"
                g = _g(seed)
                taps = [(torch.randn(B, prefix + hw, D, generator=g, device="cuda") * (1 + t) + 0.5 * t) for t in range(ngrid)]
                for t in taps:
                    t[:, :prefix] = float("nan")                     # the prefix rows are never read
                    t[0, prefix + hw // 2] = 0.0                     # a zero row: inv_norm = 1e12
                    if dtype == F32 and hw > 1:
                        t[B - 1, prefix + hw - 1, 1] = 9e4           # past fp16: the copy saturates
                taps = [t.to(dtype) for t in taps]
                ref, bound = R.tap_mean64(taps, prefix), R.tap_mean_bound(taps, prefix, dtype)
                leaves = [t.clone().requires_grad_(True) for t in taps]
                f0 = ops.tap_mean(leaves, prefix=prefix)
                f1, inv1 = ops.tap_mean([t.clone() for t in taps], prefix=prefix, with_norm=True)
                _check("tap_mean fwd", f0, ref, bound, what)
                assert torch.equal(_bits(f0.detach()), _bits(f1)), what + ": the plain and the normed form differ"
                stored = f1.double()
                inv64 = 1.0 / stored.norm(dim=-1).clamp_min(R._f32(1e-12))
                rel = R.l2_inv_rel_bound(D, V)
                _check("tap_mean inv_norm", inv1, inv64, inv64 * rel, what)
                assert float(inv1[0, hw // 2]) == float(torch.tensor(1.0) / torch.tensor(1e-12, dtype=F32)), what
                if dtype == F32:
                    f2, inv2, h2 = ops.tap_mean([t.clone() for t in taps], prefix=prefix, with_norm=2)
                    assert torch.equal(f2, f1) and torch.equal(inv2, inv1) and torch.equal(h2, R.f16_sat(f2)), what + ": fp16 form"
                # backward through autograd: dout / ngrid rounded once, prefix rows zero, every tap the same
                dout = torch.randn(B, hw, D, generator=g, device="cuda").to(dtype)
                f0.backward(dout)
                dref, dbound = R.tap_mean_bwd64(dout, ngrid, prefix), R.tap_mean_bwd_bound(dout, ngrid, prefix, dtype)
                _check("tap_mean bwd", leaves[0].grad, dref, dbound, what)
                assert prefix == 0 or float(leaves[0].grad[:, :prefix].abs().max()) == 0.0
                for t in leaves[1:]:
                    assert torch.equal(t.grad, leaves[0].grad)
                # the C entry with ngrid destinations of its own, pre-filled with NaN: fully overwritten
                dgs = [torch.full((B, prefix + hw, D), float("nan"), dtype=dtype, device="cuda") for _ in range(ngrid)]
                check(lib().gd_tap_mean_bwd(ops._ptr_array(dgs), ngrid, prefix, ptr(dout), B, hw, D, 1.0 / ngrid, dtype_code(dout), stream()),
                      "gd_tap_mean_bwd")
                for d in dgs:
                    assert torch.equal(d, leaves[0].grad), what + ": direct gd_tap_mean_bwd"


# ------------------------------------------------------------------------------------------------ layout kernels: bit equality
GEOMS = [(1, 1), (1, 4), (3, 1), (5, 7)]


def _sources(B, gh, gw, D, dtype, seed, integer=False):
    """The same grid in token layout (prefix 0, 1, 5; prefix rows NaN) and in pitched layout (separator column NaN):
    -> [(label, tensor, src_bstride, src_row0, src_pitch, grid)]"""
    g = _g(seed)
    grid = torch.randint(-8, 9, (B, gh, gw, D), generator=g, device="cuda").float() if integer else torch.randn(B, gh, gw, D, generator=g, device="cuda")
    grid = grid.to(dtype)
    out = []
    for prefix in (0, 1, 5):
        tok = torch.full((B, prefix + gh * gw, D), float("nan"), dtype=dtype, device="cuda")
        tok[:, prefix:] = grid.reshape(B, gh * gw, D)
        out.append((f"tokens prefix={prefix}", tok, (prefix + gh * gw) * D, prefix * D, gw, grid))
    pit = torch.full((B, gh, gw + 1, D), float("nan"), dtype=dtype, device="cuda")
    pit[:, :, :gw] = grid
    out.append(("pitched", pit, gh * (gw + 1) * D, 0, gw + 1, grid))
    return out


@pytest.mark.parametrize("D", [8, 40])
@pytest.mark.parametrize("ts,td", [(F32, F32), (F32, BF), (BF, BF)], ids=["f32_f32", "f32_bf16", "bf16_bf16"])
def test_stack3_rows(ts, td, D):
    from gd_amd import ops
    for gh, gw in GEOMS:
        for B in (1, 3):
            for label, src, bstride, row0, pitch, grid in _sources(B, gh, gw, D, ts, 500 + gh * 10 + gw + B):
                buf = ops.stack3_rows(src, B, gh, gw, D, bstride, row0, pitch, td)
                what = f"{label} gh={gh} gw={gw} B={B}"
                assert torch.equal(_bits(buf), _bits(R.stack3_rows_ref(grid, td))), what
                assert float(buf[0].abs().max()) == 0.0 and float(buf[-1].abs().max()) == 0.0, what + ": guard rows"
                assert float(buf[1:-1].view(B, gh, gw + 1, 3 * D)[:, :, gw].abs().max()) == 0.0, what + ": separator column"


@pytest.mark.parametrize("D", [8, 40])
def test_stacked_view_is_the_convolution(D):
    """The layout claim without a GEMM kernel: conv_view(stack3(x)) times the (kx, ky, c) weight IS F.conv2d(x) on the pitched grid, and
    conv_view(stack3(dy)) times the packed wt, unpitched, IS its input gradient — in fp64 on integer-valued data, to 1e-12."""
    from gd_amd import ops
    for gh, gw in GEOMS:
        for B in (1, 3):
            g = _g(600 + gh * 10 + gw + B)
            w = torch.randint(-4, 5, (D, D, 3, 3), generator=g, device="cuda").float()
            wk, wt, wu = ops.conv_weight_pack(w, F32, with_wu=True)
            for label, src, bstride, row0, pitch, grid in _sources(B, gh, gw, D, F32, 610 + gh * 10 + gw + B, integer=True):
                rows = B * gh * (gw + 1)
                x = grid.double().permute(0, 3, 1, 2).requires_grad_(True)
                conv = F.conv2d(x, w.double(), padding=1)
                buf = ops.stack3_rows(src, B, gh, gw, D, bstride, row0, pitch, F32)
                out = (ops.conv_view(buf, rows, D).double() @ R.stacked_view_weight(w).double().t()).view(B, gh, gw + 1, D)[:, :, :gw]
                assert float((out - conv.detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-12, (label, gh, gw, B)
            dy = torch.randint(-4, 5, (B, gh, gw, D), generator=g, device="cuda").float()
            conv.backward(dy.double().permute(0, 3, 1, 2))
            dyp = torch.full((B, gh, gw + 1, D), float("nan"), device="cuda")
            dyp[:, :, :gw] = dy
            sbuf = ops.stack3_rows(dyp, B, gh, gw, D, gh * (gw + 1) * D, 0, gw + 1, F32)
            dxp = (ops.conv_view(sbuf, rows, D).double() @ wt.double().t()).float()
            for prefix in (0, 1, 5):
                dtok = ops.unpitch_tokens(dxp, B, gh, gw, D, prefix)
                assert float((dtok[:, prefix:].double().reshape(B, gh, gw, D) - x.grad.permute(0, 2, 3, 1)).abs().max()) <= 1e-12, (gh, gw, B, prefix)
                assert prefix == 0 or float(dtok[:, :prefix].abs().max()) == 0.0


@pytest.mark.parametrize("D", [8, 40])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_unpitch_tokens(dtype, D):
    from gd_amd import ops
    for gh, gw in GEOMS:
        for B in (1, 3):
            src = torch.randn(B, gh, gw + 1, D, generator=_g(700 + gh * 10 + gw + B), device="cuda").to(dtype)
            src[:, :, gw] = float("nan")                                 # the separator column is dropped, never copied
            for prefix in (0, 1, 5):
                out = ops.unpitch_tokens(src.view(-1, D), B, gh, gw, D, prefix)
                assert torch.equal(_bits(out), _bits(R.unpitch_tokens_ref(src, B, gh, gw, D, prefix))), (gh, gw, B, prefix)
                assert prefix == 0 or float(out[:, :prefix].abs().max()) == 0.0


@pytest.mark.parametrize("D", [8, 40])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_conv_weight_pack(dtype, D):
    from gd_amd import ops
    w = torch.randn(D, D, 3, 3, generator=_g(800 + D), device="cuda")
    wk, wt, wu = ops.conv_weight_pack(w, dtype, with_wu=True)
    rk, rt, ru = R.conv_weight_pack_ref(w, dtype)
    assert torch.equal(wk, rk) and torch.equal(wt, rt) and torch.equal(wu, ru)
    assert ops.conv_weight_pack(w, dtype)[2] is None


@pytest.mark.parametrize("D", [8, 40, 6])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_im2col_col2im(dtype, D):
    """Exact against F.unfold / F.fold on integer-valued inputs.  gd_col2im3x3 takes col2im3x3_vec_kernel when a D-wide row is a multiple of 16
    bytes and everything is 16-byte aligned (D = 8, 40 in both types) and the scalar col2im3x3_kernel otherwise (D = 6: 24 and 12 bytes);
    gd_im2col3x3 has the 16-byte form only."""
    from gd_amd import ops
    for gh, gw in GEOMS:
        for B in (1, 3):
            for prefix in (0, 1, 5):
                g = _g(900 + gh * 10 + gw + B + prefix)
                Nt = prefix + gh * gw
                if D != 6:
                    tok = torch.randint(-8, 9, (B, Nt, D), generator=g, device="cuda").to(dtype)
                    col = ops.im2col3x3(tok[:, prefix:], Nt * D, B, gh, gw, D)
                    unf = F.unfold(tok[:, prefix:].float().reshape(B, gh, gw, D).permute(0, 3, 1, 2), 3, padding=1)      # [B, (c, ky, kx), L]
                    assert torch.equal(col.float().view(B, gh * gw, 9, D), unf.view(B, D, 9, gh * gw).permute(0, 3, 2, 1)), (gh, gw, B, prefix)
                dcol = torch.randint(-4, 5, (B * gh * gw, 9 * D), generator=g, device="cuda").to(dtype)
                dx = ops.col2im3x3(dcol, B, gh, gw, D, prefix=prefix)
                fold = F.fold(dcol.float().view(B, gh * gw, 9, D).permute(0, 3, 2, 1).reshape(B, D * 9, gh * gw), (gh, gw), 3, padding=1)
                assert torch.equal(dx[:, prefix:].float().reshape(B, gh, gw, D), fold.permute(0, 2, 3, 1)), (gh, gw, B, prefix)
                assert prefix == 0 or float(dx[:, :prefix].abs().max()) == 0.0


@pytest.mark.parametrize("ti,to", [(F32, BF), (BF, F32), (F32, F32), (BF, BF)], ids=["f32_bf16", "bf16_f32", "f32_f32", "bf16_bf16"])
def test_cast(ti, to):
    """gd_cast: out = round(in * scale) — the fp32 product (u |v|; exact for a power of two) and one rounding of the stored type."""
    from gd_amd import ops
    for n in (1, 255, 257, 4099):
        x = torch.randn(n, generator=_g(950 + n), device="cuda").to(ti)
        for scale in (1.0, 0.25, 0.3):
            sc = R._f32(scale)
            ref = x.double() * sc
            exact = scale != 0.3 and (to == F32 or ti == BF)             # a power-of-two scale, and a store at least as wide as the input
            b = torch.zeros_like(ref) if scale != 0.3 else R.U * ref.abs()
            if not exact and to != F32:
                b = b + R.half_ulp(ref.abs() + b, to)
            _check("cast", ops.cast(x, to, scale), ref, b, f"{ti}->{to} n={n} scale={scale}")


# ------------------------------------------------------------------------------------------------ clip + AdamW
def _ranges(n):
    """None (everything); [(0, 4)]; a range that ends at n (n % 4 != 0 for 255, 257, 4099); two disjoint ranges."""
    out = [None]
    if n >= 8:
        out += [[(0, 4)], [((n // 2) // 4 * 4, n)], [(0, 8), (16, min(100, n))]]
    return out


@pytest.mark.parametrize("mode", ["active", "inactive", "disabled"])
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_clip_adamw(n, mode):
    """gd_clip_adamw_step / gd_clip_adamw_ranges: the update p_new - p_old, both moments and the returned norm against adamw64, bounds from
    adamw_bound (relative to lr, plus the stored parameter's own rounding).  Clip active (norm >> max_norm), inactive (norm << max_norm:
    coef == grad_scale exactly), disabled (max_norm = 0 under a large gradient).  Outside the ranges nothing moves, and the norm is global."""
    from gd_amd import ops
    g = _g(1000 + n)
    for step in (1, 2, 1000):
        for gs in (0.5, 1.0):
            for ranges in _ranges(n):
                p = torch.randn(n, generator=g, device="cuda") * 0.02
                gr = torch.randn(n, generator=g, device="cuda")
                gr = torch.where(gr < 0, -1.0, 1.0) * (1 + gr.abs()) * 10 if mode != "inactive" else gr * 1e-3 / n ** 0.5
                m, v = torch.randn(n, generator=g, device="cuda") * 0.01, torch.rand(n, generator=g, device="cuda") * 1e-4
                max_norm = 0.0 if mode == "disabled" else 1.0
                what = f"n={n} {mode} step={step} gs={gs} ranges={ranges}"
                p64, m64, v64, norm64 = R.adamw64(p, gr, m, v, step, max_norm=max_norm, grad_scale=gs, ranges=ranges)
                bdp, bm, bv, bn = R.adamw_bound(p, gr, m, v, step, max_norm=max_norm, grad_scale=gs)
                active = max_norm > 0 and float(norm64) > max_norm
                assert active == (mode == "active"), what
                p1, m1, v1 = p.clone(), m.clone(), v.clone()
                norm = ops.clip_adamw_step(p1, gr, m1, v1, step, max_norm=max_norm, grad_scale=gs, ranges=ranges)
                inside = torch.zeros(n, dtype=torch.bool, device="cuda")
                for a, b in (ranges or [(0, n)]):
                    inside[a:b] = True
                z = torch.zeros(n, dtype=torch.float64, device="cuda")
                _check("adamw update", p1.double() - p.double(), p64 - p.double(), torch.where(inside, bdp, z), what)
                _check("adamw exp_avg", m1, m64, torch.where(inside, bm, z), what)
                _check("adamw exp_avg_sq", v1, v64, torch.where(inside, bv, z), what)
                _check("adamw norm", norm, norm64.reshape(1), (norm64 * bn).reshape(1), what)
                out = ~inside
                assert torch.equal(_bits(p1)[out], _bits(p)[out]) and torch.equal(_bits(m1)[out], _bits(m)[out]) and torch.equal(_bits(v1)[out], _bits(v)[out]), what
