"""The kernels on the trained-parameter path — the one-pass LoRA backward (csrc/lora.hip) and the fused bottleneck adapters (csrc/adapter.hip) —
against fp64, element by element, in every instantiation their dispatch switches ship, and the block that runs them at the magnitudes LoRA B
has when a fine-tune starts.

Same method as test_gpu_gemm_paths.py: the reference is the fp64 result of the operands AS THE KERNEL SEES THEM, computed on the GPU; bounds are
per element and derived (accumulation C_ACC n 2^-24 sum|a||b|, the split of t, one output rounding).  Four parts:

  a. exact probes: small-integer / dyadic operands whose every partial sum fits fp32's 24 bits, so the result must EQUAL fp64 under any
     summation order, atomics included.  An accumulation bound at M = 87 680 is too loose to see one 64-row chunk; equality is not.
  b. random operands with element-wise bounds: every K / 256 and operand type of lora_bwd_fused_kernel, every (D, kernel form) of the adapters
     through the real dispatch (M thresholds, the adapter_persist knob), gate edge values, device scales, fp16 saturation, the LayerNorm form.
  c. the fused fp16 LoRA backward with B formatted by vit._opw_lora_b at |B| from 0 to 1e-2.
  d. one block (q / v LoRA + adapter, tf32h engine) against an fp64 restatement, judged by the engine's own contract: no worse than TF32.

profiles/trainable_path_coverage.txt records the kernel trace of this file, profiles/trainable_path_errors.txt the ratios (c) and (d) measured.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

from test_gpu_gemm_paths import B_MAGS, C_ACC, FLOOR, ROUND, U, assert_within

pytestmark = pytest.mark.gpu

_F16, _BF16, _F32 = torch.float16, torch.bfloat16, torch.float32
F16_MAX = 65504.0


def _mk(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(dtype)


class _knob:
    """with _knob(name, value): one library knob (gd_debug_set) for the duration of the block, its previous value restored after; value None: untouched."""

    def __init__(self, name, value):
        self.name, self.value = name.encode(), value

    def __enter__(self):
        from gd_amd._lib import lib
        if self.value is not None:
            self.keep = lib().gd_debug_get(self.name)
            assert lib().gd_debug_set(self.name, int(self.value)) == 0, self.name

    def __exit__(self, *exc):
        from gd_amd._lib import lib
        if self.value is not None:
            lib().gd_debug_set(self.name, self.keep)


def assert_exact(got, ref, what):
    """every element of got equals the fp64 ref (NaN fails); names the first element that does not."""
    bad = ~(got.double() == ref)
    if bool(bad.any()):
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result (first at {list(idx)}: "
                             f"got {float(got[idx])!r}, exact {float(ref[idx])!r})")


# ------------------------------------------------------------------------------------------------------------------------------------------
# a. exact probes.  The constructors are plain index arithmetic (no random numbers, any device), so the 24-bit condition is checked on the CPU.
# ------------------------------------------------------------------------------------------------------------------------------------------
LOW_SHIFT = {_BF16: 9, _F16: 12}      # t = a + b 2^-shift, |a| <= 3: 2 + shift bits, more than the 8 (bf16) / 11 (fp16) of the high part alone


def lora_probe(m0, m1, K, dtype, device):
    """rows m0..m1-1 of the exact LoRA probe -> X [m1 - m0, K] (operand dtype), t [m1 - m0, 8] f32.
    X[m, k] in {-2, -1, 1, 2} where (5 m + k) % 257 == 0, else 0: about K / 257 entries per row and M / 257 per column, so a column's sum over
    M = 87 680 rows stays below 2^24 units while every row (hence every chunk and slab) still reaches some output element.  t[m, r] = a + b 2^-shift
    with a = (m + 3 r) % 7 - 3 and b in {-1, 0, 1} on (m + r) % 5 == 0: the entries with b != 0 need the kernel's low 16-bit part."""
    m = torch.arange(m0, m1, device=device, dtype=torch.int64)[:, None]
    k = torch.arange(K, device=device, dtype=torch.int64)[None, :]
    v = (m * 3 + k * 7) % 4
    X = torch.where((5 * m + k) % 257 == 0, torch.where(v < 2, v - 2, v - 1), torch.zeros_like(v)).to(torch.float32).to(dtype)
    r = torch.arange(8, device=device, dtype=torch.int64)[None, :]
    a = (m + 3 * r) % 7 - 3
    b = torch.where((m + r) % 5 == 0, (m + 2 * r) % 3 - 1, torch.zeros_like(a))
    t = a.to(torch.float32) + b.to(torch.float32) * 2.0 ** -LOW_SHIFT[dtype]
    return X, t


def lora_probe_b(K, dtype, device):
    """bt [8, K] integers in -3..3, g0 [8, K] integers in -5..5 (the tensor gbt accumulates into)."""
    r = torch.arange(8, device=device, dtype=torch.int64)[:, None]
    k = torch.arange(K, device=device, dtype=torch.int64)[None, :]
    return ((5 * r + k) % 7 - 3).to(torch.float32).to(dtype), ((r + 3 * k) % 11 - 5).to(torch.float32)


def lora_probe_units(M, K, dtype, device="cpu", rows=8192):
    """max over the outputs of the sum of |terms| in units of the smallest step (2^-shift for gbt, 1 for dt): below 2^24 every partial sum of any
    summation order is an integer number of units that fp32 holds exactly.  Also returns how many 64-row chunks reach no gbt element (must be 0)."""
    unit = 2.0 ** -LOW_SHIFT[dtype]
    bt, g0 = lora_probe_b(K, dtype, device)
    acc = g0.double().abs()
    dt_max, dead = 0.0, 0
    for m0 in range(0, M, rows):
        X, t = lora_probe(m0, min(M, m0 + rows), K, dtype, device)
        Xa, ta = X.double().abs(), t.double().abs()
        acc = acc + ta.t() @ Xa
        dt_max = max(dt_max, float((Xa @ bt.double().abs().t()).max()))
        live = (ta.sum(1) > 0) & (Xa.sum(1) > 0)
        live = torch.cat([live, live.new_zeros(-live.numel() % 64)]).view(-1, 64)       # (rows is a multiple of 64: chunks do not straddle calls)
        dead += int((~live.any(1)).sum())
    return float(acc.max()) / unit, dt_max, dead


# (operand type, M, K, row stride, accumulate into non-zero gbt, with bt).  M: below one chunk; M % 64 in {1, 63}; 512 * 64 + 65 rows = 514
# chunks on the 512-block grid, so blocks 0 and 1 take a second chunk (the last one ragged); the step's 87 680.  K / 256: all of 1, 2, 3, 4, 6, 8.
LORA_EXACT = [
    (_BF16, 40, 256, 256, False, True),
    (_F16, 40, 512, 768, True, True),
    (_BF16, 64 * 3 + 1, 768, 768, True, True),
    (_F16, 64 * 3 + 1, 1024, 1024, False, True),
    (_BF16, 64 * 5 + 63, 2048, 3072, False, True),
    (_F16, 64 * 5 + 63, 1536, 1536, True, False),
    (_F16, 512 * 64 + 65, 512, 512, False, True),
    (_BF16, 512 * 64 + 65, 1024, 1536, True, False),
    (_F16, 87680, 1536, 2304, True, True),
    (_BF16, 87680, 1536, 2304, False, True),
    (_F16, 87680, 1024, 1024, False, False),      # the LoRA-A gradient of ViT-L: bt = NULL
]
_lora_exact_ids = [f"{'bf16' if c[0] == _BF16 else 'f16'}-M{c[1]}-K{c[2]}-ld{c[3]}{'-acc' if c[4] else ''}{'' if c[5] else '-nobt'}" for c in LORA_EXACT]


def check_lora_probe_inputs(device):
    """(tests/test_trainable_probe_inputs.py runs this and check_adapter_probe_inputs on the CPU)"""
    for dtype, M, K, _, _, _ in LORA_EXACT:
        units, dt_units, dead = lora_probe_units(M, K, dtype, device)
        assert units < 2 ** 24 and dt_units < 2 ** 24, (dtype, M, K, units, dt_units)
        assert dead == 0, (dtype, M, K, dead)
        X, t = lora_probe(0, min(M, 512), K, dtype, device)
        # exactly representable, and some t needs its low part
        assert bool((t.to(dtype).float() != t).any())
        hi = t.to(dtype).float()
        assert torch.equal((t - hi).to(dtype).float(), t - hi)


@pytest.mark.parametrize("case", LORA_EXACT, ids=_lora_exact_ids)
def test_lora_bwd_exact_probe(case):
    """dt and gbt equal the fp64 result exactly: any dropped / doubled row, chunk, slab, rank or low part changes an integer count of units.
    fp16 cases run the scaled entry point with t_mul = 2, out_mul = 1 / 2 (powers of two: still exact), bf16 cases the plain one."""
    from gd_amd import ops
    dtype, M, K, ldx, acc, with_bt = case
    units, dt_units, dead = lora_probe_units(M, K, dtype, "cuda")
    assert units * 2 < 2 ** 24 and dt_units < 2 ** 24 and dead == 0, (units, dt_units, dead)      # (x 2: t_mul)
    X, t = lora_probe(0, M, K, dtype, "cuda")
    if ldx != K:
        buf = torch.full((M, ldx), 3.0, dtype=dtype, device="cuda")       # (the columns beside the view are non-zero: reading them would show)
        buf[:, :K] = X
        X = buf[:, :K]
    bt, g0 = lora_probe_b(K, dtype, "cuda")
    if not acc:
        g0 = torch.zeros_like(g0)
    gbt = g0.clone()
    if dtype == _F16:
        tm, om = torch.tensor([2.0], device="cuda"), torch.tensor([0.5], device="cuda")
        dt = ops.lora_bwd_fused_h(X, t, bt if with_bt else None, gbt, t_mul=tm, out_mul=om)
        dmul = 0.5
    else:
        dmul = 1.0
        if with_bt:
            dt = ops.lora_bwd_fused(X, t, bt, gbt)
        else:
            ops.skinny_tn_mfma(t, X, gbt)
    assert_exact(gbt, g0.double() + t.double().t() @ X.double(), "gbt")
    if with_bt:
        assert_exact(dt, dmul * (X.double() @ bt.double().t()), "dt")


def _pick(v, values):
    """values[v % len(values)], element-wise"""
    return torch.tensor(values, device=v.device, dtype=torch.int64)[v % len(values)]


def adapter_probe(M, D, device, back=False):
    """x [M, D], w1 [64, D], w2 [D, 64] as fp64 integers.  x in {-1, 1} on (m + d) % 16 == 0; w1[j, d] in {-1, 1, 2} on d % 64 == j;
    w2[d, j] in {-1, 1} on (d + j) % 8 == 0 (signs from index hashes).  hidden[m, j] then has D / 64 terms of at most 2 and is non-zero only for j = -m mod 16; out has four
    hidden terms per element: |hidden| <= 32 and |out| <= 129 at D = 1024, exact in bf16 (8 bits hold integers to 256).
    back: the input of the backward-to-input probe (dOut against w2^T, gated by the forward's hidden, then w1^T): non-zero on (d - m) % 16 == 0,
    the columns that meet w2's pattern at the hidden columns j = -m mod 16 the gate keeps (D / 16 terms of at most 1)."""
    m = torch.arange(M, device=device, dtype=torch.int64)[:, None]
    d = torch.arange(D, device=device, dtype=torch.int64)[None, :]
    x = torch.where(((-m if back else m) + d) % 16 == 0, _pick(m * 7 + d * 3 + (m * d) % 5, (-1, 1, 1)), torch.zeros_like(m + d)).double()
    j = torch.arange(64, device=device, dtype=torch.int64)[:, None]
    w1 = torch.where(d % 64 == j, _pick(j * 5 + (d // 64) * 3 + (j * (d // 64)) % 7, (-1, 1, 2, 1)), torch.zeros_like(j + d)).double()                 # [64, D]
    dd, jj = d.t(), j.t()
    w2 = torch.where((dd + jj) % 8 == 0, _pick((dd // 8) * 5 + jj * 3 + ((dd // 8) * jj) % 7, (-1, 1, 1)), torch.zeros_like(dd + jj)).double()       # [D, 64]
    return x, w1, w2


def adapter_probe_expect(x, w1, w2, gate=None, sin=1.0, alpha=1.0):
    pre = (x * sin) @ w1.t()
    h = torch.relu(pre) if gate is None else torch.where(gate > 0, pre, torch.zeros_like(pre))
    return h, x + alpha * (h @ w2.t())


def check_adapter_probe_inputs(device):
    for D in (256, 512, 768, 1024):
        x, w1, w2 = adapter_probe(2048 + 31, D, device)
        h, out = adapter_probe_expect(x, w1, w2)
        assert float(h.abs().max()) <= 256 and float(out.abs().max()) <= 256, (D, float(h.abs().max()), float(out.abs().max()))
        assert float((x.abs() @ w1.abs().t()).max()) * 2 < 2 ** 24 and float((h.abs() @ w2.abs().t() + x.abs()).max()) * 4 < 2 ** 24
        # structured, not degenerate: every 32-row tile has live hidden entries and rows the adapter branch moves
        n = (x.shape[0] // 32) * 32
        assert bool((h[:n] > 0).view(-1, 32 * 64).any(1).all()) and bool((out[:n] != x[:n]).view(-1, 32 * D).any(1).all()), D
        # backward form: the gate is the forward's hidden, the input the `back` probe
        g2, _, _ = adapter_probe(x.shape[0], D, device, back=True)
        dh, dx = adapter_probe_expect(g2, w2.t(), w1.t(), gate=h, sin=2.0, alpha=0.5)
        assert float(dh.abs().max()) <= 256 and float((dx * 4).abs().max()) <= 2048 and bool((dh != 0).any())
        dh, dx = adapter_probe_expect(g2, w2.t(), w1.t(), gate=h)                                    # (the bf16 form: no scales, bf16 dX)
        assert float(dh.abs().max()) <= 256 and float(dx.abs().max()) <= 256 and bool((dh != 0).any())


# (form, D, M, adapter_persist knob).  form "bf16": gd_adapter_fused — adapter_fused_kernel<D> below M = 32 768 rows (or with the knob at 0),
# adapter_persist_kernel<D> from there; "h": gd_adapter_fused_h — adapter_persist_h_kernel<D>, M >= 8192; "ln": gd_adapter_fused_h_ln —
# adapter_persist_h_kernel<D, true>.  M % 32 in {1, 31}; M = 40 < 64; 256 blocks x 32 rows + 1: block 0 takes a second tile.
ADAPTER_EXACT = [
    ("bf16", 256, 40, None), ("bf16", 512, 33, None), ("bf16", 768, 95, None), ("bf16", 1024, 2048 + 31, None),
    ("bf16", 256, 32768 + 1, None), ("bf16", 512, 32768 + 31, None), ("bf16", 768, 87680, None), ("bf16", 1024, 32768 + 33, None),
    ("bf16", 768, 32768 + 31, 0),
    ("h", 256, 8192 + 1, None), ("h", 512, 8192 + 31, None), ("h", 768, 87680, None),
    ("ln", 256, 8192 + 31, None), ("ln", 512, 8192 + 1, None), ("ln", 768, 8192 + 33, None),
]


@pytest.mark.parametrize("form,D,M,persist", ADAPTER_EXACT, ids=[f"{c[0]}-D{c[1]}-M{c[2]}" + ("" if c[3] is None else f"-persist{c[3]}") for c in ADAPTER_EXACT])
def test_adapter_exact_probe(form, D, M, persist):
    """hidden and out (and the scaled fp16 copy) equal the fp64 result exactly, forward and backward-to-input, in every kernel form."""
    from gd_amd import ops
    x, w1, w2 = adapter_probe(M, D, "cuda")
    h_ref, out_ref = adapter_probe_expect(x, w1, w2)
    assert float(h_ref.abs().max()) <= 256 and float(out_ref.abs().max()) <= 256
    g2, _, _ = adapter_probe(M, D, "cuda", back=True)
    with _knob("adapter_persist", persist):
        if form == "bf16":
            out, hid = ops.adapter_fused(x.to(_BF16), w1.to(_BF16), w2.to(_BF16))
            assert_exact(hid, h_ref, "hidden")
            assert_exact(out, out_ref, "out")
            dh_ref, dx_ref = adapter_probe_expect(g2, w2.t(), w1.t(), gate=h_ref)
            dx, dh = ops.adapter_fused(g2.to(_BF16), w2.t().contiguous().to(_BF16), w1.t().contiguous().to(_BF16), gate_src=hid)
            assert_exact(dh, dh_ref, "d(hidden)")
            assert_exact(dx, dx_ref, "dX")
            return
        x32, w1h, w2h = x.float(), w1.to(_F16), w2.to(_F16)
        if form == "ln":
            g, b = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
            out, hid, y16, mean, rstd = ops.adapter_fused_h_ln(x32, w1h, w2h, g, b, 1e-6)
            # out is exact, so the LayerNorm reference is that of out_ref (gamma = 1, beta = 0); bounds as derived in test_adapter_ln_random.
            # Pins the normed rows of the ragged last tile too.
            mu = out_ref.mean(1, keepdim=True)
            xc = out_ref - mu
            var = (xc * xc).mean(1, keepdim=True)
            rs = (var + 1e-6).rsqrt()
            e_mu = C_ACC * D * U * out_ref.abs().mean(1, keepdim=True)
            e_rs_rel = 0.5 * (C_ACC * D * U + 2 * e_mu * var.sqrt() / (var + 1e-6)) + 4 * U
            assert_within(mean, mu[:, 0], e_mu[:, 0], "row mean")
            assert_within(rstd, rs[:, 0], (rs * e_rs_rel)[:, 0], "row rstd")
            assert_within(y16, xc * rs, rs * (e_mu + U * xc.abs() + xc.abs() * e_rs_rel) + 4 * U * (xc * rs).abs(), "fp16 LayerNorm rows")
        else:
            out, hid, _ = ops.adapter_fused_h(x32, w1h, w2h)
        assert_exact(hid, h_ref, "hidden")
        assert_exact(out, out_ref, "out")
        if form == "h":
            sc = torch.tensor([2.0, 0.5, 4.0], device="cuda")
            dh_ref, dx_ref = adapter_probe_expect(g2, w2.t(), w1.t(), gate=h_ref, sin=2.0, alpha=0.5)
            dx, dh, dx16 = ops.adapter_fused_h(g2.float(), w2h.t().contiguous(), w1h.t().contiguous(), gate_src=hid, in_scale=sc[0:1], alpha_dev=sc[1:2],
                                               copy_scale=sc[2:3], want_copy=True)
            assert_exact(dh, dh_ref, "d(hidden)")
            assert_exact(dx, dx_ref, "dX")
            assert_exact(dx16, 4.0 * dx_ref, "fp16 copy of dX")


# ------------------------------------------------------------------------------------------------------------------------------------------
# b. random operands, element-wise bounds
# ------------------------------------------------------------------------------------------------------------------------------------------
SPLIT = {_BF16: 2.0 ** -16, _F16: 2.0 ** -22}     # t = hi + lo in the operand type: what is left of t after two 8-bit (11-bit) parts, relative


def _lora_expect(X, t, bt, g0, tmul, omul, dt_scaled, dt_mul=1.0):
    """-> (dt64, dt bound, gbt64, gbt bound).  dt: K products, exact in fp32, accumulated: C_ACC K u |X||bt|^T, times its multipliers.  gbt: the
    accumulation over M (in the MFMA, across a block's chunks, then fp32 atomics) plus what the two-part split drops of t * t_mul — SPLIT
    relative, and in fp16 an absolute 2^-25 per term where the low part falls below the subnormal spacing 2^-24 — then * out_mul and the add."""
    M, K = X.shape
    Xd, dtype = X.double(), X.dtype
    te = (t * tmul).double()
    gref = g0.double() + omul * (te.t() @ Xd)
    ge = abs(omul) * ((C_ACC * M * U + SPLIT[dtype]) * (te.abs().t() @ Xd.abs()) + (2.0 ** -25 if dtype == _F16 else 0.0) * Xd.abs().sum(0)[None, :])
    ge = ge + 2 * U * gref.abs() + 2 * U * g0.double().abs()
    if bt is None:
        return None, None, gref, ge
    dm = dt_mul * (1.0 if dt_scaled else omul)
    return dm * (Xd @ bt.double().t()), C_ACC * K * U * abs(dm) * (Xd.abs() @ bt.double().abs().t()), gref, ge


# the combinations vit.py makes: the plain bf16 call (bf16 engine: dqv pass and, with bt = NULL, the LoRA-A gradient); on the scaled entry point
# the (dq, dv) pass with out_mul = 1 / s and dt in either domain, the LoRA-A gradient with dt under t_mul = s (h16_dy = 0) or already scaled
LORA_MODES = [(_BF16, "plain"), (_BF16, "plain_nobt")] + [(d, m) for d in (_BF16, _F16) for m in ("dqv", "dqv_dt_scaled", "gat_tmul", "gat_scaled_dt")]


@pytest.mark.parametrize("dtype,mode", LORA_MODES, ids=[f"{'bf16' if d == _BF16 else 'f16'}-{m}" for d, m in LORA_MODES])
@pytest.mark.parametrize("nslab", [1, 2, 3, 4, 6, 8])
def test_lora_bwd_random(nslab, dtype, mode):
    """every lora_bwd_fused_kernel<T, K / 256> through both entry points (gd_lora_bwd_fused is bf16 only), nine full chunks and a 37-row tail,
    a strided operand, accumulation into a non-zero gbt."""
    from gd_amd import ops
    K, M = 256 * nslab, 64 * 9 + 37
    seed = zlib.crc32(f"{dtype}{nslab}{mode}".encode()) % 10000
    s = 4096.0
    sc = torch.tensor([s, 1.0 / s], device="cuda")
    X = _mk((M, K + 64), dtype, seed)[:, :K]
    t = _mk((M, 8), _F32, seed + 1, 0.3)
    bt = _mk((8, K), dtype, seed + 2, 0.05)
    g0 = _mk((8, K), _F32, seed + 3, 1e-3 if mode not in ("plain", "plain_nobt") else 1.0)
    gbt = g0.clone()
    if mode == "plain":
        dt = ops.lora_bwd_fused(X, t, bt, gbt)
        exp = _lora_expect(X, t, bt, g0, 1.0, 1.0, False)
    elif mode == "plain_nobt":
        dt = None
        ops.skinny_tn_mfma(t, X, gbt)
        exp = _lora_expect(X, t, None, g0, 1.0, 1.0, False)
    elif mode in ("dqv", "dqv_dt_scaled"):
        dts = mode == "dqv_dt_scaled"
        dt = ops.lora_bwd_fused_h(X, t, bt, gbt, out_mul=sc[1:2], dt_scaled=dts)
        exp = _lora_expect(X, t, bt, g0, 1.0, 1.0 / s, dts)
    else:
        tg = t * (1e-5 if mode == "gat_tmul" else 1e-5 * s)      # a gradient in the t role: true size ~1e-5, or already under s
        dt = ops.lora_bwd_fused_h(X, tg, None, gbt, t_mul=sc[0:1] if mode == "gat_tmul" else None, out_mul=sc[1:2])
        exp = _lora_expect(X, tg, None, g0, s if mode == "gat_tmul" else 1.0, 1.0 / s, False)
    dref, de, gref, ge = exp
    assert_within(gbt, gref, ge, f"gbt {mode} K={K}")
    if dref is not None:
        assert_within(dt, dref, de, f"dt {mode} K={K}")


def _adapter_expect(x16d, w1, hid_fn):
    """x16d: the first product's left operand as the kernel holds it (fp64 of the 16-bit values).  -> hidden64, bound (before its rounding)."""
    D = x16d.shape[1]
    pre = x16d @ w1.double().t()
    return hid_fn(pre), C_ACC * D * U * (x16d.abs() @ w1.double().abs().t())


def _out_expect(hid, w2, resid, alpha=1.0):
    """out from the kernel's OWN stored hidden tile (its second product's operand): 64 products accumulated, times alpha, plus the residual."""
    hd, wd = hid.double(), w2.double()
    ref = resid.double() + alpha * (hd @ wd.t())
    return ref, C_ACC * 64 * U * abs(alpha) * (hd.abs() @ wd.abs().t()) + 2 * U * ref.abs()


def _edge_gate(hid):
    """the forward's hidden as the backward's gate, with edge values planted: row 5 all zero (gated off), row M - 1 (the ragged tile) the smallest
    positive subnormal everywhere (> 0: kept), row M - 2 negative zero everywhere (not > 0: dropped), row 9 alternating +0 / subnormal / -0."""
    g = hid.clone()
    bits = g.view(torch.int16)
    M = g.shape[0]
    bits[5] = 0
    bits[M - 1] = 1
    bits[M - 2] = -32768
    bits[9, 0::3] = 0
    bits[9, 1::3] = 1
    bits[9, 2::3] = -32768
    return g


ADAPTER_BF16 = [(256, 1000 + 31, None), (512, 1000 + 1, None), (768, 2000 + 31, None), (1024, 1000 + 1, None),
                (256, 32768 + 31, None), (512, 32768 + 1, None), (768, 32768 + 31, None), (1024, 32768 + 1, None), (512, 32768 + 31, 0)]


@pytest.mark.parametrize("D,M,persist", ADAPTER_BF16, ids=[f"D{c[0]}-M{c[1]}" + ("" if c[2] is None else f"-persist{c[2]}") for c in ADAPTER_BF16])
def test_adapter_bf16_random(D, M, persist):
    """gd_adapter_fused: adapter_fused_kernel<D> (M < 32 768, or adapter_persist = 0) and adapter_persist_kernel<D>, forward and backward-to-input
    with the edge gate."""
    from gd_amd import ops
    x = _mk((M, D), _BF16, D + M)
    down, up = _mk((64, D), _BF16, D + 1, 0.05), _mk((D, 64), _BF16, D + 2, 0.05)
    dout = _mk((M, D), _BF16, D + 3)
    with _knob("adapter_persist", persist):
        out, hid = ops.adapter_fused(x, down, up)
        gate = _edge_gate(hid)
        dx, dh = ops.adapter_fused(dout, up.t().contiguous(), down.t().contiguous(), gate_src=gate)
    href, he = _adapter_expect(x.double(), down, torch.relu)
    assert_within(hid, href, he, "hidden")
    assert_within(out, *_out_expect(hid, up, x), "out")
    keep = gate.double() > 0
    assert not bool(keep[5].any()) and bool(keep[M - 1].all()) and not bool(keep[M - 2].any())
    dref, de = _adapter_expect(dout.double(), up.t(), lambda p: torch.where(keep, p, torch.zeros_like(p)))
    assert_within(dh, dref, de, "d(hidden)")
    assert bool((dh[5] == 0).all()) and bool((dh[M - 2] == 0).all()) and bool((dh[M - 1] != 0).any()), "gate edge rows"
    assert_within(dx, *_out_expect(dh, down.t(), dout), "dX")
    assert torch.equal(dx[5], dout[5]), "a row that is gated off passes dOut through unchanged"


@pytest.mark.parametrize("D,M", [(256, 8192 + 31), (512, 8192 + 1), (768, 8192 + 31), (512, 16384 + 33)])
def test_adapter_fp16_random(D, M):
    """gd_adapter_fused_h: adapter_persist_h_kernel<D>.  Forward; backward-to-input with the edge gate, a gradient-sized dOut (~1e-6) under the
    three device scales, and the fp16 copy; then a copy that saturates."""
    from gd_amd import ops
    x = _mk((M, D), _F32, D + M)
    down, up = _mk((64, D), _F32, D + 1, 0.05).half(), _mk((D, 64), _F32, D + 2, 0.05).half()
    out, hid, _ = ops.adapter_fused_h(x, down, up)
    href, he = _adapter_expect(x.half().double(), down, torch.relu)
    assert_within(hid, href, he, "hidden")
    assert_within(out, *_out_expect(hid, up, x), "out")
    dout = _mk((M, D), _F32, D + 3, 1e-6)
    sc = ops.amax_scale(dout, 8.0)
    s = float(sc[0])
    gate = _edge_gate(hid)
    keep = gate.double() > 0
    dx, dh, dx16 = ops.adapter_fused_h(dout, up.t().contiguous(), down.t().contiguous(), gate_src=gate, in_scale=sc[0:1], alpha_dev=sc[1:2],
                                       copy_scale=sc[0:1], want_copy=True)
    d16 = (dout * s).half().double()                      # (|dOut| s <= 8: no saturation; the kernel rounds to nearest even as torch does)
    dref, de = _adapter_expect(d16, up.t(), lambda p: torch.where(keep, p, torch.zeros_like(p)))
    assert_within(dh, dref, de, "d(hidden), scaled")
    assert bool((dh[5] == 0).all()) and bool((dh[M - 2] == 0).all()) and bool((dh[M - 1] != 0).any()), "gate edge rows"
    xref, xe = _out_expect(dh, down.t(), dout, alpha=1.0 / s)
    assert_within(dx, xref, xe, "dX")
    assert torch.equal(dx[5], dout[5])
    assert_within(dx16, dx.double() * s, 2 * U * (dx.double() * s).abs(), "fp16 copy of dX")      # (the copy is taken from the fp32 result)
    # saturation: a copy scale that carries part of the result past 65 504
    big = x.clone()
    big[:, 3] = 3.0e4
    big[:, 4] = -3.0e4
    cs = torch.tensor([4.0], device="cuda")
    o2, h2, c2 = ops.adapter_fused_h(big, down, up, copy_scale=cs, want_copy=True)
    assert bool(torch.isfinite(c2.float()).all()) and bool((c2[:, 3] == F16_MAX).all()) and bool((c2[:, 4] == -F16_MAX).all())
    assert_within(c2, o2.double() * 4.0, 2 * U * (o2.double() * 4.0).abs(), "saturating fp16 copy")
    assert_within(o2, *_out_expect(h2, up, big), "out beside a saturating copy")


@pytest.mark.parametrize("D,M", [(256, 8192 + 31), (512, 8192 + 1), (512, 8192 + 31), (768, 8192 + 15)])
def test_adapter_ln_random(D, M):
    """gd_adapter_fused_h_ln: adapter_persist_h_kernel<D, true>.  out / hidden as the plain form; the LayerNorm of the kernel's own stored out
    rows in fp64, with rows of large mean and one massive channel.  fp32 error of the two-reduction form: the mean to e_mu = C_ACC D u mean|x|,
    the centred values to e_mu + u |xc|, the variance relatively to C_ACC D u + 2 e_mu / sigma, rstd to half of that plus the 1-ulp rsqrt; then
    one fp16 rounding of y."""
    from gd_amd import ops
    x = _mk((M, D), _F32, D + M)
    x[:, 5] += 30.0
    x[: M // 4] += 4.0
    x[M - 1] += 50.0                                      # (the last row of the ragged tile)
    down, up = _mk((64, D), _F32, D + 1, 0.05).half(), _mk((D, 64), _F32, D + 2, 0.05).half()
    g, b = 1.0 + 0.2 * _mk((D,), _F32, D + 4), 0.3 * _mk((D,), _F32, D + 5)
    eps = 1e-6
    out, hid, y16, mean, rstd = ops.adapter_fused_h_ln(x, down, up, g, b, eps)
    href, he = _adapter_expect(x.half().double(), down, torch.relu)
    assert_within(hid, href, he, "hidden")
    assert_within(out, *_out_expect(hid, up, x), "out")
    o = out.double()
    mu = o.mean(1, keepdim=True)
    xc = o - mu
    var = (xc * xc).mean(1, keepdim=True)
    rs = (var + eps).rsqrt()
    e_mu = C_ACC * D * U * o.abs().mean(1, keepdim=True)
    e_rs_rel = 0.5 * (C_ACC * D * U + 2 * e_mu * var.sqrt() / (var + eps)) + 4 * U
    assert_within(mean, mu[:, 0], e_mu[:, 0], "row mean")
    assert_within(rstd, rs[:, 0], (rs * e_rs_rel)[:, 0], "row rstd")
    y = xc * rs * g.double() + b.double()
    ye = g.double().abs() * rs * (e_mu + U * xc.abs() + xc.abs() * e_rs_rel) + 4 * U * (y.abs() + b.double().abs())
    assert_within(y16, y, ye, "fp16 LayerNorm rows")


# ------------------------------------------------------------------------------------------------------------------------------------------
# c. LoRA B at the magnitudes training produces, through the formatting vit.py uses for the fused fp16 backward
# ------------------------------------------------------------------------------------------------------------------------------------------
def _fused_b_operand(b):
    """the fp16 B operand of the fused backward and the multiplier that undoes its shift on dt — vit.py's own helper, not a copy of it."""
    from gd_amd import vit
    return vit._opw_lora_b(b)


@pytest.mark.parametrize("dt_scaled", [False, True], ids=["dt_unscaled", "dt_scaled"])
@pytest.mark.parametrize("mag", B_MAGS)
def test_fused_lora_backward_dt_is_tf32_class_at_small_b(mag, dt_scaled):
    """dt = dqv . B^T on the one-pass kernel, B (f32, |B| ~ mag) formatted as the tf32h backward formats it, dqv the fp16 (dq, dv) block under the
    step's scale s = 2^12; against fp64 of the fp16 dqv and the fp32 B: 2^-10 |out_mul| |dqv| . |B|^T per element (B to 2^-11, the bound
    test_lora_backward_dt_is_tf32_class_at_small_b derives for the non-fused form), exactly 0 at B = 0; gbt does not see the shift.
    (B cast to fp16 as it is misses this bound at |B| ~ 1e-6: profiles/trainable_path_errors.txt.)"""
    from gd_amd import ops
    M, D = 8192 + 37, 768
    K, s = 2 * D, 4096.0
    sc = torch.tensor([s, 1.0 / s], device="cuda")
    dqv = (_mk((M, 3 * D), _F32, 5, 1e-4) * s).half()[:, :K]
    B = _mk((8, K), _F32, 6, mag)
    t = _mk((M, 8), _F32, 7, 0.3)
    bt16, dtm = _fused_b_operand(B)
    gbt = torch.zeros(8, K, device="cuda")
    dt = ops.lora_bwd_fused_h(dqv, t, bt16, gbt, out_mul=sc[1:2], dt_scaled=dt_scaled, dt_mul=dtm)
    om = 1.0 if dt_scaled else 1.0 / s
    ref = om * (dqv.double() @ B.double().t())
    bound = 2.0 ** -10 * om * (dqv.double().abs() @ B.double().abs().t()) + FLOOR[_F32]
    err = (dt.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"FUSED_DT mag={mag:g} dt_scaled={int(dt_scaled)} worst err/bound {worst:.3g}")
    if mag == 0.0:
        assert int(torch.count_nonzero(dt)) == 0
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"|B| ~ {mag:g}: {int(bad.sum())} of {bad.numel()} elements, first at {bad.nonzero()[0].tolist()}, worst err / bound {worst:.3g}"
    _, _, gref, ge = _lora_expect(dqv, t, None, torch.zeros_like(gbt), 1.0, 1.0 / s, False)
    assert_within(gbt, gref, ge, "gbt beside a shifted B")


@pytest.mark.parametrize("mag", [1e-6, 1e-5, 1e-3])
def test_batched_pack_keeps_small_lora_b_tf32_class(mag):
    """GDViT.prepare_trainables formats the (dq, dv) columns of every block's LoRA B once per step for the fused fp16 backward — the operand the
    full-size step reads.  Operand times the multiplier stored beside it equals B to fp16's 2^-11 per element (plus half the shifted subnormal
    spacing), at the magnitudes of a fine-tune's first steps: B cast without a shift is a subnormal there and misses this by orders of magnitude."""
    from gd_amd.finetune import FinetuneGD
    from gd_amd.vit import _unwrap
    torch.manual_seed(0)
    eng = FinetuneGD(r=4, variant="vggt", geometry="shared", dtype="tf32h", adapter_start_idx=4, bottleneck_dim=64, lora_b_std=mag,
                     backbone="vit_tiny_test", patch_size=14, img_size=56, teacher_patch=14).cuda()
    eng.model.prepare_trainables(None)
    try:
        packs = [tw for tw in (getattr(_unwrap(b)[0], "_tw", None) for b in eng.model.blocks) if tw is not None and "bt_qv_w3" in tw]
        assert packs, "no block carries a formatted LoRA B"
        for tw in packs:
            w16, mul, b = tw["bt_qv_w3"], tw["bt_qv_mul"], tw["bt_qv"].double()
            assert w16.dtype == _F16 and float(b.abs().max()) > 0
            assert_within((w16.double() * mul).float(), b, 2.0 ** -11 * b.abs() + 2.0 ** -25 * mul, f"|B| ~ {mag:g}: operand x multiplier")
    finally:
        eng.model.release_trainables()


# ------------------------------------------------------------------------------------------------------------------------------------------
# d. one block, end to end, at small B
# ------------------------------------------------------------------------------------------------------------------------------------------
def _tf32r(x):
    """fp64 -> the nearest TF32 value (10 explicit mantissa bits; the rounding of test_gpu_gemm.py's tf32 lambda), as fp64."""
    f = x.float().contiguous()
    return ((f.view(torch.int32) + 0x1000) & ~0x1FFF).view(torch.float32).double()


class _MMtf32(torch.autograd.Function):
    """a @ b in fp64 with both operands rounded to TF32 — in the forward and in both backward products (the gradient is an operand there)."""

    @staticmethod
    def forward(ctx, a, b):
        ar, br = _tf32r(a), _tf32r(b)
        ctx.save_for_backward(ar, br)
        return ar @ br

    @staticmethod
    def backward(ctx, g):
        ar, br = ctx.saved_tensors
        gr = _tf32r(g)
        return gr @ br.transpose(-1, -2), ar.transpose(-1, -2) @ gr


def _block64(x, P, mm, eps=1e-6):
    """fp64 restatement of one pre-LN block with q / v LoRA and the bottleneck adapter (oracle/gd_oracle.py vit_block has the arithmetic):
    every matrix product goes through mm."""
    B, Nt, D = x.shape
    H = D // 64
    xf = x.reshape(-1, D)
    y1 = F.layer_norm(xf, (D,), P["ln1w"], P["ln1b"], eps)
    qkv = mm(y1, P["wqkv"].t()) + P["bqkv"]
    dq = mm(mm(y1, P["aq"].t()), P["bq"].t())
    dv = mm(mm(y1, P["av"].t()), P["bv"].t())
    qkv = torch.cat([qkv[:, :D] + dq, qkv[:, D:2 * D], qkv[:, 2 * D:] + dv], 1)
    q, k, v = qkv.view(B, Nt, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    a = mm(torch.softmax(mm(q * 0.125, k.transpose(-1, -2)), -1), v)
    a = a.transpose(1, 2).reshape(B * Nt, D)
    x1 = xf + mm(a, P["wproj"].t()) + P["bproj"]
    y2 = F.layer_norm(x1, (D,), P["ln2w"], P["ln2b"], eps)
    h = F.gelu(mm(y2, P["w1"].t()) + P["b1"])
    x2 = x1 + mm(h, P["w2"].t()) + P["b2"]
    hd = torch.relu(mm(x2, P["down"].t()))
    return (x2 + mm(hd, P["up"].t())).view(B, Nt, D)


_BLOCK_TRAINED = ["aq", "av", "bq", "bv", "down", "up"]
BLOCK_RATIO = 2.0      # allowed Frobenius error against fp64, in units of the TF32 block's (see the test's docstring)


@pytest.mark.parametrize("h16_dy", [1, 0])
@pytest.mark.parametrize("mag", [0.0, 1e-6, 1e-5, 1e-4, 1e-3])
def test_block_gradients_are_tf32_class_at_small_b(mag, h16_dy):
    """A GDBlock with q / v LoRA (r = 4) and an adapter in the tf32h engine, D = 256, M = 32 x 257 = 8224 rows (the fused fp16 LoRA backward and
    the fused fp16 adapter both serve it), LoRA B ~ N(0, mag^2).  The gradients of A, B, down, up and the input against the fp64 block; the
    yardstick is the same fp64 block with every matmul operand — gradients included — rounded to TF32.  The engine's contract is "TF32-class":
    fp16 operands carry one more significand bit than TF32, so a ratio at or below 1 is expected from the products; BLOCK_RATIO = 2 leaves room
    for what the engine additionally stores as fp16 in the scaled domain (do, dqkv, dy with h16_dy) and the fitted GELU' of the fp16 fc1
    epilogue.  The constant comes from that reasoning, not from the measured ratios (profiles/trainable_path_errors.txt has those).

    Two operands are as small as B and need a power-of-two shift to stay out of fp16's subnormals: B itself in dt = dqv . B^T (vit._opw_lora_b) and
    dt as the split t operand of the LoRA-A gradient dt^T . LN(x) (vit.LORA_DT_TARGET); without either, the LoRA-A gradients miss this bound at
    |B| <= 1e-5."""
    import torch.nn as nn
    from gd_amd.model import Adapter, BlockWithAdapter, _LoRA_qkv
    from gd_amd.options import set_option
    from gd_amd.vit import GDBlock, run_block
    D, B, Nt, r = 256, 32, 257, 4
    torch.manual_seed(1234)
    blk = GDBlock(D, D // 64, 4.0, None, 1e-6)
    blk.split3 = "h"
    lin = lambda i, o: nn.Linear(i, o, bias=False)
    aq, bq, av, bv = lin(D, r), lin(r, D), lin(D, r), lin(r, D)
    with torch.no_grad():
        for w in (bq.weight, bv.weight):
            w.copy_(torch.randn_like(w) * mag)
        for ln in (blk.norm1, blk.norm2):
            ln.weight.add_(0.1 * torch.randn(D))
            ln.bias.add_(0.1 * torch.randn(D))
    blk.attn.qkv = _LoRA_qkv(blk.attn.qkv, aq, bq, av, bv)
    wrapped = BlockWithAdapter(blk, Adapter(D, 64)).cuda()
    g = torch.Generator(device="cuda").manual_seed(77)
    x = torch.randn(B, Nt, D, generator=g, device="cuda")
    w = torch.randn(B, Nt, D, generator=g, device="cuda") * 1e-4
    trained = {"aq": aq.weight, "av": av.weight, "bq": bq.weight, "bv": bv.weight, "down": wrapped.adapter.down.weight, "up": wrapped.adapter.up.weight}
    # ---- the engine
    xe = x.clone().requires_grad_(True)
    keep = set_option("h16_dy", h16_dy)
    try:
        out = run_block(wrapped, xe)
        assert out.dtype == _F32
        (out * w).sum().backward()
    finally:
        set_option("h16_dy", keep)
    got = {n: p.grad.detach().double() for n, p in trained.items()}
    got["x"] = xe.grad.detach().double()
    # ---- fp64, exact and with TF32 operands
    base = blk.attn.qkv.qkv
    frozen = {"ln1w": blk.norm1.weight, "ln1b": blk.norm1.bias, "ln2w": blk.norm2.weight, "ln2b": blk.norm2.bias, "wqkv": base.weight, "bqkv": base.bias,
              "wproj": blk.attn.proj.weight, "bproj": blk.attn.proj.bias, "w1": blk.mlp.fc1.weight, "b1": blk.mlp.fc1.bias,
              "w2": blk.mlp.fc2.weight, "b2": blk.mlp.fc2.bias}

    def grads(mm):
        P = {n: p.detach().double() for n, p in frozen.items()}
        P.update({n: p.detach().double().requires_grad_(True) for n, p in trained.items()})
        xd = x.double().requires_grad_(True)
        (_block64(xd, P, mm) * w.double()).sum().backward()
        res = {n: P[n].grad for n in _BLOCK_TRAINED}
        res["x"] = xd.grad
        return res
    ref = grads(torch.matmul)
    t32 = grads(_MMtf32.apply)
    fails = []
    for n in _BLOCK_TRAINED + ["x"]:
        assert bool(torch.isfinite(got[n]).all()), n
        eh, et, nr = float((got[n] - ref[n]).norm()), float((t32[n] - ref[n]).norm()), float(ref[n].norm())
        ratio = eh / et if et > 0 else (0.0 if eh == 0 else float("inf"))
        print(f"BLOCK_RATIO mag={mag:g} h16_dy={h16_dy} {n}: |ref| {nr:.3e} err tf32h {eh:.3e} err tf32 {et:.3e} ratio {ratio:.3f}")
        if not eh <= BLOCK_RATIO * et:
            fails.append(f"{n}: err {eh:.3e} against {BLOCK_RATIO:g} x {et:.3e} (ratio {ratio:.3g})")
    assert not fails, f"|B| ~ {mag:g}, h16_dy = {h16_dy}: " + "; ".join(fails)
