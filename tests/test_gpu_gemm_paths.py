"""Every gd_gemm_nt / gd_gemm_tn dispatch path against fp64, element by element.

The reference is the fp64 product of the operands AS THE KERNEL SEES THEM (the fp16 / bf16 tensors themselves; an fp32 operand that a kernel
rounds to fp16 on its way into LDS is rounded here the same way), computed on the GPU.  fp16 x fp16 and bf16 x bf16 products are exact in
fp32, so what is left is fp32 accumulation, the epilogue and the rounding of the output.  Every element is held to

    |C - C64| <= C_ACC * K * 2^-24 * (|alpha| |A| . |W|^T) + (epilogue terms) + ROUND[C] * |C64| + FLOOR[C]

A max-norm comparison cannot see a wrong 15-row tail or an epilogue term dropped on a few rows; this bound can.  Each case row names the
kernel it is there to reach, with the predicate of gemm_nt_impl / gemm_tn_impl (csrc/gemm.hip) that sends it there;
profiles/gemm_path_coverage.txt records the kernel trace of this file.
"""
import zlib

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# Recursive fp32 summation of K products has |error| <= K u sum|a b| (Higham's gamma_K, to first order).  The MFMA's adder tree and the
# blocked K loop only make the constant smaller; the factor 2 covers the alpha multiply, the ia = 1 / alpha of the LoRA chunk and the epilogue's
# own fp32 operations.  A typical error is ~sqrt(K) u |C|: the bound is loose against round-off and still ~500x tighter than |C| at K = 768,
# so any dropped term, wrong row or stale tile fails it.
C_ACC = 2.0
ROUND = {torch.float32: 4 * U, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # output rounding, relative (half an ulp)
FLOOR = {torch.float32: 1e-30, torch.bfloat16: 1e-30, torch.float16: 2.0 ** -25}        # fp16: half the subnormal spacing
OPS = {torch.float32: 8 * U, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}     # unit round-off of the rank-update operands (f32: scalar FMAs)
F16_MAX = 65504.0


def _mk(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(dtype)


def _gelu(v):
    return torch.nn.functional.gelu(v)


def _dgelu(v):
    return 0.5 * (1.0 + torch.erf(v * 0.7071067811865476)) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327


def _gelu_tol(cdt):
    """(|GELU| error, |GELU'| error) of the kernels' forms: 16-bit C uses the sigmoid-form fit (2.5e-5 / 1.1e-4 absolute, gd_common.h),
    fp32 C the erf form (__expf)."""
    return (4e-5, 1.5e-4) if cdt != torch.float32 else (3e-6, 3e-5)


def assert_within(got, ref, bound, what):
    """every element: |got - ref| <= bound + ROUND * |ref| + FLOOR; for fp16 results also finite, and +-65504 where the true value overflows."""
    dt = got.dtype
    g = got.double()
    if dt == torch.float16:
        assert bool(torch.isfinite(g).all()), f"{what}: non-finite fp16 output"
        ref = ref.clamp(-F16_MAX, F16_MAX)      # saturation: a true value past 65504 must store exactly +-65504
    tol = bound + ROUND[dt] * (ref.abs() + bound) + FLOOR[dt]
    err = (g - ref).abs()
    bad = ~(err <= tol)                         # (NaN fails)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        ratio = float((err / tol)[bad].max()) if bool(torch.isfinite(err[bad]).all()) else float("inf")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound (first at {idx}: got {float(g[tuple(idx)])!r}, "
                             f"fp64 {float(ref[tuple(idx)])!r}, bound {float(tol[tuple(idx)]):.3g}; worst err / bound {ratio:.3g})")


def _knobs(knobs):
    from gd_amd._lib import lib
    for name, val in knobs.items():
        assert lib().gd_debug_set(name.encode(), int(val)) == 0, name


_KNOB_DEFAULTS = {"gemm_persist": 1, "gemm_small_tiles": 0, "gemm_f32_big": 0, "reserve_cus": 0, "gemm_group_m": 1}


# ------------------------------------------------------------------------------------------------------------------------------------------
# gd_gemm_nt
# ------------------------------------------------------------------------------------------------------------------------------------------
def _nt_expect(a, w, *, alpha, alpha_dev, bias, lt, lb, act, preact_dt, dact, dsrc, res, acc0, cdt):
    """fp64 expected C (and preact) of gemm_nt with per-element error bounds (before output rounding)."""
    al = alpha * (float(alpha_dev[0]) if alpha_dev is not None else 1.0)
    K = a.shape[-1]
    ad, wd = a.double(), w.double()
    v = al * (ad @ wd.transpose(-1, -2))
    e = C_ACC * K * U * abs(al) * (ad.abs() @ wd.abs().transpose(-1, -2))
    if bias is not None:
        v = v + bias.double()
    if lt is not None:
        v = v + lt.double() @ lb.double()
        # rank 8 on 16-bit operands: the MFMA rank update rounds t / alpha and B to the operand type; rank < 8: fp32 FMAs
        ou = OPS[a.dtype] if lt.shape[1] == 8 else OPS[torch.float32]
        e = e + (2 * ou + 16 * U) * (lt.double().abs() @ lb.double().abs())
    e = e + 2 * U * v.abs()
    pre = pre_e = None
    g_t, dg_t = _gelu_tol(cdt)
    if preact_dt is not None:
        if act == 3:
            pre, pre_e = _dgelu(v), 0.8 * e + dg_t           # |GELU''| <= 0.8
        else:
            pre, pre_e = v.clone(), e.clone()
    if act in (1, 3):
        v, e = _gelu(v), 1.13 * e + g_t + 2 * U * v.abs()    # |GELU'| <= 1.13
    elif act == 2:
        v = v.clamp_min(0.0)
    if dact == 1:
        s = dsrc.double()
        v, e = v * _dgelu(s), e * 1.13 + dg_t * v.abs()
    elif dact == 2:
        v = torch.where(dsrc.double() > 0, v, torch.zeros_like(v))
    elif dact == 3:
        s = dsrc.double()
        v, e = v * s, e * s.abs() + 2 * U * (v * s).abs()
    if res is not None:
        v = v + res.double()
        e = e + 2 * U * v.abs()
    if acc0 is not None:
        v = v + acc0.double()
        e = e + 2 * U * v.abs()
    return v, e, pre, pre_e


# One row per path: id, operand dtype, C dtype, M, N, K, epilogue, knobs.  The epilogue keys: bias, lora (rank), alpha, alpha_dev, act,
# preact, dact, res, acc, batch, vecoff (an epilogue tensor whose row stride breaks 16-byte vectors), split, copy16.
_F16, _BF16, _F32 = torch.float16, torch.bfloat16, torch.float32
NT_CASES = [
    # ---- persistent gemm_nt_persist_kernel: big (K*es % 128 == 0, N >= 256, M >= 1024) && gemm_persist && pk && vec_epilogue && N % 8 == 0
    #      && (no LoRA || rank 8).  M % 256 in {1, 15, 255}, N % 256 == 8: a ragged last row tile and an 8-column last column tile.
    ("pk_bf16_plain_bf16c_bias_lora8", _BF16, _BF16, 1281, 264, 192, dict(bias=1, lora=8, alpha=0.5)),   # <bf16,0,0,0,false>
    ("pk_bf16_plain_f32c_bias", _BF16, _F32, 1295, 264, 192, dict(bias=1)),                              # <bf16,0,0,0,true>
    ("pk_bf16_gelu_bf16c", _BF16, _BF16, 2303, 264, 128, dict(bias=1, act=1)),                           # <bf16,0,1,0,false>
    ("pk_bf16_gelu3_f32c", _BF16, _F32, 1281, 264, 128, dict(bias=1, act=3)),                            # <bf16,0,1,0,true> (act 3 w/o preact)
    ("pk_bf16_gelu_preact_bf16c", _BF16, _BF16, 1295, 264, 128, dict(bias=1, act=1, preact=1)),          # <bf16,0,1,1,false>
    ("pk_bf16_gelu_dpre_bf16c", _BF16, _BF16, 2303, 264, 128, dict(bias=1, act=3, preact=1)),            # <bf16,0,1,2,false>
    ("pk_bf16_gelu_dpre_f32c", _BF16, _F32, 1281, 264, 128, dict(bias=1, act=3, preact=1)),              # <bf16,0,1,2,true>
    ("pk_bf16_dact1_bf16c", _BF16, _BF16, 1295, 264, 128, dict(dact=1)),                                 # <bf16,1,0,0,false>
    ("pk_bf16_dact3_bf16c", _BF16, _BF16, 2303, 264, 128, dict(dact=3)),                                 # <bf16,3,0,0,false>
    ("pk_bf16_dact3_f32c", _BF16, _F32, 1281, 264, 128, dict(dact=3)),                                   # <bf16,3,0,0,true>
    ("pk_bf16_res_bf16c", _BF16, _BF16, 1295, 264, 128, dict(bias=1, res=1)),                            # <bf16,2,0,0,false>
    ("pk_bf16_res_f32c", _BF16, _F32, 2303, 264, 128, dict(bias=1, res=1)),                              # <bf16,2,0,0,true>
    ("pk_bf16_split_gelu_dpre", _BF16, _F32, 1281, 264, 192, dict(bias=1, act=3, preact=1, split=1)),    # <bf16,0,1,2,true,0,1>
    ("pk_bf16_split_gelu", _BF16, _F32, 1295, 264, 192, dict(bias=1, act=1, split=1)),                   # <bf16,0,1,0,true,0,1>
    ("pk_bf16_split_dact3", _BF16, _F32, 2303, 264, 192, dict(dact=3, split=1)),                         # <bf16,3,0,0,true,0,1>
    ("pk_f16_plain_f16c_qkv_fwd", _F16, _F16, 1281, 264, 192, dict(bias=1, lora=8)),                     # GD_PK(0,0,0,false): vit.py QKV forward
    ("pk_f16_plain_f32c_lora8_alphadev", _F16, _F32, 1295, 264, 192, dict(lora=8, alpha_dev=2.0 ** -12)),   # GD_PK(0,0,0,true): QKV dX, f32 C
    ("pk_f16_plain_f16c_lora8_alphadev", _F16, _F16, 2303, 264, 192, dict(lora=8, alpha_dev=2.0 ** -12)),   # GD_PK(0,0,0,false): QKV dX, fp16 C
    ("pk_f16_plain_f16c", _F16, _F16, 1295, 264, 128, dict()),                                           # GD_PK(0,0,0,false): wproj_t / w1_t
    ("pk_f16_gelu_f16c", _F16, _F16, 1281, 264, 128, dict(bias=1, act=1)),                               # GD_PK(0,1,0,false)
    ("pk_f16_gelu_f32c", _F16, _F32, 1295, 264, 128, dict(bias=1, act=3)),                               # GD_PK(0,1,0,true)
    ("pk_f16_gelu_dpre_f16c", _F16, _F16, 2303, 264, 128, dict(bias=1, act=3, preact=1)),                # GD_PK(0,1,2,false): tf32h fc1
    ("pk_f16_gelu_dpre_f32c", _F16, _F32, 1281, 264, 128, dict(bias=1, act=3, preact=1)),                # GD_PK(0,1,2,true)
    ("pk_f16_dact3_f16c", _F16, _F16, 1295, 264, 128, dict(dact=3)),                                     # GD_PK(3,0,0,false)
    ("pk_f16_dact3_f32c", _F16, _F32, 2303, 264, 128, dict(dact=3, alpha_dev=0.25)),                     # GD_PK(3,0,0,true)
    ("pk_f16_res_f32c", _F16, _F32, 1281, 264, 128, dict(bias=1, res=1, alpha_dev=0.5)),                 # GD_PK(2,0,0,true)
    ("pk_f16_copy16", _F16, _F32, 1295, 264, 128, dict(bias=1, res=1, copy16=1, alpha_dev=0.5)),         # GD_PK(2,0,3,true): gemm_nt_copy16
    # several tiles per block: 37 x 3 = 111 tiles on 256 - 200 = 56 CUs
    ("pk_f16_multitile_reserve_cus", _F16, _F32, 256 * 37 + 15, 768, 128, dict(bias=1, lora=8, knobs={"reserve_cus": 200})),
    ("pk_bf16_multitile_reserve_cus", _BF16, _BF16, 256 * 37 + 1, 768, 128, dict(bias=1, act=3, preact=1, knobs={"reserve_cus": 200})),
    # ---- staged gemm_nt_kernel<T,2,4,8>: big but not persist_ok
    ("big_f16_lora4", _F16, _F16, 1295, 264, 128, dict(bias=1, lora=4)),                                 # rank != 8: scalar LoRA epilogue
    ("big_f16_vecoff_res", _F16, _F32, 1281, 264, 128, dict(res=1, vecoff=1)),                           # ldr*es % 16 != 0: !vec_epilogue
    ("big_f16_acc_lora8", _F16, _F32, 1281, 264, 128, dict(bias=1, lora=8, acc=1)),                      # accumulate: pk = null; MFMA rank update
    ("big_f16_gelu_preact", _F16, _F32, 1295, 264, 128, dict(bias=1, act=1, preact=1)),                  # act 1 + preact: no f16 pk
    ("big_f16_dact1_f16c", _F16, _F16, 2303, 264, 128, dict(dact=1)),                                    # dact 1: no f16 pk
    ("big_f16_dact2_f32c", _F16, _F32, 1281, 264, 128, dict(dact=2, act=2)),                             # dact 2, ReLU
    ("big_bf16_lora4", _BF16, _BF16, 1295, 264, 128, dict(bias=1, lora=4)),
    ("big_bf16_acc", _BF16, _F32, 1281, 264, 128, dict(bias=1, lora=8, acc=1)),
    ("big_f32_knob", _F32, _F32, 1281, 264, 64, dict(bias=1, lora=8, act=1, knobs={"gemm_f32_big": 1})),   # f32: only with gemm_f32_big
    # ---- staged gemm_nt_kernel<T,2,2,4>: K*es % 128 == 0 and not big (M < 1024 or N < 256)
    ("dma_f16_lora8_gelu_dpre", _F16, _F16, 1000, 264, 192, dict(bias=1, lora=8, act=3, preact=1)),
    ("dma_f16_f32c_res_acc", _F16, _F32, 1000, 200, 192, dict(bias=1, lora=8, res=1, acc=1, alpha_dev=0.5)),
    ("dma_bf16_lora8", _BF16, _BF16, 999, 200, 128, dict(bias=1, lora=8, act=1, res=1)),
    ("dma_f32_lora3", _F32, _F32, 1000, 200, 96, dict(bias=1, lora=3, dact=1)),
    # ---- gemm_nt_regstage_kernel<T>: K*es % 128 != 0
    ("reg_f16_k72", _F16, _F16, 1300, 264, 72, dict(bias=1, lora=8, act=3, preact=1)),
    ("reg_f16_k72_f32c_acc", _F16, _F32, 777, 136, 72, dict(bias=1, lora=5, dact=3, res=1, acc=1, alpha_dev=0.25)),
    ("reg_bf16_k72", _BF16, _BF16, 1300, 264, 72, dict(bias=1, lora=8, act=1, preact=1)),
    ("reg_f32_k36", _F32, _F32, 777, 136, 36, dict(bias=1, lora=8, dact=2, acc=1)),
    # ---- batched (grid.y = batch; the 256 x 256 kernels from M >= gemm_batch_big_m = 384)
    ("batch_f32_m383", _F32, _F32, 383, 264, 64, dict(batch=3)),                                         # <float,2,2,4>
    ("batch_f32_m384", _F32, _F32, 384, 264, 64, dict(batch=3)),                                         # <float,2,2,4> (no f32 big)
    ("batch_bf16_m383", _BF16, _F32, 383, 264, 128, dict(batch=3)),                                      # <bf16,2,2,4>
    ("batch_bf16_m384", _BF16, _F32, 384, 264, 128, dict(batch=3)),                                      # persistent <bf16,0,0,0,true>
    ("batch_bf16_m1000", _BF16, _BF16, 1000, 264, 128, dict(batch=2)),                                   # persistent <bf16,0,0,0,false>
    ("batch_f16_m383", _F16, _F16, 383, 264, 128, dict(batch=3)),                                        # <f16,2,2,4>
    ("batch_f16_m384", _F16, _F32, 384, 264, 128, dict(batch=3)),                                        # persistent GD_PK(0,0,0,true)
    ("batch_f16_m1000", _F16, _F16, 1000, 264, 128, dict(batch=2, alpha_dev=0.5)),                       # persistent GD_PK(0,0,0,false)
    ("batch_f16_m1000_small", _F16, _F16, 1000, 264, 128, dict(batch=2, knobs={"gemm_persist": 0})),     # <f16,2,4,8> batched
]


def _run_nt_case(dt, cdt, M, N, K, ep, seed):
    from gd_amd import ops
    B = ep.get("batch", 1)
    shp = (B, M, K) if B > 1 else (M, K)
    a = _mk(shp, dt, seed)
    w = _mk((B, N, K) if B > 1 else (N, K), dt, seed + 1, 1.0 / 16)
    # side tensors have C's dtype (fp32 when C is the split output)
    sdt = cdt
    kw = dict(out_dtype=cdt)
    bias = _mk((N,), _F32, seed + 2) if ep.get("bias") else None
    lt = lb = None
    if ep.get("lora"):
        r = ep["lora"]
        lt, lb = _mk((M, r), _F32, seed + 3), _mk((r, N), _F32, seed + 4, 0.1)
    alpha = ep.get("alpha", 1.0)
    alpha_dev = torch.tensor([ep["alpha_dev"]], device="cuda") if "alpha_dev" in ep else None
    act, dact = ep.get("act", 0), ep.get("dact", 0)

    def side(sd):
        if ep.get("vecoff"):      # rows of N + 1 elements: the tensor is a [:, :N] view whose row stride breaks 16-byte vectors
            return _mk((M, N + 1), sdt, sd)[:, :N]
        return _mk((M, N), sdt, sd)
    dsrc = side(seed + 5) if dact else None
    res = side(seed + 6) if ep.get("res") else None
    acc0 = None
    out = None
    if ep.get("acc"):
        acc0 = _mk((M, N), cdt, seed + 7)
        out = acc0.clone()
    pre = torch.empty(M, N, dtype=sdt, device="cuda") if ep.get("preact") else None
    v, e, pv, pe = _nt_expect(a, w, alpha=alpha, alpha_dev=alpha_dev, bias=bias, lt=lt, lb=lb, act=act, preact_dt=sdt if pre is not None else None,
                              dact=dact, dsrc=dsrc, res=res, acc0=acc0, cdt=cdt)
    if ep.get("copy16"):
        cs = torch.tensor([0.25], device="cuda")
        got, c16 = ops.gemm_nt_copy16(a, w, res, bias=bias, alpha=alpha, alpha_dev=alpha_dev, copy_scale=cs)
        return [("C", got, v, e), ("copy16", c16, v * 0.25, e * 0.25)]
    if ep.get("split"):
        got = ops.gemm_nt(a, w, bias=bias, lora_t=lt, lora_b=lb, preact=pre, act=act, dact_src=dsrc, dact=dact, residual=res, alpha=alpha,
                          alpha_dev=alpha_dev, out_split=True)
        hi, lo, hi2 = got[:, :N], got[:, N:2 * N], got[:, 2 * N:]
        assert torch.equal(hi, hi2), "split: the two hi planes differ"
        f = (hi.double() + lo.double()).float()      # the f32 result the split came from, to 2^-16
        checks = [("C(hi+lo)", f, v, e + 2.0 ** -16 * v.abs())]
    else:
        got = ops.gemm_nt(a, w, out=out, bias=bias, lora_t=lt, lora_b=lb, preact=pre, act=act, dact_src=dsrc, dact=dact, residual=res,
                          accumulate=bool(ep.get("acc")), alpha=alpha, alpha_dev=alpha_dev, **({} if out is not None else kw))
        assert got.dtype == cdt
        checks = [("C", got, v, e)]
    if pre is not None:
        checks.append(("preact", pre, pv, pe))
    return checks


@pytest.mark.parametrize("case", NT_CASES, ids=[c[0] for c in NT_CASES])
def test_gemm_nt_path(case):
    name, dt, cdt, M, N, K, ep = case
    knobs = ep.get("knobs", {})
    try:
        _knobs(knobs)
        checks = _run_nt_case(dt, cdt, M, N, K, ep, seed=zlib.crc32(name.encode()) % 10000)
    finally:
        _knobs({k: _KNOB_DEFAULTS[k] for k in knobs})
    for what, got, ref, bound in checks:
        assert_within(got, ref, bound, f"{name} {what}")


def test_gemm_nt_fp16_output_saturates():
    """fp16 C: a true value past fp16's range stores +-65504 (the next product's operand stays finite), on the persistent kernel, the
    staged 128-tile kernel and the register-staged one; the rest of the tile is unaffected."""
    from gd_amd import ops
    for M, N, K in [(1281, 264, 128), (300, 136, 128), (300, 136, 72)]:
        a, w = _mk((M, K), _F16, 5), _mk((N, K), _F16, 6, 1.0 / 16)
        bias = torch.zeros(N, device="cuda")
        bias[::3] = 1.0e5
        bias[1::3] = -7.0e4
        got = ops.gemm_nt(a, w, bias=bias, out_dtype=_F16)
        v, e, _, _ = _nt_expect(a, w, alpha=1.0, alpha_dev=None, bias=bias, lt=None, lb=None, act=0, preact_dt=None, dact=0, dsrc=None,
                                res=None, acc0=None, cdt=_F16)
        assert bool((got[:, ::3] == F16_MAX).all()) and bool((got[:, 1::3] == -F16_MAX).all()), (M, N, K)
        assert_within(got, v, e, f"saturation {M}x{N}x{K}")


# ---- skinny streaming kernel: (bf16 | fp16 operands with f32 C), N <= 8, M >= 4096, K % 128 == 0, K <= 4096, no epilogue tensors
SKINNY = [  # (operands, C, M, N, K, alpha_dev, strided A, strided C)
    (_BF16, _BF16, 4096, 8, 768, None, False, False),        # gemm_nt_skinny_kernel<bf16>
    (_BF16, _BF16, 4097, 1, 2304, None, True, True),
    (_BF16, _F32, 8192 + 31, 7, 128, 0.5, False, True),       # gemm_nt_skinny_kernel<float>
    (_BF16, _F32, 4097, 4, 768, None, True, False),
    (_F16, _F32, 4096, 8, 2304, 2.0 ** -12, True, True),     # gemm_nt_skinny_kernel<float, f16>: the tf32h LoRA-A projection / dt
    (_F16, _F32, 8192 + 31, 8, 768, 2.0 ** -12, False, False),
    (_F16, _F32, 4097, 1, 128, None, False, True),
    (_F16, _F32, 4096, 7, 768, 0.25, True, False),
]


@pytest.mark.parametrize("dt,cdt,M,N,K,adev,sa,sc", SKINNY)
def test_gemm_nt_skinny_paths(dt, cdt, M, N, K, adev, sa, sc):
    from gd_amd import ops
    a = _mk((M, K + 64), dt, M + N)[:, 32:32 + K] if sa else _mk((M, K), dt, M + N)
    w = _mk((N, K), dt, K + N, 1.0 / 16)
    alpha_dev = torch.tensor([adev], device="cuda") if adev is not None else None
    if sc:     # a column slice of a wider output: the columns around it are left alone
        big = torch.full((M, N + 11), 123.0, dtype=cdt, device="cuda")
        out = big[:, 3:3 + N]
        ops.gemm_nt(a, w, out=out, alpha=0.5, alpha_dev=alpha_dev)
        assert bool((big[:, :3] == 123.0).all()) and bool((big[:, 3 + N:] == 123.0).all())
    else:
        out = ops.gemm_nt(a, w, out_dtype=cdt, alpha=0.5, alpha_dev=alpha_dev)
    v, e, _, _ = _nt_expect(a, w, alpha=0.5, alpha_dev=alpha_dev, bias=None, lt=None, lb=None, act=0, preact_dt=None, dact=0, dsrc=None, res=None,
                            acc0=None, cdt=cdt)
    assert_within(out, v, e, f"skinny {dt} -> {cdt} {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------------------------------------------------------
# gd_gemm_tn: G[N, K] (+)= alpha * Y[M, N]^T X[M, K]
# ------------------------------------------------------------------------------------------------------------------------------------------
TN_CASES = [  # (id, Y dtype, X dtype, M, N, K, batch, alpha_dev, accumulate)
    ("f32_kernel", _F32, _F32, 1000, 200, 72, 1, None, False),              # gemm_tn_kernel (64 tiles)
    ("f32_kernel_batch_acc", _F32, _F32, 777, 72, 136, 2, 0.5, True),
    ("mixed_f32_bf16", _F32, _BF16, 1500, 200, 776, 1, None, True),         # no 16-bit MFMA form for mixed f32 / bf16: gemm_tn_kernel
    ("bf16", _BF16, _BF16, 3001, 200, 776, 1, None, False),                 # gemm_tn_bf16_kernel<bf16>: ragged N / K against 128
    ("bf16_batch_acc", _BF16, _BF16, 1000, 72, 200, 3, 0.25, True),
    ("h16", _F16, _F16, 3001, 200, 776, 1, 2.0 ** -12, False),             # gemm_tn_bf16_kernel<f16> (h16)
    ("h16_batch_acc", _F16, _F16, 1000, 776, 72, 2, None, True),
    ("hy32", _F32, _F16, 3001, 72, 200, 1, 2.0 ** -12, True),              # <f16, true, false>: Y f32 rounded to fp16 under 1 / alpha_dev
    ("hy32_big", _F32, _F16, 1000, 776, 200, 1, 0.5, False),
    ("hy32_plain", _F32, _F16, 700, 200, 72, 1, None, False),
    ("hx32", _F16, _F32, 3001, 200, 72, 1, 2.0 ** -12, True),              # <f16, false, true>: X f32 rounded to fp16
    ("hx32_batch", _F16, _F32, 1000, 72, 776, 2, None, False),
    ("f16_small_n", _F16, _F16, 1000, 8, 200, 1, 0.5, True),               # fp16, N < 64: gemm_tn_kernel
    ("f16_small_k", _F16, _F16, 1000, 200, 32, 1, None, False),            # fp16, K < 64: gemm_tn_kernel
    ("f16_y32_small_k", _F32, _F16, 1000, 200, 32, 1, None, False),        # f32 / fp16, K < 64: gemm_tn_kernel
    # skinny LoRA-gradient kernel: N == 8, ldy == 8, Y f32, batch 1, K <= 2560; narrow (K <= 1024: 8 row groups) or wide (3 groups).  M % 8 != 0:
    # the last row group ends in single rows.  (At M ~ 2000 the M u |Y|^T|X| bound is below one row's |y x|, so a dropped row fails it; the
    # 87 680-row case is the production size.)
    ("skinny_f32_narrow", _F32, _F32, 2000 + 5, 8, 768, 1, None, True),
    ("skinny_f32_wide", _F32, _F32, 2000 + 13, 8, 2304, 1, 0.5, False),
    ("skinny_bf16_narrow", _F32, _BF16, 2000 + 5, 8, 768, 1, 0.5, False),
    ("skinny_bf16_wide", _F32, _BF16, 2000 + 13, 8, 2304, 1, None, True),
    ("skinny_f16_narrow", _F32, _F16, 87680 + 5, 8, 768, 1, 2.0 ** -12, True),    # tf32h LoRA-A gradient (vit.py)
    ("skinny_f16_wide", _F32, _F16, 2000 + 13, 8, 2304, 1, 2.0 ** -12, False),
]


@pytest.mark.parametrize("case", TN_CASES, ids=[c[0] for c in TN_CASES])
def test_gemm_tn_path(case):
    from gd_amd import ops
    name, ydt, xdt, M, N, K, B, adev, accumulate = case
    lead = (B,) if B > 1 else ()
    y = _mk(lead + (M, N), ydt, M + 1, 1e-3 if ydt == _F32 and adev else 1.0)   # (a gradient-sized Y goes in with its 1 / alpha_dev)
    x = _mk(lead + (M, K), xdt, M + 2)
    alpha_dev = torch.tensor([adev], device="cuda") if adev is not None else None
    al = 0.75 * (adev if adev is not None else 1.0)
    # the operands as the kernel sees them: in the fp16 MFMA form an f32 operand is rounded to fp16 — Y times 1 / alpha_dev, the scale that
    # alpha_dev then undoes (there G = alpha Y^T X: the gradient goes in unscaled and is scaled into fp16's range in the kernel)
    yd, xd = y.double(), x.double()
    f16_mma = N >= 64 and K >= 64 and not (N == 8 and ydt == _F32)
    if f16_mma and ydt == _F32 and xdt == _F16:
        yd = (y * (1.0 / adev if adev is not None else 1.0)).half().double()
    if f16_mma and ydt == _F16 and xdt == _F32:
        xd = x.half().double()
    out0 = _mk(lead + (N, K), _F32, M + 3) if accumulate else None
    got = ops.gemm_tn(y, x, out=out0.clone() if accumulate else None, alpha=0.75, alpha_dev=alpha_dev)
    ref = al * (yd.transpose(-1, -2) @ xd)
    e = C_ACC * M * U * abs(al) * (yd.abs().transpose(-1, -2) @ xd.abs()) + 2 * U * ref.abs()
    if accumulate:
        ref = ref + out0.double()
        e = e + 2 * U * ref.abs()
    assert_within(got, ref, e, f"gemm_tn {name}")


# ------------------------------------------------------------------------------------------------------------------------------------------
# The LoRA rank update at the magnitudes of LoRA B in a fine-tune's first steps (B starts at 0 and moves by ~lr = 1e-5 per AdamW step)
# ------------------------------------------------------------------------------------------------------------------------------------------
B_MAGS = [0.0, 1e-6, 1e-5, 1e-4, 1e-2]


def _lora_delta_check(got_l, got_0, lt, lb, what):
    """C(lora) - C(no lora) of one kernel against t . B in fp64: 2^-10 |t| . |B| per element (TF32-class: t and B each to 2^-11), plus the
    rounding of the two outputs."""
    tb = lt.double() @ lb.double()
    d = got_l.double() - got_0.double()
    bound = 2.0 ** -10 * (lt.double().abs() @ lb.double().abs())
    for g in (got_l, got_0):
        bound = bound + ROUND[g.dtype] * g.double().abs() + FLOOR[g.dtype]
    err = (d - tb).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        r = float((err / bound.clamp_min(1e-300))[bad].max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements, worst err / bound {r:.3g}")


@pytest.mark.parametrize("M", [1295, 1000], ids=["persistent", "staged"])
@pytest.mark.parametrize("mag", B_MAGS)
def test_lora_rank_update_is_tf32_class_at_small_b(M, mag):
    """fp16 operands, rank-8 LoRA folded into the MFMA accumulators (gemm_nt, lora_rt == 8): t of O(1), B from 0 to 1e-2.  The main product is
    zero (W = 0) so the difference of the two calls is the rank update alone.  Forward form: bias + fp16 C (vit.py QKV), with a bias of B's
    size so fp16 C can show the term; backward form: alpha_dev = 2^-12 (t / alpha is then t * 4096), f32 and fp16 C.  (B rounded to fp16 as it
    is failed this from 1e-4 down; the kernels now shift B by a power of two first: f16_lora_shift, gd_common.h.)"""
    from gd_amd import ops
    N, K = 264, 128
    a = _mk((M, K), _F16, 1)
    w = torch.zeros(N, K, dtype=_F16, device="cuda")
    lt = _mk((M, 8), _F32, 2)
    lb = _mk((8, N), _F32, 3, mag)
    adev = torch.tensor([2.0 ** -12], device="cuda")
    bias = _mk((N,), _F32, 4, max(mag, 1e-30))
    for kw, what in [(dict(bias=bias, out_dtype=_F16), "forward, bias + fp16 C"),
                     (dict(alpha_dev=adev, out_dtype=_F32), "backward, alpha_dev, f32 C"),
                     (dict(alpha_dev=adev, out_dtype=_F16), "backward, alpha_dev, fp16 C")]:
        c0 = ops.gemm_nt(a, w, **kw)
        cl = ops.gemm_nt(a, w, lora_t=lt, lora_b=lb, **kw)
        _lora_delta_check(cl, c0, lt, lb, f"|B| ~ {mag:g}, {what}")


@pytest.mark.parametrize("mag", B_MAGS)
def test_lora_backward_dt_is_tf32_class_at_small_b(mag):
    """The backward's dt = dqkv . Bt^T as the tf32h engine builds it: Bt (LoRA B, [2r, 3D] with the dk third zero) through vit._opw ("h") then
    the skinny fp16 gemm_nt with the gradient's alpha_dev; against fp64 of the fp16 dqkv and the fp32 B."""
    from gd_amd import ops
    from gd_amd import vit
    M, D, r = 4096 + 7, 768, 4
    dq = _mk((M, 3 * D), _F16, 5)
    btz = torch.zeros(2 * r, 3 * D, device="cuda")
    btz[:, :2 * D] = _mk((2 * r, 2 * D), _F32, 6, mag)
    adev = torch.tensor([2.0 ** -12], device="cuda")
    w16, walpha = vit._opw_lora_b(btz)
    dt = ops.gemm_nt(dq, w16, out_dtype=_F32, alpha=walpha, alpha_dev=adev)
    ref = 2.0 ** -12 * (dq.double() @ btz.double().t())
    bound = 2.0 ** -10 * 2.0 ** -12 * (dq.double().abs() @ btz.double().abs().t()) + FLOOR[_F32]
    err = (dt.double() - ref).abs()
    assert bool((err <= bound).all()), f"|B| ~ {mag:g}: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3g}"
    assert rel_err(dt, ref) < 2.0 ** -10 or mag == 0.0
