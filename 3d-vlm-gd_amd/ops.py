"""Thin tensor-level wrappers over the C ABI (include/gd_hip.h).  Caller-owned memory, current
stream, no hidden allocation inside the library: outputs and workspaces are torch.empty here."""
import torch

from . import _lib
from ._lib import check, dtype_code, lib, ptr, stream
from .options import option


def _req(cond, msg):
    if not cond:
        raise _lib.GdHipError(msg)


class GemmProfiler:
    """HIP-event bracket around every gd_gemm_nt launch on the current stream (bench.py's roofline leg)."""

    def __init__(self):
        self.records = []

    def totals(self, keep=None):
        """(FLOPs, ms, launches) over the recorded launches; keep(tag) with tag = (M, N, K, B, epilogue, out dtype, operand
        dtype) selects a subset (e.g. the launches that run on the persistent MFMA kernel, leaving out the HBM-bound N <= 8
        streaming launches)."""
        torch.cuda.synchronize()
        recs = [r for r in self.records if keep is None or keep(r[3])]
        flops = sum(r[2] for r in recs)
        ms = sum(r[0].elapsed_time(r[1]) for r in recs)
        return flops, ms, len(recs)

    def roofline_time(self, keep, peak_flops, peak_bytes):
        """(sum over the kept launches of max(FLOPs / peak_flops, algorithmic bytes / peak_bytes) in ms, measured ms, launches whose bound is the
        byte term, launches).  Algorithmic bytes of a launch: both operands once, C once, every [M, N] epilogue tensor (preact, dact_src,
        residual, the accumulate read) once — what the launch must move if nothing is re-read."""
        torch.cuda.synchronize()
        es = {"float32": 4, "bfloat16": 2, "float16": 2}
        lim = ms = 0.0
        nb = n = 0
        for e0, e1, fl, tag in self.records:
            if keep is not None and not keep(tag):
                continue
            M, N, K, B, epi, odt, adt = tag
            nt = sum(epi.split("a")[0].count(c) for c in "pdr") + (1 if epi.endswith("+") else 0)
            by = B * (M * K + N * K) * es[adt] + B * M * N * es[odt] * (1 + nt)
            tf, tb = fl / peak_flops, by / peak_bytes
            lim += max(tf, tb) * 1e3
            nb += tb > tf
            ms += e0.elapsed_time(e1)
            n += 1
        return lim, ms, nb, n

    def algorithmic_bytes(self, keep=None):
        """(sum of the kept launches' algorithmic bytes — both operands once, C once, every [M, N] epilogue tensor once, as roofline_time counts
        them — and the number of launches)."""
        es = {"float32": 4, "bfloat16": 2, "float16": 2}
        tot = n = 0
        for _, _, _, tag in self.records:
            if keep is not None and not keep(tag):
                continue
            M, N, K, B, epi, odt, adt = tag
            nt = sum(epi.split("a")[0].count(c) for c in "pdr") + (1 if epi.endswith("+") else 0)
            tot += B * (M * K + N * K) * es[adt] + B * M * N * es[odt] * (1 + nt)
            n += 1
        return tot, n

    def by_shape(self):
        """{(M, N, K, B, epilogue tag): (launches, ms, TFLOP/s)} — where the step's GEMM time goes."""
        torch.cuda.synchronize()
        acc = {}
        for r in self.records:
            n, ms, fl = acc.get(r[3], (0, 0.0, 0.0))
            acc[r[3]] = (n + 1, ms + r[0].elapsed_time(r[1]), fl + r[2])
        return {k: (n, ms, fl / ms / 1e9 if ms > 0 else 0.0) for k, (n, ms, fl) in acc.items()}


_PROFILER = None


def set_gemm_profiler(p):
    global _PROFILER
    _PROFILER = p


def time_on_stream(fn, warm=2, iters=5):
    """seconds per call, HIP events on the current stream."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def gemm_nt(a, w, out=None, *, out_dtype=None, alpha=1.0, bias=None, lora_t=None, lora_b=None, preact=None,
            act=0, dact_src=None, dact=0, residual=None, accumulate=False, out_split=False, alpha_dev=None):
    """out[M,N] = epilogue(alpha * a[M,K] @ w[N,K]^T).  a, w: same dtype (f32 | bf16), last dim contiguous.
    Batched when a is 3-D ([B,M,K] x [B,N,K] -> [B,M,N], no epilogue tensors).
    Epilogue order: +bias[N] (f32) -> +lora_t[M,r] @ lora_b[r,N] (f32) -> store preact -> act (1 GELU, 2 ReLU,
    3 GELU with `preact` receiving GELU'(v)) -> *act'(dact_src) (1 dGELU(pre), 2 src>0, 3 v *= src) -> +residual
    -> +out (accumulate).
    out_split: the f32 result leaves as its bf16 operand split [M, 3N] = [hi | lo | hi] (what split3(out, "a") would give: the left
    operand of the next tf32x GEMM) without the f32 tensor ever reaching memory; preact / dact_src stay f32.  split_out_ok() says
    whether a shape is served.
    fp16 operands (tf32h engine, `cast16`): f32 results with f32 epilogue tensors, or out_dtype=torch.float16 — fp16 C (saturated), preact, dact_src;
    alpha_dev: a device scalar multiplied into alpha (the 1/s of an operand scaled by `amax_scale`)."""
    _req(a.is_cuda and w.is_cuda and a.dtype == w.dtype, "gemm_nt: a and w must be CUDA tensors of one dtype")
    _req(a.stride(-1) == 1 and w.stride(-1) == 1, "gemm_nt: a and w must be contiguous along K")
    batched = a.dim() == 3
    if batched:
        B, M, K = a.shape
        N = w.shape[1]
        _req(w.shape[0] == B and w.shape[2] == K, "gemm_nt: batched shape mismatch")
        sA, sW, lda, ldw = a.stride(0), w.stride(0), a.stride(1), w.stride(1)
    else:
        (M, K), N, B = a.shape, w.shape[0], 1
        _req(w.shape[1] == K, f"gemm_nt: K mismatch {a.shape} x {w.shape}")
        sA = sW = 0
        lda, ldw = a.stride(0), w.stride(0)
    if out_split:
        _req(out is None and not batched and a.dtype == torch.bfloat16, "gemm_nt: out_split takes bf16 (split) operands, 2-D, and allocates its output")
        out = torch.empty(M, 3 * N, dtype=torch.bfloat16, device=a.device)
    if out is None:
        odt = out_dtype or a.dtype
        out = torch.empty((B, M, N) if batched else (M, N), dtype=odt, device=a.device)
    _req(out.stride(-1) == 1, "gemm_nt: out must be contiguous along N")
    cdt = F32X3 if out_split else dtype_code(out)
    sdt = torch.float32 if out_split else out.dtype
    for t, name in ((preact, "preact"), (dact_src, "dact_src"), (residual, "residual")):
        if t is not None:
            _req(t.dtype == sdt and t.stride(-1) == 1 and tuple(t.shape) == (M, N), f"gemm_nt: bad {name}")
    for t, name in ((bias, "bias"), (lora_t, "lora_t"), (lora_b, "lora_b")):
        if t is not None:
            _req(t.dtype == torch.float32 and t.is_contiguous(), f"gemm_nt: {name} must be contiguous fp32")
    rt = 0
    if lora_t is not None:
        rt = lora_t.shape[1]
        _req(tuple(lora_t.shape) == (M, rt) and tuple(lora_b.shape) == (rt, N), "gemm_nt: bad lora shapes")
    if _PROFILER is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    tail = (ptr(bias), ptr(lora_t), ptr(lora_b), rt, ptr(preact), preact.stride(0) if preact is not None else 0, int(act),
            ptr(dact_src), dact_src.stride(0) if dact_src is not None else 0, int(dact), ptr(residual),
            residual.stride(0) if residual is not None else 0, 1 if accumulate else 0, stream())
    head = (ptr(a), ptr(w), ptr(out), M, N, K, lda, ldw, out.stride(-2), B, sA, sW, out.stride(0) if batched else 0, dtype_code(a), cdt,
            float(alpha))
    if alpha_dev is not None:
        _req(alpha_dev.is_cuda and alpha_dev.dtype == torch.float32 and alpha_dev.numel() >= 1, "gemm_nt: alpha_dev must be a CUDA fp32 scalar")
        rc = lib().gd_gemm_nt_scaled(*head, ptr(alpha_dev), *tail)
    else:
        rc = lib().gd_gemm_nt(*head, *tail)
    if _PROFILER is not None:
        e1.record()
        tag = "".join(c for c, t in (("b", bias), ("l", lora_t), ("p", preact), ("d", dact_src), ("r", residual)) if t is not None)
        _PROFILER.records.append((e0, e1, 2.0 * M * N * K * B, (M, N, K, B, f"{tag}a{act}{'+' if accumulate else ''}", str(out.dtype)[6:], str(a.dtype)[6:])))
    check(rc, "gd_gemm_nt")
    return out


def split_out_ok(M, N, K3):
    """Shapes gemm_nt(..., out_split=True) serves (the persistent kernel's: gd_gemm_nt, c_dtype GD_F32X3)."""
    return M >= 1024 and N >= 256 and N % 8 == 0 and K3 % 64 == 0


def gemm_nt_copy16(a, w, residual, *, bias=None, alpha=1.0, alpha_dev=None, copy_scale=None):
    """fp16 operands: out [M,N] f32 = alpha * alpha_dev * a.w^T + bias + residual, and copy [M,N] fp16 = sat(out * copy_scale[0]) from the same
    epilogue — the residual-stream result plus the operand the next tf32h product takes (gd_gemm_nt_copy16; copy16_ok() says which shapes)."""
    _req(a.dtype == torch.float16 and w.dtype == torch.float16 and a.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1 and
         residual.dtype == torch.float32 and residual.stride(1) == 1, "gemm_nt_copy16: fp16 operands, fp32 residual")
    (M, K), N = a.shape, w.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    copy = torch.empty(M, N, dtype=torch.float16, device=a.device)
    check(lib().gd_gemm_nt_copy16(ptr(a), ptr(w), ptr(out), M, N, K, a.stride(0), w.stride(0), N, float(alpha), ptr(alpha_dev), ptr(bias),
                                  ptr(residual), residual.stride(0), ptr(copy), N, ptr(copy_scale), stream()), "gd_gemm_nt_copy16")
    return out, copy


def copy16_ok(M, N, K):
    return M >= 1024 and N >= 256 and N % 8 == 0 and K % 64 == 0


# ---- tf32h range bookkeeping (device side; nothing here synchronises) ------------------------------------------------------------------
# _RANGE: the engine's two range counters (saturated / below-normal-range fp16 gradient operands; FinetuneGD.range_report reads them), or
# None.  _SLOTS: per device, the 256-word max-|x| scratch the amax kernels share (every user leaves it zeroed).  _AMAX: scales that a
# producer computed for the tensor it returned (layernorm_bwd(want_amax=True)), keyed by the tensor's address until its consumer takes it.
_RANGE = None
_SLOTS = {}
_AMAX = {}
GRAD_TARGET = 8.0      # |gradient| * s <= 8: 2^13 of fp16 headroom above the block's incoming gradient, 2^17 of full-precision range below


def set_range_counters(t):
    """t: a zeroed int32 CUDA tensor [128] (or None): every scaled fp16 cast of the tf32h engine adds its saturated (words 0-63) / below-normal-range
    (words 64-127) counts as per-block partial sums; `range_totals(t)` adds them up."""
    global _RANGE
    _RANGE = t


def range_totals(t):
    """[saturated, below_normal] from a range-counter tensor (one host read)."""
    return [int(v) for v in t.view(2, 64).sum(1).tolist()]


def _slots(dev):
    t = _SLOTS.get(dev)
    if t is None:
        t = _SLOTS[dev] = torch.zeros(256, dtype=torch.int32, device=dev)
    return t


def amax_register(t, sc):
    # the entry keeps the tensor alive: its address cannot be handed to another tensor while the scale waits for its consumer, so a hit is
    # never a stale scale (an unconsumed entry pins one gradient tensor until amax_clear(): FinetuneGD.backward's end, prepare_trainables)
    _AMAX[t.data_ptr()] = (sc, t)


def amax_take(t):
    """the scale a producer registered for exactly this tensor (popped), or None."""
    rec = _AMAX.pop(t.data_ptr(), None)
    return rec[0] if rec is not None and rec[1].numel() == t.numel() and rec[1].dtype == t.dtype else None


def amax_clear():
    _AMAX.clear()


# LayerNorm row statistics a block's forward took of its INPUT, offered to whoever else normalises the same tensor (a tapped block output is the
# next block's input: vit._TapFn / kp_gather apply `model.norm` to it from these statistics instead of a LayerNorm pass of their own).  Keyed by the
# tensor's address; one entry per tensor, popped by the taker, cleared with the step's other per-step state.
_LN_STATS = {}


def ln_stats_put(x, mean, rstd, eps):
    _LN_STATS[x.data_ptr()] = (mean, rstd, float(eps), x.numel())


def ln_stats_take(x, eps):
    rec = _LN_STATS.pop(x.data_ptr(), None)
    return (rec[0], rec[1]) if rec is not None and rec[3] == x.numel() and rec[2] == float(eps) and rec[0] is not None else None


def ln_stats_clear():
    _LN_STATS.clear()
    _LN_OUT.clear()


# The NEXT block's LayerNorm 1 of a block output, written by the producer that still held the rows on chip (adapter_fused_h_ln): keyed by the output's
# address until the next block's forward takes it (vit._BlockFn.forward) instead of running its own LayerNorm pass.
_LN_OUT = {}


def ln_out_put(x, y, mean, rstd, w):
    _LN_OUT[x.data_ptr()] = (y, mean, rstd, w.data_ptr(), x.numel())


def ln_out_take(x, w):
    rec = _LN_OUT.pop(x.data_ptr(), None)
    return rec[:3] if rec is not None and rec[3] == w.data_ptr() and rec[4] == x.numel() else None


def cast16(x, scale=1.0, scale_dev=None):
    """f32 [rows, K] (rows may be strided) -> fp16 [rows, K] = sat(x * scale * scale_dev[0]): an operand of the tf32h engine's products (fp16
    carries TF32's 11-bit significand).  Forward activations and weights go in unscaled; gradients with the power of two of `amax_scale`
    (those casts are counted in the range counters, when the engine has registered a pair)."""
    _req(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "cast16: a 2-D fp32 CUDA tensor with contiguous rows")
    rows, K = x.shape
    out = torch.empty(rows, K, dtype=torch.float16, device=x.device)
    rng = _RANGE if (scale_dev is not None and _RANGE is not None and _RANGE.device == x.device) else None
    check(lib().gd_cast_f16_ex(ptr(x), ptr(out), rows, K, x.stride(0), float(scale), ptr(scale_dev), ptr(rng), stream()), "gd_cast_f16_ex")
    return out


def amax_scale(x, target=64.0):
    """-> device fp32 [3] = {s, 1/s, unused}: s the power of two with target/2 < max|x| * s <= target (1 for an all-zero tensor, NaN when x holds
    a non-finite element: every product scaled with it is then NaN, as it would be in fp32).  No host round trip: s goes to
    `cast16(scale_dev=r[0:1])`, 1/s to `gemm_nt(alpha_dev=r[1:2])`."""
    _req(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "amax_scale: a 2-D fp32 CUDA tensor with contiguous rows")
    out = torch.empty(3, dtype=torch.float32, device=x.device)
    check(lib().gd_amax_scale(ptr(x), x.shape[0], x.shape[1], x.stride(0), float(target), ptr(out), ptr(_slots(x.device)), stream()), "gd_amax_scale")
    return out


def split3(x, which):
    """f32 [rows, K] (rows may be strided) -> bf16 [rows, 3K]: the hi / lo planes of the 3-term split product (gd_split3).  which = "a":
    left operand [hi | lo | hi]; "w": right operand [hi | hi | lo].  gemm_nt(split3(a, "a"), split3(w, "w"), out_dtype=torch.float32)
    is a . w^T to ~4e-6 relative (TF32: ~3e-4) on the bf16 matrix cores."""
    _req(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "split3: a 2-D fp32 CUDA tensor with contiguous rows")
    rows, K = x.shape
    out = torch.empty(rows, 3 * K, dtype=torch.bfloat16, device=x.device)
    check(lib().gd_split3(ptr(x), ptr(out), rows, K, x.stride(0), {"a": 0, "w": 1}[which], stream()), "gd_split3")
    return out


def gemm_nt_x3(a, w3, **kw):
    """gemm_nt on an fp32 left operand and a PRE-SPLIT right operand w3 = split3(w, "w") (frozen weights are split once): fp32 output and
    fp32 epilogue tensors, three bf16 MFMA products per term."""
    kw.setdefault("out_dtype", torch.float32)
    return gemm_nt(split3(a, "a"), w3, **kw)


def gemm_tn(y, x, out=None, *, alpha=1.0, alpha_dev=None):
    """out[N,K] (fp32) += alpha * y[M,N]^T @ x[M,K]   (weight gradients; fp32 accumulation).  alpha_dev: a device scalar multiplied into alpha
    (the 1/s of a scaled fp16 gradient operand, ops.amax_scale)."""
    _req(y.is_cuda and x.is_cuda and y.stride(-1) == 1 and x.stride(-1) == 1 and y.shape[:-1] == x.shape[:-1],
         "gemm_tn: bad operands")
    batched = y.dim() == 3
    M, N = y.shape[-2:]
    K = x.shape[-1]
    B = y.shape[0] if batched else 1
    if out is None:
        out = torch.zeros((B, N, K) if batched else (N, K), dtype=torch.float32, device=y.device)
    _req(out.dtype == torch.float32 and out.stride(-1) == 1, "gemm_tn: out must be fp32, contiguous rows")
    args = (ptr(y), ptr(x), ptr(out), M, N, K, y.stride(-2), x.stride(-2), out.stride(-2), B, y.stride(0) if batched else 0,
            x.stride(0) if batched else 0, out.stride(0) if batched else 0, dtype_code(y), dtype_code(x), float(alpha))
    rc = lib().gd_gemm_tn(*args, stream()) if alpha_dev is None else lib().gd_gemm_tn_scaled(*args, ptr(alpha_dev), stream())
    check(rc, "gd_gemm_tn")
    return out


VARIANTS = {"vggt": 0, "mast3r": 1}


def pad_teacher_maps(t):
    """[P, hw, hw] -> [P, hw, ldt] view-compatible copy with ldt = hw rounded up to 32 floats (128-byte rows, zero pad): the
    layout the fast cost-volume path reads (it needs 16-byte rows; whole-line rows keep a tile's 512-byte row segments from
    straddling cache lines that a neighbouring tile — on another XCD — fetches again: PMC FETCH_SIZE 1.37x -> ~1.0x of the teacher
    bytes, profiles/README.md round 3).  Done ONCE per cached pair (TeacherTargetCache), never per step."""
    P, hw, w = t.shape
    ldt = (w + 31) // 32 * 32
    if ldt == w and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 128 == 0:
        return t
    out = torch.zeros(P, hw, ldt, dtype=torch.float32, device=t.device)
    out[:, :, :w] = t
    return out


def cost_volume_teacher_stats(t1, t2):
    """Per teacher row {max(rowsum, 1e-8), W, A, 0} (see gd_cost_volume_teacher_stats): depends on the teacher maps only —
    computed once when a pair's targets are cached.  t1, t2 [P, hw, ldt] -> [P, 2, hw, 4] fp32."""
    P, hw, ldt = t1.shape
    t1, t2 = t1.contiguous().float(), t2.contiguous().float()
    out = torch.empty(P, 2, hw, 4, dtype=torch.float32, device=t1.device)
    check(lib().gd_cost_volume_teacher_stats(ptr(t1), ptr(t2), P, hw, ldt, ptr(out), stream()), "gd_cost_volume_teacher_stats")
    return out


class _CostVolumeKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, t1, t2, m1, m2, variant, tstats, inv1=None, inv2=None, x3=False, h16=None, kcap=0):
        P, hw, C = f1.shape
        f1, f2 = f1.contiguous(), f2.contiguous()
        t1, t2 = t1.contiguous().float(), t2.contiguous().float()
        ldt = t1.shape[-1]
        _req(t1.shape == (P, hw, ldt) and t2.shape == (P, hw, ldt) and ldt >= hw, "cost_volume_kl: teacher maps must be [P, hw, ldt >= hw]")
        m1 = m1.contiguous().to(torch.uint8)
        m2 = m2.contiguous().to(torch.uint8)
        dt = dtype_code(f1)
        loss = torch.empty(P, dtype=torch.float32, device=f1.device)
        stats = torch.empty(P, 2, hw, 4, dtype=torch.float32, device=f1.device)
        ws = torch.empty(lib().gd_cost_volume_kl_workspace_bytes(P, hw, C, dt, 0), dtype=torch.uint8, device=f1.device)
        if tstats is not None:
            _req(tstats.shape == (P, 2, hw, 4) and tstats.dtype == torch.float32 and tstats.is_contiguous(), "cost_volume_kl: bad tstats")
        if inv1 is not None:
            _req(inv1.shape == (P, hw) and inv2.shape == (P, hw) and inv1.dtype == torch.float32 and inv2.dtype == torch.float32 and
                 inv1.is_contiguous() and inv2.is_contiguous(), "cost_volume_kl: inv_norms must be two contiguous fp32 [P, hw] tensors")
            h16_saved = None
            rows = kcap > 0 and tstats is not None and ldt % 4 == 0      # sparse row masks: the kept-row kernel (gd_cost_volume_kl_fwd_rows)

            ctx.kcap = 0

            def fwd(fa, fb, cc, code):
                if rows and (cc * (2 if code else 4)) % 128 == 0 and cc * (2 if code else 4) >= 384:
                    ctx.kcap = kcap      # the backward takes the kept-row form too
                    wsr = torch.empty(lib().gd_cost_volume_kl_rows_workspace_bytes(P, hw, kcap), dtype=torch.uint8, device=f1.device)
                    return lib().gd_cost_volume_kl_fwd_rows(ptr(fa), ptr(fb), ptr(inv1), ptr(inv2), ptr(t1), ptr(t2), ldt, ptr(tstats), ptr(m1), ptr(m2),
                                                            P, hw, cc, kcap, VARIANTS[variant], code, ptr(loss), ptr(stats), ptr(wsr), stream())
                wsd = torch.empty(lib().gd_cost_volume_kl_workspace_bytes(P, hw, cc, code, 0), dtype=torch.uint8, device=f1.device)
                return lib().gd_cost_volume_kl_fwd_prenorm(ptr(fa), ptr(fb), ptr(inv1), ptr(inv2), ptr(t1), ptr(t2), ldt, ptr(tstats), ptr(m1), ptr(m2),
                                                           P, hw, cc, VARIANTS[variant], code, ptr(loss), ptr(stats), ptr(wsd), stream())
            if x3 == "h" and f1.dtype == torch.float32 and C % 8 == 0:
                # tf32h: S from the fp16 copies of the features (TF32's significand); the backward recomputes S from the SAME copies (kept)
                if h16 is not None:
                    a16, b16 = h16[0].contiguous(), h16[1].contiguous()
                    _req(a16.dtype == torch.float16 and a16.shape == f1.shape and b16.shape == f2.shape, "cost_volume_kl: h16 must be the fp16 copies of f1, f2")
                else:
                    a16, b16 = cast16(f1.view(P * hw, C)), cast16(f2.view(P * hw, C))
                rc = fwd(a16, b16, C, 3)
                h16_saved = (a16, b16)
            elif x3 and f1.dtype == torch.float32 and C % 8 == 0:
                # tf32x: S = f1 . f2^T as three bf16 MFMA products of the (hi, lo) splits on the bf16 tile kernel (K = 3C) instead of the
                # exact-f32 MFMA; the row norms stay those of the f32 rows, and the backward (which recomputes S in f32) reads the same
                # stats layout — logZ from this S agrees with its own to ~1e-6
                a3, b3 = split3(f1.view(P * hw, C), "a"), split3(f2.view(P * hw, C), "w")
                ws = torch.empty(lib().gd_cost_volume_kl_workspace_bytes(P, hw, 3 * C, 1, 0), dtype=torch.uint8, device=f1.device)
                rc = lib().gd_cost_volume_kl_fwd_prenorm(ptr(a3), ptr(b3), ptr(inv1), ptr(inv2), ptr(t1), ptr(t2), ldt, ptr(tstats), ptr(m1),
                                                         ptr(m2), P, hw, 3 * C, VARIANTS[variant], 1, ptr(loss), ptr(stats), ptr(ws), stream())
            else:
                rc = fwd(f1, f2, C, dt)
        else:
            rc = lib().gd_cost_volume_kl_fwd(ptr(f1), ptr(f2), ptr(t1), ptr(t2), ldt, ptr(tstats), ptr(m1), ptr(m2), P, hw, C,
                                             VARIANTS[variant], dt, ptr(loss), ptr(stats), ptr(ws), stream())
        check(rc, "gd_cost_volume_kl_fwd")
        # (the fp16 feature copies are saved tensors like the rest — autograd's lifetime and version checks apply to them; ctx keeps plain ints only)
        if inv1 is None:
            h16_saved, ctx.kcap = None, 0
        ctx.has_h16 = h16_saved is not None
        ctx.save_for_backward(f1, f2, t1, t2, m1, m2, stats, *(h16_saved or ()))
        return loss

    @staticmethod
    def backward(ctx, gloss):
        f1, f2, t1, t2, m1, m2, stats = ctx.saved_tensors[:7]
        h = tuple(ctx.saved_tensors[7:9]) if ctx.has_h16 else None
        P, hw, C = f1.shape
        kcap = ctx.kcap
        if kcap and option("cv_bwd_rows"):      # sparse row masks: G only for the kept rows of each direction (gd_cost_volume_kl_bwd_rows)
            code = 3 if h is not None else dtype_code(f1)
            dfull = torch.empty((2 * P, hw, C), dtype=f1.dtype, device=f1.device)
            ws = torch.empty(lib().gd_cost_volume_kl_bwd_rows_workspace_bytes(P, hw, C, kcap, code), dtype=torch.uint8, device=f1.device)
            g = gloss.contiguous().float()
            rc = lib().gd_cost_volume_kl_bwd_rows(ptr(f1), ptr(f2), ptr(h[0]) if h else None, ptr(h[1]) if h else None, ptr(t1), ptr(t2), t1.shape[-1],
                                                  ptr(m1), ptr(m2), P, hw, C, kcap, code, ptr(g), ptr(stats), ptr(dfull[:P]), ptr(dfull[P:]), ptr(ws), stream())
            check(rc, "gd_cost_volume_kl_bwd_rows")
            return dfull[:P], dfull[P:], None, None, None, None, None, None, None, None, None, None, None
        if h is not None:      # tf32h: fp16 S recompute and G contractions, fp32 gradient through the normalisation
            a16, b16 = h
            dfull = torch.empty((2 * P, hw, C), dtype=torch.float32, device=f1.device)
            ws = torch.empty(lib().gd_cost_volume_kl_bwd_h_workspace_bytes(P, hw, C), dtype=torch.uint8, device=f1.device)
            g = gloss.contiguous().float()
            rc = lib().gd_cost_volume_kl_bwd_h(ptr(f1), ptr(f2), ptr(a16), ptr(b16), ptr(t1), ptr(t2), t1.shape[-1], ptr(m1), ptr(m2), P, hw, C,
                                               ptr(g), ptr(stats), ptr(dfull[:P]), ptr(dfull[P:]), ptr(ws), stream())
            check(rc, "gd_cost_volume_kl_bwd_h")
            return dfull[:P], dfull[P:], None, None, None, None, None, None, None, None, None, None, None
        dt = dtype_code(f1)
        # the two halves of ONE buffer: split_pairs' backward hands it on without a concatenation pass (134 MB at the step's size)
        dfull = torch.empty((2 * P, hw, C), dtype=f1.dtype, device=f1.device)
        df1, df2 = dfull[:P], dfull[P:]
        ws = torch.empty(lib().gd_cost_volume_kl_workspace_bytes(P, hw, C, dt, 1), dtype=torch.uint8, device=f1.device)
        g = gloss.contiguous().float()
        rc = lib().gd_cost_volume_kl_bwd(ptr(f1), ptr(f2), ptr(t1), ptr(t2), t1.shape[-1], ptr(m1), ptr(m2), P, hw, C, dt, ptr(g),
                                         ptr(stats), ptr(df1), ptr(df2), ptr(ws), stream())
        check(rc, "gd_cost_volume_kl_bwd")
        return df1, df2, None, None, None, None, None, None, None, None, None, None, None


def kept_row_capacity(hw, kept_rows_max):
    """Row capacity (a multiple of 128) of the kept-row cost-volume kernels for a caller's bound on the kept rows of any (pair, view), or 0 when the
    dense hw x hw sweep is the better form: no bound given, or the two compacted problems (2 x capacity rows) would cover more than the hw rows."""
    if kept_rows_max is None or int(kept_rows_max) <= 0:
        return 0
    kc = (min(int(kept_rows_max), int(hw)) + 127) // 128 * 128
    return kc if 2 * kc <= hw else 0


def cost_volume_kl(f1, f2, t1, t2, m1, m2, variant="vggt", tstats=None, inv_norms=None, x3=False, h16=None, kept_rows_max=None):
    """Fused dense cost-volume KL for P pairs.  f1,f2 [P,hw,C] raw student features (f32|bf16); t1,t2 [P,hw,ldt] teacher
    maps (f32; ldt = hw, or hw padded to a multiple of 4 by `pad_teacher_maps`: the fast path); m1,m2 [P,hw] bool row
    masks; tstats: `cost_volume_teacher_stats(t1, t2)` computed once per cached pair (None: recomputed here, one more pass
    over the maps); inv_norms = (inv1, inv2), fp32 [P, hw] each: 1 / max(||row||, 1e-12) of the feature rows as stored, when their
    producer already took them (`tap_mean(..., with_norm=True)`) — the op then skips its own pass over the features
    x3 (fp32 features with inv_norms): the forward's similarity matrix as a split-precision bf16 product (tf32x engine)
    kept_rows_max (with inv_norms and tstats): a bound on the number of kept rows of any (pair, view) — e.g. the keypoint count behind keypoint-patch
    masks; when it is below half of hw the forward runs as two compacted row problems (gd_cost_volume_kl_fwd_rows) instead of one hw x hw sweep
    -> loss [P] (f32)."""
    if inv_norms is not None:
        kcap = kept_row_capacity(f1.shape[1], kept_rows_max) if tstats is not None else 0
        return _CostVolumeKL.apply(f1, f2, t1, t2, m1, m2, variant, tstats, inv_norms[0].detach(), inv_norms[1].detach(), x3, h16, kcap)
    return _CostVolumeKL.apply(f1, f2, t1, t2, m1, m2, variant, tstats)


F32X3 = 2      # gd_attention_* dtype code: fp32 tensors, products as three bf16 MFMAs of (hi, lo) splits (include/gd_hip.h GD_F32X3)


def attention_fwd(qkv, B, N, H, x3=False):
    """qkv [B*N, 3*H*64] packed (q|k|v, heads inner) -> o [B*N, H*64], lse [B,H,N] (f32).  x3 (fp32 tensors only): the TF32-class
    split-precision kernels instead of the exact-f32 MFMA ones."""
    _req(qkv.is_contiguous() and qkv.shape == (B * N, 3 * H * 64), "attention_fwd: qkv must be [B*N, 3*H*64]")
    o = torch.empty(B * N, H * 64, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    _req(not x3 or qkv.dtype == torch.float32, "attention_fwd: x3 needs fp32 tensors")
    rc = lib().gd_attention_fwd(ptr(qkv), ptr(o), ptr(lse), B, N, H, 64, 64 ** -0.5, F32X3 if x3 else dtype_code(qkv), stream())
    check(rc, "gd_attention_fwd")
    return o, lse


def cross_attention_fwd(q, kv, B, Nq, Nk, H, want_lse=False, x3=False):
    """q [B*Nq, H*64], kv [B*Nk, 2*H*64] (k | v, heads inner): 2-D tensors or strided 2-D views (last dim contiguous, row strides multiples
    of 16 bytes) -> o [B*Nq, H*64] contiguous, lse [B,H,Nq] (f32, natural log) or None: softmax(q k^T / 8) v per (image, head)
    (dust3r/croco/models/blocks.py:150-172).  x3 (fp32 tensors only): the split-precision kernel."""
    _req(q.is_cuda and kv.is_cuda and q.dtype == kv.dtype, "cross_attention_fwd: q and kv must be CUDA tensors of one dtype")
    _req(q.dim() == 2 and tuple(q.shape) == (B * Nq, H * 64) and q.stride(1) == 1, "cross_attention_fwd: q must be a [B*Nq, H*64] view, last dim contiguous")
    _req(kv.dim() == 2 and tuple(kv.shape) == (B * Nk, 2 * H * 64) and kv.stride(1) == 1,
         "cross_attention_fwd: kv must be a [B*Nk, 2*H*64] view, last dim contiguous")
    _req(not x3 or q.dtype == torch.float32, "cross_attention_fwd: x3 needs fp32 tensors")
    o = torch.empty(B * Nq, H * 64, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device) if want_lse else None
    rc = lib().gd_cross_attention_fwd(ptr(q), ptr(kv), ptr(o), ptr(lse), B, Nq, Nk, H, 64, q.stride(0), kv.stride(0), 64 ** -0.5,
                                      F32X3 if x3 else dtype_code(q), stream())
    check(rc, "gd_cross_attention_fwd")
    return o, lse


def attention_small_fwd(q, k, v, G0, G1, Nq, Nk, H, scale=None, out=None):
    """q [G0, G1, Nq, H*hd], k, v [G0, G1, Nk, H*hd]: fp32 strided 4-D views (last dim contiguous; every other stride, read off the tensor, a
    multiple of 4 elements — column blocks of one packed tensor and tokens that are not neighbours in memory are fine) -> o [G0, G1, Nq, H*hd]
    = softmax(scale q k^T) v per (g0, g1, head), contiguous unless `out=` (a view of the same kind, overlapping no input) is given
    (gd_attention_small_fwd: exact fp32, hd a multiple of 4 up to 64, short sequences; scale defaults to hd^-0.5)."""
    for t, n, what in ((q, Nq, "q"), (k, Nk, "k"), (v, Nk, "v")) + (((out, Nq, "out"),) if out is not None else ()):
        _req(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and tuple(t.shape[:3]) == (G0, G1, n) and t.shape[3] == q.shape[3] and
             t.stride(3) == 1, f"attention_small_fwd: {what} must be a CUDA fp32 view [{G0}, {G1}, {n}, {q.shape[3]}] with a contiguous last dim, "
             f"got {tuple(t.shape)} {t.dtype} strides {tuple(t.stride())}")
    W = q.shape[3]
    _req(H >= 1 and W % H == 0, f"attention_small_fwd: width {W} is not a multiple of H = {H}")
    hd = W // H
    o = torch.empty(G0, G1, Nq, W, dtype=torch.float32, device=q.device) if out is None else out
    # the stride of a dimension of size 1 is arbitrary in torch and addresses nothing: 0 (W for the row stride) goes down instead
    st = lambda t: tuple(t.stride(d) if t.shape[d] > 1 else 0 for d in (0, 1))
    ld = lambda t: t.stride(2) if t.shape[2] > 1 else W
    rc = lib().gd_attention_small_fwd(ptr(q), ptr(k), ptr(v), ptr(o), G0, G1, Nq, Nk, H, hd, ld(q), ld(k), ld(v), ld(o),
                                      *st(q), *st(k), *st(v), *st(o), float(hd ** -0.5 if scale is None else scale), stream())
    check(rc, "gd_attention_small_fwd")
    return o


def attention_bwd(qkv, o, dout, lse, B, N, H, vfirst=False, need_dk=True, x3=False):
    """-> dqkv [B*N, 3*H*64] (same dtype as qkv), column blocks (dq, dk, dv) — or (dq, dv, dk) with vfirst.  need_dk=False: the dK
    columns are left unwritten (bf16: the dK/dV kernel then runs its dV half only)."""
    _req(dout.is_contiguous() and dout.shape == o.shape and dout.dtype == qkv.dtype, "attention_bwd: bad dout")
    dqkv = torch.empty_like(qkv)
    # workspace: the dQ kernel leaves [-delta | -lse in log2 units] per query for the dK/dV kernel, rows padded to whole 64-query tiles; the library states its size
    delta = torch.empty(lib().gd_attention_bwd_workspace_bytes(B, N, H) // 4, dtype=torch.float32, device=qkv.device)
    rc = lib().gd_attention_bwd(ptr(qkv), ptr(o), ptr(dout), ptr(lse), ptr(dqkv), ptr(delta), B, N, H, 64,
                                64 ** -0.5, F32X3 if x3 else dtype_code(qkv), (1 if vfirst else 0) | (0 if need_dk else 2), stream())
    check(rc, "gd_attention_bwd")
    return dqkv


def qk_norm_rope(qkv, B, N, H, pos, gq, bq, gk, bk, eps, base, want_qk=False):
    """In place on the packed qkv [B*N, 3*H*64] (f32 | bf16): q <- RoPE2D(LN_64(q; gq, bq, eps), pos), k likewise with gk, bk; v untouched
    (vggt/layers/attention.py:58-65).  pos int64 [B*N, 2] (y, x); gq = bq = gk = bk = None: no normalisation.  want_qk: also returns
    (q, k) as [B, H, N, 64], the layout teacher_glue.cross_view_attention_maps takes; otherwise None."""
    _req(qkv.is_cuda and qkv.is_contiguous() and qkv.shape == (B * N, 3 * H * 64), "qk_norm_rope: qkv must be a contiguous CUDA [B*N, 3*H*64]")
    _req(pos.is_cuda and pos.dtype == torch.int64 and pos.is_contiguous() and pos.numel() == B * N * 2, "qk_norm_rope: pos must be contiguous int64 [B*N, 2]")
    for t in (gq, bq, gk, bk):
        _req(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == 64), "qk_norm_rope: gamma / beta must be fp32 [64]")
    q_out = torch.empty(B, H, N, 64, dtype=qkv.dtype, device=qkv.device) if want_qk else None
    k_out = torch.empty_like(q_out) if want_qk else None
    rc = lib().gd_qk_norm_rope(ptr(qkv), ptr(pos), ptr(gq), ptr(bq), ptr(gk), ptr(bk), ptr(q_out), ptr(k_out), B, N, H, 64, float(eps), float(base),
                               dtype_code(qkv), stream())
    check(rc, "gd_qk_norm_rope")
    return (q_out, k_out) if want_qk else None


# ----------------------------------------------------------------------------------------------
# views of the two halves of a [2P, ...] batch (view 1 / view 2 of P pairs)
# ----------------------------------------------------------------------------------------------
class _SplitPairs(torch.autograd.Function):
    """x[:P], x[P:] whose backward is ONE concatenation (autograd's own slice backward zero-fills a full-size tensor per
    half, copies, then adds the two)."""

    @staticmethod
    def forward(ctx, x, P):
        ctx.P, ctx.shape, ctx.dt = P, x.shape, x.dtype
        return x[:P], x[P:]

    @staticmethod
    def backward(ctx, g1, g2):
        P, shp = ctx.P, ctx.shape
        if g1 is None and g2 is None:
            return None, None
        if g1 is not None and g2 is not None:
            base = g1._base
            if (base is not None and base is g2._base and base.is_contiguous() and tuple(base.shape) == tuple(shp)
                    and base.dtype == g1.dtype and g1.is_contiguous() and g2.is_contiguous() and g1.data_ptr() == base.data_ptr()
                    and g2.data_ptr() == base.data_ptr() + g1.numel() * g1.element_size()):
                return base, None              # already the halves of one buffer (e.g. cost_volume_kl's backward)
        dev = (g1 if g1 is not None else g2).device
        if g1 is None:
            g1 = torch.zeros((P,) + tuple(shp[1:]), dtype=g2.dtype, device=dev)
        if g2 is None:
            g2 = torch.zeros((shp[0] - P,) + tuple(shp[1:]), dtype=g1.dtype, device=dev)
        return torch.cat([g1, g2], 0), None


def split_pairs(x, P):
    return _SplitPairs.apply(x, P)


# ----------------------------------------------------------------------------------------------
# bottleneck adapter (utils/model.py:7-25), one fused pass
# ----------------------------------------------------------------------------------------------
def adapter_fused_supported(x, bottleneck):
    return bool(lib().gd_adapter_fused_supported(int(x.shape[-1]), int(bottleneck), dtype_code(x)))


def adapter_fused(x, w1, w2, gate_src=None, save_hidden=True):
    """out = x + gate(x @ w1.T) @ w2.T, hidden = gate(x @ w1.T)   (x [M,D] bf16, w1 [64,D], w2 [D,64], same dtype).
    gate_src None: ReLU (the forward, w1 = down, w2 = up); gate_src [M,64]: keep where gate_src > 0 (the backward-to-input
    with x = dOut, w1 = up^T, w2 = down^T, gate_src = the forward's hidden).  -> (out, hidden or None)."""
    M, D = x.shape
    bott = w1.shape[0]
    _req(x.is_contiguous() and w1.is_contiguous() and w2.is_contiguous() and w1.shape == (bott, D) and
         w2.shape == (D, bott) and w1.dtype == x.dtype and w2.dtype == x.dtype, "adapter_fused: layout")
    _req(gate_src is None or (gate_src.is_contiguous() and gate_src.shape == (M, bott) and gate_src.dtype == x.dtype),
         "adapter_fused: gate_src layout")
    out = torch.empty_like(x)
    hidden = torch.empty(M, bott, dtype=x.dtype, device=x.device) if save_hidden else None
    rc = lib().gd_adapter_fused(ptr(x), ptr(w1), ptr(w2), ptr(gate_src), ptr(hidden), ptr(out), M, D, bott,
                                dtype_code(x), stream())
    check(rc, "gd_adapter_fused")
    return out, hidden


def adapter_fused_h_supported(M, D, bottleneck):
    return bool(option("adapter_h_fused")) and bool(lib().gd_adapter_fused_h_supported(int(D), int(bottleneck), int(M)))


def adapter_fused_h(x32, w1, w2, gate_src=None, in_scale=None, alpha_dev=None, copy_scale=None, want_copy=False):
    """The adapter pass of the tf32h engine in one kernel: x32 [M,D] fp32, w1 [64,D] / w2 [D,64] fp16 ->
    out32 = x32 + alpha * gate(fp16(x32 * in_scale) @ w1.T) @ w2.T (fp32), hidden [M,64] fp16 (the gated first product, still times in_scale),
    and with want_copy fp16(out32 * copy_scale).  gate_src None: ReLU (forward); gate_src [M,64] fp16: keep where gate_src > 0 (backward-to-input:
    x32 = dOut, in_scale = s, alpha = 1/s).  The three scales are device scalars (ops.amax_scale slices) or None = 1."""
    M, D = x32.shape
    bott = w1.shape[0]
    _req(x32.dtype == torch.float32 and x32.is_contiguous() and w1.dtype == torch.float16 and w2.dtype == torch.float16 and w1.is_contiguous() and
         w2.is_contiguous() and w1.shape == (bott, D) and w2.shape == (D, bott), "adapter_fused_h: layout")
    _req(gate_src is None or (gate_src.is_contiguous() and gate_src.shape == (M, bott) and gate_src.dtype == torch.float16), "adapter_fused_h: gate_src layout")
    out = torch.empty_like(x32)
    hidden = torch.empty(M, bott, dtype=torch.float16, device=x32.device)
    copy = torch.empty(M, D, dtype=torch.float16, device=x32.device) if want_copy else None
    check(lib().gd_adapter_fused_h(ptr(x32), ptr(w1), ptr(w2), ptr(gate_src), ptr(hidden), ptr(out), ptr(copy), ptr(in_scale), ptr(alpha_dev),
                                   ptr(copy_scale), M, D, bott, stream()), "gd_adapter_fused_h")
    return out, hidden, copy


def adapter_fused_h_ln(x32, w1, w2, ln_w, ln_b, ln_eps):
    """adapter_fused_h (forward form) that also writes the NEXT block's LayerNorm 1 of its result: -> (out32, hidden fp16, y16 = fp16(LN(out32)), mean, rstd)
    (gd_adapter_fused_h_ln)."""
    M, D = x32.shape
    bott = w1.shape[0]
    _req(x32.dtype == torch.float32 and x32.is_contiguous() and w1.dtype == torch.float16 and w2.dtype == torch.float16 and w1.is_contiguous() and
         w2.is_contiguous() and w1.shape == (bott, D) and w2.shape == (D, bott) and ln_w.dtype == torch.float32 and ln_b.dtype == torch.float32, "adapter_fused_h_ln: layout")
    out = torch.empty_like(x32)
    hidden = torch.empty(M, bott, dtype=torch.float16, device=x32.device)
    y16 = torch.empty(M, D, dtype=torch.float16, device=x32.device)
    mean = torch.empty(M, dtype=torch.float32, device=x32.device)
    rstd = torch.empty(M, dtype=torch.float32, device=x32.device)
    check(lib().gd_adapter_fused_h_ln(ptr(x32), ptr(w1), ptr(w2), ptr(hidden), ptr(out), ptr(ln_w), ptr(ln_b), float(ln_eps), ptr(y16), ptr(mean), ptr(rstd),
                                      M, D, bott, stream()), "gd_adapter_fused_h_ln")
    return out, hidden, y16, mean, rstd


# ----------------------------------------------------------------------------------------------
# normalisation
# ----------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, *, save_stats=True, out_dtype=None):
    """x [M,D] (rows may be strided) -> y [M,D], mean [M], rstd [M] (fp32; None when save_stats=False)."""
    M, D = x.shape
    y = torch.empty(M, D, dtype=out_dtype or x.dtype, device=x.device)
    mean = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(M, dtype=torch.float32, device=x.device) if save_stats else None
    rc = lib().gd_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), M, D, x.stride(0),
                                y.stride(0), float(eps), dtype_code(x), dtype_code(y), stream())
    check(rc, "gd_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dres=None, dyscale=1.0, dres2=None, cast_scale=None, dy_scale=None, want_amax=False):
    """dx [M,D] (dtype of x) = LN'(dy * dyscale) (+ dres) (+ dres2).  cast_scale (fp32 tensors; a device scalar, e.g. amax_scale(...)[0:1]):
    also returns fp16(dx * cast_scale) — (dx, dx16) — the tf32h engine's next left operand, from the same pass.
    tf32h extras (fp32 x): dy may be fp16 with dy_scale (a device scalar multiplied in: 1/s of a gradient kept in its scaled domain);
    want_amax: the pass also takes max |dx| and the scale for the tensor's consumer is registered under it (`amax_take`)."""
    M, D = x.shape
    if cast_scale is not None or dy_scale is not None or want_amax or dy.dtype == torch.float16:
        _req(x.is_contiguous() and x.dtype == torch.float32 and dy.dtype in (torch.float32, torch.float16) and dy.stride(-1) == 1 and
             all(t is None or (t.is_contiguous() and t.dtype == x.dtype and t.numel() == x.numel()) for t in (dres, dres2)),
             "layernorm_bwd (tf32h form): fp32 x / dres, fp32 or fp16 dy, contiguous")
        dx = torch.empty_like(x)
        dx16 = torch.empty(M, D, dtype=torch.float16, device=x.device) if cast_scale is not None else None
        slots = _slots(x.device) if want_amax else None
        rng = _RANGE if ((dx16 is not None or dy.dtype == torch.float16) and _RANGE is not None and _RANGE.device == x.device) else None      # (an fp16 dy: its saturated entries are counted here, its producer's epilogue has no counter)
        check(lib().gd_layernorm_bwd_ex(ptr(dy), dtype_code(dy), ptr(dy_scale), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dres2), ptr(dx),
                                        ptr(dx16), ptr(cast_scale), ptr(slots), ptr(rng), M, D, dy.stride(0), x.stride(0), float(dyscale), stream()),
              "gd_layernorm_bwd_ex")
        if want_amax:
            sc = torch.empty(3, dtype=torch.float32, device=x.device)
            check(lib().gd_scale_from_amax(ptr(slots), GRAD_TARGET, ptr(sc), stream()), "gd_scale_from_amax")
            amax_register(dx, sc)
        return (dx, dx16) if cast_scale is not None else dx
    _req(x.is_contiguous() and dy.stride(-1) == 1 and all(t is None or (t.is_contiguous() and t.dtype == x.dtype and
                                                                        t.numel() == x.numel()) for t in (dres, dres2)),
         "layernorm_bwd: layout")
    dx = torch.empty_like(x)
    rc = lib().gd_layernorm_bwd(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dres2), ptr(dx), M, D,
                                dy.stride(0), x.stride(0), float(dyscale), dtype_code(x), dtype_code(dy), stream())
    check(rc, "gd_layernorm_bwd")
    return dx


class _L2Norm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        x = x.contiguous().float()
        M, D = x.numel() // x.shape[-1], x.shape[-1]
        y = torch.empty_like(x)
        inv = torch.empty(M, dtype=torch.float32, device=x.device)
        check(lib().gd_l2norm_fwd(ptr(x), ptr(y), ptr(inv), M, D, float(eps), stream()), "gd_l2norm_fwd")
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        dy = dy.contiguous().float()
        dx = torch.empty_like(y)
        check(lib().gd_l2norm_bwd(ptr(y), ptr(dy), ptr(inv), ptr(dx), inv.numel(), y.shape[-1], stream()), "gd_l2norm_bwd")
        return dx, None


def l2_normalize(x, eps=1e-12):
    """F.normalize(x, p=2, dim=-1) on fp32 rows, HIP forward/backward."""
    return _L2Norm.apply(x, eps)


# ----------------------------------------------------------------------------------------------
# image prep / tokens / conv glue
# ----------------------------------------------------------------------------------------------
def patch_im2col(img, H, W, P, Kp, mean, std, dtype, stride=None):
    """img [B,3,h,w] fp32 in [0,1] -> col [B*gh*gw, Kp]: resize to (H,W) + Normalize + im2col, zero padded.  stride = (sy, sx)
    of the patch conv (default = P: gh = H/P; a smaller stride gives overlapping patches, gh = 1 + (H - P) // sy)."""
    import ctypes
    img = img.contiguous().float()
    B, _, h, w = img.shape
    sy, sx = (P, P) if stride is None else stride
    col = torch.empty(B * (1 + (H - P) // sy) * (1 + (W - P) // sx), Kp, dtype=dtype, device=img.device)
    m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
    check(lib().gd_patch_im2col_strided(ptr(img), ptr(col), B, h, w, H, W, P, sy, sx, Kp, m3, s3, dtype_code(col), stream()),
          "gd_patch_im2col_strided")
    return col


def assemble_tokens(patch, cls, pos, B, Np):
    D = patch.shape[-1]
    out = torch.empty(B * (Np + 1), D, dtype=patch.dtype, device=patch.device)
    check(lib().gd_assemble_tokens(ptr(patch), ptr(cls), ptr(pos), ptr(out), B, Np, D, dtype_code(patch), stream()),
          "gd_assemble_tokens")
    return out


def im2col3x3(x, bstride, B, gh, gw, D):
    """x: tensor whose data_ptr is grid element (b=0,y=0,x=0,c=0); batch stride `bstride` elements."""
    col = torch.empty(B * gh * gw, 9 * D, dtype=x.dtype, device=x.device)
    check(lib().gd_im2col3x3(ptr(x), bstride, ptr(col), B, gh, gw, D, dtype_code(x), stream()), "gd_im2col3x3")
    return col


def col2im3x3(dcol, B, gh, gw, D, prefix=0):
    """-> [B, prefix + gh*gw, D]: gradient of the token grid the 3x3 conv read, prefix-token rows zero."""
    dx = torch.empty(B, prefix + gh * gw, D, dtype=dcol.dtype, device=dcol.device)
    if prefix:
        dx[:, :prefix].zero_()
    check(lib().gd_col2im3x3(ptr(dcol), dx[:, prefix:].data_ptr(), (prefix + gh * gw) * D, B, gh, gw, D, dtype_code(dcol),
                             stream()), "gd_col2im3x3")
    return dx


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def kp_gather_fwd(grids, bstride, kp, B, Nk, gh, gw, D, sx, sy, img_h, img_w, patch, stride=None, pitch=None):
    """grids: list (1..4) of tensors whose data_ptr is the (b=0, token 0 of the grid) element; pitch = tokens per grid line in
    memory (default gw)."""
    out = torch.empty(B, Nk, D, dtype=torch.float32, device=kp.device)
    check(lib().gd_kp_gather_fwd(_ptr_array(grids), len(grids), bstride, dtype_code(grids[0]), ptr(kp), ptr(out), B,
                                 Nk, gh, gw, D, float(sx), float(sy), img_h, img_w, patch, patch if stride is None else stride,
                                 gw if pitch is None else pitch, stream()), "gd_kp_gather_fwd")
    return out


def kp_gather_fwd_ln(grids, means, rstds, sstride, ln_w, ln_b, bstride, kp, B, Nk, gh, gw, D, sx, sy, img_h, img_w, patch, stride=None, pitch=None):
    """kp_gather_fwd on RAW grids with the final LayerNorm applied where they are sampled: means / rstds = per-grid fp32 statistics tensors whose
    data_ptr is the statistic of the grid's first token (same offset as the grid pointers), sstride = statistics per image."""
    out = torch.empty(B, Nk, D, dtype=torch.float32, device=kp.device)
    check(lib().gd_kp_gather_fwd_ln(_ptr_array(grids), _ptr_array(means), _ptr_array(rstds), len(grids), bstride, sstride, dtype_code(grids[0]),
                                    ptr(ln_w), ptr(ln_b), ptr(kp), ptr(out), B, Nk, gh, gw, D, float(sx), float(sy), img_h, img_w, patch,
                                    patch if stride is None else stride, gw if pitch is None else pitch, stream()), "gd_kp_gather_fwd_ln")
    return out


def kp_gather_bwd(ngrid, kp, dout, B, Nk, gh, gw, D, sx, sy, img_h, img_w, patch, prefix=0, stride=None, pitch=None):
    """-> list of ngrid fp32 gradient buffers [B, prefix + gh*pitch, D] (prefix-token rows / separator columns stay zero)."""
    pt = gw if pitch is None else pitch
    dg = [torch.zeros(B, prefix + gh * pt, D, dtype=torch.float32, device=kp.device) for _ in range(ngrid)]
    dout = dout.contiguous().float()
    check(lib().gd_kp_gather_bwd(_ptr_array([t[:, prefix:] for t in dg]), ngrid, (prefix + gh * pt) * D, ptr(kp), ptr(dout), B, Nk, gh, gw, D, float(sx), float(sy),
                                 img_h, img_w, patch, patch if stride is None else stride, pt, stream()), "gd_kp_gather_bwd")
    return dg


def lora_bwd_fused(dqv, t, bt_qv, gbt):
    """dqv [M, K] bf16 view (row stride may exceed K), t [M, 8] f32, bt_qv [8, K] bf16, gbt [8, K] f32 (accumulated in place)
    -> dt [M, 8] f32.  One pass over dqv for both LoRA-backward products (gd_lora_bwd_fused)."""
    M, K = dqv.shape
    dt = torch.empty(M, 8, dtype=torch.float32, device=dqv.device)
    check(lib().gd_lora_bwd_fused(ptr(dqv), dqv.stride(0), ptr(t), ptr(bt_qv), ptr(dt), ptr(gbt), M, K, stream()), "gd_lora_bwd_fused")
    return dt


def skinny_tn_mfma(t, x, out):
    """out [8, K] f32 += t [M, 8]^T . x [M, K] (bf16 rows) on the LDS-slab MFMA kernel (gd_lora_bwd_fused with bt = NULL)."""
    M, K = x.shape
    check(lib().gd_lora_bwd_fused(ptr(x), x.stride(0), ptr(t), None, None, ptr(out), M, K, stream()), "gd_lora_bwd_fused")
    return out


def lora_bwd_fused_h(dqv, t, bt_qv, gbt, t_mul=None, out_mul=None, dt_scaled=False, dt_mul=1.0):
    """The fused LoRA backward on fp16 operands (tf32h engine): dqv [M, K] fp16 view, t [M, 8] f32, bt_qv [8, K] fp16 or None (then only
    gbt [8, K] f32 += (t * t_mul)^T . dqv * out_mul), t_mul / out_mul: one-element device tensors (the step's gradient scale s and 1 / s) or None
    -> dt [M, 8] f32 = dqv . bt_qv^T * out_mul * dt_mul (None without bt_qv); dt_scaled: dt without out_mul (still in dqv's scaled domain).
    dt_mul (host power of two): undoes the shift bt_qv was formatted under (vit._opw_lora_b) on dt alone.  gd_lora_bwd_fused_scaled."""
    M, K = dqv.shape
    dt = torch.empty(M, 8, dtype=torch.float32, device=dqv.device) if bt_qv is not None else None
    check(lib().gd_lora_bwd_fused_scaled(ptr(dqv), dqv.stride(0), ptr(t), ptr(bt_qv), ptr(dt), ptr(gbt), M, K, dtype_code(dqv), ptr(t_mul), ptr(out_mul),
                                         1 if dt_scaled else 0, float(dt_mul), stream()), "gd_lora_bwd_fused_scaled")
    return dt


def lora_bwd_fused_h_supported(dqv, t, bt_qv, gbt):
    return (option("lora_fused") and dqv.dtype == torch.float16 and (bt_qv is None or (bt_qv.dtype == torch.float16 and bt_qv.is_contiguous()))
            and t.dtype == torch.float32 and t.shape[1] == 8 and t.is_contiguous() and gbt.is_contiguous() and gbt.dtype == torch.float32
            and dqv.stride(1) == 1 and dqv.shape[1] % 256 == 0 and dqv.shape[1] // 256 in (1, 2, 3, 4, 6, 8) and dqv.stride(0) % 8 == 0
            and dqv.data_ptr() % 16 == 0)


def lora_bwd_fused_supported(dqv, t, bt_qv, gbt):
    return (option("lora_fused") and dqv.dtype == torch.bfloat16 and (bt_qv is None or bt_qv.dtype == torch.bfloat16)
            and t.dtype == torch.float32 and t.shape[1] == 8 and t.is_contiguous() and (bt_qv is None or bt_qv.is_contiguous()) and gbt.is_contiguous()
            and dqv.stride(1) == 1 and dqv.shape[1] % 256 == 0 and dqv.shape[1] // 256 in (1, 2, 3, 4, 6, 8) and dqv.stride(0) % 8 == 0)


def conv_weight_pack(weight, dtype, with_wu=False):
    """refine_conv weight [D, D, 3, 3] fp32 -> (wk [D, 9D] with K order (ky, kx, c), wt [D, 9D] = flipped kernel, K order (kx, ky, n),
    wu [9D, D] = wk transposed or None) in `dtype`, one kernel."""
    D = weight.shape[0]
    w = weight.detach().float().contiguous()
    wk = torch.empty(D, 9 * D, dtype=dtype, device=w.device)
    wt = torch.empty(D, 9 * D, dtype=dtype, device=w.device)
    wu = torch.empty(9 * D, D, dtype=dtype, device=w.device) if with_wu else None
    check(lib().gd_conv_weight_pack(ptr(w), ptr(wk), ptr(wt), ptr(wu), D, dtype_code(wk), stream()), "gd_conv_weight_pack")
    return wk, wt, wu


def kp_patch_bwd_det(U, kp, out_dtype, B, Nk, Nt, gh, gw, D, sx, sy, img_h, img_w, patch):
    """U [B*Nk, 9D] (= dfeat . W) -> the token gradient [B, Nt, D] of kp_patch_gather, deterministic, prefix rows zero."""
    out = torch.empty(B, Nt, D, dtype=out_dtype, device=U.device)
    check(lib().gd_kp_patch_bwd_det(ptr(U), ptr(out), dtype_code(out), Nt * D, Nt - gh * gw, ptr(kp), B, Nk, gh, gw, D, float(sx), float(sy),
                                    img_h, img_w, patch, patch, stream()), "gd_kp_patch_bwd_det")
    return out


def kp_gather_bwd_det(kp, dout, scale, out_dtype, B, Nk, gh, gw, D, sx, sy, img_h, img_w, patch, prefix=0, stride=None, pitch=None):
    """Deterministic interpolate_features backward (no atomics, no zero-fill, no cast pass): -> [B, prefix + gh*pitch, D] of
    `out_dtype`, every element written (prefix rows / separator columns zero).  None when the shape is outside the kernel's range
    (Nk > 1024, D % 8, D > 1024) or GD_GATHER_DET=0: the caller then takes the atomic scatter."""
    pt = gw if pitch is None else pitch
    if not option("gather_det") or Nk > 1024 or D % 8 != 0 or D > 1024:
        return None
    out = torch.empty(B, prefix + gh * pt, D, dtype=out_dtype, device=kp.device)
    dout = dout.contiguous().float()
    check(lib().gd_kp_gather_bwd_det(ptr(out), dtype_code(out), (prefix + gh * pt) * D, prefix, ptr(kp), ptr(dout), float(scale), B, Nk,
                                     gh, gw, D, float(sx), float(sy), img_h, img_w, patch, patch if stride is None else stride, pt,
                                     stream()), "gd_kp_gather_bwd_det")
    return out


def kp_patch_gather(grid, bstride, kp, B, Nk, gh, gw, D, sx, sy, img_h, img_w, patch, stride=None, pitch=None, half=False):
    """-> [B*Nk, 9*D] (grid dtype): the bilinear mix of the four neighbours' 3x3 input patches, K order (ky, kx, c) — the GEMM
    operand of refine_conv evaluated at the keypoints only (gd_kp_patch_gather).  `grid` is addressed from its data_ptr.
    half (fp32 grid): the taps leave as fp16, the tf32h engine's operand (gd_kp_patch_gather_h)."""
    if half:
        _req(grid.dtype == torch.float32 and D % 4 == 0, "kp_patch_gather(half=True): an fp32 grid with D % 4 == 0")
        out = torch.empty(B * Nk, 9 * D, dtype=torch.float16, device=grid.device)
        check(lib().gd_kp_patch_gather_h(ptr(grid), bstride, ptr(kp), ptr(out), B, Nk, gh, gw, D, float(sx), float(sy), img_h, img_w, patch,
                                         patch if stride is None else stride, gw if pitch is None else pitch, stream()), "gd_kp_patch_gather_h")
        return out
    _req(grid.dtype in (torch.float32, torch.bfloat16), "kp_patch_gather: an fp32 or bf16 grid")
    out = torch.empty(B * Nk, 9 * D, dtype=grid.dtype, device=grid.device)
    check(lib().gd_kp_patch_gather(ptr(grid), bstride, dtype_code(grid), ptr(kp), ptr(out), B, Nk, gh, gw, D, float(sx), float(sy),
                                   img_h, img_w, patch, patch if stride is None else stride, gw if pitch is None else pitch,
                                   stream()), "gd_kp_patch_gather")
    return out


def stack3_rows(src, B, gh, gw, D, src_bstride, src_row0, src_pitch, dtype):
    """-> buf [B*gh*(gw+1) + 2, 3*D] of `dtype` (see gd_stack3_rows); `src` is addressed from its data_ptr."""
    buf = torch.empty(B * gh * (gw + 1) + 2, 3 * D, dtype=dtype, device=src.device)
    check(lib().gd_stack3_rows(ptr(src), ptr(buf), B, gh, gw, D, src_bstride, src_row0, src_pitch, dtype_code(src), dtype_code(buf),
                               stream()), "gd_stack3_rows")
    return buf


def conv_view(buf, rows, D):
    """The overlapping-row GEMM operand of a stack3 buffer: A[r][k] = buf_flat[r*3D + k], [rows, 9D] with row stride 3D."""
    return torch.as_strided(buf, (rows, 9 * D), (3 * D, 1))


def unpitch_tokens(src, B, gh, gw, D, prefix):
    """pitched [B*gh*(gw+1), D] -> [B, prefix + gh*gw, D], prefix rows zero."""
    out = torch.empty(B, prefix + gh * gw, D, dtype=src.dtype, device=src.device)
    check(lib().gd_unpitch_tokens(ptr(src), ptr(out), B, gh, gw, D, prefix, dtype_code(src), stream()), "gd_unpitch_tokens")
    return out


# ------------------------------------------------------------------------------------------------ DPT head glue (csrc/dpt.hip)
DPT_ACT = {"linear": 0, "exp": 1, "inv_log": 2, "relu": 3, "sigmoid": 4}            # include/gd_hip.h GD_DPT_ACT_*
DPT_CONF_ACT = {"expp1": 0, "expp0": 1, "sigmoid": 2, "linear": 3}                  # GD_DPT_CONF_* ("linear": the pre-activation map)


def grid_resample(src, frames, sh, sw, dh, dw, C, *, step=0, addend=None, px=None, py=None, relu=False, stacked=None):
    """src: the pitched grid [frames*sh*(sw+1), C] (f32 | bf16) -> dh x dw (gd_grid_resample: bilinear align_corners=True, or every `step`-th
    pixel), + addend [frames*dh*(dw+1), C] + position tables px [dw, C/2], py [dh, C/2] (fp32), ReLU last.
    stacked=None: the pitched fp32 grid [frames*dh*(dw+1), C], separators zero;  stacked=dtype: the stack3_rows operand of that grid,
    [frames*dh*(dw+1) + 2, 3C] of `dtype`, written directly."""
    _req(src.is_cuda and src.is_contiguous() and src.numel() == frames * sh * (sw + 1) * C, "grid_resample: src is not the contiguous pitched grid")
    for t, n, what in ((addend, frames * dh * (dw + 1) * C, "addend"), (px, dw * (C // 2), "px"), (py, dh * (C // 2), "py")):
        _req(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n), f"grid_resample: bad {what}")
    rows = frames * dh * (dw + 1)
    out = torch.empty((rows, C) if stacked is None else (rows + 2, 3 * C), dtype=stacked or torch.float32, device=src.device)
    check(lib().gd_grid_resample(ptr(src), dtype_code(src), ptr(out), dtype_code(out), 0 if stacked is None else 1, frames, sh, sw, dh, dw, C, int(step),
                                 ptr(addend), ptr(px), ptr(py), 1 if relu else 0, stream()), "gd_grid_resample")
    return out


def deconv_scatter(src, bias, frames, gh, gw, src_pitch, k, Cout):
    """src [frames*gh*src_pitch, k*k*Cout] fp32 (the transposed convolution's GEMM output, columns (ky, kx, n)) -> the pitched grid
    [frames*gh*k*(gw*k+1), Cout] + bias."""
    _req(src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and tuple(src.shape) == (frames * gh * src_pitch, k * k * Cout) and
         bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Cout, "deconv_scatter: bad src / bias")
    out = torch.empty(frames * gh * k * (gw * k + 1), Cout, dtype=torch.float32, device=src.device)
    check(lib().gd_deconv_scatter(ptr(src), ptr(bias), ptr(out), frames, gh, gw, src_pitch, k, Cout, stream()), "gd_deconv_scatter")
    return out


def dpt_head_out(x, w, bias, frames, H, W, activation, conf_activation):
    """x: pitched [frames*H*(W+1), Cin] fp32, w [od, Cin], bias [od] -> preds [frames, H, W, od-1], conf [frames, H, W] (gd_dpt_head_out)."""
    _req(activation in DPT_ACT, f"dpt_head_out: activation {activation!r}: served are {sorted(DPT_ACT)}")
    _req(conf_activation in DPT_CONF_ACT, f"dpt_head_out: conf_activation {conf_activation!r}: served are {sorted(DPT_CONF_ACT)}")
    od, Cin = w.shape
    _req(all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (x, w, bias)) and tuple(x.shape) == (frames * H * (W + 1), Cin) and
         bias.numel() == od, "dpt_head_out: bad x / w / bias")
    preds = torch.empty(frames, H, W, max(od - 1, 0), dtype=torch.float32, device=x.device)
    conf = torch.empty(frames, H, W, dtype=torch.float32, device=x.device)
    check(lib().gd_dpt_head_out(ptr(x), ptr(w), ptr(bias), ptr(preds), ptr(conf), frames, H, W, Cin, od, DPT_ACT[activation],
                                DPT_CONF_ACT[conf_activation], stream()), "gd_dpt_head_out")
    return preds, conf


MH_PTS = {"linear": 0, "square": 1, "exp": 2}                 # include/gd_hip.h GD_MH_PTS_* ("linear": the value before the activation)
MH_CONF = {"exp": 0, "sigmoid": 1, "raw": 2}                  # GD_MH_CONF_*
MH_DESC = {"norm": 0, "raw": 1}                               # GD_MH_DESC_*


def mast3r_head_out(x, w, bias, lf, frames, H, W, *, patch=16, desc_dim=0, two_confs=False, pts_mode="linear", conf_mode=("raw", 0.0, 0.0),
                    desc_mode="norm", desc_conf_mode=("raw", 0.0, 0.0)):
    """x: pitched [frames*H*(W+1), Cin] fp32, w [od, Cin], bias [od] (od = 3 | 4), lf: None or token rows [frames*(H/patch)*(W/patch),
    patch*patch*(desc_dim + two_confs)] fp32 with columns packed (i, j, c) -> (pts3d [frames, H, W, 3], conf [frames, H, W] or None when od = 3,
    desc [frames, H, W, desc_dim], desc_conf [frames, H, W]; the last two None without lf) (gd_mast3r_head_out).  conf_mode, desc_conf_mode:
    (mode, vmin, vmax)."""
    _req(pts_mode in MH_PTS, f"mast3r_head_out: pts3d mode {pts_mode!r}: served are {sorted(MH_PTS)}")
    _req(conf_mode[0] in MH_CONF, f"mast3r_head_out: conf mode {conf_mode[0]!r}: served are {sorted(MH_CONF)}")
    _req(desc_conf_mode[0] in MH_CONF, f"mast3r_head_out: desc_conf mode {desc_conf_mode[0]!r}: served are {sorted(MH_CONF)}")
    _req(desc_mode in MH_DESC, f"mast3r_head_out: desc mode {desc_mode!r}: served are {sorted(MH_DESC)}")
    _req(w.dim() == 2, "mast3r_head_out: w is [od, Cin]")
    od, Cin = w.shape
    _req(all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (x, w, bias)) and tuple(x.shape) == (frames * H * (W + 1), Cin) and
         bias.numel() == od, "mast3r_head_out: bad x / w / bias")
    tc = 1 if two_confs else 0
    pts3d = torch.empty(frames, H, W, 3, dtype=torch.float32, device=x.device)
    conf = torch.empty(frames, H, W, dtype=torch.float32, device=x.device) if od == 4 else None
    desc = desc_conf = None
    if lf is not None:
        _req(patch >= 1 and H % patch == 0 and W % patch == 0 and desc_dim >= 1, "mast3r_head_out: H, W must be multiples of patch, desc_dim >= 1")
        _req(lf.is_cuda and lf.dtype == torch.float32 and lf.is_contiguous() and
             tuple(lf.shape) == (frames * (H // patch) * (W // patch), patch * patch * (desc_dim + tc)), "mast3r_head_out: bad lf")
        desc = torch.empty(frames, H, W, desc_dim, dtype=torch.float32, device=x.device)
        desc_conf = torch.empty(frames, H, W, dtype=torch.float32, device=x.device)
    check(lib().gd_mast3r_head_out(ptr(x), ptr(w), ptr(bias), ptr(lf), ptr(pts3d), ptr(conf), ptr(desc), ptr(desc_conf), frames, H, W, Cin, od, int(patch),
                                   int(desc_dim), tc, MH_PTS[pts_mode], MH_CONF[conf_mode[0]], float(conf_mode[1]), float(conf_mode[2]), MH_DESC[desc_mode],
                                   MH_CONF[desc_conf_mode[0]], float(desc_conf_mode[1]), float(desc_conf_mode[2]), stream()), "gd_mast3r_head_out")
    return pts3d, conf, desc, desc_conf


class _TapMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prefix, with_norm, *grids):
        B, Nt, D = grids[0].shape
        gs = [g.contiguous() for g in grids]
        out = torch.empty(B, Nt - prefix, D, dtype=gs[0].dtype, device=gs[0].device)
        ctx.meta = (prefix, len(gs), B, Nt, D)
        ctx.set_materialize_grads(False)      # (the inverse norms / the fp16 copy are not differentiable: no zero-filled [B, hw, D] "gradient" for them)
        if with_norm == 2:      # + the fp16 copy of the rows (tf32h engine: the cost-volume products' operands)
            _req(out.dtype == torch.float32 and D % 8 == 0, "tap_mean(with_norm=2): fp32 taps, D % 8 == 0")
            inv = torch.empty(B, Nt - prefix, dtype=torch.float32, device=gs[0].device)
            o16 = torch.empty(B, Nt - prefix, D, dtype=torch.float16, device=gs[0].device)
            check(lib().gd_tap_mean_norm_fwd_h(_ptr_array(gs), len(gs), Nt * D, prefix, ptr(out), ptr(o16), ptr(inv), B, Nt - prefix, D, stream()),
                  "gd_tap_mean_norm_fwd_h")
            ctx.mark_non_differentiable(inv, o16)
            return out, inv, o16
        if with_norm:
            inv = torch.empty(B, Nt - prefix, dtype=torch.float32, device=gs[0].device)
            check(lib().gd_tap_mean_norm_fwd(_ptr_array(gs), len(gs), Nt * D, prefix, ptr(out), ptr(inv), B, Nt - prefix, D,
                                             dtype_code(out), stream()), "gd_tap_mean_norm_fwd")
            ctx.mark_non_differentiable(inv)
            return out, inv
        check(lib().gd_tap_mean_fwd(_ptr_array(gs), len(gs), Nt * D, prefix, ptr(out), B, Nt - prefix, D,
                                    dtype_code(out), stream()), "gd_tap_mean_fwd")
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        prefix, ng, B, Nt, D = ctx.meta
        if dout is None:
            return (None, None) + (None,) * ng
        dout = dout.contiguous()
        # the ng gradients are identical (dout / ng): one buffer, handed to every grid
        dg = torch.empty(B, Nt, D, dtype=dout.dtype, device=dout.device)
        check(lib().gd_tap_mean_bwd(_ptr_array([dg]), 1, prefix, ptr(dout), B, Nt - prefix, D, 1.0 / ng, dtype_code(dout),
                                    stream()), "gd_tap_mean_bwd")
        return (None, None) + (dg,) * ng


def tap_mean(grids, prefix=1, with_norm=False):
    """mean of 1..4 tap outputs [B, prefix+hw, D], prefix tokens dropped -> contiguous [B, hw, D]; with_norm: -> (mean, inv_norm
    [B, hw] fp32 = 1 / max(||row||, 1e-12) of the rows as stored, not differentiable: an input of cost_volume_kl(inv_norms=...));
    with_norm=2 (fp32 taps): -> (mean, inv_norm, fp16 copy of mean) — cost_volume_kl(x3="h", h16=...)."""
    return _TapMean.apply(prefix, 2 if with_norm == 2 else bool(with_norm), *grids)


def kp_depth(depth, kp):
    """depth [B,H,W] f32, kp [B,Nk,2] (x,y) -> [B,Nk] 3x3 mean depth (extract_kp_depth)."""
    B, H, W = depth.shape
    Nk = kp.shape[1]
    out = torch.empty(B, Nk, dtype=torch.float32, device=kp.device)
    dm, kq = depth.contiguous().float(), kp.contiguous().float()      # keep both alive across the launch
    check(lib().gd_kp_depth(ptr(dm), ptr(kq), ptr(out), B, Nk, H, W, stream()), "gd_kp_depth")
    return out


def patch_mask(kp, H, W, P):
    """kp [B,Nk,2] -> uint8 [B, (H//P)*(W//P)] (get_patch_mask_from_kp_tensor)."""
    B, Nk, _ = kp.shape
    mask = torch.zeros(B, (H // P) * (W // P), dtype=torch.uint8, device=kp.device)
    kq = kp.contiguous().float()
    check(lib().gd_patch_mask(ptr(kq), ptr(mask), B, Nk, H, W, P, stream()), "gd_patch_mask")
    return mask


# ----------------------------------------------------------------------------------------------
# sparse losses
# ----------------------------------------------------------------------------------------------
_CONST = {}


def _const(kind, n, value, device):
    """small constant device vectors (all-ones scales, full keypoint counts), built once per (kind, length, value, device)."""
    key = (kind, int(n), value, device)
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.full((int(n),), value, dtype=torch.int32 if kind == "i" else torch.float32, device=device)
    return t


class _SmoothAP(torch.autograd.Function):
    """desc [2P, N0, C]: the unit descriptors of view 1 (first P) and view 2 (last P) as the extractor returns them — one buffer in, one gradient
    buffer out (no per-view slices, concatenations or per-tensor padding passes)."""

    @staticmethod
    def forward(ctx, desc, pts1, pts2, counts, variant, thr, temp):
        P2, N0, C = desc.shape
        P = P2 // 2
        N = (N0 + 7) // 8 * 8                                      # gemm_tn wants multiples of 8: zero-pad keypoints
        dev = desc.device
        if counts is None:
            counts = _const("i", P, N0, dev)
        desc = desc.float()
        if N == N0:
            d12 = desc.contiguous()
            pp = torch.stack([pts1, pts2]).float().contiguous()
        else:      # ONE zero-filled buffer for the padded descriptors and points of both views
            buf = torch.zeros(P2 * N * (C + 4), dtype=torch.float32, device=dev)
            d12 = buf[:P2 * N * C].view(P2, N, C)
            pp = buf[P2 * N * C:P2 * N * (C + 3)].view(2, P, N, 3)
            d12[:, :N0] = desc
            pp[0, :, :N0] = pts1
            pp[1, :, :N0] = pts2
        d1, d2 = d12[:P], d12[P:]
        sim = gemm_nt(d1, d2)                                     # [P,N,N] fp32, exact-f32 MFMA
        loss = torch.empty(P, dtype=torch.float32, device=dev)
        dsim = torch.empty_like(sim)
        rows = torch.empty(P, N, 2, dtype=torch.float32, device=dev)
        if variant == "me":      # every pair closer than thr[0] is a positive (src/finetune_timm_me.py:191-220)
            rc = lib().gd_smooth_ap_me(ptr(sim), ptr(pp[0]), ptr(pp[1]), ptr(counts), P, N, float(thr[0]), float(thr[1]),
                                       float(temp), ptr(loss), ptr(dsim), ptr(rows), stream())
            check(rc, "gd_smooth_ap_me")
        else:
            rc = lib().gd_smooth_ap(ptr(sim), ptr(pp[0]), ptr(pp[1]), ptr(counts), P, N, VARIANTS[variant], float(thr),
                                    float(temp), ptr(loss), ptr(dsim), ptr(rows), stream())
            check(rc, "gd_smooth_ap")
        ctx.save_for_backward(d12, dsim)
        ctx.n0 = N0
        return loss

    @staticmethod
    def backward(ctx, g):
        d12, dsim = ctx.saved_tensors
        P, N, _ = dsim.shape
        d1, d2 = d12[:P], d12[P:]
        gs, gst = torch.empty_like(dsim), torch.empty_like(dsim)
        check(lib().gd_scale_and_transpose(ptr(dsim), ptr(g.contiguous().float()), ptr(gs), ptr(gst), P, N, N, stream()), "gd_scale_and_transpose")
        dd = torch.zeros_like(d12)                                 # (gemm_tn accumulates)
        gemm_tn(gst, d2, out=dd[:P])                              # [P,N,C] = (dsim g) d2
        gemm_tn(gs, d1, out=dd[P:])                               # [P,N,C] = (dsim g)^T d1
        return dd[:, :ctx.n0], None, None, None, None, None, None


def smooth_ap_pairs(desc, P, pts3d_1, pts3d_2, counts=None, variant="vggt", thres3d_neg=0.1, temp=0.01, thres3d_pos=5e-3):
    """smooth_ap on the view-major batch the extractor returns: desc [2P, N, C] (view 1 of all pairs, then view 2) -> loss [P]."""
    _req(desc.shape[0] == 2 * P, "smooth_ap_pairs: desc must be [2P, N, C]")
    thr = (thres3d_pos, thres3d_neg) if variant == "me" else thres3d_neg
    return _SmoothAP.apply(desc, pts3d_1, pts3d_2, counts, variant, thr, temp)


def smooth_ap(desc1, desc2, pts3d_1, pts3d_2, counts=None, variant="vggt", thres3d_neg=0.1, temp=0.01, thres3d_pos=5e-3):
    """desc [P,N,C] unit descriptors, pts3d [P,N,3], counts int32 [P] (valid keypoints per pair) -> loss [P].
    variant "vggt" | "mast3r": positives on the diagonal; "me": every pair closer than thres3d_pos (finetune_timm_me.py)."""
    return smooth_ap_pairs(torch.cat([desc1, desc2], 0), desc1.shape[0], pts3d_1, pts3d_2, counts, variant, thres3d_neg, temp, thres3d_pos)


HEAD_KEYS = ("w1", "b1", "ln_w", "ln_b", "w2", "b2")


class _DepthLosses(torch.autograd.Function):
    """depth L1 + intra-view ranking on keypoint features [P,2,N,D] with the DepthAwareFeatureFusion head.
    The loss kernels are fused forward+backward: they emit, per keypoint set, the loss AND its gradients for a
    unit upstream gradient; backward() scales and adds them in one pass (gd_depth_bwd_combine) and contracts."""

    @staticmethod
    def forward(ctx, feats, d1, d2, counts, thr, w1, b1, ln_w, ln_b, w2, b2):
        vm = feats.dim() == 3                  # [2P,N,D] view-major (view 1 of all pairs, then view 2): no big transpose —
        dev = feats.device                     # the head's first layer is row-wise, so only its 128-wide output is re-ordered
        f = feats.contiguous().float()
        if vm:
            P, N, D = feats.shape[0] // 2, feats.shape[1], feats.shape[2]
            u = gemm_nt(f.view(2 * P * N, D), w1.contiguous()).view(2, P, N, 128).transpose(0, 1).contiguous()
        else:
            P, _, N, D = feats.shape
            u = gemm_nt(f.view(P * 2 * N, D), w1.contiguous())         # [P*2*N,128] = W1 f
        dv1, dv2 = d1.contiguous().float(), d2.contiguous().float()
        depth = torch.stack([dv1, dv2], 1)                         # [P,2,N]
        cnt2 = counts.repeat_interleave(2).contiguous() if counts is not None else None
        hp = [t.contiguous().float() for t in (b1, ln_w, ln_b, w2.view(-1), b2)]
        rank = torch.empty(2 * P, dtype=torch.float32, device=dev)
        du_r = torch.empty(2 * P, N, 128, dtype=torch.float32, device=dev)
        hg_r = torch.empty(2 * P, 516, dtype=torch.float32, device=dev)
        ws = torch.empty(lib().gd_pair_rank_workspace_bytes(2 * P), dtype=torch.uint8, device=dev)
        check(lib().gd_pair_rank(ptr(u), ptr(depth), ptr(cnt2), None, 2 * P, N, float(thr), *[ptr(t) for t in hp],
                                 ptr(rank), ptr(du_r), None, ptr(hg_r), ptr(ws), stream()), "gd_pair_rank")
        l1 = torch.empty(P, dtype=torch.float32, device=dev)
        du_l = torch.empty(P, 2, N, 128, dtype=torch.float32, device=dev)
        hg_l = torch.empty(P, 516, dtype=torch.float32, device=dev)
        check(lib().gd_depth_l1(ptr(u), ptr(dv1), ptr(dv2), ptr(counts), None, P, N, *[ptr(t) for t in hp],
                                ptr(l1), ptr(du_l), None, ptr(hg_l), None, stream()), "gd_depth_l1")
        ctx.save_for_backward(f, w1, du_r, du_l, hg_r, hg_l)
        ctx.dims = (P, N, D, vm)
        return l1, rank.view(P, 2).mean(1)

    @staticmethod
    def backward(ctx, g_l1, g_intra):
        f, w1, du_r, du_l, hg_r, hg_l = ctx.saved_tensors
        P, N, D, vm = ctx.dims
        dev = f.device
        du = torch.empty(P * 2 * N, 128, dtype=torch.float32, device=dev)                # rows in the order of f
        hg = torch.empty(516, dtype=torch.float32, device=dev)
        check(lib().gd_depth_bwd_combine(ptr(du_r), ptr(du_l), ptr(hg_r), ptr(hg_l), ptr(g_l1.contiguous().float()), ptr(g_intra.contiguous().float()),
                                         P, N, 1 if vm else 0, ptr(du), ptr(hg), stream()), "gd_depth_bwd_combine")
        df = gemm_nt(du, w1.t().contiguous()).view(f.shape)        # du . W1
        dw1 = gemm_tn(du, f.view(P * 2 * N, D))                    # du^T f  [128, D]
        return (df, None, None, None, None, dw1, hg[0:128], hg[128:256], hg[256:384], hg[384:512].view(1, 128), hg[512:513])


def depth_losses(feats, depth_1, depth_2, head, counts=None, depth_threshold=0.05):
    """feats [P,2,N,D] keypoint features of both views — or [2P,N,D] view-major as the extractor returns them —, depth_k
    [P,N]; head: dict w1,b1,ln_w,ln_b,w2,b2.  -> (depth_l1 [P], intra_rank [P])  (calculate_depth_loss tail)."""
    return _DepthLosses.apply(feats, depth_1, depth_2, counts, depth_threshold, head["w1"], head["b1"], head["ln_w"],
                              head["ln_b"], head["w2"], head["b2"])


class _DepthHead(torch.autograd.Function):
    """Eager DepthAwareFeatureFusion rows: tanh(fusion_layer(f)) for f [M, D] -> [M] (utils/model.py:101-127)."""

    @staticmethod
    def forward(ctx, feats, w1, b1, ln_w, ln_b, w2, b2):
        shp = feats.shape
        f = feats.reshape(-1, shp[-1]).contiguous().float()
        M = f.shape[0]
        w1c = w1.detach().float().contiguous()
        u = gemm_nt(f, w1c)                                                   # [M, 128]
        hp = [t.detach().contiguous().float() for t in (b1, ln_w, ln_b, w2.reshape(-1), b2)]
        out = torch.empty(M, dtype=torch.float32, device=f.device)
        check(lib().gd_depth_head_fwd(ptr(u), M, *[ptr(t) for t in hp], ptr(out), stream()), "gd_depth_head_fwd")
        ctx.save_for_backward(f, w1c, u, *hp)
        ctx.shp = shp
        return out.view(shp[:-1])

    @staticmethod
    def backward(ctx, dout):
        f, w1c, u, *hp = ctx.saved_tensors
        M = f.shape[0]
        dz = dout.reshape(-1).contiguous().float()
        du = torch.empty_like(u)
        hg = torch.zeros(516, dtype=torch.float32, device=f.device)
        check(lib().gd_depth_head_bwd(ptr(u), ptr(dz), M, *[ptr(t) for t in hp], ptr(du), ptr(hg), stream()), "gd_depth_head_bwd")
        df = gemm_nt(du, w1c.t().contiguous()).view(ctx.shp)
        dw1 = gemm_tn(du, f)
        return (df, dw1, hg[0:128].clone(), hg[128:256].clone(), hg[256:384].clone(), hg[384:512].view(1, 128).clone(),
                hg[512:513].clone())


def depth_head(feats, head):
    """feats [..., D] -> tanh(w2 . GELU(LN(W1 f + b1)) + b2) [...]; head: dict w1,b1,ln_w,ln_b,w2,b2."""
    return _DepthHead.apply(feats, head["w1"], head["b1"], head["ln_w"], head["ln_b"], head["w2"], head["b2"])


class _PairRank(torch.autograd.Function):
    """pairwise_logistic_ranking_loss over B keypoint sets, the reference's GLOBAL mean over the valid pairs of all sets
    (utils/losses.py:36-40): per-set means from gd_pair_rank, re-weighted by the per-set valid-pair counts."""

    @staticmethod
    def forward(ctx, feats, depths, thr, w1, b1, ln_w, ln_b, w2, b2):
        B, N, D = feats.shape
        dev = feats.device
        f = feats.contiguous().float()
        w1c = w1.detach().float().contiguous()
        u = gemm_nt(f.view(B * N, D), w1c).view(B, N, 128)
        hp = [t.detach().contiguous().float() for t in (b1, ln_w, ln_b, w2.reshape(-1), b2)]
        ones = torch.ones(B, dtype=torch.float32, device=dev)
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        du = torch.empty(B, N, 128, dtype=torch.float32, device=dev)
        hg = torch.empty(B, 516, dtype=torch.float32, device=dev)
        nbytes = lib().gd_pair_rank_workspace_bytes(B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dd = depths.contiguous().float()
        check(lib().gd_pair_rank(ptr(u), ptr(dd), None, ptr(ones), B, N, float(thr), *[ptr(t) for t in hp], ptr(loss),
                                 ptr(du), None, ptr(hg), ptr(ws), stream()), "gd_pair_rank")
        cnt = ws[(B * 517) * 4:(B * 518) * 4].view(torch.int32).float()         # workspace layout: hg [B,516] | loss_sum [B] | pair_cnt [B]
        wgt = cnt / cnt.sum().clamp_min(1.0)
        ctx.save_for_backward(f, w1c, du, hg, wgt)
        return (loss * wgt).sum()

    @staticmethod
    def backward(ctx, g):
        f, w1c, du, hg, wgt = ctx.saved_tensors
        B, N, D = f.shape
        sc = (g.float() * wgt)
        du = (du * sc.view(B, 1, 1)).view(B * N, 128)
        hgs = (hg * sc[:, None]).sum(0)
        df = gemm_nt(du, w1c.t().contiguous()).view(B, N, D)
        dw1 = gemm_tn(du, f.view(B * N, D))
        return (df, None, None, dw1, hgs[0:128].clone(), hgs[128:256].clone(), hgs[256:384].clone(),
                hgs[384:512].view(1, 128).clone(), hgs[512:513].clone())


def pair_rank_loss(feats, depths, head, depth_threshold=0.0):
    """feats [B,N,D], depths [B,N] -> scalar: mean of log(1 + exp(-sign(d_j - d_i) head(f_j - f_i))) over the pairs with
    |d_j - d_i| > depth_threshold (0 when there is none)."""
    return _PairRank.apply(feats, depths, depth_threshold, head["w1"], head["b1"], head["ln_w"], head["ln_b"], head["w2"],
                           head["b2"])


class _LossCombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ap, depth, intra, kl, counts, weights):
        P = ap.shape[0]
        ts = [t.contiguous().float() for t in (ap, depth, intra, kl)]
        w4 = (ctypes_float_array(weights))
        loss = torch.empty((), dtype=torch.float32, device=ap.device)
        terms = torch.empty(4, P, dtype=torch.float32, device=ap.device)
        cnt = counts.contiguous().to(device=ap.device, dtype=torch.int32) if counts is not None else None
        check(lib().gd_loss_combine_fwd(*[ptr(t) for t in ts], w4, ptr(cnt), P, ptr(loss), ptr(terms), stream()), "gd_loss_combine_fwd")
        ctx.cfg = (tuple(float(w) for w in weights), cnt, P)
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss, terms

    @staticmethod
    def backward(ctx, g, _unused=None):
        weights, cnt, P = ctx.cfg
        if g is None:
            return None, None, None, None, None, None
        grads = torch.empty(4, P, dtype=torch.float32, device=g.device)
        check(lib().gd_loss_combine_bwd(ptr(g.contiguous().float()), ctypes_float_array(weights), ptr(cnt), P, ptr(grads), stream()), "gd_loss_combine_bwd")
        return grads[0], grads[1], grads[2], grads[3], None, None


def loss_combine(ap, depth, intra, kl, weights, counts=None):
    """The step's scalar loss = mean over pairs of (w_ap ap + w_depth depth + w_intra intra + w_kl kl), a pair with counts[p] == 0 contributing a
    constant zero (src/finetune_timm_vggt.py:599-616, src/finetune_timm_mast3r.py:604-607, 650-653) -> (loss [], terms [4, P] masked the same way,
    not differentiable).  One launch each way instead of ~20 elementwise / reduce launches on [P]-vectors."""
    return _LossCombine.apply(ap, depth, intra, kl, counts, tuple(weights))


def ctypes_float_array(vals):
    import ctypes
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


# ----------------------------------------------------------------------------------------------
# stand-alone forms of the reference's loss helpers (compat.py); the step uses the fused ops above
# ----------------------------------------------------------------------------------------------
class _SigmoidTemp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, temp):
        xc = x.contiguous().float()
        y = torch.empty_like(xc)
        check(lib().gd_sigmoid_temp(ptr(xc), None, ptr(y), xc.numel(), float(temp), stream()), "gd_sigmoid_temp")
        ctx.save_for_backward(xc)
        ctx.temp = float(temp)
        return y

    @staticmethod
    def backward(ctx, dy):
        (xc,) = ctx.saved_tensors
        dyc = dy.contiguous().float()
        dx = torch.empty_like(xc)
        check(lib().gd_sigmoid_temp(ptr(xc), ptr(dyc), ptr(dx), xc.numel(), ctx.temp, stream()), "gd_sigmoid_temp")
        return dx, None


def sigmoid_temp(x, temp=1.0):
    return _SigmoidTemp.apply(x, temp)


class _MaskedPatchCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, m1, m2, eps, use_softmax, temperature):
        B, R, C = cost.shape
        c = cost.contiguous().float()
        m1c = m1.contiguous().to(torch.uint8)
        m2c = m2.contiguous().to(torch.uint8) if m2 is not None else None
        _req(m1c.numel() == R and (m2c is None or m2c.numel() == C), "masked_patch_cost: mask sizes")
        y = torch.empty_like(c)
        check(lib().gd_masked_patch_cost_fwd(ptr(c), ptr(m1c), ptr(m2c), ptr(y), B, R, C, float(eps), int(bool(use_softmax)),
                                             float(temperature), stream()), "gd_masked_patch_cost_fwd")
        ctx.save_for_backward(c, y, m1c, m2c)
        ctx.cfg = (float(eps), int(bool(use_softmax)), float(temperature))
        return y

    @staticmethod
    def backward(ctx, dy):
        c, y, m1c, m2c = ctx.saved_tensors
        B, R, C = c.shape
        dyc = dy.contiguous().float()
        dc = torch.empty_like(c)
        eps, sm, temp = ctx.cfg
        check(lib().gd_masked_patch_cost_bwd(ptr(c), ptr(y), ptr(dyc), ptr(m1c), ptr(m2c), ptr(dc), B, R, C, eps, sm, temp,
                                             stream()), "gd_masked_patch_cost_bwd")
        return dc, None, None, None, None, None


def masked_patch_cost(cost, m1, m2=None, eps=1e-8, use_softmax=False, temperature=1.0):
    return _MaskedPatchCost.apply(cost, m1, m2, eps, use_softmax, temperature)


class _KLMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, p, eps):
        _req(t.shape == p.shape, "kl_divergence_map: shapes differ")
        tc, pc = t.contiguous().float(), p.contiguous().float()
        cols = tc.shape[-1]
        rows = tc.numel() // cols
        loss = torch.empty(1, dtype=torch.float32, device=tc.device)
        ws = torch.empty(rows, dtype=torch.float32, device=tc.device)
        check(lib().gd_kl_divergence_map_fwd(ptr(tc), ptr(pc), rows, cols, float(eps), ptr(loss), ptr(ws), stream()),
              "gd_kl_divergence_map_fwd")
        ctx.save_for_backward(tc, pc)
        ctx.eps = float(eps)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        tc, pc = ctx.saved_tensors
        cols = tc.shape[-1]
        rows = tc.numel() // cols
        gt, gp = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dt = torch.empty_like(tc) if gt else None
        dp = torch.empty_like(pc) if gp else None
        gg = g.reshape(1).contiguous().float()
        check(lib().gd_kl_divergence_map_bwd(ptr(tc), ptr(pc), ptr(gg), rows, cols, ctx.eps, ptr(dt), ptr(dp), stream()),
              "gd_kl_divergence_map_bwd")
        return dt, dp, None


def kl_divergence_map(t, p, eps=1e-8):
    return _KLMap.apply(t, p, eps)


# ----------------------------------------------------------------------------------------------
# optimiser
# ----------------------------------------------------------------------------------------------
def clip_adamw_step(params, grads, exp_avg, exp_avg_sq, step, lr=1e-5, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8,
                    max_norm=1.0, grad_scale=1.0, ranges=None):
    """In place on the flat fp32 buffers; returns the pre-clip global grad norm (device scalar).  `ranges` = [(a, b), ...]
    restricts the UPDATE (moments, decay, step) to those element ranges — parameters outside them are left untouched, as
    torch.optim.AdamW leaves a parameter whose .grad is None; the norm is always taken over the whole buffer (their
    gradient slice is zero)."""
    norm = torch.empty(1, dtype=torch.float32, device=params.device)
    ws = torch.empty(lib().gd_adamw_workspace_bytes(), dtype=torch.uint8, device=params.device)
    n = params.numel()
    if not ranges or (len(ranges) == 1 and tuple(ranges[0]) == (0, n)):
        check(lib().gd_clip_adamw_step(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), n, int(step),
                                       lr, weight_decay, betas[0], betas[1], eps, max_norm, grad_scale, ptr(norm), ptr(ws),
                                       stream()), "gd_clip_adamw_step")
        return norm
    check(lib().gd_clip_adamw_ranges(ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), n, int(step), lr, weight_decay,
                                     betas[0], betas[1], eps, max_norm, grad_scale, ptr(norm), ptr(ws),
                                     (ctypes_long_array([x for ab in ranges for x in ab])), len(ranges), stream()),
          "gd_clip_adamw_ranges")
    return norm


def ctypes_long_array(vals):
    import ctypes
    return (ctypes.c_long * len(vals))(*[int(v) for v in vals])


def cast(x, dtype, scale=1.0):
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    check(lib().gd_cast(ptr(x), ptr(out), x.numel(), float(scale), dtype_code(x), dtype_code(out), stream()), "gd_cast")
    return out


# ---------------------------------------------------------------------------------------------------------------- correspondence evaluation
class MatchResult(tuple):
    """(row_idx, col_idx, mutual, row_score, col_score) of `match_argmax`; fields that were not asked for are None."""
    __slots__ = ()
    _fields = ("row_idx", "col_idx", "mutual", "row_score", "col_score")

    def __new__(cls, *vals):
        return tuple.__new__(cls, vals)

    row_idx = property(lambda s: s[0])
    col_idx = property(lambda s: s[1])
    mutual = property(lambda s: s[2])
    row_score = property(lambda s: s[3])
    col_score = property(lambda s: s[4])


_MATCH_TARGET = 32768.0      # fp16 operands: max |x| * s in (2^14, 2^15] — half of fp16's range is left as headroom, nothing can saturate


def _f16_operand(x):
    """f32 [rows, D] -> (fp16 copy under a power-of-two scale, device scalar 1/s).  A non-finite element is an error, not a NaN scale."""
    sc = amax_scale(x, _MATCH_TARGET)
    _req(bool(torch.isfinite(sc[0]).item()), "match_argmax: the operand holds a non-finite element")
    out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    check(lib().gd_cast_f16_ex(ptr(x), ptr(out), x.shape[0], x.shape[1], x.stride(0), 1.0, ptr(sc[0:1]), None, stream()), "gd_cast_f16_ex")
    return out, sc[1:2]


def match_argmax(a, b, *, both=True, precision="f16", want_scores=False, want_mutual=False):
    """Nearest neighbours by dot product in both directions from one pass (gd_match_argmax): a [M, D], b [N, D] (D a multiple of 8) ->
    MatchResult(row_idx [M] int64 = argmax_j a_i . b_j, col_idx [N] int64 = argmax_i a_i . b_j (both=True), mutual [M] bool =
    (col_idx[row_idx] == arange(M)) (want_mutual), row_score / col_score fp32 (want_scores)).  Ties pick the smallest index, as
    torch.argmax does.  precision "f32": exact fp32 products of fp32 inputs; "f16": fp32 inputs rounded to fp16 under a power-of-two
    per-tensor scale (the reference's TF32 class; argmax is scale-invariant) or fp16 inputs as they are; "bf16": bf16 inputs."""
    _req(precision in ("f32", "f16", "bf16"), f"match_argmax: precision must be 'f32', 'f16' or 'bf16', not {precision!r}")
    _req(a.dim() == 2 and b.dim() == 2, "match_argmax: a and b must be 2-D [rows, D]")
    _req(a.shape[1] == b.shape[1], f"match_argmax: descriptor widths differ ({a.shape[1]} vs {b.shape[1]})")
    (M, D), N = a.shape, b.shape[0]
    _req(M > 0 and N > 0 and D > 0 and D % 8 == 0, f"match_argmax: need non-empty inputs and D a multiple of 8 (M={M} N={N} D={D})")
    _req(not want_mutual or both, "match_argmax: the mutual mask needs both directions")
    _req(a.is_cuda and b.is_cuda, "match_argmax: a and b must be CUDA tensors")
    inv_a = inv_b = None
    if precision == "f32":
        _req(a.dtype == torch.float32 and b.dtype == torch.float32, "match_argmax: precision 'f32' takes fp32 inputs")
        a, b = a.contiguous(), b.contiguous()
    elif precision == "bf16":
        _req(a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16, "match_argmax: precision 'bf16' takes bf16 inputs")
        a, b = a.contiguous(), b.contiguous()
    else:
        _req(a.dtype in (torch.float32, torch.float16) and b.dtype in (torch.float32, torch.float16), "match_argmax: precision 'f16' takes fp32 or fp16 inputs")
        if a.dtype == torch.float32:
            a, inv_a = _f16_operand(a.contiguous())
        if b.dtype == torch.float32:
            b, inv_b = _f16_operand(b.contiguous())
        a, b = a.contiguous(), b.contiguous()
    dev = a.device
    flags = _lib.MATCH_COLS if both else 0
    ws = torch.empty(lib().gd_match_argmax_workspace_bytes(M, N, flags), dtype=torch.uint8, device=dev)
    row = torch.empty(M, dtype=torch.int64, device=dev)
    col = torch.empty(N, dtype=torch.int64, device=dev) if both else None
    mut = torch.empty(M, dtype=torch.bool, device=dev) if want_mutual else None
    rs = torch.empty(M, dtype=torch.float32, device=dev) if want_scores else None
    cs = torch.empty(N, dtype=torch.float32, device=dev) if want_scores and both else None
    check(lib().gd_match_argmax(ptr(a), ptr(b), M, N, D, dtype_code(a), flags, ptr(inv_a), ptr(inv_b), ptr(row), ptr(rs), ptr(col), ptr(cs),
                                ptr(mut), ptr(ws), stream()), "gd_match_argmax")
    return MatchResult(row, col, mut, rs, cs)


def transfer_argmax(S, img_hw, patch, stride, *, want_score=False):
    """Semantic-transfer argmax over the upsampled, edge-padded score field (gd_transfer_argmax): S [K, gh, gw] fp32 (or [K, gh, pitch]
    with only the first gw = 1 + (img_w - patch) // stride columns used) -> xy [K, 2] int64 (x, y) of the raster-first maximum of
    pad(interpolate(S, (ds_h, ds_w), bilinear, align_corners=True)), ds = ((img - patch) // stride) * stride + 1, edge pads patch // 2
    top / left; (xy, score [K]) with want_score."""
    img_h, img_w = (int(v) for v in img_hw)
    _req(S.dtype == torch.float32 and S.dim() == 3, "transfer_argmax: S must be a 3-D fp32 tensor [K, gh, gw]")
    _req(patch > 0 and stride > 0 and img_h >= patch and img_w >= patch, f"transfer_argmax: bad geometry image {img_h}x{img_w} patch {patch} stride {stride}")
    K, gh, pitch = S.shape
    gw = 1 + (img_w - patch) // stride
    _req(gh == 1 + (img_h - patch) // stride and pitch >= gw,
         f"transfer_argmax: score grid {gh}x{pitch} does not match image {img_h}x{img_w} at patch {patch}, stride {stride} "
         f"(expected {1 + (img_h - patch) // stride}x{gw})")
    _req(S.is_cuda, "transfer_argmax: S must be a CUDA tensor")
    S = S.contiguous()
    xy = torch.empty(K, 2, dtype=torch.int64, device=S.device)
    sc = torch.empty(K, dtype=torch.float32, device=S.device) if want_score else None
    ws = torch.empty(lib().gd_transfer_argmax_workspace_bytes(K), dtype=torch.uint8, device=S.device)
    check(lib().gd_transfer_argmax(ptr(S), K, gh, gw, pitch, img_h, img_w, int(patch), int(stride), ptr(xy), ptr(sc), ptr(ws), stream()),
          "gd_transfer_argmax")
    return (xy, sc) if want_score else xy


# ---------------------------------------------------------------------------------------------------------------- tracking evaluation
def row_norms(x):
    """||x_r|| fp32 for every row of a CUDA tensor [..., D] (fp32 / fp16 / bf16; gd_track_row_norms) -> [...] fp32."""
    _req(x.is_cuda and x.dim() >= 1 and x.shape[-1] > 0, "row_norms: a CUDA tensor [..., D] with D > 0")
    x = x.contiguous()
    out = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    rows = x.numel() // x.shape[-1]
    if rows:
        check(lib().gd_track_row_norms(ptr(x), rows, x.shape[-1], dtype_code(x), ptr(out), stream()), "gd_track_row_norms")
    return out


class TrackFeatures:
    """A video's token grid prepared once for `track_points`: the fp32 (or input) features, their per-cell norms, and the MFMA operand
    (for precision "f16": an fp16 copy of the fp32 grid under a power-of-two scale).  feats [T, gh * pitch, D] token-major."""

    def __init__(self, feats, precision="f16"):
        _req(precision in ("f32", "f16", "bf16"), f"track_points: precision must be 'f32', 'f16' or 'bf16', not {precision!r}")
        _req(feats.is_cuda and feats.dim() == 3, "track_points: feats must be a CUDA tensor [T, gh * pitch, D]")
        self.src = feats.contiguous()
        self.precision = precision
        self.T, self.ncell, self.D = self.src.shape
        self.norms = row_norms(self.src)
        self.op, self.inv = _track_operand(self.src, precision)


def _track_operand(x, precision):
    if precision == "f32":
        _req(x.dtype == torch.float32, "track_points: precision 'f32' takes fp32 inputs")
        return x, None
    if precision == "bf16":
        _req(x.dtype == torch.bfloat16, "track_points: precision 'bf16' takes bf16 inputs")
        return x, None
    _req(x.dtype in (torch.float32, torch.float16), "track_points: precision 'f16' takes fp32 or fp16 inputs")
    if x.dtype == torch.float16:
        return x, None
    op, inv = _f16_operand(x.reshape(-1, x.shape[-1]))
    return op.view(x.shape), inv


def track_tiles(frames, max_rows=128):
    """frame-per-row [R] int -> (order [R] int64: rows grouped by frame, stable; tiles int32 [n, 4] {frame, row0, nrows, out0}
    over the ordered rows, at most max_rows rows each; out0 == row0).  Host tensors."""
    f = torch.as_tensor(frames).to("cpu", torch.int64).reshape(-1)
    order = torch.sort(f, stable=True).indices
    fs = f[order].tolist()
    tiles, i = [], 0
    while i < len(fs):
        j = i
        while j < len(fs) and fs[j] == fs[i] and j - i < max_rows:
            j += 1
        tiles.append([fs[i], i, j - i, i])
        i = j
    return order, torch.tensor(tiles, dtype=torch.int32).reshape(-1, 4)


def track_points(E, feats, frames=None, geometry=None, radius=35, precision="f16", want_cell=False, *, tiles=None):
    """The tracker head (tracking_model.py:147-200 after the relu'd cosine map of :292-308) on gd_track_points.
    E [R, D] embeddings (CUDA, fp32; bf16 for precision 'bf16'); feats [T, gh * pitch, D] or a TrackFeatures; frames [R] int: the
    target frame of every row (rows are grouped by frame into tiles of up to 128), or tiles int [n, 4] {frame, row0, nrows, out0}
    given directly; geometry = (img_h, img_w, patch, stride, gh, gw, pitch).  -> xy [R, 2] fp32 (pixels), and with want_cell the
    argmax cell [R] int64 (raster index in the gh x gw grid)."""
    tf = feats if isinstance(feats, TrackFeatures) else TrackFeatures(feats, precision)
    _req(tf.precision == precision, f"track_points: features prepared for {tf.precision!r}, asked for {precision!r}")
    _req(geometry is not None and len(geometry) == 7, "track_points: geometry = (img_h, img_w, patch, stride, gh, gw, pitch)")
    img_h, img_w, patch, stride, gh, gw, pitch = (int(v) for v in geometry)
    _req(E.is_cuda and E.dim() == 2 and E.shape[1] == tf.D, f"track_points: E must be a CUDA tensor [R, {tf.D}]")
    _req(tf.ncell == gh * pitch, f"track_points: feats hold {tf.ncell} cells per frame, the geometry {gh} x {pitch}")
    _req((frames is None) != (tiles is None), "track_points: give frames or tiles, not both")
    R = E.shape[0]
    dev = E.device
    if tiles is None:
        order, tl = track_tiles(frames)
        _req(order.numel() == R, f"track_points: {order.numel()} frames for {R} rows")
        if R == 0:
            xy = torch.empty(0, 2, dtype=torch.float32, device=dev)
            return (xy, torch.empty(0, dtype=torch.int64, device=dev)) if want_cell else xy
        ident = bool(torch.equal(order, torch.arange(R)))
        Eo = E if ident else E.index_select(0, order.to(dev))
    else:
        tl = torch.as_tensor(tiles).to("cpu", torch.int32).reshape(-1, 4)
        ident, Eo = True, E
    src = Eo.contiguous()
    e_op, e_inv = _track_operand(src, precision)
    e_norm = row_norms(src)
    src_code = dtype_code(tf.src)
    _req(dtype_code(src) == src_code, "track_points: E and feats must have the same dtype")
    n_out = R if tiles is None else int((tl[:, 3].long() + tl[:, 2].long()).max())
    xy = torch.empty(n_out, 2, dtype=torch.float32, device=dev)
    cell = torch.empty(n_out, dtype=torch.int32, device=dev) if want_cell else None
    tl = tl.contiguous()
    ws = torch.empty(max(1, lib().gd_track_points_workspace_bytes(tl.shape[0])), dtype=torch.uint8, device=dev)
    check(lib().gd_track_points(ptr(e_op), ptr(tf.op), ptr(src), ptr(tf.src), dtype_code(tf.op), src_code, src.shape[0], tf.T, gh, gw,
                                pitch, tf.D, img_h, img_w, patch, stride, int(radius), ptr(e_norm), ptr(tf.norms), ptr(e_inv), ptr(tf.inv),
                                tl.data_ptr(), tl.shape[0], n_out, ptr(xy), ptr(cell), ptr(ws), stream()), "gd_track_points")
    if not ident:
        out = torch.empty_like(xy)
        out[order.to(dev)] = xy
        xy = out
        if want_cell:
            c = torch.empty_like(cell)
            c[order.to(dev)] = cell
            cell = c
    return (xy, cell.long()) if want_cell else xy


# ------------------------------------------------------------------------------------------------ VGGT tracker tail (csrc/vggt_track.hip)
def _f32c(t, shape, what):
    _req(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape),
         f"{what} must be a contiguous CUDA fp32 tensor {tuple(shape)}, got {tuple(t.shape)} {t.dtype} on {t.device}")


def avgpool2_cl(src, W=None, pitch_out=None):
    """src: a channel-last map [F, H, pitch, 128] fp32 with W <= pitch data columns (default: all of them) -> the next pyramid level
    [F, H // 2, pitch_out, 128] (gd_avgpool2_cl: 2 x 2 mean, stride 2, odd last row / column dropped); pitch_out defaults to W // 2."""
    _req(src.dim() == 4, "avgpool2_cl: src must be [F, H, pitch, C]")
    F, H, pitch, C = src.shape
    W = pitch if W is None else int(W)
    _f32c(src, (F, H, pitch, C), "avgpool2_cl: src")
    _req(2 <= W <= pitch and H >= 2, f"avgpool2_cl: W {W} must be in [2, pitch {pitch}] and H {H} >= 2")
    po = W // 2 if pitch_out is None else int(pitch_out)
    _req(po >= W // 2, f"avgpool2_cl: pitch_out {po} < W // 2 = {W // 2}")
    out = torch.empty(F, H // 2, po, C, dtype=torch.float32, device=src.device)
    check(lib().gd_avgpool2_cl(ptr(src), ptr(out), F, H, W, pitch, po, C, stream()), "gd_avgpool2_cl")
    return out


def corr_pyramid(fmap, W, levels):
    """fmap [F, H, pitch, 128] (W <= pitch data columns) -> [(map, H, W, pitch)] of `levels` levels, each pooled from the previous (blocks.py:166-176)."""
    pyr = [(fmap, fmap.shape[1], int(W), fmap.shape[2])]
    for _ in range(levels - 1):
        m, h, w, _p = pyr[-1]
        _req(h >= 2 and w >= 2, f"corr_pyramid: level {len(pyr) - 1} is {h} x {w}: it cannot be pooled further ({levels} levels asked)")
        nxt = avgpool2_cl(m, w)
        pyr.append((nxt, h // 2, w // 2, w // 2))
    return pyr


def corr_sample(pyramid, targets, coords, radius, ld=None):
    """pyramid: [(map [F, H, pitch, 128], H, W, pitch)] per level (corr_pyramid); targets [B, N, S, 128], coords [B, N, S, 2] (level-0 cells),
    F = B * S -> [B * S, N, ld] fp32 (gd_corr_sample), ld >= levels * (2 radius + 1)^2 (default: exactly that), the columns beyond written as zeros."""
    import ctypes
    _req(targets.dim() == 4 and coords.dim() == 4, "corr_sample: targets [B, N, S, C] and coords [B, N, S, 2]")
    B, N, S, C = targets.shape
    _f32c(targets, (B, N, S, C), "corr_sample: targets")
    _f32c(coords, (B, N, S, 2), "corr_sample: coords")
    L, r = len(pyramid), int(radius)
    dims = []
    for l, (m, h, w, p) in enumerate(pyramid):
        _f32c(m, (B * S, h, p, C), f"corr_sample: level {l}")
        _req(w <= p, f"corr_sample: level {l}: W {w} > pitch {p}")
        dims += [int(h), int(w), int(p)]
    n = L * (2 * r + 1) ** 2
    ld = n if ld is None else int(ld)
    _req(ld >= n, f"corr_sample: ld {ld} < levels * (2r + 1)^2 = {n}")
    out = torch.empty(B * S, N, ld, dtype=torch.float32, device=targets.device)
    check(lib().gd_corr_sample(_ptr_array([m for m, _, _, _ in pyramid]), (ctypes.c_int * len(dims))(*dims), L, r, ptr(targets), ptr(coords), B, S, N, C,
                               ptr(out), ld, stream()), "gd_corr_sample")
    return out


def points_bilinear(fmap, W, points, frame_step=1):
    """fmap [F, H, pitch, 128] (W data columns), points [B, N, 2] (x, y) in cells -> [B, N, 128]: the bilinear sample (align_corners=True, border
    clamp) of frame b * frame_step (gd_points_bilinear)."""
    _req(fmap.dim() == 4 and points.dim() == 3, "points_bilinear: fmap [F, H, pitch, C] and points [B, N, 2]")
    F, H, pitch, C = fmap.shape
    B, N, _ = points.shape
    _f32c(fmap, (F, H, pitch, C), "points_bilinear: fmap")
    _f32c(points, (B, N, 2), "points_bilinear: points")
    _req(1 <= W <= pitch and frame_step >= 1 and (B - 1) * frame_step < F, f"points_bilinear: W {W} / pitch {pitch}, or frame {(B - 1) * frame_step} outside the {F} frames")
    out = torch.empty(B, N, C, dtype=torch.float32, device=fmap.device)
    check(lib().gd_points_bilinear(ptr(fmap), ptr(points), ptr(out), B, N, H, int(W), pitch, C, int(frame_step), stream()), "gd_points_bilinear")
    return out


def track_pos_omega(D, device):
    """omega [D / 4] fp32 of get_1d_sincos_pos_embed_from_grid(D / 2, .) (utils.py:79-81), computed in double."""
    q = D // 4
    return (1.0 / 10000 ** (torch.arange(q, dtype=torch.float64) / q)).float().to(device)


def track_pos_embed(points, H, W, D, omega=None):
    """points [M, 2] (x, y) in cells -> [M, D]: get_2d_sincos_pos_embed(D, (H, W)) sampled bilinearly with border clamp (gd_track_pos_embed)."""
    _req(points.dim() == 2 and D % 4 == 0, "track_pos_embed: points [M, 2], D a multiple of 4")
    M = points.shape[0]
    _f32c(points, (M, 2), "track_pos_embed: points")
    omega = track_pos_omega(D, points.device) if omega is None else omega
    _f32c(omega, (D // 4,), "track_pos_embed: omega")
    out = torch.empty(M, D, dtype=torch.float32, device=points.device)
    check(lib().gd_track_pos_embed(ptr(points), ptr(omega), ptr(out), M, int(H), int(W), int(D), stream()), "gd_track_pos_embed")
    return out


def track_assemble(coords, corr, feats, pos, ref_token, max_scale):
    """coords [B, N, S, 2], corr [B, S, N, C] (corr_mlp's rows), feats [B, N, S, C], pos [B * N, 3C + 4], ref_token [2, 3C + 4] ->
    the update transformer's input [B, N, S, 3C + 4] (gd_track_assemble)."""
    _req(feats.dim() == 4, "track_assemble: feats [B, N, S, C]")
    B, N, S, C = feats.shape
    D = 3 * C + 4
    for t, shape, what in ((coords, (B, N, S, 2), "coords"), (corr, (B, S, N, C), "corr"), (feats, (B, N, S, C), "feats"), (pos, (B * N, D), "pos"),
                           (ref_token, (2, D), "ref_token")):
        _f32c(t, shape, f"track_assemble: {what}")
    x = torch.empty(B, N, S, D, dtype=torch.float32, device=feats.device)
    check(lib().gd_track_assemble(ptr(coords), ptr(corr), ptr(feats), ptr(pos), ptr(ref_token), ptr(x), B, S, N, C, float(max_scale), stream()),
          "gd_track_assemble")
    return x


def track_update(delta, coords, mul1=1.0, mul2=1.0):
    """delta [B, N, S, C + 2] (last dim contiguous, equal row strides), coords [B, N, S, 2] (updated IN PLACE for s > 0) ->
    (pred [B, S, N, 2] = (coords * mul1) * mul2, dfeat [B * N * S, C] = delta[..., 2:]) (gd_track_update)."""
    _req(delta.dim() == 4 and coords.dim() == 4, "track_update: delta [B, N, S, C + 2] and coords [B, N, S, 2]")
    B, N, S, C2 = delta.shape
    C = C2 - 2
    _f32c(coords, (B, N, S, 2), "track_update: coords")
    ldd = delta.stride(2)
    if delta.is_contiguous():
        d = delta.reshape(B * N * S, C2)
    elif ldd >= C2 and all(n == 1 or s == w for n, s, w in zip(delta.shape, delta.stride(), (N * S * ldd, S * ldd, ldd, 1))):
        d = torch.as_strided(delta, (B * N * S, C2), (ldd, 1))          # the columns of wider rows (e.g. a GEMM's padded output): read in place
    else:
        d = delta.contiguous().view(B * N * S, C2)
    _req(d.is_cuda and d.dtype == torch.float32, "track_update: delta must be a CUDA fp32 tensor")
    pred = torch.empty(B, S, N, 2, dtype=torch.float32, device=d.device)
    dfeat = torch.empty(B * N * S, C, dtype=torch.float32, device=d.device)
    check(lib().gd_track_update(ptr(d), d.stride(0), ptr(coords), ptr(pred), ptr(dfeat), B, S, N, C, float(mul1), float(mul2), stream()), "gd_track_update")
    return pred, dfeat


# ------------------------------------------------------------------------------------------------ DINOv2 patch embedder ends (csrc/norm.hip)
def dino_assemble_tokens(patch, cls, reg, pos, BS, Np, out=None):
    """patch [BS * Np, D] f32 | bf16, cls [D], reg [R, D] or None, pos [1 + Np, D] (fp32) -> out fp32 [BS, 1 + R + Np, D]: cls + pos[0] | reg |
    patch + pos[1:] (gd_dino_assemble_tokens)."""
    D = patch.shape[-1]
    R = 0 if reg is None else reg.shape[0]
    _req(patch.is_cuda and patch.is_contiguous() and tuple(patch.shape) == (BS * Np, D), f"dino_assemble_tokens: patch must be a contiguous CUDA tensor {(BS * Np, D)}")
    _f32c(cls, (D,), "dino_assemble_tokens: cls")
    _f32c(pos, (1 + Np, D), "dino_assemble_tokens: pos")
    if reg is not None:
        _f32c(reg, (R, D), "dino_assemble_tokens: reg")
    if out is None:
        out = torch.empty(BS, 1 + R + Np, D, dtype=torch.float32, device=patch.device)
    else:
        _f32c(out, (BS, 1 + R + Np, D), "dino_assemble_tokens: out")
    check(lib().gd_dino_assemble_tokens(ptr(patch), dtype_code(patch), ptr(cls), ptr(reg), ptr(pos), ptr(out), BS, Np, R, D, stream()),
          "gd_dino_assemble_tokens")
    return out


def vggt_tokens_from_dino(x, gamma, beta, eps, camera, regs, B, S, gh, gw, R, tokens=None, pos=None):
    """x fp32 [B * S, 1 + R + gh * gw, D] (the embedder's residual stream after its last block), camera [2, D], regs [2, Rg, D] or None ->
    (tokens fp32 [B * S, 1 + Rg + gh * gw, D], pos int64 [B * S, 1 + Rg + gh * gw, 2]): the aggregator's block inputs (gd_vggt_tokens_from_dino)."""
    D = x.shape[-1]
    Rg = 0 if regs is None else regs.shape[1]
    P = 1 + Rg + gh * gw
    _f32c(x, (B * S, 1 + R + gh * gw, D), "vggt_tokens_from_dino: x")
    _f32c(gamma, (D,), "vggt_tokens_from_dino: gamma")
    _f32c(beta, (D,), "vggt_tokens_from_dino: beta")
    _f32c(camera, (2, D), "vggt_tokens_from_dino: camera")
    if regs is not None:
        _f32c(regs, (2, Rg, D), "vggt_tokens_from_dino: regs")
    if tokens is None:
        tokens = torch.empty(B * S, P, D, dtype=torch.float32, device=x.device)
    else:
        _f32c(tokens, (B * S, P, D), "vggt_tokens_from_dino: tokens")
    if pos is None:
        pos = torch.empty(B * S, P, 2, dtype=torch.int64, device=x.device)
    else:
        _req(pos.is_cuda and pos.dtype == torch.int64 and pos.is_contiguous() and tuple(pos.shape) == (B * S, P, 2),
             f"vggt_tokens_from_dino: pos must be a contiguous CUDA int64 tensor {(B * S, P, 2)}")
    check(lib().gd_vggt_tokens_from_dino(ptr(x), ptr(gamma), ptr(beta), float(eps), ptr(camera), ptr(regs), ptr(tokens), ptr(pos), B, S, gh, gw, R, Rg, D,
                                         stream()), "gd_vggt_tokens_from_dino")
    return tokens, pos


# ------------------------------------------------------------------------------------------------ camera head on a few rows (csrc/rows.hip)
ROWS_MAX_M, ROWS_LDS_FLOATS = 8, 16384


def _f32rows(t, what, cols=None):
    """A CUDA fp32 2-D view with a contiguous last dim (rows may be strided)."""
    _req(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and (cols is None or t.shape[1] == cols),
         f"{what} must be a CUDA fp32 view [rows, {'cols' if cols is None else cols}] with a contiguous last dim, got "
         f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__} {getattr(t, 'dtype', None)} on {getattr(t, 'device', None)}")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] + (-t.shape[1]) % 4        # the stride of a single row addresses nothing


def rows_linear(x, w, bias=None, *, out=None, residual=None, gamma=None, silu=False, gelu=False):
    """x [M, K] fp32 (M <= 8, rows may be strided), w [N, K] fp32 | bf16 (rows may be strided) -> y [M, N] fp32 =
    epilogue(prologue(x) w^T) (gd_rows_linear): prologue SiLU(x) with silu=True; epilogue + bias, exact GELU with gelu=True, then
    residual + gamma * v when residual [M, N] is given (gamma [N] or None = 1).  out= a view to write (default: a new tensor); out may be
    `residual` itself (in place), never x or w."""
    ldx = _f32rows(x, "rows_linear: x")
    M, K = x.shape
    _req(torch.is_tensor(w) and w.is_cuda and w.dtype in (torch.float32, torch.bfloat16) and w.dim() == 2 and w.shape[1] == K and w.stride(1) == 1,
         f"rows_linear: w must be a CUDA fp32 | bf16 view [N, {K}] with a contiguous last dim, got {tuple(w.shape) if torch.is_tensor(w) else type(w).__name__} "
         f"{getattr(w, 'dtype', None)} on {getattr(w, 'device', None)}")
    N = w.shape[0]
    ldw = w.stride(0) if N > 1 else K
    y = torch.empty(M, N + (-N) % 4, dtype=torch.float32, device=x.device)[:, :N] if out is None else out
    ldy = _f32rows(y, "rows_linear: out", N)
    _req(y.shape[0] == M, f"rows_linear: out has {y.shape[0]} rows, x has {M}")
    ldr = 0
    if residual is not None:
        ldr = _f32rows(residual, "rows_linear: residual", N)
        _req(residual.shape[0] == M, f"rows_linear: residual has {residual.shape[0]} rows, x has {M}")
    for t, what in ((bias, "bias"), (gamma, "gamma")):
        _req(t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (N,)), f"rows_linear: {what} must be a contiguous CUDA fp32 [{N}]")
    check(lib().gd_rows_linear(ptr(x), ptr(w), dtype_code(w), ptr(y), M, N, K, ldx, ldw, ldy, ptr(bias), ptr(residual), ldr, ptr(gamma), int(bool(silu)),
                               int(bool(gelu)), stream()), "gd_rows_linear")
    return y


def rows_attention(qkv, B, S, H, scale=None, out=None):
    """qkv [B * S, 3 * H * hd] fp32 (q | k | v, head-major; rows may be strided) -> o [B * S, H * hd] = softmax(scale q k^T) v per (b, head) over the
    S <= 8 rows of that batch entry (gd_rows_attention: exact fp32, hd a multiple of 4 up to 256; scale defaults to hd^-0.5)."""
    ld = _f32rows(qkv, "rows_attention: qkv")
    _req(qkv.shape[0] == B * S and H >= 1 and qkv.shape[1] % (3 * H) == 0, f"rows_attention: qkv {tuple(qkv.shape)} is not [{B} * {S}, 3 * {H} * hd]")
    W = qkv.shape[1] // 3
    hd = W // H
    o = torch.empty(B * S, W, dtype=torch.float32, device=qkv.device) if out is None else out
    ldo = _f32rows(o, "rows_attention: out", W)
    _req(o.shape[0] == B * S, f"rows_attention: out has {o.shape[0]} rows, not {B * S}")
    check(lib().gd_rows_attention(ptr(qkv), ptr(o), B, S, H, hd, ld, ldo, float(hd ** -0.5 if scale is None else scale), stream()), "gd_rows_attention")
    return o


def adaln_modulate(x, mod, eps=1e-6, out=None):
    """x [M, D], mod [M, 3 D] = shift | scale | gate (fp32, rows may be strided) -> gate * (LN0(x) * (1 + scale) + shift) + x, LN0 a LayerNorm
    without affine parameters (gd_adaln_modulate; D a multiple of 4 up to 8192)."""
    ldx = _f32rows(x, "adaln_modulate: x")
    M, D = x.shape
    ldm = _f32rows(mod, "adaln_modulate: mod", 3 * D)
    o = torch.empty(M, D, dtype=torch.float32, device=x.device) if out is None else out
    ldo = _f32rows(o, "adaln_modulate: out", D)
    _req(mod.shape[0] == M and o.shape[0] == M, f"adaln_modulate: x has {M} rows, mod {mod.shape[0]}, out {o.shape[0]}")
    check(lib().gd_adaln_modulate(ptr(x), ptr(mod), ptr(o), M, D, ldx, ldm, ldo, float(eps), stream()), "gd_adaln_modulate")
    return o


POSE_ACTS = {"linear": 0, "inv_log": 1, "exp": 2, "relu": 3}


def pose_update(delta, raw, first, acts=("linear", "linear", "relu"), image_hw=None, enc=None):
    """delta [M, 9] fp32 (rows may be strided), raw [M, 12] contiguous fp32, updated IN PLACE: raw[:, :9] = (first ? 0 : raw[:, :9]) + delta, columns
    9..11 stay 0 -> enc [M, 9] = the activated encoding (acts: translation, quaternion, field of view; names of POSE_ACTS); with image_hw = (H, W)
    also (extrinsic [M, 3, 4], intrinsic [M, 3, 3]) (gd_pose_update)."""
    ldd = _f32rows(delta, "pose_update: delta", 9)
    M = delta.shape[0]
    _f32c(raw, (M, 12), "pose_update: raw")
    codes = []
    for a in acts:
        _req(a in POSE_ACTS, f"pose_update: unknown activation {a!r} (known: {sorted(POSE_ACTS)})")
        codes.append(POSE_ACTS[a])
    _req(len(codes) == 3, "pose_update: acts = (translation, quaternion, field of view)")
    if enc is None:
        enc = torch.empty(M, 9, dtype=torch.float32, device=delta.device)
    else:
        _f32c(enc, (M, 9), "pose_update: enc")
    E = K = None
    H = W = 0
    if image_hw is not None:
        H, W = int(image_hw[0]), int(image_hw[1])
        E = torch.empty(M, 3, 4, dtype=torch.float32, device=delta.device)
        K = torch.empty(M, 3, 3, dtype=torch.float32, device=delta.device)
    check(lib().gd_pose_update(ptr(delta), ldd, ptr(raw), ptr(enc), ptr(E), ptr(K), M, int(bool(first)), *codes, H, W, stream()), "gd_pose_update")
    return enc if image_hw is None else (enc, E, K)


# ------------------------------------------------------------------------------------------------ small-tile fp32 linear (csrc/tokens_linear.hip)
def tokens_linear(x, w, bias=None, *, out=None, residual=None, gelu=False, accumulate=False):
    """x [M, K] fp32, w [N, K] fp32 (rows of both may be strided; K a multiple of 4) -> y [M, N] fp32 = epilogue(x w^T) on exact f32 MFMA products
    (gd_tokens_linear: 32 x 32 / 64 x 32 tiles whose four waves split K — the linear for tens to a couple of thousand token rows, where
    gemm_nt's 128 x 128 tiles leave most of the device idle).  Epilogue in gemm_nt's order: + bias [N], exact GELU with gelu=True, + residual
    [M, N], + out with accumulate=True (which needs out=).  out= a view to write (default: a new tensor whose rows are padded to a multiple of 4);
    out may be `residual` itself (in place), never x or w.  Honours set_gemm_profiler like gemm_nt; the record's epilogue tag starts with "t" ("tbra0+"), which tells the two kernels apart in by_shape()."""
    ldx = _f32rows(x, "tokens_linear: x")
    M, K = x.shape
    ldw = _f32rows(w, "tokens_linear: w", K)
    N = w.shape[0]
    _req(not accumulate or out is not None, "tokens_linear: accumulate=True adds onto out=, which is missing")
    y = torch.empty(M, N + (-N) % 4, dtype=torch.float32, device=x.device)[:, :N] if out is None else out
    ldy = _f32rows(y, "tokens_linear: out", N)
    _req(y.shape[0] == M, f"tokens_linear: out has {y.shape[0]} rows, x has {M}")
    ldr = 0
    if residual is not None:
        ldr = _f32rows(residual, "tokens_linear: residual", N)
        _req(residual.shape[0] == M, f"tokens_linear: residual has {residual.shape[0]} rows, x has {M}")
    _req(bias is None or (torch.is_tensor(bias) and bias.is_cuda and bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (N,)),
         f"tokens_linear: bias must be a contiguous CUDA fp32 [{N}]")
    if _PROFILER is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    rc = lib().gd_tokens_linear(ptr(x), ptr(w), ptr(y), M, N, K, ldx, ldw, ldy, ptr(bias), int(bool(gelu)), ptr(residual), ldr, int(bool(accumulate)), stream())
    if _PROFILER is not None:
        e1.record()
        tag = "t" + ("b" if bias is not None else "") + ("r" if residual is not None else "")
        _PROFILER.records.append((e0, e1, 2.0 * M * N * K, (M, N, K, 1, f"{tag}a{int(bool(gelu))}{'+' if accumulate else ''}", "float32", "float32")))
    check(rc, "gd_tokens_linear")
    return y
