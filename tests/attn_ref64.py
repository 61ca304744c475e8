"""fp64 restatement of the self-attention kernels (csrc/attention.hip, csrc/attn_common.h), the three input families and the per-element error
bounds tests/test_gpu_attention_paths.py holds the kernels to, plus deliberately WRONG restatements (mutants) that tests/test_attn_ref_host.py
uses to show that the bounds are not vacuous.  Plain torch, CPU, no autograd in a checked formula.  A test helper, not a test module.

Everything works per head on [B, H, N, 64] fp64 tensors (`heads` / `heads_o` take the packed layouts apart).  scale = 1/8.

What the kernels compute (every dtype, every staging variant):
  forward    s = q k^T / 8,  lse = log sum_j exp(s_ij),  o = sum_j exp(s_ij - lse_i) v_j
  backward   as a function of the GIVEN o and lse:  delta_i = sum_d dO_id o_id,  p = exp(s - lse),  dP = dO v^T,  dS = p o (dP - delta),
             dq = dS k / 8,  dk = dS^T q / 8,  dv = p^T dO          (attn_bwd_dq*: delta, dq;  attn_bwd_dkv*: dk, dv)

Notation of the bound derivations.  U = 2^-24 (fp32 unit roundoff).  Per operand type T (KINDS):
  u_q   the rounding of a COMPUTED fp32 value to an MFMA operand of the scaled q (k in the dK/dV kernels): frag_scale, attn_common.h:72-87
  u_p   the rounding of p / dS to an MFMA operand: acc_to_bfrag, attn_common.h:184-201 (f32: none, the accumulator is the operand)
  u_in  the error of an operand taken from memory: 0 for bf16 / fp16 / f32; x3 splits an fp32 value x into hi = bf16(x), lo = bf16(x - hi),
        |x - hi - lo| <= 2^-18 |x|, and drops the lo_a lo_b product, <= 2^-18 |a b| (attn_common.h:11-14: "~4e-6 relative"): charging EACH operand
        2^-17 covers the two split residuals and the dropped term (3 * 2^-18 <= 2 * 2^-17).  The same 2^-17 is x3's u_q and u_p.
  bf16: u = 2^-9, fp16: u = 2^-12 (round to nearest, 8 / 11 significand bits).
An MFMA chain that adds n products onto an accumulator c is charged ACC * n * U * (sum |products| + |c|): ACC = 2 fp32 roundings per term, because
the matrix unit's internal adder is not documented to round to nearest after every term.  v_exp_f32, v_log_f32 and v_rcp_f32 are 1-ulp instructions:
relative 2 U each.  First-order bounds carry ONE factor SECOND = 2 for every dropped higher-order term; it is not tuned.

Forward (attn_fwd_kernel, attn_fwd_dma_kernel; softmax_lagged, attn_common.h:104-143), in the exp2 domain, c2 = fl(log2(e) / 8):
  q~ = round_T(fl(q c2))                                   relative U (c2) + U (product) + u_q per element
  s'_ij = sum_d k_jd q~_id - m_i, one MFMA chain of 64 terms started from -m_i, m_i a (lagged) score of row i, |m_i| <= max_j |s2_ij|:
      e_s(i, j) = (u_q + u_in + 2 U) A_ij + ACC 65 U (A_ij + M_i),   A_ij = c2 sum_d |q_id k_jd|,  M_i = max_j |s2_ij|          (log2 units)
  p~_ij = round_T(exp2(s'_ij)): relative  eps_ij = ln 2 e_s(i, j) + 2 U + u_p
  o_id = (sum_j p~_ij v_jd) / (sum_j p~_ij): with weights w_j, d o / d w_j = (v_j - o) / sum w, so to first order
      |d o_id| <= sum_j p_ij |v_jd - o_id| eps_ij                                      (weights)
                + (u_in + ACC L U) (sum_j p_ij |v_jd| + |o_id|)                        (v operands; both accumulations, L terms)
                + 3 U |o_id|                                                           (1 / l: v_rcp 2 U; the product U)
      then ONE rounding of the stored type (half_ulp).  L = N + 3 ntile: N products, and per 64-key tile at most one rescale o, l *= exp2(-d)
      (the product U and, for lse only, alpha's own 2 U).
  lse_i = (m_i + log2 l_i) ln 2:
      |d lse_i| <= sum_j p_ij eps_ij + ACC L U                                          (l, relative = absolute in the log)
                 + ln 2 (2 U |log2 l_i| + U (M_i + |log2 l_i|))                         (v_log; the fp32 sum), |log2 l_i| <= ATT_THR + log2 N
                 + 2 U |lse_i|                                                          (ln 2 as an fp32 constant; the product)

Backward (attn_bwd_dq_kernel, attn_bwd_dq_dma_kernel, attn_bwd_dkv_kernel, attn_bwd_dkv_dma_kernel), lse2 = fl(lse log2 e) (2 U |lse2|):
  S'_ij = sum_d k q~ - lse2_i (the dK/dV kernels scale and round k instead of q: the same A_ij):
      e_s(i, j) = (u_q + u_in + 2 U) A_ij + ACC 65 U (A_ij + |lse2_i|) + 2 U |lse2_i|;      p = exp2(S'): relative eps_ij = ln 2 e_s + 2 U
  delta_i: 16 fmaf per lane + 2 shuffle adds on operands as loaded:   e_delta_i = (18 U + 2 u_in) sum_d |dO_id o_id|
  dP'_ij = sum_d v_jd dO_id - delta_i, one chain of 64 terms started from -delta_i:
      e_dp(i, j) = 2 u_in B_ij + ACC 65 U (B_ij + |delta_i|) + e_delta_i,   B_ij = sum_d |dO_id v_jd|
  dS_ij = round_T(fl(p dP')):   e_dS(i, j) = |dS_ij| (eps_ij + U + u_p) + p_ij e_dp(i, j)
  dq_id = fl(sum_j dS_ij k_jd / 8):   |d dq| <= ( sum_j e_dS |k_jd| + (u_in + ACC N U + U) sum_j |dS_ij k_jd| ) / 8, then the store's rounding
  dk_jd likewise over i with q;   dv_jd = sum_i round_T(p_ij) dO_id:   |d dv| <= sum_i p_ij (eps_ij + u_p) |dO_id| + (u_in + ACC N U) sum_i p_ij |dO_id|

Uniform-count probe (q = 0; k, v, dout small integers): every score is exactly 0, m = 0, p = 1 in every operand type, l = N exactly
(N < 2^24), so  lse = fl(fl(log2 N) ln 2): |d lse| <= 4 U ln N  (v_log 2 U, the constant U, the product U; N = 1: exactly 0), and
o = fl((sum_j v_j) fl(1 / N)) with an exact integer sum: |d o| <= 3 U |o| + one rounding of the stored type.  dk = dS^T q / 8 is exactly 0."""
import math

import torch

U = 2.0 ** -24
SECOND = 2.0          # the one factor for higher-order terms
ACC = 2.0             # fp32 roundings charged per term of an MFMA accumulation
ATT_THR = 8.0         # attn_common.h:66
TOPK = 4              # keys per row whose v_j - o enters the forward bound exactly (a cost setting: any value gives a valid bound)
LOG2E = 1.4426950408889634
SCALE = 0.125
PREC = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}
EMIN = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}

# name -> (tensor dtype, x3 flag, u_q, u_p, u_in)
KINDS = {"f32": (torch.float32, False, 0.0, 0.0, 0.0),
         "bf16": (torch.bfloat16, False, 2.0 ** -9, 2.0 ** -9, 0.0),
         "f16": (torch.float16, False, 2.0 ** -12, 2.0 ** -12, 0.0),
         "x3": (torch.float32, True, 2.0 ** -17, 2.0 ** -17, 2.0 ** -17)}


def half_ulp(v, dtype):
    """The error of ONE round-to-nearest of v to `dtype` (half the spacing at |v|; half the subnormal spacing below the normal range)."""
    _, e = torch.frexp(v.abs().double())
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype]), torch.clamp(e - 1, min=EMIN[dtype]))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - PREC[dtype])


def _store(bound, value, kind):
    dt = KINDS[kind][0]
    return bound if dt == torch.float32 else bound + half_ulp(value.abs() + bound, dt)


# ------------------------------------------------------------------------------------------------ layouts
def heads(qkv, B, N, H):
    """packed [B*N, 3*H*64] -> q, k, v [B, H, N, 64] fp64"""
    x = qkv.double().cpu().reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    return x[0].contiguous(), x[1].contiguous(), x[2].contiguous()


def heads_o(o, B, N, H):
    """[B*N, H*64] -> [B, H, N, 64] fp64"""
    return o.double().cpu().reshape(B, N, H, 64).permute(0, 2, 1, 3).contiguous()


def pack_qkv(q, k, v):
    B, H, N, _ = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * 64).contiguous()


def pack_o(o):
    B, H, N, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(B * N, H * 64).contiguous()


# ------------------------------------------------------------------------------------------------ inputs
FAMILIES = ("random", "uniform", "pair")
PAIR_STEP = 67
PAIR_R = 16.0         # r^2 / 8 = 32


def make_inputs(family, B, N, H, kind, seed=None):
    """-> (qkv [B*N, 3*H*64], dout [B*N, H*64]) on the CPU, rounded to the kind's tensor dtype."""
    g = torch.Generator().manual_seed(N if seed is None else seed)
    dt = KINDS[kind][0]
    if family == "random":
        qkv = torch.randn(B * N, 3 * H * 64, generator=g)
        dout = torch.randn(B * N, H * 64, generator=g)
        return qkv.to(dt), dout.to(dt)
    if family == "uniform":
        q = torch.zeros(B, H, N, 64)
        k = torch.randint(-3, 4, (B, H, N, 64), generator=g).float()
        v = torch.randint(-3, 4, (B, H, N, 64), generator=g).float()
        d = torch.zeros(B, H, N, 64)
        i = torch.arange(N)
        sign = (torch.randint(0, 2, (B, H, N), generator=g) * 2 - 1).float()
        d[:, :, i, i % 64] = sign
        return pack_qkv(q, k, v).to(dt), pack_o(d).to(dt)
    assert family == "pair"
    u = torch.randn(B, H, N, 64, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    k = PAIR_R * u
    # row i: u_i + u_{(i + 67) mod N}; where the partner is the row itself (N = 1, 67) the query selects its one key with the same score r^2 / 8
    q = PAIR_R * (u + u.roll(-(PAIR_STEP % N), dims=2)) if PAIR_STEP % N else PAIR_R * u
    v = torch.randn(B, H, N, 64, generator=g, dtype=torch.float64)
    d = torch.randn(B, H, N, 64, generator=g, dtype=torch.float64)
    return pack_qkv(q, k, v).float().to(dt), pack_o(d).float().to(dt)


# ------------------------------------------------------------------------------------------------ the restatement, with mutation hooks
class Mutant:
    """key_w [N]: multiplicity of every key (0 dropped, 2 counted twice) in every sum over keys and as the owner of its dk / dv row;
    row_w [N]: multiplicity of every query in the dK / dV sums only; head_roll: k / v come from head (h + 1) mod H; lse_next: row i uses the lse of
    row (i + 1) mod N in the backward."""

    def __init__(self, name, key_w=None, row_w=None, head_roll=False, lse_next=False):
        self.name, self.key_w, self.row_w, self.head_roll, self.lse_next = name, key_w, row_w, head_roll, lse_next


def mutants(N, H):
    """-> [(name, Mutant or None)]; None where the mutant IS the reference at this size (no pad rows when N % 64 == 0; one row has no next row;
    one head has no neighbour) — the host test asserts that these are the only gaps."""
    ones = torch.ones(N, dtype=torch.float64)

    def kw(j, w):
        t = ones.clone()
        t[j] = w
        return t
    tail0 = N - N % 64 if N % 64 else N - 64              # the first key of the tail tile (of the last tile when there is no tail)
    tail0 = max(tail0, 0)
    ntile = (N + 63) // 64
    t = (ntile - 1) // 2
    tile = ones.clone()
    tile[t * 64:min(N, t * 64 + 64)] = 0.0
    pad = (N + 63) // 64 * 64 - N
    return [("drop_last_key", Mutant("drop_last_key", key_w=kw(N - 1, 0.0))),
            ("drop_tail_first_key", Mutant("drop_tail_first_key", key_w=kw(tail0, 0.0))),
            ("key_twice", Mutant("key_twice", key_w=kw(N // 2, 2.0))),
            ("skip_tile", Mutant("skip_tile", key_w=tile)),
            ("skip_query_dkv", Mutant("skip_query_dkv", row_w=kw((2 * N) // 3, 0.0))),
            ("pad_query_live", Mutant("pad_query_live", row_w=kw(N - 1, 1.0 + pad)) if pad else None),
            ("neighbour_head_kv", Mutant("neighbour_head_kv", head_roll=True) if H > 1 else None),
            ("lse_of_next_row", Mutant("lse_of_next_row", lse_next=True) if N > 1 else None)]


def fwd64(q, k, v, mut=None):
    """-> o [B, H, N, 64], lse [B, H, N]"""
    if mut is not None and mut.head_roll:
        k, v = k.roll(-1, dims=1), v.roll(-1, dims=1)
    s = (q @ k.transpose(-1, -2)) * SCALE
    if mut is not None and mut.key_w is not None:
        s = s + torch.log(mut.key_w)                       # log 0 = -inf: the key is gone
    lse = torch.logsumexp(s, -1)
    o = torch.exp(s - lse[..., None]) @ v
    return o, lse


def bwd64(q, k, v, o, lse, dout, mut=None):
    """dq, dk, dv [B, H, N, 64] as functions of the GIVEN o and lse."""
    if mut is not None and mut.head_roll:
        k, v = k.roll(-1, dims=1), v.roll(-1, dims=1)
    if mut is not None and mut.lse_next:
        lse = lse.roll(-1, dims=-1)
    delta = (dout * o).sum(-1)
    p = torch.exp((q @ k.transpose(-1, -2)) * SCALE - lse[..., None])
    if mut is not None and mut.key_w is not None:
        p = p * mut.key_w
    ds = p * (dout @ v.transpose(-1, -2) - delta[..., None])
    dq = (ds @ k) * SCALE
    if mut is not None and mut.row_w is not None:
        p, ds = p * mut.row_w[:, None], ds * mut.row_w[:, None]
    dk = (ds.transpose(-1, -2) @ q) * SCALE
    dv = p.transpose(-1, -2) @ dout
    return dq, dk, dv


def fwd_autograd64(q, k, v, dout):
    """Plain softmax attention and its autograd gradients: what the restatement is checked against."""
    q, k, v = [t.clone().requires_grad_(True) for t in (q, k, v)]
    s = (q @ k.transpose(-1, -2)) * SCALE
    o = torch.softmax(s, -1) @ v
    o.backward(dout)
    return o.detach(), torch.logsumexp(s.detach(), -1), q.grad, k.grad, v.grad


# ------------------------------------------------------------------------------------------------ bounds
def fwd_bound(q, k, v, kind):
    """-> (o, lse, bound_o, bound_lse): the fp64 forward and the per-element bounds on |kernel - fp64| (o after its store)."""
    _, _, u_q, u_p, u_in = KINDS[kind]
    N = q.shape[-2]
    c2 = SCALE * LOG2E
    s2 = (q @ k.transpose(-1, -2)) * c2
    A = (q.abs() @ k.abs().transpose(-1, -2)) * c2
    M = s2.abs().amax(-1)
    lse2 = torch.logsumexp(s2 * math.log(2.0), -1) / math.log(2.0)
    p = torch.exp2(s2 - lse2[..., None])
    o = p @ v
    lse = lse2 * math.log(2.0)
    eps = math.log(2.0) * ((u_q + u_in + 2 * U) * A + ACC * 65 * U * (A + M[..., None])) + 2 * U + u_p
    L = N + 3 * ((N + 63) // 64)
    pe = p * eps
    # sum_j p eps |v_jd - o_id|: exactly for the TOPK heaviest keys of every row (the cancellation v_j - o is what makes the pair probe sharp),
    # and |v_jd - o_id| <= |v_jd| + |o_id| for the rest (a valid, slightly larger bound at 1 / 64 of the cost)
    K = min(TOPK, N)
    top, idx = pe.topk(K, -1)
    vsel = torch.stack([torch.gather(v, -2, idx[..., kk][..., None].expand(*idx.shape[:-1], 64)) for kk in range(K)], -2)      # [B, H, N, K, 64]
    bo = (top[..., None] * (vsel - o[..., None, :]).abs()).sum(-2)
    rest = pe.scatter(-1, idx, 0.0)
    bo = bo + rest @ v.abs() + rest.sum(-1, keepdim=True) * o.abs()
    bo = bo + (u_in + ACC * L * U) * (p @ v.abs() + o.abs()) + 3 * U * o.abs()
    bo = _store(SECOND * bo, o, kind)
    logl = ATT_THR + math.log2(N)
    bl = SECOND * (pe.sum(-1) + ACC * L * U) + math.log(2.0) * (2 * U * logl + U * (M + logl)) + 2 * U * lse.abs()
    return o, lse, bo, bl


def bwd_bound(q, k, v, o, lse, dout, kind):
    """-> (dq, dk, dv, bound_dq, bound_dk, bound_dv) for the GIVEN o and lse."""
    _, _, u_q, u_p, u_in = KINDS[kind]
    N = q.shape[-2]
    c2 = SCALE * LOG2E
    kt, vt = k.transpose(-1, -2), v.transpose(-1, -2)
    lse2 = (lse * LOG2E)[..., None]
    s2 = (q @ kt) * c2
    A = (q.abs() @ kt.abs()) * c2
    p = torch.exp2(s2 - lse2)
    eps = math.log(2.0) * ((u_q + u_in + 2 * U) * A + ACC * 65 * U * (A + lse2.abs()) + 2 * U * lse2.abs()) + 2 * U
    del A, s2
    delta = (dout * o).sum(-1)[..., None]
    e_delta = (18 * U + 2 * u_in) * (dout * o).abs().sum(-1)[..., None]
    Bm = dout.abs() @ vt.abs()
    e_dp = 2 * u_in * Bm + ACC * 65 * U * (Bm + delta.abs()) + e_delta
    del Bm
    ds = p * (dout @ vt - delta)
    e_ds = ds.abs() * (eps + U + u_p) + p * e_dp
    del e_dp
    acc = u_in + ACC * N * U
    dq, dk, dv = (ds @ k) * SCALE, (ds.transpose(-1, -2) @ q) * SCALE, p.transpose(-1, -2) @ dout
    bdq = (e_ds @ k.abs() + (acc + U) * (ds.abs() @ k.abs())) * SCALE
    bdk = (e_ds.transpose(-1, -2) @ q.abs() + (acc + U) * (ds.abs().transpose(-1, -2) @ q.abs())) * SCALE
    bdv = (p * (eps + u_p)).transpose(-1, -2) @ dout.abs() + acc * (p.transpose(-1, -2) @ dout.abs())
    return dq, dk, dv, _store(SECOND * bdq, dq, kind), _store(SECOND * bdk, dk, kind), _store(SECOND * bdv, dv, kind)


def uniform_fwd(v, kind):
    """The uniform-count probe's closed forms -> (o, lse, bound_o, bound_lse)."""
    N = v.shape[-2]
    o = v.sum(-2, keepdim=True).expand_as(v) / N
    lse = torch.full(v.shape[:-1], math.log(N), dtype=torch.float64)
    return o, lse, _store(3 * U * o.abs(), o, kind), 4 * U * lse.abs()


def ratio(got, ref, bound):
    """-> (worst err / bound, flat index); a NaN or an infinity anywhere is an infinite ratio; bound 0 demands equality."""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(t) for t in torch.unravel_index(torch.tensor(i), r.shape))
