"""fp64 restatement of the four kernels of csrc/rows.hip (gd_rows_linear, gd_rows_attention, gd_adaln_modulate, gd_pose_update) with per-element
bounds on |kernel - fp64| derived from the kernels' operation order, the case tables the host and GPU tests share, and the mutants the host test
shows to break those bounds.  u = 2^-24 is fp32's unit round-off; gamma_n = n u / (1 - n u) bounds a sum of n terms IN ANY ORDER, so no bound here
depends on how a kernel splits a reduction over lanes.

Every function takes `mutant=`: None for the kernel's arithmetic, or the name of one deliberate mistake (MUTANTS)."""
import math

import torch

from rowwise_ref64 import SECOND, U, ln_fwd_bound, ln_stats64

MUTANTS = ("last_k_chunk_dropped", "neighbour_bias", "gamma_on_residual", "silu_omitted", "attention_across_entries", "dropped_key", "gate_scale_swapped",
           "activated_fed_back", "scalar_first_quaternion")
ACT_NAMES = ("linear", "inv_log", "exp", "relu")


def gamma_n(n):
    return n * U / (1.0 - n * U)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------------------ linear
# M, K, N, weight type, what surrounds the product, and the padding of the three row strides (elements beyond K, K, N)
def _lc(M, K, N, wt="f32", bias=True, silu=False, gelu=False, residual=False, gamma=False, pads=(0, 0, 0)):
    return dict(M=M, K=K, N=N, wt=wt, bias=bias, silu=silu, gelu=gelu, residual=residual, gamma=gamma, pads=pads)


# fp32 weights: a lane takes 4 k per step of 256, 4 steps are unrolled -> K = 4 / 12 (a few lanes of the tail step), 252 / 256 / 260 (around one
# step), 1284 (one unrolled group + one single step + a tail), 2048 (two groups), 8192 (M = 2: the LDS budget's other corner).  bf16: 8 k per lane,
# steps of 512 -> 8, 256 (tail only), 520 (one step + one lane), 2048 (one group), 8192.  N against the 8 columns of a workgroup and the 2 of a
# wave: 1, 9, 31, 32, 33, 2048.
LINEAR_CASES = [
    _lc(1, 4, 1),
    _lc(2, 12, 33, pads=(4, 0, 3)),                                           # embed_pose
    _lc(3, 252, 31, silu=True, pads=(4, 8, 5)),                                # the modulation's form
    _lc(8, 256, 32, gelu=True),                                                # fc1
    _lc(2, 260, 9, pads=(0, 4, 3)),                                            # pose_branch.fc2: 9 columns in rows of 12
    _lc(8, 2048, 33, residual=True, gamma=True),                               # proj / fc2 on the token stream
    _lc(2, 2048, 2048, residual=True, gamma=True),
    _lc(2, 8192, 31, residual=True),                                           # a block without LayerScale
    _lc(3, 2048, 32, silu=True),
    _lc(1, 1284, 9, gelu=True, pads=(0, 0, 3)),
    _lc(2, 256, 33, "bf16", pads=(0, 0, 3)),
    _lc(8, 2048, 31, "bf16", silu=True, pads=(0, 0, 1)),
    _lc(2, 8192, 32, "bf16", residual=True, gamma=True),
    _lc(3, 520, 1, "bf16", gelu=True, pads=(4, 8, 3)),
    _lc(1, 8, 9, "bf16", pads=(0, 0, 3)),
    _lc(2, 2048, 2048, "bf16", gelu=True),
]


def linear_inputs(c, seed=0):
    """x [M, K], w [N, K] (fp32 or bf16), bias / residual / gamma or None, on the host.  Families: x and w standard normal, except the last
    min(8, K) columns, which are positive and about 4 in both (the last chunk of K weighs in with products that do not cancel); bias and residual
    64 x normal and gamma 0.5 x normal, so that a wrong column's bias or a misplaced gamma moves the result by far more than the accumulation bound."""
    g = gen(1000 + 7 * c["M"] + 13 * c["K"] + 17 * c["N"] + seed)
    M, K, N = c["M"], c["K"], c["N"]
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    t = min(8, K)
    x[:, K - t:] = 4.0 + 0.5 * torch.randn(M, t, generator=g).abs()
    w[:, K - t:] = 4.0 + torch.randn(N, t, generator=g).abs()
    if c["wt"] == "bf16":
        w = w.bfloat16()
    return dict(x=x, w=w, bias=64 * torch.randn(N, generator=g) if c["bias"] else None, residual=64 * torch.randn(M, N, generator=g) if c["residual"] else None,
                gamma=0.5 * torch.randn(N, generator=g) if c["gamma"] else None)


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _gelu(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def linear64(x, w, bias=None, residual=None, gamma=None, silu=False, gelu=False, mutant=None, dtype=torch.float64):
    """-> (y, bound) [M, N].  dtype=torch.float32 evaluates the same expression in fp32 (the host test's check that fp32 stays inside the bound).

    The bound, term by term (absacc = sum_k |x_k w_k| with the prologue applied):
      accumulation  gamma_K absacc: K fused multiply-adds and the wave's tree, in whatever order;
      prologue      SiLU(x) = x / (1 + expf(-x)): expf 1 ulp = 2 u, the addition u, the division u -> 5 u relative on every term -> 5 u absacc;
      bias          one addition: u |v|;
      GELU          v <- 0.5 v (1 + erff(v / sqrt 2)): the argument's rounding moves erf by <= 0.5 u (z erf'(z) <= 0.48), erff 2 ulp = 4 u |erf| <= 4 u,
                    the addition 2 u: (1 + erf) carries 6.5 u ABSOLUTE — for negative v it is small and the error is not relative to the result —
                    so 0.5 |v| 6.5 u <= 4 u |v|, + 3 u |g| for the two products; what v already carried passes through |GELU'| <= 1.13;
      residual      y = fmaf(gamma, v, r) or r + v: one rounding, u |y|; what v carried is scaled by |gamma|."""
    xd, wd = x.to(dtype), w.to(dtype)
    K = xd.shape[1]
    if silu and mutant != "silu_omitted":
        xd = _silu(xd)
    if mutant == "last_k_chunk_dropped":
        ch = 8 if w.dtype == torch.bfloat16 else 4
        xd = xd.clone()
        xd[:, K - ch:] = 0
    v = xd @ wd.T
    absacc = xd.abs().double() @ wd.abs().double().T
    e = (gamma_n(K) + (5 * U if silu else 0.0)) * absacc
    if bias is not None:
        b = bias.to(dtype)
        if mutant == "neighbour_bias":
            N = b.numel()
            b = torch.cat([b[1:], b[N - 2:N - 1]]) if N > 1 else torch.zeros_like(b)
        v = v + b
        e = e + U * v.abs().double()
    if gelu:
        gv = _gelu(v)
        e = 1.13 * e + 4 * U * v.abs().double() + 3 * U * gv.abs().double()
        v = gv
    if residual is not None:
        r = residual.to(dtype)
        gm = gamma.to(dtype) if gamma is not None else torch.ones(v.shape[1], dtype=dtype)
        v = (gm * r + v) if mutant == "gamma_on_residual" else (r + gm * v)
        e = gm.abs().double() * e + U * v.abs().double()
    return v, e * SECOND + 1e-300


# ------------------------------------------------------------------------------------------------------------------------------------ attention
ATTENTION_CASES = [(1, 2, 16, 128), (2, 3, 4, 16), (1, 1, 2, 4), (1, 8, 2, 256), (3, 2, 2, 12)]         # (B, S, H, hd)


def attention_inputs(B, S, H, hd, pad=0, huge_entry=None, seed=0):
    """qkv [B * S, 3 H hd + pad]; huge_entry: the keys of that batch entry are 64 x as large (a query that crossed into it would see only them)."""
    W = H * hd
    qkv = torch.randn(B * S, 3 * W + pad, generator=gen(2000 + 11 * B + 13 * S + 17 * H + hd + seed))
    if huge_entry is not None:
        qkv[huge_entry * S:(huge_entry + 1) * S, W:2 * W] *= 64.0
    return qkv


def attention64(qkv, B, S, H, hd, scale=None, mutant=None, dtype=torch.float64):
    """-> (o, bound) [B * S, H hd].  s_j = scale sum_d q_d k_jd carries e_s = (gamma_hd + 2 u) scale sum |q k|; p_j = expf(s_j - max) then has the
    relative error 2 E + 3 u with E = max_j e_s (both s_j and the maximum moved; expf 1 ulp, the subtraction); l = sum p adds gamma_S, o = sum p v / l
    the products, gamma_S and the division: |do| <= (4 E + (2 S + 10) u) sum_j p_j |v_j| / l."""
    W = H * hd
    scale = hd ** -0.5 if scale is None else scale
    x = qkv[:, :3 * W].to(dtype)
    G, L = (1, B * S) if mutant == "attention_across_entries" else (B, S)
    q, k, v = (x[:, i * W:(i + 1) * W].reshape(G, L, H, hd).permute(0, 2, 1, 3) for i in range(3))
    if mutant == "dropped_key" and L > 1:
        k, v = k[:, :, :L - 1], v[:, :, :L - 1]
    s = scale * (q @ k.transpose(-2, -1))
    e_s = (gamma_n(hd) + 2 * U) * scale * (q.abs().double() @ k.abs().double().transpose(-2, -1))
    p = torch.softmax(s, dim=-1)
    o = p @ v
    E = e_s.amax(-1, keepdim=True)
    bound = (4 * E + (2 * L + 10) * U) * (p.double() @ v.abs().double())
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * S, W)
    return back(o), back(bound) * SECOND + 1e-300


# ------------------------------------------------------------------------------------------------------------------------------------ adaLN
ADALN_CASES = [(2, 4), (3, 64), (8, 260), (2, 2048)]             # (M, D)


def adaln_inputs(M, D, seed=0):
    g = gen(3000 + 7 * M + D + seed)
    x = torch.randn(M, D, generator=g) * 2.0 + 0.5
    mod = torch.randn(M, 3 * D, generator=g)
    mod[:, 2 * D:] *= 3.0                                         # gate and scale on different scales: swapping them shows
    return x, mod


def adaln64(x, mod, eps=1e-6, mutant=None, dtype=torch.float64):
    """-> (out, bound).  n = LN0(x) (1 + scale) + shift is gd_layernorm_fwd's row body with gamma = 1 + scale (one more rounding, u |t|) and
    beta = shift: rowwise_ref64.ln_fwd_bound; out = gate n + x then adds |gate| times that, u |gate n| for the product and u |out| for the sum."""
    D = x.shape[1]
    xd, md = x.to(dtype), mod.to(dtype)
    shift, scale, gate = md[:, :D], md[:, D:2 * D], md[:, 2 * D:]
    if mutant == "gate_scale_swapped":
        scale, gate = gate, scale
    mean = xd.mean(-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(-1, keepdim=True)
    t = (xd - mean) * (var + eps) ** -0.5 * (1 + scale)
    n = t + shift
    out = gate * n + xd
    by, _, _ = ln_fwd_bound(x, (1 + scale).double(), shift.double(), eps, torch.float32)
    bound = gate.abs().double() * (by + U * t.abs().double()) + U * (gate * n).abs().double() + U * out.abs().double()
    return out, bound * SECOND + 1e-300


# ------------------------------------------------------------------------------------------------------------------------------------ pose
FOV_RANGE = (0.2, 2.5)            # fx, fy are held to FOCAL_REL inside it; outside, only the exact-zero case is tested
# tan(y) at y = fov / 2 <= 1.25 has the condition number 2 y / sin(2 y) <= 4.2, times the field of view's own rounding (u; 3 u behind expf), + tanf's
# documented 1 ulp = 2 u (HIP's math API table), + the division and the halving: about 4.2 * 3 u + 2 u + u < 16 u.  The issue sets 32 u.
FOCAL_REL = 32 * U
# (first, (trans_act, quat_act, fl_act)): the head's own activations on a first and a later iteration, then the other codes
POSE_CASES = [(True, ("linear", "linear", "relu")), (False, ("linear", "linear", "relu")), (False, ("inv_log", "exp", "exp")), (False, ("exp", "inv_log", "linear"))]
POSE_HW = (42, 70)


def pose_inputs(first, acts, M=5, seed=0):
    """(delta [M, 9], raw_prev [M, 12]).  The raw fields of view are placed so that the activated ones lie inside FOV_RANGE, except — relu only — row 0,
    whose new raw fov_h is negative (an exact 0, fy = +inf); with relu the previous raw values are negative in rows 1.., so that feeding the
    ACTIVATED encoding back instead of the raw sum shows."""
    g = gen(4000 + 10 * int(first) + sum(ACT_NAMES.index(a) * 4 ** i for i, a in enumerate(acts)) + seed)
    delta, raw = torch.randn(M, 9, generator=g) * 0.5, torch.zeros(M, 12)
    raw[:, :9] = torch.randn(M, 9, generator=g) * 0.5
    fl = acts[2]
    lo, hi = (math.log(FOV_RANGE[0]), math.log(FOV_RANGE[1])) if fl == "exp" else (math.log1p(FOV_RANGE[0]), math.log1p(FOV_RANGE[1])) if fl == "inv_log" else FOV_RANGE
    target = lo + (hi - lo) * torch.rand(M, 2, generator=g)                          # the new raw field of view
    if first:
        delta[:, 7:] = target
    else:
        raw[:, 7:9] = -0.3 - torch.rand(M, 2, generator=g) if fl == "relu" else torch.randn(M, 2, generator=g) * 0.5
        delta[:, 7:] = target - raw[:, 7:9]
    if fl == "relu":
        delta[0, 7] -= target[0, 0] + 0.25                                            # row 0: the new raw fov_h = -0.25
    return delta, raw


def _act(t, name):
    return {"linear": lambda v: v, "inv_log": lambda v: torch.sign(v) * torch.expm1(v.abs()), "exp": torch.exp, "relu": lambda v: v.clamp_min(0)}[name](t)


def pose64(delta, raw_prev, first, acts, image_hw=None, mutant=None, dtype=torch.float64):
    """-> dict(raw [M, 12], enc [M, 9], extrinsic [M, 3, 4], intrinsic [M, 3, 3]) and the bounds b_raw, b_enc, b_extrinsic (absolute).
    raw: one addition, u |raw| (none on the first iteration).  enc: linear / relu pass that on; exp multiplies it by enc and adds expf's 2 u + u;
    inv_log the same with expm1f.  A rotation entry is delta - two_s (a b +- c d) with two_s = 2 / sum q^2: with q good to rel_q, two_s carries
    2 rel_q + 5 u and the bracket 2 rel_q + 3 u of |a b| + |c d|, + 2 u for the last product and subtraction: (4 rel_q + 12 u) two_s (|a b| + |c d|) + 2 u."""
    d, rp = delta.to(dtype), raw_prev.to(dtype)
    groups = [(0, 3, acts[0]), (3, 7, acts[1]), (7, 9, acts[2])]
    if first:
        new = d.clone()
    elif mutant == "activated_fed_back":
        new = torch.cat([_act(rp[:, a:b], n) for a, b, n in groups], dim=1) + d
    else:
        new = rp[:, :9] + d
    raw = torch.zeros(d.shape[0], 12, dtype=dtype)
    raw[:, :9] = new
    enc = torch.cat([_act(new[:, a:b], n) for a, b, n in groups], dim=1)
    b_raw = (0.0 if first else U) * new.abs().double()
    b_enc = torch.cat([b_raw[:, a:b] if n in ("linear", "relu") else
                       (b_raw[:, a:b] * (enc[:, a:b].abs().double() + (1.0 if n == "inv_log" else 0.0)) + 3 * U * enc[:, a:b].abs().double()) for a, b, n in groups], dim=1)
    out = dict(raw=raw, enc=enc, b_raw=b_raw * SECOND + 1e-300, b_enc=b_enc * SECOND + 1e-300)
    if image_hw is None:
        return out
    H, W = image_hw
    q = enc[:, 3:7]
    i, j, k, r = (q[:, [1, 2, 3, 0]] if mutant == "scalar_first_quaternion" else q).unbind(-1)
    s2 = 2.0 / (q * q).sum(-1)
    pairs = [(j, j, k, k, -1), (i, j, k, r, -1), (i, k, j, r, 1), (i, j, k, r, 1), (i, i, k, k, -1), (j, k, i, r, -1), (i, k, j, r, -1), (j, k, i, r, 1), (i, i, j, j, -1)]
    diag = (0, 4, 8)
    ent, mag = [], []
    for n, (a, b, c, e, sg) in enumerate(pairs):
        if n in diag:
            ent.append(1 - s2 * (a * b + c * e))
        else:
            ent.append(s2 * (a * b + sg * c * e))
        mag.append(s2.double() * ((a * b).abs().double() + (c * e).abs().double()))
    R = torch.stack(ent, dim=-1).reshape(-1, 3, 3)
    rel_q = (out["b_enc"][:, 3:7] / q.abs().double().clamp_min(1e-300)).amax(-1)
    b_R = ((4 * rel_q + 12 * U)[:, None] * torch.stack(mag, dim=-1) + 2 * U).reshape(-1, 3, 3)
    out["extrinsic"] = torch.cat([R, enc[:, :3, None]], dim=-1)
    out["b_extrinsic"] = torch.cat([b_R, out["b_enc"][:, :3, None]], dim=-1) * SECOND
    K = torch.zeros(d.shape[0], 3, 3, dtype=dtype)
    K[:, 0, 0] = (W / 2.0) / torch.tan(enc[:, 8] / 2.0)
    K[:, 1, 1] = (H / 2.0) / torch.tan(enc[:, 7] / 2.0)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = W / 2, H / 2, 1.0
    out["intrinsic"] = K
    return out


def pose_ratio(got, want):
    """The worst err / bound over raw, enc, the extrinsics and fx / fy (FOCAL_REL relative where the field of view lies inside FOV_RANGE; a field of
    view of exactly 0 must give +inf in both; other fields of view are not judged); the constant intrinsic entries must be equal."""
    worst = 0.0
    for k in ("raw", "enc", "extrinsic"):
        if k in want:
            b = want["b_" + k] if k != "raw" else torch.cat([want["b_raw"], torch.full_like(want["b_raw"][:, :3], 1e-300)], dim=1)
            worst = max(worst, float(((got[k].double() - want[k].double()).abs() / b).max()))
    if "intrinsic" in want:
        Kg, Kw, fov = got["intrinsic"].double(), want["intrinsic"].double(), want["enc"][:, 7:9].double()
        for col, (a, b) in ((0, (1, 1)), (1, (0, 0))):                            # fov_h -> fy = K[1, 1], fov_w -> fx = K[0, 0]
            f, g, w = fov[:, col], Kg[:, a, b], Kw[:, a, b]
            inside = (f >= FOV_RANGE[0]) & (f <= FOV_RANGE[1])
            if bool(inside.any()):
                worst = max(worst, float((((g - w).abs() / w.abs())[inside] / FOCAL_REL).max()))
            zero = f == 0
            if bool(zero.any()) and not bool((torch.isposinf(g[zero]) & torch.isposinf(w[zero])).all()):
                worst = float("inf")
        const = torch.ones(3, 3, dtype=torch.bool)
        const[0, 0] = const[1, 1] = False
        if not torch.equal(Kg[:, const], Kw[:, const]):
            worst = float("inf")
    return worst
